"""Routing of ``use_bias_in_linear`` / ``readout_as_fcn`` models (no GPU):
nn.sevennet0_kinds -- the predicate model.load_model and model_build's family
label share with e3gnn_load -- keeps a SevenNet-0 manifest with either option on
the SevenNet-0 kernels (the biases ride in the node-linear epilogues, the FCN
readout has its own kernel, csrc/node.hip), within the readout kernel's limits
(1-4 hidden layers of 1-128 units)."""
import pytest

from sevennet_finetuning_amd import model_build as mb
from sevennet_finetuning_amd.nn import sevennet0_kinds

SN0_IRREPS = ['128x0e'] + ['128x0e+64x1e+32x2e'] * 4 + ['128x0e']
BIAS = {'use_bias_in_linear': True}
FCN = {'readout_as_fcn': True}


def _sevennet0_manifest(**opts):
    cfg = mb.sevennet_shaped_config(128, 5)
    cfg['irreps_manual'] = SN0_IRREPS
    cfg.update(opts)
    return mb.model_manifest(mb.resolve_config(cfg))


@pytest.mark.parametrize('opts', [BIAS, FCN, dict(BIAS, **FCN)], ids=['bias', 'fcn', 'both'])
def test_sevennet0_with_options_keeps_the_sevennet0_kernels(opts):
    man = _sevennet0_manifest(**opts)
    assert man['use_bias_in_linear'] == bool(opts.get('use_bias_in_linear'))
    assert man['readout']['type'] == ('fcn' if opts.get('readout_as_fcn') else 'linear')
    assert sevennet0_kinds(man) == [0, 1, 1, 1, 2]
    assert man['family'] == 'sevennet0'


@pytest.mark.parametrize('hidden', [[160], [8, 8, 8, 8, 8], []])
def test_fcn_beyond_the_readout_kernel_limits_is_not_sevennet0(hidden):
    """What e3gnn_load sends to the generic engine (fused_family, csrc/model_load.cpp)."""
    man = _sevennet0_manifest(readout_as_fcn=True)
    man['readout'] = dict(man['readout'], hidden=hidden)
    assert sevennet0_kinds(man) is None
    assert sevennet0_kinds(man, conv_only=True) == [0, 1, 1, 1, 2]   # the convolution is unchanged


@pytest.mark.parametrize('opts', [BIAS, FCN, dict(BIAS, **FCN)], ids=['bias', 'fcn', 'both'])
def test_channel8_option_configs_stay_generic(opts):
    """The small option configs of test_model_build.py (channel 8, a 16-16
    radial MLP) are not SevenNet-0-shaped whatever their options."""
    cfg = {'chemical_species': ['Hf', 'O'], 'cutoff': 4.0, 'channel': 8, 'lmax': 2,
           'is_parity': False, 'num_convolution_layer': 3, 'conv_denominator': 7.0,
           'weight_nn_hidden_neurons': [16, 16], 'self_connection_type': 'linear',
           'cutoff_function': {'cutoff_function_name': 'XPLOR', 'cutoff_on': 3.5}}
    cfg.update(opts)
    man = mb.model_manifest(mb.resolve_config(cfg))
    assert sevennet0_kinds(man) is None and man['family'] == 'nequip'
