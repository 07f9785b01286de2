"""Shared by test_train_explicit_options.py and test_gpu_train_options.py:
SevenNet-0-shaped three-block deployments (kernel kinds 0, 1, 2; species Cl,
Li, P, S, Si) with ``use_bias_in_linear`` and / or ``readout_as_fcn``, built
as tests/test_gpu_options_fused.py builds them -- ``deploy_config(seed=7)``,
then every bias redrawn N(0, 0.5) and the species scale / shift set to
distinct values away from 1 / 0 (with e3nn's zero biases and the unit rescale
a dropped forward add or a seed without the scale would pass)."""
import json
import os

import numpy as np

SPECIES = ['Cl', 'Li', 'P', 'S', 'Si']


def fcn(hidden, act):
    return {'readout_as_fcn': True, 'readout_fcn_hidden_neurons': list(hidden),
            'readout_fcn_activation': act}


BIAS = {'use_bias_in_linear': True}


def config(options):
    from sevennet_finetuning_amd import model_build as mb
    cfg = mb.sevennet_shaped_config(128, 3)
    assert cfg['chemical_species'] == SPECIES
    cfg['irreps_manual'] = ['128x0e', '128x0e+64x1e+32x2e', '128x0e+64x1e+32x2e', '128x0e']
    cfg.update(options)
    return cfg


def deploy(options, out_dir, seed=11):
    """the deployment directory (manifest.json + weights.bin)"""
    from sevennet_finetuning_amd import model_build as mb
    mb.deploy_config(config(options), out_dir, seed=7)
    with open(os.path.join(out_dir, 'manifest.json')) as f:
        man = json.load(f)
    path = os.path.join(out_dir, 'weights.bin')
    flat = np.fromfile(path, dtype='<f4')
    g = np.random.default_rng(seed)
    for t in man['tensors']:
        o, n = t['offset'], t['numel']
        if t['name'].endswith('.bias'):
            flat[o:o + n] = g.normal(0, 0.5, n)
        elif t['name'] == 'rescale_atomic_energy.scale':
            flat[o:o + n] = 0.5 + 0.7 * np.arange(n)
        elif t['name'] == 'rescale_atomic_energy.shift':
            flat[o:o + n] = 0.3 - 0.9 * np.arange(n)
    flat.astype('<f4').tofile(path)
    return out_dir


class Deployments:
    """each deployment written once per module"""

    def __init__(self, root):
        self.root, self.dirs = root, {}

    def dir(self, name, options):
        if name not in self.dirs:
            self.dirs[name] = deploy(options, str(self.root / name))
        return self.dirs[name]
