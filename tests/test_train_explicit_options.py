"""The hand-scheduled fine-tune derivatives (train_explicit.py) for models with
linear biases (``use_bias_in_linear``) and / or the FCN readout
(``readout_as_fcn``), against autograd of the trainable model: float64 on the
CPU, conv op _conv_cpu.py, deployments of _train_options.py (three blocks:
kernel kinds 0, 1, 2; random biases, species scale / shift away from 1 / 0).

A bias is a row-broadcast add on the primal rows (its gradient: the column sum
of the primal cotangent), the FCN readout a small per-atom MLP taken to second
order (_Fcn's torch formulas here; its HIP kernels are compared with the same
formulas in test_gpu_train_options.py)."""
import numpy as np
import pytest
import torch

import _train_options as opts
from _conv_cpu import CpuConvBackend
from sevennet_finetuning_amd import _keys as KEY
from sevennet_finetuning_amd import train
from sevennet_finetuning_amd.nn import SevenNetTrainable
from sevennet_finetuning_amd.structures import diamond_primitive, mixed_symbols

OPTIONS = {
    'bias': opts.BIAS,
    'fcn30x30_relu': opts.fcn([30, 30], 'relu'),
    'bias_fcn24_silu': dict(opts.BIAS, **opts.fcn([24], 'silu')),
    'fcn7x5x3_tanh': opts.fcn([7, 5, 3], 'tanh'),
    'fcn5_sigmoid': opts.fcn([5], 'sigmoid'),
    'fcn5_abs': opts.fcn([5], 'abs'),
    'fcn5_elu': opts.fcn([5], 'elu'),
    # beyond the FCN kernels' limits
    'fcn160_relu': opts.fcn([160], 'relu'),
    'fcn5layers_silu': opts.fcn([8, 6, 8, 6, 4], 'silu'),
}
SERVED = ['bias', 'fcn30x30_relu', 'bias_fcn24_silu', 'fcn7x5x3_tanh', 'fcn5_sigmoid', 'fcn5_abs',
          'fcn5_elu']


@pytest.fixture(scope='module')
def deps(tmp_path_factory):
    return opts.Deployments(tmp_path_factory.mktemp('train_options'))


def _model(deps, opt, **kw):
    kw = dict(dict(train_shift_scale=True, train_denominator=True), **kw)
    return SevenNetTrainable(deps.dir(opt, OPTIONS[opt]), device='cpu', conv_backend=CpuConvBackend(),
                             dtype=torch.float64, **kw)


def _batch(seeds=(0, 1), cells=(2, 2, 1)):
    gs = []
    for s in seeds:
        pos, cell = diamond_primitive(cells, sigma=0.08, seed=s)
        types = np.array([opts.SPECIES.index(x) for x in mixed_symbols(len(pos), seed=s + 1)])
        rng = np.random.default_rng(50 + s)
        gs.append(train.labeled_graph(pos, cell, types, 5.0, energy=-4.0 * len(pos),
                                      force=rng.normal(size=(len(pos), 3)),
                                      stress=rng.normal(size=6) * 1e-2))
    return train.collate(gs, dtype=torch.float64)


def _losses(kind):
    cfg = {'loss': kind, 'force_loss_weight': 0.7, 'stress_loss_weight': 0.05,
           'is_train_stress': True, 'continue': {'fisher_information': False, 'opt_params': False}}
    if kind == 'huber':
        cfg['loss_param'] = {'delta': 0.05}
    return train.get_loss_functions_from_config(cfg)


def _autograd(model, batch, fns):
    model.train(True)
    model.zero_grad()
    out = model(batch)
    loss = sum(f.get_loss(out, model) * w for f, w in fns)
    loss.backward()
    model.train(False)
    return out, float(loss), model.flat_grad.clone()


def _explicit(model, batch, fns):
    from sevennet_finetuning_amd.train_explicit import ExplicitStep
    step = ExplicitStep(model)
    model.zero_grad()
    out = step.forward(batch)
    loss = sum(f.get_loss(out, model) * w for f, w in fns)
    leaves = [out[KEY.PRED_TOTAL_ENERGY], out[KEY.PRED_FORCE], out[KEY.PRED_STRESS]]
    cE, cF, cS = torch.autograd.grad(loss, leaves, allow_unused=True)
    step.backward(cE, cF, cS)
    return out, float(loss), model.flat_grad.clone()


def _compare(model, batch, fns):
    """the bars of test_train_explicit.py::test_explicit_gradient_equals_autograd"""
    oa, la, ga = _autograd(model, batch, fns)
    oe, le, ge = _explicit(model, batch, fns)
    for k in (KEY.PRED_TOTAL_ENERGY, KEY.PRED_FORCE, KEY.PRED_STRESS):
        assert torch.allclose(oe[k].detach(), oa[k].detach(), rtol=1e-11, atol=1e-12), k
    assert abs(le - la) <= 1e-11 * abs(la)
    scale = ga.abs().max()
    bad = {}
    for name, (off, n, _) in model.slices.items():
        d = (ge[off:off + n] - ga[off:off + n]).abs().max()
        if d > 1e-9 * scale:
            bad[name] = (float(d), float(ga[off:off + n].abs().max()))
    assert not bad, bad
    return ga, ge


@pytest.mark.parametrize('kind', ['mse', 'huber'])
@pytest.mark.parametrize('opt', SERVED)
def test_explicit_gradient_equals_autograd(deps, opt, kind):
    model = _model(deps, opt)
    assert model._sevennet0_kinds() == [0, 1, 2]
    ga, _ = _compare(model, _batch(), _losses(kind))
    # the comparison is not 0 = 0: every bias and every FCN matrix has a gradient
    checked = [n for n in model.slices if n.endswith('.bias') or n.startswith('readout_FCN.')]
    # biases: the embedding and si1 / si2 of three blocks, plus the two readout
    # linears' where the readout is not an FCN
    want = (7 if 'bias' in opt else 0) + (len(OPTIONS[opt]['readout_fcn_hidden_neurons']) + 1
                                          if 'fcn' in opt else (2 if 'bias' in opt else 0))
    assert len(checked) == want, checked
    for name in checked:
        off, n, _ = model.slices[name]
        assert float(ga[off:off + n].abs().max()) > 0, name


def test_frozen_bias_and_frozen_fcn_layer(deps):
    """A frozen bias and a frozen FCN layer get exactly zero in both paths and
    leave every other gradient as it was (as
    test_train_explicit.py::test_explicit_gradient_frozen_linear)."""
    m = _model(deps, 'bias_fcn24_silu')
    batch = _batch(seeds=(4,))
    fns = _losses('mse')
    _, _, g_all = _explicit(m, batch, fns)
    frozen = ['1_self_interaction_2.linear.bias', 'readout_FCN.fcn.layer1.weight']
    for name in frozen:
        m.param(name).requires_grad_(False)
    _, _, ga = _autograd(m, batch, fns)
    _, _, ge = _explicit(m, batch, fns)
    keep = torch.ones_like(ge, dtype=torch.bool)
    for name in frozen:
        off, n, _ = m.slices[name]
        assert float(ga[off:off + n].abs().max()) == 0.0
        assert float(ge[off:off + n].abs().max()) == 0.0
        assert float(g_all[off:off + n].abs().max()) > 0
        keep[off:off + n] = False
    assert torch.allclose(ge, ga, rtol=1e-9, atol=1e-9 * float(ga.abs().max()))
    assert torch.allclose(ge[keep], g_all[keep], rtol=1e-12, atol=1e-14)


def test_frozen_denominators_do_not_divide_the_si2_bias(deps):
    """The default trainability: the frozen convolution denominators are folded
    into si2's matrices, its bias is not divided by them."""
    from sevennet_finetuning_amd.train_explicit import ExplicitStep
    m = _model(deps, 'bias', train_shift_scale=False, train_denominator=False)
    assert ExplicitStep(m).fold_den
    _compare(m, _batch(seeds=(3,)), _losses('mse'))


def test_routing(deps):
    from sevennet_finetuning_amd import train_explicit
    from sevennet_finetuning_amd.train_explicit import ExplicitStep
    cfg = {'loss': 'mse', 'force_loss_weight': 0.5, 'stress_loss_weight': 1e-3, 'is_train_stress': True,
           'optimizer': 'sgd', 'optim_param': {'lr': 1e-3}, 'scheduler': 'exponentiallr',
           'scheduler_param': {'gamma': 0.99},
           'continue': {'fisher_information': False, 'opt_params': False}, 'device': 'cpu'}
    for opt in ('bias', 'fcn30x30_relu', 'bias_fcn24_silu', 'fcn7x5x3_tanh'):
        m = _model(deps, opt)
        assert train_explicit.supported(m), opt
        assert train.Trainer(m, cfg).explicit is not None, opt
    for opt in ('fcn160_relu', 'fcn5layers_silu'):
        m = _model(deps, opt)
        assert not train_explicit.supported(m), opt
        assert train.Trainer(m, cfg).explicit is None, opt
        with pytest.raises(ValueError, match='FCN readout'):
            ExplicitStep(m)


@pytest.mark.parametrize('act', ['relu', 'silu', 'tanh', 'sigmoid', 'abs', 'elu'])
def test_fcn_activation_derivatives(act):
    """f' and f'' of the torch form against autograd of f and of f', on 1,000
    float64 points away from the kinks (|z| >= 1e-3)."""
    from sevennet_finetuning_amd.train_explicit import fcn_act_derivs
    g = torch.Generator().manual_seed(3)
    z = torch.randn(1000, generator=g, dtype=torch.float64) * 3
    z = torch.where(z.abs() < 1e-3, torch.full_like(z, 0.5), z).requires_grad_(True)
    ref = {'relu': torch.relu, 'silu': torch.nn.functional.silu, 'tanh': torch.tanh,
           'sigmoid': torch.sigmoid, 'abs': torch.abs, 'elu': torch.nn.functional.elu}[act]
    f, d1, d2 = fcn_act_derivs(act, z)
    assert float((f - ref(z)).abs().max()) <= 1e-12
    a1, = torch.autograd.grad(ref(z).sum(), z, create_graph=True)
    assert float((d1 - a1).abs().max()) <= 1e-12
    if a1.requires_grad:
        a2, = torch.autograd.grad(a1.sum(), z, allow_unused=True)
        a2 = torch.zeros_like(z) if a2 is None else a2
    else:                       # a piecewise-constant f' (relu, abs)
        a2 = torch.zeros_like(z)
    assert float((d2.detach() - a2).abs().max()) <= 1e-12
    # ... and of the formula for f' itself
    b2 = None
    if d1.requires_grad:
        b2, = torch.autograd.grad(d1.sum(), z, allow_unused=True)
    b2 = torch.zeros_like(z) if b2 is None else b2
    assert float((d2.detach() - b2).abs().max()) <= 1e-12
