"""Fine-tuning models with linear biases and / or the FCN readout on the
explicit step's HIP kernels (train_explicit.py; csrc/fcn_train.hip, the
column-sum kernel of csrc/train_ops.hip).  Needs an MI355X: ``pytest -m gpu``.

The FCN kernels are compared with the float64 torch formulas of the same
module (which test_train_explicit_options.py pins against autograd), the whole
step with float64 autograd of the trainable model at the project's bars
(test_gpu_train.py), on the deployments of _train_options.py."""
import ctypes

import numpy as np
import pytest
import torch

import _train_options as opts
from _conv_cpu import CpuConvBackend
from sevennet_finetuning_amd import _keys as KEY
from sevennet_finetuning_amd import train
from sevennet_finetuning_amd.structures import diamond_primitive, mixed_symbols

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

OPTIONS = {
    'bias': opts.BIAS,
    'bias_fcn24_silu': dict(opts.BIAS, **opts.fcn([24], 'silu')),
    'fcn7x5x3_tanh': opts.fcn([7, 5, 3], 'tanh'),
}


@pytest.fixture(scope='module')
def deps(tmp_path_factory):
    return opts.Deployments(tmp_path_factory.mktemp('gpu_train_options'))


def _graphs(seeds, cells=(3, 3, 3)):
    """test_gpu_train.py::_batch on this module's species"""
    gs = []
    for s in seeds:
        pos, cell = diamond_primitive(cells, sigma=0.05, seed=s)
        types = np.array([opts.SPECIES.index(x) for x in mixed_symbols(len(pos), seed=s + 1)])
        rng = np.random.default_rng(1000 + s)
        gs.append(train.labeled_graph(pos, cell, types, 5.0, energy=-4.0 * len(pos),
                                      force=rng.normal(0, 0.3, (len(pos), 3)),
                                      stress=rng.normal(0, 2e-3, 6)))
    return gs


def _coll(seeds):
    return train.collate(_graphs(seeds), device=DEV, dtype=torch.float32)


# ------------------------------------------------------------------ the FCN kernels
HIDDEN = [[30, 30], [7, 5, 3], [1], [128, 96], [128, 128, 128, 128]]
ACTS = ['relu', 'silu', 'tanh', 'sigmoid', 'abs', 'elu']
ATOMS = [1, 7, 8, 9, 61, 257]
KINKED = ('relu', 'abs', 'elu')


def fcn_problem(hidden, act, n, seed=0):
    """float32-representable inputs as float64: x, x' ~ N(0, 1) [n, 128], the
    matrices ~ N(0, 1) / sqrt(fan_in), seeds sb ~ N(0, 1), sbd ~ U(0.5, 2)"""
    g = torch.Generator().manual_seed(1000 * seed + 10 * n + len(hidden) + ACTS.index(act))
    r32 = lambda t: t.float().double()   # noqa: E731
    w = [128] + list(hidden)
    Ws = [r32(torch.randn(a, b, generator=g, dtype=torch.float64) / a ** 0.5)
          for a, b in zip(w, w[1:] + [1])]
    x, xd = (r32(torch.randn(n, 128, generator=g, dtype=torch.float64)) for _ in range(2))
    if act in KINKED:
        # up to 512 units per atom, each within 1e-4 of the kink with probability
        # ~1e-4: at the small atom counts one such atom is already more than
        # the 10 % the comparison may leave out.  While the float64 reference
        # alone is over that cap, the rows of x of those atoms are drawn again.
        from sevennet_finetuning_amd.train_explicit import _Fcn
        for _ in range(50):
            keep = fcn_kept_atoms(act, _Fcn(w, act, 1.3).forward(x, Ws, None, need_dx=False), n)
            if int((~keep).sum()) <= n // 10:
                break
            x[~keep] = r32(torch.randn(int((~keep).sum()), 128, generator=g, dtype=torch.float64))
    sb = r32(torch.randn(n, generator=g, dtype=torch.float64))
    sbd = r32(0.5 + 1.5 * torch.rand(n, generator=g, dtype=torch.float64))
    return w, Ws, x, xd, sb, sbd


def fcn_run(f, Ws, packed, x, xd, sb, sbd):
    """the three passes; every output by name"""
    st = f.forward(x, Ws, packed, seed=None)
    sd = f.tangent(st, xd)
    XB = f.dual(st, sb, sbd)
    out = {'s': st['s'], 'ds/dx': st['dx'], "s'": sd, 'xbar': XB}
    for k in range(f.nh):
        out.update({f'z{k + 1}': st['Z'][k], f"z'{k + 1}": st['ZD'][k], f'a{k + 1}': st['A'][k],
                    f'zbar{k + 1}': st['ZB'][k]})
    return st, out


def fcn_kept_atoms(act, st, n):
    """atoms kept in the comparison: for the kinked activations those with
    every float64 |z_k| >= 1e-4 (a sign flip at a kink is not an error)"""
    keep = torch.ones(n, dtype=torch.bool)
    if act in KINKED:
        for z in st['Z']:
            keep &= (z.abs() >= 1e-4).all(1)
    return keep


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('hidden', HIDDEN, ids=lambda h: 'x'.join(map(str, h)))
def test_fcn_kernels_vs_fp64(hidden, act):
    """Forward + first reverse, tangent and dual reverse of csrc/fcn_train.hip
    against _Fcn's float64 torch formulas, every output within 2e-5 of its
    largest entry (the bar of test_radial_mlp_chain_kernels_vs_fp64); atom
    counts around the 8-atoms-per-wave pass and a ragged tail, widths whose
    weights sit in LDS or are read from global memory; the same call twice
    gives identical bits."""
    from sevennet_finetuning_amd import _lib
    from sevennet_finetuning_amd.train_explicit import _Fcn
    lib = _lib.load()
    for n in ATOMS:
        w, Ws, x, xd, sb, sbd = fcn_problem(hidden, act, n)
        ref_st, ref = fcn_run(_Fcn(w, act, 1.3), Ws, None, x, xd, sb, sbd)
        keep = fcn_kept_atoms(act, ref_st, n)
        assert int((~keep).sum()) <= n // 10, (n, int((~keep).sum()))
        f = _Fcn(w, act, 1.3, lib=lib)
        assert int(lib.e3gnn_fcn_packed_floats(f.nh, f.cw)) == f.packed_floats
        T = lambda t: t.float().to(DEV)   # noqa: E731
        packed = f.pack([T(W) for W in Ws])
        assert packed.numel() == f.packed_floats
        runs = [fcn_run(f, None, packed, T(x), T(xd), T(sb), T(sbd))[1] for _ in range(2)]
        torch.cuda.synchronize()
        for name, want in ref.items():
            got = runs[0][name].double().cpu()
            assert torch.equal(runs[0][name], runs[1][name]), (n, name)
            assert torch.isfinite(got).all(), (n, name)
            rows = keep if want.shape[0] == n else torch.cat([keep, keep])
            if not bool(rows.any()):
                continue
            err = float((got[rows] - want[rows]).abs().max())
            top = float(want[rows].abs().max())
            assert err <= 2e-5 * max(top, 1e-30), (n, name, err, top)


def test_fcn_kernels_refuse_dims_beyond_their_limits():
    from sevennet_finetuning_amd import _lib
    lib = _lib.load()
    for widths in ([128, 160], [128, 8, 6, 8, 6, 4], [200, 8]):
        cw = (ctypes.c_int32 * len(widths))(*widths)
        assert lib.e3gnn_fcn_packed_floats(len(widths) - 1, cw) < 0
        assert lib.e3gnn_fcn_train_forward(0, len(widths) - 1, cw, 0, 1.0, *([None] * 8)) != 0


def test_column_sums_vs_fp64():
    """e3gnn_colsum_grouped: several blocks of different shapes in one launch
    (leading columns of wider rows, more than 64 columns, a single row), added
    to what dst holds, twice the same bits."""
    from sevennet_finetuning_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    shapes = [(108, 576, 224), (1, 128, 128), (7, 1, 1), (257, 130, 65), (1031, 64, 64)]
    srcs = [torch.randn(r, ld, generator=g).to(DEV) for r, ld, _ in shapes]
    init = [torch.randn(c, generator=g) for _, _, c in shapes]
    outs = []
    for _ in range(2):
        dst = [t.clone().to(DEV) for t in init]
        descs = (_lib.ColsumDesc * len(shapes))()
        for d, s, o, (r, ld, c) in zip(descs, srcs, dst, shapes):
            d.src, d.dst, d.ld, d.rows, d.cols = s.data_ptr(), o.data_ptr(), ld, r, c
        _lib.check(lib.e3gnn_colsum_grouped(len(shapes), descs, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        outs.append(dst)
    for a, b, s, i, (r, ld, c) in zip(outs[0], outs[1], srcs, init, shapes):
        assert torch.equal(a, b)
        blk = s.double().cpu()[:, :c]
        want = i.double() + blk.sum(0)
        # r + 1 float32 additions per column: the worst-case bound of a summation
        bound = (r + 1) * 2.0 ** -24 * float((i.double().abs() + blk.abs().sum(0)).max())
        assert float((a.double().cpu() - want).abs().max()) <= bound


# ------------------------------------------------------------------ the whole step
@pytest.mark.parametrize('opt', list(OPTIONS))
def test_explicit_step_gradients_vs_fp64(deps, opt):
    """The explicit step on the HIP kernels against float64 autograd of the
    same loss, at the bars of test_gpu_train.py::test_explicit_step_gradients_vs_fp64."""
    from sevennet_finetuning_amd.nn import SevenNetTrainable
    from sevennet_finetuning_amd.train_explicit import ExplicitStep
    d = deps.dir(opt, OPTIONS[opt])
    m32 = SevenNetTrainable(d, device=DEV)
    m64 = SevenNetTrainable(d, device='cpu', conv_backend=CpuConvBackend(), dtype=torch.float64)
    cfg = {'loss': 'huber', 'loss_param': {'delta': 0.01}, 'force_loss_weight': 1.0,
           'stress_loss_weight': 1e-2, 'is_train_stress': True,
           'continue': {'fisher_information': False, 'opt_params': False}}
    fns = train.get_loss_functions_from_config(cfg)
    gs = _graphs([8, 9])
    step = ExplicitStep(m32)
    m32.zero_grad()
    out = step.forward(train.collate(gs, device=DEV, dtype=torch.float32))
    loss = sum(f.get_loss(out, m32) * w for f, w in fns)
    loss.backward()
    step.backward(out[KEY.PRED_TOTAL_ENERGY].grad, out[KEY.PRED_FORCE].grad, out[KEY.PRED_STRESS].grad)
    g32 = m32.flat_grad.detach().cpu().double().clone()
    m64.train(True)
    m64.zero_grad()
    o64 = m64(train.collate(gs, dtype=torch.float64))
    sum(f.get_loss(o64, m64) * w for f, w in fns).backward()
    m64.train(False)
    g64 = m64.flat_grad.detach().clone()
    ferr = float((out[KEY.PRED_FORCE].detach().cpu().double() - o64[KEY.PRED_FORCE]).abs().max())
    gerr = float((g32 - g64).norm() / g64.norm())
    worst = []
    zero = []
    for name, (off, n, _) in m64.slices.items():
        ref = g64[off:off + n]
        if float(ref.abs().max()) == 0.0:
            zero.append((name, float(g32[off:off + n].abs().max())))
            continue
        worst.append((float((g32[off:off + n] - ref).norm() / ref.norm()), name))
    worst.sort(reverse=True)
    print(f'{opt}: force error {ferr:.3g} eV/A, whole-gradient error {gerr:.3g}; '
          'per-tensor relative gradient errors, worst five:', worst[:5])
    assert ferr < 1e-4
    assert gerr < 1e-4
    for name, top in zero:
        assert top == 0.0, name
    for err, name in worst:
        assert err < 2e-4, name
    assert any(n.endswith('.bias') or n.startswith('readout_FCN.') for _, n in worst)


SGD = {'loss': 'mse', 'force_loss_weight': 0.5, 'stress_loss_weight': 1e-3,
       'is_train_stress': True, 'optimizer': 'sgd', 'optim_param': {'lr': 1e-3},
       'scheduler': 'exponentiallr', 'scheduler_param': {'gamma': 0.99},
       'continue': {'fisher_information': False, 'opt_params': False}}


def test_trainer_picks_the_explicit_step_and_takes_the_autograd_step(deps):
    """as test_gpu_train.py::test_explicit_and_autograd_trainers_take_the_same_step,
    for the bias + FCN model"""
    from sevennet_finetuning_amd.nn import SevenNetTrainable
    d = deps.dir('bias_fcn24_silu', OPTIONS['bias_fcn24_silu'])
    b, mem = _coll([11, 12]), _coll([13])
    deltas = []
    for explicit in (True, False):
        m = SevenNetTrainable(d, device=DEV)
        before = m.flat.detach().clone()
        tr = train.Trainer(m, dict(SGD, explicit_grad=explicit))
        assert (tr.explicit is not None) == explicit
        tr.rehearsal_step(b, mem)
        deltas.append((m.flat.detach() - before).double())
    assert float(deltas[1].norm()) > 0
    err = float((deltas[0] - deltas[1]).norm() / deltas[1].norm())
    print('explicit vs autograd SGD step, relative norm of the difference:', err)
    assert err < 1e-4


def test_graphed_rehearsal_step_equals_eager(deps):
    """The captured step (train.GraphedRehearsalStep) with the FCN kernels, the
    bias adds and the column-sum launch in it, against the eager step over
    three batches of one shape, Adam and EWC: the bars of
    test_gpu_train.py::test_graphed_rehearsal_step_equals_eager."""
    from sevennet_finetuning_amd.nn import SevenNetTrainable
    d = deps.dir('bias_fcn24_silu', OPTIONS['bias_fcn24_silu'])
    batches = [(_coll([1, 2]), _coll([3])), (_coll([4, 5]), _coll([6])), (_coll([7, 8]), _coll([9]))]

    def run(graph):
        m = SevenNetTrainable(d, device=DEV)
        fisher = {n: torch.full_like(p, 1e-3) for n, p in m.named_parameters()}
        opt = {n: p.detach().clone() for n, p in m.named_parameters()}
        cfg = {'loss': 'huber', 'loss_param': {'delta': 0.01}, 'force_loss_weight': 1.0,
               'stress_loss_weight': 0.01, 'is_train_stress': True, 'optimizer': 'adam',
               'optim_param': {'lr': 1e-4}, 'scheduler': 'exponentiallr',
               'scheduler_param': {'gamma': 0.99}, 'device': DEV, 'hip_graph': graph,
               'continue': {'fisher_information': fisher, 'opt_params': opt, 'ewc_lambda': 1e2}}
        tr = train.Trainer(m, cfg)
        assert tr.explicit is not None
        m.train(True)
        losses = [tuple(float(x) for x in tr.rehearsal_step(b, mm)) for b, mm in batches]
        if graph:
            assert len(tr._graphed.cache) == 1
        return m.flat.detach().double().cpu(), losses

    theta0 = SevenNetTrainable(d, device=DEV).flat.detach().double().cpu()
    fe, le = run(False)
    fg, lg = run(True)
    for a, b in zip(le, lg):
        assert abs(a[0] - b[0]) <= 1e-5 * abs(a[0]) and abs(a[1] - b[1]) <= 1e-5 * abs(a[1])
    de, dg = fe - theta0, fg - theta0
    err = float((de - dg).norm() / de.norm())
    print('graphed vs eager parameter moves, relative norm of the difference:', err)
    assert err < 1e-2
