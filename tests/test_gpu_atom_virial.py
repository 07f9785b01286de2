"""Per-atom virial on the device (csrc/atom_virial.hip behind
e3gnn_atom_virial) and through every layer above it: both engines of the
library, the segment API with ghosts, the decomposed Python driver, the LAMMPS
pair styles and the calculator.  Needs an MI355X: ``pytest -m gpu``.

The quantity is the edge-gradient partition (_atom_virial.py; DESIGN.md
"Per-atom virial"): W_a = 1/2 sum_{centre(e)=a} v_e + 1/2 sum_{nbr(e)=a} v_e
with v_e the edge's virial term.  Bounds, with u = 2^-24, m_a the number of
edge ends on atom a and S_aq the fp64 sum of the absolute values of the terms
of entry (a, q) (every product r g, scaled as in W):

* kernel against its own fp32 inputs: (m_a + 4) u S_aq  (_atom_virial.kernel_bound);
* sum over atoms against the library's virial6: (E + 4) u sum_e |terms|;
* against an independent gradient that may differ by F_TOL per edge component:
  F_TOL 1/2 sum_ends w_q(r_e) + sum_ends u |r||g| + the kernel bound, with
  F_TOL = 1e-4 eV/A, the project's per-edge gradient and decomposed-force bar.

Measured on the MI355X: kernel against its inputs 1.5-12 % of
the bound (largest error 7.6e-7 eV); against the fp64 oracle 4.2e-6 eV (Si
2x2x1) and 1.2e-5 eV (HfO2 res.dat) under bounds of 0.0054-0.0099 eV; two
ranks against serial 6.6e-6 eV; pair styles' vatom 2.6e-6 eV.
"""
import json
import os
import socket

import numpy as np
import pytest
import torch

from _atom_virial import U, gradient_bound, kernel_bound, partition, sum_bound
from _systems import load_manifest_symbols, system

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HFO2 = os.path.join(ROOT, 'sevennet_finetuning_amd', 'assets', 'hfo2_example')
SYMS = load_manifest_symbols()
DEV = 'cuda:0'
F_TOL = 1e-4


@pytest.fixture(scope='module')
def model():
    from sevennet_finetuning_amd.model import E3GNNModel
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return E3GNNModel(device=DEV)


def _structure(name):
    """(pos, cell or None, types, pbc) of a T1 system."""
    si = SYMS.index('Si')
    if name == 'diamond_primitive':
        # two atoms, every second neighbour is the atom's own image (12 edges
        # with centre == nbr per atom); the second atom pushed 0.1 A along x
        a = 5.43
        cell = 0.5 * a * np.array([[0., 1, 1], [1, 0, 1], [1, 1, 0]])
        pos = np.array([[0., 0, 0], [0.25 * a + 0.1, 0.25 * a, 0.25 * a]])
        return pos, cell, np.array([si, si]), True
    if name == 'cluster_plus_far_atom':
        # an open 5-atom cluster and one atom 20 A away: a row without edges
        pos = np.array([[0., 0, 0], [2.3, 0.1, 0], [-0.2, 2.4, 0.3], [0.4, -0.3, 2.2],
                        [1.9, 2.1, 1.8], [20.0, 0, 0]])
        return pos, None, np.array([si, SYMS.index('O'), si, SYMS.index('Hf'), si, si]), False
    pos, cell, types = system(name, SYMS)
    return pos, cell, types, True


def _graph(pos, cell, cutoff, pbc):
    from sevennet_finetuning_amd.neighbor import neighbor_list
    ei, sh = neighbor_list(pos, cell, cutoff, pbc=(pbc,) * 3)
    vec = pos[ei[1]] - pos[ei[0]] + (sh @ cell if cell is not None else 0.0)
    return ei, vec.astype(np.float32)


def _evaluate(m, pos, cell, types, pbc=True):
    ei, vec = _graph(pos, cell, m.cutoff, pbc)
    t = lambda a, dt=torch.int32: torch.as_tensor(a, dtype=dt, device=DEV)  # noqa: E731
    args = (t(types), t(ei[0]), t(ei[1]), t(vec, torch.float32))
    r = m.energy_forces(*args, want_edge_grad=True, want_atom_virial=True)
    again = m.energy_forces(*args, want_edge_grad=True, want_atom_virial=True)
    plain = m.energy_forces(*args)
    h = lambda x: x.detach().cpu().numpy()  # noqa: E731
    return {'ei': ei, 'vec': vec, 'W': h(r['atomic_virial']), 'W2': h(again['atomic_virial']),
            'grad': h(r['edge_grad']), 'virial': h(r['virial']), 'forces': h(r['forces']),
            'plain': {k: h(v) for k, v in plain.items()}}


_CACHE = {}


def _sevennet0(model, name):
    """One evaluation per system, shared by T1-T3."""
    if name not in _CACHE:
        pos, cell, types, pbc = _structure(name)
        _CACHE[name] = (_evaluate(model, pos, cell, types, pbc), pos, cell, types)
    return _CACHE[name]


def _check_kernel(ev, n, tag):
    """T1 and T2 on one evaluation."""
    ei, vec, g, W = ev['ei'], ev['vec'], ev['grad'], ev['W']
    assert W.shape == (n, 6) and W.dtype == np.float32
    want, S, m = partition(n, ei[0], ei[1], vec, g)
    err, bound = np.abs(W - want), kernel_bound(S, m)
    print(f'{tag}: T1 max err {err.max():.3e}, max err/bound '
          f'{(err / np.maximum(bound, 1e-300)).max():.3f}, max |W| {np.abs(want).max():.3e}, '
          f'max ends {int(m.max())}')
    assert np.all(err <= bound)
    assert np.all(W[m == 0] == 0)
    assert np.array_equal(W, ev['W2'])                    # fixed order, no atomics
    tot, sb = W.astype(np.float64).sum(0), sum_bound(vec, g)
    print(f'{tag}: T2 max |sum_a W_a - virial| {np.abs(tot - ev["virial"]).max():.3e}, '
          f'bound {sb.min():.3e}..{sb.max():.3e}')
    assert np.all(np.abs(tot - ev['virial']) <= sb)
    # the option changes nothing else, and the default dict has no new key
    assert 'atomic_virial' not in ev['plain'] and 'edge_grad' not in ev['plain']
    assert np.array_equal(ev['plain']['forces'], ev['forces'])
    assert np.array_equal(ev['plain']['virial'], ev['virial'])
    return want, S, m


T1_SYSTEMS = ['si_rng0_2x2x1', 'hfo2_resdat', 'diamond_primitive', 'cluster_plus_far_atom']


@pytest.mark.parametrize('name', T1_SYSTEMS)
def test_kernel_against_its_inputs_and_sum_rule(model, name):
    """T1 + T2 on SevenNet-0: W recomputed in fp64 from the returned fp32
    edge_grad and edge_vec, two calls bit for bit, rows sum to ``virial``."""
    ev, pos, _, _ = _sevennet0(model, name)
    want, _, m = _check_kernel(ev, len(pos), name)
    assert np.abs(want).max() > 1e-3                      # a real result, not zeros
    if name == 'diamond_primitive':
        ei = ev['ei']
        assert [(int(((ei[0] == a) & (ei[1] == a)).sum())) for a in (0, 1)] == [12, 12]
    if name == 'cluster_plus_far_atom':
        assert m[5] == 0 and np.all(ev['W'][5] == 0) and m[:5].min() > 0


@pytest.mark.parametrize('name', ['si_rng0_2x2x1', 'hfo2_resdat'])
def test_atom_virial_against_the_fp64_oracle(model, name):
    """T3: the partition of the fp64 oracle's own edge-vector gradient
    (torch.autograd.grad(E, edge_vec) of SevenNet0Ref.energy)."""
    from oracle.neighbor import neighbor_list
    from oracle.sevennet_ref import SevenNet0Ref
    ev, pos, cell, types = _sevennet0(model, name)
    n = len(pos)
    ref = SevenNet0Ref(dtype=torch.float64)
    ei, sh = neighbor_list(pos, cell, ref.cutoff)
    o = ref.energy(torch.tensor(pos).requires_grad_(True), torch.tensor(types), torch.tensor(ei),
                   torch.tensor(sh), torch.tensor(cell), False)
    g, = torch.autograd.grad(o['energy'], o['edge_vec'])
    rv, g = o['edge_vec'].detach().numpy(), g.numpy()
    want, _, _ = partition(n, ei[0], ei[1], rv, g)
    _, S, m = partition(n, ev['ei'][0], ev['ei'][1], ev['vec'], ev['grad'])
    bound = gradient_bound(n, ei[0], ei[1], rv, g, F_TOL) + kernel_bound(S, m)
    err = np.abs(ev['W'] - want)
    print(f'{name}: T3 max err {err.max():.3e}, max err/bound {(err / bound).max():.3f}, '
          f'bound {bound.min():.3e}..{bound.max():.3e}, median |W| {np.median(np.abs(want)):.3e}')
    assert np.all(err <= bound)


def test_generic_engine(model):
    """T4: the HfO2 example deployment (generic engine of the same library)
    on res.dat: T1, T2, and sum_a W_a / V against the oracle's stress."""
    from oracle.neighbor import neighbor_list
    from oracle.nequip_ref import NequIPRef
    from sevennet_finetuning_amd.model import E3GNNModel
    m = E3GNNModel(HFO2, device=DEV)
    assert m.family == -1
    pos, cell, types = system('hfo2_resdat', m.chemical_symbols)
    ev = _evaluate(m, pos, cell, types)
    want, _, _ = _check_kernel(ev, len(pos), 'hfo2_example')
    assert np.abs(want).max() > 1e-3
    ref = NequIPRef(HFO2)
    ei, sh = neighbor_list(pos, cell, ref.cutoff)
    stress = ref(torch.tensor(pos), torch.tensor(types), torch.tensor(ei), torch.tensor(sh),
                 torch.tensor(cell))['stress'].numpy()
    got = ev['W'].astype(np.float64).sum(0) / abs(np.linalg.det(cell))
    print(f'hfo2_example: T4 max |sum W / V - stress| {np.abs(got - stress).max():.3e}')
    assert np.abs(got - stress).max() <= 2e-6


def test_segment_api_ghost_rows_and_state_flag(model):
    """T5: e3gnn_graph_set with ghosts (rank 0 of 2 of si_rng0_3x3x3): ghost
    rows hold the neighbour-side halves alone and are not zero; the call is
    refused before e3gnn_forces and after a new e3gnn_graph_set."""
    from sevennet_finetuning_amd import _lib
    from sevennet_finetuning_amd.parallel import (HipSegmentEngine, ParallelE3GNN, brick_grid,
                                                  build_rank_graph, local_handshake)
    pos, cell, types = system('si_rng0_3x3x3', SYMS)
    grid = brick_grid(2)
    rgs = local_handshake([build_rank_graph(pos, cell, types, model.cutoff, grid, r) for r in range(2)])
    rg = rgs[0]
    nl, n = rg.n_local, rg.n_local + rg.n_ghost
    assert rg.n_ghost > 0
    eng = HipSegmentEngine(model)
    drv = ParallelE3GNN(eng)
    drv.set_graph(rg, emulate=True)      # one rank's call sequence, exchanges as local copies
    lib, ctx, s = model.lib, model._ctx, model.stream_handle()
    w = torch.full((n, 6), float('nan'), device=DEV)
    eng.graph_set()
    assert lib.e3gnn_atom_virial(ctx, w.data_ptr(), s) == 1          # E3GNN_ERR_ARG
    assert b'e3gnn_forces' in lib.e3gnn_last_error()
    assert lib.e3gnn_atom_virial(ctx, None, s) == 1
    drv.evaluate()
    # the same per-edge gradient again, this time copied out
    egrad = torch.empty(len(rg.center), 3, device=DEV)
    _lib.check(lib.e3gnn_forces(ctx, None, None, egrad.data_ptr(), s))
    _lib.check(lib.e3gnn_atom_virial(ctx, w.data_ptr(), s))
    W, g = w.cpu().numpy(), egrad.cpu().numpy()
    assert np.isfinite(W).all() and np.isfinite(g).all()
    vec = np.asarray(rg.vec, dtype=np.float32)
    want, S, m = partition(n, rg.center, rg.nbr, vec, g)
    assert np.all(np.abs(W - want) <= kernel_bound(S, m))
    nb_only, S1, m1 = partition(n, rg.center, rg.nbr, vec, g, sides=(False, True))
    assert np.all(np.abs(W[nl:] - nb_only[nl:]) <= kernel_bound(S1, m1)[nl:])
    assert np.all(np.abs(W[nl:]).max(1) > 0) and m1[nl:].min() > 0   # every ghost row carries halves
    assert np.abs(nb_only[:nl] - want[:nl]).max() > 1e-3             # owned rows have both sides
    # the per-edge gradient belongs to the graph it was computed on
    eng.graph_set()
    assert lib.e3gnn_atom_virial(ctx, w.data_ptr(), s) == 1
    assert b'e3gnn_forces' in lib.e3gnn_last_error()


def test_decomposed_python_path(model, tmp_path):
    """T6: two gloo ranks on one GPU, mixed_3x3x3, evaluate(atom_virial=True):
    W gathered by owner against the serial W within the decomposed-versus-
    serial bar (1e-4 per edge gradient component), one more exchange than the
    default, energy and forces bit for bit those of the default call."""
    import torch.multiprocessing as mp
    from _atom_virial_workers import worker
    name = 'mixed_3x3x3'
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    out = str(tmp_path / 'w2.npz')
    mp.spawn(worker, args=(2, port, name, 'hip', out), nprocs=2, join=True)
    got = np.load(out)
    pos, cell, types = system(name, SYMS)
    ev = _evaluate(model, pos, cell, types)
    n = len(pos)
    ei, vec, g = ev['ei'], ev['vec'], ev['grad']
    _, S, m = partition(n, ei[0], ei[1], vec, g)
    bound = gradient_bound(n, ei[0], ei[1], vec, g, F_TOL) + kernel_bound(S, m)
    err = np.abs(got['atomic_virial'] - ev['W'])
    print(f'{name}: T6 max err {err.max():.3e}, max err/bound {(err / bound).max():.3f}')
    assert got['rows'][2] > 0 and got['rows'][0] == got['rows'][1]
    assert np.all(err <= bound)
    assert got['exchanges'][1] == got['exchanges'][0] + 1
    assert got['same'][0] and not got['default_has_key'][0]


def _pair_case(case, tmp_path):
    from test_gpu_native import ASSET, KATS, _write_structure
    if case == 'si':
        pos, cell, _ = system('si_rng0_3x3x3', SYMS)
        path = tmp_path / 'si333.txt'
        _write_structure(path, pos, cell, ['Si'] * len(pos))
        kat = next(k for k in KATS['kats'] if k['name'] == 'si_rng0_3x3x3')
        return ASSET, path, kat['energy'], 216, True
    from sevennet_finetuning_amd.structures import tile
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'hfo2_resdat.npz'))
    pos, cell = tile(d['pos'], d['cell'], (2, 2, 1))
    path = tmp_path / 'hfo2_221.txt'
    _write_structure(path, pos, cell, [str(s) for s in d['symbols']] * 4)
    return HFO2, path, 4 * KATS['kats_hfo2_example']['energy'], 384, False


@pytest.mark.parametrize('case,grid', [('si', (1, 1, 1)), ('si', (2, 2, 2)), ('hfo2', (2, 2, 1))])
def test_lammps_pair_styles_vatom(case, grid, tmp_path):
    """T7: both pair styles with VIRIAL_ATOM set inside the mini-LAMMPS
    scaffold, vatom reverse-communicated as compute stress/atom does: per atom
    against the library's own e3gnn_atom_virial of the whole box (an edge
    gradient may differ by 1e-4 per component between the decompositions: at
    most 1/2 ends x cutoff of that), summed against the style's global virial,
    bit for bit on a second compute; everything the run reports without
    --vatom still holds."""
    from test_gpu_native import _check_pair_run, _pair_check
    model_dir, path, kat_energy, n_atoms, thin = _pair_case(case, tmp_path)
    cutoff = float(json.load(open(os.path.join(model_dir, 'manifest.json')))['cutoff'])
    out = _pair_check(model_dir, path, grid, '--vatom')
    print(json.dumps({k: {q: v for q, v in out[k].items() if q.startswith('vatom')}
                      for k in ('serial', 'parallel')}))
    _check_pair_run(out, grid, kat_energy, n_atoms, thin=thin)
    for k in ('serial', 'parallel'):
        o = out[k]
        assert o['vatom_max_ends'] > 0
        assert o['vatom_max_diff'] <= 1e-4 * 0.5 * o['vatom_max_ends'] * cutoff, out
        assert o['vatom_sum_max_diff'] <= 1e-5 * max(1.0, out['max_virial_ref']), out
        assert o['vatom_repeat_bitwise'], out


def test_calculator_stresses(model):
    """T8: SevenNetCalculator 'stresses' on a stand-in atoms object: absent
    unless asked for, and summing to ``stress`` (same order, sign and 1/V)
    within the sum-rule bound over V; the mixed-periodicity host path too."""
    from sevennet_finetuning_amd.sevennet_calculator import SevenNetCalculator, SevenNetD3Calculator
    from sevennet_finetuning_amd.structures import Atoms
    pos, cell, types = system('si_rng0_2x2x1', SYMS)
    atoms = Atoms(symbols=['Si'] * len(pos), positions=pos, cell=cell)
    calc = SevenNetCalculator('SevenNet-0', device=DEV)
    assert 'stresses' in calc.implemented_properties
    calc.calculate(atoms)
    assert 'stresses' not in calc.results and 'stress' in calc.results
    calc.calculate(atoms, properties=['energy', 'forces'])
    assert 'stresses' not in calc.results
    stress0 = calc.results['stress'].copy()
    calc.calculate(atoms, properties=['energy', 'stresses'])
    r = calc.results
    assert r['stresses'].shape == (len(pos), 6) and np.array_equal(r['stress'], stress0)
    vol = abs(np.linalg.det(cell))
    ev, _, _, _ = _sevennet0(model, 'si_rng0_2x2x1')
    bound = sum_bound(ev['vec'], ev['grad'])[[0, 1, 2, 4, 5, 3]] / vol
    d = np.abs(r['stresses'].astype(np.float64).sum(0) - r['stress'])
    print(f'T8 max |sum stresses - stress| {d.max():.3e}, bound {bound.min():.3e}')
    assert np.all(d <= bound)
    # same values as the model's W, reordered, negated and over V
    assert np.array_equal(r['stresses'], -(ev['W'] / vol)[:, [0, 1, 2, 4, 5, 3]])
    # a slab (mixed periodicity): the host graph and the torch partition
    slab = Atoms(symbols=['Si'] * len(pos), positions=pos, cell=cell, pbc=[True, True, False])
    calc.calculate(slab, properties=['stresses'])
    r = calc.results
    assert r['stresses'].shape == (len(pos), 6)
    # two fp32 sums of the slab's E terms (2E halves): (2E + 8) u sum |terms| over V, and
    # sum_a |stresses_aq| <= sum_e |terms_q| / V makes this the tighter side of that bound
    from sevennet_finetuning_amd.util import unlabeled_atoms_to_graph
    E = unlabeled_atoms_to_graph(slab, calc.cutoff)['edge_index'].shape[1]
    d = np.abs(r['stresses'].astype(np.float64).sum(0) - r['stress'])
    assert 0 < E < len(ev['grad']) and np.all(d <= (2 * E + 8) * U * np.abs(r['stresses']).sum(0))
    calc.calculate(slab)
    assert 'stresses' not in calc.results
    # SevenNet-0 + D3: the D3 term has no per-atom virial, so the sum offers none
    both = SevenNetD3Calculator(device=DEV)
    assert 'stresses' not in both.implemented_properties
    both.calculate(atoms, properties=['energy', 'stresses'])
    assert 'stresses' not in both.results and 'stress' in both.results
