"""The lock-step backward's tiles packed across centre boundaries (fused.hip,
k_conv_bwd_ls: a workgroup walks a contiguous range of CSR edges in rounds of
four consecutive 16-edge tiles, a lane takes its centre from center[] and the
centre's dE/dagg row from a window of four LDS slots).  The GPU tests need an
MI355X: ``pytest -m gpu``.

What can go wrong is an edge reading another centre's row, a window row staged
late or overwritten early, and a round or a workgroup range clipped at the
wrong edge.  The structures put the centre boundaries where each of these
shows:

* ``si``: Si diamond, 2 x 2 x 2 cells, 64 atoms of 28 edges, 1,792 edges: three
  tiles of every seven straddle two centres;
* ``hfo2``: the HfO2 cell, 96 atoms of 41-49 edges: boundaries at irregular
  slots, up to three centres in a round;
* ``stretched``: the Si lattice stretched to twice its constant, 3-4 edges per
  centre: every round is clipped by the four-centre window;
* ``cluster``: groups of atoms in vacuum with degrees 0, 1, 2 and 4, an
  isolated atom between bonded ones, 28 edges in all (one partly filled
  round, a centre without edges inside it);
* ``odd``: a mixed-species box of 898 edges (not a multiple of 16: the last
  tile of the last workgroup is partly filled);
* decomposed: the HfO2 cell x (3, 1, 1) over two ranks on one device, whose
  interior / boundary edge split (2,809 and 2,534 edges) is no multiple of 16.

SevenNet-0 is compared with the v1 kernels (``set_impl('v1')``) and the fp64
oracle: energy to 2e-6 relative, forces and the per-edge gradients (edge_grad:
an edge that read the wrong centre's row shows there first) to 1e-4 eV/A.  The
c64 and c32 families (two images with one pair per barrier) have no v1 kernels
and no SevenNet-0 oracle; their reference is the generic runtime-table engine,
at the same bars.  Every case is evaluated twice and the outputs compared bit
for bit.
"""
import numpy as np
import pytest
import torch

from _systems import load_manifest_symbols, system
from test_gpu_bwd_image import family_models, sevennet0  # noqa: F401

gpu = pytest.mark.gpu
SYMS = load_manifest_symbols()
CUTOFF = 5.0
E_TOL, F_TOL = 2e-6, 1e-4
CASES = ('si', 'hfo2', 'stretched', 'cluster', 'odd')
KEYS = ('energy', 'atomic_energy', 'forces', 'virial', 'edge_grad')


def _cluster():
    """Five atoms of degree 4, a triangle (2), a pair (1) split over the first
    and last index, and an isolated atom between the bonded groups."""
    tet = np.array([[0, 0, 0], [2.5, 0, 0], [0, 2.5, 0], [0, 0, 2.5], [1.6, 1.6, 1.6]])
    tri = np.array([[0, 0, 0], [2.7, 0, 0], [1.2, 2.5, 0.2]])
    pos = np.zeros((11, 3))
    pos[0], pos[10] = [5, 5, 5], [7.6, 5.3, 5]
    pos[1:6] = tet + [20, 5, 5]
    pos[6] = [20, 20, 20]
    pos[7:10] = tri + [5, 20, 8]
    return pos, np.eye(3) * 40.0, ['Si', 'Hf', 'O', 'O', 'O', 'O', 'Si', 'Si', 'O', 'Hf', 'O']


def structure(name):
    """(pos, cell, symbols) of a case."""
    from sevennet_finetuning_amd.structures import si_diamond
    if name == 'si':
        pos, cell = si_diamond((2, 2, 2), sigma=0.05)
        return pos, cell, ['Si'] * len(pos)
    if name == 'stretched':
        pos, cell = si_diamond((2, 2, 2), sigma=0.05)
        return 2.0 * pos, 2.0 * cell, ['Si'] * len(pos)
    if name == 'cluster':
        return _cluster()
    pos, cell, types = system({'hfo2': 'hfo2_resdat', 'odd': 'mixed_2x2x1'}[name], SYMS)
    return pos, cell, [SYMS[t] for t in types]


def make_case(name):
    from oracle.neighbor import neighbor_list
    pos, cell, symbols = structure(name)
    ei, sh = neighbor_list(pos, cell, CUTOFF)
    order = np.argsort(ei[0], kind='stable')
    ei, sh = ei[:, order], sh[order]
    vec = pos[ei[1]] - pos[ei[0]] + sh @ cell
    return {'name': name, 'pos': pos, 'cell': cell, 'symbols': symbols, 'ei': ei, 'sh': sh, 'vec': vec}


@pytest.fixture(scope='module', params=CASES)
def case(request):
    return make_case(request.param)


def rounds(center, n, per=512):
    """The kernel's rounds as (first edge, end) over workgroup ranges of ``per``
    edges: at most 64 consecutive edges of at most 4 consecutive centres."""
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(center, minlength=n))])
    out = []
    for ws in range(0, len(center), per):
        we, q = min(ws + per, len(center)), ws
        while q < we:
            end = min(q + 64, we, row_ptr[min(center[q] + 4, n)])
            out.append((q, end))
            q = end
    return out


def test_structures_cover_the_boundary_patterns():
    c = {k: make_case(k) for k in CASES}
    deg = {k: np.bincount(v['ei'][0], minlength=len(v['pos'])) for k, v in c.items()}
    rnd = {k: rounds(v['ei'][0], len(v['pos'])) for k, v in c.items()}
    assert len(deg['si']) == 64 and set(deg['si']) == {28}
    straddle = [c['si']['ei'][0][16 * t] != c['si']['ei'][0][16 * t + 15] for t in range(1792 // 16)]
    assert sum(straddle) * 7 == len(straddle) * 3   # 7 tiles = 4 centres: 3 of them straddle
    assert len(deg['hfo2']) == 96 and deg['hfo2'].min() == 41 and deg['hfo2'].max() == 49
    assert max(len(set(c['hfo2']['ei'][0][a:b])) for a, b in rnd['hfo2']) >= 3
    # every round of the stretched lattice ends at the window, not at 64 edges
    assert deg['stretched'].max() <= 4 and deg['stretched'].min() >= 1
    assert all(b - a < 64 for a, b in rnd['stretched']) and len(rnd['stretched']) >= 16
    d = deg['cluster']
    assert d.sum() < 64 and d.min() == 0 and {1, 2, 4} <= set(d)
    iso = int(np.nonzero(d == 0)[0][0])
    assert d[:iso].max() > 0 and d[iso + 1:].max() > 0
    assert deg['odd'].sum() % 16 != 0 and deg['odd'].sum() > 512
    # every edge is in exactly one round
    for k in CASES:
        assert rnd[k][0][0] == 0 and rnd[k][-1][1] == deg[k].sum(), k
        assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(rnd[k], rnd[k][1:])), k


@pytest.fixture(scope='module')
def oracle(case):
    """fp64 oracle of the case on its own edge list: energy, forces, dE/dvec."""
    from oracle.sevennet_ref import SevenNet0Ref
    ref = SevenNet0Ref(dtype=torch.float64)
    pos = torch.tensor(case['pos'], dtype=torch.float64, requires_grad=True)
    types = torch.tensor([SYMS.index(s) for s in case['symbols']])
    out = ref.energy(pos, types, torch.tensor(case['ei']), torch.tensor(case['sh'], dtype=torch.float64),
                     torch.tensor(case['cell'], dtype=torch.float64), False)
    g_pos, g_vec = torch.autograd.grad(out['energy'], [pos, out['edge_vec']])
    return {'energy': float(out['energy'].detach()), 'forces': -g_pos.numpy(), 'edge_grad': g_vec.numpy()}


def evaluate(model, case, symbols_all):
    dev = model.device
    t = lambda a, dt=torch.int32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
    types = [symbols_all.index(s) for s in case['symbols']]
    out = model.energy_forces(t(types), t(case['ei'][0]), t(case['ei'][1]), t(case['vec'], torch.float32),
                              want_edge_grad=True)
    return {k: out[k].cpu().numpy() for k in KEYS}


def _close(tag, got, ref, escale):
    de = abs(float(got['energy']) - float(ref['energy']))
    df = float(np.abs(got['forces'] - ref['forces']).max())
    dg = float(np.abs(got['edge_grad'] - ref['edge_grad']).max())
    print(f'{tag}: E={float(ref["energy"]):.6f} |dE|={de:.3e} (bar {E_TOL * escale:.3e}) '
          f'max|dF|={df:.3e} max|dgrad|={dg:.3e}')
    assert de <= E_TOL * escale
    assert df <= F_TOL
    assert dg <= F_TOL


@gpu
def test_sevennet0_matches_v1_and_oracle_and_repeats(sevennet0, case, oracle):  # noqa: F811
    model = sevennet0
    try:
        model.set_impl('v1')
        v1 = evaluate(model, case, SYMS)
    finally:
        model.set_impl('fused')
    a = evaluate(model, case, SYMS)
    b = evaluate(model, case, SYMS)
    assert all(np.isfinite(a[k]).all() for k in KEYS)
    escale = abs(oracle['energy'])
    _close(case['name'] + ' vs v1', a, v1, escale)
    _close(case['name'] + ' vs oracle', a, oracle, escale)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


@gpu
@pytest.mark.parametrize('name', ['si', 'stretched'])
def test_family_matches_generic_engine_and_repeats(family_models, name):  # noqa: F811
    fused, generic = family_models
    c = make_case(name)
    a, ref = evaluate(fused, c, fused.chemical_symbols), evaluate(generic, c, generic.chemical_symbols)
    b = evaluate(fused, c, fused.chemical_symbols)
    assert all(np.isfinite(a[k]).all() for k in KEYS)
    _close(f'{name} family {fused.family} vs generic', a, ref, abs(float(ref['energy'])))
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


DECOMPOSED = ('hfo2_resdat', (3, 1, 1))


def test_decomposed_split_is_no_multiple_of_16():
    from sevennet_finetuning_amd.parallel import brick_grid, build_rank_graph
    from sevennet_finetuning_amd.structures import tile
    pos, cell, types = system(DECOMPOSED[0], SYMS)
    pos, cell = tile(pos, cell, DECOMPOSED[1])
    types = np.tile(types, len(pos) // len(types))
    for rank in range(2):
        rg = build_rank_graph(pos, cell, types, CUTOFF, brick_grid(2), rank)
        center = np.asarray(rg.center)
        e_int = int((center < rg.n_interior).sum())
        # both parts span several workgroups of 512 edges
        assert e_int % 16 != 0 and e_int > 1024 and len(center) - e_int > 1024


@gpu
def test_decomposed_matches_single_device(sevennet0, tmp_path):  # noqa: F811
    """Two gloo ranks on the one device: interior and boundary edges are two
    launches over [0, e_int) and [e_int, E)."""
    import socket

    import torch.multiprocessing as mp
    from _parallel_workers import worker
    from oracle.neighbor import neighbor_list
    from sevennet_finetuning_amd.structures import tile
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    out = str(tmp_path / 'packed2.npz')
    mp.spawn(worker, args=(2, port, DECOMPOSED[0], 'hip', out, None, DECOMPOSED[1]), nprocs=2, join=True)
    got = np.load(out)
    pos, cell, types = system(DECOMPOSED[0], SYMS)
    pos, cell = tile(pos, cell, DECOMPOSED[1])
    ei, sh = neighbor_list(pos, cell, CUTOFF)
    order = np.argsort(ei[0], kind='stable')
    ei, sh = ei[:, order], sh[order]
    c = {'symbols': [SYMS[t] for t in np.tile(types, len(pos) // len(types))], 'ei': ei,
         'vec': pos[ei[1]] - pos[ei[0]] + sh @ cell}
    one = evaluate(sevennet0, c, SYMS)
    de = abs(float(got['energy']) - float(one['energy']))
    df = float(np.abs(got['forces'] - one['forces']).max())
    print(f'decomposed: E={float(one["energy"]):.6f} |dE|={de:.3e} max|dF|={df:.3e}')
    assert bool(got['repeat_same'][0]) and got['n_ghost'][0] > 0
    assert de <= E_TOL * abs(float(one['energy']))
    assert df <= F_TOL
