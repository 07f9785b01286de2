"""Conditions on the inputs of the cell-list GPU tests (tests/_cells.py), on
the CPU.  These are conditions, not measurements: they keep
tests/test_gpu_d3.py, tests/test_gpu_neighbor.py and the batch case of
tests/test_gpu_batch.py from passing or failing for the wrong reason.

D3 table (``_cells.D3_CASES``): no pair image within 1e-5 (relative, r^2) of
either squared cutoff -- the kernel classifies pairs in fp32 and the oracle in
fp64, and at these short cutoffs one pair on the edge is worth ~1e-4 of the
energy -- and the outer 10 % of the cutoff sphere (in r^2) carries at least
1e-3 of the energy, a hundred times the GPU tests' energy bar, so that one
dropped boundary cell of the stencil is visible.

Oracle invariants: the equivalent lattice of ``relabelled`` gives the same D3
result and the same neighbour pairs; the host list equals the brute force of
oracle/neighbor.py on every periodic geometry.  oracle/neighbor.py enumerates
ceil(rc / height) images only and is right only for positions wrapped into
the cell it is given: it gets the wrapped copy throughout.
"""
import numpy as np
import pytest

import _cells as C
from oracle.neighbor import neighbor_list as brute_list
from sevennet_finetuning_amd.neighbor import neighbor_list

DAMPINGS = ('damp_bj', 'damp_zero')


# ------------------------------------------------------------------ makers
def test_makers_are_deterministic_and_as_described():
    for maker in (C.jittered_hfo2, C.sheared_hfo2, C.relabelled_hfo2, C.tiled_hfo2, C.dense_box):
        a, b = maker(), maker()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(C.ball(65)[0], C.ball(65)[0])
    _, cell, _ = C.sheared_hfo2()
    assert np.allclose(C.heights(cell), [7.84, 9.78, 10.26], atol=0.01)
    assert np.allclose(np.linalg.norm(cell, axis=1), [10.1, 12.1, 11.4], atol=0.05)
    _, cell, _ = C.relabelled_hfo2()
    assert np.allclose(C.heights(cell), [2.68, 7.30, 10.26], atol=0.01)
    assert np.allclose(np.linalg.norm(cell, axis=1), [10.1, 24.3, 16.8], atol=0.05)
    pos, cell, z = C.tiled_hfo2()
    assert len(pos) == len(z) == 384 and abs(cell[2, 2] - 41.05) < 0.01
    assert C.d3_default_nb(cell) == (1, 1, 2)
    assert C.d3_default_nb(C.jittered_hfo2()[1]) == (1, 1, 1)


@pytest.mark.parametrize('N', [64, 65, 66, 128, 129, 257, 513, 514])
def test_ball_is_a_complete_graph_at_5A(N):
    pos, _, _ = C.ball(N)
    d = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    assert np.linalg.norm(pos, axis=1).max() <= 2.4
    assert d.max() < 4.8 and d[~np.eye(N, dtype=bool)].min() > 1e-3


# ----------------------------------------------------------- D3 conditions
@pytest.mark.parametrize('name', list(C.D3_CASES))
def test_d3_case_conditions(name):
    pos, cell, z, pbc, kw = C.d3_case(name)
    assert 250.0 <= kw['rthr'] <= 400.0 and 120.0 <= kw['cn_thr'] <= 200.0
    gaps = [C.cutoff_gap(pos, cell, kw[k], pbc) for k in ('rthr', 'cn_thr')]
    print(f'{name}: cutoff gaps {gaps[0]:.2e} (rthr) {gaps[1]:.2e} (cn_thr)')
    assert min(gaps) >= 1e-5
    for damping in DAMPINGS:
        full = C.oracle_d3(pos, cell, z, damping, pbc, **kw)['energy']
        inner = C.oracle_d3(pos, cell, z, damping, pbc, rthr=0.9 * kw['rthr'],
                            cn_thr=kw['cn_thr'])['energy']
        shell = abs(full - inner) / abs(full)
        print(f'{name} {damping}: shell weight {shell:.2e}')
        assert shell >= 1e-3
    if not all(pbc):
        # inside the cell along the free axes (with a margin against rounding):
        # there the oracle, which wraps all three axes as the reference does,
        # and the kernel, which does not wrap a free axis, see the same atoms
        frac = pos @ np.linalg.inv(cell)
        free = [k for k in range(3) if not pbc[k]]
        assert frac[:, free].min() > 1e-9 and frac[:, free].max() < 1.0 - 1e-9


def test_slab_oracle_virial_is_inplane_strain_derivative():
    """The reference of the GPU slab-virial check: with no pair within 1e-5 of
    a cutoff, a strain step of 2e-6 moves no pair across one (r^2 changes by
    < 4.1e-6 relative) and the central difference is that of a smooth function."""
    pos, cell, z, pbc, kw = C.d3_case('slab_ttf')
    ref = C.oracle_d3(pos, cell, z, 'damp_bj', pbc, **kw)
    for eps, want in C.inplane_strain_derivatives(pos, cell, z, 'damp_bj', pbc, kw):
        got = np.sum(eps * C.virial33(ref['virial']))
        assert abs(got - want) <= 1e-6 * np.abs(ref['virial']).max()


# -------------------------------------------------------- oracle invariants
def test_relabelled_lattice_same_d3():
    pos, cell, z = C.jittered_hfo2()
    kw = dict(rthr=300.0, cn_thr=130.0)
    a = C.oracle_d3(pos, cell, z, 'damp_bj', **kw)
    for wrap in (True, False):
        p2, c2, _ = C.relabelled_hfo2(wrap=wrap)
        b = C.oracle_d3(p2, c2, z, 'damp_bj', **kw)
        assert abs(a['energy'] - b['energy']) <= 1e-12 * abs(a['energy'])
        assert np.abs(a['forces'] - b['forces']).max() <= 1e-12


def edge_lengths(pos, cell, ei, sh):
    return np.linalg.norm(pos[ei[1]] + sh @ cell - pos[ei[0]], axis=1)


@pytest.mark.parametrize('rc', [5.0, 6.0])
def test_relabelled_lattice_same_neighbours(rc):
    pos, cell, _ = C.jittered_hfo2()
    ea, sa = brute_list(C.wrapped(pos, cell), cell, rc)
    la = np.sort(edge_lengths(C.wrapped(pos, cell), cell, ea, sa))
    pw, c2, _ = C.relabelled_hfo2(wrap=True)
    pu, _, _ = C.relabelled_hfo2(wrap=False)
    eb, sb = brute_list(pw, c2, rc)              # the oracle: wrapped positions only
    eh, sh = neighbor_list(pu, c2, rc)           # the host list takes either copy
    if rc == 5.0:
        assert ea.shape[1] == 4302
        assert np.abs(sh).max() == 5
    for e, s, p in ((eb, sb, pw), (eh, sh, pu)):
        assert np.array_equal(e, ea)             # same (i, j), multiplicity included
        assert np.abs(np.sort(edge_lengths(p, c2, e, s)) - la).max() <= 1e-9


PERIODIC = {
    'hfo2': lambda: C.jittered_hfo2(),
    'sheared': lambda: C.sheared_hfo2(),
    'relabelled': lambda: C.relabelled_hfo2(wrap=True),
    'tiled': lambda: C.tiled_hfo2(),
    'dense_box': lambda: C.dense_box(),
    'sparse_box': lambda: C.sparse_box(),
}


@pytest.mark.parametrize('name', list(PERIODIC))
def test_host_list_equals_brute_force(name):
    pos, cell, _ = PERIODIC[name]()
    pos = C.wrapped(pos, cell)
    for rc in ((5.0, 6.0) if name == 'relabelled' else (5.0,)):
        ei, sh = neighbor_list(pos, cell, rc)
        ej, sj = brute_list(pos, cell, rc)
        assert np.array_equal(ei, ej) and np.array_equal(sh, sj)
    if name == 'dense_box':
        deg = np.bincount(ei[0], minlength=len(pos))
        print(f'dense_box: {ei.shape[1]} edges, degrees {deg.min()}..{deg.max()}')
        assert 256 < deg.max() <= 512            # under the device cap, past one sort tile
    if name == 'sparse_box':
        assert np.array_equal(ei, [[0, 1], [1, 0]])
        assert np.array_equal(sh, [[-1, 0, 0], [1, 0, 0]])
