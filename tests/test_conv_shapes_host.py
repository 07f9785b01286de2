"""Conditions on the launch-shape problems of _conv_shapes.py (no GPU): each
centre count gives the split it is listed for, each graph holds every degree
class and edges in the first and the last workgroup, a dropped edge would show
far above the GPU test's bar, and the restated wave -> edge mapping of the
backward kernels visits every edge exactly once."""
import numpy as np
import pytest
import torch

import _conv_shapes as cs
from _conv_cpu import CpuConvBackend

CASES = [(kind, n) for kind in (0, 1, 2) for n in cs.NS]


@pytest.fixture(scope='module', params=CASES, ids=lambda c: f'kind{c[0]}-n{c[1]}')
def case(request):
    """one problem per (kind, n), shared by the tests of that pair"""
    kind, n = request.param
    return (kind, n) + cs.problem(kind, n, seed=kind)


def test_table_splits_and_remainders():
    assert [cs.splits(n) for n in cs.NS] == [(s, s2) for _, s, s2 in cs.TABLE]
    assert cs.NS == [1100, 2305, 6553, 8191, 8192, 10922, 16383, 16385, 32769]
    for n in (6553, 16385, 32769):
        assert n % 4 != 0
    splits = {s for _, s, _ in cs.TABLE}
    assert any(s % 2 for s in splits if 1 < s < 32)          # an odd split
    assert any(s2 % 2 and s2 > 1 for _, _, s2 in cs.TABLE)   # an odd split2
    assert any(s > 1 and s2 == 1 for _, s, s2 in cs.TABLE)   # two-edge step at split2 = 1
    assert 32768 // cs.NS[-1] == 0                           # the clamp acts


def test_graph_conditions(case):
    kind, n, split, split2, center, nbr, (h, Y, w), g, probe = case
    assert (split, split2) == cs.splits(n) == {r[0]: r[1:] for r in cs.TABLE}[n]
    assert np.all(np.diff(center) >= 0) and nbr.min() >= 0 and nbr.max() < n
    deg = np.bincount(center, minlength=n)
    assert set(cs.degree_menu(split, split2)) <= set(deg[deg > 0].tolist())
    assert deg[0] > 0 and deg[n - 1] == 2 * split + 1
    assert np.all(deg[:4] > 0) and np.all(deg[n - 4:] > 0)
    assert int((deg > 0).sum()) == cs.N_BUSY
    assert len(center) <= 9000
    dx, dw, dm = cs.dims(kind)
    assert h.shape == (n, dx) and w.shape == (len(center), dw) and g.shape == (n, dm)
    assert [p.shape for p in probe] == [h.shape, Y.shape, w.shape]


def test_a_dropped_edge_cannot_hide(case):
    """The fp64 double with every edge as its own centre gives the per-edge
    messages; the smallest of them is at least 5e-3 of the aggregate's max
    magnitude: 250 times the 2e-5 bar of test_gpu_conv_shapes.py."""
    kind, n, _, _, center, nbr, (h, Y, w), _, _ = case
    cpu = CpuConvBackend()
    T = lambda a: torch.tensor(a, dtype=torch.float64)   # noqa: E731

    class G:
        pass
    per_edge, whole = G(), G()
    per_edge.n_nodes, per_edge.edge_center = len(center), torch.arange(len(center))
    whole.n_nodes, whole.edge_center = n, torch.tensor(center)
    per_edge.edge_nbr = whole.edge_nbr = torch.tensor(nbr)
    msg = cpu.forward(kind, per_edge, T(h), T(Y), T(w))
    agg = cpu.forward(kind, whole, T(h), T(Y), T(w))
    ratio = float(msg.abs().amax(1).min() / agg.abs().max())
    print(f'kind {kind} n {n}: min_e max|msg_e| / max|agg| = {ratio:.3e}')
    assert ratio >= 5e-3


@pytest.mark.parametrize('kind,n', CASES)
def test_mapping_model_visits_every_edge_once(kind, n):
    """cs.wave_visits over the launches of k_tp_bwd and k_tp_bwd_dual: every
    part visits every edge exactly once, and the waves that return at once
    are exactly those the grid rounds up to."""
    center, _ = cs.graph(n, seed=kind)
    row_ptr = cs.row_ptr_of(center, n)
    for launches in (cs.backward_launches(kind, n), cs.dual_launches(kind, n)):
        for split, pairs in launches:
            visits, idle = cs.wave_visits(row_ptr, split, pairs)
            assert visits.shape == (len(pairs), len(center))
            assert np.all(visits == 1), (split, pairs, np.argwhere(visits != 1)[:5])
            waves = n * split * len(pairs)
            assert np.array_equal(idle, np.arange(waves, 4 * ((waves + 3) // 4)))
            assert len(idle) == -waves % 4


def test_mapping_model_notices_a_wrong_offset():
    """The exactly-once count is not vacuous: a two-edge step whose upper
    half sits one edge after the lower one (the forward's pairing) under the
    backward's stride of 2 split2 skips and doubles edges at split2 = 7."""
    n = 2305
    split, split2 = cs.splits(n)
    center, _ = cs.graph(n, 0)
    row_ptr = cs.row_ptr_of(center, n)
    good, _ = cs.wave_visits(row_ptr, split2, (2,))
    assert np.all(good == 1)
    # split2 waves per centre striding 2 split2, but each wave's halves one
    # edge apart: the model of a different (wrong) kernel
    wg = np.arange(n * split2)
    c, k0 = wg // split2, wg % split2
    visits = np.zeros(len(center), dtype=np.int64)
    for s in range(int(np.diff(row_ptr).max()) // split2 + 1):
        for q in (0, 1):
            e = row_ptr[c] + k0 + 2 * s * split2 + q
            m = e < row_ptr[c + 1]
            np.add.at(visits, e[m], 1)
    assert np.any(visits != 1)
