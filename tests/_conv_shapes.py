"""Convolution problems at every centre-count launch shape of csrc/tp.hip
(TEST INFRASTRUCTURE; importable without a GPU).

The training convolutions choose their launch geometry from the number of
centres alone:

    tp_fwd_impl        n < 8192: k_tp_fwd_split, else k_tp_fwd
    tp_bwd_impl        split  = max(1, min(32, 32768 // n)) waves per centre,
    tp_bwd_dual_impl   wave k0 taking the centre's edges k0, k0 + split, ...
    tp_bwd_dual_impl   (middle block, 32-channel part) split2 = max(1, split // 2)
                       waves per centre on a grid of its own, two edges per
                       wave step: lanes 32..63 at an edge offset of split2
    every backward     grid = ceil(waves / 4): the last workgroup may hold waves
                       past the last centre (`if (c >= n_centers) return`)

``TABLE`` lists the centre counts the tests run, ``problem`` builds a sparse
graph of that many centres (the fp64 reference costs time per edge, the launch
shape does not depend on the edges), and ``wave_visits`` restates the
wave -> edge mapping for the host test.  The splits here are recomputed from
the formula as plain arithmetic, never read from the library.
"""
import numpy as np

from _conv_cpu import KINDS

# n, split, split2: the line of tp.hip the centre count is there for
TABLE = [
    (1100, 29, 14),    # split 29: tp_bwd_impl / tp_bwd_dual_impl min(32, .) no longer acts; odd split
    (2305, 14, 7),     # split 14, split2 7: odd split2 in the dual's two-edge launch
    (6553, 5, 2),      # split 5: small odd split; n = 1 mod 4, a partly idle last workgroup
    (8191, 4, 2),      # split 4: the last n of `n_centers < 8192` (k_tp_fwd_split)
    (8192, 4, 2),      # split 4: the first n of k_tp_fwd
    (10922, 3, 1),     # split 3, split2 1: two-edge step at stride 2, offset 1, under split > 1
    (16383, 2, 1),     # split 2, split2 = max(1, 1) = 1
    (16385, 1, 1),     # split 1: k_tp_bwd_dual one wave per centre and part; n = 1 mod 4
    (32769, 1, 1),     # 32768 // n == 0: the max(1, .) clamp
]
NS = [row[0] for row in TABLE]
N_BUSY = 250

_DIMS = {}


def dims(kind):
    """(dx, dw, dm) of a training kind, from the oracle's instruction list"""
    if not _DIMS:
        from _conv_cpu import CpuConvBackend
        _DIMS.update(CpuConvBackend().dims)
    return _DIMS[kind]


def splits(n):
    split = max(1, min(32, 32768 // n))
    return split, max(1, split // 2)


def degree_menu(split, split2):
    menu = {1, 2, 3, 5, split - 1, split, split + 1, 2 * split + 1, 2 * split2 + 1,
            4 * split + 3, 70}
    return sorted(d for d in menu if d > 0)


def graph(n, seed):
    """(center, nbr) of a sparse graph of n centres: N_BUSY busy ones, always
    0..3 and n-4..n-1 (edges in the first and the last workgroup of every
    grid), degrees from degree_menu in equal shares, centre n-1 with
    2 split + 1 edges, every other centre without edges; neighbours uniform
    over all n nodes."""
    assert n >= N_BUSY + 8
    split, split2 = splits(n)
    rng = np.random.default_rng(seed)
    ends = np.r_[0:4, n - 4:n]
    busy = np.sort(np.r_[ends, 4 + rng.choice(n - 8, N_BUSY - len(ends), replace=False)])
    menu = degree_menu(split, split2)
    deg = np.zeros(n, dtype=np.int64)
    deg[busy] = rng.permutation(np.resize(menu, N_BUSY))
    deg[n - 1] = 2 * split + 1
    center = np.repeat(np.arange(n), deg)
    nbr = rng.integers(0, n, len(center))
    return center, nbr


def problem(kind, n, seed):
    """(split, split2, center, nbr, (h, Y, w), g, probe): graph(n, seed) with
    N(0, 1) operands, cotangent and probes (as test_gpu_train._problem)."""
    assert kind in KINDS
    split, split2 = splits(n)
    center, nbr = graph(n, seed)
    rng = np.random.default_rng([seed, kind, n])
    e = len(center)
    dx, dw, dm = dims(kind)
    h = rng.normal(size=(n, dx))
    Y = rng.normal(size=(e, 9))
    w = rng.normal(size=(e, dw))
    g = rng.normal(size=(n, dm))
    probe = [rng.normal(size=(n, dx)), rng.normal(size=(e, 9)), rng.normal(size=(e, dw))]
    return split, split2, center, nbr, (h, Y, w), g, probe


def row_ptr_of(center, n):
    return np.concatenate([[0], np.cumsum(np.bincount(center, minlength=n))])


def wave_visits(row_ptr, split, pairs):
    """A RESTATEMENT of the wave -> edge mapping of one backward launch, built
    from the comments of k_tp_bwd / k_tp_bwd_dual in csrc/tp.hip -- not the
    kernel: it documents the contract that test_gpu_conv_shapes.py enforces
    on the device.

    ``split`` waves per (centre, part); ``pairs[p]`` edges per wave step of
    part p (1: one edge; 2: lanes 0..31 at the step's edge, lanes 32..63 at an
    offset of ``split``, the step advancing 2 split).  The grid is
    ceil(waves / 4) workgroups of four waves; wave wg is

        part = wg % len(pairs),  rest = wg // len(pairs)
        c = rest // split,  k0 = rest % split          (c >= n: the wave returns)
        step s, half q < pairs[part]:  e = row_ptr[c] + k0 + (s pairs[part] + q) split

    and takes e while e < row_ptr[c + 1].  Returns (visits[part, edge], the
    ids of the waves that return at once)."""
    n, n_edges = len(row_ptr) - 1, int(row_ptr[-1])
    nparts = len(pairs)
    grid = (n * split * nparts + 3) // 4
    wg = np.arange(4 * grid)
    part, rest = wg % nparts, wg // nparts
    c, k0 = rest // split, rest % split
    live = c < n
    part, c, k0 = part[live], c[live], k0[live]
    beg, end = row_ptr[c], row_ptr[c + 1]
    pair = np.asarray(pairs)[part]
    visits = np.zeros((nparts, n_edges), dtype=np.int64)
    max_deg = int(np.diff(row_ptr).max())
    for s in range(max_deg // split + 1):
        for q in range(max(pairs)):
            e = beg + k0 + (s * pair + q) * split
            m = (q < pair) & (e < end)
            np.add.at(visits, (part[m], e[m]), 1)
    return visits, wg[~live]


def backward_launches(kind, n):
    """[(split, pairs)] of tp_bwd_impl's launches for a kind: every part of
    k_tp_bwd takes one edge per wave step."""
    split, _ = splits(n)
    return [(split, (1,))] * (3 if kind == 1 else 1)


def dual_launches(kind, n):
    """[(split, pairs)] of tp_bwd_dual_impl's launches: the 128-channel l1 = 0
    irrep is two parts (64 channels each); the 32-channel l1 = 2 irrep takes
    two edges per step.  The first block has l1 = 0 only; the middle block
    runs three launches, the last on split2; the last block one launch."""
    split, split2 = splits(n)
    if kind == 0:
        return [(split, (1, 1))]
    if kind == 1:
        return [(split, (1, 1)), (split, (1,)), (split2, (2,))]
    return [(split, (1, 1, 1, 2))]
