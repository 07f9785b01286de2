"""The list filter on the device (csrc/pairlist.hip behind e3gnn_plist_* and
``neighbor.ListFilter``) against the numpy restatement of the serial pair
style's host loop (tests/_plist_ref.py): the same edges in the same order, vec
bit for bit.  Needs an MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

from _plist_ref import NEIGHMASK, RC, SPECIAL, SYSTEMS, case, filter_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def flt():
    from sevennet_finetuning_amd.neighbor import ListFilter
    return ListFilter('cuda:0')


def _run(flt, L, x=None, rc=RC):
    flt.set(L['row_atom'], L['cand_ptr'], L['cand'], L['atom_row'], NEIGHMASK)
    return _again(flt, L['x'] if x is None else x, rc)


def _again(flt, x, rc=RC):
    c, nb, v = flt(torch.tensor(np.asarray(x)), rc)
    torch.cuda.synchronize()
    return c.cpu().numpy(), nb.cpu().numpy(), v.cpu().numpy()


def _assert_same(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float32
    assert got[2].shape == (len(got[0]), 3)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.int32), want[2].view(np.int32))


@pytest.mark.parametrize('name', SYSTEMS)
def test_parity_with_the_host_loop(flt, name):
    _, _, L, ref = case(name)
    assert len(ref[0]) > 0
    _assert_same(_run(flt, L), ref)


# ---------------------------------------------------------------- wave shapes
COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 700)


def _cluster():
    """One isolated cluster, atom_row the identity.  Twelve centres 100 A apart,
    each with a cloud of its own: COUNTS candidates uniform in the ball of
    radius 6 (about (5/6)^3 of them inside rc 5), 40 in the shell (5.1, 6) (all
    miss), 40 inside 4.9 (all hit), 700 inside 4.9 (more than 512 hits, the
    cap of the sorted device list).  Every cloud atom is a row too, with three
    candidates: its centre and two atoms of its cloud."""
    rng = np.random.default_rng(11)

    def ball(k, r0, r1):
        v = rng.normal(size=(k, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        return v * rng.uniform(r0 ** 3, r1 ** 3, size=(k, 1)) ** (1.0 / 3.0)

    clouds = [ball(k, 0.0, 6.0) for k in COUNTS] + [ball(40, 5.1, 6.0), ball(40, 0.5, 4.9),
                                                     ball(700, 0.5, 4.9)]
    nc = len(clouds)
    x = [np.array([[100.0 * r, 0.0, 0.0] for r in range(nc)])]
    first = nc
    rows = [None] * nc
    tail = []
    for r, cl in enumerate(clouds):
        ids = np.arange(first, first + len(cl), dtype=np.int32)
        rows[r] = rng.permutation(ids).astype(np.int32)
        x.append(cl + x[0][r])
        for k, a in enumerate(ids):
            tail.append(np.array([ids[(k + 1) % len(ids)], r, ids[(k + 7) % len(ids)]],
                                 dtype=np.int32))
        first += len(cl)
    lists = rows + tail
    cand_ptr = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64)
    n = first
    ident = np.arange(n, dtype=np.int32)
    return dict(x=np.concatenate(x), row_atom=ident, atom_row=ident, cand_ptr=cand_ptr,
                cand=np.concatenate(lists).astype(np.int32), n=n, n_total=n), nc


def test_rows_at_the_wave_boundaries(flt):
    L, nc = _cluster()
    ref = filter_ref(L['x'], L['row_atom'], L['cand_ptr'], L['cand'], NEIGHMASK, L['atom_row'], RC)
    ncand = np.diff(L['cand_ptr'])
    hits = np.bincount(ref[0], minlength=L['n'])
    # the inputs hold what the test is about
    assert ncand[:len(COUNTS)].tolist() == list(COUNTS)
    for r, k in enumerate(COUNTS):
        if k >= 63:
            assert 0 < hits[r] < k                       # hits and misses interleaved
    assert ncand[nc - 3] == 40 and hits[nc - 3] == 0     # all miss
    assert ncand[nc - 2] == 40 and hits[nc - 2] == 40    # all hit
    assert hits[nc - 1] == 700 > 512                     # beyond the sorted list's cap
    assert L['n'] > 4 * 256                              # many blocks
    assert 0.5 < hits[len(COUNTS) - 1] / 700 < 0.65      # about (5/6)^3
    _assert_same(_run(flt, L), ref)


# ------------------------------------------------------------ scan boundaries
SCAN_BLOCK = 1024        # rows per workgroup of the scan of the degrees (csrc/scan.hip)
SCAN_N = (1, 1023, 1024, 1025, 4096, 4097, 1024 * 1024 + 1025)   # 4096: the last one-workgroup n


def _scan_case(n):
    """n rows over n + 1 atoms, the maps the identity.  Atom a < n sits at
    (0.1 (a mod 7), 0, 0), atom n at (100, 0, 0) with graph row 0.  Row t has 0-3
    candidates, each either (t + 1) mod n (a hit) or atom n (a miss)."""
    rng = np.random.default_rng(n)
    x = np.zeros((n + 1, 3))
    x[:n, 0] = 0.1 * (np.arange(n) % 7)
    x[n, 0] = 100.0
    ncand = rng.integers(0, 4, size=n)
    rows = np.repeat(np.arange(n), ncand)
    cand = np.where(rng.integers(0, 2, size=len(rows)) == 1, (rows + 1) % n, n)
    atom_row = np.arange(n + 1, dtype=np.int32)
    atom_row[n] = 0
    return dict(x=x, row_atom=np.arange(n, dtype=np.int32), atom_row=atom_row,
                cand_ptr=np.concatenate([[0], np.cumsum(ncand)]).astype(np.int64),
                cand=cand.astype(np.int32))


@pytest.mark.parametrize('n', SCAN_N)
def test_row_offsets_at_the_scan_boundaries(flt, n):
    """Rows of any degree from 0 to 3, so ``center`` is exactly repeat(arange(n),
    deg): one row, one short of a scan block, a block, one more (the carry of
    the one-workgroup scan), the last n it serves and the first of the scan over
    many workgroups, and more than 1,024 blocks (the carry over the block totals)."""
    L = _scan_case(n)
    ref = filter_ref(L['x'], L['row_atom'], L['cand_ptr'], L['cand'], NEIGHMASK, L['atom_row'], RC)
    deg = np.bincount(ref[0], minlength=n)
    assert np.array_equal(ref[0], np.repeat(np.arange(n), deg))
    if n > 1:                                            # one row has one degree
        assert deg.min() == 0 and deg.max() == 3
    if n == SCAN_N[-1]:
        assert -(-n // SCAN_BLOCK) > 1024
    _assert_same(_run(flt, L), ref)


def test_the_cutoff_is_strict(flt):
    """d^2 = rc^2 exactly is no edge; one ulp inside is."""
    inside = np.nextafter(5.0, 0.0)
    x = np.array([[0, 0, 0], [5, 0, 0], [3, 4, 0], [inside, 0, 0]], dtype=np.float64)
    ident = np.arange(4, dtype=np.int32)
    L = dict(x=x, row_atom=ident, atom_row=ident, cand_ptr=np.array([0, 3, 3, 3, 3], dtype=np.int64),
             cand=np.array([1, 2, 3], dtype=np.int32))
    c, nb, v = _run(flt, L, rc=5.0)
    assert c.tolist() == [0] and nb.tolist() == [3]
    assert v.tolist() == [[np.float32(inside), 0.0, 0.0]]


def test_special_bits_are_masked(flt):
    _, _, L, ref = case('hfo2_resdat')
    assert (L['cand'] & SPECIAL).any()
    plain = dict(L, cand=L['cand'] & NEIGHMASK)
    assert not (plain['cand'] & SPECIAL).any()
    with_bits, without = _run(flt, L), _run(flt, plain)
    _assert_same(with_bits, without)
    _assert_same(with_bits, ref)


def _edge_set(r):
    return set(zip(r[0].tolist(), r[1].tolist(), map(tuple, r[2].view(np.int32).tolist())))


def test_one_set_serves_moving_atoms(flt):
    """set once, then build and fetch with x0, with x1 = x0 + delta (every image
    of an atom moved alike, as LAMMPS moves its ghosts), and with x0 again."""
    _, _, L, ref0 = case('si_rng0_2x2x1')
    delta = np.random.default_rng(4).uniform(-0.4, 0.4, size=(L['n'], 3))
    x1 = L['x'] + delta[L['tag'] - 1]
    ref1 = filter_ref(x1, L['row_atom'], L['cand_ptr'], L['cand'], NEIGHMASK, L['atom_row'], RC)
    # a move that changed nothing would hide a stale buffer
    assert len(ref0[0]) != len(ref1[0])
    s0, s1 = _edge_set(ref0), _edge_set(ref1)
    assert s0 - s1 and s1 - s0
    got0 = _run(flt, L)
    got1 = _again(flt, x1)
    _assert_same(got0, ref0)
    _assert_same(got1, ref1)
    _assert_same(_again(flt, L['x']), got0)


def test_two_builds_are_bitwise_equal(flt):
    _, _, L, _ = case('mixed_2x1x1')
    a = _run(flt, L)
    b = _run(flt, L)
    _assert_same(a, b)
    _assert_same(_again(flt, L['x']), a)
