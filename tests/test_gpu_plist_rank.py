"""The rank-graph filter on the device (k_pl_rank of csrc/pairlist.hip behind
e3gnn_plist_set_rank / _rank_build / _rank_fetch and ``neighbor.ListFilter``)
against the numpy restatement of the parallel pair style's host loop
(tests/_plist_rank_ref.py): the same edges in the same order, the same
first-seen ghost rows, vec bit for bit.  Needs an MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

from _plist_rank_ref import NEIGHMASK, RC, SYSTEMS, classes, rank_case, rank_ref, vacuity

pytestmark = pytest.mark.gpu
KEYS = ('center', 'nbr', 'vec', 'ghost_atom')


@pytest.fixture(scope='module')
def flt():
    from sevennet_finetuning_amd.neighbor import ListFilter
    return ListFilter('cuda:0')


def _again(flt, x, rc=RC):
    out = flt.rank(torch.tensor(np.asarray(x)), rc)
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in KEYS}
    assert out['n_edges'] == len(got['center']) and out['n_ghost'] == len(got['ghost_atom'])
    got['n_ghost'] = out['n_ghost']
    return got


def _run(flt, L, x=None, rc=RC):
    flt.set_rank(L['row_atom'], L['cand_ptr'], L['cand'], L['atom_class'], L['n_class'], NEIGHMASK)
    return _again(flt, L['x'] if x is None else x, rc)


def _ref(L, x=None, rc=RC):
    return rank_ref(L['x'] if x is None else x, L['row_atom'], L['cand_ptr'], L['cand'], NEIGHMASK,
                    L['atom_class'], rc)


def _assert_same(got, want):
    for k in ('center', 'nbr', 'ghost_atom'):
        assert got[k].dtype == np.int32, k
        assert np.array_equal(got[k], want[k]), k
    assert got['vec'].dtype == np.float32 and got['vec'].shape == (len(got['center']), 3)
    assert np.array_equal(got['vec'].view(np.int32), want['vec'].view(np.int32))
    assert got['n_ghost'] == want['n_ghost']


@pytest.mark.parametrize('name', SYSTEMS)
def test_parity_with_the_host_loop(flt, name):
    """The inputs are not vacuous in three of the four ways: ghost atoms sharing
    a row, self-images landing on owned rows, a class whose first two edges sit
    in different rows.  No system has a class without an edge (every atom
    outside the half box has an image within the cutoff of an owned atom in
    cells this small): test_synthetic_rows and test_all_miss hold that."""
    L, ref = rank_case(name)
    v = vacuity(L, ref)
    assert v['shared_row'] and v['self_image'] and v['rows_apart'], v
    assert len(ref['center']) > 0 and ref['n_ghost'] > 0 and L['n'] > 4      # more than one block
    _assert_same(_run(flt, L), ref)


# ---------------------------------------------------------------- wave shapes
COUNTS = (0, 1, 63, 64, 65, 128, 129)


def _synthetic():
    """Owned centres 100 A apart, each with a cloud of ghost atoms of its own as
    candidates, uniform in the ball of radius 6 (hits and misses interleaved;
    a ghost that misses is a class without an edge).  Rows: one per COUNTS
    entry, then
      S   the centre at the origin with ghosts at (5, 0, 0), (3, 4, 0) (d^2 =
          rc^2: out) and one ulp inside (in);
      A   65 candidates, entries 63 and 64 forced hits of one new class (first
          met in lane 63 of the first trip, again in lane 0 of the second);
      B,C the last candidate of B and the first of C forced hits of one new
          class (the last edge of a row, then the first edge of the next).
    Every seventh ghost of the clouds is a self-image: its class is an owned
    row.  ``row_atom`` is a permutation of the owned atoms."""
    rng = np.random.default_rng(23)
    sizes = list(COUNTS) + [3, 65, 40, 40]
    S, A, B, C = (len(COUNTS) + k for k in range(4))
    n = len(sizes)
    row_atom = rng.permutation(n).astype(np.int32)
    centre = np.zeros((n, 3))
    for t in range(n):
        centre[row_atom[t]] = (0.0, 0.0, 0.0) if t == S else (100.0 * (t + 1), 0.0, 0.0)

    def ball(k, r0, r1):
        v = rng.normal(size=(k, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        return v * rng.uniform(r0 ** 3, r1 ** 3, size=(k, 1)) ** (1.0 / 3.0)

    x, tag, cand, cand_ptr = [centre], list(range(1, n + 1)), [], [0]
    first, next_tag = n, n + 1
    for t, k in enumerate(sizes):
        off = ball(k, 0.0, 6.0)
        if t == S:
            off = np.array([[5.0, 0, 0], [3.0, 4.0, 0], [np.nextafter(5.0, 0.0), 0, 0]])
        if t == A:
            off[63:65] = ball(2, 0.5, 4.9)
        if t == B:
            off[-1] = ball(1, 0.5, 4.9)
        if t == C:
            off[0] = ball(1, 0.5, 4.9)
        x.append(off + centre[row_atom[t]])
        tags = np.arange(next_tag, next_tag + k)
        next_tag += k
        tags[np.arange(k) % 7 == 6] = rng.integers(1, n + 1, size=int((np.arange(k) % 7 == 6).sum()))
        if t == A:
            tags[64] = tags[63]
        if t == C:
            tags[0] = tag[-1]                      # B's last ghost
        tag += tags.tolist()
        ids = np.arange(first, first + k, dtype=np.int32)
        ids[1::2] |= np.int32(1 << 30)
        cand.append(ids)
        cand_ptr.append(cand_ptr[-1] + k)
        first += k
    # tags of owned atoms: atom a carries tag a + 1; dense class numbering below
    tag = np.array(tag, dtype=np.int64)
    atom_class, n_class = classes(tag, row_atom, first)
    L = dict(x=np.concatenate(x), tag=tag, row_atom=row_atom,
             cand_ptr=np.array(cand_ptr, dtype=np.int64), cand=np.concatenate(cand).astype(np.int32),
             atom_class=atom_class, n_class=n_class, n=n, n_total=first)
    return L, (S, A, B, C)


def test_synthetic_rows(flt):
    L, (S, A, B, C) = _synthetic()
    ref = _ref(L)
    n, c, nb = L['n'], ref['center'], ref['nbr']
    ncand = np.diff(L['cand_ptr'])
    hits = np.bincount(c, minlength=n)
    # the inputs hold what the test is about
    assert ncand[:len(COUNTS)].tolist() == list(COUNTS)
    for r, k in enumerate(COUNTS):
        if k >= 63:
            assert 0 < hits[r] < k                                  # hits and misses interleaved
    assert hits[S] == 1 and ref['vec'][c == S].tolist() == [[np.float32(np.nextafter(5.0, 0.0)), 0, 0]]
    assert ref['n_ghost'] < L['n_class']                            # classes without an edge
    assert (nb < n).any() and (nb >= n).any()                       # self-images and ghost rows
    # A: entries 63 and 64 are edges of one ghost row that appears nowhere else
    a0 = L['cand_ptr'][A]
    ja, jb = a0 + 63, a0 + 64
    ea = np.flatnonzero(c == A)
    jh = (L['cand'] & NEIGHMASK)[_hit_mask(L)]
    ra = nb[ea][jh[ea] == (L['cand'][ja] & NEIGHMASK)]
    rb = nb[ea][jh[ea] == (L['cand'][jb] & NEIGHMASK)]
    assert len(ra) == 1 and len(rb) == 1 and ra[0] == rb[0] >= n and (nb == ra[0]).sum() == 2
    assert ref['ghost_atom'][ra[0] - n] == (L['cand'][ja] & NEIGHMASK)
    # B, C: the last edge of row B and the first edge of row C share a new ghost row
    eb, ec = np.flatnonzero(c == B), np.flatnonzero(c == C)
    assert ec[0] == eb[-1] + 1 and nb[eb[-1]] == nb[ec[0]] >= n
    assert (nb == nb[ec[0]]).sum() == 2
    assert jh[eb[-1]] == L['n_total'] - 40 - 1 and jh[ec[0]] == L['n_total'] - 40
    assert ref['ghost_atom'][nb[ec[0]] - n] == jh[eb[-1]]
    _assert_same(_run(flt, L), ref)


def _hit_mask(L, x=None, rc=RC):
    x = L['x'] if x is None else x
    rows = np.repeat(np.arange(L['n']), np.diff(L['cand_ptr']))
    j = L['cand'] & NEIGHMASK
    d = x[j] - x[L['row_atom'][rows]]
    return ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2]) < rc * rc


def test_all_miss(flt):
    """No candidate inside the cutoff: no edge, no ghost row, classes left over."""
    x = np.array([[0, 0, 0], [50, 0, 0], [0, 6, 0], [50, 0, 7], [5, 0, 0]], dtype=np.float64)
    L = dict(x=x, row_atom=np.array([1, 0], dtype=np.int32),
             cand_ptr=np.array([0, 1, 4], dtype=np.int64), cand=np.array([3, 4, 2, 1], dtype=np.int32),
             atom_class=np.array([1, 0, 3, 2, 3], dtype=np.int32), n_class=2, n=2, n_total=5)
    got = _run(flt, L)
    assert len(got['center']) == 0 and got['n_ghost'] == 0 and got['vec'].shape == (0, 3)
    _assert_same(got, _ref(L))


# ------------------------------------------------------------ scan boundaries
def _scan_case(n):
    """n rows of 0-3 candidates; n // 2 + 1 ghosts of which ghost g carries the
    class n + g // 2 (two images a class) and sits within 1.2 A of every owned
    atom, and one far ghost (a miss, a class without an edge)."""
    rng = np.random.default_rng(n)
    m = n // 2 + 1
    x = np.zeros((n + m + 1, 3))
    x[:n, 0] = 0.1 * (np.arange(n) % 7)
    x[n:n + m, 0] = 0.05 * (np.arange(m) % 11)
    x[n:n + m, 2] = 1.0
    x[n + m, 0] = 100.0
    ncand = rng.integers(0, 4, size=n)
    total = int(ncand.sum())
    cand = np.where(rng.integers(0, 4, size=total) > 0, n + rng.integers(0, m, size=total), n + m)
    atom_class = np.concatenate([np.arange(n), n + np.arange(m) // 2, [n + (m - 1) // 2 + 1]])
    return dict(x=x, row_atom=np.arange(n, dtype=np.int32), atom_class=atom_class.astype(np.int32),
                n_class=(m - 1) // 2 + 2, n=n, n_total=n + m + 1,
                cand_ptr=np.concatenate([[0], np.cumsum(ncand)]).astype(np.int64),
                cand=cand.astype(np.int32))


@pytest.mark.parametrize('n', (1, 1025, 4096, 4097))
def test_ghost_rows_at_the_scan_boundaries(flt, n):
    """The scan of the first edges per row at one row, past one scan block (the
    carry), the last n of the one-workgroup scan and the first n of the scan
    over many workgroups; ghost rows first met in rows all over the list."""
    L = _scan_case(n)
    ref = _ref(L)
    if n > 1:
        first_rows = ref['center'][np.unique(ref['nbr'], return_index=True)[1]]
        assert first_rows.max() > n // 2 and ref['n_ghost'] > n // 8
        assert ref['n_ghost'] < L['n_class']
    _assert_same(_run(flt, L), ref)


# ------------------------------------------------------------------ contract
@pytest.mark.parametrize('name', ('hfo2_resdat', 'synthetic'))
def test_the_class_numbering_does_not_matter(flt, name):
    """The classes [n, n + n_class) renumbered by a random permutation: every
    output identical, edge_nbr and ghost_atom too (rows come from the order of
    the first edges, never from the class ids)."""
    L = _synthetic()[0] if name == 'synthetic' else rank_case(name)[0]
    n, nc = L['n'], L['n_class']
    perm = np.random.default_rng(5).permutation(nc)
    assert not np.array_equal(perm, np.arange(nc))
    cls = L['atom_class'].copy()
    g = cls >= n
    cls[g] = n + perm[cls[g] - n]
    assert not np.array_equal(cls, L['atom_class'])
    ref = _ref(L)
    _assert_same(_run(flt, dict(L, atom_class=cls)), ref)
    _assert_same(_run(flt, L), ref)


def test_one_set_rank_serves_moving_atoms(flt):
    """set_rank once, then x0, x1 = x0 + delta (every image of an atom moved
    alike, keyed by its tag) and x0 again."""
    L, ref0 = rank_case('si_rng0_2x2x1')
    delta = np.random.default_rng(5).uniform(-0.4, 0.4, size=(int(L['tag'].max()) + 1, 3))
    x1 = L['x'] + delta[L['tag']]
    ref1 = _ref(L, x1)
    # a move that changed nothing would hide a stale buffer
    assert len(ref0['center']) != len(ref1['center'])
    assert not np.array_equal(ref0['ghost_atom'], ref1['ghost_atom'])
    got0 = _run(flt, L)
    got1 = _again(flt, x1)
    _assert_same(got0, ref0)
    _assert_same(got1, ref1)
    _assert_same(_again(flt, L['x']), got0)


def test_two_builds_are_bitwise_equal(flt):
    L, _ = rank_case('mixed_2x1x1')
    a = _run(flt, L)
    b = _run(flt, L)
    _assert_same(a, b)
    _assert_same(_again(flt, L['x']), a)


def test_the_plain_filter_still_works_on_the_handle(flt):
    """A rank build, then set + build + fetch on the same handle: the serial
    style's edges (tests/_plist_ref.py), and a rank fetch is over."""
    from _plist_ref import case
    from sevennet_finetuning_amd._lib import E3GNNError
    L, ref = rank_case('mixed_2x1x1')
    _assert_same(_run(flt, L), ref)
    _, _, P, want = case('mixed_2x1x1')
    flt.set(P['row_atom'], P['cand_ptr'], P['cand'], P['atom_row'], NEIGHMASK)
    c, nb, v = flt(torch.tensor(P['x']), RC)
    torch.cuda.synchronize()
    assert np.array_equal(c.cpu().numpy(), want[0]) and np.array_equal(nb.cpu().numpy(), want[1])
    assert np.array_equal(v.cpu().numpy().view(np.int32), want[2].view(np.int32))
    with pytest.raises(E3GNNError, match='rank_build before set_rank'):
        flt.rank(torch.tensor(P['x']), RC)
    _assert_same(_run(flt, L), ref)
