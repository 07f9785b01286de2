"""Conditions on tests/_gemm_cases.py, and the argument refusals of
e3gnn_gemm_grouped that come before any launch -- no GPU needed.

The device tests (tests/test_gpu_gemm_grouped.py) are only as good as the
table: a row that claims to run split through the 16-wide reduction loop but
settles on six splits tests nothing.  So every column and every property a row
relies on is recomputed here, from the library's own host code
(e3gnn_gemm_workspace_floats: tg_splits, no HIP call) and from a restatement
of tg_add's arithmetic (_gemm_cases.settle).
"""
import ctypes

import numpy as np
import pytest
import torch

import _gemm_cases as gc
from sevennet_finetuning_amd import _lib

ARG = 1   # E3GNN_ERR_ARG
FAKE = 1 << 20   # an address that is never dereferenced: the checks come first


def _fake_desc(b, kr=True):
    return b.desc(lambda o: FAKE, FAKE if kr else None)


@pytest.mark.parametrize('name', gc.NAMES + ['small0', 'small1'])
def test_operands_lie_inside_their_storages(name):
    b = gc.built(name)
    for o, ix in b.idx.items():
        if ix.size:
            assert ix.min() >= gc.OFF[o] > 0 and ix.max() < len(b.stor[o]), o
    if b.cidx.size:
        assert b.cidx.min() >= gc.OFF['c'] > 0 and b.cidx.max() < len(b.c0)
        assert len(np.unique(b.cidx)) == b.cidx.size          # C's layout never aliases itself
        # room for sentinels behind the block: a 64-row tile's overhang past M
        assert len(b.c0) - b.cidx.max() > 64 // b.case.c.crep * b.case.c.ldc
    # operands carved out with row strides wider than the block
    cs = b.case
    if cs.plain is not None and cs.K1:
        assert cs.ld['a'] > (cs.M if cs.plain[0] else cs.K1) and cs.ld['b'] > (cs.K1 if cs.plain[1] else cs.N)
        assert cs.c.ldc > cs.N


def test_outputs_of_one_launch_do_not_overlap():
    """every row owns its C storage (Device.run_many copies Built.c0 per
    problem), so the problems of the twelve-problem launch and of the 33-problem
    reduce cannot overlap; the launch list itself is what the issue asks for"""
    assert len(gc.GROUP) == 12 and len(set(gc.GROUP)) == 12
    st = [gc.settle(gc.BY_NAME[n]) for n in gc.GROUP]
    cs = [gc.BY_NAME[n] for n in gc.GROUP]
    assert {s['tile'] for s, c in zip(st, cs) if c.M} == {32, 64}
    assert any(s['splits'] > 1 for s in st) and any(s['splits'] == 1 and c.M for s, c in zip(st, cs))
    mid = [i for i, c in enumerate(cs) if c.M == 0]
    assert mid and 0 < mid[0] < 11
    assert any(c.M and c.tile == 64 and c.splits == 1 for c in cs)       # 64 x 64 unsplit beside the rest
    assert gc.N_SMALL == 33   # one past TG_MAX_RED = 32 (csrc/tgemm.h)


@pytest.mark.parametrize('name', [c.name for c in gc.CASES if c.general()])
def test_index_reference_equals_lay_torch(name):
    """the index-formula reference against train_explicit._Gemms._lay_torch
    (the torch fallback of the same layouts) on float64 copies: 1e-12 relative"""
    from sevennet_finetuning_amd.train_explicit import _Gemms
    b = gc.built(name)
    cs = b.case
    lay = _lib.GemmLayouts()
    for o, L in cs.lay.items():
        g = getattr(lay, o)
        g.ld, g.kst, g.sst, g.rep, g.rs, g.ks = L
    lay.ldc, lay.crep, lay.crs, lay.cns = cs.c
    t = {o: torch.from_numpy(s.astype(np.float64)) for o, s in b.stor.items()}
    c = torch.from_numpy(np.nan_to_num(b.c0.astype(np.float64)))
    gm = _Gemms.__new__(_Gemms)
    A2 = (t['a2'], gc.OFF['a2']) if cs.K2 else None
    B2 = (t['b2'], gc.OFF['b2']) if cs.K2 else None
    gm._lay_torch(cs.M, cs.N, cs.K1, (c, gc.OFF['c']), (t['a'], gc.OFF['a']), (t['b'], gc.OFF['b']), lay,
                  A2, B2, cs.K2, float(np.float32(cs.alpha)), cs.beta)
    got = c.numpy()
    ref = b.ref()
    assert np.abs(got[b.cidx] - ref).max() <= 1e-12 * np.abs(ref).max()
    rest = np.ones(len(got), dtype=bool)
    rest[b.cidx.ravel()] = False
    assert np.array_equal(got[rest], b.c0.astype(np.float64)[rest])


@pytest.mark.parametrize('name', gc.KR_NAMES)
def test_ranges_cover_every_nonzero_of_their_tile(name):
    """per 64 x 64 tile and pair: a k at which some row of the tile's A and
    some column of the tile's B are both nonzero lies inside the tile's range
    (hi beyond K: to the pair's end); and the row has ranges that exclude
    something, or the table would not be read to any effect"""
    b = gc.built(name)
    cs = b.case
    tab, sm = b.krtab, cs.kr[1]
    tn_all = -(-cs.N // 64)
    assert len(tab) == (-(-cs.M // 64) * tn_all if sm else tn_all) and sm in (0, tn_all)
    excluded = 0
    for pair, (oa, ob, K) in enumerate((('a', 'b', cs.K1), ('a2', 'b2', cs.K2))):
        if not K:
            continue
        A, B = b.operand(oa) != 0, b.operand(ob) != 0
        for tm in range(-(-cs.M // 64)):
            for tn in range(tn_all):
                live = A[64 * tm:64 * tm + 64].any(0) & B[64 * tn:64 * tn + 64].any(0)
                lo, hi = tab[tm * sm + tn, 2 * pair:2 * pair + 2]
                inside = np.zeros(K, dtype=bool)
                inside[lo:min(hi, K)] = True
                assert not (live & ~inside).any(), (pair, tm, tn)
                excluded += int((~inside).sum())
    assert excluded > 0 or name == 'kr_hi_beyond_k1'


@pytest.mark.parametrize('name', gc.NAMES + ['small0', 'small1'])
def test_split_and_tile_columns(name):
    """the requested split count is the library's (e3gnn_gemm_workspace_floats
    of the one problem / (m n): tg_splits, no HIP call), the restated tg_splits
    agrees with it, and the tile-shape column follows tg_add's rule: 32 x 32 if
    and only if unsplit and under 256 tiles of 64 x 64"""
    lib = _lib.load()
    b = gc.built(name)
    cs = b.case
    d = _fake_desc(b)
    w = int(lib.e3gnn_gemm_workspace_floats(1, ctypes.byref(d)))
    if cs.M == 0:
        assert w == 0
        return
    req = w // (cs.M * cs.N) if w else 1
    assert w == (req * cs.M * cs.N if req > 1 else 0)
    assert req == cs.splits == gc.tg_splits(cs.M, cs.N, cs.K)
    tiles = -(-cs.M // 64) * -(-cs.N // 64)
    assert cs.tile == (32 if req == 1 and tiles < 256 else 64) == gc.settle(cs)['tile']


def test_paths_named_in_the_table_are_reached():
    """Every path a row is there for, computed from the row.  tg_add settles
    ksteps = ceil(nk / requested) and splits = ceil(nk / ksteps), nk the k
    steps of 16 with every segment padded to whole steps:

      seg_split22    5 x ceil(601 / 16) = 190 steps, 23 requested: ksteps 9,
                     splits 22 = 16 + 4 + 2 -- all three loops of k_tgemm_reduce
      seg_split7     3 x 19 = 57 steps, 7 requested: ksteps 9, splits 7 = 4 + 3
      seg_split4     33 steps, 4 requested: ksteps 9, splits 4 (the four-wide loop alone)
      seg_two_pairs  3 x 8 + 5 x 5 = 24 + 25 steps, 5 requested: ksteps 10,
                     slices [0,10) [10,20) [20,30) [30,40) [40,49): [20,30)
                     contains the switch at step 24, [30,40) starts at step 6
                     of the second pair (segment 1), [40,49) in segment 3
      kr_tile_split_tail  65 steps, 8 requested: ksteps 9, 8 x 9 = 72 > 65 --
                     the last slice reaches past the steps (a range of
                     [0, 1 << 30) must not carry it on)
    """
    S = {n: gc.settle(gc.BY_NAME[n]) for n in gc.NAMES}
    assert (S['seg_split22']['nk'], S['seg_split22']['ksteps'], S['seg_split22']['splits']) == (190, 9, 22)
    assert gc.reduce_loops(22) == (True, True, True)
    assert (S['seg_split7']['nk'], S['seg_split7']['splits']) == (57, 7) and gc.reduce_loops(7) == (False, True, True)
    assert S['seg_split4']['splits'] == 4 and gc.reduce_loops(4) == (False, True, False)
    splits = [S[n]['splits'] for n in gc.SPLIT_NAMES]
    assert any(s >= 16 and s % 16 for s in splits)                # at least 16 with a remainder
    assert any(5 <= s <= 15 and s % 4 for s in splits)
    assert min(splits) == 4 and all(s > 1 for s in splits)
    seen = [False, False, False]
    for s in splits:
        seen = [a or b for a, b in zip(seen, gc.reduce_loops(s))]
    assert all(seen)
    # the reduction's crep store under a split
    assert gc.BY_NAME['irreps_split'].c.crep == 3 and S['irreps_split']['splits'] > 1
    # two segmented pairs: a slice that contains the switch, one that starts inside the second pair
    tp, cs = S['seg_two_pairs'], gc.BY_NAME['seg_two_pairs']
    assert cs.segments('a') == 3 and cs.segments('a2') == 5 and cs.lay['a'].ks != cs.lay['a2'].ks
    assert (tp['nk1'], tp['nk'], tp['ksteps'], tp['splits']) == (24, 49, 10, 5)
    starts = [s * tp['ksteps'] for s in range(tp['splits'])]
    assert any(j < tp['nk1'] < min(j + tp['ksteps'], tp['nk']) for j in starts)
    sps2 = -(-cs.lay['a2'].ks // 16)
    assert any(j > tp['nk1'] and (j - tp['nk1']) // sps2 > 0 for j in starts)
    # segmented unsplit: every segment ends in a masked partial step of the 32-wide tile
    for d in (1, 3, 5, 9):
        c = gc.BY_NAME[f'seg_d{d}']
        assert c.segments('a') == d and c.lay['a'].ks % 32 and S[c.name]['splits'] == 1 and c.beta == 1
    # irreps rows: every rep the ABI takes, K under and over one 32-wide step
    assert {gc.BY_NAME[f'irreps_d{d}_k{K}'].lay['a'].rep for d in (1, 3, 5, 7, 9) for K in (24, 40)} == {1, 3, 5, 7, 9}
    assert S['irreps_d9_k24']['nk'] == 1 and S['irreps_d9_k40']['nk'] == 2
    big = gc.BY_NAME['irreps_big']
    assert -(-big.M // 64) * -(-big.N // 64) == 264 and S['irreps_big'] ['tile'] == 64
    assert gc.BY_NAME['bias'].lay['a2'] == gc.Lay(0, 1, 0, 1, 0, 1) and gc.BY_NAME['bias'].K2 == 1
    # k ranges: bounds on no step boundary, kb2 > 0 in both tile shapes, empty entries
    col = gc.built('kr_col_b0').krtab
    assert all(v % 16 for v in col[[0, 3]].ravel()) and col[1, 2] // 32 > 0
    assert (col[1, :2] == 0).all() and col[1, 3] > 0 and (col[2] == 0).all()
    assert S['kr_col_b0']['tile'] == 32 and gc.BY_NAME['kr_col_b0'].cinit == 'nan'
    kb = gc.built('kr_big').krtab
    assert S['kr_big']['tile'] == 64 and S['kr_big']['splits'] == 1 and (kb[:, 2] // 16 > 0).any()
    for n in ('kr_tile_split', 'kr_tile_split_nan', 'kr_tile_split_tail', 'kr_tile_unsplit'):
        t = gc.built(n).krtab
        assert gc.BY_NAME[n].kr[1] == 3 and (t[:, 1] == gc.WHOLE).any() and (t[:, 1] == 0).any()
    assert S['kr_tile_split']['splits'] == 7 and S['kr_tile_unsplit']['tile'] == 32
    tl = S['kr_tile_split_tail']
    assert (tl['nk'], tl['ksteps'], tl['splits']) == (65, 9, 8) and tl['ksteps'] * tl['splits'] > tl['nk']
    # the tight range of the per-tile tables lies in one slice of the unranged
    # product, so skipping the rest leaves the order of the sums alone
    for n in ('kr_tile_split', 'kr_tile_split_tail'):
        lo, hi = gc.built(n).krtab[3, :2]
        assert lo // 16 // S[n]['ksteps'] == (hi - 1) // 16 // S[n]['ksteps']
    hb = gc.BY_NAME['kr_hi_beyond_k1']
    assert hb.kr[0][0, 1] > hb.K1 and hb.K2 > 0
    sm = gc.settle(gc.small_split(0))
    assert sm['splits'] == 4


# ------------------------------------------------------------------ refusals
def _call(descs, ws=None, ws_floats=0):
    lib = _lib.load()
    arr = (_lib.GemmDesc * len(descs))(*descs)
    rc = lib.e3gnn_gemm_grouped(len(descs), arr, ws, ws_floats, None)
    return rc, lib.e3gnn_last_error()


def _lay_desc(K=48, K2=0, over=None):
    """a small general-layout problem; over: {(operand, field): value}"""
    lay = {'a': gc.Lay(60, 1, 0, 1, 0, K), 'b': gc.Lay(60, 1, 0, 1, 0, K)}
    if K2:
        lay.update(a2=gc.Lay(60, 1, 0, 1, 0, K2), b2=gc.Lay(60, 1, 0, 1, 0, K2))
    c = gc.CLay(40, 1, 0, 1)
    for (o, f), v in (over or {}).items():
        if o == 'c':
            c = c._replace(**{f: v})
        else:
            lay[o] = lay[o]._replace(**{f: v})
    return gc.Built(gc.Case('refused', '', 32, 1, 16, 16, K, K2, lay=lay, c=c))


def test_refusals_come_before_any_launch():
    """fake pointers throughout: a call that got as far as a launch would
    fault, a refused one returns E3GNN_ERR_ARG with a message"""
    ok = gc.built('plain_nn_b0')
    rc, msg = _call([_fake_desc(ok)] * 13)
    assert rc == ARG and b'problems' in msg
    d = _fake_desc(ok)
    d.beta = 2
    rc, msg = _call([d])
    assert rc == ARG and b'beta' in msg
    # a workspace one float short (and none at all)
    sp = gc.built('seg_split4')
    d = _fake_desc(sp)
    need = int(_lib.load().e3gnn_gemm_workspace_floats(1, ctypes.byref(d)))
    assert need == 4 * 24 * 40
    for ws, n in ((ctypes.c_void_p(FAKE), need - 1), (None, need)):
        rc, msg = _call([d], ws, n)
        assert rc == ARG and b'workspace' in msg
    # K not whole segments; ten segments; rep and crep of 10; a.ks != b.ks
    bad = [_lay_desc(K=48, over={('a', 'ks'): 20, ('b', 'ks'): 20}),
           _lay_desc(K=50, over={('a', 'ks'): 5, ('b', 'ks'): 5, ('a', 'sst'): 1, ('b', 'sst'): 1}),
           _lay_desc(over={('a', 'rep'): 10}), _lay_desc(over={('b', 'rep'): 10}), _lay_desc(over={('c', 'crep'): 10}),
           _lay_desc(K=48, over={('a', 'ks'): 24}),
           _lay_desc(K=48, K2=48, over={('a2', 'ks'): 24})]
    for b in bad:
        rc, msg = _call([_fake_desc(b)])
        assert rc == ARG and msg, b.case.lay
    # (nine segments and rep = crep = 9, the last accepted, run on the device:
    # seg_d9 and irreps_d9_* of the table)


def test_krange_with_several_segments_is_refused():
    """krange counts k rows, the kernel k steps, and segments are padded to
    whole steps: with more than one segment in either pair the two disagree,
    so the combination is refused (include/e3gnn.h at krange)"""
    tab = (np.array([[0, gc.WHOLE, 0, gc.WHOLE]], dtype=np.int32), 0)
    seg = {('a', 'ks'): 24, ('b', 'ks'): 24, ('a', 'sst'): 1, ('b', 'sst'): 1}
    seg2 = {('a2', 'ks'): 24, ('b2', 'ks'): 24}
    for K2, over in ((0, seg), (48, seg), (48, seg2)):
        b = _lay_desc(K=48, K2=K2, over=over)
        b.case.kr = tab
        rc, msg = _call([_fake_desc(b)])
        assert rc == ARG and b'krange' in msg and b'segment' in msg
        assert _lib.load().e3gnn_gemm_reduce(1, ctypes.byref(_fake_desc(b)), (ctypes.c_void_p * 1)(FAKE), None) == ARG
    # one segment per pair with a layout and a table stays accepted
    b = _lay_desc(K=48, K2=48)
    b.case.kr = tab
    d = _fake_desc(b)
    d.m = 0
    assert _call([d])[0] == 0
