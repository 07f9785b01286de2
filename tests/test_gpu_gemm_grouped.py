"""e3gnn_gemm_grouped / k_tgemm / k_tgemm_reduce (csrc/tgemm.hip) on the rows
of tests/_gemm_cases.py: the general layouts, per-tile k ranges, both tile
shapes, split-K with immediate and deferred reductions, grouping -- against a
float64 reference gathered through explicit index arrays, through the C ABI's
descriptors directly.

Every row runs alone once (``_alone``); the grouping, deferral and k-range
tests compare further launches with those results bitwise.  The bar is the
project's own for this kernel: 2e-6 of the output's scale (f32 MFMA
accumulation), times sqrt(K / 4096) above 4096 summed rows.
"""
import numpy as np
import pytest

import _gemm_cases as gc
from sevennet_finetuning_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

_STATE = {}


def _dev():
    if 'dev' not in _STATE:
        _STATE['dev'] = gc.Device(_lib.load(), DEV)
    return _STATE['dev']


def _alone(name):
    """the C storage after the row's own launch (made once)"""
    res = _STATE.setdefault('alone', {})
    if name not in res:
        res[name] = _dev().run([name])[0]
    return res[name]


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _same(x, y):
    return np.array_equal(_bits(x), _bits(y))


def _check(name, got):
    """the output block within the bar of the float64 reference; every other
    float of C's storage -- the rows beyond M that the last tile overhangs, the
    columns between the block and the row stride, the floats before the base --
    bitwise as it was"""
    b = gc.built(name)
    ref = b.ref()
    out = got[b.cidx].astype(np.float64)
    err = float(np.abs(out - ref).max()) if ref.size else 0.0
    print(f'{name}: max err {err:.3e}, bar {b.bound():.3e}')
    assert np.isfinite(out).all()
    assert err <= b.bound(), (name, err, b.bound())
    rest = np.ones(len(got), dtype=bool)
    rest[b.cidx.ravel()] = False
    assert _same(got[rest], b.c0[rest]), name


@pytest.mark.parametrize('name', gc.NAMES)
def test_case_matches_fp64(name):
    """Every row of the table against float64, and sentinels around the output.

    kr_hi_beyond_k1 (a k range with hi1 = 1 << 30 > K1 while a second pair
    exists) and kr_tile_split_tail (such a range in a split whose last slice is
    longer than the steps left) failed before tg_tile clamped a tile's ranges
    to its pair's own steps: the load cursor walked past the first pair's last
    segment and, sst being 0, re-read the pair from k = 0."""
    _check(name, _alone(name))
    cs = gc.BY_NAME[name]
    if cs.K == 0 and cs.M:           # no product at all: exact zeros, or C bitwise as it was
        b = gc.built(name)
        got = _alone(name)[b.cidx]
        assert _same(got, b.c0[b.cidx]) if cs.beta else _same(got, np.zeros_like(got))


@pytest.mark.parametrize('name', gc.KR_NAMES)
def test_ranged_product_equals_unranged_bitwise(name):
    """the same operands (zeros outside the ranges) without the table: the
    skipped steps only add exact zeros, in the same order.  A range is rounded
    outward to whole k steps, so the steps that remain are the unranged
    product's own; in the split rows the slices are cut from the tile's own
    step sequence, which a range [0, 1 << 30) leaves as it is and the one
    tight range shortens to steps that lie in ONE slice of the unranged
    product (test_gemm_cases_host.py) -- a range spanning several unranged
    slices would group the same terms into other partial sums."""
    got = _dev().run([name], ranged=False)[0]
    assert _same(got, _alone(name))


@pytest.mark.parametrize('name', gc.KR_NAMES)
def test_empty_ranges(name):
    """tiles whose ranges are empty in both pairs: beta 1 leaves C bitwise
    untouched, beta 0 overwrites NaN with 0 -- unsplit (the tile returns early
    or stores zeros) and split (zero slabs through k_tgemm_reduce)"""
    b = gc.built(name)
    cs = b.case
    tab, sm = b.krtab, cs.kr[1]
    got = _alone(name)
    n_empty = 0
    for tm in range(-(-cs.M // 64)):
        for tn in range(-(-cs.N // 64)):
            lo1, hi1, lo2, hi2 = tab[tm * sm + tn]
            if hi1 > lo1 or (cs.K2 and hi2 > lo2):
                continue
            n_empty += 1
            ix = b.cidx[64 * tm:64 * tm + 64, 64 * tn:64 * tn + 64]
            if cs.beta:
                assert _same(got[ix], b.c0[ix]), (tm, tn)
            else:
                assert np.isnan(b.c0[ix]).all() and _same(got[ix], np.zeros_like(got[ix])), (tm, tn)
    assert n_empty > 0 or name == 'kr_hi_beyond_k1'


def test_twelve_problem_launch_equals_single_launches():
    """twelve problems of one launch (both tile shapes, split and unsplit, an
    m = 0 problem in the middle): every output bitwise the problem's own launch"""
    outs = _dev().run(gc.GROUP)
    for name, got in zip(gc.GROUP, outs):
        assert _same(got, _alone(name)), name
    # and without the m = 0 neighbour
    rest = [n for n in gc.GROUP if gc.BY_NAME[n].M]
    for name, got in zip(rest, _dev().run(rest)):
        assert _same(got, _alone(name)), name


def test_deferred_reductions_equal_immediate():
    """E3GNN_GEMM_DEFER_REDUCE + e3gnn_gemm_reduce on every split row (layouts,
    k ranges, two pairs): bitwise the immediate result, and a second run
    bitwise the first"""
    names = gc.SPLIT_NAMES
    assert len(names) <= 12
    for rep in range(2):
        outs = _dev().run(names, defer=True)
        for name, got in zip(names, outs):
            assert _same(got, _alone(name)), (name, rep)
    for name, got in zip(names, _dev().run(names)):
        assert _same(got, _alone(name)), name


def test_thirty_three_deferred_problems_in_one_reduce_call():
    """33 split problems deferred over three launches, reduced by one
    e3gnn_gemm_reduce call: one more than a reduction launch holds
    (TG_MAX_RED = 32), so the call launches twice"""
    names = [f'small{i}' for i in range(gc.N_SMALL)]
    launches = [names[0:12], names[12:24], names[24:]]
    now = _dev().run_many(launches)
    later = _dev().run_many(launches, defer=True)
    again = _dev().run_many(launches, defer=True)
    for ln, a, b, c in zip(launches, now, later, again):
        for name, x, y, z in zip(ln, a, b, c):
            _check(name, x)
            assert _same(x, y) and _same(y, z), name
