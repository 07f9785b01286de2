"""Problems for the fine-tune step's grouped GEMM (csrc/tgemm.hip,
e3gnn_gemm_grouped) -- TEST INFRASTRUCTURE; importable without a GPU.

``CASES`` is the one table: each row names the path of k_tgemm /
k_tgemm_reduce it is there to hit, the tile shape (32 or 64) tg_add must choose
for it and the split count tg_splits must request.  tests/
test_gemm_cases_host.py checks those columns (and every other condition the
rows rely on) against the library's host code and a restatement of tg_add;
tests/test_gpu_gemm_grouped.py runs the rows on the device.

``Built`` turns a row into float32 storages with every operand at a non-zero
element offset of a larger storage (row strides wider than the block, as the
model's column slices are), fills ``_lib.GemmDesc`` / ``_lib.GemmLayouts``
directly (the C ABI is under test, not train_explicit._Gemms) and holds the
float64 reference.  The reference gathers the operands through explicit index
arrays from the header's formula

    X[(i / rep) * ld + (i % rep) * rs + (k % ks) * kst + (k / ks) * sst]

and scatters alpha * product (+ beta * C) to
c[(m / crep) * ldc + (m % crep) * crs + n * cns]; it shares no code with
_Gemms._lay_view.  Operand entries outside a tile's k range are zero in the
storage, so the reference of a k-range row is the plain product.
"""
import ctypes
from collections import namedtuple

import numpy as np

# element strides of one operand (e3gnn_gemm_layout)
Lay = namedtuple('Lay', 'ld kst sst rep rs ks')
CLay = namedtuple('CLay', 'ldc crep crs cns')
WHOLE = 1 << 30              # "the whole K" as ExplicitStep._kr(grad=) writes it
OFF = {'a': 7, 'b': 11, 'a2': 5, 'b2': 3, 'c': 13}   # element offsets of the operand bases
PAD = 17                     # floats past an operand's last element
C_PAD_ROWS = 70              # rows of sentinel past C's last (a 64-row tile's overhang)


class Case:
    """One problem C = beta C + alpha (op(A1) op(B1) [+ op(A2) op(B2)]).

    plain: (trans_a, trans_b, trans_a2, trans_b2) for the lda / trans_*
    descriptor fields (row strides a little wider than the block), or None for
    the general layouts ``lay`` = {'a': Lay, 'b': Lay[, 'a2', 'b2']} and ``c``.
    kr: (int table [tiles, 4], row-tile stride) or None.  sup: {'a' | 'b' |
    'a2' | 'b2': [(lo, hi) per 64-row (a) / 64-column (b) tile]} -- the k
    support outside which the operand is zeroed; a per-column-tile table zeroes
    B by its own ranges when sup is not given.  cinit 'nan': the output block
    starts as NaN (beta 0 must overwrite it)."""

    def __init__(self, name, path, tile, splits, M, N, K1, K2=0, plain=None, lay=None, c=None,
                 alpha=1.0, beta=0, kr=None, sup=None, cinit='rand'):
        self.name, self.path, self.tile, self.splits = name, path, tile, splits
        self.M, self.N, self.K1, self.K2 = M, N, K1, K2
        self.plain, self.alpha, self.beta, self.kr, self.cinit = plain, alpha, beta, kr, cinit
        if plain is not None:
            ta, tb, ta2, tb2 = plain
            # as gemm_prob reads the plain fields: op(A)(m, k) = X[m][k] or
            # X[k][m]; op(B)(k, n) as element (n, k) = B[k][n] or B[n][k]
            self.ld = {'a': (M + 5) if ta else (K1 + 3), 'b': (K1 + 2) if tb else (N + 6),
                       'a2': (M + 4) if ta2 else (K2 + 5), 'b2': (K2 + 1) if tb2 else (N + 8)}
            kfast = {'a': not ta, 'b': bool(tb), 'a2': not ta2, 'b2': bool(tb2)}
            kk = {'a': K1, 'b': K1, 'a2': K2, 'b2': K2}
            self.lay = {o: (Lay(self.ld[o], 1, 0, 1, 0, kk[o]) if kfast[o] else
                            Lay(1, self.ld[o], 0, 1, 0, kk[o])) for o in ('a', 'b', 'a2', 'b2')}
            self.c = CLay(N + 9, 1, 0, 1)
        else:
            self.lay, self.c = dict(lay), c
        if K2 == 0:
            self.lay.pop('a2', None), self.lay.pop('b2', None)
        self.sup = dict(sup or {})
        if kr is not None and kr[1] == 0 and sup is None:
            t = np.asarray(kr[0])
            self.sup = {'b': [tuple(r) for r in np.minimum(t[:, 0:2], K1)]}
            if K2:
                self.sup['b2'] = [tuple(r) for r in np.minimum(t[:, 2:4], K2)]

    @property
    def K(self):
        return self.K1 + self.K2

    def general(self):
        return self.plain is None

    def segments(self, o):
        K = self.K1 if o in ('a', 'b') else self.K2
        ks = self.lay[o].ks
        return K // ks if K and ks else (1 if K else 0)

    def ops(self):
        """(name, Lay, rows, K) of the operands present"""
        out = [('a', self.lay['a'], self.M, self.K1), ('b', self.lay['b'], self.N, self.K1)]
        if self.K2:
            out += [('a2', self.lay['a2'], self.M, self.K2), ('b2', self.lay['b2'], self.N, self.K2)]
        return out


def op_index(L, rows, K, off=0):
    """[rows, K] element indices of an operand from the header's formula"""
    i = np.arange(rows, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    ks = L.ks if L.ks > 0 else max(K, 1)
    rep = max(L.rep, 1)
    return off + (i // rep) * L.ld + (i % rep) * L.rs + (k % ks) * L.kst + (k // ks) * L.sst


def c_index(c, M, N, off=0):
    m = np.arange(M, dtype=np.int64)[:, None]
    n = np.arange(N, dtype=np.int64)[None, :]
    return off + (m // c.crep) * c.ldc + (m % c.crep) * c.crs + n * c.cns


class Built:
    """A row's storages (float32 numpy, seeded), index arrays and reference."""

    def __init__(self, case, seed=0):
        self.case = case
        rng = np.random.default_rng([seed, sum(map(ord, case.name)), case.M, case.N, case.K])
        self.idx, self.stor = {}, {}
        for o, L, rows, K in case.ops():
            ix = op_index(L, rows, K, OFF[o])
            self.idx[o] = ix
            size = (int(ix.max()) + 1 if ix.size else OFF[o]) + PAD
            self.stor[o] = rng.standard_normal(size).astype(np.float32)
        for o, ranges in case.sup.items():
            if o not in self.idx:
                continue
            ix = self.idx[o]
            for t, (lo, hi) in enumerate(ranges):
                rows = slice(64 * t, min(64 * (t + 1), ix.shape[0]))
                dead = np.ones(ix.shape[1], dtype=bool)
                dead[lo:hi] = False
                self.stor[o][ix[rows][:, dead].ravel()] = 0.0
        self.cidx = c_index(case.c, case.M, case.N, OFF['c'])
        top = int(self.cidx.max()) + 1 if self.cidx.size else OFF['c']
        self.c0 = rng.standard_normal(top + C_PAD_ROWS * case.c.ldc + PAD).astype(np.float32)
        if case.cinit == 'nan':
            self.c0[self.cidx.ravel()] = np.nan
        self.krtab = None if case.kr is None else np.ascontiguousarray(case.kr[0], dtype=np.int32)
        self._ref = None
        self._layouts = None

    def operand(self, o):
        """the operand as a float64 [rows, K] matrix"""
        return self.stor[o].astype(np.float64)[self.idx[o]]

    def ref(self):
        """float64 values of the output block [M, N]"""
        if self._ref is None:
            cs = self.case
            prod = self.operand('a') @ self.operand('b').T
            if cs.K2:
                prod = prod + self.operand('a2') @ self.operand('b2').T
            r = float(np.float32(cs.alpha)) * prod
            if cs.beta:
                r = r + self.c0.astype(np.float64)[self.cidx]
            self._ref = r
        return self._ref

    def bound(self):
        """the project's bar for this kernel (test_gpu_train.py
        test_grouped_gemm_matches_fp64): f32 MFMA accumulation, 2e-6 of the
        output's scale, growing with sqrt(K / 4096)"""
        r = self.ref()
        scale = float(np.abs(r).max()) if r.size else 0.0
        return 2e-6 * scale * max(1.0, self.case.K / 4096) ** 0.5

    def desc(self, ptr, kr_ptr=None):
        """_lib.GemmDesc of the row; ptr(name) = address of storage `name`
        ('a', 'b', 'a2', 'b2', 'c'), kr_ptr the table's address"""
        from sevennet_finetuning_amd import _lib
        cs = self.case
        d = _lib.GemmDesc()
        at = lambda o: ptr(o) + 4 * OFF[o]   # noqa: E731
        d.a, d.b, d.c = at('a'), at('b'), at('c')
        if cs.K2:
            d.a2, d.b2 = at('a2'), at('b2')
        d.m, d.n, d.k, d.k2 = cs.M, cs.N, cs.K1, cs.K2
        d.alpha, d.beta = float(cs.alpha), int(cs.beta)
        if cs.general():
            lay = _lib.GemmLayouts()
            for o, L in cs.lay.items():
                g = getattr(lay, o)
                g.ld, g.kst, g.sst, g.rep, g.rs, g.ks = L
            lay.ldc, lay.crep, lay.crs, lay.cns = cs.c
            self._layouts = lay          # the descriptor holds its address
            d.layout = ctypes.addressof(lay)
        else:
            d.trans_a, d.trans_b, d.trans_a2, d.trans_b2 = cs.plain
            d.lda, d.ldb, d.lda2, d.ldb2 = (cs.ld[o] for o in ('a', 'b', 'a2', 'b2'))
            d.ldc = cs.c.ldc
        if cs.kr is not None and kr_ptr is not None:
            d.krange, d.krange_stride_m = kr_ptr, int(cs.kr[1])
        return d


# ------------------------------------------------- tg_splits / tg_add restated
def tg_splits(M, N, K):
    """csrc/tgemm.hip tg_splits, as plain arithmetic"""
    tiles = -(-M // 64) * -(-N // 64)
    nk = -(-K // 16)
    if tiles >= 512 or nk < 32:
        return 1
    return max(1, min(-(-1024 // tiles), nk // 8, 256))


def settle(case):
    """what tg_add settles for a row: dict(tile, nk1, nk, ksteps, splits)"""
    if case.M == 0 or case.N == 0:
        return dict(tile=case.tile, nk1=0, nk=0, ksteps=1, splits=1)
    req = tg_splits(case.M, case.N, case.K)
    tiles = -(-case.M // 64) * -(-case.N // 64)
    small = tiles * req < 256 and req == 1
    BK = 32 if small else 16

    def steps(o, K):
        if K <= 0:
            return 0
        ks = case.lay[o].ks
        return (K // ks) * -(-ks // BK)
    nk1 = steps('a', case.K1)
    nk = nk1 + steps('a2', case.K2)
    ksteps = max(1, -(-nk // req))
    return dict(tile=32 if small else 64, nk1=nk1, nk=nk, ksteps=ksteps, splits=max(1, -(-nk // ksteps)))


def reduce_loops(splits):
    """which of k_tgemm_reduce's three loops a split count runs: (the
    sixteen-wide, the four-wide, the single)"""
    return (splits >= 16, splits % 16 >= 4, splits % 4 != 0)


# ------------------------------------------------------------------ the table
def _irreps(name, path, tile, splits, d, nodes, N, K, **kw):
    """rows (node, m) of X[node][mul][d] times the m = 0 diagonal of a dense
    weight block, into C[node][mul][d] (ExplicitStep._lin)"""
    dout = N * d + 12            # the dense matrix's row: the block at an offset
    lay = {'a': Lay(K * d + 6, d, 0, d, 1, K), 'b': Lay(d, d * dout, 0, 1, 0, K)}
    return Case(name, path, tile, splits, nodes * d, N, K, lay=lay, c=CLay(N * d + 10, d, 1, d), **kw)


def _segmented(name, path, tile, splits, d, ks, M=24, N=40, second=None, **kw):
    """a linear's weight gradient (ExplicitStep._lin_grad): K = d segments of
    ks rows, u over X[node][in_lo + u d + m], into the m = 0 diagonal of the
    dense gradient; second = (d2, ks2): another such pair"""
    def pair(d, ks):
        return (Lay(d, M * d + 9, 1, 1, 0, ks), Lay(d, N * d + 7, 1, 1, 0, ks))
    lay = dict(zip(('a', 'b'), pair(d, ks)))
    K2 = 0
    if second:
        lay.update(zip(('a2', 'b2'), pair(*second)))
        K2 = second[0] * second[1]
    dout = N * d + 20
    return Case(name, path, tile, splits, M, N, d * ks, K2, lay=lay, c=CLay(d * dout, 1, 0, d), **kw)


def _col_table(rows):
    return (np.array(rows, dtype=np.int32), 0)


def _tile_case(name, path, K, splits, beta, cinit='rand', tile=64, scale=1.0):
    """130 x 130 = A^T B with a per-tile table as _kr(grad=) writes it: row
    tile a holds k in SA[a] only, column tile b in SB[b] only, tile (a, b) is
    empty where they do not meet, [0, 1 << 30) where they do, and (1, 0) the
    tight [300, 350) (one slice of the unranged product, so ranged equals
    unranged bitwise)"""
    f = lambda v: int(v * scale)   # noqa: E731
    SA = [(0, f(400)), (f(300), f(700)), (f(650), K)]
    SB = [(0, f(350)), (f(400), f(640)), (f(700), K)]
    tab = np.zeros((3, 3, 4), dtype=np.int32)
    for a in range(3):
        for b in range(3):
            if max(SA[a][0], SB[b][0]) < min(SA[a][1], SB[b][1]):
                tab[a, b, 1] = WHOLE
    tab[1, 0, :2] = (f(300), f(350))
    return Case(name, path, tile, splits, 130, 130, K, plain=(1, 0, 0, 0), beta=beta, cinit=cinit,
                kr=(tab.reshape(9, 4), 3), sup={'a': SA, 'b': SB})


def _cases():
    out = []
    add = out.append
    # ---- plain layouts
    for ta in (0, 1):
        for tb in (0, 1):
            for beta in (0, 1):
                add(Case(f'plain_{"nt"[ta]}{"nt"[tb]}_b{beta}', 'ragged 33 x 31 x 65, every transpose, alpha, beta',
                         32, 1, 33, 31, 65, plain=(ta, tb, 0, 0), alpha=0.5, beta=beta))
    add(Case('k0_b0', 'K = 0 and K2 = 0, beta 0: exact zeros over NaN', 32, 1, 40, 40, 0, plain=(0, 0, 0, 0),
             cinit='nan'))
    add(Case('k0_b1', 'K = 0 and K2 = 0, beta 1: C untouched', 32, 1, 40, 40, 0, plain=(0, 0, 0, 0), beta=1))
    add(Case('pairs_33_1', 'two plain pairs, K1 = 33 (a masked second step), K2 = 1', 32, 1, 33, 31, 33, 1,
             plain=(0, 1, 0, 1)))
    # ---- irreps rows: rep = d by multiply-high, K below and above one 32-wide step
    for d in (1, 3, 5, 7, 9):
        for K in (24, 40):
            add(_irreps(f'irreps_d{d}_k{K}', f'irreps rows, rep = crep = {d}, K = {K}', 32, 1, d, 13, 20, K))
    add(_irreps('irreps_big', 'irreps rows in the 64 x 64 shape unsplit: 33 x 8 = 264 tiles', 64, 1, 3, 700, 512, 24))
    # transposed use (C = A D^T): k over the output block, b.kst = d, b.ld = d * dout
    add(Case('irreps_trans', 'irreps rows against the transposed weight block (k over the output block)',
             32, 1, 39, 24, 20, lay={'a': Lay(20 * 3 + 6, 3, 0, 3, 1, 20), 'b': Lay(3 * 70, 3, 0, 1, 0, 20)},
             c=CLay(24 * 3 + 10, 3, 1, 3)))
    # bias idiom on the l = 0 problem: every row reads the one element of a ones column
    add(Case('bias', 'second pair a2.ld = 0, ks = 1, K2 = 1 (the bias)', 32, 1, 13, 20, 24, 1,
             lay={'a': Lay(30, 1, 0, 1, 0, 24), 'b': Lay(1, 32, 0, 1, 0, 24),
                  'a2': Lay(0, 1, 0, 1, 0, 1), 'b2': Lay(1, 1, 0, 1, 0, 1)},
             c=CLay(30, 1, 0, 1)))
    # ---- segmented K, unsplit: every segment ends in a masked partial step
    for d in (1, 3, 5, 9):
        add(_segmented(f'seg_d{d}', f'{d} K segments of 50 rows, unsplit, beta 1', 32, 1, d, 50, beta=1))
    # ---- segmented K, split: the three loops of k_tgemm_reduce
    add(_segmented('seg_split22', '5 x 601: 23 requested, 22 settled = 16 + 4 + 2 (all three loops)',
                   64, 23, 5, 601, beta=1))
    add(_segmented('seg_split7', '3 x 300: 7 splits = 4 + 3 (four-wide loop and singles)', 64, 7, 3, 300, beta=1))
    add(_segmented('seg_split4', '1 x 520: the minimum split count, 4', 64, 4, 1, 520, beta=1))
    add(_irreps('irreps_split', 'irreps rows split: the reduction\'s crep = 3 store', 64, 4, 3, 13, 20, 600))
    add(_segmented('seg_two_pairs', '3 x 115 and 5 x 75 split: a slice contains the switch, others start in pair 2',
                   64, 5, 3, 115, second=(5, 75), beta=1))
    # ---- k ranges (plain layouts)
    col = [[5, 77, 10, 61], [0, 0, 40, 70], [0, 0, 0, 0], [37, 99, 7, 45]]
    for beta, cinit in ((0, 'nan'), (1, 'rand')):
        add(Case(f'kr_col_b{beta}', 'per-column-tile ranges on 32 x 32 tiles (the hull\'s entry), kb2 > 0, '
                 'a tile empty in pair 1, a tile empty in both', 32, 1, 70, 200, 100, 70,
                 plain=(0, 0, 0, 1), beta=beta, cinit=cinit, kr=_col_table(col)))
    add(_tile_case('kr_tile_split', 'per-tile table, split: empty tiles and [0, 1 << 30)', 1000, 7, 1))
    add(_tile_case('kr_tile_split_nan', 'per-tile table, split, beta 0 over NaN', 1000, 7, 0, 'nan'))
    add(_tile_case('kr_tile_split_tail', 'per-tile table, split, the last slice longer than the steps left '
                   '(65 steps in 8 slices of 9)', 1040, 8, 1))
    add(_tile_case('kr_tile_unsplit', 'per-tile table on 32 x 32 tiles: entry (tm >> 1) stride + (tn >> 1)',
                   400, 1, 1, tile=32, scale=0.4))
    big = [[0, 48, 0, 20] if t % 4 == 0 else [5, 30, 17, 20] if t % 4 == 1 else [0, 0, 0, 0] if t % 4 == 2
           else [17, 47, 3, 11] for t in range(16)]
    add(Case('kr_big', 'ranges in the 64 x 64 shape unsplit (256 tiles), kb2 > 0', 64, 1, 1024, 1024, 48, 20,
             plain=(0, 0, 0, 0), beta=1, kr=_col_table(big)))
    add(Case('kr_hi_beyond_k1', 'hi1 = 1 << 30 > K1 with a second pair: "to the end of that pair"', 32, 1,
             33, 31, 65, 40, plain=(0, 0, 0, 0), kr=_col_table([[0, WHOLE, 0, WHOLE]])))
    # ---- grouping
    add(Case('m0', 'an m = 0 problem (no tiles)', 32, 1, 0, 40, 33, plain=(0, 0, 0, 0)))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c.name for c in CASES]
KR_NAMES = [c.name for c in CASES if c.kr is not None]
# split rows whose deferred reduction is compared with the immediate one
SPLIT_NAMES = [c.name for c in CASES if c.splits > 1]
# twelve problems of one launch: both tile shapes, split and unsplit, m = 0 in the middle
GROUP = ['plain_nt_b1', 'irreps_d5_k40', 'seg_d5', 'seg_split22', 'irreps_big', 'kr_tile_split', 'm0',
         'kr_col_b1', 'bias', 'seg_two_pairs', 'irreps_split', 'pairs_33_1']
# 33 small split problems, one more than one reduction launch holds (TG_MAX_RED = 32)
N_SMALL = 33


def small_split(i):
    return Case(f'small{i}', '16 x 16 x 512 split four ways', 64, 4, 16, 16, 512, plain=(i % 2, 0, 0, 0),
                beta=i % 2)


_BUILT = {}


def built(name):
    """the row's Built, made once and shared (the tests never write to it)"""
    if name not in _BUILT:
        cs = BY_NAME[name] if name in BY_NAME else small_split(int(name[5:]))
        _BUILT[name] = Built(cs)
    return _BUILT[name]


# ------------------------------------------------------------------- launching
class Device:
    """the rows' storages on a device and launches of them through the C ABI"""

    def __init__(self, lib, dev):
        import torch
        self.lib, self.dev, self.torch = lib, dev, torch
        self.ops = {}

    def _operands(self, name):
        if name not in self.ops:
            b = built(name)
            t = {o: self.torch.from_numpy(s).to(self.dev) for o, s in b.stor.items()}
            if b.krtab is not None:
                t['kr'] = self.torch.from_numpy(b.krtab).to(self.dev)
            self.ops[name] = t
        return self.ops[name]

    def run(self, names, ranged=True, defer=False):
        """one launch of the named rows on fresh copies of their C storages;
        defer: E3GNN_GEMM_DEFER_REDUCE, then e3gnn_gemm_reduce.  Returns the C
        storages (float32 numpy)."""
        return self.run_many([names], ranged, defer)[0]

    def run_many(self, launches, ranged=True, defer=False):
        """several launches (lists of names); deferred: all their split
        problems reduced by ONE e3gnn_gemm_reduce call at the end"""
        from sevennet_finetuning_amd import _lib
        torch, lib = self.torch, self.lib
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        outs, keep, red_d, red_w = [], [], [], []
        for names in launches:
            n = len(names)
            descs = (_lib.GemmDesc * n)()
            cs = []
            for i, nm in enumerate(names):
                b, t = built(nm), self._operands(nm)
                c = torch.from_numpy(b.c0).to(self.dev)
                ptrs = dict(t, c=c)
                descs[i] = b.desc(lambda o: ptrs[o].data_ptr() if o in ptrs else 0,
                                  t['kr'].data_ptr() if ranged and 'kr' in t else None)
                keep.append(b._layouts)
                cs.append(c)
            need = int(lib.e3gnn_gemm_workspace_floats(n, descs))
            ws = torch.empty(max(need, 1), device=self.dev)
            keep.append((ws, descs))
            _lib.check(lib.e3gnn_gemm_grouped_ex(n, descs, ws.data_ptr(), need, 1 if defer else 0, stream))
            off = 0
            for i in range(n):
                w = int(lib.e3gnn_gemm_workspace_floats(1, ctypes.byref(descs[i])))
                if defer and w > 0:
                    red_d.append(descs[i])
                    red_w.append(ws.data_ptr() + 4 * off)
                off += w
            outs.append(cs)
        if defer and red_d:
            arr = (_lib.GemmDesc * len(red_d))(*red_d)
            wsp = (ctypes.c_void_p * len(red_w))(*red_w)
            _lib.check(lib.e3gnn_gemm_reduce(len(red_d), arr, wsp, stream))
        torch.cuda.synchronize(self.dev)
        return [[c.cpu().numpy() for c in cs] for cs in outs]
