"""Every interaction block's forward and VJP on the GPU against the fp64 block
oracle (tests/_block_oracle.py), one block at a time, with random N(0,1)
features and random cotangents, measured per irreps entry.  The GPU tests need
an MI355X: ``pytest -m gpu``.

The end-to-end tests see only the energy's own cotangent -- one row per
species, l = 1 and l = 2 parts far below the scalars -- and only the sum of
the five blocks' edge gradients.  Here the segment API drives one block with
any input and any cotangent: ``HipSegmentEngine.unpack`` with an ``arange``
index list writes the feature and gradient buffers in stream order, ``pack``
reads them.  For block t: upload, graph_set, the forwards (x[t] overwritten
just before forward t), readout, the cotangent into grad[t + 1], backward t,
forces with edge_grad.  Compared with the oracle on the same inputs cast to
fp64: the features after the block, dE/dx[t] on all rows (t > 0; block 0
writes none) and the block's own dE/dedge_vec.  One sweep L-1 .. 0 with fresh
cotangents then compares the summed edge_grad (the per-edge accumulators start
from nonzero values), and one sweep runs on the model's real features.

Bars, per irreps entry (``block_errors``):

* forward, every engine: 1e-5, the project's layerwise bar
  (test_gpu_parity.test_layerwise_features_vs_oracle), now per entry;
* backward of the all-f32 arms (v1 kernels, generic engine): 2e-5, the
  project's bar for f32 derivative kernels against fp64 (test_gpu_train.py);
* backward of the fused kernels: 2e-5 + 4 x 2^-16 = 8.1e-5.  The three-product
  forms drop the p1 q1 term, 2^-16 relative to the product of magnitudes
  (DESIGN.md 0c item 1); a gradient entry passes through at most two such
  products (the w recompute feeding dE/dx and dE/dY; dw -> dH2 feeding the MLP
  chain), and the scale is the entry's maximum, not a sum of magnitudes: a
  factor of four, not two.

Graphs: the five of test_gpu_bwd_packed.make_case and the hub graph of
test_gpu_bwd_image.py (an explicit edge list without positions).  A model with
a shorter cutoff gets the edge vectors scaled by cutoff / 5 A; a model without
the graph's species gets them mapped onto its own, round-robin.

Also here: the two halo-overlap contracts of include/e3gnn.h on one rank of a
decomposition (forward part 0 reads only owned rows; the ghost rows of dE/dx
are complete after backward part 0), and e3gnn_halo_pack / e3gnn_halo_unpack
against numpy indexing.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _block_oracle as bo
from _systems import load_manifest_symbols, system

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, 'sevennet_finetuning_amd', 'assets')
SYMS = load_manifest_symbols()
CUTOFF = 5.0
DEV = 'cuda:0'
FWD_BAR = 1e-5
F32_BWD_BAR = 2e-5
FUSED_BWD_BAR = 2e-5 + 4 * 2.0 ** -16
GRAPHS = ('si', 'hfo2', 'stretched', 'cluster', 'odd', 'hub')
# engine -> (deployment, kernels)
ENGINES = {'sn0-fused': ('sn0', 'fused'), 'sn0-v1': ('sn0', 'v1'),
           'c64-fused': ('c64', 'fused'), 'c64-generic': ('c64', 'generic'),
           'c32-fused': ('c32', 'fused'), 'c32-generic': ('c32', 'generic'),
           'bias-fused': ('bias', 'fused'), 'hfo2ex-generic': ('hfo2ex', 'generic')}
FAMILY = {'c64': (64, 1), 'c32': (32, 2)}
SPECIES = ('Hf', 'O', 'Si')


# ------------------------------------------------------------------ cases
_graphs = {}


def graph_of(name):
    """{n, center, nbr, vec, labels}: an edge list sorted by centre and one
    species label per node."""
    if name not in _graphs:
        if name == 'hub':
            from test_gpu_bwd_image import make_graph, types_of
            n, center, nbr, vec = make_graph(143)
            labels = [SYMS[t] for t in types_of(SYMS, n)]
        else:
            from test_gpu_bwd_packed import make_case
            c = make_case(name)
            n, center, nbr, vec, labels = len(c['pos']), c['ei'][0], c['ei'][1], c['vec'], c['symbols']
        _graphs[name] = {'name': name, 'n': n, 'center': np.asarray(center), 'nbr': np.asarray(nbr),
                         'vec': np.asarray(vec, dtype=np.float64), 'labels': list(labels)}
    return _graphs[name]


def types_for(labels, symbols):
    """Species index of every node in a model's species list; labels the model
    lacks are mapped onto its species round-robin (a block test needs distinct
    species, not these ones)."""
    if all(s in symbols for s in labels):
        return np.array([symbols.index(s) for s in labels], dtype=np.int64)
    kinds = sorted(set(labels))
    return np.array([kinds.index(s) % len(symbols) for s in labels], dtype=np.int64)


# 'stretched' keeps its edge list (3-4 edges per centre) with the edges at
# Si's bond length: at 4.7 A they lie in the cutoff's switching region, the
# messages vanish and the convolution-only entries fail ``check_scales``
VEC_SCALE = {'stretched': 0.5}


def vec_for(g, ref):
    """fp32-representable edge vectors inside the model's cutoff."""
    f = VEC_SCALE.get(g['name'], 1.0) * ref.cutoff / CUTOFF
    return (g['vec'] * f).astype(np.float32).astype(np.float64)


def inputs(ref, g, n_local, seed):
    """N(0,1) features entering and cotangents leaving every block, rounded to
    fp32 (the GPU gets the same numbers), from a seeded CPU generator."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda r, d: torch.randn(r, d, generator=gen, dtype=torch.float32).double()  # noqa: E731
    x = [rnd(g['n'], bo.nequip_ref.dim(ref.irreps[t])) for t in range(ref.nlayer)]
    G = [rnd(n_local, bo.nequip_ref.dim(ref.irreps[t + 1])) for t in range(ref.nlayer)]
    G2 = [rnd(n_local, bo.nequip_ref.dim(ref.irreps[t + 1])) for t in range(ref.nlayer)]
    return x, G, G2


class Oracle:
    """The fp64 references of one (deployment, graph): computed once, shared by
    the engines of the deployment, read-only."""

    def __init__(self, ref, g):
        self.ref, self.g = ref, g
        self.types = types_for(g['labels'], ref.symbols)
        self.vec = vec_for(g, ref)
        self.x, self.G, self.G2 = inputs(ref, g, g['n'], seed=len(g['name']) + g['n'])
        self.iso, self.sweep = [], None
        vec = torch.tensor(self.vec)
        total = torch.zeros_like(vec)
        for t in range(ref.nlayer):
            (out, gx, gv), (_, _, gv2) = self.vjps(t, self.x[t], [self.G[t], self.G2[t]])
            self.iso.append((out, gx, gv))
            total += gv2
        self.sweep = total

    def vjps(self, t, x, Gs, n_local=None):
        g = self.g
        return [bo.vjp(self.ref, t, x, self.vec, g['center'], g['nbr'], self.types,
                       g['n'] if n_local is None else n_local, G) for G in Gs]


# ------------------------------------------------------------------ fixtures
def deploy_all(mkdir):
    """name -> deployment directory.  The c64 / c32 three-block models are
    deployed as test_gpu_bwd_image.family_models does and the linear-bias model
    as test_gpu_options_fused does (random biases), all three with
    conv_denominator 1: with e3nn's initial weights and SevenNet-0's 36 the
    convolution carries 1/200 of the self-connection, and the entries that only
    the convolution feeds (block 0's l > 0 outputs, the last block's l > 0
    dE/dx) fail ``check_scales``."""
    from sevennet_finetuning_amd import model_build as mb
    from test_gpu_options_fused import _config, _rewrite
    out = {'sn0': os.path.join(ASSETS, 'sevennet0'), 'hfo2ex': os.path.join(ASSETS, 'hfo2_example')}
    for name, (ch, _) in FAMILY.items():
        out[name] = mkdir(f'blk_{name}')
        mb.deploy_config(mb.sevennet_shaped_config(ch, 3, species=list(SPECIES), avg_num_neigh=1.0),
                         out[name], seed=ch + 3)
    out['bias'] = mkdir('blk_bias')
    mb.deploy_config(dict(_config('sn0_l3', 'bias'), conv_denominator=1.0), out['bias'], seed=7)
    _rewrite(out['bias'], seed=11)
    return out


@pytest.fixture(scope='module')
def deployments(tmp_path_factory):
    return deploy_all(lambda name: str(tmp_path_factory.mktemp(name)))


@pytest.fixture(scope='module')
def refs(deployments):
    from oracle.nequip_ref import NequIPRef
    cache = {}

    def get(dep):
        if dep not in cache:
            cache[dep] = NequIPRef(deployments[dep])
        return cache[dep]
    return get


@pytest.fixture(scope='module')
def oracles(refs):
    cache = {}

    def get(dep, graph):
        if (dep, graph) not in cache:
            cache[dep, graph] = Oracle(refs(dep), graph_of(graph))
        return cache[dep, graph]
    return get


@pytest.fixture(scope='module')
def models(deployments):
    from sevennet_finetuning_amd.model import E3GNNModel
    cache = {}

    def get(dep, kernels):
        key = (dep, kernels == 'generic')
        if key not in cache:
            assert torch.cuda.is_available(), 'GPU tests need a HIP device'
            old = os.environ.get('E3GNN_GENERIC')
            if key[1]:
                os.environ['E3GNN_GENERIC'] = '1'
            try:
                cache[key] = E3GNNModel(deployments[dep], device=DEV)
            finally:
                if key[1]:
                    if old is None:
                        del os.environ['E3GNN_GENERIC']
                    else:
                        os.environ['E3GNN_GENERIC'] = old
            fam = cache[key].family
            assert fam == (-1 if key[1] else {'sn0': 0, 'bias': 0, **{k: v[1] for k, v in FAMILY.items()}}[dep])
        return cache[key]
    return get


WORST = {}


@pytest.fixture(scope='module', autouse=True)
def worst_table():
    """Prints the measured worst case per engine, block and quantity."""
    yield
    if WORST:
        print('\nworst measured error per engine, block and quantity (block_errors, per irreps entry)')
        print(f'{"engine":<16}{"block":>6} {"quantity":<18}{"worst":>10}{"bar":>10}  where')
        for (eng, t, q), (e, bar, where) in sorted(WORST.items()):
            print(f'{eng:<16}{t:>6} {q:<18}{e:>10.2e}{bar:>10.2e}  {where}')


# ------------------------------------------------------------------ driver
class Driver:
    """One graph on a ``HipSegmentEngine``; buffers read and written through
    its pack / unpack with an arange index list (stream order)."""

    def __init__(self, model, g, types, vec, n_local=None, n_interior=0):
        from sevennet_finetuning_amd.parallel import HipSegmentEngine
        self.model, self.eng = model, HipSegmentEngine(model)
        self.n = g['n']
        self.nl = self.n if n_local is None else n_local
        self.E = len(g['center'])
        self.L = model.num_layers
        self.eng.upload(SimpleNamespace(n_local=self.nl, n_ghost=self.n - self.nl,
                                        n_interior=n_interior, types=types, center=g['center'],
                                        nbr=g['nbr'], vec=vec))
        self.idx = torch.arange(self.n, dtype=torch.int32, device=model.device)

    def put(self, kind, t, a, rows=None):
        """Rows ``rows`` (default all) of buffer (kind, t) <- a."""
        idx = self.idx if rows is None else self.idx[rows[0]:rows[1]]
        src = torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(self.model.device)
        assert src.shape == (idx.numel(), self.eng.dim(kind, t)), (src.shape, idx.numel())
        self.eng.unpack(kind, t, idx, src.contiguous(), False)

    def get(self, kind, t):
        out = self.eng.empty(self.n, self.eng.dim(kind, t))
        self.eng.pack(kind, t, self.idx, out)
        return out.cpu().double()

    def cotangent(self, t, G):
        """dE/dx[t + 1] of the owned rows <- G (the ghost rows are not read)."""
        full = torch.zeros(self.n, G.shape[1], dtype=torch.float64)
        full[:self.nl] = G
        self.put('grad', t + 1, full)

    def edge_grad(self):
        from sevennet_finetuning_amd import _lib
        f = torch.empty(max(self.n, 1), 3, device=self.model.device)
        vir = torch.empty(6, device=self.model.device)
        eg = torch.empty(max(self.E, 1), 3, device=self.model.device)
        _lib.check(self.model.lib.e3gnn_forces(self.model._ctx, f.data_ptr(), vir.data_ptr(),
                                               eg.data_ptr(), self.model.stream_handle()))
        return eg[:self.E].cpu().double()

    def isolated(self, t, x, G):
        """(features after block t, dE/dx[t] on all rows or None, the block's
        own dE/dvec) with x[t] <- x and dE/dx[t + 1] <- G."""
        e = self.eng
        e.graph_set()
        for s in range(self.L):
            if s == t:
                self.put('x', t, x)
            e.layer_forward(s)
        out = self.get('x', t + 1)[:self.nl]
        e.readout()
        self.cotangent(t, G)
        e.layer_backward(t)
        eg = self.edge_grad()
        return out, (self.get('grad', t) if t > 0 else None), eg

    def sweep(self, xs, Gs):
        """One backward L-1 .. 0 with x[t] <- xs[t] (None: the model's own
        features) and dE/dx[t + 1] <- Gs[t] per block: (x[t] as used, features
        after every block, dE/dx[t] per block, the summed edge_grad)."""
        e = self.eng
        e.graph_set()
        used, outs = [], []
        for s in range(self.L):
            if xs is not None:
                self.put('x', s, xs[s])
            used.append(self.get('x', s))
            e.layer_forward(s)
            outs.append(self.get('x', s + 1)[:self.nl])
        e.readout()
        gx = [None] * self.L
        for t in reversed(range(self.L)):
            self.cotangent(t, Gs[t])
            e.layer_backward(t)
            if t > 0:
                gx[t] = self.get('grad', t)
        return used, outs, gx, self.edge_grad()


class Judge:
    """Collects block_errors against the bars; one assertion at the end, after
    every figure is printed."""

    def __init__(self, engine, kernels, where):
        self.engine, self.where, self.fail = engine, where, []
        self.bwd_bar = FUSED_BWD_BAR if kernels == 'fused' else F32_BWD_BAR

    def compare(self, t, quantity, got, want, irreps, rows=None):
        if rows is not None:
            got, want = got[rows[0]:rows[1]], want[rows[0]:rows[1]]
        bar = FWD_BAR if quantity.startswith('forward') else self.bwd_bar
        scales = bo.check_scales(want, irreps)
        errs = bo.block_errors(got, want, irreps)
        print(f'{self.engine:<16}{self.where:<12}block {t} {quantity:<18} '
              + ' '.join(f'{e:.2e}' for e in errs) + f'  (bar {bar:.1e}; scales '
              + ' '.join(f'{s:.2e}' for s in scales) + ')')
        key = (self.engine, t, quantity)
        if key not in WORST or max(errs) > WORST[key][0]:
            WORST[key] = (max(errs), bar, self.where)
        if not max(errs) <= bar:
            self.fail.append((self.where, t, quantity, errs, bar))

    def done(self):
        assert not self.fail, self.fail


class impl:
    """set_impl('v1') for the v1 arm, restored on exit."""

    def __init__(self, model, kernels):
        self.model, self.v1 = model, kernels == 'v1'

    def __enter__(self):
        if self.v1:
            self.model.set_impl('v1')

    def __exit__(self, *exc):
        if self.v1:
            self.model.set_impl('fused')


# ------------------------------------------------------------------ blocks
@gpu
@pytest.mark.parametrize('graph', GRAPHS)
@pytest.mark.parametrize('engine', list(ENGINES))
def test_block_forward_and_vjp(models, oracles, engine, graph):
    dep, kernels = ENGINES[engine]
    orc = oracles(dep, graph)
    ref, g = orc.ref, orc.g
    model = models(dep, kernels)
    assert model.num_layers == ref.nlayer
    judge = Judge(engine, kernels, graph)
    with impl(model, kernels):
        d = Driver(model, g, orc.types, orc.vec)
        for t in range(ref.nlayer):
            out, gx, eg = d.isolated(t, orc.x[t], orc.G[t])
            want_out, want_gx, want_gv = orc.iso[t]
            judge.compare(t, 'forward', out, want_out, ref.irreps[t + 1])
            if t > 0:
                judge.compare(t, 'dE/dx', gx, want_gx, ref.irreps[t])
            judge.compare(t, 'dE/dvec', eg, want_gv, None)
        # every block in one sweep, fresh cotangents: the summed edge_grad
        _, _, _, eg = d.sweep(orc.x, orc.G2)
        judge.compare(ref.nlayer, 'sum dE/dvec', eg, orc.sweep, None)
    judge.done()


@gpu
@pytest.mark.parametrize('engine', list(ENGINES))
def test_real_features_random_cotangents(models, refs, engine):
    """The model's own features (no overwrite of x), random cotangents per
    block: the oracle gets the features the GPU used, cast to fp64."""
    dep, kernels = ENGINES[engine]
    ref, g = refs(dep), graph_of('odd')
    model = models(dep, kernels)
    types, vec = types_for(g['labels'], ref.symbols), vec_for(g, ref)
    _, G, _ = inputs(ref, g, g['n'], seed=17)
    judge = Judge(engine, kernels, 'odd/real')
    with impl(model, kernels):
        used, outs, gx, eg = Driver(model, g, types, vec).sweep(None, G)
    total = torch.zeros(len(g['center']), 3, dtype=torch.float64)
    for t in range(ref.nlayer):
        want_out, want_gx, want_gv = bo.vjp(ref, t, used[t], vec, g['center'], g['nbr'], types,
                                            g['n'], G[t])
        judge.compare(t, 'forward (real)', outs[t], want_out, ref.irreps[t + 1])
        if t > 0:
            judge.compare(t, 'dE/dx (real)', gx[t], want_gx, ref.irreps[t])
        total += want_gv
    judge.compare(ref.nlayer, 'sum dE/dvec (real)', eg, total, None)
    judge.done()


# ------------------------------------------------------------------ overlap
@pytest.fixture(scope='module')
def rank0():
    """Rank 0 of two bricks of the HfO2 cell x (3, 1, 1): the case
    test_gpu_bwd_packed.test_decomposed_split_is_no_multiple_of_16 pins."""
    from sevennet_finetuning_amd.parallel import brick_grid, build_rank_graph
    from sevennet_finetuning_amd.structures import tile
    pos, cell, types = system('hfo2_resdat', SYMS)
    pos, cell = tile(pos, cell, (3, 1, 1))
    types = np.tile(types, len(pos) // len(types))
    rg = build_rank_graph(pos, cell, types, CUTOFF, brick_grid(2), 0)
    assert 0 < rg.n_interior < rg.n_local and rg.n_ghost > 0
    g = {'name': 'rank0', 'n': rg.n_local + rg.n_ghost, 'center': np.asarray(rg.center),
         'nbr': np.asarray(rg.nbr), 'vec': np.asarray(rg.vec, dtype=np.float32).astype(np.float64)}
    return rg, g


@gpu
@pytest.mark.parametrize('t', [2, 4], ids=['middle', 'last'])
def test_overlap_contracts(models, refs, rank0, t):
    """Forward part 0 reads only owned rows (the ghost rows hold NaN while it
    runs); after backward part 0 alone the ghost rows of dE/dx[t] are complete,
    after part 1 the owned rows too (the buffer holds NaN before)."""
    rg, g = rank0
    ref, model = refs('sn0'), models('sn0', 'fused')
    n, nl = g['n'], rg.n_local
    x, G, _ = inputs(ref, g, nl, seed=23)
    want_out, want_gx, _ = bo.vjp(ref, t, x[t], g['vec'], g['center'], g['nbr'], rg.types, nl, G[t])
    d = Driver(model, g, rg.types, g['vec'], n_local=nl, n_interior=rg.n_interior)
    e = d.eng
    judge = Judge('sn0-fused', 'fused', 'rank0')
    e.graph_set()
    for s in range(t):
        e.layer_forward(s)
    poisoned = x[t].clone()
    poisoned[nl:] = float('nan')
    d.put('x', t, poisoned)
    e.layer_forward_part(t, 0)
    d.put('x', t, x[t][nl:], rows=(nl, n))
    e.layer_forward_part(t, 1)
    out = d.get('x', t + 1)[:nl]
    assert torch.isfinite(out).all()
    judge.compare(t, 'forward (parts)', out, want_out, ref.irreps[t + 1])
    for s in range(t + 1, d.L):
        e.layer_forward(s)
    e.readout()
    d.cotangent(t, G[t])
    d.put('grad', t, torch.full((n, e.dim('grad', t)), float('nan')))
    e.layer_backward_part(t, 0)
    ghost = d.get('grad', t)
    e.layer_backward_part(t, 1)
    owned = d.get('grad', t)
    judge.compare(t, 'dE/dx ghost rows', ghost, want_gx, ref.irreps[t], rows=(nl, n))
    judge.compare(t, 'dE/dx owned rows', owned, want_gx, ref.irreps[t], rows=(0, nl))
    assert torch.equal(owned[nl:], ghost[nl:])      # part 1 leaves the ghost rows alone
    judge.done()


# ------------------------------------------------------------------ halo kernels
@gpu
@pytest.mark.parametrize('dim', [1, 3, 6, 128, 480])
@pytest.mark.parametrize('count', [0, 1, 300])
def test_halo_pack_unpack_equal_numpy_indexing(dim, count):
    """e3gnn_halo_pack / _unpack against numpy: a permuted subset of the rows,
    strides wider than ``dim``, accumulate 0 and 1; exact, and the rows (and
    the columns past ``dim``) that ``idx`` does not name are untouched."""
    from sevennet_finetuning_amd import _lib
    lib = _lib.load()
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    rng = np.random.default_rng(dim * 1000 + count)
    rows, stride = 701, dim + 5
    assert count % 256 != 0 or count == 0
    idx = rng.permutation(rows)[:count].astype(np.int32)
    table = rng.normal(size=(rows, stride)).astype(np.float32)
    dev = lambda a: torch.as_tensor(a).to(DEV)  # noqa: E731
    s = torch.cuda.current_stream(DEV).cuda_stream
    d_idx, d_table = dev(idx if count else np.zeros(1, np.int32)), dev(table)
    # pack: dst[r, :] = src[idx[r], :dim]
    packed = torch.full((max(count, 1), dim), -7.0, dtype=torch.float32, device=DEV)
    _lib.check(lib.e3gnn_halo_pack(d_idx.data_ptr(), count, dim, d_table.data_ptr(), stride,
                                   packed.data_ptr(), s))
    want = np.full((max(count, 1), dim), -7.0, dtype=np.float32)
    want[:count] = table[idx, :dim]
    assert np.array_equal(packed.cpu().numpy(), want)
    assert np.array_equal(d_table.cpu().numpy(), table)
    # unpack: dst[idx[r], :dim] (+)= src[r, :]
    src = rng.normal(size=(max(count, 1), dim)).astype(np.float32)
    d_src = dev(src)
    for acc in (0, 1):
        d_dst = dev(table)
        _lib.check(lib.e3gnn_halo_unpack(d_idx.data_ptr(), count, dim, d_src.data_ptr(),
                                         d_dst.data_ptr(), stride, acc, s))
        want = table.copy()
        want[idx, :dim] = table[idx, :dim] + src[:count] if acc else src[:count]
        assert np.array_equal(d_dst.cpu().numpy(), want), acc
