"""The lock-step backward's one W2 image per block pair (csrc/w2_image.h: row
reads for dH2, transposed reads for the w recompute) on the graphs where its
staging can go wrong: workgroups whose four centres differ in tile count, so
that one, two or three waves have no tile left (and skip the image reads)
while the others still stage and read, a partly filled last workgroup, and
the channel families with other weight widths and pair counts.  Needs an
MI355X: ``pytest -m gpu``.

The graph is an explicit edge list (every edge with its reverse, so a node's
in-degree is its out-degree): 'hub' nodes of degrees 0, 1, 15, 16, 17 and 33
(0, 1, 1, 1, 2 and 3 tiles of 16 edges) joined to distinct 'filler' nodes,
random directions with lengths uniform in the volume of the 1.5-4.5 A shell,
Hf / O / Si mixed.  A workgroup is four consecutive centres: the hubs take the
node ids HEAD lists, group by group, the fillers follow, and the last n mod 4
ids (the partly filled workgroup) are hubs again.
"""
import os

import numpy as np
import pytest
import torch

from _systems import load_manifest_symbols

pytestmark = pytest.mark.gpu
SYMS = load_manifest_symbols()
SPECIES = ('Hf', 'O', 'Si')
# hub degrees by node id, one row per workgroup; tiles per wave in the comment
HEAD = ((33, 1, 0, 15),     # 3 1 0 1: three waves without a tile in tiles 1, 2
        (33, 33, 16, 1),    # 3 3 1 1: two waves
        (33, 33, 33, 1),    # 3 3 3 1: one wave
        (17, 16, 15, 1),    # 2 1 1 1: three waves in tile 1
        (33, 17, 17, 16))   # 3 2 2 1: one wave in tile 1, three in tile 2
TAIL = (33, 17, 16)         # the first n mod 4 of them end the node list
NODES = (141, 142, 143)     # n mod 4 = 1, 2, 3


def make_graph(n, seed=0):
    rng = np.random.default_rng(seed)
    head = [d for grp in HEAD for d in grp]
    tail = list(TAIL[:n % 4])
    fill = np.arange(len(head), n - len(tail))
    hubs = list(enumerate(head)) + [(n - len(tail) + i, d) for i, d in enumerate(tail)]
    pairs = np.array([(h, f) for h, d in hubs for f in rng.choice(fill, size=d, replace=False)])
    u = rng.normal(size=(len(pairs), 3))
    r = np.cbrt(rng.uniform(1.5 ** 3, 4.5 ** 3, size=len(pairs)))
    u *= (r / np.linalg.norm(u, axis=1))[:, None]
    center = np.concatenate([pairs[:, 0], pairs[:, 1]])
    nbr = np.concatenate([pairs[:, 1], pairs[:, 0]])
    vec = np.concatenate([u, -u])
    order = np.lexsort((nbr, center))
    return n, center[order], nbr[order], vec[order]


@pytest.fixture(scope='module', params=NODES)
def graph(request):
    return make_graph(request.param)


def types_of(symbols, n):
    pick = np.array([symbols.index(s) for s in SPECIES])
    t = pick[np.random.default_rng(3).integers(0, len(pick), size=n)]
    assert len(set(t.tolist())) == len(SPECIES)
    return t


def evaluate(model, graph, types):
    n, center, nbr, vec = graph
    t = lambda a, dt=torch.int32: torch.as_tensor(a, dtype=dt, device=model.device)  # noqa: E731
    out = model.energy_forces(t(types), t(center), t(nbr), t(vec, torch.float32))
    return {k: out[k].cpu().numpy() for k in ('energy', 'atomic_energy', 'forces', 'virial')}


def test_graph_covers_the_tile_patterns(graph):
    n, center, nbr, _ = graph
    assert n <= 300 and n % 4 in (1, 2, 3)
    deg = np.bincount(center, minlength=n)
    assert np.array_equal(deg, np.bincount(nbr, minlength=n))
    assert {0, 1, 15, 16, 17, 33} <= set(deg.tolist())
    tiles = (deg + 15) // 16
    groups = [tiles[c:c + 4] for c in range(0, n, 4)]
    # waves of a workgroup without a tile while another of its waves has one
    idle = {int((g < t + 1).sum()) for g in groups for t in range(int(g.max())) if len(g) == 4}
    assert {1, 2, 3} <= idle
    # the partly filled last workgroup has multi-tile centres
    assert len(groups[-1]) == n % 4 and groups[-1].max() >= 2


@pytest.fixture(scope='module')
def sevennet0():
    from sevennet_finetuning_amd.model import E3GNNModel
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return E3GNNModel(device='cuda:0')


def test_fused_matches_v1_and_repeats(sevennet0, graph):
    """SevenNet-0, fused against the v1 kernels (the tolerances of
    test_gpu_rowsum.test_fused_matches_v1_and_repeats), and two fused runs
    with equal bits."""
    model = sevennet0
    types = types_of(SYMS, graph[0])
    try:
        model.set_impl('v1')
        a = evaluate(model, graph, types)
    finally:
        model.set_impl('fused')
    b = evaluate(model, graph, types)
    c = evaluate(model, graph, types)
    fscale = max(1.0, float(np.abs(a['forces']).max()))
    de = abs(float(a['energy']) - float(b['energy']))
    df = float(np.abs(a['forces'] - b['forces']).max())
    print(f'n={graph[0]}: E={float(a["energy"]):.6f} |dE|={de:.3e} max|F|={fscale:.3e} max|dF|={df:.3e}')
    assert np.isfinite(b['forces']).all()
    assert de <= 2e-6 * abs(float(a['energy']))
    assert df <= 5e-5 * fscale
    for k in b:
        assert np.array_equal(b[k], c[k]), k


@pytest.fixture(scope='module', params=[(64, 1), (32, 2)], ids=['c64', 'c32'])
def family_models(request, tmp_path_factory):
    """A three-block deployment of the channel family on the fused kernels and
    on the generic runtime-table engine (deployed as test_gpu_family.py does)."""
    from sevennet_finetuning_amd import model_build as mb
    from sevennet_finetuning_amd.model import E3GNNModel
    ch, fam = request.param
    d = str(tmp_path_factory.mktemp(f'img_c{ch}'))
    mb.deploy_config(mb.sevennet_shaped_config(ch, 3, species=list(SPECIES)), d, seed=ch + 3)
    a = E3GNNModel(d, device='cuda:0')
    old = os.environ.get('E3GNN_GENERIC')
    os.environ['E3GNN_GENERIC'] = '1'
    try:
        b = E3GNNModel(d, device='cuda:0')
    finally:
        if old is None:
            del os.environ['E3GNN_GENERIC']
        else:
            os.environ['E3GNN_GENERIC'] = old
    assert a.family == fam and b.family == -1
    return a, b


def test_family_matches_generic_engine(family_models, graph):
    """The c64 and c32 families (other weight widths and pair counts), fused
    against the generic engine with the tolerances of
    test_gpu_family.test_family_model_equals_generic_engine."""
    a, b = family_models
    types = types_of(a.chemical_symbols, graph[0])
    ra, rb = evaluate(a, graph, types), evaluate(b, graph, types)
    de = abs(float(ra['energy']) - float(rb['energy']))
    df = float(np.abs(ra['forces'] - rb['forces']).max())
    print(f'n={graph[0]}: E={float(rb["energy"]):.6f} |dE|={de:.3e} '
          f'max|F|={float(np.abs(rb["forces"]).max()):.3e} max|dF|={df:.3e}')
    assert np.isfinite(ra['forces']).all()
    assert de <= 2e-6 * abs(float(rb['energy']))
    assert df <= 5e-5
    again = evaluate(a, graph, types)
    assert np.array_equal(again['energy'], ra['energy']) and np.array_equal(again['forces'], ra['forces'])
