"""The lock-step backward's staging of TWO block pairs per barrier (fused.hip,
LsQuads: SevenNet-0's middle block; each of the two LDS buffers holds the W2
images of a group of four blocks, and the second pair of a group starts without
a barrier) beside the families that keep one pair per barrier (c64, c32, every
first block).  Needs an MI355X: ``pytest -m gpu``.

The graphs are the explicit edge lists of test_gpu_bwd_image.py (hubs of degree
0, 1, 15, 16, 17 and 33 joined to filler nodes, Hf / O / Si mixed, n mod 4 =
1, 2, 3) with other random edges.  What they cover here:

* workgroups in which one, two or three waves have no tile left (they skip the
  image reads of both pairs of a group) while the others still stage, read
  and flip buffers;
* a centre without edges beside centres with tiles, and the empty slots of
  the partly filled last workgroup, which stage and wait with the others;
* the last centre has edges, so the last workgroup runs whole tiles.
"""
import numpy as np
import pytest

from _systems import load_manifest_symbols
from test_gpu_bwd_image import NODES, evaluate, family_models, make_graph, sevennet0, types_of  # noqa: F401

pytestmark = pytest.mark.gpu
SYMS = load_manifest_symbols()


@pytest.fixture(scope='module', params=NODES)
def graph(request):
    return make_graph(request.param, seed=11)


def test_graph_covers_the_group_patterns(graph):
    n, center, nbr, _ = graph
    assert n <= 150 and n % 4 in (1, 2, 3)
    deg = np.bincount(center, minlength=n)
    assert {0, 1, 15, 16, 17, 33} <= set(deg.tolist())
    tiles = (deg + 15) // 16
    groups = [tiles[c:c + 4] for c in range(0, n, 4)]
    idle = {int((g < t + 1).sum()) for g in groups for t in range(int(g.max())) if len(g) == 4}
    assert {1, 2, 3} <= idle
    # a centre without edges in a workgroup that runs tiles
    assert any(g.min() == 0 and g.max() >= 2 for g in groups if len(g) == 4)
    # the partly filled last workgroup runs tiles, the last centre among them
    assert len(groups[-1]) == n % 4 and groups[-1].max() >= 2 and deg[n - 1] > 0


def test_fused_matches_v1_and_repeats(sevennet0, graph):  # noqa: F811
    """SevenNet-0, fused against the v1 kernels with the tolerances of
    test_gpu_bwd_image.py, and two fused runs with equal bits."""
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


def test_family_matches_generic_engine(family_models, graph):  # noqa: F811
    """The c64 and c32 three-block deployments (one pair per barrier), fused
    against the generic engine with the tolerances of test_gpu_bwd_image.py."""
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
