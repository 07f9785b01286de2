"""The fused kernels' row sums as reduce-scatters (k_conv_fwd: the lane group
that owns a component stores it) on the degrees where the batching, the empty
second tile, the second pass's accumulate arm, the empty node and the last
block's per-neighbour reduction can go wrong.  Needs an MI355X: ``pytest -m gpu``.

The graph is an explicit edge list (every edge with its reverse, so a node's
in-degree is its out-degree and the last block's backward, which walks the
transposed CSR, meets the same tile counts): 'hub' nodes of the wanted degrees
joined to distinct 'filler' nodes, one node without edges, random unit
directions with lengths of 1.5-4.5 A, node ids shuffled so a workgroup's four
centres differ in tile count.
"""
import numpy as np
import pytest
import torch

from _systems import load_manifest_symbols

pytestmark = pytest.mark.gpu
SYMS = load_manifest_symbols()
# tile edges of the two-tile pass (16, 32, 48) +- 1, one edge, more than two passes
DEGREES = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 70)
N_FILL = 96


def make_graph(seed=0):
    rng = np.random.default_rng(seed)
    hubs = [d for d in DEGREES for _ in range(2)]
    n = len(hubs) + N_FILL + 1          # + the node without edges
    label = rng.permutation(n)
    pairs = []
    for h, d in enumerate(hubs):
        for f in rng.choice(N_FILL, size=d, replace=False):
            pairs.append((label[h], label[len(hubs) + f]))
    pairs = np.array(pairs)
    u = rng.normal(size=(len(pairs), 3))
    # lengths uniform in the VOLUME of the 1.5-4.5 A shell, as a neighbour
    # shell fills: lengths uniform in r put a sixth of a 70-neighbour node's
    # edges below 2 A, an environment whose atomic energies are hundreds of eV
    # of either sign and cancel in the total the energy tolerance is taken from
    r = np.cbrt(rng.uniform(1.5 ** 3, 4.5 ** 3, size=len(pairs)))
    u *= (r / np.linalg.norm(u, axis=1))[:, None]
    center = np.concatenate([pairs[:, 0], pairs[:, 1]])
    nbr = np.concatenate([pairs[:, 1], pairs[:, 0]])
    vec = np.concatenate([u, -u])
    order = np.lexsort((nbr, center))
    return n, center[order], nbr[order], vec[order]


@pytest.fixture(scope='module')
def model():
    from sevennet_finetuning_amd.model import E3GNNModel
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return E3GNNModel(device='cuda:0')


@pytest.fixture(scope='module')
def graph():
    return make_graph()


def types_of(case, n):
    if case == 'si':
        return np.full(n, SYMS.index('Si'))
    pick = np.array([SYMS.index(s) for s in ('Hf', 'O', 'Si')])   # the species of the suite's Si and HfO2 systems
    return pick[np.random.default_rng(3).integers(0, len(pick), size=n)]


def evaluate(model, graph, types):
    n, center, nbr, vec = graph
    t = lambda a, dt=torch.int32: torch.as_tensor(a, dtype=dt, device=model.device)
    out = model.energy_forces(t(types), t(center), t(nbr), t(vec, torch.float32))
    return {k: out[k].cpu().numpy() for k in ('energy', 'atomic_energy', 'forces', 'virial')}


def test_degree_coverage(graph):
    n, center, nbr, _ = graph
    want = set(DEGREES) | {0}
    assert want >= {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49} and max(want) > 64
    assert want <= set(np.bincount(center, minlength=n).tolist())
    assert want <= set(np.bincount(nbr, minlength=n).tolist())
    assert n <= 300


@pytest.mark.parametrize('case', ['si', 'mixed'])
def test_fused_matches_v1_and_repeats(model, graph, case):
    """Fused against the v1 kernels (test_fused_matches_v1_kernels' tolerances,
    the force one relative to the largest force where forces are large, as in
    test_high_degree_centres), and two fused runs with equal bits."""
    types = types_of(case, graph[0])
    if case == 'mixed':
        assert len(set(types.tolist())) > 1
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
    print(f'{case}: E={float(a["energy"]):.6f} |dE|={de:.3e} max|F|={fscale:.3e} max|dF|={df:.3e}')
    assert np.isfinite(b['forces']).all()
    assert de <= 2e-6 * abs(float(a['energy']))
    assert df <= 5e-5 * fscale
    for k in b:
        assert np.array_equal(b[k], c[k]), k
    # the node without edges: its one-body energy only, no force
    lone = int(np.flatnonzero(np.bincount(graph[1], minlength=graph[0]) == 0)[0])
    assert np.all(b['forces'][lone] == 0)
