"""The fused backward's radial derivative in forward mode (fused.hip
mlp_chain_jvp, w2_block_tan; node.hip k_edge_embed's embd and k_edge_force's
drad): the radial MLP has one scalar input r, so the kernels carry the tangent
H2' = dH2/dr beside H2, form w' = W2^T H2' from the w recompute's operand
registers and sum dE/dw . w' per edge, instead of running the MLP backward from
dH2 to dE/demb.  The GPU tests need an MI355X: ``pytest -m gpu``.

Isolating the new code: for a model with normalised SH the per-edge gradient
g = dE/dvec splits exactly into r_hat (r_hat . g), which is the radial MLP's
derivative and nothing else, and the component orthogonal to r_hat, which is
the untouched dE/dY path.  Both are compared separately with the fp64 oracle's
autograd w.r.t. the edge vectors and with the v1 kernels (``set_impl('v1')``,
which keep the reverse-mode dE/demb path).

* dimers: two atoms in a 40 A cell (one edge per centre, every other slot of
  its tile padded: the padded slots' tangent must be zero), Si-Si and Hf-O at
  1.6 A, on both sides of r_on = 4.5 A, in the middle of the switching region
  and within 1 % of the cutoff, where d emb / dr is dominated by the envelope's
  derivative;
* the five structures of test_gpu_bwd_packed.py: ``hfo2`` has 41-49 edges per
  atom (three tiles: the last block's second pass), displaced Si has its third
  shell at 4.50 A, on both sides of r_on;
* the c64 / c32 families against the generic engine;
* the raw-SH deployment of test_gpu_parity.py against oracle/nequip_ref.py on
  the full edge gradient (the split does not hold there: the SH of the raw
  vector depend on r).

Bars: energy 2e-6 relative, forces and edge gradients 1e-4 eV/A (the project's
bars) cap everything.  The radial component has a sharper one: at most twice
the parent commit's own distance to the oracle (PARENT_RADIAL, measured with
this file on the parent's library, profiles/fwdmode_radial_parent.log).  Both
forms drop terms of 2^-16 per bf16 product and sum them in another order, so
they may differ by a small factor; a lost piece product would show as about
2^8 times the parent's figure.  A dimer pair is one case of that bar (the
largest figure over its five distances): beyond r_on the gradient itself goes
to zero with the envelope, and its error there is the float noise floor, which
carries no information on a lost term.

Every evaluation is made twice and compared bit for bit, and a sequence large
case, smaller case, large case again must reproduce the first result (the
per-edge accumulators of the larger graph are zeroed again).
"""
import numpy as np
import pytest
import torch

from _systems import load_manifest_symbols
from test_gpu_bwd_image import family_models, sevennet0  # noqa: F401
from test_gpu_bwd_packed import CASES, CUTOFF, E_TOL, F_TOL, KEYS, evaluate, make_case
from test_gpu_parity import raw_sh_dir  # noqa: F401

gpu = pytest.mark.gpu
SYMS = load_manifest_symbols()
R_ON = 4.5
DIMER_PAIRS = (('Si', 'Si'), ('Hf', 'O'))
# 1.6 A; below and above r_on; the middle of the switch; within 1 % of the cutoff
DIMER_R = (1.6, 4.45, 4.55, 4.75, 4.96)
ORACLE_CASES = tuple(f'dimer_{a}{b}' for a, b in DIMER_PAIRS) + CASES

# max |r_hat . (g - g_oracle)| (eV/A) of the PARENT commit's library (reverse-mode
# dH2 -> MLP chain -> dE/demb) per case, measured with this file:
# profiles/fwdmode_radial_parent.log
PARENT_RADIAL = {
    'dimer_SiSi': 1.061359e-06,
    'dimer_HfO': 2.618139e-05,
    'si': 3.173324e-06,
    'hfo2': 9.115320e-06,
    'stretched': 2.327273e-06,
    'cluster': 7.265235e-06,
    'odd': 7.497943e-06,
}


def dimer(a, b, r):
    """Two atoms r apart along a generic direction in a 40 A cell."""
    from oracle.neighbor import neighbor_list
    u = np.array([0.36, -0.48, 0.8])
    pos = np.array([[20.0, 20.0, 20.0], [20.0, 20.0, 20.0] + r * u])
    cell = np.eye(3) * 40.0
    ei, sh = neighbor_list(pos, cell, CUTOFF)
    order = np.argsort(ei[0], kind='stable')
    ei, sh = ei[:, order], sh[order]
    return {'name': f'dimer_{a}{b}_{r}', 'pos': pos, 'cell': cell, 'symbols': [a, b], 'ei': ei, 'sh': sh,
            'vec': pos[ei[1]] - pos[ei[0]] + sh @ cell}


_cache = {}


def members(name):
    """The structures of an oracle case: one, or a dimer pair's five distances."""
    if name not in _cache:
        if name.startswith('dimer_'):
            a, b = DIMER_PAIRS[[f'dimer_{p}{q}' for p, q in DIMER_PAIRS].index(name)]
            _cache[name] = [dimer(a, b, r) for r in DIMER_R]
        else:
            _cache[name] = [make_case(name)]
    return _cache[name]


_oracle = {}


def oracle_of(case):
    """fp64 oracle of a structure on its own edge list (computed once)."""
    if case['name'] not in _oracle:
        from oracle.sevennet_ref import SevenNet0Ref
        ref = SevenNet0Ref(dtype=torch.float64)
        pos = torch.tensor(case['pos'], dtype=torch.float64, requires_grad=True)
        types = torch.tensor([SYMS.index(s) for s in case['symbols']])
        out = ref.energy(pos, types, torch.tensor(case['ei']), torch.tensor(case['sh'], dtype=torch.float64),
                         torch.tensor(case['cell'], dtype=torch.float64), False)
        g_pos, g_vec = torch.autograd.grad(out['energy'], [pos, out['edge_vec']])
        _oracle[case['name']] = {'energy': float(out['energy'].detach()), 'forces': -g_pos.numpy(),
                                 'edge_grad': g_vec.numpy()}
    return _oracle[case['name']]


def split(case, g):
    """(radial component r_hat . g [E], orthogonal part [E, 3]) of a per-edge gradient."""
    v = np.asarray(case['vec'], dtype=np.float64)
    rh = v / np.linalg.norm(v, axis=1)[:, None]
    rad = (np.asarray(g, dtype=np.float64) * rh).sum(1)
    return rad, g - rad[:, None] * rh


def distances(got, ref, case):
    ra, pa = split(case, got['edge_grad'])
    rb, pb = split(case, ref['edge_grad'])
    return {'de': abs(float(got['energy']) - float(ref['energy'])),
            'df': float(np.abs(got['forces'] - ref['forces']).max()),
            'radial': float(np.abs(ra - rb).max()), 'perp': float(np.abs(pa - pb).max())}


def test_cases_contain_what_they_claim():
    for a, b in DIMER_PAIRS:
        for c in members(f'dimer_{a}{b}'):
            assert len(c['pos']) == 2 and c['ei'].shape[1] == 2      # one edge per centre: 15 padded slots
            assert sorted(c['ei'][0].tolist()) == [0, 1]
    r = np.array(DIMER_R)
    assert r.min() == 1.6
    assert ((r < R_ON) & (r > R_ON - 0.1)).any() and ((r > R_ON) & (r < R_ON + 0.1)).any()
    assert (np.abs(r - 0.5 * (R_ON + CUTOFF)) < 1e-9).any()
    assert ((r > 0.99 * CUTOFF) & (r < CUTOFF)).any()
    for c in members('dimer_SiSi'):
        assert np.allclose(np.linalg.norm(c['vec'], axis=1), float(c['name'].rsplit('_', 1)[1]), atol=1e-12)
    tiles = set()
    for name in CASES:
        c = members(name)[0]
        rr = np.linalg.norm(c['vec'], axis=1)
        n = len(c['pos'])
        # tiles per centre (first / middle blocks' origin) and per neighbour node (the last block's passes)
        for idx in c['ei']:
            tiles |= set(((np.bincount(idx, minlength=n) + 15) // 16).tolist())
        if name in ('si', 'hfo2', 'odd'):
            assert (rr < R_ON).any() and ((rr > R_ON) & (rr < CUTOFF)).any(), name
    assert {1, 2, 3} <= tiles
    hf = members('hfo2')[0]
    deg = np.bincount(hf['ei'][1], minlength=len(hf['pos']))
    assert deg.min() >= 33 and deg.max() <= 64        # three tiles per neighbour node: two passes
    rs = np.linalg.norm(members('si')[0]['vec'], axis=1)
    assert ((rs > R_ON - 0.1) & (rs < R_ON)).any() and ((rs > R_ON) & (rs < R_ON + 0.1)).any()   # the third shell
    every = np.concatenate([np.linalg.norm(c['vec'], axis=1) for k in ORACLE_CASES for c in members(k)])
    assert (every > 0.99 * CUTOFF).any() and ((every > R_ON + 0.2) & (every < CUTOFF - 0.2)).any()


@gpu
@pytest.mark.parametrize('name', ORACLE_CASES)
def test_radial_and_angular_parts_match_oracle_and_v1(sevennet0, name):  # noqa: F811
    model = sevennet0
    worst = 0.0
    for case in members(name):
        try:
            model.set_impl('v1')
            v1 = evaluate(model, case, SYMS)
        finally:
            model.set_impl('fused')
        a = evaluate(model, case, SYMS)
        b = evaluate(model, case, SYMS)
        ref = oracle_of(case)
        assert all(np.isfinite(a[k]).all() for k in KEYS)
        do, dv, dvo = distances(a, ref, case), distances(a, v1, case), distances(v1, ref, case)
        print(f'{case["name"]}: vs oracle |dE|={do["de"]:.3e} max|dF|={do["df"]:.3e} radial={do["radial"]:.3e} '
              f'perp={do["perp"]:.3e}; vs v1 radial={dv["radial"]:.3e} perp={dv["perp"]:.3e}; '
              f'v1 vs oracle radial={dvo["radial"]:.3e}')
        escale = abs(ref['energy'])
        for d in (do, dv):
            assert d['de'] <= E_TOL * escale
            assert d['df'] <= F_TOL
            assert d['radial'] <= F_TOL
            assert d['perp'] <= F_TOL
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), k
        worst = max(worst, do['radial'])
    print(f'radial figure: case={name} value={worst:.6e} parent={PARENT_RADIAL[name]:.6e}')
    assert worst <= 2.0 * PARENT_RADIAL[name]


@gpu
def test_smaller_graph_in_between_leaves_no_trace(sevennet0):  # noqa: F811
    big, small = members('hfo2')[0], members('cluster')[0]
    first = evaluate(sevennet0, big, SYMS)
    evaluate(sevennet0, small, SYMS)
    third = evaluate(sevennet0, big, SYMS)
    for k in KEYS:
        assert np.array_equal(first[k], third[k]), k


@gpu
@pytest.mark.parametrize('name', ['si', 'hfo2'])
def test_family_parts_match_generic_engine(family_models, name):  # noqa: F811
    fused, generic = family_models
    case = members(name)[0]
    a, ref = evaluate(fused, case, fused.chemical_symbols), evaluate(generic, case, generic.chemical_symbols)
    b = evaluate(fused, case, fused.chemical_symbols)
    assert all(np.isfinite(a[k]).all() for k in KEYS)
    d = distances(a, ref, case)
    print(f'{name} family {fused.family} vs generic: |dE|={d["de"]:.3e} max|dF|={d["df"]:.3e} '
          f'radial={d["radial"]:.3e} perp={d["perp"]:.3e}')
    assert d['de'] <= E_TOL * abs(float(ref['energy']))
    assert d['df'] <= F_TOL and d['radial'] <= F_TOL and d['perp'] <= F_TOL
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


@gpu
@pytest.mark.parametrize('name', ['si', 'odd'])
def test_raw_sh_edge_gradient_matches_nequip_ref(raw_sh_dir, name):  # noqa: F811
    from oracle.nequip_ref import NequIPRef
    from sevennet_finetuning_amd.model import E3GNNModel
    m = E3GNNModel(raw_sh_dir, device='cuda:0')
    assert m.family == 0
    case = members(name)[0]
    a, b = evaluate(m, case, SYMS), evaluate(m, case, SYMS)
    ref_m = NequIPRef(raw_sh_dir)
    assert not ref_m.sh_normalize
    # positions 0 and the unit cell: the reference's edge vectors are the shifts
    vec = torch.tensor(case['vec'], dtype=torch.float64, requires_grad=True)
    types = torch.tensor([SYMS.index(s) for s in case['symbols']])
    out = ref_m.energy(torch.zeros(len(types), 3, dtype=torch.float64), types, torch.tensor(case['ei']), vec,
                       torch.eye(3, dtype=torch.float64), False)
    g, = torch.autograd.grad(out['energy'], [vec])
    de = abs(float(a['energy']) - float(out['energy']))
    dg = float(np.abs(a['edge_grad'] - g.numpy()).max())
    print(f'raw SH {name}: |dE|={de:.3e} max|dgrad|={dg:.3e}')
    assert de <= E_TOL * abs(float(out['energy']))
    assert dg <= F_TOL
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
