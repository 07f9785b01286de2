"""Awkward cells for the cell-list kernels (DFT-D3, device neighbour list) --
TEST INFRASTRUCTURE ONLY.

Both kernel families walk a stencil of (bin, image) cells whose extent the
host derives from the cell's heights; a stencil one cell short, a wrong bin
diagonal or wrong image arithmetic drops pairs without faulting.  The makers
below give the geometry classes where that shows: strongly skewed and
unreduced lattices (heights far below the edge lengths), many bins on one axis
only, bins of more than 64 atoms, degrees at the sort's padding boundaries and
at the 512 cap, and few atoms in a large cell.  All are seeded and
deterministic; each maker returns ``(pos, cell, z)`` in Angstrom.

``D3_CASES`` is the one table of D3 geometries and squared cutoffs (bohr^2)
that tests/test_cells_host.py checks the conditions of and
tests/test_gpu_d3.py runs.
"""
import os

import numpy as np

from oracle import d3_ref as D
from sevennet_finetuning_amd.structures import CHEMICAL_SYMBOLS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SHEAR = np.array([[1.0, 0.0, 0.0], [0.45, 1.0, 0.0], [0.4, -0.35, 1.0]])
RELABEL = np.array([[1, 0, 0], [2, 1, 0], [-1, 1, 1]])
T3, F3 = (True, True, True), (False, False, False)
TABLES, FUNCS = D.load_tables()


# ---------------------------------------------------------------- transforms
def wrapped(pos, cell):
    """pos with every fractional coordinate brought into [0, 1)."""
    frac = pos @ np.linalg.inv(cell)
    return (frac - np.floor(frac)) @ cell


def sheared(pos, cell, S=SHEAR):
    """The lattice mapped to ``S @ cell``; positions keep their fractional
    coordinates.  Returns (pos, cell)."""
    new = np.asarray(S, dtype=np.float64) @ cell
    return (pos @ np.linalg.inv(cell)) @ new, new


def relabelled(pos, cell, M=RELABEL):
    """The same crystal described by the equivalent lattice ``M @ cell`` (M
    integer, det 1).  Returns (pos unchanged, new cell, pos wrapped into the
    new cell)."""
    M = np.asarray(M)
    assert M.dtype.kind == 'i' and round(np.linalg.det(M)) == 1
    new = M.astype(np.float64) @ cell
    return pos, new, wrapped(pos, new)


def tiled(pos, cell, reps):
    """reps[k] copies along lattice vector k.  Returns (pos, cell)."""
    out = [pos + i * cell[0] + j * cell[1] + k * cell[2]
           for i in range(reps[0]) for j in range(reps[1]) for k in range(reps[2])]
    return np.concatenate(out), np.asarray(reps, dtype=np.float64)[:, None] * cell


def heights(cell):
    vol = abs(np.linalg.det(cell))
    return np.array([vol / np.linalg.norm(np.cross(cell[(k + 1) % 3], cell[(k + 2) % 3]))
                     for k in range(3)])


# -------------------------------------------------------------------- makers
def jittered_hfo2(seed=1):
    """tests/golden/hfo2_resdat.npz plus N(0, 0.05 A) noise: the noise breaks
    the crystal's degenerate distances (without it pairs sit within 1e-7
    relative of a cutoff)."""
    d = np.load(os.path.join(GOLD, 'hfo2_resdat.npz'))
    z = np.array([CHEMICAL_SYMBOLS.index(str(s)) for s in d['symbols']])
    pos = d['pos'] + np.random.default_rng(seed).normal(0.0, 0.05, d['pos'].shape)
    return pos, np.array(d['cell'], dtype=np.float64), z


def sheared_hfo2(seed=1):
    """Heights 7.84 / 9.78 / 10.26 A against lengths 10.1 / 12.1 / 11.4 A;
    every atom inside the cell."""
    pos, cell, z = jittered_hfo2(seed)
    pos, cell = sheared(pos, cell)
    return wrapped(pos, cell), cell, z


def relabelled_hfo2(seed=1, wrap=True):
    """Heights 2.68 / 7.30 / 10.26 A against lengths 10.1 / 24.3 / 16.8 A.
    ``wrap=False`` keeps the positions of the original cell (fractional
    coordinates of the new cell outside [0, 1))."""
    pos, cell, z = jittered_hfo2(seed)
    pos, cell, pos_w = relabelled(pos, cell)
    return (pos_w if wrap else pos), cell, z


def tiled_hfo2(seed=1, reps=(1, 1, 4)):
    """384 atoms, c = 41 A = 77 bohr: two default 30-bohr D3 bins on one axis,
    one on the other two; 8 neighbour-list bins along c, 1-2 along a and b."""
    pos, cell, z = jittered_hfo2(seed)
    pos, cell = tiled(pos, cell, reps)
    return pos, cell, np.tile(z, int(np.prod(reps)))


def ball(N, seed=0):
    """N points uniform in a ball of radius 2.4 A, no cell: at cutoff 5 A every
    atom has exactly N - 1 neighbours."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(N, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return v * (2.4 * rng.uniform(size=(N, 1)) ** (1.0 / 3.0)), None, np.full(N, 14)


def dense_box(seed=0):
    """700 uniform points in a periodic 10.5 A cube: 2 x 2 x 2 bins of ~87
    atoms at cutoff 5 A (two trips of the 64-lane loop over a bin)."""
    pos = np.random.default_rng(seed).uniform(0.0, 10.5, size=(700, 3))
    return pos, np.eye(3) * 10.5, np.full(700, 14)


def sparse_box():
    """Three atoms in a periodic 60 A cube: 12^3 bins at cutoff 5 A against the
    4 n + 64 = 76 limit (the bin-halving loop), exactly two edges 0 <-> 1
    across the x boundary."""
    pos = np.array([[0.5, 30.0, 30.0], [58.5, 30.0, 30.0], [30.0, 10.0, 45.0]])
    return pos, np.eye(3) * 60.0, np.full(3, 14)


# ------------------------------------------------------------- D3 conditions
def cutoff_gap(pos, cell, thr, pbc=T3):
    """Smallest |r^2 / thr - 1| over all pair images (float64, bohr^2): how far
    the nearest pair is from the squared cutoff ``thr``.  The kernel classifies
    pairs in fp32 and the oracle in fp64, so a pair closer to the cutoff than
    fp32 resolves may be counted by one and not by the other."""
    x, lat = D.wrap_bohr(pos, cell)
    tau, _ = D.translations(lat, D.repetitions(lat, thr, pbc))
    iu, ju = np.triu_indices(len(x))
    gap = np.inf
    for t in tau:                                    # one image at a time: memory
        d = x[ju] - x[iu] + t
        r2 = np.einsum('pi,pi->p', d, d)
        if not t.any():
            r2 = r2[iu != ju]
        gap = min(gap, np.abs(r2 / thr - 1.0).min())
    return float(gap)


def d3_default_nb(cell):
    """Bins per axis of the D3 host code at the default 30-bohr bin edge."""
    return tuple(max(1, int(h / D.AU_TO_ANG / 30.0)) for h in heights(cell))


# name -> (maker, maker kwargs, pbc, rthr, cn_thr); short cutoffs (rthr 250-400,
# cn_thr 120-200 bohr^2) so that one boundary cell of the stencil carries ~1e-3
# of the energy, a hundred times the energy bar of tests/test_gpu_d3.py
D3_CASES = {
    'hfo2': (jittered_hfo2, {}, T3, 300.0, 130.0),
    'sheared': (sheared_hfo2, {}, T3, 380.0, 150.0),
    'relabelled': (relabelled_hfo2, {'wrap': True}, T3, 300.0, 130.0),
    'relabelled_unwrapped': (relabelled_hfo2, {'wrap': False}, T3, 300.0, 130.0),
    'tiled': (tiled_hfo2, {}, T3, 250.0, 130.0),
    'slab_ttf': (sheared_hfo2, {}, (True, True, False), 350.0, 150.0),
    'wire_tff': (sheared_hfo2, {}, (True, False, False), 350.0, 150.0),
    'slab_ftt': (sheared_hfo2, {}, (False, True, True), 350.0, 150.0),
}


def d3_case(name):
    """(pos, cell, z, pbc, {'rthr': .., 'cn_thr': ..}) of a D3_CASES row."""
    maker, kw, pbc, rthr, cn_thr = D3_CASES[name]
    pos, cell, z = maker(**kw)
    return pos, cell, z, pbc, dict(rthr=rthr, cn_thr=cn_thr)


def oracle_d3(pos, cell, z, damping, pbc=T3, **kw):
    elems = sorted(set(int(v) for v in z))
    types = np.searchsorted(np.asarray(elems), z)
    return D.d3(pos, cell, types, D.type_tables(elems, TABLES),
                D.functional(FUNCS, damping, 'pbe'), damping, pbc=pbc, **kw)


def virial33(v):
    return np.array([[v[0], v[3], v[4]], [v[3], v[1], v[5]], [v[4], v[5], v[2]]])


def inplane_strain_derivatives(pos, cell, z, damping, pbc, kw, h=2e-6):
    """[(eps, -dE/ds)] of the oracle for the three strains eps spanning the
    plane of the two periodic lattice vectors (central differences, step h)."""
    u, v = [cell[k] for k in range(3) if pbc[k]]
    e1 = u / np.linalg.norm(u)
    e2 = v - np.dot(v, e1) * e1
    e2 /= np.linalg.norm(e2)
    out = []
    for a, b in ((e1, e1), (e2, e2), (e1, e2)):
        eps = 0.5 * (np.outer(a, b) + np.outer(b, a))

        def e(s):
            m = np.eye(3) + s * eps
            return oracle_d3(pos @ m.T, cell @ m.T, z, damping, pbc, **kw)['energy']
        out.append((eps, -(e(h) - e(-h)) / (2 * h)))
    return out
