"""The list filter's reference and LAMMPS-like inputs -- TEST INFRASTRUCTURE ONLY.

``filter_ref`` restates the edge loop of ``SerialStep`` (native/
pair_e3gnn_core.cpp, the host graph build) in numpy: a pure function of the
arrays ``e3gnn_plist_set`` / ``_build`` take.  ``lammps_like`` turns a periodic
structure into what LAMMPS would hand the serial pair style: owned atoms, one
explicit ghost row per periodic image within rc + skin of an owned atom,
shuffled tags, candidate lists at rc + skin in an order of their own with a
special bit on every other entry.
"""
import functools

import numpy as np

from sevennet_finetuning_amd.neighbor import _brute

NEIGHMASK = 0x1FFFFFFF
SPECIAL = 1 << 30


def filter_ref(x, row_atom, cand_ptr, cand, neighmask, atom_row, rc):
    """(center int32 [E], nbr int32 [E], vec float32 [E, 3]): for row t in order,
    for candidate c in the list's order, j = cand[c] & neighmask, d = x[j] -
    x[row_atom[t]] in f64, kept when ((d0 d0) + (d1 d1)) + (d2 d2) < rc rc."""
    x = np.asarray(x, dtype=np.float64)
    cand_ptr = np.asarray(cand_ptr, dtype=np.int64)
    rows = np.repeat(np.arange(len(row_atom), dtype=np.int64), np.diff(cand_ptr))
    j = np.asarray(cand, dtype=np.int32) & np.int32(neighmask)
    d = x[j] - x[np.asarray(row_atom)[rows]]
    r2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
    hit = r2 < float(rc) * float(rc)
    return (rows[hit].astype(np.int32), np.asarray(atom_row)[j[hit]].astype(np.int32),
            d[hit].astype(np.float32))


def lammps_like(pos, cell, rc, skin, seed=0):
    """dict(x [n_total, 3], tag [n_total], row_atom [n], cand_ptr [n + 1], cand,
    atom_row [n_total], n, n_total) of the periodic structure (pos, cell).

    Atom rows: the n owned atoms as given, then a ghost row for every image
    (j, S != 0) within rc + skin of an owned atom, x = pos[j] + S cell (the
    operation order of ``neighbor._rij``, so x[ghost] - x[i] is the host
    list's r_ij bit for bit).  Tags are a seeded shuffle of 1..n, a ghost
    carries its atom's; graph rows are tags - 1.  A row's candidates are all
    its pairs at rc + skin from ``neighbor._brute``, listed by descending atom
    row (an order no sort of this library produces), entries at odd positions
    carrying the special bit 1 << 30."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    n = len(pos)
    rng = np.random.default_rng(seed)
    i, j, S = _brute(pos, cell, rc + skin, (True, True, True))
    S = S.astype(np.int64)
    img = np.concatenate([j[:, None], S], axis=1)
    ghosts = np.unique(img[S.any(axis=1)], axis=0)            # distinct (j, S != 0)
    gj, gS = ghosts[:, 0], ghosts[:, 1:].astype(np.float64)
    sc = [((gS[:, 0] * cell[0, d]) + (gS[:, 1] * cell[1, d])) + (gS[:, 2] * cell[2, d])
          for d in range(3)]
    xg = np.stack([pos[gj, d] + sc[d] for d in range(3)], axis=1)
    x = np.concatenate([pos, xg])
    n_total = len(x)
    tag = rng.permutation(n) + 1
    tag = np.concatenate([tag, tag[gj]])
    index_of = {tuple(g): n + k for k, g in enumerate(ghosts)}
    atom = np.array([jj if not s.any() else index_of[(jj, *s)] for jj, s in zip(j, S)],
                    dtype=np.int64)
    row_atom = np.empty(n, dtype=np.int32)
    row_atom[tag[:n] - 1] = np.arange(n)
    cand, cand_ptr = [], [0]
    for t in range(n):
        c = np.sort(atom[i == row_atom[t]])[::-1].astype(np.int32)
        c[1::2] |= np.int32(SPECIAL)
        cand.append(c)
        cand_ptr.append(cand_ptr[-1] + len(c))
    return dict(x=x, tag=tag, row_atom=row_atom, cand_ptr=np.array(cand_ptr, dtype=np.int64),
                cand=np.concatenate(cand).astype(np.int32), atom_row=(tag - 1).astype(np.int32),
                n=n, n_total=n_total)


SYSTEMS = ('si_rng0_2x2x1', 'hfo2_resdat', 'mixed_2x1x1')
RC, SKIN = 5.0, 1.0


@functools.lru_cache(maxsize=None)
def case(name):
    """(pos, cell, lammps_like inputs, filter_ref output) of a SYSTEMS member
    at rc 5.0, skin 1.0; computed once, shared, never modified."""
    from _systems import load_manifest_symbols, system
    pos, cell, _ = system(name, load_manifest_symbols())
    L = lammps_like(pos, cell, RC, SKIN, seed=len(name))
    ref = filter_ref(L['x'], L['row_atom'], L['cand_ptr'], L['cand'], NEIGHMASK, L['atom_row'], RC)
    for a in (*L.values(), *ref, pos, cell):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return pos, cell, L, ref
