"""The rank-graph filter's reference and brick-like inputs -- TEST INFRASTRUCTURE ONLY.

``rank_ref`` restates the loop of ``ParallelStep::build`` (native/
pair_e3gnn_core.cpp, the host graph build of the parallel pair style) in numpy:
a pure function of the arrays ``e3gnn_plist_set_rank`` / ``_rank_build`` take.
``brick_like`` extends ``_plist_ref.lammps_like`` to one rank of a decomposed
run: the atoms with fractional x < 0.5 are owned, every other (atom, image)
within rc + skin of an owned atom is a ghost row, so ghosts carry owned tags
(periodic self-images) and tags the rank does not own, several images of one
tag among them.
"""
import functools

import numpy as np

from _plist_ref import NEIGHMASK, RC, SKIN, SPECIAL, SYSTEMS  # noqa: F401  (shared constants)
from sevennet_finetuning_amd.neighbor import _brute


def rank_ref(x, row_atom, cand_ptr, cand, neighmask, atom_class, rc):
    """dict(center, nbr int32 [E], vec float32 [E, 3], ghost_atom int32
    [n_ghost], n_ghost): for row t in order, for candidate c in the list's
    order, j = cand[c] & neighmask, d = x[j] - x[row_atom[t]] in f64, kept when
    ((d0 d0) + (d1 d1)) + (d2 d2) < rc rc; nbr = atom_class[j] when that is an
    owned row (< n), else n + r with r counting the classes >= n in the order
    they are first met; ghost_atom[r] = the j they are first met with."""
    x = np.asarray(x, dtype=np.float64)
    cand_ptr = np.asarray(cand_ptr, dtype=np.int64)
    n = len(row_atom)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(cand_ptr))
    j = np.asarray(cand, dtype=np.int32) & np.int32(neighmask)
    d = x[j] - x[np.asarray(row_atom)[rows]]
    r2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
    hit = r2 < float(rc) * float(rc)
    jh = j[hit]
    cls = np.asarray(atom_class, dtype=np.int64)[jh]
    nbr = cls.copy()
    ge = np.flatnonzero(cls >= n)                       # edges to classes the rank does not own
    uniq, first = np.unique(cls[ge], return_index=True)  # first: first position in ge of each class
    order = np.argsort(first, kind='stable')             # classes by first edge
    row_of = np.empty(len(uniq), dtype=np.int64)
    row_of[order] = n + np.arange(len(uniq))
    nbr[ge] = row_of[np.searchsorted(uniq, cls[ge])]
    ghost_atom = jh[ge[first[order]]].astype(np.int32)
    return dict(center=rows[hit].astype(np.int32), nbr=nbr.astype(np.int32),
                vec=d[hit].astype(np.float32), ghost_atom=ghost_atom, n_ghost=len(uniq))


def classes(tag, row_atom, n_total):
    """(atom_class int32 [n_total], n_class): the row of an owned atom and of a
    ghost with an owned tag; n + k for the k-th distinct tag (ascending) that
    no owned atom carries."""
    n = len(row_atom)
    row_of_tag = {int(tag[a]): t for t, a in enumerate(row_atom)}
    foreign = sorted({int(t) for t in tag[:n_total]} - set(row_of_tag))
    k_of_tag = {t: n + k for k, t in enumerate(foreign)}
    cls = np.array([row_of_tag.get(int(t), k_of_tag.get(int(t))) for t in tag[:n_total]],
                   dtype=np.int32)
    return cls, len(foreign)


def brick_like(pos, cell, rc, skin, seed=0):
    """dict(x, tag [n_total], row_atom [n], cand_ptr [n + 1], cand, atom_class
    [n_total], n_class, n, n_total) of the rank owning fractional x < 0.5 of the
    periodic structure (pos, cell).

    Atom rows: the n owned atoms (a seeded shuffle of their file order), then a
    ghost row for every other (atom, image) within rc + skin of an owned atom,
    x = pos[j] + S cell.  Tags are a seeded shuffle of 1..N over all N atoms of
    the structure, a ghost carries its atom's.  Graph rows are a second shuffle
    of the owned atoms (``row_atom``: LAMMPS' ilist order is no sorted order).
    Candidates as in ``lammps_like``: descending atom row, special bit on the
    entries at odd positions."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    N = len(pos)
    rng = np.random.default_rng(seed)
    frac = pos @ np.linalg.inv(cell)
    frac -= np.floor(frac)
    owned = rng.permutation(np.flatnonzero(frac[:, 0] < 0.5))
    n = len(owned)
    is_owned = np.zeros(N, dtype=bool)
    is_owned[owned] = True
    i, j, S = _brute(pos, cell, rc + skin, (True, True, True))
    S = S.astype(np.int64)
    keep = is_owned[i]
    i, j, S = i[keep], j[keep], S[keep]
    img = np.concatenate([j[:, None], S], axis=1)
    is_ghost = S.any(axis=1) | ~is_owned[j]
    ghosts = np.unique(img[is_ghost], axis=0)                 # distinct (j, S) not an owned atom
    gj, gS = ghosts[:, 0], ghosts[:, 1:].astype(np.float64)
    sc = [((gS[:, 0] * cell[0, d]) + (gS[:, 1] * cell[1, d])) + (gS[:, 2] * cell[2, d])
          for d in range(3)]
    xg = np.stack([pos[gj, d] + sc[d] for d in range(3)], axis=1)
    x = np.concatenate([pos[owned], xg])
    n_total = len(x)
    tag_of = rng.permutation(N) + 1
    tag = np.concatenate([tag_of[owned], tag_of[gj]])
    local = np.full(N, -1, dtype=np.int64)
    local[owned] = np.arange(n)
    index_of = {tuple(g): n + k for k, g in enumerate(ghosts)}
    atom = np.array([index_of[(jj, *s)] if g else local[jj] for jj, s, g in zip(j, S, is_ghost)],
                    dtype=np.int64)
    row_atom = rng.permutation(n).astype(np.int32)
    li = local[i]
    cand, cand_ptr = [], [0]
    for t in range(n):
        c = np.sort(atom[li == row_atom[t]])[::-1].astype(np.int32)
        c[1::2] |= np.int32(SPECIAL)
        cand.append(c)
        cand_ptr.append(cand_ptr[-1] + len(c))
    atom_class, n_class = classes(tag, row_atom, n_total)
    return dict(x=x, tag=tag, row_atom=row_atom, cand_ptr=np.array(cand_ptr, dtype=np.int64),
                cand=np.concatenate(cand).astype(np.int32), atom_class=atom_class,
                n_class=n_class, n=n, n_total=n_total)


def vacuity(L, ref):
    """The four things a brick-like input must hold for the rank graph to be
    tested by it, from the reference alone (dict of bools):
    shared_row    a non-owned class with two or more distinct ghost atoms inside
                  the cutoff, sharing one row;
    self_image    a ghost with an owned tag inside the cutoff (an owned row);
    edgeless      a class without an edge (n_ghost < n_class);
    rows_apart    a class whose first edge sits in another row than its second."""
    n = L['n']
    c, nb = ref['center'], ref['nbr']
    # the atom of every edge, recovered the way the reference walked the list
    rows = np.repeat(np.arange(n), np.diff(L['cand_ptr']))
    j = L['cand'] & NEIGHMASK
    d = L['x'][j] - L['x'][L['row_atom'][rows]]
    hit = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2]) < RC * RC
    jh = j[hit]
    assert len(jh) == len(c)
    shared = rows_apart = False
    for r in range(n, n + ref['n_ghost']):
        e = np.flatnonzero(nb == r)
        shared = shared or len(np.unique(jh[e])) >= 2
        rows_apart = rows_apart or (len(e) >= 2 and c[e[0]] != c[e[1]])
    return dict(shared_row=bool(shared), self_image=bool(((jh >= n) & (nb < n)).any()),
                edgeless=ref['n_ghost'] < L['n_class'], rows_apart=bool(rows_apart))


@functools.lru_cache(maxsize=None)
def rank_case(name):
    """(brick_like inputs, rank_ref output) of a SYSTEMS member at rc 5.0, skin
    1.0; computed once, shared, never modified."""
    from _systems import load_manifest_symbols, system
    pos, cell, _ = system(name, load_manifest_symbols())
    L = brick_like(pos, cell, RC, SKIN, seed=len(name))
    ref = rank_ref(L['x'], L['row_atom'], L['cand_ptr'], L['cand'], NEIGHMASK, L['atom_class'], RC)
    for a in (*L.values(), *ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return L, ref
