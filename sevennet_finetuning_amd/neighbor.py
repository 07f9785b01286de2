"""Host periodic neighbor list (cell list), reference edge convention.

Replaces the graph-building step before the hot path: ASE
``primitive_neighbor_list('ijDS')`` in the reference
(sevenn/train/dataload.py:31-68, :113-125) and the host loops of
pair_e3gnn.cpp:155-182.  Convention:

* edge_index[0] = i (centre, aggregation target), edge_index[1] = j
  (neighbor, gathered source);
* integer image shift S with r_ij = pos[j] + S @ cell - pos[i], |r_ij| < rc;
* every image is an edge, i == j only with S != 0 (periodic self images);
* edges sorted by (i, j, S) -- CSR by centre, which the HIP kernels require.
"""
import itertools

import numpy as np


def _rij(pos_j, pos_i, S, cell):
    """r_ij = (pos_j + S cell) - pos_i, term by term in this order (elementwise
    f64, no fused multiply-add): the device list (csrc/neighbor.hip) evaluates
    the same expression, so the inclusion test agrees bit for bit."""
    S = np.asarray(S, dtype=np.float64)
    sc = [((S[..., 0] * cell[0, d]) + (S[..., 1] * cell[1, d])) + (S[..., 2] * cell[2, d])
          for d in range(3)]
    return np.stack([(pos_j[..., d] + sc[d]) - pos_i[..., d] for d in range(3)], axis=-1)


def _r2(d):
    return ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])


def _heights(cell):
    vol = abs(np.linalg.det(cell))
    return np.array([vol / np.linalg.norm(np.cross(cell[(k + 1) % 3], cell[(k + 2) % 3]))
                     for k in range(3)])


def _brute(pos, cell, cutoff, pbc, centers=None):
    h = _heights(cell) if any(pbc) else np.ones(3)
    ci = np.arange(len(pos)) if centers is None else np.asarray(centers, dtype=np.int64)
    reps = [int(np.ceil(cutoff / h[k])) if pbc[k] else 0 for k in range(3)]
    # unwrapped coordinates (MD-style): the images are enumerated around the
    # wrapped atoms, S = image + f0[i] - f0[j] as in _cell_list, and the test
    # runs on the positions as given (f0 = 0 throughout for wrapped input)
    f0 = np.zeros((len(pos), 3))
    if any(pbc):
        per = np.array([bool(p) for p in pbc])
        f0[:, per] = np.floor(pos @ np.linalg.inv(cell))[:, per]
    ii, jj, ss = [], [], []
    for s in itertools.product(*[range(-r, r + 1) for r in reps]):
        S = np.array(s, dtype=np.float64) + f0[ci][:, None, :] - f0[None, :, :]
        d = _rij(pos[None, :, :], pos[ci, None, :], S, cell)
        mask = _r2(d) < cutoff * cutoff
        if not any(s):
            mask[np.arange(len(ci)), ci] = False
        i, j = np.nonzero(mask)
        ii.append(ci[i])
        jj.append(j)
        ss.append(S[i, j])
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(ss)


def _cell_list(pos, cell, cutoff, centers=None):
    inv = np.linalg.inv(cell)
    frac = pos @ inv
    f0 = np.floor(frac)
    frac = frac - f0
    nb = np.maximum((_heights(cell) / cutoff).astype(np.int64), 1)
    b3 = np.minimum((frac * nb).astype(np.int64), nb - 1)
    bid = (b3[:, 0] * nb[1] + b3[:, 1]) * nb[2] + b3[:, 2]
    order = np.argsort(bid, kind='stable')
    nbins = int(nb.prod())
    counts = np.bincount(bid, minlength=nbins)
    start = np.concatenate([[0], np.cumsum(counts)])
    m = int(counts.max())
    table = np.full((nbins, m), -1, dtype=np.int64)
    slot = np.arange(len(pos)) - start[bid[order]]
    table[bid[order], slot] = order
    ii, jj, ss = [], [], []
    rc2 = cutoff * cutoff
    idx = np.arange(len(pos)) if centers is None else np.asarray(centers, dtype=np.int64)
    for off in itertools.product((-1, 0, 1), repeat=3):
        nbc = b3[idx] + np.array(off)
        sh = np.floor_divide(nbc, nb)
        nbc = nbc - sh * nb
        nbid = (nbc[:, 0] * nb[1] + nbc[:, 1]) * nb[2] + nbc[:, 2]
        cand = table[nbid]                                  # [N, m]
        valid = cand >= 0
        c = np.where(valid, cand, 0)
        # image of the unwrapped positions: S = bin-image shift + f0[i] - f0[j]
        S = sh[:, None, :] + f0[idx][:, None, :] - f0[c]
        d = _rij(pos[c], pos[idx][:, None, :], S, cell)
        ok = valid & (_r2(d) < rc2)
        ok &= ~((c == idx[:, None]) & ~S.any(axis=2))
        r, k = np.nonzero(ok)
        ii.append(idx[r])
        jj.append(c[r, k])
        ss.append(S[r, k])
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(ss)


def neighbor_list(pos, cell, cutoff, pbc=(True, True, True), centers=None):
    """Returns (edge_index int64 [2,E], shift float64 [E,3]) sorted by centre.
    ``centers``: optional subset of centre atoms (a rank's owned atoms in the
    domain decomposition); neighbours are still taken from every atom."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    cell = np.zeros((3, 3)) if cell is None else np.ascontiguousarray(cell, dtype=np.float64)
    if all(pbc) and np.all(_heights(cell) >= 3 * cutoff):
        i, j, s = _cell_list(pos, cell, cutoff, centers)
    else:
        i, j, s = _brute(pos, cell, cutoff, pbc, centers)
    order = np.lexsort((s[:, 2], s[:, 1], s[:, 0], j, i))
    return (np.stack([i[order], j[order]]).astype(np.int64),
            np.ascontiguousarray(s[order]))


def batch_neighbor_list(structs, cutoff):
    """The graph of a batch of structures: every structure's ``neighbor_list``
    with its first row added to i and j, one structure after the other -- the
    contract of ``DeviceNeighborList.batch`` stated on the host.

    ``structs``: sequence of ``(pos, cell, pbc)`` (``cell`` may be None for an
    isolated structure).  Returns ``(edge_index int64 [2, E], shift float64
    [E, 3], atom_ptr int64 [B + 1], edge_ptr int64 [B + 1])``."""
    eis, shs, atom_ptr, edge_ptr = [], [], [0], [0]
    for pos, cell, pbc in structs:
        ei, sh = neighbor_list(pos, cell, cutoff, tuple(bool(p) for p in pbc))
        eis.append(ei + atom_ptr[-1])
        shs.append(sh)
        atom_ptr.append(atom_ptr[-1] + len(pos))
        edge_ptr.append(edge_ptr[-1] + ei.shape[1])
    ei = np.concatenate(eis, axis=1) if eis else np.zeros((2, 0), dtype=np.int64)
    sh = np.concatenate(shs) if shs else np.zeros((0, 3))
    return (ei.astype(np.int64), np.ascontiguousarray(sh, dtype=np.float64),
            np.array(atom_ptr, dtype=np.int64), np.array(edge_ptr, dtype=np.int64))


class DeviceNeighborList:
    """Neighbour list on the GPU (libe3gnn_hip.so ``e3gnn_nlist_*``), the same
    edges, order and integer shifts as ``neighbor_list`` (bit for bit).

    ``__call__(pos, cell, cutoff, pbc)`` returns device tensors
    ``(edge_center int32 [E], edge_nbr int32 [E], shift int32 [E, 3],
    edge_vec float32 [E, 3])``.  pbc must be all True or all False (the
    device list raises ``E3GNNError`` otherwise; ``neighbor_list`` covers the
    mixed case on the host).

    ``rank_graph(pos, cell, cutoff, owner, rank, world)`` builds one rank's
    graph of a spatial decomposition on the same handle (see there and
    ``parallel.build_rank_graph_device``).

    ``batch(positions_list, cells_list, cutoff, pbc_list)`` builds the graphs of
    many structures in one set of launches (``batch_neighbor_list`` on the
    device)."""

    def __init__(self, device='cuda:0'):
        import torch
        from . import _lib
        self._torch, self._L = torch, _lib
        self.lib = _lib.load()
        self.device = torch.device(device)
        idx = self.device.index if self.device.index is not None else 0
        self._h = self.lib.e3gnn_nlist_create(idx)
        if not self._h:
            raise _lib.E3GNNError(self.lib.e3gnn_last_error().decode())

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            self.lib.e3gnn_nlist_free(h)

    def __call__(self, pos, cell, cutoff, pbc=(True, True, True)):
        import ctypes
        torch, L = self._torch, self._L
        dev = self.device
        pos = torch.as_tensor(pos).to(dev, torch.float64).contiguous()
        n = int(pos.shape[0])
        cellh = (ctypes.c_double * 9)(*np.asarray(cell, dtype=np.float64).reshape(-1).tolist()) \
            if cell is not None else (ctypes.c_double * 9)()
        pbch = (ctypes.c_int * 3)(*[int(bool(p)) for p in pbc])
        ne = ctypes.c_int64()
        s = torch.cuda.current_stream(dev).cuda_stream
        L.check(self.lib.e3gnn_nlist_build(self._h, n, pos.data_ptr(), cellh, pbch,
                                           float(cutoff), ctypes.byref(ne), s))
        E = ne.value
        center = torch.empty(E, dtype=torch.int32, device=dev)
        nbr = torch.empty(E, dtype=torch.int32, device=dev)
        shift = torch.empty(E, 3, dtype=torch.int32, device=dev)
        vec = torch.empty(E, 3, dtype=torch.float32, device=dev)
        L.check(self.lib.e3gnn_nlist_fetch(self._h, center.data_ptr(), nbr.data_ptr(),
                                           shift.data_ptr(), vec.data_ptr(), s))
        return center, nbr, shift, vec

    def batch(self, positions_list, cells_list, cutoff, pbc_list=None):
        """The graphs of B structures in one build (``e3gnn_nlist_batch_*``):
        ``batch_neighbor_list`` integer for integer.

        ``positions_list``: B arrays [n_s, 3]; ``cells_list``: B cells (None
        for an isolated structure); ``pbc_list``: B triples (default: all
        periodic).  Returns device tensors ``(center int32 [E], nbr int32 [E],
        shift int32 [E, 3], vec float32 [E, 3], atom_ptr int32 [B + 1],
        edge_ptr int64 [B + 1])``; ``center`` / ``nbr`` are rows of the
        concatenated batch.

        Limits: every structure has at least one atom and is fully periodic
        or fully isolated (anything else raises ``E3GNNError`` naming the
        structure; ``neighbor_list`` covers those on the host), at most 512
        neighbours per centre, shifts within +-1024 cells.  The outputs are
        bitwise reproducible."""
        import ctypes
        torch, L = self._torch, self._L
        dev = self.device
        B = len(positions_list)
        if pbc_list is None:
            pbc_list = [(True, True, True)] * B
        if len(cells_list) != B or len(pbc_list) != B:
            raise ValueError('positions_list, cells_list and pbc_list must have one entry per '
                             'structure')
        pos = [np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in positions_list]
        atom_ptr = np.zeros(B + 1, dtype=np.int64)
        np.cumsum([len(p) for p in pos], out=atom_ptr[1:])
        n = int(atom_ptr[-1])
        cells = np.zeros((max(B, 1), 9), dtype=np.float64)
        for k, c in enumerate(cells_list):
            if c is not None:
                cells[k] = np.asarray(c, dtype=np.float64).reshape(-1)
        periodic = np.array([sum(int(bool(p)) << d for d, p in enumerate(pbc))
                             for pbc in pbc_list], dtype=np.int32)
        posd = torch.as_tensor(np.concatenate(pos) if B else np.zeros((0, 3))).to(dev).contiguous()
        ne = ctypes.c_int64()
        s = torch.cuda.current_stream(dev).cuda_stream
        L.check(self.lib.e3gnn_nlist_batch_build(
            self._h, B, atom_ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), posd.data_ptr(),
            cells.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            periodic.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), float(cutoff),
            ctypes.byref(ne), s))
        E = ne.value
        center = torch.empty(E, dtype=torch.int32, device=dev)
        nbr = torch.empty(E, dtype=torch.int32, device=dev)
        shift = torch.empty(E, 3, dtype=torch.int32, device=dev)
        vec = torch.empty(E, 3, dtype=torch.float32, device=dev)
        edge_ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
        L.check(self.lib.e3gnn_nlist_batch_fetch(self._h, center.data_ptr(), nbr.data_ptr(),
                                                 shift.data_ptr(), vec.data_ptr(),
                                                 edge_ptr.data_ptr(), s))
        return (center, nbr, shift, vec,
                torch.as_tensor(atom_ptr.astype(np.int32), device=dev), edge_ptr)

    def rank_graph(self, pos, cell, cutoff, owner, rank, world, pbc=(True, True, True)):
        """One rank's graph of a spatial decomposition, built on the device
        (``e3gnn_nlist_rank_*``): the rows, ghosts and edges of
        ``parallel.build_rank_graph``, integer for integer.

        ``owner``: int32 [n] owner rank of every atom, an input (the device
        does not recompute the bricks).  Returns a dict of device tensors
        ``owned`` int32 [n_local] and ``ghosts`` int32 [n_ghost] (global ids;
        interior rows first, ghosts by (owner, id)), ``recv_counts`` int64
        [world], ``center`` / ``nbr`` int32 [E] (local rows), ``shift`` int32
        [E, 3], ``vec`` float32 [E, 3], and the host integers ``n_local``,
        ``n_interior``, ``n_ghost``.

        Limits: all three dimensions periodic (anything else raises
        ``E3GNNError``; the host builder serves those cases), at most 512
        neighbours per centre (``NL_MAXD``), shifts within +-1024 cells,
        ``world`` <= 256.  The outputs are bitwise reproducible."""
        import ctypes
        torch, L = self._torch, self._L
        dev = self.device
        if not all(bool(p) for p in pbc):
            raise L.E3GNNError('e3gnn error 1: device rank graph: all three dimensions must be '
                               'periodic (parallel.build_rank_graph covers the rest on the host)')
        pos = torch.as_tensor(pos).to(dev, torch.float64).contiguous()
        n = int(pos.shape[0])
        owner = torch.as_tensor(owner).to(dev, torch.int32).contiguous()
        if owner.shape != (n,):
            raise ValueError('owner must have one entry per atom')
        cellh = (ctypes.c_double * 9)(*np.asarray(cell, dtype=np.float64).reshape(-1).tolist())
        cnt = [ctypes.c_int64() for _ in range(4)]
        s = torch.cuda.current_stream(dev).cuda_stream
        L.check(self.lib.e3gnn_nlist_rank_build(self._h, n, pos.data_ptr(), cellh, float(cutoff),
                                                owner.data_ptr(), int(rank), int(world),
                                                *[ctypes.byref(c) for c in cnt], s))
        nl, ni, ng, E = (c.value for c in cnt)
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)  # noqa: E731
        out = {'owned': i32(nl), 'ghosts': i32(ng),
               'recv_counts': torch.empty(int(world), dtype=torch.int64, device=dev),
               'center': i32(E), 'nbr': i32(E), 'shift': i32(E, 3),
               'vec': torch.empty(E, 3, dtype=torch.float32, device=dev)}
        L.check(self.lib.e3gnn_nlist_rank_fetch(
            self._h, *[out[k].data_ptr() for k in ('owned', 'ghosts', 'recv_counts', 'center',
                                                   'nbr', 'shift', 'vec')], s))
        out.update(n_local=nl, n_interior=ni, n_ghost=ng)
        return out


class ListFilter:
    """Cutoff filter over a neighbour list a host code already built
    (libe3gnn_hip.so ``e3gnn_plist_*``): the loop of the serial LAMMPS pair
    style on the device, for callers who hold a LAMMPS list (through the
    ``lammps`` module, say).

    ``set(row_atom, cand_ptr, cand, atom_row, neighmask)`` uploads the list
    (host arrays): graph row t has the centre atom ``row_atom[t]`` and the
    candidates ``cand[cand_ptr[t]:cand_ptr[t + 1]]`` (raw entries, masked with
    ``neighmask``); ``atom_row[a]`` is the graph row of atom index a (owned or
    ghost).  A list that breaks a rule raises ``E3GNNError`` naming the row.

    ``__call__(x, cutoff)`` (any number of times after one ``set``; ``x`` f64
    [n_total, 3]) returns device tensors ``(center int32 [E], nbr int32 [E],
    vec float32 [E, 3])``: every candidate within the cutoff, rows one after
    the other, each row in the list's order -- bitwise the host loop's edges.

    ``set_rank`` / ``check_rank`` / ``rank`` are the same for one rank of a
    decomposed run (``e3gnn_plist_set_rank`` / ``_check_rank_list`` /
    ``_rank_build`` + ``_rank_fetch``): ghosts of tags the rank does not own
    get graph rows in first-seen order, as the parallel pair style gives them."""

    def __init__(self, device='cuda:0'):
        import torch
        from . import _lib
        self._torch, self._L = torch, _lib
        self.lib = _lib.load()
        self.device = torch.device(device)
        idx = self.device.index if self.device.index is not None else 0
        self._h = self.lib.e3gnn_plist_create(idx)
        if not self._h:
            raise _lib.E3GNNError(self.lib.e3gnn_last_error().decode())
        self.n_total = 0

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            self.lib.e3gnn_plist_free(h)

    def set(self, row_atom, cand_ptr, cand, atom_row, neighmask=0x1FFFFFFF):
        import ctypes
        i32, i64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
        row_atom = np.ascontiguousarray(row_atom, dtype=np.int32)
        cand_ptr = np.ascontiguousarray(cand_ptr, dtype=np.int64)
        cand = np.ascontiguousarray(cand, dtype=np.int32)
        atom_row = np.ascontiguousarray(atom_row, dtype=np.int32)
        if cand_ptr.shape != (len(row_atom) + 1,) or (len(cand_ptr) and cand_ptr[-1] != len(cand)):
            raise ValueError('cand_ptr must have one entry per row plus one and end at len(cand)')
        s = self._torch.cuda.current_stream(self.device).cuda_stream
        self.n_total = 0
        self._L.check(self.lib.e3gnn_plist_set(
            self._h, len(row_atom), len(atom_row), row_atom.ctypes.data_as(i32),
            cand_ptr.ctypes.data_as(i64), cand.ctypes.data_as(i32), int(neighmask),
            atom_row.ctypes.data_as(i32), s))
        self.n_total = len(atom_row)

    def __call__(self, x, cutoff):
        import ctypes
        torch, dev = self._torch, self.device
        x = torch.as_tensor(x).to(dev, torch.float64).contiguous()
        if self.n_total and x.shape != (self.n_total, 3):
            raise ValueError('x must have one row per atom of the list (owned and ghost)')
        ne = ctypes.c_int64()
        s = torch.cuda.current_stream(dev).cuda_stream
        self._L.check(self.lib.e3gnn_plist_build(self._h, x.data_ptr(), float(cutoff),
                                                 ctypes.byref(ne), s))
        E = ne.value
        center = torch.empty(E, dtype=torch.int32, device=dev)
        nbr = torch.empty(E, dtype=torch.int32, device=dev)
        vec = torch.empty(E, 3, dtype=torch.float32, device=dev)
        self._L.check(self.lib.e3gnn_plist_fetch(self._h, center.data_ptr(), nbr.data_ptr(),
                                                 vec.data_ptr(), s))
        # the fill pass reads x in stream order: keep it alive until then
        x.record_stream(torch.cuda.current_stream(dev))
        return center, nbr, vec

    @staticmethod
    def _rank_arrays(row_atom, cand_ptr, cand, atom_class):
        row_atom = np.ascontiguousarray(row_atom, dtype=np.int32)
        cand_ptr = np.ascontiguousarray(cand_ptr, dtype=np.int64)
        cand = np.ascontiguousarray(cand, dtype=np.int32)
        atom_class = np.ascontiguousarray(atom_class, dtype=np.int32)
        if cand_ptr.shape != (len(row_atom) + 1,) or (len(cand_ptr) and cand_ptr[-1] != len(cand)):
            raise ValueError('cand_ptr must have one entry per row plus one and end at len(cand)')
        return row_atom, cand_ptr, cand, atom_class

    def check_rank(self, row_atom, cand_ptr, cand, atom_class, n_class, neighmask=0x1FFFFFFF):
        """The check of ``set_rank`` alone, on the host (no device work): raises
        ``E3GNNError`` naming the atom, row or class that breaks a rule."""
        import ctypes
        i32, i64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
        row_atom, cand_ptr, cand, atom_class = self._rank_arrays(row_atom, cand_ptr, cand, atom_class)
        self._L.check(self.lib.e3gnn_plist_check_rank_list(
            len(row_atom), len(atom_class), row_atom.ctypes.data_as(i32),
            cand_ptr.ctypes.data_as(i64), cand.ctypes.data_as(i32), int(neighmask),
            atom_class.ctypes.data_as(i32), int(n_class)))

    def set_rank(self, row_atom, cand_ptr, cand, atom_class, n_class, neighmask=0x1FFFFFFF):
        """Uploads the list of one rank of a decomposed run (the parallel LAMMPS
        pair style's): as ``set``, with ``atom_class[a]`` in place of
        ``atom_row`` -- the row in [0, n) of an owned atom and of every ghost
        carrying an owned atom's tag, ``n + k`` for a ghost whose tag the rank
        does not own, k in [0, n_class) numbering those tags in any order.  It
        replaces a list given to ``set``, and the other way round."""
        import ctypes
        i32, i64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
        row_atom, cand_ptr, cand, atom_class = self._rank_arrays(row_atom, cand_ptr, cand, atom_class)
        s = self._torch.cuda.current_stream(self.device).cuda_stream
        self.n_total = 0
        self._L.check(self.lib.e3gnn_plist_set_rank(
            self._h, len(row_atom), len(atom_class), row_atom.ctypes.data_as(i32),
            cand_ptr.ctypes.data_as(i64), cand.ctypes.data_as(i32), int(neighmask),
            atom_class.ctypes.data_as(i32), int(n_class), s))
        self.n_total = len(atom_class)

    def rank(self, x, cutoff):
        """After ``set_rank`` (any number of times): the rank graph of the host
        loop of the parallel pair style, bit for bit.  Returns a dict of device
        tensors ``center`` / ``nbr`` int32 [E], ``vec`` float32 [E, 3] and
        ``ghost_atom`` int32 [n_ghost], with ``n_edges`` and ``n_ghost``.  Rows
        [0, n) are the list rows; a non-owned class with an edge has the row
        n + r, r counting such classes in the order of their first edge, and
        ``ghost_atom[r]`` is the atom index of that first edge."""
        import ctypes
        torch, dev = self._torch, self.device
        x = torch.as_tensor(x).to(dev, torch.float64).contiguous()
        if self.n_total and x.shape != (self.n_total, 3):
            raise ValueError('x must have one row per atom of the list (owned and ghost)')
        ne, ng = ctypes.c_int64(), ctypes.c_int64()
        s = torch.cuda.current_stream(dev).cuda_stream
        self._L.check(self.lib.e3gnn_plist_rank_build(self._h, x.data_ptr(), float(cutoff),
                                                      ctypes.byref(ne), ctypes.byref(ng), s))
        E, G = ne.value, ng.value
        out = {'center': torch.empty(E, dtype=torch.int32, device=dev),
               'nbr': torch.empty(E, dtype=torch.int32, device=dev),
               'vec': torch.empty(E, 3, dtype=torch.float32, device=dev),
               'ghost_atom': torch.empty(G, dtype=torch.int32, device=dev)}
        self._L.check(self.lib.e3gnn_plist_rank_fetch(
            self._h, *[out[k].data_ptr() for k in ('center', 'nbr', 'vec', 'ghost_atom')], s))
        x.record_stream(torch.cuda.current_stream(dev))
        out.update(n_edges=E, n_ghost=G)
        return out
