"""Device-resident training data: the dataset on the GPU and a loader whose
batches fall into a small, fixed set of shapes.

Mirrors the host side of the reference's training input:
  graph list of a dataset      sevenn/train/dataload.py:71-140  -> DeviceDataset
  DataLoader + PyG Collater    sevenn/train/collate.py,
                               rehearsal/train_rehearsal.py:20-71 -> DeviceLoader

A ``DeviceLoader`` batch has the keys, dtypes and layouts of
``train.collate(graphs, device, dtype=torch.float32)`` (without ``pos``), padded
to one of the loader's shapes: ``batch_size + 1`` structure slots, the real
structures first, every other slot a dummy structure (type-0 atoms, NaN
labels, volume 1) whose atoms carry the padded edges -- self edges of length
exactly the cutoff, where the cutoff polynomial and its first derivative are
0.  The losses drop NaN labels and structures interact only through the loss,
so a padded batch trains like the unpadded one, and every step of an epoch
replays one of a few captured HIP graphs (``train.GraphedRehearsalStep``).
"""
import ctypes
import re

import numpy as np
import torch

from . import _keys as KEY
from . import _lib, train

MAX_SLOTS = 64   # COLLATE_MAX_SLOTS (csrc/collate.h)


def _type_index(types, type_map_or_types):
    """type indices of one structure: as given (None), through a mapping, or
    by position in a sequence (the model's chemical symbols)"""
    if type_map_or_types is None:
        return np.asarray(types, dtype=np.int32)
    if isinstance(type_map_or_types, dict):
        return np.array([type_map_or_types[t] for t in types], dtype=np.int32)
    seq = list(type_map_or_types)
    return np.array([seq.index(t) for t in types], dtype=np.int32)


class DeviceDataset:
    """A labelled dataset held on the GPU as concatenated arrays (the C ABI's
    ``e3gnn_dataset``): per atom ``type`` int32 and the force label, per edge
    ``edge_center`` / ``edge_nbr`` int32 (rows relative to the structure's
    first atom), ``edge_vec`` f32 and optionally the image shift, per structure
    energy, stress [6] and volume.  The tensors are owned by this object."""

    def __init__(self, device, cutoff, atom_ptr, edge_ptr, arrays, max_degree):
        self.device = torch.device(device)
        self.cutoff = float(cutoff)
        self.atom_ptr = np.ascontiguousarray(atom_ptr, dtype=np.int64)
        self.edge_ptr = np.ascontiguousarray(edge_ptr, dtype=np.int64)
        self.arrays = arrays          # name -> device tensor (kept alive here)
        self.max_degree = int(max_degree)
        self.lib = _lib.load()
        a = _lib.DatasetArrays(**{k: (v.data_ptr() if v is not None and v.numel() else None)
                                  for k, v in arrays.items()})
        idx = self.device.index if self.device.index is not None else 0
        p64 = ctypes.POINTER(ctypes.c_int64)
        self._h = self.lib.e3gnn_dataset_create(
            idx, len(self.atom_ptr) - 1, self.atom_ptr.ctypes.data_as(p64),
            self.edge_ptr.ctypes.data_as(p64), ctypes.byref(a))
        if not self._h:
            raise _lib.E3GNNError(self.lib.e3gnn_last_error().decode())

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            self.lib.e3gnn_dataset_free(h)

    @classmethod
    def from_structures(cls, structures, cutoff, type_map_or_types=None, device='cuda:0',
                        max_atoms_per_build=1 << 16, with_shift=False):
        """Build the dataset from ``structures``, a sequence of ``(pos, cell,
        types[, energy[, force[, stress]]])`` with the label conventions of
        ``train.labeled_graph`` (a missing or None label is NaN; stress [6] in
        the model's output order xx,yy,zz,xy,yz,zx).

        The graphs come from ``DeviceNeighborList.batch`` in chunks of at most
        ``max_atoms_per_build`` atoms (the edges, order and f32 edge vectors of
        the host list).  Every structure is periodic (a cell is required) with
        at most 512 neighbours per centre; anything else raises, naming the
        structure's index.  ``type_map_or_types``: None (``types`` are type
        indices), a dict, or the sequence of the model's chemical symbols.
        ``with_shift``: also keep the image shifts (batches then carry
        ``pbc_shift``; the model reads ``edge_vec`` only)."""
        from .neighbor import DeviceNeighborList
        dev = torch.device(device)
        S = len(structures)
        if S < 1:
            raise ValueError('a dataset needs at least one structure')
        pos, cells, types = [], [], []
        energy = np.full(S, np.nan, dtype=np.float32)
        stress = np.full((S, 6), np.nan, dtype=np.float32)
        volume = np.zeros(S, dtype=np.float32)
        forces = []
        for k, st in enumerate(structures):
            st = tuple(st) + (None,) * (6 - len(st))
            p = np.asarray(st[0], dtype=np.float64).reshape(-1, 3)
            if st[1] is None:
                raise ValueError(f'structure {k}: no cell (training structures are periodic)')
            c = np.asarray(st[1], dtype=np.float64).reshape(3, 3)
            t = _type_index(st[2], type_map_or_types)
            if len(p) < 1 or len(t) != len(p):
                raise ValueError(f'structure {k}: {len(p)} positions, {len(t)} types')
            pos.append(p)
            cells.append(c)
            types.append(t)
            volume[k] = abs(float(np.linalg.det(c)))
            if st[3] is not None:
                energy[k] = float(st[3])
            f = np.full((len(p), 3), np.nan, dtype=np.float32) if st[4] is None \
                else np.asarray(st[4], dtype=np.float64).reshape(len(p), 3).astype(np.float32)
            forces.append(f)
            if st[5] is not None:
                stress[k] = np.asarray(st[5], dtype=np.float64).reshape(6)
        natoms = np.array([len(p) for p in pos], dtype=np.int64)
        atom_ptr = np.concatenate([[0], np.cumsum(natoms)])
        # chunks of whole structures, at most max_atoms_per_build atoms each
        chunks, lo = [], 0
        while lo < S:
            hi = lo + 1
            while hi < S and atom_ptr[hi + 1] - atom_ptr[lo] <= max_atoms_per_build:
                hi += 1
            chunks.append((lo, hi))
            lo = hi
        dnl = DeviceNeighborList(dev)
        cen, nbr, vec, shf, nedges, max_degree = [], [], [], [], [], 0
        for lo, hi in chunks:
            try:
                c, n, s, v, ap, ep = dnl.batch(pos[lo:hi], cells[lo:hi], cutoff)
            except _lib.E3GNNError as err:
                msg = re.sub(r'structure (\d+)', lambda m: f'structure {lo + int(m.group(1))}',
                             str(err))
                raise _lib.E3GNNError(msg) from None
            cnt = (ep[1:] - ep[:-1])
            base = torch.repeat_interleave(ap[:-1].long(), cnt).to(torch.int32)
            if c.numel():
                max_degree = max(max_degree, int(torch.bincount(c.long()).max()))
            cen.append(c - base)
            nbr.append(n - base)
            vec.append(v)
            if with_shift:
                shf.append(s.to(torch.float32))
            nedges.append(cnt.cpu().numpy())
        edge_ptr = np.concatenate([[0], np.cumsum(np.concatenate(nedges))])
        t32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)   # noqa: E731
        arrays = {'type': t32(np.concatenate(types)), 'force': t32(np.concatenate(forces)),
                  'edge_center': torch.cat(cen).contiguous(), 'edge_nbr': torch.cat(nbr).contiguous(),
                  'edge_vec': torch.cat(vec).contiguous(),
                  'shift': torch.cat(shf).contiguous() if with_shift else None,
                  'energy': t32(energy), 'stress': t32(stress), 'volume': t32(volume)}
        return cls(dev, cutoff, atom_ptr, edge_ptr, arrays, max_degree)

    def __len__(self):
        return len(self.atom_ptr) - 1

    @property
    def has_shift(self):
        return self.arrays['shift'] is not None

    def sizes(self):
        """host (atoms int64 [S], edges int64 [S])"""
        return np.diff(self.atom_ptr), np.diff(self.edge_ptr)

    def graph(self, k):
        """structure ``k`` as a host ``train.labeled_graph``-shaped dict (f32
        values, no ``pos``): for tests and debugging"""
        a0, a1 = int(self.atom_ptr[k]), int(self.atom_ptr[k + 1])
        e0, e1 = int(self.edge_ptr[k]), int(self.edge_ptr[k + 1])
        A = self.arrays
        g = {KEY.NODE_FEATURE: A['type'][a0:a1].long().cpu(),
             KEY.EDGE_IDX: torch.stack([A['edge_center'][e0:e1], A['edge_nbr'][e0:e1]]).long().cpu(),
             KEY.EDGE_VEC: A['edge_vec'][e0:e1].cpu(),
             KEY.CELL_VOLUME: A['volume'][k].cpu(),
             KEY.NUM_ATOMS: torch.tensor(a1 - a0),
             KEY.ENERGY: A['energy'][k].cpu(),
             KEY.FORCE: A['force'][a0:a1].cpu(),
             KEY.STRESS: A['stress'][k].cpu().reshape(1, 6)}
        if self.has_shift:
            g[KEY.CELL_SHIFT] = A['shift'][e0:e1].cpu()
        return g

    def collate_into(self, index, slots, out):
        """``e3gnn_dataset_collate`` of the structures ``index`` into the batch
        dict ``out`` (device tensors of one shape, see ``empty_batch``) on the
        current stream; returns at once"""
        idx = np.ascontiguousarray(index, dtype=np.int64)
        b = _lib.BatchArrays(**{k: out[k].data_ptr() for k in _BATCH_FIELDS if k in out})
        s = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self.lib.e3gnn_dataset_collate(
            self._h, len(idx), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), int(slots),
            int(out[KEY.NODE_FEATURE].shape[0]), int(out[KEY.EDGE_IDX].shape[1]),
            self.max_degree, float(np.float32(self.cutoff)), ctypes.byref(b), s))

    def empty_batch(self, slots, atom_cap, edge_cap):
        """uninitialised buffers of one batch shape"""
        dev = self.device
        f32 = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)   # noqa: E731
        i64 = lambda *sh: torch.empty(*sh, dtype=torch.int64, device=dev)     # noqa: E731
        out = {KEY.NODE_FEATURE: i64(atom_cap), KEY.EDGE_IDX: i64(2, edge_cap),
               KEY.EDGE_VEC: f32(edge_cap, 3), KEY.FORCE: f32(atom_cap, 3), KEY.BATCH: i64(atom_cap),
               KEY.NUM_ATOMS: i64(slots), KEY.CELL_VOLUME: f32(slots), KEY.ENERGY: f32(slots),
               KEY.STRESS: f32(slots, 6)}
        if self.has_shift:
            out[KEY.CELL_SHIFT] = f32(edge_cap, 3)
        return out


# e3gnn_batch_arrays fields are named by the batch keys
_BATCH_FIELDS = (KEY.NODE_FEATURE, KEY.EDGE_IDX, KEY.EDGE_VEC, KEY.CELL_SHIFT, KEY.FORCE, KEY.BATCH,
                 KEY.NUM_ATOMS, KEY.CELL_VOLUME, KEY.ENERGY, KEY.STRESS)


def plan_shapes(atoms, edges, batch_size, n_edge_buckets, max_degree):
    """The complete set of batch shapes of a loader (pure host logic).

    ``atoms`` / ``edges``: per-structure counts.  Returns ``(atom_cap,
    edge_caps)``: at most ``n_edge_buckets`` increasing edge capacities that
    evenly divide the span from the sum of the ``batch_size`` smallest edge
    counts to the sum of the ``batch_size`` largest (a batch takes the smallest
    that holds it), and one atom capacity: the most real atoms a batch can
    have plus enough dummy atoms that the most padded edges a batch can need,
    dealt out evenly, stay within ``max_degree`` per dummy atom -- for the
    full batches and for the short last one, which has fewer real atoms and
    more padding."""
    atoms = np.sort(np.asarray(atoms, dtype=np.int64))
    edges = np.sort(np.asarray(edges, dtype=np.int64))
    S, bs, nb = len(atoms), int(batch_size), int(n_edge_buckets)
    if bs < 1 or bs + 1 > MAX_SLOTS:
        raise ValueError(f'batch_size must be in [1, {MAX_SLOTS - 1}]')
    if nb < 1:
        raise ValueError('n_edge_buckets must be at least 1')
    full = min(bs, S)
    e_lo, e_hi = int(edges[:full].sum()), int(edges[-full:].sum())
    caps = sorted({e_lo + -((e_lo - e_hi) * i // nb) for i in range(1, nb + 1)})   # ceil
    assert caps[-1] == e_hi

    def dummy_atoms(m, need):
        """dummy atoms a batch of m real structures may need: one per dummy
        slot, and the worst padding of a feasible edge total over max_degree"""
        lo, hi = int(edges[:m].sum()), int(edges[-m:].sum()) if m else 0
        pad, prev = 0, -1
        for c in caps:
            if hi > prev and lo <= c:      # totals in (prev, c] are possible
                pad = max(pad, c - max(prev + 1, lo))
            prev = c
        if pad and max_degree < 1:
            raise ValueError('padded edges need a positive degree cap')
        return max(need, -(-pad // max_degree) if pad else 0)

    rem = S % bs if S >= bs else S
    atom_cap = 0
    for m in {full if S >= bs else 0, rem} - {0}:
        atom_cap = max(atom_cap, int(atoms[-m:].sum()) + dummy_atoms(m, bs + 1 - m))
    return atom_cap, caps


class DeviceLoader:
    """Iterable of padded training batches over a ``DeviceDataset``.

    Batches have ``batch_size + 1`` structure slots: the real structures in the
    loader's order, then dummy slots (always at least one; the short last
    batch of an epoch -- ``drop_last=False`` -- has several).  All batches
    share one atom capacity and take the smallest of at most
    ``n_edge_buckets`` edge capacities that holds their edges (``shapes``, fixed
    at construction), so the loader yields at most ``n_edge_buckets`` distinct
    tensor signatures over any number of epochs.

    ``shuffle=True``: epoch k (the k-th ``iter()`` of this loader, from 0) has
    the order ``np.random.default_rng(seed + k).permutation(S)`` (``order(k)``);
    otherwise the dataset order.  ``pad_fraction``: padded edges over real
    edges of the batches yielded since the last ``iter()``.

    The loader owns two sets of output buffers per shape and alternates
    between them: a batch stays valid until the next-but-one batch is
    requested, no longer.  Every batch is assembled on the current stream by
    one kernel launch (no host synchronisation) and is marked with
    ``train.mark_edges_sorted``."""

    def __init__(self, dataset, batch_size, shuffle=True, seed=0, n_edge_buckets=2):
        self.dataset = dataset
        self.batch_size, self.shuffle, self.seed = int(batch_size), bool(shuffle), int(seed)
        self.slots = self.batch_size + 1
        self._atoms, self._edges = dataset.sizes()
        self.atom_cap, self.edge_caps = plan_shapes(self._atoms, self._edges, self.batch_size,
                                                    n_edge_buckets, dataset.max_degree)
        self.shapes = [(self.atom_cap, c) for c in self.edge_caps]
        self._bufs = {}      # edge capacity -> [two batch dicts, next to use]
        self.epoch = 0       # epochs started (iter() calls)
        self.padded_edges = self.real_edges = 0

    def __len__(self):
        return -(-len(self.dataset) // self.batch_size)

    def order(self, epoch):
        S = len(self.dataset)
        if not self.shuffle:
            return np.arange(S)
        return np.random.default_rng(self.seed + int(epoch)).permutation(S)

    def batch_indices(self, epoch):
        """the index lists of epoch ``epoch``'s batches, in order"""
        o, bs = self.order(epoch), self.batch_size
        return [o[i:i + bs] for i in range(0, len(o), bs)]

    def capacity_of(self, index):
        """the edge capacity the batch of structures ``index`` takes"""
        e = int(self._edges[np.asarray(index, dtype=np.int64)].sum())
        return next(c for c in self.edge_caps if c >= e)

    @property
    def pad_fraction(self):
        return self.padded_edges / self.real_edges if self.real_edges else 0.0

    def _next_buffers(self, cap):
        ent = self._bufs.get(cap)
        if ent is None:
            ds = self.dataset
            ent = self._bufs[cap] = [[ds.empty_batch(self.slots, self.atom_cap, cap)
                                      for _ in range(2)], 0]
        out = ent[0][ent[1]]
        ent[1] ^= 1
        return out

    def __iter__(self):
        epoch, self.epoch = self.epoch, self.epoch + 1
        self.padded_edges = self.real_edges = 0
        for index in self.batch_indices(epoch):
            cap = self.capacity_of(index)
            out = self._next_buffers(cap)
            self.dataset.collate_into(index, self.slots, out)
            real = int(self._edges[index].sum())
            self.real_edges += real
            self.padded_edges += cap - real
            batch = dict(out)
            train.mark_edges_sorted(batch)
            yield batch
