"""The padding contract of the device loader stated in numpy
(TEST INFRASTRUCTURE): what ``e3gnn_dataset_collate`` must write, bit for bit.

``graphs``: host ``train.labeled_graph``-shaped dicts of the real structures,
in batch order.  The batch has ``slots`` structure slots, ``atom_cap`` atom
rows and ``edge_cap`` edges:

* real structures fill the first slots, concatenated as ``train.collate`` does
  (f32 values, edge rows offset to batch rows);
* every other slot is a dummy structure: the first dummy slots hold one atom,
  the last one the rest of the rows; type 0, NaN force / energy / stress
  labels, volume 1;
* the edges past the real ones are self edges of dummy atoms, ``edge_vec``
  (r_pad, 0, 0), shift 0, dealt out in blocks of ceil(padded / dummy atoms)
  over the dummy atoms in row order (centres non-decreasing).
"""
import numpy as np

KEYS = ('x', 'edge_index', 'edge_vec', 'pbc_shift', 'force_of_atoms', 'batch', 'num_atoms',
        'cell_volume', 'total_energy', 'stress')


def _np(t, dtype):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t).astype(dtype)


def padded_batch(graphs, slots, atom_cap, edge_cap, r_pad, with_shift=False):
    n_real = len(graphs)
    n_dummy = slots - n_real
    assert n_dummy >= 1
    natoms = [int(_np(g['x'], np.int64).shape[0]) for g in graphs]
    nedges = [int(_np(g['edge_index'], np.int64).shape[1]) for g in graphs]
    A, E = sum(natoms), sum(nedges)
    D, P = atom_cap - A, edge_cap - E
    assert D >= n_dummy and P >= 0
    nan = np.float32(np.nan)
    out = {'x': np.zeros(atom_cap, np.int64),
           'edge_index': np.zeros((2, edge_cap), np.int64),
           'edge_vec': np.zeros((edge_cap, 3), np.float32),
           'force_of_atoms': np.full((atom_cap, 3), nan, np.float32),
           'batch': np.zeros(atom_cap, np.int64),
           'num_atoms': np.zeros(slots, np.int64),
           'cell_volume': np.ones(slots, np.float32),
           'total_energy': np.full(slots, nan, np.float32),
           'stress': np.full((slots, 6), nan, np.float32)}
    if with_shift:
        out['pbc_shift'] = np.zeros((edge_cap, 3), np.float32)
    a = e = 0
    for s, g in enumerate(graphs):
        n, m = natoms[s], nedges[s]
        out['x'][a:a + n] = _np(g['x'], np.int64)
        out['force_of_atoms'][a:a + n] = _np(g['force_of_atoms'], np.float32)
        out['batch'][a:a + n] = s
        out['edge_index'][:, e:e + m] = _np(g['edge_index'], np.int64) + a
        out['edge_vec'][e:e + m] = _np(g['edge_vec'], np.float32)
        if with_shift:
            out['pbc_shift'][e:e + m] = _np(g['pbc_shift'], np.float32)
        out['num_atoms'][s] = n
        out['cell_volume'][s] = _np(g['cell_volume'], np.float32)
        out['total_energy'][s] = _np(g['total_energy'], np.float32)
        out['stress'][s] = _np(g['stress'], np.float32).reshape(6)
        a, e = a + n, e + m
    # dummy slots: one atom each, the last takes the rest
    for j in range(n_dummy):
        n = 1 if j < n_dummy - 1 else D - (n_dummy - 1)
        out['batch'][a:a + n] = n_real + j
        out['num_atoms'][n_real + j] = n
        a += n
    assert a == atom_cap
    if P:
        block = -(-P // D)
        rows = A + np.arange(P) // block
        out['edge_index'][:, E:] = rows
        out['edge_vec'][E:, 0] = np.float32(r_pad)
    return out


def same_bits(a, b):
    """equal including the NaN payloads"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
