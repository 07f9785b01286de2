"""Batched graph build and dataset inference, the parts that need no GPU: the
new C-ABI entries are exported and refuse bad arguments before any device
work, ``batch_neighbor_list`` is the per-structure host list with offsets,
``inference.errors`` against hand-computed numbers, ``group_batches`` as pure
logic."""
import ctypes

import numpy as np
import pytest

from sevennet_finetuning_amd import _lib
from sevennet_finetuning_amd.inference import KBAR, errors, group_batches
from sevennet_finetuning_amd.neighbor import batch_neighbor_list, neighbor_list
from sevennet_finetuning_amd.structures import si_diamond

ERR_ARG = 1
NEW = ('e3gnn_nlist_batch_build', 'e3gnn_nlist_batch_fetch', 'e3gnn_energy_forces_batch',
       'e3gnn_segment_sum')


def test_batch_entries_are_exported_and_bound():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.e3gnn_abi_version() == 1


def _build(lib, h, B, atom_ptr, pos, cells, periodic, cutoff):
    ap = (ctypes.c_int64 * len(atom_ptr))(*atom_ptr) if atom_ptr is not None else None
    ce = (ctypes.c_double * len(cells))(*cells) if cells is not None else None
    pe = (ctypes.c_int32 * len(periodic))(*periodic) if periodic is not None else None
    ne = ctypes.c_int64(-1)
    rc = lib.e3gnn_nlist_batch_build(h, B, ap, pos, ce, pe, cutoff, ctypes.byref(ne), None)
    return rc, lib.e3gnn_last_error().decode()


def test_batch_build_argument_rules():
    """Every rule returns E3GNN_ERR_ARG with its message.  The handle and the
    device pointer are fakes that are never dereferenced: a HIP call (or any
    use of the handle) before the checks would crash or return E3GNN_ERR_HIP
    on a machine without a GPU."""
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)
    cells = [10.0, 0, 0, 0, 10.0, 0, 0, 0, 10.0] * 2
    good = dict(B=2, atom_ptr=[0, 3, 5], pos=fake, cells=cells, periodic=[7, 0], cutoff=5.0)

    def refused(h=fake, **change):
        rc, msg = _build(lib, h, **{**good, **change})
        assert rc == ERR_ARG, (rc, msg)
        return msg

    assert 'null neighbour-list handle' in refused(h=None)
    assert 'number of structures' in refused(B=0, atom_ptr=[0])
    assert 'number of structures' in refused(B=-1)
    assert 'null atom_ptr' in refused(atom_ptr=None)
    assert 'null positions' in refused(pos=None)
    assert 'null periodic' in refused(periodic=None)
    assert 'null cells' in refused(cells=None)
    assert 'atom_ptr[0]' in refused(atom_ptr=[1, 3, 5])
    assert 'structure 1 is empty' in refused(atom_ptr=[0, 3, 3])       # an empty range
    assert 'structure 1 is empty' in refused(atom_ptr=[0, 3, 2])       # non-monotonic
    assert 'structure 0 is empty' in refused(atom_ptr=[0, 0, 5])
    assert 'out of range' in refused(atom_ptr=[0, 3, 1 << 30])
    assert 'cutoff must be positive' in refused(cutoff=0.0)
    assert 'cutoff must be positive' in refused(cutoff=-1.0)
    assert 'cutoff must be positive' in refused(cutoff=float('nan'))
    # mixed periodicity stays refused on the device list, and names the structure
    msg = refused(periodic=[7, 3])
    assert 'structure 1' in msg and 'all true or all false' in msg
    # a fetch without a build
    assert lib.e3gnn_nlist_batch_fetch(None, None, None, None, None, None, None) == ERR_ARG
    assert 'not built' in lib.e3gnn_last_error().decode()


def test_energy_forces_batch_and_segment_sum_argument_rules():
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)

    def call(ctx=fake, n=5, E=0, B=2, atom_ptr=fake, energy=fake):
        rc = lib.e3gnn_energy_forces_batch(ctx, n, E, B, atom_ptr, fake, fake, fake, fake, energy,
                                           None, None, None, None, None)
        assert rc == ERR_ARG, rc
        return lib.e3gnn_last_error().decode()

    assert 'null context' in call(ctx=None)
    assert 'number of structures' in call(B=0)
    assert 'more structures than atoms' in call(B=6)
    assert 'null atom_ptr' in call(atom_ptr=None)
    assert 'energy output is required' in call(energy=None)

    def ssum(nseg=2, ptr=fake, rows=5, width=6, src=fake, out=fake):
        rc = lib.e3gnn_segment_sum(nseg, ptr, rows, width, src, out, None)
        assert rc == ERR_ARG, rc
        return lib.e3gnn_last_error().decode()

    assert 'number of segments' in ssum(nseg=0)
    assert 'width must be 1 or 6' in ssum(width=3)
    assert 'row count' in ssum(rows=-1)
    assert 'null array' in ssum(ptr=None)
    assert 'null array' in ssum(out=None)
    assert 'null array' in ssum(src=None)


def _structure_set():
    """small members of the GPU test's set: cubic Si, the 2-atom fcc primitive
    cell (heights < rc), a lone atom (no edges), unwrapped coordinates, an
    isolated cluster"""
    rng = np.random.default_rng(5)
    a = 5.43
    si, si_cell = si_diamond((2, 2, 1), sigma=0.05)
    prim = 0.5 * a * np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], dtype=np.float64)
    un, un_cell = si_diamond((2, 1, 1), sigma=0.05, seed=2)
    un = un + rng.integers(-2, 3, size=(len(un), 3)).astype(np.float64) @ un_cell
    T, F = (True,) * 3, (False,) * 3
    return [(si, si_cell, T),
            (np.array([[0, 0, 0], [0.25 * a] * 3], dtype=np.float64), prim, T),
            (np.zeros((1, 3)), np.eye(3) * 20.0, T),
            (un, un_cell, T),
            (rng.uniform(-3, 3, size=(11, 3)), None, F)]


def test_batch_neighbor_list_is_the_per_structure_list_with_offsets():
    S = _structure_set()
    rc = 5.0
    ei, sh, atom_ptr, edge_ptr = batch_neighbor_list(S, rc)
    assert atom_ptr.tolist() == np.concatenate([[0], np.cumsum([len(s[0]) for s in S])]).tolist()
    assert ei.dtype == np.int64 and atom_ptr.dtype == np.int64 and edge_ptr.dtype == np.int64
    assert edge_ptr[0] == 0 and edge_ptr[-1] == ei.shape[1] == len(sh)
    for k, (pos, cell, pbc) in enumerate(S):
        ej, sj = neighbor_list(pos, cell, rc, pbc)
        e0, e1 = edge_ptr[k], edge_ptr[k + 1]
        assert np.array_equal(ei[:, e0:e1], ej + atom_ptr[k])
        assert np.array_equal(sh[e0:e1], sj)
    assert edge_ptr[3] == edge_ptr[2]                # the lone atom has no edge
    assert np.all(np.diff(ei[0]) >= 0)               # CSR order through the whole batch
    # no edge joins two structures
    owner = np.repeat(np.arange(len(S)), np.diff(atom_ptr))
    assert np.array_equal(owner[ei[0]], owner[ei[1]])


def test_host_list_takes_unwrapped_coordinates_in_a_small_cell():
    """heights < 3 rc (the brute-force branch): atoms moved by whole cells keep
    their edges, the shifts absorb the offsets -- what the device list gives"""
    pos, cell = si_diamond((2, 2, 1), sigma=0.05)
    n_off = np.random.default_rng(7).integers(-3, 4, size=(len(pos), 3))
    moved = pos + n_off.astype(np.float64) @ cell
    ei, sh = neighbor_list(pos, cell, 5.0)
    ej, sj = neighbor_list(moved, cell, 5.0)
    assert ei.shape[1] == 32 * 28
    # (i, j, S) <-> (i, j, S + off[i] - off[j]); the order within (i, j) follows S
    key = lambda e, s: sorted(map(tuple, np.concatenate([e.T, s.astype(np.int64)], axis=1)))
    assert key(ej, sj) == key(ei, sh + n_off[ei[0]] - n_off[ei[1]])
    vb = (moved[ej[1]] + sj @ cell) - moved[ej[0]]
    assert np.linalg.norm(vb, axis=1).max() < 5.0


def test_errors_against_hand_computed_numbers():
    # structure 0: 2 atoms, with stress; structure 1: 1 atom, isolated (no stress)
    ref = [{'energy': -10.0, 'forces': np.zeros((2, 3)), 'stress': np.zeros(6)},
           {'energy': -4.0, 'forces': np.zeros((1, 3))}]
    pred = [{'energy': -9.8, 'forces': np.array([[0.3, 0.0, -0.4], [0.0, 0.0, 0.0]]),
             'stress': np.array([1e-3, -1e-3, 0.0, 0.0, 2e-3, 0.0])},
            {'energy': -4.3, 'forces': np.array([[0.0, 1.2, 0.0]])}]
    e = errors(pred, ref)
    # energy per atom: +0.1 and -0.3
    assert e['energy_rmse'] == pytest.approx(np.sqrt((0.01 + 0.09) / 2))
    assert e['energy_mae'] == pytest.approx(0.2)
    # forces: |dF|^2 per atom 0.25, 0, 1.44 -> sqrt(1.69 / 3); components: 1.9 / 9
    assert e['force_rmse'] == pytest.approx(np.sqrt(1.69 / 3))
    assert e['force_mae'] == pytest.approx(1.9 / 9)
    # stress: one structure, squares 1 + 1 + 4 (x 1e-6), components 4e-3 / 6, in kbar
    assert KBAR == 1602.1766208
    assert e['stress_rmse'] == pytest.approx(np.sqrt(6e-6) * 1602.1766208)
    assert e['stress_mae'] == pytest.approx(4e-3 / 6 * 1602.1766208)
    z = errors(pred, pred)
    assert all(v == 0.0 for v in z.values())
    assert np.isnan(errors(ref[1:], ref[1:])['stress_rmse'])
    with pytest.raises(ValueError):
        errors(pred, ref[:1])


def test_group_batches_keeps_order_and_budget():
    sizes = [30, 30, 30, 200, 10, 50, 50, 1]
    groups = group_batches(sizes, 100)
    assert [k for g in groups for k in g] == list(range(len(sizes)))     # order kept, none lost
    assert groups == [[0, 1, 2], [3], [4, 5], [6, 7]]
    for g in groups:
        assert sum(sizes[k] for k in g) <= 100 or len(g) == 1            # budget, or alone
    assert [3] in groups                                                 # larger than the budget
    assert group_batches([], 100) == []
    assert group_batches([100, 1], 100) == [[0], [1]]
    assert group_batches([5, 5], 1) == [[0], [1]]
    with pytest.raises(ValueError):
        group_batches([1], 0)
