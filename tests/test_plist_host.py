"""The list filter (e3gnn_plist_*), the parts that need no GPU: the numpy
reference and the LAMMPS-like generator of tests/_plist_ref.py against the host
neighbour list, the argument rules of the C ABI before any device work, and the
validation of a list on the host."""
import ctypes

import numpy as np
import pytest

from _plist_ref import NEIGHMASK, RC, SPECIAL, SYSTEMS, case, filter_ref
from sevennet_finetuning_amd import _lib
from sevennet_finetuning_amd.neighbor import _rij, neighbor_list

ERR_ARG = 1
NEW = ('e3gnn_plist_create', 'e3gnn_plist_free', 'e3gnn_plist_check_list', 'e3gnn_plist_set',
       'e3gnn_plist_build', 'e3gnn_plist_fetch')
I32, I64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)


@pytest.mark.parametrize('name', SYSTEMS)
def test_reference_gives_the_host_neighbour_list(name):
    """filter_ref over lammps_like inputs = neighbor_list at the same cutoff, as
    a multiset of (centre tag, neighbour tag, f32 vec): pins the reference and
    the generator before the GPU tests lean on them."""
    pos, cell, L, (center, nbr, vec) = case(name)
    ei, sh = neighbor_list(pos, cell, RC)
    want_vec = _rij(pos[ei[1]], pos[ei[0]], sh, cell).astype(np.float32)
    tag = L['tag']

    def keys(ct, nt, v):
        rows = np.concatenate([ct[:, None].astype(np.int64), nt[:, None].astype(np.int64),
                               v.view(np.int32).astype(np.int64)], axis=1)
        return rows[np.lexsort(rows.T[::-1])]

    got = keys(center.astype(np.int64) + 1, nbr.astype(np.int64) + 1, vec)
    want = keys(tag[ei[0]], tag[ei[1]], want_vec)
    assert len(got) == ei.shape[1] > 0
    assert np.array_equal(got, want)
    # the generator really is LAMMPS-like: ghosts, special bits, rows by tag, a skin
    assert L['n_total'] > L['n'] and (L['cand'] & SPECIAL).any()
    assert not np.array_equal(L['row_atom'], np.arange(L['n']))
    assert L['cand_ptr'][-1] > len(center)
    assert np.all(np.diff(center) >= 0)


def test_plist_entries_are_exported_and_bound():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def _arrays(n=2, n_total=3):
    return dict(n=n, n_total=n_total, row_atom=np.array([1, 0], dtype=np.int32),
                cand_ptr=np.array([0, 2, 3], dtype=np.int64),
                cand=np.array([0, 2 | SPECIAL, 1], dtype=np.int32),
                atom_row=np.array([1, 0, 1], dtype=np.int32), neighmask=NEIGHMASK)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def test_plist_argument_rules():
    """Every rule returns E3GNN_ERR_ARG with its message, before any HIP call:
    this machine has no GPU, the handle of the set rules is a fake that is never
    dereferenced, and so is the device pointer of the build rules."""
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)

    def set_refused(h=fake, **change):
        a = {**_arrays(), **change}
        rc = lib.e3gnn_plist_set(h, a['n'], a['n_total'], _p(a['row_atom'], I32),
                                 _p(a['cand_ptr'], I64), _p(a['cand'], I32), a['neighmask'],
                                 _p(a['atom_row'], I32), None)
        assert rc == ERR_ARG, rc
        return lib.e3gnn_last_error().decode()

    assert 'null list-filter handle' in set_refused(h=None)
    assert 'n must be in' in set_refused(n=0)
    assert 'n must be in' in set_refused(n=-3)
    assert 'n_total must be in' in set_refused(n_total=1)
    assert 'null row_atom' in set_refused(row_atom=None)
    assert 'null cand_ptr' in set_refused(cand_ptr=None)
    assert 'null atom_row' in set_refused(atom_row=None)
    assert 'null cand' in set_refused(cand=None)

    h = lib.e3gnn_plist_create(0)          # no HIP call: works without a device
    assert h
    try:
        ne = ctypes.c_int64(-1)

        def build_refused(handle=h, x=fake, cutoff=5.0):
            rc = lib.e3gnn_plist_build(handle, x, cutoff, ctypes.byref(ne), None)
            assert rc == ERR_ARG, rc
            return lib.e3gnn_last_error().decode()

        assert 'null list-filter handle' in build_refused(handle=None)
        assert 'null positions' in build_refused(x=None)
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            assert 'cutoff must be positive and finite' in build_refused(cutoff=bad)
        assert 'build before set' in build_refused()
        assert lib.e3gnn_plist_fetch(None, fake, fake, fake, None) == ERR_ARG
        assert 'null list-filter handle' in lib.e3gnn_last_error().decode()
        assert lib.e3gnn_plist_fetch(h, fake, fake, fake, None) == ERR_ARG
        assert 'fetch before build' in lib.e3gnn_last_error().decode()
        assert ne.value == -1
    finally:
        lib.e3gnn_plist_free(h)
    assert not lib.e3gnn_plist_create(-1)
    assert 'negative device' in lib.e3gnn_last_error().decode()


def _check(lib, **change):
    a = {**_arrays(), **change}
    rc = lib.e3gnn_plist_check_list(a['n'], a['n_total'], _p(a['row_atom'], I32),
                                    _p(a['cand_ptr'], I64), _p(a['cand'], I32), a['neighmask'],
                                    _p(a['atom_row'], I32))
    return rc, lib.e3gnn_last_error().decode()


def test_list_validation_names_the_row():
    """e3gnn_plist_set validates through the function e3gnn_plist_check_list
    exports (the handle's set needs the device for its pinned buffer)."""
    lib = _lib.load()
    assert _check(lib)[0] == 0

    def refused(**change):
        rc, msg = _check(lib, **change)
        assert rc == ERR_ARG, (rc, msg)
        return msg

    def cand(k, v):
        c = _arrays()['cand'].copy()
        c[k] = v
        return c

    msg = refused(cand=cand(2, 3))                       # == n_total, in row 1
    assert 'row 1' in msg and 'candidate 3 outside' in msg
    msg = refused(cand=cand(1, 3 | SPECIAL))             # the same behind a special bit, row 0
    assert 'row 0' in msg and 'candidate 3 outside' in msg
    msg = refused(cand=cand(0, -1))                      # negative: masks to 2^29 - 1
    assert 'row 0' in msg and f'candidate {NEIGHMASK} outside' in msg
    assert 'row 0' in refused(cand=cand(0, -1), neighmask=-1)        # ... and stays negative
    msg = refused(cand_ptr=np.array([0, 3, 2], dtype=np.int64))
    assert 'row 1' in msg and 'cand_ptr decreases' in msg
    assert 'cand_ptr[0] must be 0' in refused(cand_ptr=np.array([1, 2, 3], dtype=np.int64))
    msg = refused(atom_row=np.array([1, 0, -1], dtype=np.int32))
    assert 'atom 2' in msg and 'atom_row -1 outside' in msg
    assert 'atom 2' in refused(atom_row=np.array([1, 0, 2], dtype=np.int32))     # == n
    msg = refused(row_atom=np.array([1, 3], dtype=np.int32))
    assert 'row 1' in msg and 'row_atom 3 outside' in msg
    assert 'row 0' in refused(row_atom=np.array([-1, 0], dtype=np.int32))
    msg = refused(row_atom=np.array([0, 1], dtype=np.int32))         # the maps disagree
    assert 'row 0' in msg and 'must agree' in msg


def test_reference_is_order_preserving_and_strict():
    """The reference itself on a hand-made row: list order kept, d^2 = rc^2 out."""
    x = np.array([[0, 0, 0], [5, 0, 0], [3, 4, 0], [1, 0, 0], [0, 2, 0]], dtype=np.float64)
    c, nb, v = filter_ref(x, [0], [0, 4], np.array([4, 1, 2 | SPECIAL, 3], dtype=np.int32),
                          NEIGHMASK, np.arange(5), 5.0)
    assert c.tolist() == [0, 0] and nb.tolist() == [4, 3]
    assert v.tolist() == [[0, 2, 0], [1, 0, 0]]
