"""The rank-graph filter (e3gnn_plist_set_rank / _rank_build / _rank_fetch), the
parts that need no GPU: the numpy reference and the brick-like generator of
tests/_plist_rank_ref.py, the validation of a rank list on the host
(e3gnn_plist_check_rank_list) and the argument and ordering rules of the C ABI
before any device work."""
import ctypes

import numpy as np
import pytest

from _plist_rank_ref import NEIGHMASK, RC, SPECIAL, SYSTEMS, rank_case, rank_ref, vacuity
from sevennet_finetuning_amd import _lib

ERR_ARG = 1
NEW = ('e3gnn_plist_check_rank_list', 'e3gnn_plist_set_rank', 'e3gnn_plist_rank_build',
       'e3gnn_plist_rank_fetch')
I32, I64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)


def test_rank_entries_are_exported_and_bound():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _check(lib, a):
    rc = lib.e3gnn_plist_check_rank_list(a['n'], a['n_total'], _p(a['row_atom'], I32),
                                         _p(a['cand_ptr'], I64), _p(a['cand'], I32),
                                         a.get('neighmask', NEIGHMASK), _p(a['atom_class'], I32),
                                         a['n_class'])
    return rc, lib.e3gnn_last_error().decode()


def test_reference_on_a_hand_made_list():
    """Two owned rows, five ghosts: tag classes 2 (atoms 3 and 5: two images of
    one atom), 3 (atom 4) and 4 (atom 6, out of reach); atom 2 is a self-image
    of row 0.  Row 0 meets class 3 then class 2, row 1 meets class 2 through
    its other image."""
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 4, 0], [0, 0, 3], [2, 0, 0], [1, 0, 3], [9, 9, 9]],
                 dtype=np.float64)
    row_atom = np.array([1, 0], dtype=np.int32)            # row 0 is atom 1
    atom_class = np.array([1, 0, 0, 2, 3, 2, 4], dtype=np.int32)
    cand_ptr = np.array([0, 5, 8], dtype=np.int64)
    cand = np.array([6, 4 | SPECIAL, 3, 2, 0, 5, 1 | SPECIAL, 6], dtype=np.int32)
    r = rank_ref(x, row_atom, cand_ptr, cand, NEIGHMASK, atom_class, 5.0)
    assert r['center'].tolist() == [0, 0, 0, 0, 1, 1]
    assert r['nbr'].tolist() == [2, 3, 0, 1, 3, 0]
    assert r['ghost_atom'].tolist() == [4, 3] and r['n_ghost'] == 2
    assert r['vec'][0].tolist() == [1.0, 0.0, 0.0]
    lib = _lib.load()
    assert _check(lib, dict(n=2, n_total=7, row_atom=row_atom, cand_ptr=cand_ptr, cand=cand,
                            atom_class=atom_class, n_class=3))[0] == 0


@pytest.mark.parametrize('name', SYSTEMS)
def test_generated_lists_pass_and_are_not_vacuous(name):
    """e3gnn_plist_check_rank_list accepts what brick_like makes, and the input
    holds what the GPU tests need it to hold (asserted there again, next to the
    comparison).  Three of the four conditions hold on every system.  The
    fourth, a class without an edge, holds on none: in all three cells (10.9,
    10.1 and 10.9 A along the first lattice vector) every atom outside the half box has an
    image within 5 A of an owned atom, so every ghost tag gets a row; the
    synthetic lists of tests/test_gpu_plist_rank.py cover it."""
    L, ref = rank_case(name)
    lib = _lib.load()
    rc, msg = _check(lib, L)
    assert rc == 0, msg
    assert vacuity(L, ref) == dict(shared_row=True, self_image=True, edgeless=False,
                                   rows_apart=True)
    assert 0 < L['n'] < L['n_total'] and len(ref['center']) > 0
    assert not np.array_equal(L['row_atom'], np.arange(L['n']))
    assert (L['cand'] & SPECIAL).any() and L['cand_ptr'][-1] > len(ref['center'])


def test_rank_list_validation_names_the_culprit():
    L, _ = rank_case('si_rng0_2x2x1')
    lib = _lib.load()
    n, nc = L['n'], L['n_class']

    def refused(**change):
        rc, msg = _check(lib, {**L, **change})
        assert rc == ERR_ARG, (rc, msg)
        return msg

    def cls(a, v):
        c = L['atom_class'].copy()
        c[a] = v
        return c

    ghost = int(np.flatnonzero(L['atom_class'] >= n)[0])
    # a class out of range, at either end
    msg = refused(atom_class=cls(ghost, n + nc))
    assert f'atom {ghost}:' in msg and f'atom_class {n + nc} outside' in msg
    msg = refused(atom_class=cls(ghost, -1))
    assert f'atom {ghost}:' in msg and 'atom_class -1 outside' in msg
    # the two maps disagree on a node
    t = 3
    msg = refused(atom_class=cls(int(L['row_atom'][t]), (t + 1) % n))
    assert f'row {t}:' in msg and 'must agree' in msg
    # a class no atom names: every atom of the last class renamed to the first
    last = L['atom_class'] == n + nc - 1
    assert last.any() and nc >= 2
    c = L['atom_class'].copy()
    c[last] = n
    msg = refused(atom_class=c)
    assert f'class {n + nc - 1}' in msg and 'named by no atom' in msg
    # ... and one class too many declared
    msg = refused(n_class=nc + 1)
    assert f'class {n + nc}' in msg and 'named by no atom' in msg
    # the list rules of e3gnn_plist_set
    c = L['cand'].copy()
    c[L['cand_ptr'][2]] = L['n_total'] | SPECIAL
    msg = refused(cand=c)
    assert 'row 2:' in msg and f"candidate {L['n_total']} outside" in msg
    p = L['cand_ptr'].copy()
    p[5] = p[4] - 1
    msg = refused(cand_ptr=p)
    assert 'row 4' in msg and 'cand_ptr decreases' in msg
    p = L['cand_ptr'].copy()
    p[0] = 1
    assert 'cand_ptr[0] must be 0' in refused(cand_ptr=p)
    r = L['row_atom'].copy()
    r[1] = L['n_total']
    msg = refused(row_atom=r)
    assert 'row 1:' in msg and f"row_atom {L['n_total']} outside" in msg
    # the sizes
    assert 'n_class must be in' in refused(n_class=-1)
    assert 'n_class must be in' in refused(n_class=L['n_total'] - n + 1)
    assert 'null atom_class' in refused(atom_class=None)
    assert 'n must be in' in refused(n=0)


def test_rank_argument_and_ordering_rules():
    """Every rule returns E3GNN_ERR_ARG with its message before any HIP call:
    this machine has no GPU, and the fake pointers are never dereferenced."""
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)
    L, _ = rank_case('si_rng0_2x2x1')

    def set_refused(h=fake, **change):
        a = {**L, **change}
        rc = lib.e3gnn_plist_set_rank(h, a['n'], a['n_total'], _p(a['row_atom'], I32),
                                      _p(a['cand_ptr'], I64), _p(a['cand'], I32), NEIGHMASK,
                                      _p(a['atom_class'], I32), a['n_class'], None)
        assert rc == ERR_ARG, rc
        return lib.e3gnn_last_error().decode()

    assert 'null list-filter handle' in set_refused(h=None)
    assert 'n must be in' in set_refused(n=-3)
    assert 'n_total must be in' in set_refused(n_total=L['n'] - 1)
    assert 'null row_atom' in set_refused(row_atom=None)
    assert 'null cand_ptr' in set_refused(cand_ptr=None)
    assert 'null atom_class' in set_refused(atom_class=None)
    assert 'null cand' in set_refused(cand=None)
    assert 'n_class must be in' in set_refused(n_class=-1)

    h = lib.e3gnn_plist_create(0)          # no HIP call: works without a device
    assert h
    try:
        ne, ng = ctypes.c_int64(-1), ctypes.c_int64(-1)

        def build_refused(handle=h, x=fake, cutoff=5.0):
            rc = lib.e3gnn_plist_rank_build(handle, x, cutoff, ctypes.byref(ne), ctypes.byref(ng), None)
            assert rc == ERR_ARG, rc
            return lib.e3gnn_last_error().decode()

        assert 'null list-filter handle' in build_refused(handle=None)
        assert 'null positions' in build_refused(x=None)
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            assert 'cutoff must be positive and finite' in build_refused(cutoff=bad)
        assert 'rank_build before set_rank' in build_refused()
        assert lib.e3gnn_plist_rank_fetch(None, fake, fake, fake, fake, None) == ERR_ARG
        assert 'null list-filter handle' in lib.e3gnn_last_error().decode()
        assert lib.e3gnn_plist_rank_fetch(h, fake, fake, fake, fake, None) == ERR_ARG
        assert 'rank_fetch before rank_build' in lib.e3gnn_last_error().decode()
        # the plain entry points keep their answers on the same handle
        assert lib.e3gnn_plist_build(h, fake, 5.0, ctypes.byref(ne), None) == ERR_ARG
        assert 'build before set' in lib.e3gnn_last_error().decode()
        assert lib.e3gnn_plist_fetch(h, fake, fake, fake, None) == ERR_ARG
        assert 'fetch before build' in lib.e3gnn_last_error().decode()
        assert ne.value == -1 and ng.value == -1
    finally:
        lib.e3gnn_plist_free(h)
