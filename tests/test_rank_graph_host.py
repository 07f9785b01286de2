"""Device rank graph, the parts that need no GPU: the two C-ABI calls are
exported and refuse bad arguments before any device work, and
``DeviceRankGraph`` converts to and from the host ``RankGraph``."""
import ctypes

import numpy as np

from _systems import load_manifest_symbols, system
from sevennet_finetuning_amd import _lib
from sevennet_finetuning_amd.parallel import (DeviceRankGraph, RankGraph, build_rank_graph,
                                              local_handshake)

NEW = ('e3gnn_nlist_rank_build', 'e3gnn_nlist_rank_fetch')
FIELDS = ('owned', 'ghosts', 'types', 'center', 'nbr', 'recv_counts', 'recv_rows', 'req_ids')


def _graphs(name, grid):
    pos, cell, types = system(name, load_manifest_symbols())
    return [build_rank_graph(pos, cell, types, 5.0, grid, r) for r in range(int(np.prod(grid)))]


def _same(a, b):
    assert isinstance(a, RankGraph) and isinstance(b, RankGraph)
    assert (a.rank, a.world, tuple(a.grid)) == (b.rank, b.world, tuple(b.grid))
    assert (a.n_local, a.n_ghost, a.n_interior) == (b.n_local, b.n_ghost, b.n_interior)
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and np.array_equal(x, y), k
    assert a.vec.dtype == np.float32
    assert np.array_equal(a.vec, np.asarray(b.vec, dtype=np.float32))


def test_rank_graph_symbols_are_exported():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert lib.e3gnn_abi_version() == 1


def test_rank_build_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    cell = (ctypes.c_double * 9)(10, 0, 0, 0, 10, 0, 0, 0, 10)
    cnt = [ctypes.c_int64() for _ in range(4)]
    refs = [ctypes.byref(c) for c in cnt]
    # a null handle
    assert lib.e3gnn_nlist_rank_build(None, 0, None, cell, 5.0, None, 0, 2, *refs, None) == 1
    assert b'handle' in lib.e3gnn_last_error()
    # rank outside [0, world): the scalar arguments are checked first, so this
    # refusal is reachable without a device (and a handle) as well
    for rank, world in ((2, 2), (5, 2), (-1, 2), (0, 0)):
        assert lib.e3gnn_nlist_rank_build(None, 0, None, cell, 5.0, None, rank, world, *refs,
                                          None) == 1
        assert b'handle' not in lib.e3gnn_last_error()
    assert b'rank' in lib.e3gnn_last_error() or b'world' in lib.e3gnn_last_error()
    # a world beyond the supported bound is refused, not run
    assert lib.e3gnn_nlist_rank_build(None, 0, None, cell, 5.0, None, 0, 100000, *refs, None) == 1
    assert b'world' in lib.e3gnn_last_error()
    # a fetch before a build
    assert lib.e3gnn_nlist_rank_fetch(None, None, None, None, None, None, None, None, None) == 1


def test_device_rank_graph_round_trips_a_host_graph():
    for rg in _graphs('mixed_3x3x3', (2, 1, 1)) + _graphs('si_rng0_6x2x2', (2, 2, 1)):
        d = DeviceRankGraph.from_host(rg, 'cpu')
        assert (d.n_local, d.n_ghost, d.n_interior) == (rg.n_local, rg.n_ghost, rg.n_interior)
        assert np.array_equal(d.recv_counts_host, rg.recv_counts)
        assert d.vec.dtype.is_floating_point and d.vec.element_size() == 4
        _same(d.to_host(), rg)


def test_local_handshake_over_round_tripped_graphs():
    host = local_handshake(_graphs('mixed_3x3x3', (2, 1, 1)))
    back = local_handshake([DeviceRankGraph.from_host(rg, 'cpu').to_host()
                            for rg in _graphs('mixed_3x3x3', (2, 1, 1))])
    for a, b in zip(back, host):
        assert a.send_counts.sum() > 0
        assert np.array_equal(a.send_counts, b.send_counts)
        assert np.array_equal(a.send_rows, b.send_rows)
        # the send lists survive the device form too
        c = DeviceRankGraph.from_host(b, 'cpu').to_host()
        assert np.array_equal(c.send_counts, b.send_counts)
        assert np.array_equal(c.send_rows, b.send_rows)
