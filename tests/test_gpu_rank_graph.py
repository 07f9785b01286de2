"""Device rank graph (e3gnn_nlist_rank_*, csrc/neighbor.hip;
parallel.build_rank_graph_device) vs the host builder parallel.build_rank_graph:
identical rows, ghosts, edges and integer shifts (integer for integer), edge
vectors within f32 rounding, bitwise reproducible, and the decomposed
evaluation on device-built graphs.  Needs an MI355X: ``pytest -m gpu``."""
import ctypes
import functools
import socket

import numpy as np
import pytest
import torch

from _systems import load_manifest_symbols, system
from sevennet_finetuning_amd._lib import E3GNNError
from sevennet_finetuning_amd.neighbor import neighbor_list
from sevennet_finetuning_amd.parallel import (DeviceRankGraph, ParallelE3GNN, HipSegmentEngine,
                                              build_rank_graph, build_rank_graph_device, owners)
from sevennet_finetuning_amd.structures import si_diamond

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
RC = 5.0
SYMS = load_manifest_symbols()
INT_FIELDS = ('owned', 'ghosts', 'types', 'center', 'nbr', 'recv_counts', 'recv_rows', 'req_ids')
GRIDS = [(1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 1)]


@pytest.fixture(scope='module')
def dnl():
    from sevennet_finetuning_amd.neighbor import DeviceNeighborList
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return DeviceNeighborList(DEV)


@functools.lru_cache(maxsize=None)
def _system(name):
    return system(name, SYMS)


def host_graph(pos, cell, types, grid, rank, rc=RC):
    """The reference: the host graph and the host list's shifts by local row."""
    rg = build_rank_graph(pos, cell, types, rc, grid, rank)
    mine = np.nonzero(owners(pos, cell, grid) == rank)[0]
    ei, sh = neighbor_list(pos, cell, rc, centers=mine)
    lid = np.full(len(pos), -1, dtype=np.int64)
    lid[rg.owned] = np.arange(rg.n_local)
    order = np.argsort(lid[ei[0]], kind='stable')
    return rg, sh[order].astype(np.int32)


def compare(dnl, pos, cell, types, grid, rank, rc=RC):
    rg, sh = host_graph(pos, cell, types, grid, rank, rc)
    dev = build_rank_graph_device(pos, cell, types, rc, grid, rank, DEV, nlist=dnl)
    assert isinstance(dev, DeviceRankGraph)
    assert all(getattr(dev, k).device.type == 'cuda' for k in INT_FIELDS + ('vec', 'shift'))
    got = dev.to_host()
    for k in INT_FIELDS:
        assert np.array_equal(getattr(got, k), getattr(rg, k)), (k, grid, rank)
    assert got.n_interior == rg.n_interior == dev.n_interior
    assert (dev.n_local, dev.n_ghost) == (rg.n_local, rg.n_ghost)
    assert np.array_equal(dev.recv_counts_host, rg.recv_counts)
    assert dev.shift.dtype == torch.int32
    assert np.array_equal(dev.shift.cpu().numpy().reshape(-1, 3), sh.reshape(-1, 3))
    assert got.vec.dtype == np.float32 and got.vec.shape == (len(rg.center), 3)
    if len(rg.center):
        assert np.abs(got.vec - np.asarray(rg.vec, dtype=np.float32)).max() <= 1e-5
    return rg, dev


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: 'x'.join(map(str, g)))
@pytest.mark.parametrize('name', ['si_rng0_3x3x3', 'si_rng0_6x2x2', 'mixed_2x1x1', 'hfo2_resdat'])
def test_every_rank_equals_the_host_graph(dnl, name, grid):
    pos, cell, types = _system(name)
    world = int(np.prod(grid))
    n_local = 0
    for rank in range(world):
        rg, dev = compare(dnl, pos, cell, types, grid, rank)
        n_local += dev.n_local
        if world == 1:
            assert dev.n_interior == dev.n_local == len(pos) and dev.n_ghost == 0
            assert np.array_equal(dev.owned.cpu().numpy(), np.arange(len(pos)))
    assert n_local == len(pos)
    if name == 'si_rng0_6x2x2' and grid == (2, 1, 1):   # the interior-first order is exercised
        assert 0 < rg.n_interior < rg.n_local


def test_more_ghosts_than_one_sort_block(dnl):
    """1728 atoms on (2,2,2): every rank has several hundred ghosts from all
    seven peers, so the owner sort of the ghosts runs over more than one
    block of 256, and there are interior rows next to boundary rows."""
    pos, cell, types = _system('si_rng0_6x6x6')
    for rank in (0, 3, 7):
        rg, _ = compare(dnl, pos, cell, types, (2, 2, 2), rank)
        assert rg.n_ghost > 256 and np.count_nonzero(rg.recv_counts) == 7
        assert 0 < rg.n_interior < rg.n_local


def test_unwrapped_positions(dnl):
    """MD-style unwrapped coordinates: the shifts absorb the offsets, every
    integer list equals that of the wrapped system."""
    pos, cell, types = _system('si_rng0_3x3x3')
    rng = np.random.default_rng(7)
    off = rng.integers(-3, 4, size=(len(pos), 3)).astype(np.float64) @ cell
    for rank in range(4):
        _, a = compare(dnl, pos + off, cell, types, (2, 2, 1), rank)
        a = a.to_host()
        _, b = compare(dnl, pos, cell, types, (2, 2, 1), rank)
        b = b.to_host()
        for k in INT_FIELDS:
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert a.n_interior == b.n_interior


def test_empty_rank(dnl):
    """A rank that owns nothing: all counts 0, the fetch writes nothing."""
    pos, cell = si_diamond((4, 4, 4), sigma=0.05)
    frac = pos @ np.linalg.inv(cell)
    frac -= np.floor(frac)
    pos = pos[frac[:, 0] < 0.5]
    types = np.full(len(pos), SYMS.index('Si'), dtype=np.int64)
    compare(dnl, pos, cell, types, (2, 1, 1), 0)
    _, dev = compare(dnl, pos, cell, types, (2, 1, 1), 1)
    assert (dev.n_local, dev.n_interior, dev.n_ghost, dev.center.numel()) == (0, 0, 0, 0)
    assert dev.types.numel() == 0 and not dev.recv_counts_host.any()
    # the C ABI on the same case, outputs preset: nothing but recv_counts is written
    own = torch.as_tensor(owners(pos, cell, (2, 1, 1)).astype(np.int32), device=DEV)
    assert int((own == 1).sum()) == 0
    posd = torch.as_tensor(pos, device=DEV)
    cellh = (ctypes.c_double * 9)(*cell.reshape(-1).tolist())
    cnt = [ctypes.c_int64(-1) for _ in range(4)]
    assert dnl.lib.e3gnn_nlist_rank_build(dnl._h, len(pos), posd.data_ptr(), cellh, RC,
                                          own.data_ptr(), 1, 2, *[ctypes.byref(c) for c in cnt],
                                          None) == 0
    assert [c.value for c in cnt] == [0, 0, 0, 0]
    bufs = [torch.full((8,), -7, dtype=torch.int32, device=DEV) for _ in range(5)]
    vec = torch.full((8,), -7.0, dtype=torch.float32, device=DEV)
    recv = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    assert dnl.lib.e3gnn_nlist_rank_fetch(dnl._h, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                          recv.data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                          bufs[4].data_ptr(), vec.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert all(bool((b == -7).all()) for b in bufs) and bool((vec == -7.0).all())
    assert recv.tolist() == [0, 0]


def test_isolated_atom(dnl):
    """A rank whose only atom has no neighbour: one interior row, no edges."""
    pos = np.array([[1.0, 1.0, 1.0], [2.5, 1.0, 1.0], [30.0, 30.0, 30.0]])
    cell = np.eye(3) * 40.0
    types = np.full(3, SYMS.index('Si'), dtype=np.int64)
    rg0, _ = compare(dnl, pos, cell, types, (2, 1, 1), 0)
    assert rg0.n_local == 2 and len(rg0.center) == 2
    _, dev = compare(dnl, pos, cell, types, (2, 1, 1), 1)
    assert (dev.n_local, dev.n_interior, dev.n_ghost, dev.center.numel()) == (1, 1, 0, 0)
    assert dev.owned.tolist() == [2]


def _bytes(d):
    return [getattr(d, k).cpu().numpy().tobytes()
            for k in INT_FIELDS + ('shift', 'vec')] + [d.n_interior]


@pytest.mark.parametrize('name,grid,rank', [('hfo2_resdat', (2, 2, 2), 5),
                                            ('mixed_2x1x1', (2, 1, 1), 1)])
def test_bitwise_determinism(dnl, name, grid, rank):
    """Two builds on one handle and one on a fresh handle: identical bytes."""
    from sevennet_finetuning_amd.neighbor import DeviceNeighborList
    pos, cell, types = _system(name)
    a = _bytes(build_rank_graph_device(pos, cell, types, RC, grid, rank, DEV, nlist=dnl))
    b = _bytes(build_rank_graph_device(pos, cell, types, RC, grid, rank, DEV, nlist=dnl))
    c = _bytes(build_rank_graph_device(pos, cell, types, RC, grid, rank, DEV,
                                       nlist=DeviceNeighborList(DEV)))
    assert len(a[3]) > 0   # there are edges to compare
    assert a == b and a == c


def test_errors(dnl):
    pos, cell, types = _system('si_rng0_3x3x3')
    own = owners(pos, cell, (2, 1, 1)).astype(np.int32)
    # mixed periodicity
    with pytest.raises(E3GNNError):
        build_rank_graph_device(pos, cell, types, RC, (2, 1, 1), 0, DEV, nlist=dnl,
                                pbc=(True, True, False))
    with pytest.raises(E3GNNError):
        dnl.rank_graph(pos, cell, RC, own, 0, 2, pbc=(False, False, False))
    # rank >= world
    with pytest.raises(E3GNNError, match='e3gnn error 1'):
        dnl.rank_graph(pos, cell, RC, own, 2, 2)
    with pytest.raises(E3GNNError, match='e3gnn error 1'):
        build_rank_graph_device(pos, cell, types, RC, (2, 1, 1), 2, DEV, nlist=dnl)
    # an owner value equal to world: found on the device
    bad = own.copy()
    bad[17] = 2
    with pytest.raises(E3GNNError, match='e3gnn error 4.*owner'):
        dnl.rank_graph(pos, cell, RC, bad, 0, 2)
    # about 700 neighbours per centre at rc = 15: over NL_MAXD, reported ...
    with pytest.raises(E3GNNError, match='e3gnn error 4.*512'):
        build_rank_graph_device(pos, cell, types, 15.0, (2, 1, 1), 0, DEV, nlist=dnl)
    # ... a fetch without a finished build is refused, and the handle serves the next build
    assert dnl.lib.e3gnn_nlist_rank_fetch(dnl._h, None, None, None, None, None, None, None,
                                          None) == 1
    compare(dnl, pos, cell, types, (2, 1, 1), 0)
    compare(dnl, pos, cell, types, (2, 1, 1), 1)


def test_end_to_end_one_process(dnl):
    """set_graph(DeviceRankGraph) + evaluate at world 1 = the single-device
    evaluation on the device neighbour list of the same box; the engine takes
    the graph's tensors in place."""
    from sevennet_finetuning_amd.model import E3GNNModel
    model = E3GNNModel(device=DEV)
    pos, cell, types = _system('mixed_3x3x3')
    drg = build_rank_graph_device(pos, cell, types, model.cutoff, (1, 1, 1), 0, DEV, nlist=dnl)
    eng = HipSegmentEngine(model)
    drv = ParallelE3GNN(eng)
    drv.set_graph(drg)
    assert [t.data_ptr() for t in eng._in] == [drg.types.data_ptr(), drg.center.data_ptr(),
                                               drg.nbr.data_ptr(), drg.vec.data_ptr()]
    a = drv.evaluate()
    c, n, _, v = dnl(pos, cell, model.cutoff)
    b = model.energy_forces(torch.as_tensor(types, dtype=torch.int32, device=DEV), c, n, v)
    assert abs(float(a['energy']) - float(b['energy'])) <= 1e-6 * abs(float(b['energy']))
    assert (a['forces'] - b['forces']).abs().max().item() <= 1e-5
    assert b['forces'].abs().max().item() > 1e-2   # a real force field


def test_end_to_end_two_ranks(tmp_path):
    """Two gloo ranks on one GPU, mixed_3x3x3 on (2,1,1): device-built graphs
    give the gathered energy, forces and virial of host-built graphs bitwise
    (identical integer lists and f32 vectors are identical engine inputs).
    Were the builders' f32 vectors to differ in any element (the host forms
    S @ cell with a matrix product, the device term by term), the
    decomposed-vs-serial bounds of test_gpu_family.py apply instead."""
    import torch.multiprocessing as mp
    from _rank_graph_workers import worker
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    out = str(tmp_path / 'rg2.npz')
    mp.spawn(worker, args=(2, port, 'mixed_3x3x3', out), nprocs=2, join=True)
    got = np.load(out)
    assert got['n_ghost'][0] > 0 and got['in_place'][0]
    assert np.abs(got['host_forces']).max() > 1e-2
    if got['vec_same'][0]:
        assert float(got['dev_energy']) == float(got['host_energy'])
        assert np.array_equal(got['dev_forces'], got['host_forces'])
        assert np.array_equal(got['dev_virial'], got['host_virial'])
    else:
        e = float(got['host_energy'])
        assert abs(float(got['dev_energy']) - e) <= 2e-6 * abs(e)
        assert np.abs(got['dev_forces'] - got['host_forces']).max() <= 1e-4
