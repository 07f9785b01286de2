"""Spawn target of the device rank-graph decomposition test (gloo, two ranks
sharing one GPU): one evaluation with host-built and one with device-built
rank graphs in the same processes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def worker(rank, world, port, name, out):
    """Evaluate system `name` over `world` ranks twice, with the graphs of
    ``build_rank_graph`` and of ``build_rank_graph_device``; rank 0 saves the
    gathered energy / virial / forces of both and whether the builders' f32
    edge vectors agree in every element on every rank."""
    import torch
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from _systems import load_manifest_symbols, system
    from sevennet_finetuning_amd.model import E3GNNModel
    from sevennet_finetuning_amd.parallel import (DeviceRankGraph, HipSegmentEngine,
                                                  ParallelE3GNN, brick_grid, build_rank_graph,
                                                  build_rank_graph_device, gather_all)
    pos, cell, types = system(name, load_manifest_symbols())
    grid = brick_grid(world)
    torch.cuda.set_device(0)
    eng = HipSegmentEngine(E3GNNModel(device='cuda:0'))
    host = build_rank_graph(pos, cell, types, 5.0, grid, rank)
    dev = build_rank_graph_device(pos, cell, types, 5.0, grid, rank, 'cuda:0')
    assert isinstance(dev, DeviceRankGraph)
    vec_same = torch.tensor([int(np.array_equal(np.asarray(host.vec, dtype=np.float32),
                                                dev.vec.cpu().numpy()))])
    dist.all_reduce(vec_same, op=dist.ReduceOp.MIN)
    res = {}
    for key, rg in (('host', host), ('dev', dev)):
        drv = ParallelE3GNN(eng)
        drv.set_graph(rg)
        r = drv.evaluate()
        f, _ = gather_all(r, len(pos))
        res[key] = (float(r['energy']), r['virial'].cpu().numpy(), f.numpy())
    in_place = eng._in[1].data_ptr() == dev.center.data_ptr() and \
        eng._in[3].data_ptr() == dev.vec.data_ptr()
    if rank == 0:
        np.savez(out, vec_same=np.array([int(vec_same)]), in_place=np.array([in_place]),
                 n_ghost=np.array([dev.n_ghost]),
                 **{f'{k}_{q}': v[i] for k, v in res.items()
                    for i, q in enumerate(('energy', 'virial', 'forces'))})
    dist.barrier()
    dist.destroy_process_group()
