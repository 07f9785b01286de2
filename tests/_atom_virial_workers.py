"""Spawn target of the decomposed per-atom virial tests (gloo, world_size > 1)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def worker(rank, world, port, name, engine, out):
    """System `name` over `world` ranks, evaluated without and with
    ``atom_virial``; rank 0 saves the per-atom virial gathered by owner, the
    exchange counts of both calls and whether energy and forces kept their bits."""
    import torch
    import torch.distributed as dist
    if engine == 'cpu':
        torch.set_num_threads(1)   # bitwise comparison below (see _parallel_workers.py)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from _systems import load_manifest_symbols, system
    from sevennet_finetuning_amd.parallel import ParallelE3GNN, brick_grid, build_rank_graph
    pos, cell, types = system(name, load_manifest_symbols())
    rg = build_rank_graph(pos, cell, types, 5.0, brick_grid(world), rank)
    if engine == 'cpu':
        from _segment_cpu_virial import make_engine
        eng = make_engine(rg)
    else:
        from sevennet_finetuning_amd.model import E3GNNModel
        from sevennet_finetuning_amd.parallel import HipSegmentEngine
        torch.cuda.set_device(0)
        eng = HipSegmentEngine(E3GNNModel(device='cuda:0'))
    drv = ParallelE3GNN(eng)
    drv.set_graph(rg)
    t0, t1 = {}, {}
    plain = drv.evaluate(timing=t0)
    e0, f0 = float(plain['energy']), plain['forces'].detach().cpu().clone()
    res = drv.evaluate(timing=t1, atom_virial=True)
    same = e0 == float(res['energy']) and torch.equal(f0, res['forces'].detach().cpu())
    res = drv.evaluate(atom_virial=True)   # the overlapped (untimed) exchanges
    same = same and e0 == float(res['energy']) and torch.equal(f0, res['forces'].detach().cpu())
    w = torch.zeros(len(pos), 6, dtype=torch.float64)
    w[torch.as_tensor(rg.owned, dtype=torch.int64)] = res['atomic_virial'].detach().cpu().to(torch.float64)
    dist.all_reduce(w)
    if rank == 0:
        np.savez(out, atomic_virial=w.numpy(), virial=res['virial'].cpu().numpy(),
                 exchanges=np.array([t0['exchanges'], t1['exchanges']]), same=np.array([same]),
                 default_has_key=np.array(['atomic_virial' in plain]),
                 rows=np.array([res['atomic_virial'].shape[0], rg.n_local, rg.n_ghost]))
    dist.barrier()
    dist.destroy_process_group()
