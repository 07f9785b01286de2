#!/usr/bin/env python
"""Time the device rank-graph build against the host builder on the
778,688-atom Si box (46^3 cells) split 2x2x2, ranks 0 and 7 by default.

For each rank: parallel.build_rank_graph on the host (one run, wall time),
then e3gnn_nlist_rank_build + e3gnn_nlist_rank_fetch with the positions and
the owner array resident on the device (torch.cuda.synchronize around each,
median of 5 runs after 1 warm-up), the integer lists asserted equal, and one
JSON line.  ``wrapper_ms`` is parallel.build_rank_graph_device as a whole:
the host ``owners`` pass (``owners_ms``), the uploads and the type gather on
top of the device build.

    python tools/rank_graph_time.py [--cells 46] [--grid 2,2,2] [--ranks 0,7]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=46)
    ap.add_argument('--grid', default='2,2,2')
    ap.add_argument('--ranks', default='0,7')
    ap.add_argument('--cutoff', type=float, default=5.0)
    ap.add_argument('--runs', type=int, default=5)
    a = ap.parse_args()
    import torch
    from sevennet_finetuning_amd.neighbor import DeviceNeighborList
    from sevennet_finetuning_amd.parallel import (build_rank_graph, build_rank_graph_device,
                                                  owners)
    from sevennet_finetuning_amd.structures import si_diamond
    dev = 'cuda:0'
    grid = tuple(int(x) for x in a.grid.split(','))
    world = int(np.prod(grid))
    pos, cell = si_diamond((a.cells,) * 3, sigma=0.05)
    types = np.zeros(len(pos), dtype=np.int64)
    nl = DeviceNeighborList(dev)
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    t0 = time.perf_counter()
    own_h = owners(pos, cell, grid).astype(np.int32)
    owners_ms = 1e3 * (time.perf_counter() - t0)
    posd = torch.as_tensor(pos, device=dev)
    own = torch.as_tensor(own_h, device=dev)
    cellh = (ctypes.c_double * 9)(*cell.reshape(-1).tolist())
    for rank in (int(r) for r in a.ranks.split(',')):
        t0 = time.perf_counter()
        rg = build_rank_graph(pos, cell, types, a.cutoff, grid, rank)
        host_s = time.perf_counter() - t0
        tb, tf, tw = [], [], []
        for it in range(a.runs + 1):
            cnt = [ctypes.c_int64() for _ in range(4)]
            s = torch.cuda.current_stream(dev).cuda_stream
            sync()
            t0 = time.perf_counter()
            rc = nl.lib.e3gnn_nlist_rank_build(nl._h, len(pos), posd.data_ptr(), cellh, a.cutoff,
                                               own.data_ptr(), rank, world,
                                               *[ctypes.byref(c) for c in cnt], s)
            sync()
            t1 = time.perf_counter()
            assert rc == 0, nl.lib.e3gnn_last_error()
            n_local, _, n_ghost, E = (c.value for c in cnt)
            i32 = lambda *sh: torch.empty(*sh, dtype=torch.int32, device=dev)  # noqa: E731
            o = [i32(n_local), i32(n_ghost), torch.empty(world, dtype=torch.int64, device=dev),
                 i32(E), i32(E), i32(E, 3), torch.empty(E, 3, dtype=torch.float32, device=dev)]
            sync()
            t2 = time.perf_counter()
            rc = nl.lib.e3gnn_nlist_rank_fetch(nl._h, *[t.data_ptr() for t in o], s)
            sync()
            t3 = time.perf_counter()
            assert rc == 0, nl.lib.e3gnn_last_error()
            if it:   # the first run is the warm-up (workspaces grow)
                tb.append(1e3 * (t1 - t0))
                tf.append(1e3 * (t3 - t2))
        for it in range(a.runs + 1):
            sync()
            t0 = time.perf_counter()
            drg = build_rank_graph_device(pos, cell, types, a.cutoff, grid, rank, dev, nlist=nl)
            sync()
            if it:
                tw.append(1e3 * (time.perf_counter() - t0))
        got = drg.to_host()
        for k in ('owned', 'ghosts', 'types', 'center', 'nbr', 'recv_counts', 'recv_rows',
                  'req_ids'):
            assert np.array_equal(getattr(got, k), getattr(rg, k)), k
        assert got.n_interior == rg.n_interior
        build_ms, fetch_ms = statistics.median(tb), statistics.median(tf)
        print(json.dumps({
            'atoms': len(pos), 'grid': list(grid), 'rank': rank, 'host_s': round(host_s, 3),
            'device_ms': round(build_ms + fetch_ms, 3), 'build_ms': round(build_ms, 3),
            'fetch_ms': round(fetch_ms, 3), 'wrapper_ms': round(statistics.median(tw), 3),
            'owners_ms': round(owners_ms, 3), 'n_local': rg.n_local,
            'n_interior': rg.n_interior, 'n_ghost': rg.n_ghost, 'n_edges': int(len(rg.center)),
            'lists_equal': True}), flush=True)


if __name__ == '__main__':
    main()
