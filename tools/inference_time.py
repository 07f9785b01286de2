#!/usr/bin/env python
"""Dataset-inference throughput: structures per second over 512 structures of
the fine-tune benchmark's 54-atom mixed-species cell (the 3x3x3 primitive
diamond cell of ``bench_train.py``, one seed per structure), two ways:

  (a) a loop of ``SevenNetCalculator.calculate`` -- one device graph build and
      one evaluation per structure;
  (b) ``inference.predict_many`` at 64 structures per batch -- one build
      (``DeviceNeighborList.batch``) and one evaluation
      (``E3GNNModel.energy_forces_batch``) per batch.

One process; a warm-up pass of each, then three repetitions alternating (a) and
(b), each timed with the host clock between two device synchronisations; the
batched window sweeps the set ``--sweeps`` times so that it is not a few tens of
milliseconds long.  A last pass times the graph builds of (b) alone, for their
share of the batched call.  JSON lines go to ``--out`` (default
``profiles/inference_time.log``) and to stdout: one per timed pass, then a
summary.

    python tools/inference_time.py [--structures 512] [--per-batch 64] [--reps 3] [--sweeps 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--structures', type=int, default=512)
    ap.add_argument('--per-batch', type=int, default=64)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sweeps', type=int, default=8,
                    help='passes over the set inside one timed batched window')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'inference_time.log'))
    a = ap.parse_args()
    import torch
    from sevennet_finetuning_amd.inference import group_batches, predict_many
    from sevennet_finetuning_amd.sevennet_calculator import SevenNetCalculator
    from sevennet_finetuning_amd.structures import Atoms, diamond_primitive, mixed_symbols
    dev = torch.device('cuda', 0)
    calc = SevenNetCalculator('SevenNet-0', device=dev)
    atoms = []
    for k in range(a.structures):
        pos, cell = diamond_primitive((3, 3, 3), sigma=0.05, seed=k)
        atoms.append(Atoms(symbols=mixed_symbols(len(pos), seed=k + 1), positions=pos, cell=cell))
    n_atoms = len(atoms[0])
    budget = a.per_batch * n_atoms

    def loop():
        out = []
        for x in atoms:
            calc.calculate(x)
            out.append(dict(calc.results))
        return out

    def batched():
        return predict_many(calc, atoms, max_atoms_per_batch=budget)

    def batched_sweeps():   # a timed window of the loop's order of length
        for _ in range(a.sweeps):
            batched()

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    # warm-up of both (workspaces, code objects), and the two must agree
    ref = loop()[:a.per_batch]
    got = batched()[:a.per_batch]
    de = max(abs(p['energy'] - r['energy']) / abs(r['energy']) for p, r in zip(got, ref))
    df = max(float(np.abs(p['forces'] - r['forces']).max()) for p, r in zip(got, ref))
    rate = {'loop': [], 'batched': []}
    for rep in range(a.reps):
        for name, fn, count in (('loop', loop, a.structures),
                                ('batched', batched_sweeps, a.sweeps * a.structures)):
            dt, _ = timed(fn)
            rate[name].append(count / dt)
            emit({'pass': name, 'rep': rep, 'structures': count, 'seconds': round(dt, 4),
                  'structures_per_s': round(count / dt, 1)})
    # the graph builds of the batched call alone
    groups = group_batches([len(x) for x in atoms], budget)

    def builds():
        for g in groups:
            calc._nlist.batch([atoms[k].get_positions() for k in g],
                              [atoms[k].get_cell() for k in g], calc.cutoff)

    builds()
    t_build = min(timed(builds)[0] for _ in range(a.reps))
    t_batched = a.structures / max(rate['batched'])
    emit({'summary': 'inference_time', 'atoms_per_structure': n_atoms,
          'structures': a.structures, 'structures_per_batch': a.per_batch,
          'loop_structures_per_s': [round(r, 1) for r in rate['loop']],
          'batched_structures_per_s': [round(r, 1) for r in rate['batched']],
          'batched_beats_loop_in_every_pair': all(b > l for b, l in zip(rate['batched'],
                                                                        rate['loop'])),
          'speedup_min': round(min(b / l for b, l in zip(rate['batched'], rate['loop'])), 2),
          'batched_graph_build_share': round(t_build / t_batched, 3),
          'graph_build_ms_per_batch': round(1e3 * t_build / len(groups), 3),
          'max_energy_rel_diff': de, 'max_force_diff': df})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
