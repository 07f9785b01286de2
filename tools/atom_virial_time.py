#!/usr/bin/env python
"""Time the per-atom virial launch (k_atom_virial, e3gnn_atom_virial) beside
the force scatter (k_atom_force) on the 97,336-atom Si box (23^3 cells).

Both launches walk the same two index lists (the centre CSR and the
transposed CSR); the virial one also reads the edge vectors and writes six
values a row instead of three, about twice the bytes.  The times are the
library's own event brackets (e3gnn_set_timing / e3gnn_kernel_stats), taken in
one run: ``--warmup`` evaluations, then ``--steps`` timed ones, each
``energy_forces(..., want_atom_virial=True)``.  One JSON line.

    python tools/atom_virial_time.py [--cells 23] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=23)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    import torch
    from sevennet_finetuning_amd.model import E3GNNModel
    from sevennet_finetuning_amd.neighbor import DeviceNeighborList
    from sevennet_finetuning_amd.structures import si_diamond
    dev = 'cuda:0'
    pos, cell = si_diamond((a.cells,) * 3, sigma=0.05)
    model = E3GNNModel(device=dev)
    center, nbr, _, vec = DeviceNeighborList(dev)(pos, cell, model.cutoff)
    types = torch.full((len(pos),), model.chemical_symbols.index('Si'), dtype=torch.int32, device=dev)
    for _ in range(a.warmup):
        out = model.energy_forces(types, center, nbr, vec, want_atom_virial=True)
    torch.cuda.synchronize(dev)
    model.set_timing(True)
    model.reset_stats()
    for _ in range(a.steps):
        out = model.energy_forces(types, center, nbr, vec, want_atom_virial=True)
    torch.cuda.synchronize(dev)
    st = model.kernel_stats()
    model.set_timing(False)
    per = lambda k: st[k]['ms'] / max(st[k]['launches'], 1)  # noqa: E731
    w = out['atomic_virial'].double().sum(0).cpu().numpy()
    v = out['virial'].double().cpu().numpy()
    step_ms = sum(c['ms'] for c in st.values()) / a.steps
    print(json.dumps({
        'atoms': len(pos), 'edges': int(center.numel()), 'steps': a.steps,
        'atom_virial_ms': round(per('atom_virial'), 4), 'atom_force_ms': round(per('atom_force'), 4),
        'ratio': round(per('atom_virial') / per('atom_force'), 3),
        'atom_virial_launches': st['atom_virial']['launches'],
        'atom_virial_GBps': round(st['atom_virial']['bytes'] / st['atom_virial']['ms'] / 1e6, 1),
        'kernel_ms_per_step': round(step_ms, 3),
        'sum_minus_virial_max': float(np.abs(w - v).max()), 'virial_max': float(np.abs(v).max())}),
        flush=True)


if __name__ == '__main__':
    main()
