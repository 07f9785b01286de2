"""Benchmark of the model options served by the fused kernels:
``use_bias_in_linear`` (e3nn Linear biases, added in the node-linear epilogues)
and ``readout_as_fcn`` (the FCN readout kernel, csrc/node.hip k_readout_fcn).

``python bench_options.py [--cells 23] [--steps 20] [--warmup 3]``: SevenNet-0's
architecture (its irreps, five blocks) with e3nn-initialised weights and random
biases, on the Si box of bench.py (23^3 cells = 97,336 atoms), one leg per
option set in one process:

    plain, plain again (the run-to-run noise floor), bias, fcn [30, 30], both

Each leg reports ``ms_per_step`` (host-timed, device-synchronised) and, from a
separate pass with the library's event timing on, the per-step time of every
kernel class (``node_linear``, ``readout``, the ``conv_*`` classes, ...).  The
FCN readout is compared with its bound: one read of x[L] and one write of
dE/dx[L] at the achievable HBM rate.  The bias + FCN deployment also runs on the
generic engine (``E3GNN_GENERIC=1``, a fresh child process, 11^3 cells =
10,648 atoms, 3 steps) beside the fused engine on the same box: the ratio is
what routing these options to the fused kernels gains.  Prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
HBM_TBS = 6.3   # achievable HBM3E rate of an MI355X (8 TB/s peak)
L = 5
LEGS = [('plain', {}), ('plain_again', {}),
        ('bias', {'use_bias_in_linear': True}),
        ('fcn', {'readout_as_fcn': True, 'readout_fcn_hidden_neurons': [30, 30],
                 'readout_fcn_activation': 'relu'}),
        ('bias_fcn', {'use_bias_in_linear': True, 'readout_as_fcn': True,
                      'readout_fcn_hidden_neurons': [30, 30], 'readout_fcn_activation': 'relu'})]


def log(msg):
    print(f'[bench_options] {msg}', file=sys.stderr, flush=True)


def deployment(opts, out_dir):
    """SevenNet-0's irreps with ``opts``: e3nn initialisation (seed 0), biases N(0, 0.5)."""
    from sevennet_finetuning_amd import model_build as mb
    cfg = mb.sevennet_shaped_config(128, L)
    cfg['irreps_manual'] = ['128x0e'] + ['128x0e+64x1e+32x2e'] * (L - 1) + ['128x0e']
    cfg.update(opts)
    mb.deploy_config(cfg, out_dir, seed=0)
    with open(os.path.join(out_dir, 'manifest.json')) as f:
        man = json.load(f)
    path = os.path.join(out_dir, 'weights.bin')
    flat = np.fromfile(path, dtype='<f4')
    g = np.random.default_rng(1)
    for t in man['tensors']:
        if t['name'].endswith('.bias'):
            flat[t['offset']:t['offset'] + t['numel']] = g.normal(0, 0.5, t['numel'])
    flat.tofile(path)
    return out_dir


def run_leg(model_dir, box, device, steps, warmup, stat_steps):
    from sevennet_finetuning_amd.model import E3GNNModel
    model = E3GNNModel(model_dir, device=device)

    def step():
        return model.energy_forces(box['types'], box['center'], box['nbr'], box['vec'])
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    res = {'family': model.family, 'ms_per_step': round(ms, 3), 'energy_eV': float(out['energy'])}
    if stat_steps:
        model.set_timing(True)
        model.reset_stats()
        for _ in range(stat_steps):
            step()
        torch.cuda.synchronize()
        stats = model.kernel_stats()
        model.set_timing(False)
        res['classes_ms'] = {k: round(v['ms'] / stat_steps, 4) for k, v in stats.items() if v['launches']}
    model.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=23)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--stat-steps', type=int, default=5)
    ap.add_argument('--generic-cells', type=int, default=11)
    ap.add_argument('--generic-steps', type=int, default=3)
    ap.add_argument('--no-generic', action='store_true')
    ap.add_argument('--child', default=None, metavar='DIR',
                    help='(internal) time the deployment DIR on --cells and print one JSON line')
    args = ap.parse_args()
    from bench import make_box
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    if args.child:
        with open(os.path.join(args.child, 'manifest.json')) as f:
            si = json.load(f)['chemical_symbols'].index('Si')
        box = make_box(args.cells, device, si)
        print(json.dumps(run_leg(args.child, box, device, args.steps, args.warmup, 0)), flush=True)
        return
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {}
        for name, opts in LEGS:
            key = json.dumps(opts, sort_keys=True)
            if key not in dirs:
                dirs[key] = deployment(opts, os.path.join(tmp, name))
        with open(os.path.join(dirs['{}'], 'manifest.json')) as f:
            si = json.load(f)['chemical_symbols'].index('Si')
        box = make_box(args.cells, device, si)
        n = box['n']
        log(f'box: {n} atoms, {box["E"]} edges')
        legs = {}
        for name, opts in LEGS:
            legs[name] = run_leg(dirs[json.dumps(opts, sort_keys=True)], box, device, args.steps,
                                 args.warmup, args.stat_steps)
            log(f'{name}: {legs[name]["ms_per_step"]} ms/step')
        a, b = legs['plain'], legs['plain_again']
        spread = {k: round(abs(a['classes_ms'][k] - b['classes_ms'].get(k, 0.0)), 4) for k in a['classes_ms']}
        D = 128
        bound_ms = 2.0 * n * D * 4 / (HBM_TBS * 1e12) * 1e3
        fcn_ms = legs['fcn']['classes_ms'].get('readout')
        result = {
            'metric': 'ms/step of SevenNet-0-shaped models with use_bias_in_linear / readout_as_fcn '
                      'on the fused kernels',
            'n_atoms': n, 'n_edges': box['E'], 'steps': args.steps, 'warmup': args.warmup,
            'stat_steps': args.stat_steps, 'legs': legs,
            'plain_spread': {'ms_per_step': round(abs(a['ms_per_step'] - b['ms_per_step']), 3),
                             'classes_ms': spread},
            'fcn_readout_bound': {'bytes': 2 * n * D * 4, 'hbm_tbs': HBM_TBS,
                                  'bound_ms': round(bound_ms, 4), 'readout_class_ms': fcn_ms,
                                  'note': 'the readout class also holds the energy sum and the '
                                          'atomic-energy copy',
                                  'ratio': round(fcn_ms / bound_ms, 2) if fcn_ms else None},
        }
        if not args.no_generic:
            small = make_box(args.generic_cells, device, si)
            dep = dirs[json.dumps(LEGS[-1][1], sort_keys=True)]
            fused = run_leg(dep, small, device, args.steps, args.warmup, 0)
            del small
            env = dict(os.environ, E3GNN_GENERIC='1')
            cmd = [sys.executable, os.path.abspath(__file__), '--child', dep, '--cells',
                   str(args.generic_cells), '--steps', str(args.generic_steps), '--warmup', '1']
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f'generic-engine child failed:\n{r.stdout}\n{r.stderr}')
            generic = json.loads(r.stdout.strip().splitlines()[-1])
            result['engines_bias_fcn'] = {
                'n_atoms': 8 * args.generic_cells ** 3, 'fused': fused, 'generic': generic,
                'generic_over_fused': round(generic['ms_per_step'] / fused['ms_per_step'], 2)}
        print(json.dumps(result), flush=True)


if __name__ == '__main__':
    main()
