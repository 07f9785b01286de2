"""Benchmark of the fine-tune step for the model options the explicit step
covers: ``use_bias_in_linear`` and ``readout_as_fcn`` (train_explicit.py;
csrc/fcn_train.hip and the column-sum kernel of csrc/train_ops.hip).

``python bench_train_options.py [--steps 20] [--warmup 5] [--leg NAME] [--grad explicit|autograd]``:
SevenNet-0's architecture (its irreps, five blocks) with e3nn-initialised
weights and random biases (bench_options.py's deployments), the rehearsal step
of bench_train.py (2 x 8 54-atom structures, Huber + EWC, Adam, HIP graph), one
leg per option set

    plain, bias, fcn [30, 30] silu, bias + fcn

each with the hand-scheduled derivatives (``explicit_grad`` True) and with the
autograd double backward (False) -- the path these option models took before
the explicit step covered them.  Prints one JSON line per leg with ms per step
and structures/s; ``--leg`` / ``--grad`` run one of them (a profiler's kernel
trace of one leg: tools/train_census.py).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
FCN = {'readout_as_fcn': True, 'readout_fcn_hidden_neurons': [30, 30], 'readout_fcn_activation': 'silu'}
LEGS = [('plain', {}), ('bias', {'use_bias_in_linear': True}), ('fcn', FCN),
        ('bias_fcn', dict({'use_bias_in_linear': True}, **FCN))]


def log(msg):
    print(f'[bench_train_options] {msg}', file=sys.stderr, flush=True)


def run_leg(model_dir, device, explicit, steps, warmup, batch=8):
    """bench_train.step_bench's timed rehearsal step on the deployment model_dir"""
    from bench_train import make_batches
    from sevennet_finetuning_amd import train
    from sevennet_finetuning_amd.nn import SevenNetTrainable
    model = SevenNetTrainable(model_dir, device=device)
    fisher = {n: torch.full_like(p, 1e-3) for n, p in model.named_parameters()}
    opt = {n: p.detach().clone() for n, p in model.named_parameters()}
    cfg = {'loss': 'huber', 'loss_param': {'delta': 0.01}, 'force_loss_weight': 1.0,
           'stress_loss_weight': 0.01, 'is_train_stress': True, 'optimizer': 'adam',
           'optim_param': {'lr': 1e-5}, 'scheduler': 'exponentiallr',
           'scheduler_param': {'gamma': 0.99}, 'is_ddp': False, 'device': device,
           'hip_graph': True, 'explicit_grad': explicit,
           'continue': {'fisher_information': fisher, 'opt_params': opt, 'ewc_lambda': 1e5}}
    tr = train.Trainer(model, cfg)
    if explicit and tr.explicit is None:
        raise RuntimeError('the explicit step does not cover this model')
    n_b = 4
    batches = [train.collate(b, device=device, dtype=torch.float32)
               for b in make_batches(0, 2 * n_b, batch, model.chemical_symbols)]
    model.train(True)

    def step(i):
        return tr.rehearsal_step(batches[(2 * i) % (2 * n_b)], batches[(2 * i + 1) % (2 * n_b)])
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        loss, mloss = step(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {'ms_per_step': round(dt / steps * 1e3, 3), 'structures_per_s': round(2 * batch * steps / dt, 2),
            'explicit_grad': tr.explicit is not None, 'hip_graph': bool(tr.hip_graph),
            'loss': float(loss), 'mem_loss': float(mloss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--leg', default=None, choices=[n for n, _ in LEGS])
    ap.add_argument('--grad', default=None, choices=['explicit', 'autograd'])
    args = ap.parse_args()
    from bench_options import deployment
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    with tempfile.TemporaryDirectory() as tmp:
        for name, opts in LEGS:
            if args.leg not in (None, name):
                continue
            d = deployment(opts, os.path.join(tmp, name))
            for grad in ('explicit', 'autograd'):
                if args.grad not in (None, grad):
                    continue
                r = run_leg(d, device, grad == 'explicit', args.steps, args.warmup)
                log(f'{name} / {grad}: {r["ms_per_step"]} ms per step')
                print(json.dumps(dict({'metric': 'fine-tune rehearsal step, 2 x 8 structures, HIP graph',
                                       'leg': name, 'options': opts, 'grad': grad, 'steps': args.steps,
                                       'warmup': args.warmup}, **r)), flush=True)


if __name__ == '__main__':
    main()
