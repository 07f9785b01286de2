"""Golden vectors for the fine-tune step, taken from the reference's own
fine-tuning example (read as text; nothing is executed or copied as source):

  example_inputs/fine_tuning/FT_w_reEWC/log.sevenn   "Epoch N/610  lr: X" lines
      -> the cosineannealingwarmuplr schedule (scheduler_param of the same log,
         :67) stepped once per epoch after a fresh reset (reset_scheduler: True)

  example_inputs/fine_tuning/estimate_Fisher/{fisher,opt_params}_sevenn.pt
      -> what tests/test_train.py needs of the two 3.4 MB state dicts: every
         parameter's name and shape in both, the SHA-256 of its optimum's
         float32 bytes (the converted weights must equal it bit for bit) and
         the first FISHER_HEAD Fisher values (the test tiles them to the shape)

usage: python tools/make_train_golden.py [/root/reference]
writes tests/golden/ft_lr_schedule.json and tests/golden/ft_fisher_opt.npz
"""
import hashlib
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(ref='/root/reference'):
    log = open(os.path.join(ref, 'example_inputs/fine_tuning/FT_w_reEWC/log.sevenn')).read()
    sched = re.search(r"scheduler_param\s*:\s*(\{.*?\})", log).group(1)
    param = json.loads(sched.replace("'", '"'))
    lrs = [(int(e), float(lr))
           for e, lr in re.findall(r'Epoch (\d+)/\d+\s+lr: ([0-9.eE+-]+)', log)]
    out = {'source': 'example_inputs/fine_tuning/FT_w_reEWC/log.sevenn',
           'optim_param': {'lr': 0.0}, 'scheduler': 'cosineannealingwarmuplr',
           'scheduler_param': param, 'printed_decimals': 6,
           'epochs': [e for e, _ in lrs], 'lr': [v for _, v in lrs]}
    path = os.path.join(ROOT, 'tests', 'golden', 'ft_lr_schedule.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(path, out)
    fisher_opt(ref)


FISHER_HEAD = 1024


def fisher_opt(ref):
    import torch
    d = os.path.join(ref, 'example_inputs/fine_tuning/estimate_Fisher')
    fisher = torch.load(os.path.join(d, 'fisher_sevenn.pt'), weights_only=True, map_location='cpu')
    opt = torch.load(os.path.join(d, 'opt_params_sevenn.pt'), weights_only=True, map_location='cpu')
    assert all(v.dtype == torch.float32 for v in [*fisher.values(), *opt.values()])
    meta = {'source': 'example_inputs/fine_tuning/estimate_Fisher/{fisher,opt_params}_sevenn.pt',
            'fisher_names': list(fisher), 'opt_names': list(opt), 'params': {}}
    arrays = {}
    for k in opt:
        o = opt[k].contiguous().numpy()
        meta['params'][k] = {'opt_shape': list(o.shape), 'fisher_shape': list(fisher[k].shape),
                             'opt_sha256': hashlib.sha256(o.astype('<f4').tobytes()).hexdigest()}
        arrays['fisher_head/' + k] = fisher[k].numpy().reshape(-1)[:FISHER_HEAD].copy()
    path = os.path.join(ROOT, 'tests', 'golden', 'ft_fisher_opt.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(*sys.argv[1:])
