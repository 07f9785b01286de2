"""Spawned gloo ranks for test_error_recorder_host.py: every rank records its
own batch, then ``ErrorRecorder.reduce()`` makes the sums the group's."""
import os

import numpy as np
import torch

from sevennet_finetuning_amd import _keys as KEY

CONFIG = {'loss': 'huber', 'loss_param': {'delta': 0.01}, 'force_loss_weight': 1.0,
          'stress_loss_weight': 0.01, 'is_train_stress': True,
          'error_record': [['Energy', 'RMSE'], ['Force', 'RMSE'], ['Stress', 'RMSE'],
                           ['Energy', 'MAE'], ['Force', 'MAE'], ['Stress', 'MAE'],
                           ['Force', 'VectorMAE'], ['Force', 'ComponentRMSE'],
                           ['Energy', 'Loss'], ['Force', 'Loss'], ['Stress', 'Loss'],
                           ['TotalLoss', 'None']]}


def rank_batch(seed, nb=3):
    """a float64 CPU (output + labels) dict with a few unlabelled entries"""
    rng = np.random.default_rng(seed)
    natoms = rng.integers(2, 6, nb)
    n = int(natoms.sum())
    f_ref = rng.normal(0, 1, (n, 3))
    f_ref[seed % n, 1] = np.nan
    e_ref = rng.normal(-10, 1, nb)
    s_ref = rng.normal(0, 1e-3, (nb, 6))
    s_ref[nb - 1] = np.nan
    t = torch.as_tensor
    return {KEY.PRED_TOTAL_ENERGY: t(e_ref + rng.normal(0, 0.05, nb)), KEY.ENERGY: t(e_ref),
            KEY.PRED_FORCE: t(np.nan_to_num(f_ref) + rng.normal(0, 0.02, (n, 3))), KEY.FORCE: t(f_ref),
            KEY.PRED_STRESS: t(np.nan_to_num(s_ref) + rng.normal(0, 1e-5, (nb, 6))), KEY.STRESS: t(s_ref),
            KEY.NUM_ATOMS: t(natoms)}


def reduce_worker(rank, world, port, out):
    import torch.distributed as dist
    from sevennet_finetuning_amd.error_recorder import ErrorRecorder
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    rec = ErrorRecorder.from_config(CONFIG)
    rec.update(rank_batch(11 + rank))
    rec.reduce()
    d = rec.get_metric_dict()
    np.savez(out + f'.{rank}.npz', keys=np.array(list(d)), values=np.array(list(d.values())),
             sums=rec.sums.numpy())
    dist.barrier()
    dist.destroy_process_group()
