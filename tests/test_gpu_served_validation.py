"""The served validation pass and the recorders inside the fine-tune step, on
the GPU: (a) e3gnn_set_weights / e3gnn_load_memory against a deployment from
files, (b) Trainer.validate against the eager pass on padded DeviceLoader
batches, (c) the recorders' launches inside the captured rehearsal step,
(d) rehearsal_epochs with ReduceLROnPlateau."""
import json
import math
import os

import numpy as np
import pytest
import torch

from sevennet_finetuning_amd import _keys as KEY
from sevennet_finetuning_amd import _lib, train
from sevennet_finetuning_amd import model_build as mb
from sevennet_finetuning_amd.error_recorder import KBAR, ErrorRecorder
from sevennet_finetuning_amd.model import E3GNNModel
from sevennet_finetuning_amd.train_data import DeviceDataset, DeviceLoader

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HFO2 = os.path.join(ROOT, 'sevennet_finetuning_amd', 'assets', 'hfo2_example')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'finetune_log_header.json')
NS = _lib.ERR_SUMS_PER_QUANTITY
ROWS = [['Energy', 'RMSE'], ['Force', 'RMSE'], ['Stress', 'RMSE'], ['Energy', 'MAE'], ['Force', 'MAE'],
        ['Stress', 'MAE'], ['Energy', 'Loss'], ['Force', 'Loss'], ['Stress', 'Loss'], ['TotalLoss', 'None']]


def config(**kw):
    cfg = {'loss': 'huber', 'loss_param': {'delta': 0.01}, 'force_loss_weight': 1.0,
           'stress_loss_weight': 0.01, 'is_train_stress': True, 'optimizer': 'adam',
           'optim_param': {'lr': 1e-4}, 'scheduler': 'exponentiallr',
           'scheduler_param': {'gamma': 0.99}, 'device': DEV, 'error_record': ROWS,
           'best_metric': 'TotalLoss'}
    cfg.update(kw)
    return cfg


def trainer(**kw):
    from sevennet_finetuning_amd.nn import SevenNetTrainable
    m = SevenNetTrainable(device=DEV)
    fisher = {n: torch.full_like(p, 1e-3) for n, p in m.named_parameters()}
    opt = {n: p.detach().clone() for n, p in m.named_parameters()}
    tr = train.Trainer(m, config(**{'continue': {'fisher_information': fisher, 'opt_params': opt,
                                                 'ewc_lambda': 1e2}, **kw}))
    return m, tr


def coll(seeds, cells=(3, 3, 3)):
    from test_gpu_train import _batch
    return train.collate(_batch(seeds, cells), device=DEV, dtype=torch.float32)


def evaluate(served, g):
    ei = g[KEY.EDGE_IDX]
    r = served.energy_forces(g[KEY.NODE_FEATURE], ei[0], ei[1], g[KEY.EDGE_VEC])
    return {k: r[k].cpu().numpy().copy() for k in ('energy', 'atomic_energy', 'forces', 'virial')}


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------ (a) the refresh
def test_set_weights_equals_a_load_from_memory_and_from_files(tmp_path):
    from sevennet_finetuning_amd.nn import SevenNetTrainable
    from test_gpu_deploy import finetune, graphs
    model = SevenNetTrainable(device=DEV)
    served = E3GNNModel.from_trainable(model)       # its context exists before the refresh
    gs = graphs([5, 6], cells=(2, 2, 2))
    pretrained = [evaluate(served, g) for g in gs]
    finetune(model, steps=3)
    served.set_weights(model.flat)
    from_memory = E3GNNModel.from_trainable(model)
    from_files = E3GNNModel(mb.deploy(model, str(tmp_path / 'ft')), device=DEV)
    for g, pre in zip(gs, pretrained):
        a = evaluate(served, g)
        assert same(a, evaluate(from_memory, g)) and same(a, evaluate(from_files, g))
        assert float(a['energy']) != float(pre['energy'])
    # a host array takes the same route
    served.set_weights(model.flat.detach().cpu().numpy())
    assert same(evaluate(served, gs[0]), evaluate(from_files, gs[0]))
    # refusals leave the model as it was
    want = evaluate(served, gs[0])
    with pytest.raises(_lib.E3GNNError, match='numel'):
        served.set_weights(model.flat[:-1])
    assert same(evaluate(served, gs[0]), want)
    generic = E3GNNModel(HFO2, device=DEV)
    assert generic.family == -1
    pos, cell = np.array([[0.0, 0, 0], [1.1, 1.2, 1.3], [2.5, 0.2, 2.2]]), np.eye(3) * 5.1
    g = train.labeled_graph(pos, cell, np.array([0, 1, 1]), generic.cutoff)
    before = evaluate(generic, g)
    with pytest.raises(_lib.E3GNNError, match='generic-engine'):
        generic.set_weights(np.zeros(16, dtype=np.float32))
    assert same(evaluate(generic, g), before)


# ------------------------------------------------------------ (b) validate
def test_validate_equals_the_eager_pass_on_padded_batches():
    from test_gpu_loader import RC, structure
    S = [structure((3, 3, 3), 300 + k) for k in range(5)]
    loader = DeviceLoader(DeviceDataset.from_structures(S, RC, None, DEV), 2, shuffle=False)
    assert len(loader) == 3
    m, tr = trainer()
    m.train(True)
    tr.rehearsal_step(coll([1]), coll([2]))     # parameters the served model was not made from
    rec_a = tr.validate(loader, ErrorRecorder.from_config(config()))
    rec_b = ErrorRecorder.from_config(config())
    tr.run_one_epoch(loader, False, rec_b)
    emax = 0.0
    for batch in loader:                        # the bound's max |E| over the real slots
        e = m(batch)[KEY.PRED_TOTAL_ENERGY].detach()[~torch.isnan(batch[KEY.ENERGY])]
        emax = max(emax, float(e.abs().max()))
    sa, sb = rec_a.sums.cpu().numpy(), rec_b.sums.cpu().numpy()
    counts = {q: (sa[q * NS + _lib.ERRS_COMPONENTS], sa[q * NS + _lib.ERRS_VECTORS])
              for q in range(_lib.ERR_QUANTITIES)}
    # 5 structures of 54 atoms: the dummy slots and dummy atoms were dropped
    assert counts == {_lib.ERRQ_TOTAL_ENERGY: (5, 5), _lib.ERRQ_ENERGY: (5, 5),
                      _lib.ERRQ_FORCE: (810, 270), _lib.ERRQ_STRESS: (30, 5)}
    idx = [q * NS + s for q in range(_lib.ERR_QUANTITIES) for s in (_lib.ERRS_COMPONENTS, _lib.ERRS_VECTORS)]
    assert np.array_equal(sa[idx], sb[idx])
    a, b = rec_a.epoch_forward(), rec_b.epoch_forward()
    # the served-vs-trainable bars (test_gpu_deploy: E 2e-6 relative, F 1e-4, S 2e-6) bound
    # every residual's change; by the triangle inequality on the residual norms:
    bound = {'Force_RMSE (eV/Å)': math.sqrt(3) * 1e-4, 'Force_MAE (eV/Å)': 1e-4,
             'Energy_RMSE (eV/atom)': 2e-6 * emax / 54, 'Energy_MAE (eV/atom)': 2e-6 * emax / 54,
             'Stress_RMSE (kbar)': math.sqrt(6) * 2e-6 * KBAR, 'Stress_MAE (kbar)': 2e-6 * KBAR}
    for k in a:
        print(f'{k}: served {a[k]:.9g} eager {b[k]:.9g} diff {abs(a[k] - b[k]):.3e}'
              + (f' bound {bound[k]:.3e}' if k in bound else ''))
    for k, v in bound.items():
        assert abs(a[k] - b[k]) <= v, k
    for k in ('Energy_Loss', 'Force_Loss', 'Stress_Loss', 'TotalLoss'):
        assert math.isfinite(a[k]) and a[k] > 0 and math.isfinite(b[k]) and b[k] > 0


# ------------------------------------------------------------ (c) inside the graph
def test_recorders_inside_the_captured_step():
    steps = [(coll([10 + 3 * i, 11 + 3 * i]), coll([12 + 3 * i])) for i in range(6)]

    def run(graph):
        m, tr = trainer(hip_graph=graph)
        m.train(True)
        recs = [ErrorRecorder.from_config(config()) for _ in range(3)]   # train, valid, memory
        for b, mm in steps:
            tr.rehearsal_step(b, mm, recs[0], recs[2])
        return m, tr, recs

    mg, tg, rg = run(True)
    assert tg._graphed.stats['captured'] == 1 and tg._graphed.stats['replayed'] == 5
    assert tg._graphed.stats['eager'] == 0
    for rec, atoms, nb in ((rg[0], 108, 2), (rg[2], 54, 1)):
        s = rec.sums.cpu().numpy()
        # 6 x the batch: not 8 x or 9 x (the warm-ups were rolled back), not 1 x (the
        # launches replay with the graph)
        assert s[_lib.ERRQ_ENERGY * NS + _lib.ERRS_COMPONENTS] == 6 * nb
        assert s[_lib.ERRQ_FORCE * NS + _lib.ERRS_COMPONENTS] == 6 * 3 * atoms
        assert s[_lib.ERRQ_FORCE * NS + _lib.ERRS_VECTORS] == 6 * atoms
        assert s[_lib.ERRQ_STRESS * NS + _lib.ERRS_COMPONENTS] == 6 * 6 * nb
    assert float(rg[1].sums.abs().sum()) == 0
    me, te, re_ = run(False)
    for g, e in ((rg[0], re_[0]), (rg[2], re_[2])):
        dg, de = g.get_metric_dict(), e.get_metric_dict()
        for k in dg:
            print(f'{k}: graphed {dg[k]:.9g} eager {de[k]:.9g}')
            assert abs(dg[k] - de[k]) <= 1e-5 * abs(de[k]), k
    # detached: a new capture, and the old sums are not written any more
    kept = [r.sums.clone() for r in rg]
    tg.rehearsal_step(*steps[0])
    assert tg._graphed.stats['captured'] == 2
    torch.cuda.synchronize()
    assert all(torch.equal(r.sums, k) for r, k in zip(rg, kept))
    # attached again: the first graph replays, and records
    tg.rehearsal_step(*steps[0], rg[0], rg[2])
    assert tg._graphed.stats['captured'] == 2
    assert rg[0].sums[_lib.ERRQ_ENERGY * NS].item() == 7 * 2


# ------------------------------------------------------------ (d) the epoch loop
def test_rehearsal_epochs_rows_and_plateau_scheduler():
    """Three epochs, so that a row follows a non-improving epoch: epoch 0
    improves on the scheduler's initial infinity, epoch 1 cannot (lr 1e-6 and
    an improvement threshold of one half), so row 2 has the reduced rate.
    (With lr 0 the reduced rate would be 0 too and show nothing; and the
    scheduler ignores reductions below its eps of 1e-8.)"""
    m, tr = trainer(optim_param={'lr': 1e-6}, scheduler='reducelronplateau',
                    scheduler_param={'factor': 0.5, 'patience': 0, 'threshold': 0.5})
    small = (2, 2, 2)
    rows = list(train.rehearsal_epochs(tr, [coll([1], small)], [coll([2], small)], [coll([3], small)],
                                       config(), epochs=3))
    with open(GOLDEN, encoding='utf-8') as f:
        golden = json.load(f)
    assert [r['Epoch'] for r in rows] == [0, 1, 2]
    for r in rows:
        assert list(r) == golden
        assert all(math.isfinite(r[k]) for k in golden)
    assert rows[1]['Valid_TotalLoss'] > 0.5 * rows[0]['Valid_TotalLoss']      # no improvement
    assert rows[0]['Learning_rate'] == rows[1]['Learning_rate'] == pytest.approx(1e-6)
    assert rows[2]['Learning_rate'] == pytest.approx(0.5 * rows[1]['Learning_rate'])
    with pytest.raises(KeyError, match='Energy_RMSE'):
        next(train.rehearsal_epochs(tr, [coll([1], small)], [coll([2], small)], [coll([3], small)],
                                    config(best_metric='NoSuchMetric'), epochs=1))
