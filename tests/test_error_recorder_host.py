"""The error recorder without a GPU: the reference's ``from_config`` rules and
metric keys, the torch definition of the device sums against hand-written
numbers, ``epoch_forward`` / ``reduce``, and the argument rules of the three
new C entries (refused before any HIP call)."""
import ctypes
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from sevennet_finetuning_amd import _keys as KEY
from sevennet_finetuning_amd import _lib, train
from sevennet_finetuning_amd.error_recorder import (GPA, KBAR, ErrorRecorder, csv_header,
                                                    error_sums_torch)

ERR_ARG = 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'finetune_log_header.json')


def reference_config():
    """the training section of the reference's FT_w_reEWC/input_full.yaml that the recorder reads"""
    return {'is_train_stress': True, 'loss': 'Huber', 'loss_param': {'delta': 0.01},
            'force_loss_weight': 1.00, 'stress_loss_weight': 0.01,
            'error_record': [['Energy', 'RMSE'], ['Force', 'RMSE'], ['Stress', 'RMSE'],
                             ['Energy', 'MAE'], ['Force', 'MAE'], ['Stress', 'MAE'],
                             ['Energy', 'Loss'], ['Force', 'Loss'], ['Stress', 'Loss'],
                             ['TotalLoss', 'None']],
            'best_metric': 'TotalLoss'}


def test_from_config_on_the_reference_input_and_its_log_header():
    rec = ErrorRecorder.from_config(reference_config())
    assert rec.criterion == (1, 0.01)
    assert (rec.force_weight, rec.stress_weight) == (1.0, 0.01) and rec.stress
    assert rec.keys() == ['Energy_RMSE (eV/atom)', 'Force_RMSE (eV/Å)', 'Stress_RMSE (kbar)',
                          'Energy_MAE (eV/atom)', 'Force_MAE (eV/Å)', 'Stress_MAE (kbar)',
                          'Energy_Loss', 'Force_Loss', 'Stress_Loss', 'TotalLoss']
    with open(GOLDEN, encoding='utf-8') as f:
        golden = json.load(f)
    assert csv_header(rec) == golden and train.csv_header(rec) == golden
    assert (KEY.ERROR_RECORD, KEY.BEST_METRIC) == ('error_record', 'best_metric')


def test_from_config_rules():
    cfg = reference_config()
    cfg['is_train_stress'] = False
    rec = ErrorRecorder.from_config(cfg)
    assert not any('Stress' in k for k in rec.keys()) and len(rec.keys()) == 7
    assert not rec.stress and rec.stress_weight is None
    cfg = reference_config()
    cfg['error_record'] = [['TotalEnergy', 'MAE'], ['Stress_GPa', 'RMSE'], ['Force', 'VectorMAE'],
                           ['Force', 'ComponentRMSE'], ['EWCLoss', 'None']]
    cfg['continue'] = {'ewc_lambda': 100.0}
    rec = ErrorRecorder.from_config(cfg)
    assert rec.keys() == ['Energy_MAE (eV)', 'Stress_RMSE (GPa)', 'Force_VectorMAE (eV/Å)',
                          'Force_ComponentRMSE (eV/Å)', 'EWC']
    assert rec.wants_ewc
    cfg['loss'], cfg['loss_param'] = 'mse', {}
    assert ErrorRecorder.from_config(cfg).criterion == (0, 0.0)
    # a Huber loss in GPa is not a rescaled Huber loss in kbar: refused, not misreported
    cfg = reference_config()
    cfg['error_record'] = [['Stress_GPa', 'Loss']]
    with pytest.raises(ValueError, match='Stress_GPa'):
        ErrorRecorder.from_config(cfg)
    cfg['loss'] = 'mse'
    assert ErrorRecorder.from_config(cfg).keys() == ['Stress_Loss']


def hand_case(stress=None):
    """2 structures (2 atoms, 1 atom): one unlabelled energy, one unlabelled
    force component (with a NaN prediction under it), stress all unlabelled"""
    nan = math.nan
    t = lambda a: torch.tensor(a, dtype=torch.float64)   # noqa: E731
    return {KEY.PRED_TOTAL_ENERGY: t([1.0, 3.0]), KEY.ENERGY: t([0.5, nan]),
            KEY.NUM_ATOMS: torch.tensor([2, 1]),
            KEY.PRED_FORCE: t([[1, 0, 0], [0, 2, 0], [nan, 0, 0.5]]),
            KEY.FORCE: t([[0, 0, 0], [0, 0, 0], [nan, 0, 0]]),
            KEY.PRED_STRESS: t([[1.0] * 6, [math.inf] * 6]),
            KEY.STRESS: t([[nan] * 6] * 2) if stress is None else t(stress)}


ALL_ROWS = [[t, m] for t in ('TotalEnergy', 'Energy', 'Force', 'Stress')
            for m in ('RMSE', 'ComponentRMSE', 'MAE', 'VectorMAE', 'Loss')] + [['TotalLoss', 'None']]


def test_sums_against_hand_numbers():
    cfg = {'is_train_stress': True, 'loss': 'huber', 'loss_param': {'delta': 0.75},
           'force_loss_weight': 2.0, 'stress_loss_weight': 0.5, 'error_record': ALL_ROWS}
    rec = ErrorRecorder.from_config(cfg)
    out = hand_case()
    labels = {k: out.pop(k) for k in (KEY.ENERGY, KEY.FORCE, KEY.STRESS, KEY.NUM_ATOMS)}
    rec.update(out, labels)              # the labels are looked up in the batch
    s = rec.sums.numpy().reshape(_lib.ERR_QUANTITIES, _lib.ERR_SUMS_PER_QUANTITY)
    #                   components vectors |d|  d^2   ||d|| crit     d^2 of full vectors
    assert list(s[_lib.ERRQ_TOTAL_ENERGY]) == [1, 1, 0.5, 0.25, 0.5, 0.125, 0.25]
    assert list(s[_lib.ERRQ_ENERGY]) == [1, 1, 0.25, 0.0625, 0.25, 0.03125, 0.0625]
    # crit: 0.75 (1 - 0.375) + 0.75 (2 - 0.375) + 0.5 * 0.25
    assert list(s[_lib.ERRQ_FORCE]) == [8, 2, 3.5, 5.25, 3.0, 1.8125, 5.0]
    assert list(s[_lib.ERRQ_STRESS]) == [0] * 7
    m = rec.get_metric_dict()
    assert m['Energy_RMSE (eV)'] == 0.5 and m['Energy_MAE (eV)'] == 0.5
    assert m['Energy_RMSE (eV/atom)'] == 0.25 and m['Energy_MAE (eV/atom)'] == 0.25
    assert m['Energy_VectorMAE (eV/atom)'] == 0.25 and m['Energy_ComponentRMSE (eV/atom)'] == 0.25
    # the MAE keeps the two labelled components of the third atom; RMSE and VectorMAE drop it
    assert m['Force_MAE (eV/Å)'] == 3.5 / 8
    assert m['Force_ComponentRMSE (eV/Å)'] == math.sqrt(5.25 / 8)
    assert m['Force_RMSE (eV/Å)'] == math.sqrt(5.0 / 2)
    assert m['Force_VectorMAE (eV/Å)'] == 1.5
    assert m['Energy_Loss'] == 0.03125 and m['Force_Loss'] == 1.8125 / 8
    for k in ('Stress_RMSE (kbar)', 'Stress_ComponentRMSE (kbar)', 'Stress_MAE (kbar)',
              'Stress_VectorMAE (kbar)', 'Stress_Loss', 'TotalLoss'):
        assert math.isnan(m[k]), k
    # without stress training the total is finite: E + w_F F
    cfg.update(is_train_stress=False)
    rec2 = ErrorRecorder.from_config(cfg)
    rec2.update(hand_case())
    assert rec2.get_metric_dict()['TotalLoss'] == 0.03125 + 2.0 * 1.8125 / 8
    # MSE: crit = d^2
    cfg.update(loss='mse')
    rec3 = ErrorRecorder.from_config(cfg)
    rec3.update(hand_case())
    assert rec3.get_metric_dict()['Force_Loss'] == 5.25 / 8


def test_stress_units_and_total_loss():
    k32 = float(np.float32(KBAR))
    stress = [[1e-3, 0, 0, 0, 0, 0], [0, 0, 0, 0, -2e-3, 0]]
    case = hand_case(stress)
    case[KEY.PRED_STRESS] = torch.zeros(2, 6, dtype=torch.float64)
    cfg = {'is_train_stress': True, 'loss': 'huber', 'loss_param': {'delta': 0.75},
           'force_loss_weight': 2.0, 'stress_loss_weight': 0.5,
           'error_record': ALL_ROWS + [['Stress_GPa', 'RMSE'], ['Stress_GPa', 'MAE'],
                                       ['Stress_GPa', 'VectorMAE']]}
    rec = ErrorRecorder.from_config(cfg)
    rec.update(case)
    m = rec.get_metric_dict()
    d1, d2 = 1e-3 * k32, 2e-3 * k32              # kbar: both beyond delta
    assert m['Stress_RMSE (kbar)'] == pytest.approx(math.sqrt((d1 * d1 + d2 * d2) / 2), rel=1e-14)
    assert m['Stress_MAE (kbar)'] == pytest.approx((d1 + d2) / 12, rel=1e-14)
    assert m['Stress_VectorMAE (kbar)'] == pytest.approx((d1 + d2) / 2, rel=1e-14)
    s_loss = (0.75 * (d1 - 0.375) + 0.75 * (d2 - 0.375)) / 12
    assert m['Stress_Loss'] == pytest.approx(s_loss, rel=1e-14)
    assert m['TotalLoss'] == pytest.approx(0.03125 + 2.0 * 1.8125 / 8 + 0.5 * s_loss, rel=1e-14)
    # GPa from the kbar sums by the linear factor
    assert GPA / KBAR == pytest.approx(0.1, rel=1e-15)
    for name in ('RMSE', 'MAE', 'VectorMAE'):
        assert m[f'Stress_{name} (GPa)'] == pytest.approx(m[f'Stress_{name} (kbar)'] / 10, rel=1e-14)


def test_epoch_forward_resets_and_the_history_grows():
    rec = ErrorRecorder.from_config(reference_config())
    assert all(math.isnan(v) for v in rec.get_metric_dict().values())   # a count of 0 gives NaN
    rec.update(hand_case([[0.0] * 6] * 2))
    ptr = rec.buffer().data_ptr()
    snap = rec.snapshot()
    rec.update(hand_case([[0.0] * 6] * 2))
    assert rec.sums[_lib.ERRQ_FORCE * _lib.ERR_SUMS_PER_QUANTITY].item() == 16
    rec.restore(snap)                                   # the second update rolled back
    assert rec.sums[_lib.ERRQ_FORCE * _lib.ERR_SUMS_PER_QUANTITY].item() == 8
    first = rec.epoch_forward()
    assert first['Force_MAE (eV/Å)'] == 3.5 / 8 and rec.get_history() == [first]
    assert float(rec.sums.abs().sum()) == 0 and rec.buffer().data_ptr() == ptr
    second = rec.epoch_forward()
    assert len(rec.get_history()) == 2 and math.isnan(second['Force_MAE (eV/Å)'])


def test_ewc_value_is_the_first_update_after_a_reset():
    cfg = reference_config()
    cfg['error_record'] = [['EWCLoss', 'None']]
    cfg['continue'] = {'ewc_lambda': 2.0}
    rec = ErrorRecorder.from_config(cfg)
    assert math.isnan(rec.get_metric_dict()['EWC'])
    rec.update(hand_case(), ewc=torch.tensor([0.25]))
    rec.update(hand_case(), ewc=torch.tensor([0.75]))
    assert rec.epoch_forward()['EWC'] == 0.25
    rec.update(hand_case(), ewc=torch.tensor([0.75]))
    assert rec.epoch_forward()['EWC'] == 0.75


def test_reduce_over_two_gloo_ranks(tmp_path):
    from _recorder_workers import CONFIG, rank_batch, reduce_worker
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    out = str(tmp_path / 'rec')
    mp.spawn(reduce_worker, args=(2, port, out), nprocs=2, join=True)
    one = ErrorRecorder.from_config(CONFIG)
    one.update(rank_batch(11))
    one.update(rank_batch(12))
    want = one.get_metric_dict()
    assert all(math.isfinite(v) for v in want.values())
    for rank in range(2):
        got = np.load(out + f'.{rank}.npz')
        assert list(got['keys']) == list(want)
        # counts exact; two f64 terms per slot added in either order
        assert np.array_equal(got['sums'], one.sums.numpy())
        assert np.array_equal(got['values'], np.array(list(want.values())))


def test_new_entries_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in ('e3gnn_error_sums', 'e3gnn_load_memory', 'e3gnn_set_weights'):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.e3gnn_abi_version() == 1
    assert _lib.ERR_SUMS == 28 == error_sums_torch(0, 0.0, torch.zeros(0), torch.zeros(0),
                                                   torch.zeros(0)).numel()


def test_error_sums_argument_rules():
    """Every rule returns E3GNN_ERR_ARG with its message before any HIP call:
    the pointers are fakes that are never dereferenced."""
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)
    good = dict(criterion=1, delta=0.01, nb=2, n=5, e_pred=fake, e_ref=fake, natoms=fake, f_pred=fake,
                f_ref=fake, s_pred=fake, s_ref=fake, s_scale=1.0, sums=fake)

    def refused(**change):
        a = {**good, **change}
        rc = lib.e3gnn_error_sums(*[a[k] for k in good], None)
        assert rc == ERR_ARG, rc
        return lib.e3gnn_last_error().decode()

    assert 'null sums' in refused(sums=None)
    assert 'criterion' in refused(criterion=2)
    assert 'criterion' in refused(criterion=-1)
    assert 'out of range' in refused(nb=-1)
    assert 'out of range' in refused(n=-1)
    assert 'out of range' in refused(n=1 << 31)
    assert 'out of range' in refused(nb=1 << 31)
    assert 'go together' in refused(f_ref=None)
    assert 'go together' in refused(s_pred=None)
    assert 'go together' in refused(e_ref=None)
    assert 'null natoms' in refused(natoms=None)
    assert 'null energies' in refused(e_pred=None, e_ref=None)
    # nb = 0 with n = 0: nothing to do, and nothing is touched
    a = {**good, 'nb': 0, 'n': 0}
    assert lib.e3gnn_error_sums(*[a[k] for k in good], None) == 0


def test_load_memory_and_set_weights_argument_rules():
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)
    assert not lib.e3gnn_load_memory(None, fake, 4, 0)
    assert 'null manifest or weights' in lib.e3gnn_last_error().decode()
    assert not lib.e3gnn_load_memory(b'{}', None, 4, 0)
    assert 'null manifest or weights' in lib.e3gnn_last_error().decode()
    assert not lib.e3gnn_load_memory(b'{}', fake, -1, 0)
    assert 'negative numel' in lib.e3gnn_last_error().decode()
    assert lib.e3gnn_set_weights(None, fake, 4, None) == ERR_ARG
    assert 'null model' in lib.e3gnn_last_error().decode()


def test_trainer_signatures_are_the_references():
    import inspect
    p = inspect.signature(train.Trainer.run_one_epoch).parameters
    assert list(p) == ['self', 'loader', 'is_train', 'error_recorder']
    assert p['is_train'].default is False and p['error_recorder'].default is None
    p = inspect.signature(train.Trainer.run_one_epoch_rehearsal).parameters
    assert list(p) == ['self', 'loader', 'memloader', 'is_train', 'error_recorder', 'mem_recorder']
    assert p['error_recorder'].default is None and p['mem_recorder'].default is None
    assert callable(train.Trainer.validate) and callable(train.rehearsal_epochs)
