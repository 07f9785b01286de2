"""The reference's error recorder surface (sevenn/error_recorder.py:11-432)
on sums kept on the device.

The reference accumulates every metric with one ``.item()`` per metric per
batch (error_recorder.py:66-68): a host synchronisation inside every step,
which the captured fine-tune step exists to avoid.  Here one recorder owns
one persistent float64 device buffer; ``update`` adds a batch's sums to it
with one ``e3gnn_error_sums`` launch on the current stream (no
synchronisation, capturable in a HIP graph), and ``epoch_forward`` makes the
one device-to-host copy of the epoch and finalises every metric from the sums:

    RMSE          sqrt(sum d^2 over fully labelled vectors / their count)
    ComponentRMSE sqrt(sum d^2 / labelled components)
    MAE           sum |d| / labelled components
    VectorMAE     sum ||d|| / fully labelled vectors
    Loss          sum crit(d) / labelled components   (crit: the config's MSE or Huber)
    TotalLoss     Energy_Loss + w_F Force_Loss (+ w_S Stress_Loss)

(energy per atom; stress in kbar inside the criterion, as ``StressLoss``).  A
NaN label drops its component alone (``delete_unlabled``); a vector counts
towards RMSE and VectorMAE only when all its components are labelled; a count
of zero gives NaN (``AverageNumber.get``).  The layout of the sums is the enum
of include/e3gnn.h (``_lib.ERRQ_*`` / ``_lib.ERRS_*``).

CPU tensors, or any dtype other than float32, take ``error_sums_torch``: the
same sums by torch in float64, the executable definition the kernel is tested
against.  Both convert to float64 before subtracting and multiply the stress
difference by the float32 value of the unit factor.
"""
import math

import numpy as np
import torch

from . import _keys as KEY
from . import _lib

KBAR = 1602.1766208          # eV/A^3 -> kbar (StressLoss.TO_KB)
GPA = 160.21766208

# error_recorder.py:11-58
ERROR_TYPES = {
    'TotalEnergy': {'name': 'Energy', 'unit': 'eV', 'quantity': _lib.ERRQ_TOTAL_ENERGY},
    'Energy': {'name': 'Energy', 'unit': 'eV/atom', 'quantity': _lib.ERRQ_ENERGY},
    'Force': {'name': 'Force', 'unit': 'eV/Å', 'quantity': _lib.ERRQ_FORCE},
    'Stress': {'name': 'Stress', 'unit': 'kbar', 'quantity': _lib.ERRQ_STRESS},
    # finalised from the kbar sums by the linear factor
    'Stress_GPa': {'name': 'Stress', 'unit': 'GPa', 'quantity': _lib.ERRQ_STRESS,
                   'factor': GPA / KBAR},
    'TotalLoss': {'name': 'TotalLoss', 'unit': None},
    'EWCLoss': {'name': 'EWC', 'unit': None},
}
METRICS = ('RMSE', 'ComponentRMSE', 'MAE', 'VectorMAE', 'Loss')
ERROR_RECORD, BEST_METRIC = KEY.ERROR_RECORD, KEY.BEST_METRIC

_NS = _lib.ERR_SUMS_PER_QUANTITY
# the buffer: the kernel's sums, then the EWC value and its "set" flag
_EWC_VALUE, _EWC_SET, _BUF = _lib.ERR_SUMS, _lib.ERR_SUMS + 1, _lib.ERR_SUMS + 2


def _f32(x):
    return float(np.float32(x))


def error_sums_torch(criterion, delta, e_pred, e_ref, natoms, f_pred=None, f_ref=None,
                     s_pred=None, s_ref=None, s_scale=KBAR):
    """``e3gnn_error_sums`` by torch in float64: the sums of one batch as a
    float64 tensor [ERR_SUMS] (not accumulated).  The definition of the
    kernel: the same terms in float64 from the same inputs (``delta`` and
    ``s_scale`` at their float32 values, which is what the C entry receives);
    only the order of the additions differs."""
    dev = e_pred.device
    out = torch.zeros(_lib.ERR_SUMS, dtype=torch.float64, device=dev)
    delta, s_scale = _f32(delta), _f32(s_scale)

    def quantity(q, pred, ref, vdim, div=None, scale=None):
        p = pred.detach().reshape(-1, vdim).to(torch.float64)
        r = ref.detach().reshape(-1, vdim).to(device=dev, dtype=torch.float64)
        ok = ~torch.isnan(r)
        d = p - r
        if div is not None:
            d = d / div.detach().reshape(-1, 1).to(device=dev, dtype=torch.float64)
        if scale is not None:
            d = d * scale
        zero = torch.zeros_like(d)
        d = torch.where(ok, d, zero)      # a dropped label's prediction enters no sum
        sq = d * d
        vsq = sq[:, 0]
        for c in range(1, vdim):
            vsq = vsq + sq[:, c]
        full = ok.all(dim=1)
        if criterion == 0:
            cr = sq
        else:
            a = d.abs()
            cr = torch.where(a < delta, 0.5 * d * d, delta * (a - 0.5 * delta))
        cr = torch.where(ok, cr, zero)
        vzero = torch.zeros_like(vsq)
        o = q * _NS
        out[o + _lib.ERRS_COMPONENTS] = ok.sum().to(torch.float64)
        out[o + _lib.ERRS_VECTORS] = full.sum().to(torch.float64)
        out[o + _lib.ERRS_ABS] = d.abs().sum()
        out[o + _lib.ERRS_SQ] = vsq.sum()
        out[o + _lib.ERRS_NORM] = torch.where(full, vsq.sqrt(), vzero).sum()
        out[o + _lib.ERRS_CRIT] = cr.sum()
        out[o + _lib.ERRS_SQ_VECTORS] = torch.where(full, vsq, vzero).sum()

    if e_pred.numel():
        quantity(_lib.ERRQ_TOTAL_ENERGY, e_pred, e_ref, 1)
        quantity(_lib.ERRQ_ENERGY, e_pred, e_ref, 1, div=natoms)
    if f_pred is not None and f_pred.numel():
        quantity(_lib.ERRQ_FORCE, f_pred, f_ref, 3)
    if s_pred is not None and s_pred.numel():
        quantity(_lib.ERRQ_STRESS, s_pred, s_ref, 6, scale=s_scale)
    return out


class ErrorMetric:
    """One column of the record: an error type (``ERROR_TYPES``) and a metric
    (``METRICS``), or one of the specials ``TotalLoss`` / ``EWCLoss``.
    ``key_str`` is the reference's (error_recorder.py:135-139)."""

    def __init__(self, err_type, metric):
        t = ERROR_TYPES[err_type]
        self.err_type, self.metric = err_type, metric
        self.special = err_type in ('TotalLoss', 'EWCLoss')
        self.name = t['name'] if self.special else f"{t['name']}_{metric}"
        self.unit = None if self.special or metric == 'Loss' else t['unit']
        self.quantity = t.get('quantity')
        self.factor = t.get('factor', 1.0)

    def key_str(self):
        return self.name if self.unit is None else f'{self.name} ({self.unit})'


def _ratio(num, den):
    return num / den if den > 0 else math.nan


def _finalise(metric, h, o):
    c, v = h[o + _lib.ERRS_COMPONENTS], h[o + _lib.ERRS_VECTORS]
    if metric == 'RMSE':
        return math.sqrt(_ratio(h[o + _lib.ERRS_SQ_VECTORS], v)) if v > 0 else math.nan
    if metric == 'ComponentRMSE':
        return math.sqrt(_ratio(h[o + _lib.ERRS_SQ], c)) if c > 0 else math.nan
    if metric == 'MAE':
        return _ratio(h[o + _lib.ERRS_ABS], c)
    if metric == 'VectorMAE':
        return _ratio(h[o + _lib.ERRS_NORM], v)
    return _ratio(h[o + _lib.ERRS_CRIT], c)     # Loss


class ErrorRecorder:
    """error_recorder.py:317-432 on device sums.  ``criterion``: (0, 0.0) MSE
    or (1, delta) Huber; ``weights``: (w_F, w_S or None without stress
    training) of ``TotalLoss``.

    ``EWCLoss``: the value is w x the EWC term as the step computed it, on the
    recorder's first update after a reset, i.e. at the parameters that step
    started from.  The reference evaluates it after that step's optimizer
    update (trainer.py: ``update_not_only_data`` follows ``optimizer.step``),
    one step later.  It is held on the device and converted at
    ``epoch_forward``."""

    def __init__(self, metrics, criterion=(0, 0.0), weights=(1.0, None)):
        self.history = []
        self.metrics = list(metrics)
        self.criterion = (int(criterion[0]), float(criterion[1]))
        self.force_weight, self.stress_weight = weights
        self.stress = self.stress_weight is not None or any(
            m.quantity == _lib.ERRQ_STRESS for m in self.metrics)
        self.wants_ewc = any(m.err_type == 'EWCLoss' for m in self.metrics)
        self._buf = None
        self._lib = None

    # ------------------------------------------------------------ the buffer
    def buffer(self, device=None):
        """The persistent float64 buffer (created on first use, on ``device``;
        zeroed in place at every epoch, never replaced: a captured graph that
        records into it stays valid)."""
        if self._buf is None:
            self._buf = torch.zeros(_BUF, dtype=torch.float64, device=device or 'cpu')
        return self._buf

    @property
    def sums(self):
        return self.buffer()[:_lib.ERR_SUMS]

    def snapshot(self):
        """A copy of the sums (and the EWC value), for ``restore``: the graphed
        step's warm-ups are rolled back out of the record."""
        return None if self._buf is None else self._buf.clone()

    def restore(self, snap):
        if self._buf is None:
            return
        if snap is None:
            self._buf.zero_()
        else:
            self._buf.copy_(snap)

    # ------------------------------------------------------------ recording
    @staticmethod
    def _label(key, output, batch):
        if key in output:
            return output[key]
        if batch is not None and key in batch:
            return batch[key]
        raise KeyError(f'no label {key!r} in the output or the batch')

    def update(self, output, batch=None, ewc=None):
        """Add one batch: predictions from ``output``, labels from ``output``,
        then ``batch``.  ``ewc``: the weighted EWC term of this step (a scalar
        tensor), kept on the first update after a reset.  No synchronisation."""
        E = output[KEY.PRED_TOTAL_ENERGY].detach()
        F = output[KEY.PRED_FORCE].detach()
        S = output[KEY.PRED_STRESS].detach() if self.stress else None
        Er, Fr = self._label(KEY.ENERGY, output, batch), self._label(KEY.FORCE, output, batch)
        Sr = self._label(KEY.STRESS, output, batch) if self.stress else None
        natoms = self._label(KEY.NUM_ATOMS, output, batch)
        buf = self.buffer(E.device)
        ts = [t for t in (E, F, S, Er, Fr, Sr) if t is not None]
        if all(t.is_cuda and t.dtype == torch.float32 for t in ts) and natoms.is_cuda and buf.is_cuda:
            if self._lib is None:
                self._lib = _lib.load()
            c = [t.contiguous() if t is not None else None for t in (E, Er, F, Fr, S, Sr)]
            na = natoms.to(torch.long).contiguous()
            p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
            nb, n = int(E.numel()), int(F.shape[0])
            if any(t is not None and t.numel() != k for t, k in
                   zip(c, (nb, nb, 3 * n, 3 * n, 6 * nb, 6 * nb))) or na.numel() != nb:
                raise ValueError('error recorder: predictions and labels differ in shape')
            with torch.cuda.device(E.device):
                _lib.check(self._lib.e3gnn_error_sums(
                    self.criterion[0], self.criterion[1], nb, n, p(c[0]), p(c[1]), p(na), p(c[2]),
                    p(c[3]), p(c[4]), p(c[5]), KBAR, buf.data_ptr(),
                    torch.cuda.current_stream(E.device).cuda_stream))
        else:
            s = error_sums_torch(self.criterion[0], self.criterion[1], E, Er, natoms, F, Fr, S, Sr, KBAR)
            buf[:_lib.ERR_SUMS] += s.to(buf.device)
        if ewc is not None and self.wants_ewc:
            v = ewc.detach().reshape(-1)[0].to(buf.device, torch.float64)
            buf[_EWC_VALUE] = torch.where(buf[_EWC_SET] > 0, buf[_EWC_VALUE], v)
            buf[_EWC_SET] = 1.0

    def reduce(self):
        """One all-reduce of the sums over the process group (the reference
        reduces every metric's sum and count on their own, error_recorder.py:70-76)."""
        import torch.distributed as dist
        dist.all_reduce(self.buffer()[:_lib.ERR_SUMS], op=dist.ReduceOp.SUM)

    # ------------------------------------------------------------ reading
    def _metrics_of(self, h):
        out = {}
        for m in self.metrics:
            if m.err_type == 'EWCLoss':
                out[m.key_str()] = float(h[_EWC_VALUE]) if h[_EWC_SET] > 0 else math.nan
            elif m.err_type == 'TotalLoss':
                val = _finalise('Loss', h, _lib.ERRQ_ENERGY * _NS)
                val += self.force_weight * _finalise('Loss', h, _lib.ERRQ_FORCE * _NS)
                if self.stress_weight is not None:
                    val += self.stress_weight * _finalise('Loss', h, _lib.ERRQ_STRESS * _NS)
                out[m.key_str()] = val
            else:
                f = m.factor ** 2 if m.metric == 'Loss' else m.factor   # (Loss: MSE only, from_config)
                out[m.key_str()] = _finalise(m.metric, h, m.quantity * _NS) * f
        return out

    def get_metric_dict(self):
        """The metrics of the sums so far (one device-to-host copy)."""
        return self._metrics_of(self.buffer().detach().cpu().numpy())

    def epoch_forward(self):
        """The epoch's metrics appended to the history; the buffer zeroed in place."""
        self.history.append(self.get_metric_dict())
        self.buffer().zero_()
        return self.history[-1]

    def get_history(self):
        return self.history

    def keys(self):
        return [m.key_str() for m in self.metrics]

    # ------------------------------------------------------------ from_config
    @staticmethod
    def from_config(config):
        """error_recorder.py:395-432: the rows of ``error_record``, the
        'Stress' rows dropped without stress training."""
        loss = str(config['loss']).lower()
        param = config.get('loss_param', {}) or {}
        if loss == 'mse':
            criterion = (0, 0.0)
        elif loss == 'huber':
            criterion = (1, float(param.get('delta', 1.0)))
        else:
            raise NotImplementedError(f'error recorder: loss {config["loss"]!r} (mse or huber)')
        stress = bool(config['is_train_stress'])
        metrics = []
        for err_type, metric in config[ERROR_RECORD]:
            if not stress and 'Stress' in err_type:
                continue
            if err_type not in ERROR_TYPES:
                raise KeyError(f'unknown error type {err_type!r}: {", ".join(ERROR_TYPES)}')
            if err_type == 'EWCLoss':
                assert float(config['continue']['ewc_lambda']) != 0
            elif err_type != 'TotalLoss':
                if metric not in METRICS:
                    raise KeyError(f'unknown metric {metric!r}: {", ".join(METRICS)}')
                if err_type == 'Stress_GPa' and metric == 'Loss' and criterion[0] == 1:
                    raise ValueError(
                        "error_record ['Stress_GPa', 'Loss'] with the Huber loss: the criterion is "
                        'not linear in the unit and the sums are kept in kbar; record '
                        "['Stress', 'Loss'] instead")
            metrics.append(ErrorMetric(err_type, metric))
        return ErrorRecorder(metrics, criterion,
                             (float(config['force_loss_weight']),
                              float(config['stress_loss_weight']) if stress else None))


def csv_header(recorder):
    """The reference's log.csv header (processing_epoch_with_rehearsal.py:29-35)."""
    header = ['Epoch', 'Learning_rate']
    for k in recorder.keys():
        header += [f'Train_{k}', f'Valid_{k}', f'Memory_{k}']
    return header
