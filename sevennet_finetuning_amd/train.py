"""Fine-tune step (rehearsal + EWC, data parallel) over the trainable HIP
model -- SURVEY.md §8f row 1, BASELINE config 5.

Mirrors, by name and behaviour:
  LossDefinition / PerAtomEnergyLoss / ForceLoss / StressLoss / EWCLoss,
  get_loss_functions_from_config          sevenn/train/loss.py:8-309
  optim_dict / scheduler_dict / loss_dict sevenn/train/optim.py
  Trainer.run_one_epoch, compute_fisher_matrix,
  RehearsalTrainer.run_one_epoch_rehearsal  sevenn/train/trainer.py:15-222
  PyG Collater of AtomGraphData           sevenn/train/collate.py, torch_geometric
                                          (edge_index offset by the running atom
                                          count, ``batch`` vector, per-graph rows)

Data parallelism: one process per GPU (torch.distributed, backend "nccl" =
RCCL over xGMI; "gloo" in the CPU tests).  Where the reference wraps the model
in DDP (trainer.py:18-23), this build keeps every parameter gradient in ONE
contiguous buffer (``SevenNetTrainable.flat_grad``) and averages it with a
single all-reduce after each backward -- the same arithmetic as DDP's
bucketed averaging (earlier, already-synchronised accumulation + the mean of
the new contributions), one collective of 3.4 MB per backward.
"""
import contextlib
import gc
import math
import os

import numpy as np
import torch

from . import _keys as KEY


@contextlib.contextmanager
def _capturing(g, pool=None):
    """``torch.cuda.graph(g, pool=pool)`` with the cyclic garbage collector
    held off.  torch no longer collects before a capture, so a dead reference
    cycle that owns a CUDAGraph (a dropped Trainer and its graphed step) could
    be freed by a collection that happens to start inside the capture; the
    graph's destructor then makes HIP calls that are illegal while a stream
    captures, and the process aborts.  Collect first, then keep the collector
    off until the capture has ended."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, pool=pool):
            yield
    finally:
        if was_enabled:
            gc.enable()

# config keys (sevenn/_keys.py:100-233)
LOSS, LOSS_PARAM = 'loss', 'loss_param'
OPTIMIZER, OPTIM_PARAM = 'optimizer', 'optim_param'
SCHEDULER, SCHEDULER_PARAM = 'scheduler', 'scheduler_param'
FORCE_WEIGHT, STRESS_WEIGHT = 'force_loss_weight', 'stress_loss_weight'
IS_TRAIN_STRESS, DEVICE = 'is_train_stress', 'device'
CONTINUE, FISHER, OPT_PARAMS, EWC_LAMBDA = 'continue', 'fisher_information', 'opt_params', \
    'ewc_lambda'
LOAD_DATASET_WITH_WEIGHTS, DATA_WEIGHT = 'load_dataset_with_weights', 'data_weight'
PER_ATOM_ENERGY = 'per_atom_energy'
IS_DDP, LOCAL_RANK = 'is_ddp', 'local_rank'
HIP_GRAPH = 'hip_graph'
BLAS = 'blas'
# EXPLICIT_GRAD (this build, default on where it applies): the loss gradient by
# the hand-scheduled derivatives of train_explicit.py instead of autograd's
# double backward (same values; a few hundred launches per batch, not thousands)
EXPLICIT_GRAD = 'explicit_grad'


# ------------------------------------------------------------------ losses
class LossDefinition:
    """loss.py:8-94: criterion on flattened (pred, ref), NaN labels dropped."""

    def __init__(self, name, unit=None, criterion=None, ref_key=None, pred_key=None,
                 vdim=None, use_weight=False, weight_key=None, delete_unlabled=True):
        if criterion is not None and hasattr(criterion, 'reduction'):
            if use_weight:
                assert criterion.reduction == 'none'
                assert weight_key is not None
            else:
                assert criterion.reduction != 'none'
        assert isinstance(vdim, int)
        self.name, self.unit, self.vdim = name, unit, vdim
        self.criterion = criterion
        self.ref_key, self.pred_key = ref_key, pred_key
        self.use_weight, self.weight_key = use_weight, weight_key
        self.delete_unlabeled = delete_unlabled

    def assign_criteria(self, criterion):
        if self.criterion is not None:
            raise ValueError('Loss uses its own criterion.')
        self.criterion = criterion

    def _preprocess(self, batch_data, model=None):
        if self.pred_key is None or self.ref_key is None:
            raise NotImplementedError('LossDefinition is not implemented.')
        return (torch.reshape(batch_data[self.pred_key], (-1,)),
                torch.reshape(batch_data[self.ref_key], (-1,)))

    def _get_data_weight(self, batch_data):
        return torch.repeat_interleave(batch_data[DATA_WEIGHT][self.weight_key], self.vdim)

    # static = True: no data-dependent shapes (the HIP-graph-captured step):
    # unlabeled entries get ref := pred (zero loss, zero gradient) and the mean
    # is rescaled from all entries to the labelled ones -- the same value as
    # dropping them, without a host round trip
    static = False

    def get_loss(self, batch_data, model=None):
        if self.criterion is None:
            raise NotImplementedError('LossDefinition has no criterion.')
        pred, ref = self._preprocess(batch_data, model)
        weights = self._get_data_weight(batch_data) if self.use_weight else None
        if self.delete_unlabeled and self.static:
            keep = ~torch.isnan(ref)
            ref = torch.where(keep, ref, pred.detach())
            scale = ref.numel() / keep.sum().clamp_min(1).to(pred.dtype)
            if self.use_weight:
                return torch.mean(self.criterion(pred, ref) * weights) * scale
            return self.criterion(pred, ref) * scale
        if self.delete_unlabeled:
            keep = ~torch.isnan(ref)
            pred, ref = pred[keep], ref[keep]
            if len(pred) == 0:
                return torch.zeros(1, device=pred.device)
            if self.use_weight:
                weights = weights[keep]
        if self.use_weight:
            return torch.mean(self.criterion(pred, ref) * weights)
        return self.criterion(pred, ref)


class PerAtomEnergyLoss(LossDefinition):
    """loss.py:97-130: (E_pred / N, E_ref / N) per graph."""

    def __init__(self, name='Energy', unit='eV/atom', criterion=None, ref_key=KEY.ENERGY,
                 pred_key=KEY.PRED_TOTAL_ENERGY, weight_key=PER_ATOM_ENERGY, **kwargs):
        super().__init__(name=name, unit=unit, criterion=criterion, ref_key=ref_key,
                         pred_key=pred_key, weight_key=weight_key, vdim=1, **kwargs)

    def _preprocess(self, batch_data, model=None):
        n = batch_data[KEY.NUM_ATOMS]
        return batch_data[self.pred_key] / n, batch_data[self.ref_key] / n


class ForceLoss(LossDefinition):
    """loss.py:133-171."""

    def __init__(self, name='Force', unit='eV/A', criterion=None, ref_key=KEY.FORCE,
                 pred_key=KEY.PRED_FORCE, weight_key=KEY.FORCE, **kwargs):
        super().__init__(name=name, unit=unit, criterion=criterion, ref_key=ref_key,
                         pred_key=pred_key, vdim=3, weight_key=weight_key, **kwargs)

    def _get_data_weight(self, batch_data):
        w = batch_data[DATA_WEIGHT][self.weight_key][batch_data[KEY.BATCH]]
        return torch.repeat_interleave(w, self.vdim)


class StressLoss(LossDefinition):
    """loss.py:174-206: both sides in kbar."""

    TO_KB = 1602.1766208  # eV/A^3 to kbar

    def __init__(self, name='Stress', unit='kbar', criterion=None, ref_key=KEY.STRESS,
                 pred_key=KEY.PRED_STRESS, weight_key=KEY.STRESS, **kwargs):
        super().__init__(name=name, unit=unit, criterion=criterion, ref_key=ref_key,
                         pred_key=pred_key, vdim=6, weight_key=weight_key, **kwargs)

    def _preprocess(self, batch_data, model=None):
        return (torch.reshape(batch_data[self.pred_key] * self.TO_KB, (-1,)),
                torch.reshape(batch_data[self.ref_key] * self.TO_KB, (-1,)))


class EWCLoss(LossDefinition):
    """loss.py:209-252: sum over named parameters of F * (theta - theta*)^2."""

    def __init__(self, fisher_dict, opt_params_dict, name='EWC', device=None, **kwargs):
        super().__init__(criterion=None, name=name, ref_key=None, pred_key=None,
                         weight_key=None, use_weight=False, vdim=0, **kwargs)
        self.fisher_dict, self.opt_params_dict = fisher_dict, opt_params_dict
        self.device = device
        if device is not None:
            self.to(device)

    def to(self, device):
        for d in (self.fisher_dict, self.opt_params_dict):
            for k in d:
                d[k] = d[k].to(device)
        self.device = device

    def _flat_terms(self, model):
        """(fisher, theta*) laid out like ``model.flat`` (zero Fisher where a
        parameter is absent from either dict), built once per model."""
        params = dict(model.named_parameters())
        key = (id(model), model.flat.data_ptr(), tuple(p.requires_grad for p in params.values()))
        if getattr(self, '_flat_key', None) != key:
            f = torch.zeros_like(model.flat)
            o = torch.zeros_like(model.flat)
            trainable = torch.zeros_like(model.flat)
            for name, (off, n, _) in model.slices.items():
                if name in self.fisher_dict and name in self.opt_params_dict:
                    f[off:off + n] = self.fisher_dict[name].reshape(-1).to(f)
                    o[off:off + n] = self.opt_params_dict[name].reshape(-1).to(o)
                trainable[off:off + n] = float(params[name].requires_grad)
            self._flat, self._flat_key = (f, o, f * trainable), key
        return self._flat

    def get_loss(self, batch_data, model=None):
        if model is None:
            raise ValueError('EWC requires model to compute loss')
        if hasattr(model, 'flat') and hasattr(model, 'flat_grad') and model.grads_in_flat_buffer():
            # SevenNetTrainable: every parameter is a view of model.flat and
            # every .grad a view of model.flat_grad -> one fused term
            f, o, f_train = self._flat_terms(model)
            return _FlatEWC.apply(model, f, o, f_train, *model.parameters()).view(1)
        ewc = torch.zeros(1, device=self.device)
        for name, p in model.named_parameters():
            if name not in self.fisher_dict or name not in self.opt_params_dict:
                continue
            ewc = ewc + torch.sum(self.fisher_dict[name] * (p - self.opt_params_dict[name]) ** 2)
        return ewc


def _sum_two_level(v):
    """Sum of a long 1-D tensor as rows of 1024 reduced per block, then the row
    sums: no reduction spans blocks.  A single torch.sum over the 842k-entry
    flat buffer is PyTorch's multi-block global reduction, whose semaphores
    are re-zeroed by a hipMemsetAsync before each launch; captured in a HIP
    graph (the graphed rehearsal step) it returned wrong sums on replays that
    other work ran between (the diagnostic scripts of
    round 3, in git history: the reported EWC loss, never the gradients, which
    _FlatEWC.backward forms element-wise)."""
    m = v.numel() // 1024 * 1024
    s = v[:m].view(-1, 1024).sum(1).sum() if m else v.new_zeros(())
    return s + v[m:].sum() if m < v.numel() else s


class _FlatEWC(torch.autograd.Function):
    """sum F (theta - theta*)^2 over the model's flat parameter buffer in one
    pass; the backward adds 2 F (theta - theta*) straight into the flat
    gradient buffer (trainable slots only) instead of one accumulation per
    parameter tensor -- the same .grad values the per-tensor loop produces."""

    @staticmethod
    def forward(ctx, model, f, o, f_train, *params):
        d = model.flat.detach() - o
        ctx.model, ctx.f_train = model, f_train
        ctx.save_for_backward(d)
        return _sum_two_level(f * d * d)

    @staticmethod
    def backward(ctx, g):
        d, = ctx.saved_tensors
        ctx.model.flat_grad.add_(2.0 * g * ctx.f_train * d)
        return (None,) * (4 + len(ctx.model.slices))


loss_dict = {'mse': torch.nn.MSELoss, 'huber': torch.nn.HuberLoss, 'custom': 'custom'}


def get_loss_functions_from_config(config):
    """loss.py:255-297 -> list of (LossDefinition, weight)."""
    loss = loss_dict[config[LOSS].lower()]
    loss_param = config.get(LOSS_PARAM, {}) or {}
    if loss == 'custom':
        raise NotImplementedError('custom loss callbacks are not part of this build')
    reduction, use_weight = 'mean', False
    if LOAD_DATASET_WITH_WEIGHTS in config:
        reduction, use_weight = 'none', True
    common = {'criterion': loss(reduction=reduction, **loss_param), 'use_weight': use_weight}
    fns = [(PerAtomEnergyLoss(**common), 1.0), (ForceLoss(**common), config[FORCE_WEIGHT])]
    if config[IS_TRAIN_STRESS]:
        fns.append((StressLoss(**common), config[STRESS_WEIGHT]))
    cont = config.get(CONTINUE, {}) or {}
    fpath, opath = cont.get(FISHER, False), cont.get(OPT_PARAMS, False)
    if fpath is not False and opath is not False:
        fisher = fpath if isinstance(fpath, dict) else torch.load(fpath, weights_only=True)
        opt = opath if isinstance(opath, dict) else torch.load(opath, weights_only=True)
        lam = float(cont[EWC_LAMBDA])
        fns.append((EWCLoss(dict(fisher), dict(opt), device=config.get(DEVICE)), lam / 2.0))
    return fns


# ------------------------------------------------------------------ schedulers
def _set_lr(group, lr):
    """in place for a tensor lr (a captured optimizer step reads its memory)"""
    if torch.is_tensor(group['lr']):
        group['lr'].fill_(float(lr))
    else:
        group['lr'] = lr


class CosineAnnealingWarmupRestarts(torch.optim.lr_scheduler.LRScheduler):
    """Restatement of the ``cosine_annealing_warmup`` package's scheduler
    (katsura-jp/pytorch-cosine-annealing-with-warmup, unpinned VCS dependency,
    pyproject.toml:29; used via optim.py:22): linear warmup from min_lr to
    max_lr over ``warmup_steps``, cosine decay to min_lr over the rest of the
    cycle, cycles growing by ``cycle_mult``, max_lr decaying by ``gamma`` per
    cycle.  Pinned by the learning-rate column of the reference's fine-tuning
    log (example_inputs/fine_tuning/FT_w_reEWC/log.sevenn:284-374)."""

    def __init__(self, optimizer, first_cycle_steps, cycle_mult=1.0, max_lr=0.1, min_lr=0.001,
                 warmup_steps=0, gamma=1.0, last_epoch=-1):
        assert warmup_steps < first_cycle_steps
        self.first_cycle_steps = first_cycle_steps
        self.cycle_mult = cycle_mult
        self.base_max_lr = self.max_lr = max_lr
        self.min_lr = min_lr
        self.warmup_steps = warmup_steps
        self.gamma = gamma
        self.cur_cycle_steps = first_cycle_steps
        self.cycle = 0
        self.step_in_cycle = last_epoch
        super().__init__(optimizer, last_epoch)
        self.base_lrs = []
        for g in self.optimizer.param_groups:
            _set_lr(g, self.min_lr)
            self.base_lrs.append(self.min_lr)

    def get_lr(self):
        if self.step_in_cycle == -1:
            return self.base_lrs
        if self.step_in_cycle < self.warmup_steps:
            return [(self.max_lr - b) * self.step_in_cycle / self.warmup_steps + b
                    for b in self.base_lrs]
        span = self.cur_cycle_steps - self.warmup_steps
        return [b + (self.max_lr - b) * (1 + math.cos(
            math.pi * (self.step_in_cycle - self.warmup_steps) / span)) / 2
            for b in self.base_lrs]

    def step(self, epoch=None):
        if epoch is None:
            epoch = self.last_epoch + 1
            self.step_in_cycle += 1
            if self.step_in_cycle >= self.cur_cycle_steps:
                self.cycle += 1
                self.step_in_cycle -= self.cur_cycle_steps
                self.cur_cycle_steps = int((self.cur_cycle_steps - self.warmup_steps)
                                           * self.cycle_mult) + self.warmup_steps
        else:
            if epoch >= self.first_cycle_steps:
                if self.cycle_mult == 1.0:
                    self.step_in_cycle = epoch % self.first_cycle_steps
                    self.cycle = epoch // self.first_cycle_steps
                else:
                    n = int(math.log(epoch / self.first_cycle_steps * (self.cycle_mult - 1) + 1,
                                     self.cycle_mult))
                    self.cycle = n
                    self.step_in_cycle = epoch - int(self.first_cycle_steps
                                                     * (self.cycle_mult ** n - 1)
                                                     / (self.cycle_mult - 1))
                    self.cur_cycle_steps = self.first_cycle_steps * self.cycle_mult ** n
            else:
                self.cur_cycle_steps = self.first_cycle_steps
                self.step_in_cycle = epoch
        self.max_lr = self.base_max_lr * (self.gamma ** self.cycle)
        self.last_epoch = math.floor(epoch)
        for g, lr in zip(self.optimizer.param_groups, self.get_lr()):
            _set_lr(g, lr)


_S = torch.optim.lr_scheduler
optim_dict = {'sgd': torch.optim.SGD, 'adagrad': torch.optim.Adagrad, 'adam': torch.optim.Adam,
              'adamw': torch.optim.AdamW, 'radam': torch.optim.RAdam}
scheduler_dict = {'steplr': _S.StepLR, 'multisteplr': _S.MultiStepLR,
                  'exponentiallr': _S.ExponentialLR, 'cosineannealinglr': _S.CosineAnnealingLR,
                  'reducelronplateau': _S.ReduceLROnPlateau, 'linearlr': _S.LinearLR,
                  'cosineannealingwarmuplr': CosineAnnealingWarmupRestarts}


# ------------------------------------------------------------------ batching
def _float(a):
    """float tensor, keeping float64 inputs float64 (the model casts to its own dtype)"""
    t = torch.as_tensor(a)
    return t if t.is_floating_point() else t.to(torch.float32)


_PER_GRAPH = (KEY.ENERGY, KEY.STRESS, KEY.CELL_VOLUME, KEY.NUM_ATOMS)


def labeled_graph(pos, cell, types, cutoff, energy=None, force=None, stress=None):
    """AtomGraphData dict of one labelled structure, as
    sevenn/train/dataload.py:71-140 builds it: reference edge convention
    (util.unlabeled_atoms_to_graph), ``x`` = type index, labels ``total_energy``
    (eV), ``force_of_atoms`` [N,3] and ``stress`` [1,6] in the model's output
    convention (xx,yy,zz,xy,yz,zx, i.e. -ASE stress reordered, dataload.py:104-105);
    a missing label is NaN, which the losses drop (loss.py:70-80)."""
    from .neighbor import neighbor_list
    pos = np.asarray(pos, dtype=np.float64)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    ei, sh = neighbor_list(pos, cell, cutoff)
    vec = pos[ei[1]] + sh @ cell - pos[ei[0]]
    n = len(pos)
    return {
        KEY.NODE_FEATURE: torch.as_tensor(np.asarray(types), dtype=torch.long),
        KEY.POS: torch.as_tensor(pos),
        KEY.EDGE_IDX: torch.as_tensor(ei, dtype=torch.long),
        KEY.EDGE_VEC: torch.as_tensor(vec),
        KEY.CELL_SHIFT: torch.as_tensor(sh),
        KEY.CELL_VOLUME: torch.tensor(abs(float(np.linalg.det(cell)))),
        KEY.NUM_ATOMS: torch.tensor(n),
        KEY.ENERGY: torch.tensor(float('nan') if energy is None else float(energy)),
        KEY.FORCE: torch.as_tensor(np.full((n, 3), np.nan) if force is None
                                   else np.asarray(force, dtype=np.float64)),
        KEY.STRESS: torch.as_tensor(np.full((1, 6), np.nan) if stress is None
                                    else np.asarray(stress, dtype=np.float64).reshape(1, 6)),
    }


def collate(graphs, device=None, dtype=None):
    """PyG ``Collater`` over AtomGraphData dicts: node rows concatenated,
    ``edge_index`` offset by the running atom count, a ``batch`` vector,
    per-graph scalars/rows stacked (``num_atoms`` [B], ``cell_volume`` [B],
    ``total_energy`` [B], ``stress`` [B,6]); floating tensors cast to
    ``dtype`` when given (the model's)."""
    nodes, edges, pg = {}, {}, {k: [] for k in _PER_GRAPH}
    batch, off = [], 0
    for b, g in enumerate(graphs):
        n = int(torch.as_tensor(g[KEY.NODE_FEATURE]).shape[0])
        for k in (KEY.NODE_FEATURE, KEY.FORCE, KEY.POS):
            if k in g:
                nodes.setdefault(k, []).append(torch.as_tensor(g[k]))
        edges.setdefault(KEY.EDGE_IDX, []).append(torch.as_tensor(g[KEY.EDGE_IDX]).long() + off)
        for k in (KEY.EDGE_VEC, KEY.CELL_SHIFT):
            if k in g:
                edges.setdefault(k, []).append(_float(g[k]))
        for k in _PER_GRAPH:
            if k in g:
                pg[k].append(_float(g[k]).reshape(1, -1))
        batch.append(torch.full((n,), b, dtype=torch.long))
        off += n
    out = {k: torch.cat(v, 0) for k, v in nodes.items()}
    out[KEY.NODE_FEATURE] = out[KEY.NODE_FEATURE].long()
    if KEY.FORCE in out:
        out[KEY.FORCE] = _float(out[KEY.FORCE])
    out[KEY.EDGE_IDX] = torch.cat(edges[KEY.EDGE_IDX], 1)
    for k in (KEY.EDGE_VEC, KEY.CELL_SHIFT):
        if k in edges:
            out[k] = torch.cat(edges[k], 0)
    # edges stably sorted by centre here, on the host (the neighbour lists
    # already are: a no-op permutation then), so the captured step needs no
    # device sort (GraphedStep._centre_sorted)
    cen = out[KEY.EDGE_IDX][0].numpy()
    if cen.size > 1 and (cen[1:] < cen[:-1]).any():
        perm = torch.from_numpy(np.argsort(cen, kind='stable'))
        out[KEY.EDGE_IDX] = out[KEY.EDGE_IDX][:, perm]
        for k in (KEY.EDGE_VEC, KEY.CELL_SHIFT):
            if k in out:
                out[k] = out[k][perm]
    for k, v in pg.items():
        if v:
            t = torch.cat(v, 0)
            out[k] = t if k == KEY.STRESS else t.view(-1)
    out[KEY.NUM_ATOMS] = out[KEY.NUM_ATOMS].long()
    out[KEY.BATCH] = torch.cat(batch)
    if dtype is not None:
        out = {k: v.to(dtype) if v.is_floating_point() else v for k, v in out.items()}
    if device is not None:
        out = {k: v.to(device, non_blocking=True) for k, v in out.items()}
    mark_edges_sorted(out)
    return out


def mark_edges_sorted(b):
    """Record that b's edge_index is CSR-sorted by centre: the flag (a host
    tensor) names the edge_index storage and its version counter, so
    replacing or editing the edges afterwards makes it stale by itself"""
    ei = b[KEY.EDGE_IDX]
    b[KEY.EDGE_SORTED] = torch.tensor([ei.data_ptr(), ei._version], dtype=torch.int64)


def edges_marked_sorted(b):
    """True only when b's EDGE_SORTED flag still describes its edge_index
    (a stale flag -- edges reordered or modified after collate -- is ignored
    and the callers sort as for an unflagged batch)"""
    f, ei = b.get(KEY.EDGE_SORTED), b.get(KEY.EDGE_IDX)
    if f is None or ei is None or not torch.is_tensor(f) or f.numel() != 2 or f.is_cuda:
        return False
    return int(f[0]) == ei.data_ptr() and int(f[1]) == ei._version


# ------------------------------------------------------------------ trainer
class Trainer:
    """trainer.py:15-152 over a SevenNetTrainable (flat parameter/grad
    buffers).  ``config`` uses the reference's keys."""

    def __init__(self, model, config):
        self.distributed = bool(config.get(IS_DDP, False))
        self.model = model
        self.model.set_is_batch_data(True)
        self.device = model.flat.device
        if self.distributed:
            import torch.distributed as dist
            self.world = dist.get_world_size()
            dist.barrier()
            # every rank starts from rank 0's parameters (DDP's broadcast)
            dist.broadcast(self.model.flat, 0)
        else:
            self.world = 1
        # BLAS (this build): the radial-MLP GEMMs of the step (12k x 64 x 960
        # and transposes) run 1.4x faster per step on rocBLAS than on torch's
        # default hipBLASLt on MI355X (bench_train: 29.1 -> 21.1 ms); fp32 either
        # way.  Process-wide torch setting, applied when the model is on a GPU.
        blas = str(config.get(BLAS, 'rocblas')).lower()
        if self.device.type == 'cuda' and blas in ('rocblas', 'hipblaslt'):
            torch.backends.cuda.preferred_blas_library('cublas' if blas == 'rocblas'
                                                       else 'cublaslt')
        params = [p for p in self.model.parameters() if p.requires_grad]
        opt = optim_dict[config[OPTIMIZER].lower()]
        optim_param = dict(config.get(OPTIM_PARAM, {}))
        # HIP_GRAPH (this build): replay the rehearsal step as captured HIP
        # graphs per batch-shape signature (one graph in a single process; three
        # segments around the two gradient all-reduces with is_ddp); the
        # optimizer then keeps its step count and lr on the device
        self.hip_graph = bool(config.get(HIP_GRAPH, False))
        if self.hip_graph:
            if config[OPTIMIZER].lower() not in ('adam', 'adamw'):
                raise ValueError('hip_graph supports the adam/adamw optimizers')
            optim_param['capturable'] = True
            optim_param['lr'] = torch.tensor(float(optim_param.get('lr', 1e-3)),
                                             device=self.device)
        # Adam / AdamW on the GPU: torch's fused kernel (one multi-tensor launch
        # per update; the default foreach form issued ~70 launches per update,
        # 1/3 of the fine-tune step's element-wise kernels).  Same update rule;
        # 'optim_fused': False keeps the foreach form.
        if (self.device.type == 'cuda' and config[OPTIMIZER].lower() in ('adam', 'adamw')
                and bool(config.get('optim_fused', True))
                and 'foreach' not in optim_param and 'fused' not in optim_param):
            optim_param['fused'] = True
        self.optimizer = opt(params, **optim_param)
        sch = scheduler_dict[config[SCHEDULER].lower()]
        self.scheduler = sch(self.optimizer, **config.get(SCHEDULER_PARAM, {}))
        self.loss_functions = get_loss_functions_from_config(config)
        for loss_def, _ in self.loss_functions:
            if isinstance(loss_def, EWCLoss) and loss_def.device is None:
                loss_def.to(self.device)
            if isinstance(loss_def, EWCLoss) and hasattr(self.model, 'flat'):
                # the flat (F, theta*) terms now, on this stream: never inside a
                # graphed step's side-stream warm-up or capture
                loss_def._flat_terms(self.model)
            loss_def.static = self.hip_graph
        self.explicit = None
        if bool(config.get(EXPLICIT_GRAD, True)) and hasattr(self.model, 'blocks'):
            from . import train_explicit
            if train_explicit.supported(self.model):
                self.explicit = train_explicit.ExplicitStep(self.model)
        self._graphed = GraphedRehearsalStep(self, config.get('hip_graph_max', 16)) \
            if self.hip_graph else None
        # (None: the loss by autograd over its torch expression)
        self._fused_loss = self._fused_loss_plan() if self.explicit is not None else None
        self._served = None   # validate()'s E3GNNModel of this model, made on first use

    # ---- the pieces of one step
    def zero_grad(self):
        self.model.zero_grad()

    def total_loss(self, output):
        total = torch.zeros(1, device=self.device)
        for loss_def, w in self.loss_functions:
            total = total + loss_def.get_loss(output, self.model) * w
        return total

    def backward(self, loss):
        loss.backward()
        if self.distributed:
            self.all_reduce_grad()

    def loss_backward(self, batch, graph=None, reduce=True):
        """Forward, loss, and its parameter gradient accumulated into the
        model's gradient buffer (+ the data-parallel average when ``reduce``):
        loss.backward() through the model's autograd graph, or the explicit
        derivatives (train_explicit.py) -- the loss itself is the same
        autograd expression on (E, F, S) either way."""
        if self.explicit is None:
            output = self.model(batch, graph=graph)
            loss = self.total_loss(output)
            loss.backward()
        elif self._fused_loss is not None:
            output = self.explicit.forward(batch, graph)
            loss = self._fused_loss_backward(output, batch)
        else:
            output = self.explicit.forward(batch, graph)
            loss = self.total_loss(output)
            loss.backward()          # cotangents of E, F, S (+ the flat EWC term)
            S = output.get(KEY.PRED_STRESS)
            self.explicit.backward(output[KEY.PRED_TOTAL_ENERGY].grad, output[KEY.PRED_FORCE].grad,
                                   S.grad if S is not None else None)
        if reduce and self.distributed:
            self.all_reduce_grad()
        return loss, output

    def _fused_loss_plan(self):
        """The loss terms the library computes in one launch with their
        cotangents (e3gnn_loss_efs: MSE / Huber, mean over labelled entries of
        the energy-per-atom, force and stress terms) and the flat EWC term
        (e3gnn_ewc_flat), or None when the configuration needs autograd
        (weighted data, another criterion, non-standard keys, CPU / float64)."""
        if self.device.type != 'cuda' or self.model.dtype != torch.float32:
            return None
        plan = {'w': [0.0, 0.0, 0.0], 'stress': False, 'ewc': None, 'crit': None}
        std = {PerAtomEnergyLoss: (0, KEY.PRED_TOTAL_ENERGY, KEY.ENERGY),
               ForceLoss: (1, KEY.PRED_FORCE, KEY.FORCE),
               StressLoss: (2, KEY.PRED_STRESS, KEY.STRESS)}
        for f, w in self.loss_functions:
            if isinstance(f, EWCLoss):
                if plan['ewc'] is not None:
                    return None
                plan['ewc'] = (f, float(w))
                continue
            if type(f) not in std or f.use_weight or not f.delete_unlabeled:
                return None
            term, pk, rk = std[type(f)]
            if (f.pred_key, f.ref_key) != (pk, rk) or plan['w'][term]:
                return None
            c = f.criterion
            if isinstance(c, torch.nn.HuberLoss) and c.reduction == 'mean':
                crit = (1, float(c.delta))
            elif isinstance(c, torch.nn.MSELoss) and c.reduction == 'mean':
                crit = (0, 0.0)
            else:
                return None
            if plan['crit'] not in (None, crit):
                return None
            plan['crit'] = crit
            plan['w'][term] = float(w)
            plan['stress'] |= term == 2
        if plan['crit'] is None or not plan['w'][0] or not plan['w'][1]:
            return None
        from . import _lib
        plan['lib'] = _lib.load()
        plan['terms'] = torch.zeros(3, device=self.device)
        plan['ewc_val'] = torch.zeros(1, device=self.device)
        n = self.model.flat.numel()
        plan['part'] = torch.empty(n + n // 256 + 2, device=self.device)
        return plan

    def _fused_loss_backward(self, output, batch):
        """loss + cotangents in one launch (+ EWC value and its gradient into
        the flat gradient buffer), then the explicit step's reverse sweep"""
        from . import _lib
        P, lib = self._fused_loss, self._fused_loss['lib']
        st = torch.cuda.current_stream(self.device).cuda_stream
        E, F = output[KEY.PRED_TOTAL_ENERGY].detach(), output[KEY.PRED_FORCE].detach()
        S = output.get(KEY.PRED_STRESS) if P['stress'] else None
        if P['stress'] and S is None:   # the autograd path's KeyError, not a silent zero term
            raise KeyError(f'stress loss configured but the output has no {KEY.PRED_STRESS}')
        S = S.detach().contiguous() if S is not None else None
        nb, n = int(E.numel()), int(F.shape[0])
        ref = lambda k, like: batch[k].to(like.device, like.dtype).contiguous()   # noqa: E731
        cE, cF = torch.empty_like(E), torch.empty_like(F)
        cS = torch.empty_like(S) if S is not None else None
        natoms = batch[KEY.NUM_ATOMS].to(E.device, torch.long).contiguous()
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        _lib.check(lib.e3gnn_loss_efs(
            P['crit'][0], P['crit'][1], nb, n, p(E), p(ref(KEY.ENERGY, E)), p(natoms), p(F),
            p(ref(KEY.FORCE, F)), p(S), p(ref(KEY.STRESS, S)) if S is not None else None,
            P['w'][0], P['w'][1], P['w'][2], StressLoss.TO_KB, p(P['terms']), p(cE), p(cF),
            p(cS), st))
        loss = P['terms'].sum().view(1)
        if P['ewc'] is not None:
            f_def, w = P['ewc']
            f, o, f_train = f_def._flat_terms(self.model)
            m = self.model
            _lib.check(lib.e3gnn_ewc_flat(m.flat.numel(), p(m.flat), p(f), p(o), p(f_train),
                                          2.0 * w, p(m.flat_grad), p(P['part']), p(P['ewc_val']), st))
            loss = loss + w * P['ewc_val']
        self.explicit.backward(cE, cF, cS)
        return loss

    def all_reduce_grad(self):
        """DDP's gradient average (one all-reduce of the flat gradient buffer)."""
        import torch.distributed as dist
        g = self.model.flat_grad
        dist.all_reduce(g)
        g.div_(self.world)

    def _record(self, recorder, output, batch, fresh=False):
        """One forward's (output, batch) into ``recorder`` (error_recorder.py):
        one launch on the current stream, no synchronisation.  ``fresh``: the
        call follows this forward's loss_backward, whose EWC term is still in
        place; otherwise a recorder with an EWCLoss row has it computed."""
        if recorder is None:
            return
        ewc = None
        if recorder.wants_ewc:
            for f, w in self.loss_functions:
                if not isinstance(f, EWCLoss):
                    continue
                if fresh and self._fused_loss is not None and self._fused_loss['ewc'] is not None:
                    ewc = self._fused_loss['ewc_val'] * w
                else:
                    with torch.no_grad():
                        ewc = f.get_loss(output, self.model) * w
        recorder.update(output, batch, ewc=ewc)

    def train_step(self, batch, error_recorder=None):
        """One optimizer step of Trainer.run_one_epoch (trainer.py:55-68)."""
        self.zero_grad()
        loss, output = self.loss_backward(batch)
        self._record(error_recorder, output, batch, fresh=True)
        self.optimizer.step()
        return loss.detach(), output

    def rehearsal_step(self, batch, batch_mem, error_recorder=None, mem_recorder=None):
        """One iteration of RehearsalTrainer.run_one_epoch_rehearsal
        (trainer.py:174-206): zero_grad once, backward+step on the new batch,
        then backward (accumulating) + step on the memory batch; each forward
        recorded right after its backward (``error_recorder`` the new batch,
        ``mem_recorder`` the memory batch)."""
        recorders = (error_recorder, mem_recorder)
        if self._graphed is not None:
            return self._graphed(batch, batch_mem, recorders)
        return self._rehearsal_body(batch, batch_mem, recorders=recorders)

    def _rehearsal_body(self, batch, batch_mem, graphs=(None, None), recorders=(None, None)):
        self.zero_grad()
        loss, out = self.loss_backward(batch, graphs[0])
        self._record(recorders[0], out, batch, fresh=True)
        self.optimizer.step()
        mem_loss, out = self.loss_backward(batch_mem, graphs[1])
        self._record(recorders[1], out, batch_mem, fresh=True)
        self.optimizer.step()
        return loss.detach(), mem_loss.detach()

    def _to_device(self, batch, non_blocking=False):
        """The batch on the trainer's device with its EDGE_SORTED flag still
        valid: the flag (a host tensor naming the edge_index storage) stays on
        the host, and a move that copied edge_index re-marks the copy.  Host
        checks only: no device sort later, no synchronisation here."""
        was_sorted = edges_marked_sorted(batch)
        out = {k: v if k == KEY.EDGE_SORTED else v.to(self.device, non_blocking=non_blocking)
               for k, v in batch.items()}
        if was_sorted and out[KEY.EDGE_IDX] is not batch[KEY.EDGE_IDX]:
            mark_edges_sorted(out)
        return out

    def run_one_epoch(self, loader, is_train=False, error_recorder=None):
        self.model.train(is_train)
        losses = []
        for batch in loader:
            batch = self._to_device(batch, non_blocking=True)
            if is_train:
                losses.append(self.train_step(batch, error_recorder)[0])
            else:
                output = self.model(batch)
                losses.append(self.total_loss(output).detach())
                self._record(error_recorder, output, batch)
        if error_recorder is not None and self.distributed:
            error_recorder.reduce()
        return losses

    def _served_output(self, batch, want_stress):
        """The served engine's predictions of one (padded or plain) batch as
        the trainable's output keys.  No padded edge touches a real atom and
        the recorder never reads a dummy slot's prediction, so DeviceLoader
        batches go in as they are; ``atom_ptr`` is a device prefix sum."""
        batch = GraphedRehearsalStep._centre_sorted(batch)
        ei = batch[KEY.EDGE_IDX]
        na = batch[KEY.NUM_ATOMS].view(-1)
        atom_ptr = torch.zeros(na.numel() + 1, dtype=torch.int32, device=self.device)
        atom_ptr[1:] = torch.cumsum(na, 0)
        res = self._served.energy_forces_batch(batch[KEY.NODE_FEATURE], ei[0], ei[1],
                                               batch[KEY.EDGE_VEC], atom_ptr, want_virial=want_stress)
        out = {KEY.PRED_TOTAL_ENERGY: res['energy'], KEY.PRED_FORCE: res['forces'],
               KEY.ATOMIC_ENERGY: res['atomic_energy'].unsqueeze(-1)}
        if want_stress:
            # virial6 = -dE/dstrain = inferred_stress * volume, the same order
            # (xx, yy, zz, xy, yz, zx) and sign as the trainable's inferred_stress
            vol = batch[KEY.CELL_VOLUME].to(self.device, torch.float32).view(-1, 1)
            out[KEY.PRED_STRESS] = res['virial'] / vol
        return out

    def validate(self, loader, error_recorder):
        """The validation pass on the served kernels: the trainer's own
        ``E3GNNModel`` of this model (``from_trainable`` on first use) takes the
        current parameters in place (``set_weights``, once per call), evaluates
        every batch by ``energy_forces_batch`` and records it.  For a model the
        explicit step supports, on a GPU in float32; any other model takes
        ``run_one_epoch(loader, False, error_recorder)``.  Returns the recorder."""
        from . import train_explicit
        m = self.model
        served = (self.device.type == 'cuda' and getattr(m, 'dtype', None) == torch.float32
                  and hasattr(m, 'blocks') and train_explicit.supported(m))
        if served and self._served is None:
            from .model import E3GNNModel
            self._served = E3GNNModel.from_trainable(m)
        if not served or self._served.family < 0:
            self.run_one_epoch(loader, False, error_recorder)
            return error_recorder
        self._served.set_weights(m.flat)
        for batch in loader:
            batch = self._to_device(batch, non_blocking=True)
            self._record(error_recorder, self._served_output(batch, error_recorder.stress), batch)
        if self.distributed:
            error_recorder.reduce()
        return error_recorder

    def run_one_epoch_rehearsal(self, loader, memloader, is_train=False, error_recorder=None,
                                mem_recorder=None):
        self.model.train(is_train)
        mem_iter = iter(memloader)
        out = []
        for batch in loader:
            try:
                batch_mem = next(mem_iter)
            except StopIteration:
                mem_iter = iter(memloader)
                batch_mem = next(mem_iter)
            batch = self._to_device(batch)
            batch_mem = self._to_device(batch_mem)
            if is_train:
                if error_recorder is None and mem_recorder is None:
                    out.append(self.rehearsal_step(batch, batch_mem))
                else:
                    out.append(self.rehearsal_step(batch, batch_mem, error_recorder, mem_recorder))
            else:
                o, om = self.model(batch), self.model(batch_mem)
                out.append((self.total_loss(o).detach(), self.total_loss(om).detach()))
                self._record(error_recorder, o, batch)
                self._record(mem_recorder, om, batch_mem)
        if self.distributed:
            for rec in (error_recorder, mem_recorder):
                if rec is not None:
                    rec.reduce()
        return out

    def scheduler_step(self, metric=None):
        if self.scheduler is None:
            return
        if isinstance(self.scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
            self.scheduler.step(metric)
        else:
            self.scheduler.step()

    def get_lr(self):
        return self.optimizer.param_groups[0]['lr']

    def compute_fisher_matrix(self, loader, loss_thr):
        """trainer.py:124-152: mean over batches (below loss_thr, if >= 0) of
        squared loss gradients, and the current parameters."""
        fisher = {n: torch.zeros_like(p) for n, p in self.model.named_parameters()}
        self.model.train()
        cnt = 0
        for batch in loader:
            self.zero_grad()
            batch = self._to_device(batch)
            total = self.total_loss(self.model(batch))
            if loss_thr < 0 or total < loss_thr:
                self.backward(total)
                for n, p in self.model.named_parameters():
                    if p.grad is not None and p.requires_grad:
                        fisher[n] += p.grad.detach().clone() ** 2
                cnt += 1
        for n in fisher:
            fisher[n] /= cnt
        opt = {n: p.data.detach().clone() for n, p in self.model.named_parameters()}
        return fisher, opt, cnt


class GraphedRehearsalStep:
    """The rehearsal step as ONE captured HIP graph per batch-shape signature
    (launch-bound at the reference's batch sizes: ~8k kernels per step).  With
    is_ddp the step is three graphs sharing one memory pool -- [new batch
    forward + backward], [optimizer step, memory batch forward + backward],
    [optimizer step] -- replayed around the two eager gradient all-reduces
    (trainer.py:174-206 with DDP's averaging), so any backend works and every
    rank issues the same collectives whether its step is graphed or not.

    Per call: the batch tensors are copied into the graph's static inputs, the
    two edge CSRs are rebuilt in place (e3gnn_conv_graph, which also validates
    the graph), and the graph is replayed.  A new signature is captured after
    two eager warm-up steps on a side stream; the warm-ups' parameter and
    optimizer updates are rolled back, so the trajectory equals the eager
    step's.  Everything inside is device-side: the model takes the prebuilt
    ConvGraphs, the losses run in static mode, the optimizer is capturable."""

    def __init__(self, trainer, max_graphs=16):
        self.tr = trainer
        self.cache = {}
        # each captured shape keeps its own memory pool: beyond max_graphs
        # distinct shapes (variable-size datasets) new shapes run eagerly
        self.max_graphs = int(max_graphs)
        # steps by path (captured: those that captured a new signature, which
        # also replay it) and device argsorts of batches not marked sorted
        self.stats = {'captured': 0, 'replayed': 0, 'eager': 0, 'device_sorts': 0}

    @staticmethod
    def _sig(b):
        return tuple((k, tuple(v.shape), str(v.dtype)) for k, v in sorted(b.items())
                     if torch.is_tensor(v))

    def _graph_of(self, b):
        from . import conv_ops
        ei = b[KEY.EDGE_IDX]
        n = int(b[KEY.NODE_FEATURE].shape[0])
        return conv_ops.ConvGraph(n, ei[0], ei[1], self.tr.model.conv_backend)

    def _state(self):
        opt = self.tr.optimizer
        st = {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()}
              for p, s in opt.state.items()}
        return self.tr.model.flat.detach().clone(), st

    def _restore(self, snap):
        flat, st = snap
        with torch.no_grad():
            self.tr.model.flat.copy_(flat)
        for p, s in self.tr.optimizer.state.items():
            for k, v in st.get(id(p), {}).items():
                if torch.is_tensor(s.get(k)):
                    s[k].copy_(v)

    def _capture(self, batch, mem, recorders=(None, None)):
        tr = self.tr
        sb = {k: v.clone() for k, v in batch.items()}
        sm = {k: v.clone() for k, v in mem.items()}
        graphs = (self._graph_of(sb), self._graph_of(sm))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        # warm-ups are local (no collectives: the other ranks may not be
        # capturing at this step) and rolled back
        # (restored even if a warm-up raises: a rank left non-distributed
        # would skip its all-reduces while its peers issue theirs)
        dist_flag, tr.distributed = tr.distributed, False
        try:
            with torch.cuda.stream(side):
                # the warm-ups record like the captured step (the same launches)
                # and are rolled back out of the sums like out of the parameters
                rec_snaps = [r.snapshot() if r is not None else None for r in recorders]
                first = not tr.optimizer.state
                if first:   # create the optimizer state, then undo the update
                    snap0 = tr.model.flat.detach().clone()
                    tr._rehearsal_body(sb, sm, graphs, recorders)
                    with torch.no_grad():
                        tr.model.flat.copy_(snap0)
                    for s in tr.optimizer.state.values():
                        for v in s.values():
                            if torch.is_tensor(v):
                                v.zero_()
                snap = self._state()
                for _ in range(2):
                    tr._rehearsal_body(sb, sm, graphs, recorders)
                self._restore(snap)
                for r, rs in zip(recorders, rec_snaps):
                    if r is not None:
                        r.restore(rs)
        finally:
            tr.distributed = dist_flag
        torch.cuda.current_stream().wait_stream(side)
        if not tr.distributed:
            g = torch.cuda.CUDAGraph()
            with _capturing(g):
                loss, mloss = tr._rehearsal_body(sb, sm, graphs, recorders)
            return {'g': [g], 'b': sb, 'm': sm, 'graphs': graphs, 'out': (loss, mloss)}
        segs = [torch.cuda.CUDAGraph() for _ in range(3)]
        with _capturing(segs[0]):
            tr.zero_grad()
            loss, out = tr.loss_backward(sb, graphs[0], reduce=False)
            tr._record(recorders[0], out, sb, fresh=True)
        pool = segs[0].pool()
        with _capturing(segs[1], pool=pool):
            tr.optimizer.step()
            mloss, out = tr.loss_backward(sm, graphs[1], reduce=False)
            tr._record(recorders[1], out, sm, fresh=True)
        with _capturing(segs[2], pool=pool):
            tr.optimizer.step()
        return {'g': segs, 'b': sb, 'm': sm, 'graphs': graphs,
                'out': (loss.detach(), mloss.detach())}

    @staticmethod
    def _centre_sorted(b):
        """The captured model takes a prebuilt ConvGraph, i.e. edges CSR-sorted
        by centre (the eager model sorts them itself).  Batches from collate()
        are sorted on the host already (EDGE_SORTED); anything else gets a
        stable device argsort of the per-edge entries, no host sync."""
        ei = b.get(KEY.EDGE_IDX)
        if ei is None or ei.shape[1] < 2 or edges_marked_sorted(b):   # (collate sorted it)
            return b
        perm = torch.argsort(ei[0], stable=True)
        out = dict(b)
        out[KEY.EDGE_IDX] = ei[:, perm]
        for k in (KEY.EDGE_VEC, KEY.CELL_SHIFT):
            if k in b and torch.is_tensor(b[k]):
                out[k] = b[k][perm]
        return out

    def __call__(self, batch, mem, recorders=(None, None)):
        given = (batch, mem)
        batch, mem = self._centre_sorted(batch), self._centre_sorted(mem)
        self.stats['device_sorts'] += (batch is not given[0]) + (mem is not given[1])
        # a captured graph records into the sums buffers it was captured with:
        # their identity is part of the key, so attaching, detaching or
        # swapping recorders captures anew instead of replaying a graph that
        # writes elsewhere or nowhere
        rec_key = tuple(r.buffer(self.tr.device).data_ptr() if r is not None else None
                        for r in recorders)
        key = (self._sig(batch), self._sig(mem)) if rec_key == (None, None) else \
            (self._sig(batch), self._sig(mem), rec_key)
        ent = self.cache.get(key)
        if ent is None:
            if len(self.cache) >= self.max_graphs:
                self.stats['eager'] += 1
                return self.tr._rehearsal_body(batch, mem, recorders=recorders)
            ent = self.cache[key] = self._capture(batch, mem, recorders)
            ent['recorders'] = recorders   # (their buffers stay alive with the graph)
            self.stats['captured'] += 1
        else:
            self.stats['replayed'] += 1
        # the batch tensors into the graph's static inputs: one multi-tensor
        # copy per dtype (a copy launch per tensor was ~26 launches a step)
        groups = {}
        for dst, src in ((ent['b'], batch), (ent['m'], mem)):
            for k, v in src.items():
                if torch.is_tensor(v):
                    if v.device != dst[k].device or v.dtype != dst[k].dtype or not v.is_contiguous():
                        dst[k].copy_(v, non_blocking=True)
                    elif v.numel():
                        g = groups.setdefault(v.dtype, ([], []))
                        g[0].append(dst[k].view(-1))
                        g[1].append(v.view(-1))
        for dsts, srcs in groups.values():
            torch._foreach_copy_(dsts, srcs, non_blocking=True)
        for gr, b in zip(ent['graphs'], (ent['b'], ent['m'])):
            gr.rebuild(b[KEY.EDGE_IDX][0], b[KEY.EDGE_IDX][1])
        for i, g in enumerate(ent['g']):
            if i:   # between the segments of a multi-rank step
                self.tr.all_reduce_grad()
            g.replay()
        return ent['out'][0].detach().clone(), ent['out'][1].detach().clone()


def setup_distributed(backend=None):
    """One process per GPU from torchrun's env (RANK/LOCAL_RANK/WORLD_SIZE/
    MASTER_*); backend "nccl" (RCCL) on GPUs, "gloo" otherwise.

    The rank's device is bound BEFORE the process group exists (as the
    reference's entry point does, sevenn/main/sevenn.py:39-49 with
    torch.cuda.set_device(local_rank) ahead of init_process_group): RCCL takes
    its device from the current one, so without it every rank of a node would
    drive cuda:0.  Returns (rank, world_size, local_rank, device); build the
    model on that device."""
    import torch.distributed as dist
    local = int(os.environ.get('LOCAL_RANK', 0))
    gpu = torch.cuda.is_available()
    device = torch.device('cuda', local) if gpu else torch.device('cpu')
    if gpu:
        if local >= torch.cuda.device_count():
            raise RuntimeError(f'LOCAL_RANK={local} but only {torch.cuda.device_count()} '
                               'GPU(s) are visible: one process per GPU')
        torch.cuda.set_device(device)
    if not dist.is_initialized():
        if backend is None:
            backend = 'nccl' if gpu else 'gloo'
        kw = {'device_id': device} if (gpu and backend == 'nccl') else {}
        dist.init_process_group(backend, **kw)
    return dist.get_rank(), dist.get_world_size(), local, device


# ------------------------------------------------------------------ epoch loop
def csv_header(recorder):
    """The reference's log.csv header of a recorder's metrics
    (processing_epoch_with_rehearsal.py:29-35)."""
    from .error_recorder import csv_header as header
    return header(recorder)


def rehearsal_epochs(trainer, train_loader, mem_loader, valid_loader, config, epochs, start_epoch=0):
    """The epoch loop of processing_epoch_with_rehearsal.py:47-97 without its
    files (checkpoints and logs stay with the caller): per epoch a rehearsal
    pass over (train_loader, mem_loader) with the train and memory recorders,
    ``validate`` on valid_loader, ``scheduler_step(val)`` with ``val`` the first
    validation metric whose key contains ``config['best_metric']``.  Yields
    one row dict per epoch: ``Epoch``, ``Learning_rate`` (the epoch's), then
    ``Train_k``, ``Valid_k``, ``Memory_k`` per metric key k (``csv_header``)."""
    from .error_recorder import ErrorRecorder
    train_rec, valid_rec, mem_rec = (ErrorRecorder.from_config(config) for _ in range(3))
    best_metric = config[KEY.BEST_METRIC]
    for epoch in range(start_epoch, start_epoch + epochs):
        lr = float(trainer.get_lr())
        trainer.run_one_epoch_rehearsal(train_loader, mem_loader, is_train=True,
                                        error_recorder=train_rec, mem_recorder=mem_rec)
        train_err, memory_err = train_rec.epoch_forward(), mem_rec.epoch_forward()
        trainer.validate(valid_loader, valid_rec)
        valid_err = valid_rec.epoch_forward()
        row = {'Epoch': epoch, 'Learning_rate': lr}
        for k in train_err:
            row[f'Train_{k}'], row[f'Valid_{k}'], row[f'Memory_{k}'] = \
                train_err[k], valid_err[k], memory_err[k]
        val = next((valid_err[k] for k in valid_err if best_metric in k), None)
        if val is None:
            raise KeyError(f'best_metric {best_metric!r} matches no recorded metric: '
                           f'{", ".join(valid_err)}')
        trainer.scheduler_step(val)
        yield row
