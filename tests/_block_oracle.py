"""One interaction block of ``oracle/nequip_ref.NequIPRef`` in fp64 on a
caller-given edge list, its VJP for a caller-given cotangent, and the
per-irreps-entry error metric of the block tests (TEST INFRASTRUCTURE).

``block`` is the body of the ``NequIPRef.energy`` loop in the segment layout of
include/e3gnn.h: rows [0, n_local) are owned (the edge centres), the rest are
ghosts; ``vec[e]`` = x[nbr[e]] - x[center[e]] (+ image), so no positions are
needed and explicit edge lists are served.  ``embed`` and ``readout`` are the
two ends of the same loop, for chaining the blocks into an energy.

``block_errors`` is the point of this file: max |got - ref| over the columns of
ONE irreps entry divided by max |ref| over the same columns, per entry, so that
an error confined to the l = 1 or l = 2 rows is not measured against the
scalars.  ``check_scales`` keeps a case honest: every entry that is compared
must carry at least 1e-2 of the largest entry's scale.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import nequip_ref  # noqa: E402
from oracle.nequip_ref import (add_bias, e3nn_linear, fctp_scalar, gate_irreps,  # noqa: E402
                               offsets, spherical_harmonics)

MIN_SCALE_RATIO = 1e-2


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(dtype)


def onehot_of(ref, types):
    return torch.nn.functional.one_hot(_t(types, torch.int64), ref.nsp).to(ref.dtype)


def embed(ref, types):
    """Layer-0 features (the head of ``NequIPRef.energy``)."""
    x = (onehot_of(ref, types) @ ref.t('onehot_to_feature_x.linear.weight').reshape(ref.nsp, -1)) \
        / math.sqrt(ref.nsp)
    return add_bias(x, ref.irreps[0], ref.p.get('onehot_to_feature_x.linear.bias'))


def block(ref, t, x, vec, center, nbr, types, n_local):
    """Features after block ``t`` on the owned rows, from features ``x`` on all
    n_local + n_ghost rows: self-connection and self_interaction_2 on the owned
    rows, self_interaction_1 and the gather on all of them."""
    dt = ref.dtype
    center, nbr = _t(center, torch.int64), _t(nbr, torch.int64)
    irr_x, irr_out = ref.irreps[t], ref.irreps[t + 1]
    gin = gate_irreps(irr_out)[0]
    emb = ref.edge_embedding(vec.norm(dim=-1))
    sh = spherical_harmonics(vec, ref.lmax_edge, ref.sh_normalize)
    xl = x[:n_local]
    if ref.sc_type == 'nequip':
        sc = fctp_scalar(xl, irr_x, onehot_of(ref, types)[:n_local], gin,
                         ref.p[f'{t}_self_connection_intro.fc_tensor_product.weight'])
    else:
        sc = e3nn_linear(xl, irr_x, gin, ref.p[f'{t}_self_connection_intro.linear.weight'])
    h = ref.lin(x.to(dt), irr_x, irr_x, f'{t}_self_interaction_1')
    agg, mid = ref.convolution(t, h, emb, sh, nbr, center, irr_x, ref.conv_out[t])
    y = ref.lin(agg[:n_local], mid, gin, f'{t}_self_interaction_2') + sc
    return ref.gate(y, irr_out)


def readout(ref, x, types):
    """Atomic energies of the owned rows ``x`` (the tail of ``NequIPRef.energy``)."""
    types = _t(types, torch.int64)[:x.shape[0]]
    if ref.man.get('readout', {}).get('type', 'linear') == 'fcn':
        e_s = ref.readout_fcn(x)
    else:
        hid = ref.lin(x, ref.irreps[-1], [(ref.hidden, 0, 1)], 'reduce_input_to_hidden')
        e_s = ref.lin(hid, [(ref.hidden, 0, 1)], [(1, 0, 1)], 'reduce_hidden_to_energy')
    return e_s[:, 0] * ref.t('rescale_atomic_energy.scale')[types] + \
        ref.t('rescale_atomic_energy.shift')[types]


def vjp(ref, t, x, vec, center, nbr, types, n_local, G):
    """(out, dE/dx on all rows, dE/dvec per edge) of block ``t`` for the
    cotangent ``G`` of its output (owned rows)."""
    dt = ref.dtype
    x = _t(x, dt).detach().clone().requires_grad_(True)
    vec = _t(vec, dt).detach().clone().requires_grad_(True)
    out = block(ref, t, x, vec, center, nbr, types, n_local)
    gx, gv = torch.autograd.grad(out, [x, vec], grad_outputs=_t(G, dt)[:n_local], allow_unused=True)
    gx = torch.zeros_like(x) if gx is None else gx
    gv = torch.zeros_like(vec) if gv is None else gv
    return out.detach(), gx.detach(), gv.detach()


def _np(a):
    return a.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(a) else \
        np.asarray(a, dtype=np.float64)


def block_scales(ref, irreps=None):
    """max |ref| per irreps entry (``irreps`` None: one entry, all columns)."""
    ref = _np(ref)
    if irreps is None:
        return [float(np.abs(ref).max()) if ref.size else 0.0]
    o = offsets(irreps)
    assert o[-1] == ref.shape[1], (o[-1], ref.shape)
    return [float(np.abs(ref[:, o[k]:o[k + 1]]).max()) if ref.shape[0] else 0.0
            for k in range(len(irreps))]


def block_errors(got, ref, irreps=None):
    """Per irreps entry: max |got - ref| over the entry's columns / max |ref|
    over the same columns.  ``irreps`` None (per-edge gradients): one scale,
    the maximum over all edges.  Non-finite ``got`` gives inf."""
    got, ref = _np(got), _np(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scales = block_scales(ref, irreps)
    o = [0, ref.shape[1]] if irreps is None else offsets(irreps)
    errs = []
    for k, s in enumerate(scales):
        d = np.abs(got[:, o[k]:o[k + 1]] - ref[:, o[k]:o[k + 1]])
        if not np.isfinite(d).all():
            errs.append(float('inf'))
        else:
            errs.append(float(d.max()) / s if d.size else 0.0)
    return errs


def check_scales(ref, irreps=None):
    """Every compared entry carries at least MIN_SCALE_RATIO of the largest
    entry's scale (else its relative error says nothing about the kernel and
    the case's inputs have to change)."""
    s = block_scales(ref, irreps)
    assert min(s) > 0.0 and min(s) >= MIN_SCALE_RATIO * max(s), s
    return s


__all__ = ['block', 'block_errors', 'block_scales', 'check_scales', 'embed', 'nequip_ref',
           'readout', 'vjp']
