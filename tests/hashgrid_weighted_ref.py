"""One hash-grid training step at points with a WEIGHT PER POINT in its loss, in float64 (a helper, not a test).

Made of oracle/hashgrid_train_ref.py's own pieces - ``rows``, ``noise``, ``level_weights``, ``encode``, ``decoder`` - the weighted loss

    loss = loss_scale sum_n w_n sum_o (y[n, o] - t[n, o])^2 / (3 N),     w_n = weight[n] > 0 ? weight[n] : 0 (in fp32; a NaN counts 0)

and ONE ``torch.autograd.grad`` over the decoder, the tables, the points and - with a level of detail - the level weights as a leaf, from which
dlod = -(dW . ramp).sum(1) . passes with ``ramp_f32`` of tests/test_hashgrid_lodgrad_cpu.py, as tests/test_hashgrid_lodtrain_cpu.py does.  At
w = 1 the products with w are exact, so it equals ``T.step`` bit for bit (tests/test_hashgrid_weighted_cpu.py).

``MISTAKES`` are the wrong kernels of the teeth: the same step with one rule of the weights damaged.  ``weights`` makes the two weight vectors
tests/test_gpu_hashgrid_weighted.py runs; both files see the same bytes."""
import types

import numpy as np
import torch

from oracle import hashgrid_train_ref as T
from tests.test_hashgrid_lodgrad_cpu import ramp_f32

F32 = np.float32
MISTAKES = ("weight ignored", "weight squared", "normalised by the sum of the weights", "weight read at pos instead of order[pos]",
            "negative weights kept", "weight on the gradient but not on the loss")
LAST_WEIGHT = 3.0


def weights(n, kind, last_row=None):
    """fp32 [n].  "mixed": uniform in [0, 4), every fifth weight 0, one NaN (row 1) and one negative (row 2) where the launch has those rows;
    "last": zeros but for ``LAST_WEIGHT`` at ``last_row`` (default n - 1: without an order the last lane of the last, partial wave)"""
    if kind == "mixed":
        w = (torch.rand(n, generator=torch.Generator().manual_seed(41)) * 4.0).numpy().astype(F32)
        w[4::5] = 0.0
        if n > 2:
            w[1], w[2] = np.nan, -1.5
        return w
    assert kind == "last"
    w = np.zeros(n, dtype=F32)
    w[n - 1 if last_row is None else int(last_row)] = LAST_WEIGHT
    return w


def clamp_weight(weight, n):
    """w_n as float64 [n] holding fp32 values: None is ones; weight > 0 ? weight : 0"""
    if weight is None:
        return np.ones(n, dtype=np.float64)
    w = np.asarray(weight, dtype=F32).reshape(n)
    with np.errstate(invalid="ignore"):
        return np.where(w > 0, w, F32(0)).astype(np.float64)


def weighted_loss(y, target, w, loss_scale):
    """loss_scale sum_n w_n sum_o (y - t)^2 / (3 N): N the number of points, not the sum of the weights"""
    return (w[:, None] * (y - target) ** 2).sum() / (3 * y.shape[0]) * float(loss_scale)


def step(geo, table, params, target, points, weight=None, loss_scale=1.0, noise_key=None, lod=None, frozen=False, mistake=None, order=None):
    """``T.step``'s arguments at points, with ``weight`` (None, or fp32 [N]).  ``lod``: None or (fade [L], lod per point [N] or None, lod_uniform);
    with it the result has ``dlod``.  ``mistake``: None or one of ``MISTAKES`` (``order``: the int64 [N] walk order "weight read at pos" needs).
    Returns y, loss, table_grad (per level, or None when frozen), decoder_grads, dpoints, row, dlod (None without ``lod``), w"""
    tab = T.as_f64(table)
    tables = [tab[l].clone().requires_grad_(not frozen) for l in range(geo.levels)]
    ps = [T.as_f64(p).clone().requires_grad_(True) for p in params]
    tgt = T.as_f64(target)
    pos = T.rows(geo, points=points)
    n = pos.t.shape[0]
    if tuple(tgt.shape) != (n, 3):
        raise ValueError(f"target must be [{n}, 3], got {tuple(tgt.shape)}")
    w = clamp_weight(weight, n)
    w_loss = None
    if mistake == "weight ignored":
        w = np.ones(n, dtype=np.float64)
    elif mistake == "weight squared":
        w = w * w
    elif mistake == "weight read at pos instead of order[pos]":
        moved = np.empty_like(w)
        moved[np.asarray(order, dtype=np.int64)] = w                      # row order[pos] is weighed by weight[pos]
        w = moved
    elif mistake == "negative weights kept":
        raw = np.asarray(weight, dtype=F32).reshape(n).astype(np.float64)
        w = np.where(np.isnan(raw), 0.0, raw)
    elif mistake == "weight on the gradient but not on the loss":
        w_loss = np.ones(n, dtype=np.float64)
    elif mistake is not None and mistake != "normalised by the sum of the weights":
        raise ValueError(mistake)
    wt = torch.from_numpy(w)
    nz = None if noise_key is None else torch.from_numpy(T.noise(n, geo.width, *noise_key))
    W = None if lod is None else torch.from_numpy(T.level_weights(geo, n, lod[0], lod[1], lod[2])).requires_grad_(True)
    row = T.encode(geo, tables, pos, nz, W)
    y = T.decoder(row, ps)
    loss = weighted_loss(y, tgt, wt, loss_scale)
    if mistake == "normalised by the sum of the weights":
        loss = loss * (n / float(w.sum()))
    leaves = ps + ([] if frozen else tables) + [pos.points] + ([] if W is None else [W])
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]
    k = len(ps)
    tg = None if frozen else list(grads[k:k + geo.levels])
    dp = grads[k + (0 if frozen else geo.levels)]
    dlod = None
    if W is not None:
        _, ramp, passes = ramp_f32(lod[0], lod[1], lod[2], n)
        dlod = -(grads[-1] * torch.from_numpy(ramp)).sum(dim=1) * torch.from_numpy(passes)
    if w_loss is not None:
        loss = weighted_loss(y, tgt, torch.from_numpy(w_loss), loss_scale)
    return types.SimpleNamespace(y=y.detach(), loss=loss.detach(), table_grad=tg, decoder_grads=list(grads[:k]), dpoints=dp, row=row.detach(), dlod=dlod,
                                 w=w)


def summed(refs):
    """the reference of a pass walked in chunks: rows back to back, losses and gradients added; dpoints / dlod row by row"""
    return types.SimpleNamespace(y=torch.cat([r.y for r in refs]), loss=sum(r.loss for r in refs),
                                 table_grad=None if refs[0].table_grad is None else [sum(r.table_grad[l] for r in refs) for l in range(len(refs[0].table_grad))],
                                 decoder_grads=[sum(r.decoder_grads[k] for r in refs) for k in range(6)], dpoints=torch.cat([r.dpoints for r in refs]),
                                 dlod=None if refs[0].dlod is None else torch.cat([r.dlod for r in refs]))
