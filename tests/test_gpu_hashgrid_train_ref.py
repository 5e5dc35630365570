"""GPU tests that hold EVERY hash-grid training route to the float64 reference step, directly and to nothing else (oracle/hashgrid_train_ref.py;
DESIGN 4.7.17).  The inputs, the reference evaluations and the metric are those of tests/test_hashgrid_train_ref_cpu.py, which shows on the
CPU that the reference's backward is right and that these very inputs notice eight deliberate mistakes.

Routes: the layer-wise composition (hash_encode* -> DecoderFunction -> hash_encode*_backward) on crops and at points, the fused crop step, the
fused point steps (plain, ordered, with a level of detail, with the position gradient), the step with a bit depth per level, and the batched
step.  Each returns y, loss, the table gradient, six decoder gradients (and dpoints where it has them).

Metric: y by its largest absolute error (5e-6, TOL_Y); the loss relatively (TOL_Y); every decoder gradient and dpoints over the reference
tensor's largest magnitude (1e-4, TOL_G); the table gradient PER LEVEL over that level's largest magnitude in the reference (TOL_G), and an
entry the reference leaves at zero must keep the bits the buffer had; a clamped axis of dpoints is exactly 0.0.  Gradient buffers start from
non-zero contents: where the contract says "added" the base is subtracted, where it says "overwritten" the base must be gone.

One optimiser step (``HashGridField.train_step`` / ``train_points`` on both routes with num_bits = 6, ``HashGridFieldBatch.train_step``): see
``StepCase``."""
import math
import types

import numpy as np
import pytest
import torch

from oracle import hashgrid_train_ref as T
from oracle.hashgrid_fit_ref import step_bound
from tests import test_hashgrid_train_ref_cpu as C
from tests.test_hashgrid_train_ref_cpu import LOSS_SCALE, NAMES, SHAPES, TOL_G, TOL_Y, shape_id

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _geo(inp):
    from neural_image_compression_v2_amd.hashgrid import HashGeometry
    g = inp.geo
    return HashGeometry(tuple(g.field_size), tuple(g.resolutions), g.features, g.log2_table)


def _table_base(table_grad_ref, dev, seed=5):
    """[L, T, F] fp32, non-zero everywhere: half the level's largest reference gradient times U(-1, 1) - of the gradient's own size, so that
    adding to it and taking it off again costs a few ulps of the gradient and not of something larger"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for gl in table_grad_ref:
        m = float(gl.abs().max())
        u = torch.rand(gl.shape, generator=g) * 2 - 1
        u = torch.where(u == 0, torch.ones_like(u), u)
        out.append((u * (0.5 * m if m > 0 else 1e-3)).float())
    return torch.stack(out).to(dev)


def _check(what, got, ref):
    m = C.measure(got, ref)
    bad = []
    for q, (err, bound) in m.items():
        print(f"MEASURED {what} | {q} | {err:.3e} | {bound:.0e}")
        if not err <= bound:
            bad.append(f"{q}: {err:.3e} > {bound:.0e}")
    assert not bad, f"{what}: " + "; ".join(bad)


def _summed(refs):
    """the reference of a pass walked in chunks: rows back to back, losses and gradients added"""
    return types.SimpleNamespace(y=torch.cat([r.y for r in refs]), loss=sum(r.loss for r in refs),
                                 table_grad=None if refs[0].table_grad is None else [sum(r.table_grad[l] for r in refs) for l in range(len(refs[0].table_grad))],
                                 decoder_grads=[sum(r.decoder_grads[k] for r in refs) for k in range(6)], dpoints=None)


class Harness:
    """one route on one run: device copies of the run's inputs, gradient buffers with a base, the comparison"""

    def __init__(self, dev, shape, run, field=0, ref=None, frozen=False):
        self.dev, self.inp, self.run = dev, C.inputs(*shape, field), run
        self.kw = C.runs(self.inp)[run]
        self.ref = C.reference(*shape, run, field) if ref is None else ref
        self.geo = _geo(self.inp)
        self.table = self.kw["table"].to(dev)
        self.params = [p.to(dev) for p in self.inp.params]
        self.target = self.kw["target"].to(dev)
        self.frozen = frozen or self.ref.table_grad is None
        self.base = None if self.frozen else _table_base(self.ref.table_grad, dev)
        self.tg = None if self.frozen else self.base.clone()
        self.gm = [torch.full_like(p, 7.0) for p in self.params]          # overwritten: the sevens must be gone
        self.points = None if "points" not in self.kw else torch.from_numpy(self.kw["points"]).to(dev)
        lod = self.kw.get("lod")
        self.fade = None if lod is None else lod[0]
        self.lod_t = None if lod is None or lod[1] is None else torch.from_numpy(lod[1]).to(dev)
        self.lod_u = 0.0 if lod is None else lod[2]
        self.quant = self.kw.get("noise_key")
        self.scale = self.kw["loss_scale"]

    def finish(self, what, y, loss, dpoints=None):
        tgd = None
        if not self.frozen:
            tgd = [(self.tg[l].double() - self.base[l].double()).cpu() for l in range(self.geo.levels)]
        got = types.SimpleNamespace(y=y.detach().cpu(), loss=loss.detach().reshape(()).cpu(), table_grad=tgd,
                                    decoder_grads=[g.detach().cpu() for g in self.gm], dpoints=None if dpoints is None else dpoints.detach().cpu())
        _check(what, got, self.ref)
        if not self.frozen:                                               # what the reference leaves at zero keeps the buffer's bits
            for l, gl in enumerate(self.ref.table_grad):
                z = (gl == 0).to(self.dev)
                assert torch.equal(self.tg[l][z].view(torch.int32), self.base[l][z].view(torch.int32)), f"{what}: level {l}, an untouched entry moved"
        if dpoints is not None:
            _, moved = T.clamp_points(self.inp.geo, self.kw["points"])
            d = dpoints.cpu().numpy()
            assert moved.any() or d.shape[0] < C.G.N_POINTS                    # the whole set has points outside, NaN and +-inf
            assert (d[moved] == 0.0).all(), f"{what}: a clamped axis of dpoints is not 0.0"

    def layerwise(self, x, backward):
        """the decoder and the loss of the layer-wise route behind the row ``x``; ``backward(dx)`` scatters"""
        from neural_image_compression_v2_amd.fused import DecoderFunction
        x.requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in self.params]
        y = DecoderFunction.apply(x, *ps)
        loss = ((y - self.target) ** 2).mean() * self.scale
        loss.backward()
        if not self.frozen:
            backward(x.grad)
        for g, p in zip(self.gm, ps):
            g.copy_(p.grad)
        return y, loss, x.grad


CROP_RUNS = ["crops", "crops_noise", "single"]


# ---- 1. crops: layer-wise and fused
@pytest.mark.parametrize("run", CROP_RUNS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_layerwise_crops(dev, shape, run):
    from neural_image_compression_v2_amd.hashgrid import hash_encode, hash_encode_backward, hash_encode_noisy
    h = Harness(dev, shape, run)
    org, ext = h.geo.upload_origins(h.kw["origins"], h.kw["extent"], dev), h.kw["extent"]
    x = hash_encode_noisy(h.geo, h.table, org, ext, *h.quant) if h.quant else hash_encode(h.geo, h.table, org, ext)
    y, loss, _ = h.layerwise(x, lambda dx: hash_encode_backward(h.geo, org, ext, dx, h.tg))
    h.finish(f"layer-wise {run} {shape_id(shape)}", y, loss)


@pytest.mark.parametrize("run", CROP_RUNS + ["crops_frozen"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fused_crops(dev, shape, run):
    from neural_image_compression_v2_amd.hashgrid import hash_fused_forward_backward
    h = Harness(dev, shape, run)
    loss = torch.full((1,), 7.0, device=dev)
    _, y = hash_fused_forward_backward(h.geo, h.table, h.kw["origins"], h.kw["extent"], h.params, h.target, h.gm, table_grad=h.tg, loss=loss,
                                       loss_scale=h.scale, want_y=True, quant=h.quant)
    h.finish(f"fused {run} {shape_id(shape)}", y, loss)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fused_crops_two_chunks_add(dev, shape):
    """a pass in two chunks: the first overwrites the decoder gradients and the loss, the second adds (NIC_HASH_FUSED_ADD_GRADS / _ADD_LOSS)
    and draws its noise at its own sample_base"""
    from neural_image_compression_v2_amd.hashgrid import hash_fused_forward_backward
    refs = [C.reference(*shape, "chunk0"), C.reference(*shape, "chunk1")]
    h = Harness(dev, shape, "chunk0", ref=_summed(refs))
    loss = torch.full((1,), 7.0, device=dev)
    ys = []
    for k, name in enumerate(("chunk0", "chunk1")):
        kw = C.runs(h.inp)[name]
        _, y = hash_fused_forward_backward(h.geo, h.table, kw["origins"], kw["extent"], h.params, kw["target"].to(dev), h.gm, table_grad=h.tg, loss=loss,
                                           loss_scale=kw["loss_scale"], want_y=True, quant=kw["noise_key"], add_grads=k > 0, add_loss=k > 0)
        ys.append(y)
    h.finish(f"fused two chunks {shape_id(shape)}", torch.cat(ys), loss)


# ---- 2. points: layer-wise and fused
def _layerwise_points(h, order):
    from neural_image_compression_v2_amd.hashgrid import (hash_encode_points, hash_encode_points_backward, hash_encode_points_backward_lod,
                                                          hash_encode_points_grad, hash_encode_points_lod)
    if h.fade is None:
        x = hash_encode_points(h.geo, h.table, h.points, quant=h.quant)
        y, loss, dx = h.layerwise(x, lambda dx: hash_encode_points_backward(h.geo, h.points, dx, h.tg, order=order))
        dp = hash_encode_points_grad(h.geo, h.table, h.points, dx)
    else:
        x = hash_encode_points_lod(h.geo, h.table, h.points, h.lod_t, h.lod_u, h.fade, quant=h.quant)
        y, loss, dx = h.layerwise(x, lambda dx: hash_encode_points_backward_lod(h.geo, h.points, dx, h.tg, h.lod_t, h.lod_u, h.fade, order=order))
        dp = hash_encode_points_grad(h.geo, h.table, h.points, dx, lod=h.lod_t, lod_uniform=h.lod_u, fade=h.fade)
    return y, loss, dp


POINT_RUNS = ["points", "points_noise", "points_lod", "points_lod_noise", "points_lod_uniform"] + [f"points_{n}" for n in C.PREFIXES]


def _order(h, kind):
    from neural_image_compression_v2_amd.hashgrid import hash_point_order
    n = h.points.shape[0]
    if kind == "cell":
        return hash_point_order(h.geo, h.points)
    if kind == "given":
        return torch.randperm(n, generator=torch.Generator().manual_seed(11)).to(torch.int32).to(h.dev)
    return None


@pytest.mark.parametrize("order", [None, "cell"])
@pytest.mark.parametrize("run", ["points", "points_noise", "points_lod", "points_1", "points_63", "points_65"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_layerwise_points(dev, shape, run, order):
    h = Harness(dev, shape, run)
    y, loss, dp = _layerwise_points(h, _order(h, order))
    h.finish(f"layer-wise {run} order={order} {shape_id(shape)}", y, loss, dp)


@pytest.mark.parametrize("order", [None, "given"])
@pytest.mark.parametrize("run", POINT_RUNS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fused_points(dev, shape, run, order):
    """``hash_fused_forward_backward_points`` / ``_points_lod`` for y, loss and the parameter gradients, then ``_points_grad`` on fresh buffers for
    the same again plus dpoints"""
    from neural_image_compression_v2_amd.hashgrid import (hash_fused_forward_backward_points, hash_fused_forward_backward_points_grad,
                                                          hash_fused_forward_backward_points_lod)
    h = Harness(dev, shape, run)
    od = _order(h, order)
    loss = torch.full((1,), 7.0, device=dev)
    common = dict(table_grad=h.tg, order=od, loss=loss, loss_scale=h.scale, want_y=True, quant=h.quant)
    if h.fade is None:
        _, y = hash_fused_forward_backward_points(h.geo, h.table, h.points, h.params, h.target, h.gm, **common)
    else:
        _, y = hash_fused_forward_backward_points_lod(h.geo, h.table, h.points, h.params, h.target, h.gm, h.lod_t, h.lod_u, h.fade, **common)
    h.finish(f"fused {run} order={order} {shape_id(shape)}", y, loss)
    h = Harness(dev, shape, run)
    loss = torch.full((1,), 7.0, device=dev)
    dp = torch.full((h.points.shape[0], h.geo.dim), 7.0, device=dev)
    _, y, _ = hash_fused_forward_backward_points_grad(h.geo, h.table, h.points, h.params, h.target, h.gm, h.lod_t, h.lod_u, h.fade, table_grad=h.tg, order=od,
                                                      loss=loss, loss_scale=h.scale, want_y=True, quant=h.quant, dpoints=dp)
    h.finish(f"fused+dpoints {run} order={order} {shape_id(shape)}", y, loss, dp)


def test_fused_points_grad_frozen(dev):
    """table_grad = None: no scatter; dpoints and the decoder gradients are still produced"""
    from neural_image_compression_v2_amd.hashgrid import hash_fused_forward_backward_points_grad
    h = Harness(dev, (3, 4, 8), "points_lod_noise", frozen=True)
    h.ref = types.SimpleNamespace(**{**vars(h.ref), "table_grad": None})
    loss = torch.full((1,), 7.0, device=dev)
    _, y, dp = hash_fused_forward_backward_points_grad(h.geo, h.table, h.points, h.params, h.target, h.gm, h.lod_t, h.lod_u, h.fade, table_grad=None, loss=loss,
                                                       loss_scale=h.scale, want_y=True, quant=h.quant)
    h.finish("fused+dpoints frozen", y, loss, dp)


# ---- 3. a bit depth per level
@pytest.mark.parametrize("run", ["levels_crops", "levels_points"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fused_levels(dev, shape, run):
    from neural_image_compression_v2_amd.hashgrid import hash_fused_forward_backward_levels
    h = Harness(dev, shape, run)
    loss = torch.full((1,), 7.0, device=dev)
    where = dict(points=h.points, order=_order(h, "given")) if h.points is not None else dict(coord=h.kw["origins"], extent=h.kw["extent"])
    _, y = hash_fused_forward_backward_levels(h.geo, h.table, h.quant[0], h.params, h.target, h.gm, table_grad=h.tg, loss=loss, loss_scale=h.scale,
                                              want_y=True, quant=h.quant[1:], **where)
    h.finish(f"fused {run} {shape_id(shape)}", y, loss)


@pytest.mark.parametrize("run", ["levels_crops", "levels_points"])
@pytest.mark.parametrize("shape", [(2, 2, 16), (3, 4, 8)], ids=shape_id)
def test_layerwise_levels(dev, shape, run):
    from neural_image_compression_v2_amd.hashgrid import hash_encode_backward, hash_encode_levels, hash_encode_points_backward
    h = Harness(dev, shape, run)
    if h.points is not None:
        x = hash_encode_levels(h.geo, h.table, h.quant[0], points=h.points, quant=h.quant[1:])
        y, loss, _ = h.layerwise(x, lambda dx: hash_encode_points_backward(h.geo, h.points, dx, h.tg))
    else:
        org, ext = h.geo.upload_origins(h.kw["origins"], h.kw["extent"], dev), h.kw["extent"]
        x = hash_encode_levels(h.geo, h.table, h.quant[0], coord=org, extent=ext, quant=h.quant[1:])
        y, loss, _ = h.layerwise(x, lambda dx: hash_encode_backward(h.geo, org, ext, dx, h.tg))
    h.finish(f"layer-wise {run} {shape_id(shape)}", y, loss)


# ---- 4. the batch
@pytest.mark.parametrize("run", ["crops", "crops_noise"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_batch(dev, shape, run):
    """B = 3 fields that differ in table, decoder, crops and target; every field against ITS reference, its loss included"""
    from neural_image_compression_v2_amd.hashgrid import hash_batch_forward_backward
    hs = [Harness(dev, shape, run, field=b) for b in range(C.N_FIELDS)]
    geo = hs[0].geo
    tables = torch.stack([h.table for h in hs])
    params = [torch.stack([h.params[k] for h in hs]).contiguous() for k in range(6)]
    gm = [torch.full_like(p, 7.0) for p in params]
    tg = torch.stack([h.tg for h in hs])
    loss = torch.full((C.N_FIELDS,), 7.0, device=dev)
    coord = torch.tensor([h.kw["origins"] for h in hs])
    _, y = hash_batch_forward_backward(geo, tables, coord, hs[0].kw["extent"], params, torch.stack([h.target for h in hs]), gm, table_grads=tg, loss=loss,
                                       loss_scale=LOSS_SCALE, want_y=True, quant=hs[0].quant)
    for b, h in enumerate(hs):
        h.tg, h.gm = tg[b], [g[b] for g in gm]
        h.finish(f"batch {run} field {b} {shape_id(shape)}", y[b], loss[b])


# ---- 5. one optimiser step
NUM_BITS = 6
ADAM_STEP = 3                    # steps already taken: the state is not the first step's
N_EDGE = 4                       # table entries put on each edge of the quantiser's range


def _ulp32(x):
    return torch.from_numpy(np.spacing(np.abs(x.float().numpy()).astype(np.float32)).astype(np.float64))


def _step_bound(gmax, m_max, lr, betas, eps, step):
    """the Lipschitz constant of Adam's update in the gradient, times TOL_G gmax (see ``StepCase``): ``step_bound`` of
    oracle/hashgrid_fit_ref.py with this file's floor, sqrt(v') >= sqrt(beta2 v) >= sqrt(beta2) 0.1 gmax whatever g is"""
    return step_bound(gmax, m_max, lr, betas, eps, step, s0=math.sqrt(betas[1]) * 0.1 * gmax)


class Moments:
    """Adam's state of one tensor (one level of one field's table, or one decoder tensor of one field) and the largest reference gradient"""

    def __init__(self, g, gen):
        self.gmax = float(g.abs().max())
        assert self.gmax > 0
        self.m = 0.01 * self.gmax * (torch.rand(g.shape, generator=gen, dtype=torch.float64) * 2 - 1)
        self.v = (0.1 * self.gmax) ** 2 * (1.001 + torch.rand(g.shape, generator=gen, dtype=torch.float64))


class StepCase:
    """One optimiser step of a field (``mode`` "crops" / "points") or of a batch of three ("batch") against ``adam_step`` on the reference's
    gradients, from a state both sides know.  ``run`` is the whole test; the methods are its stages in order.

    The pass is walked in two chunks (accumulate, scale = 1/2 each, step on the last).  Noise keys by the documented rule: offset = the
    optimiser steps taken (3), sample_base = the samples of the pass before the chunk.  Adam's state (``Moments``): step = 3, exp_avg = 0.01
    gmax U(-1, 1), exp_avg_sq = (0.1 gmax)^2 (1.001 + U(0, 1)) >= (0.1 gmax)^2 also once rounded to fp32, gmax = the largest reference
    gradient of this very step per tensor - per level (and field) for the table.  It goes in through the optimiser's torch-compatible
    state_dict; ``field.steps`` = 3 is the field's own counter.  N_EDGE table entries of the coarsest level sit exactly on each edge of the
    quantiser's range where the gradient pushes outward (asserted): after the step they equal the edge exactly, on both sides.

    Bound.  The new parameter is p - U(g), U(g) = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps), m' = b1 m + (1 - b1) g,
    v' = b2 v + (1 - b2) g^2, bc_i = 1 - b_i^4.  dU/dg = (lr / bc1) [ (1 - b1) / D - m' (1 - b2) g / (sqrt(v') sqrt(bc2) D^2) ] with
    D = sqrt(v' / bc2) + eps.  With the floor, sqrt(v') >= sqrt(b2) 0.1 gmax =: s0 and D >= s0 / sqrt(bc2) + eps =: D0 for EVERY g, and on the
    segment between the reference gradient and one within TOL_G gmax of it |g| <= gmax (1 + TOL_G) =: g+ and |m'| <= b1 max|m| + (1 - b1) g+
    =: m+.  So |dU/dg| <= Lip = (lr / bc1) [ (1 - b1) / D0 + m+ (1 - b2) g+ / (s0 sqrt(bc2) D0^2) ], and a gradient that meets TOL_G moves
    the parameter by at most Lip TOL_G gmax.  The fp32 arithmetic of the update itself and the final rounding add one fp32 ulp of the
    parameter.  A clamp only shrinks a difference.  bound = Lip TOL_G gmax + ulp32(p) - about 2e-7 for a table level at lr 0.01, 1e-7 for a
    decoder tensor - per tensor, per level and field for the table."""

    def __init__(self, dev, shape, mode, fused, frozen):
        from neural_image_compression_v2_amd import hashgrid
        self.dev, self.shape, self.mode, self.fused, self.frozen = dev, shape, mode, fused, frozen
        self.batch = mode == "batch"
        self.B = C.N_FIELDS if self.batch else 1
        self.inps = [C.inputs(*shape, b) for b in range(self.B)]
        self.L = shape[2]
        spec = C.SPECS[shape[0]]
        args = dict(levels=shape[2], features=shape[1], log2_table=spec["log2_table"], base_resolution=spec["base"], device=dev, seed=1,
                    num_bits=NUM_BITS, noise_seed=C.NOISE_SEED)
        if self.batch:
            self.field = hashgrid.HashGridFieldBatch(self.B, spec["field_size"], **args)
            self.tab_p, self.dec_p = self.field.tables, self.field.params
        else:
            self.field = hashgrid.HashGridField(spec["field_size"], fused=fused, **args)
            assert self.field.route == ("fused" if fused else "layerwise")
            self.tab_p, self.dec_p = self.field.table, self.field.decoder.linear_params()
        assert tuple(self.field.geo.resolutions) == tuple(self.inps[0].geo.resolutions)
        self.lo, self.hi = T.q_range(NUM_BITS)
        self.tables = [i.table_c.clamp(self.lo, self.hi).clone() for i in self.inps]       # own copies: the edges are written into them
        self.params = [[p.clone() for p in i.params] for i in self.inps]
        n_pts, cut = self.inps[0].points.shape[0], 100
        self.sizes = [cut, n_pts - cut] if mode == "points" else [self.inps[0].n_chunk] * 2
        self.what = f"step {mode} {'fused' if fused else 'layer-wise'}{' frozen' if frozen else ''} {shape_id(shape)}"

    # fields stacked for a batch, the single field's tensor otherwise - and back
    def stacked(self, per_field):
        return torch.stack(per_field) if self.batch else per_field[0]

    def of_field(self, t, b):
        return t[b] if self.batch else t

    def install_parameters(self):
        with torch.no_grad():
            self.tab_p.copy_(self.stacked(self.tables).to(self.dev))
            for k, p in enumerate(self.dec_p):
                p.copy_(self.stacked([q[k] for q in self.params]).to(self.dev))

    def freeze(self):
        """quantise on the device; what the table holds then is the input of both sides"""
        self.field.freeze()
        self.frozen_bits = self.tab_p.detach().clone()
        back = self.tab_p.detach().cpu()
        self.tables = [self.of_field(back, b) for b in range(self.B)]

    def chunk_kw(self, i, k):
        if self.mode == "points":
            sl = slice(0, self.sizes[0]) if k == 0 else slice(self.sizes[0], None)
            return dict(points=i.points[sl], target=i.target_points[sl])
        return dict(origins=i.crops[k:k + 1], extent=i.extent, target=i.target[k * i.n_chunk:(k + 1) * i.n_chunk])

    def reference(self):
        """per field the two chunks' ``T.step``, and their summed gradients"""
        self.refs = []
        for b, i in enumerate(self.inps):
            keys = [None if self.frozen else (NUM_BITS, C.NOISE_SEED, ADAM_STEP, sum(self.sizes[:k])) for k in range(2)]
            self.refs.append([T.step(i.geo, self.tables[b], self.params[b], loss_scale=0.5, noise_key=keys[k], frozen=self.frozen, **self.chunk_kw(i, k))
                              for k in range(2)])
        self.grads_t = None if self.frozen else [[sum(r.table_grad[l] for r in rs) for l in range(self.L)] for rs in self.refs]
        self.grads_d = [[sum(r.decoder_grads[k] for r in rs) for k in range(6)] for rs in self.refs]

    def put_edges(self):
        """entries of the coarsest level onto the edges of the range, where the gradient pushes outward; then the reference again"""
        for b in range(self.B):
            order = self.grads_t[b][0].reshape(-1).argsort()
            flat = self.tables[b][0].reshape(-1)
            flat[order[:N_EDGE]] = self.hi           # the most negative gradients: the step goes up, out of the range
            flat[order[-N_EDGE:]] = self.lo
        self.install_parameters()
        self.reference()
        self.edges = []
        for b in range(self.B):
            flat = self.tables[b][0].reshape(-1)
            at_hi, at_lo = torch.nonzero(flat == self.hi).reshape(-1), torch.nonzero(flat == self.lo).reshape(-1)
            assert len(at_hi) == N_EDGE and len(at_lo) == N_EDGE
            self.edges.append((at_hi, at_lo))

    def adam_state(self):
        gen = torch.Generator().manual_seed(17)
        self.st_t = None if self.frozen else [[Moments(g, gen) for g in self.grads_t[b]] for b in range(self.B)]
        self.st_d = [[Moments(g, gen) for g in self.grads_d[b]] for b in range(self.B)]
        if not self.frozen:
            for b, (at_hi, at_lo) in enumerate(self.edges):
                g, st = self.grads_t[b][0].reshape(-1), self.st_t[b][0]
                st.m.reshape(-1)[torch.cat([at_hi, at_lo])] = 0.0
                assert (g[at_hi] < -0.01 * st.gmax).all() and (g[at_lo] > 0.01 * st.gmax).all(), "the edge entries' gradients must push outward"

    def install_state(self):
        """through the optimiser's state_dict; afterwards the moments are read back: the fp32 values are what both sides start from"""
        opt = self.field.optimizer
        sd = opt.state_dict()
        index = {id(p): idx for grp, ids in zip(opt.param_groups, sd["param_groups"]) for p, idx in zip(grp["params"], ids["params"])}

        def entry(per_field_m, per_field_v):
            return {"step": torch.tensor(float(ADAM_STEP)), "exp_avg": self.stacked(per_field_m).float(), "exp_avg_sq": self.stacked(per_field_v).float()}

        state = {}
        if not self.frozen:
            state[index[id(self.tab_p)]] = entry([torch.stack([s.m for s in self.st_t[b]]) for b in range(self.B)],
                                                 [torch.stack([s.v for s in self.st_t[b]]) for b in range(self.B)])
        for k, p in enumerate(self.dec_p):
            state[index[id(p)]] = entry([self.st_d[b][k].m for b in range(self.B)], [self.st_d[b][k].v for b in range(self.B)])
        opt.load_state_dict({"state": state, "param_groups": sd["param_groups"]})
        self.field.steps = ADAM_STEP
        for b in range(self.B):
            if not self.frozen:
                s = opt.state[self.tab_p]
                m, v = self.of_field(s["exp_avg"].detach().cpu().double(), b), self.of_field(s["exp_avg_sq"].detach().cpu().double(), b)
                for l, st in enumerate(self.st_t[b]):
                    st.m, st.v = m[l], v[l]
                    assert float(st.v.min()) >= (0.1 * st.gmax) ** 2
            for k, p in enumerate(self.dec_p):
                s, st = opt.state[p], self.st_d[b][k]
                st.m, st.v = self.of_field(s["exp_avg"].detach().cpu().double(), b), self.of_field(s["exp_avg_sq"].detach().cpu().double(), b)

    def run_pass(self):
        """the two chunks on the GPU; the chunk losses against the reference's"""
        f, dev, i0 = self.field, self.dev, self.inps[0]
        for k in range(2):
            kws = [self.chunk_kw(i, k) for i in self.inps]
            acc = dict(accumulate=k > 0, scale=0.5, step=k == 1)
            if self.mode == "points":
                loss = f.train_points(torch.from_numpy(kws[0]["points"]).to(dev), kws[0]["target"].to(dev), fused=self.fused, **acc)
            elif self.batch:
                loss = f.train_step(torch.tensor([kw["origins"] for kw in kws]), i0.extent, torch.stack([kw["target"] for kw in kws]).to(dev), **acc)
            else:
                loss = f.train_step(kws[0]["origins"], i0.extent, kws[0]["target"].to(dev), **acc)
            for b in range(self.B):
                got, want = float(loss.reshape(-1)[b]), float(self.refs[b][k].loss)
                err = abs(got - want) / abs(want)
                print(f"MEASURED {self.what} | loss chunk {k} field {b} | {err:.3e} | {TOL_Y:.0e}")
                assert err <= TOL_Y, (self.what, k, b, err)
        assert f.steps == ADAM_STEP + 1

    def off_bound(self, got, start, grad, st, lr, betas, eps, clamp=None):
        """the largest |got - adam_step(...)| / bound over one tensor"""
        want, _, _ = T.adam_step(start, grad, st.m, st.v, ADAM_STEP + 1, lr, betas, eps, clamp=clamp)
        bound = _step_bound(st.gmax, float(st.m.abs().max()), lr, betas, eps, ADAM_STEP + 1) + _ulp32(want)
        return float(((got.double() - want).abs() / bound).max())

    def compare_parameters(self):
        groups = self.field.optimizer.param_groups
        lr_t, lr_d, betas, eps = groups[0]["lr"], groups[1]["lr"], groups[0]["betas"], groups[0]["eps"]
        assert (lr_t, lr_d, tuple(betas), eps) == (0.01, 0.005, (0.9, 0.999), 1e-8)
        if self.frozen:
            assert torch.equal(self.tab_p.detach().view(torch.int32), self.frozen_bits.view(torch.int32)), "a frozen table moved"
        worst_t, worst_d = 0.0, 0.0
        for b in range(self.B):
            if not self.frozen:
                new_t = self.of_field(self.tab_p.detach().cpu(), b)
                for l in range(self.L):
                    ratio = self.off_bound(new_t[l], self.tables[b][l], self.grads_t[b][l], self.st_t[b][l], lr_t, betas, eps, clamp=(self.lo, self.hi))
                    worst_t = max(worst_t, ratio)
                    assert ratio <= 1.0, f"{self.what}: field {b} level {l}: the table is {ratio:.2f} x its bound off"
                at_hi, at_lo = self.edges[b]
                flat = new_t[0].reshape(-1)
                assert (flat[at_hi] == self.hi).all() and (flat[at_lo] == self.lo).all(), f"{self.what}: an edge entry left the edge"
            for k in range(6):
                ratio = self.off_bound(self.of_field(self.dec_p[k].detach().cpu(), b), self.params[b][k], self.grads_d[b][k], self.st_d[b][k], lr_d, betas, eps)
                worst_d = max(worst_d, ratio)
                assert ratio <= 1.0, f"{self.what}: field {b} {NAMES[k][1:]}: {ratio:.2f} x its bound off"
        print(f"MEASURED {self.what} | parameters after the step, error / bound | table {worst_t:.3f} | decoder {worst_d:.3f}")

    def run(self):
        self.install_parameters()
        if self.frozen:
            self.freeze()
        self.reference()
        if not self.frozen:
            self.put_edges()
        self.adam_state()
        self.install_state()
        self.run_pass()
        self.compare_parameters()


def _optimiser_step(dev, shape, mode, fused, frozen=False):
    StepCase(dev, shape, mode, fused, frozen).run()


STEP_SHAPES = [(2, 2, 16), (3, 4, 8)]


@pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])
@pytest.mark.parametrize("mode", ["crops", "points"])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=shape_id)
def test_optimiser_step_field(dev, shape, mode, fused):
    _optimiser_step(dev, shape, mode, fused)


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=shape_id)
def test_optimiser_step_batch(dev, shape):
    _optimiser_step(dev, shape, "batch", True)


@pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])
@pytest.mark.parametrize("mode", ["crops", "points"])
def test_optimiser_step_frozen_field(dev, mode, fused):
    """after ``freeze()`` the table keeps its bits and the decoder meets the same bound"""
    _optimiser_step(dev, (2, 2, 16), mode, fused, frozen=True)
