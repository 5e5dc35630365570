"""GPU tests of the per-point loss weights of the training step at points (nic_hash_fused_forward_backward_points_weighted,
csrc/hashgrid_weighted.hip; HashGridField.train_points_weighted / train_points_weighted_differentiable / fit_points_weighted /
fit_mips_weighted).  Inputs are tests/test_hashgrid_train_ref_cpu.py's nine shapes with their 209 points; the float64 reference
is tests/hashgrid_weighted_ref.py's ``step``, held on the CPU (tests/test_hashgrid_weighted_cpu.py) to ``T.step`` at w = 1, to differences of its
own loss and to six deliberate mistakes on these very inputs and weights.  Metric and bounds are ``C.measure``'s: TOL_Y = 5e-6 for y and the
loss, TOL_G = 1e-4 for every gradient, the table per level; dlod over the reference's largest magnitude to TOL_G.

1. the fused entry against the weighted reference: every ``points*`` run, with and without a given order, with and without dpoints / dlod, two
   weight vectors (mixed; one non-zero weight on the last lane of the last, partial wave); buffers start non-zero; a frozen table;
2. all weights zero;
3. weight = None and ones against the four siblings, bit for bit (the table gradient as two calls of one sibling agree);
4. weights 4 w: exactly 4 x the loss, the decoder gradients, dpoints and dlod;
5. the layer-wise route of ``train_points_weighted``;
6. bookkeeping: an accumulate pass in two chunks; three steps with ones against three of ``train_points``;
7. one optimiser step against ``T.adam_step`` on the reference's gradients (tests/test_gpu_hashgrid_train_ref.py's ``StepCase``);
8. ``train_points_weighted_differentiable``;
9. ``fit_points_weighted`` / ``fit_mips_weighted``."""
import types

import numpy as np
import pytest
import torch

from oracle import hashgrid_train_ref as T
from tests import hashgrid_weighted_ref as W
from tests import test_gpu_hashgrid_train_ref as R
from tests import test_hashgrid_train_ref_cpu as C
from tests import test_hashgrid_weighted_cpu as WC
from tests.test_gpu_hashgrid_train_ref import Harness, dev  # noqa: F401
from tests.test_hashgrid_train_ref_cpu import LOSS_SCALE, SHAPES, TOL_G, TOL_Y, shape_id

pytestmark = pytest.mark.gpu

TOL_ORDER = 1e-5                  # the table gradient against a sibling's: the order of the atomics (tests/test_gpu_hashgrid_lodtrain.py)
SIBLING_SHAPES = [(2, 2, 16), (2, 4, 10), (3, 4, 8)]
TWO_SHAPES = [(2, 2, 16), (3, 4, 8)]


def _hg():
    from neural_image_compression_v2_amd import hashgrid
    return hashgrid


def _check_rows(what, ref, dp, dl):
    """dlod against the reference; rows of weight 0 are == 0.0 in dpoints and dlod"""
    zero = torch.from_numpy(ref.w == 0)
    if dp is not None:
        assert bool((dp.cpu()[zero] == 0.0).all()), f"{what}: dpoints of a row of weight 0"
    if dl is not None:
        err = C.relmax(dl.cpu(), ref.dlod)
        print(f"MEASURED {what} | dlod | {err:.3e} | {TOL_G:.0e}")
        assert err <= TOL_G, f"{what}: dlod {err:.3e}"
        assert bool((dl.cpu()[zero] == 0.0).all()) and bool(torch.isfinite(dl).all()), f"{what}: dlod of a row of weight 0"


# ---- 1. the fused entry against the weighted reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", WC.POINT_RUNS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fused_entry_against_the_weighted_reference(dev, shape, run):
    hg = _hg()
    inp = C.inputs(*shape)
    kw = C.runs(inp)[run]
    n = kw["points"].shape[0]
    perm = WC.permutation(n)
    refs = {}
    for order in (None, "given"):
        od = None if order is None else perm.to(torch.int32).to(dev)
        for kind in WC.KINDS:
            last = None if (order is None or kind == "mixed") else int(perm[n - 1])            # the row the last lane handles
            weight = W.weights(n, kind, last)
            key = (kind, last)
            if key not in refs:
                refs[key] = W.step(inp.geo, params=inp.params, weight=weight, **WC.step_kw(kw))
            ref = refs[key]
            for grads in (True, False):
                h = Harness(dev, shape, run, ref=ref)
                what = f"weighted {run} order={order} {kind} grads={grads} {shape_id(shape)}"
                dp = torch.full((n, h.geo.dim), 7.0, device=dev) if grads else None
                dl = torch.full((n,), 7.0, device=dev) if grads and h.fade is not None else None
                y = torch.full((n, 3), 7.0, device=dev)
                wt = torch.from_numpy(weight).to(dev)
                loss = torch.full((1,), 7.0, device=dev)
                out = hg.hash_fused_forward_backward_points_weighted(h.geo, h.table, h.points, h.params, h.target, wt, h.gm, h.lod_t, h.lod_u, h.fade,
                                                                     table_grad=h.tg, order=od, loss=loss, loss_scale=h.scale, want_y=True, quant=h.quant,
                                                                     dpoints=dp, dlod=dl)
                assert out[0] is loss and out[2] is dp and out[3] is dl
                h.finish(what, out[1], loss, dp)
                _check_rows(what, ref, dp, dl)


def test_fused_entry_with_a_frozen_table(dev):
    """table_grad = None: no scatter; everything else is still produced"""
    shape, run = (3, 4, 8), "points_lod_noise"
    inp = C.inputs(*shape)
    kw = C.runs(inp)[run]
    n = kw["points"].shape[0]
    weight = W.weights(n, "mixed")
    ref = W.step(inp.geo, params=inp.params, weight=weight, frozen=True, **WC.step_kw(kw))
    h = Harness(dev, shape, run, ref=ref, frozen=True)
    dp, dl = torch.full((n, 3), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    loss = torch.full((1,), 7.0, device=dev)
    out = _hg().hash_fused_forward_backward_points_weighted(h.geo, h.table, h.points, h.params, h.target, torch.from_numpy(weight).to(dev), h.gm, h.lod_t,
                                                            h.lod_u, h.fade, table_grad=None, loss=loss, loss_scale=h.scale, want_y=True, quant=h.quant,
                                                            dpoints=dp, dlod=dl)
    h.finish("weighted frozen", out[1], loss, dp)
    _check_rows("weighted frozen", ref, dp, dl)


# ---- 2. all weights zero --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["points", "points_lod_noise"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_all_weights_zero(dev, shape, run):
    """loss exactly 0.0, every decoder gradient exactly 0 (overwrite mode), the table gradient buffer == its base, dpoints / dlod == 0.0; y is the
    plain forward's bit for bit: the sibling step's y with the same arguments (noise included) and, without noise, the decode kernel's
    (``hash_fused_forward_points``)"""
    hg = _hg()
    tsize = C.inputs(*shape).geo.table_size
    h = Harness(dev, shape, run, ref=types.SimpleNamespace(table_grad=[torch.ones(tsize, shape[1])] * shape[2]))      # only the base of the buffer is made from it
    n = h.points.shape[0]
    lodded = h.fade is not None
    dp = torch.full((n, h.geo.dim), 7.0, device=dev)
    dl = torch.full((n,), 7.0, device=dev) if lodded else None
    loss = torch.full((1,), 7.0, device=dev)
    out = hg.hash_fused_forward_backward_points_weighted(h.geo, h.table, h.points, h.params, h.target, torch.zeros(n, device=dev), h.gm, h.lod_t, h.lod_u,
                                                         h.fade, table_grad=h.tg, loss=loss, loss_scale=h.scale, want_y=True, quant=h.quant, dpoints=dp, dlod=dl)
    assert float(loss) == 0.0 and not bool(torch.signbit(loss).any())
    assert all(bool((g == 0).all()) for g in h.gm)
    assert torch.equal(h.tg.view(torch.int32), h.base.view(torch.int32))
    assert bool((dp == 0.0).all()) and (dl is None or bool((dl == 0.0).all()))
    gm = [torch.zeros_like(p) for p in h.params]
    if lodded:
        _, y_s = hg.hash_fused_forward_backward_points_lod(h.geo, h.table, h.points, h.params, h.target, gm, h.lod_t, h.lod_u, h.fade, loss_scale=h.scale,
                                                           want_y=True, quant=h.quant)
    else:
        _, y_s = hg.hash_fused_forward_backward_points(h.geo, h.table, h.points, h.params, h.target, gm, loss_scale=h.scale, want_y=True, quant=h.quant)
    assert torch.equal(out[1], y_s)
    if h.quant is None:
        assert torch.equal(out[1], hg.hash_fused_forward_points(h.geo, h.table, h.points, h.params))


# ---- 3. weight = None and ones against the four siblings -----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [None, "given"])
@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("shape", SIBLING_SHAPES, ids=shape_id)
def test_none_and_ones_are_the_siblings(dev, shape, noise, order):
    hg = _hg()
    inp = C.inputs(*shape)
    n = inp.points.shape[0]
    od = None if order is None else WC.permutation(n).to(torch.int32).to(dev)
    for lodded in (False, True):
        run = ("points_lod" if lodded else "points") + ("_noise" if noise else "")
        h = Harness(dev, shape, run)
        lod_args = (h.lod_t, h.lod_u, h.fade)
        common = dict(order=od, loss_scale=h.scale, want_y=True, quant=h.quant)

        def fresh():
            return [torch.zeros_like(p) for p in h.params], torch.zeros_like(h.table)
        siblings = {}
        gm, tg = fresh()
        if lodded:
            out = hg.hash_fused_forward_backward_points_lod(h.geo, h.table, h.points, h.params, h.target, gm, *lod_args, table_grad=tg, **common)
        else:
            out = hg.hash_fused_forward_backward_points(h.geo, h.table, h.points, h.params, h.target, gm, table_grad=tg, **common)
        siblings["step"] = (out[0], out[1], gm, tg, None, None)
        gm, tg = fresh()
        out = hg.hash_fused_forward_backward_points_grad(h.geo, h.table, h.points, h.params, h.target, gm, *lod_args, table_grad=tg, **common)
        siblings["grad"] = (out[0], out[1], gm, tg, out[2], None)
        if lodded:
            gm, tg = fresh()
            out = hg.hash_fused_forward_backward_points_grad_lod(h.geo, h.table, h.points, h.params, h.target, gm, *lod_args, table_grad=tg, **common)
            siblings["grad_lod"] = (out[0], out[1], gm, tg, out[2], out[3])
        for name, (loss_s, y_s, gm_s, tg_s, dp_s, dl_s) in siblings.items():
            for weight in (None, torch.ones(n, device=dev)):
                gm, tg = fresh()
                dp = None if dp_s is None else torch.full_like(dp_s, 7.0)
                dl = None if dl_s is None else torch.full_like(dl_s, 7.0)
                out = hg.hash_fused_forward_backward_points_weighted(h.geo, h.table, h.points, h.params, h.target, weight, gm, *lod_args, table_grad=tg,
                                                                     dpoints=dp, dlod=dl, **common)
                what = (run, name, order, "None" if weight is None else "ones")
                assert torch.equal(out[0], loss_s) and torch.equal(out[1], y_s), what
                assert all(torch.equal(a, b) for a, b in zip(gm, gm_s)), what
                assert (dp is None or torch.equal(dp, dp_s)) and (dl is None or torch.equal(dl, dl_s)), what
                e_t = float((tg - tg_s).abs().max() / tg_s.abs().max())
                assert e_t <= TOL_ORDER, (what, e_t)


# ---- 4. power-of-two scaling ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TWO_SHAPES, ids=shape_id)
def test_four_times_the_weights_is_four_times_everything(dev, shape):
    """the weight enters once and linearly: a factor 4 commutes with every rounding, so the bits are those of the exact product"""
    run = "points_lod_noise"
    n = C.inputs(*shape).points.shape[0]
    weight = W.clamp_weight(W.weights(n, "mixed"), n).astype(np.float32)
    got = []
    for factor in (1.0, 4.0):
        h = Harness(dev, shape, run)
        h.gm = [torch.zeros_like(p) for p in h.params]
        dp, dl = torch.full((n, h.geo.dim), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
        loss = torch.full((1,), 7.0, device=dev)
        _hg().hash_fused_forward_backward_points_weighted(h.geo, h.table, h.points, h.params, h.target, torch.from_numpy(weight * np.float32(factor)).to(dev),
                                                          h.gm, h.lod_t, h.lod_u, h.fade, table_grad=None, loss=loss, loss_scale=h.scale, quant=h.quant,
                                                          dpoints=dp, dlod=dl)
        got.append([loss] + h.gm + [dp, dl])
    for a, b in zip(*got):
        assert bool((a != 0).any()) and torch.equal(4.0 * a, b)


# ---- 5. the layer-wise route ----------------------------------------------------------------------------------------------------------------
def _field_of(dev, shape, fused, table, params, num_bits=None):
    """a field of the shape's geometry holding ``table`` and ``params``"""
    spec = C.SPECS[shape[0]]
    f = _hg().HashGridField(spec["field_size"], levels=shape[2], features=shape[1], log2_table=spec["log2_table"], base_resolution=spec["base"], device=dev,
                            seed=1, num_bits=num_bits, noise_seed=C.NOISE_SEED, fused=fused)
    assert f.route == ("fused" if fused else "layerwise") and tuple(f.geo.resolutions) == tuple(C.inputs(*shape).geo.resolutions)
    with torch.no_grad():
        f.table.copy_(table.to(dev))
        for p, q in zip(f.decoder.linear_params(), params):
            p.copy_(q.to(dev))
    return f


def _field_grads(f, fused):
    """(table gradient per level, decoder gradients) a step=False call left in the field, as CPU tensors"""
    dec = f._fused_gm if fused else [p.grad for p in f.decoder.linear_params()]
    return [f.table.grad[l].detach().double().cpu() for l in range(f.geo.levels)], [g.detach().cpu() for g in dec]


@pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])
@pytest.mark.parametrize("shape", TWO_SHAPES, ids=shape_id)
def test_train_points_weighted_against_the_reference(dev, shape, fused):
    inp = C.inputs(*shape)
    kw = C.runs(inp)["points_lod"]
    n = kw["points"].shape[0]
    weight = W.weights(n, "mixed")
    ref = W.step(inp.geo, params=inp.params, weight=weight, **WC.step_kw(kw))
    assert tuple(kw["lod"][0]) == tuple(T.default_fade(inp.geo))
    f = _field_of(dev, shape, fused, kw["table"], inp.params)
    pts, target, lod = torch.from_numpy(kw["points"]).to(dev), kw["target"].to(dev), torch.from_numpy(kw["lod"][1]).to(dev)
    dp, dl = torch.full((n, inp.dim), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    y = f.query(pts, lod=lod)
    loss = f.train_points_weighted(pts, target, torch.from_numpy(weight).to(dev), lod=lod, dpoints=dp, dlod=dl, scale=LOSS_SCALE, step=False, fused=fused)
    tg, dec = _field_grads(f, fused)
    got = types.SimpleNamespace(y=y.detach().cpu(), loss=loss.detach().reshape(()).cpu(), table_grad=tg, decoder_grads=dec, dpoints=dp.cpu())
    what = f"train_points_weighted {'fused' if fused else 'layer-wise'} {shape_id(shape)}"
    R._check(what, got, ref)
    _check_rows(what, ref, dp, dl)
    assert f.steps == 0 and f._pass_samples == n


# ---- 6. bookkeeping -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])
@pytest.mark.parametrize("shape", TWO_SHAPES, ids=shape_id)
def test_an_accumulate_pass_in_two_chunks_adds(dev, shape, fused):
    """one pass in two ``accumulate`` chunks equals the reference's sum of the two, the second chunk's noise keyed by the samples before it"""
    inp = C.inputs(*shape)
    kw = C.runs(inp)["points_lod_noise"]
    n, n1 = kw["points"].shape[0], 100
    weight = W.weights(n, "mixed")
    cuts = [slice(0, n1), slice(n1, n)]
    refs = [W.step(inp.geo, kw["table"], inp.params, kw["target"][sl], kw["points"][sl], weight[sl], loss_scale=LOSS_SCALE * (sl.stop - sl.start) / n,
                   noise_key=(C.NOISE_BITS, C.NOISE_SEED, 0, sl.start), lod=(kw["lod"][0], kw["lod"][1][sl], 0.0)) for sl in cuts]
    ref = W.summed(refs)
    f = _field_of(dev, shape, fused, kw["table"], inp.params, num_bits=C.NOISE_BITS)
    pts, target, lod, wt = (torch.from_numpy(kw["points"]).to(dev), kw["target"].to(dev), torch.from_numpy(kw["lod"][1]).to(dev),
                            torch.from_numpy(weight).to(dev))
    dps, dls, losses = [], [], []
    for k, sl in enumerate(cuts):
        dp, dl = torch.full((sl.stop - sl.start, inp.dim), 7.0, device=dev), torch.full((sl.stop - sl.start,), 7.0, device=dev)
        losses.append(f.train_points_weighted(pts[sl].contiguous(), target[sl].contiguous(), wt[sl].contiguous(), lod=lod[sl].contiguous(), dpoints=dp, dlod=dl,
                                              accumulate=k > 0, scale=LOSS_SCALE * (sl.stop - sl.start) / n, step=False, fused=fused))
        dps.append(dp)
        dls.append(dl)
        assert f._pass_samples == sl.stop and f.steps == 0
    tg, dec = _field_grads(f, fused)
    ref.w = W.clamp_weight(weight, n)
    got = types.SimpleNamespace(y=ref.y.float(), loss=(losses[0] + losses[1]).detach().reshape(()).cpu(), table_grad=tg, decoder_grads=dec,
                                dpoints=torch.cat(dps).cpu())
    what = f"two chunks {'fused' if fused else 'layer-wise'} {shape_id(shape)}"
    R._check(what, got, ref)
    _check_rows(what, ref, torch.cat(dps), torch.cat(dls))


@pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])
@pytest.mark.parametrize("shape", TWO_SHAPES, ids=shape_id)
def test_three_steps_with_ones_are_three_steps_of_train_points(dev, shape, fused):
    """equal losses, decoder parameters and Adam moments bit for bit, the tables within 1e-5 of the largest update, ``steps`` / ``_pass_samples``
    equal.  The 63-point prefix: one wave makes all the adds into the table, so its gradient does not depend on the order of the atomics and
    the second and third step start from the same bits on both sides; across waves only the first step could be held bit for bit"""
    inp = C.inputs(*shape)
    kw = C.runs(inp)["points_lod_noise"]
    n = 63
    pts, target, lod = torch.from_numpy(kw["points"][:n]).to(dev), kw["target"][:n].contiguous().to(dev), torch.from_numpy(kw["lod"][1][:n]).to(dev)
    a, b = (_field_of(dev, shape, fused, kw["table"], inp.params, num_bits=C.NOISE_BITS) for _ in range(2))
    start = a.table.detach().clone()
    ones = torch.ones(n, device=dev)
    for k in range(3):
        la = a.train_points_weighted(pts, target, ones, lod=lod, fused=fused, order="cell")
        lb = b.train_points(pts, target, lod=lod, fused=fused, order="cell")
        assert torch.equal(la, lb), k
        assert a.steps == b.steps == k + 1 and a._pass_samples == b._pass_samples == n
    for pa, pb in zip(a.decoder.linear_params(), b.decoder.linear_params()):
        assert torch.equal(pa, pb)
        sa, sb = a.optimizer.state[pa], b.optimizer.state[pb]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    upd = float((b.table.detach() - start).abs().max())
    e_t = float((a.table.detach() - b.table.detach()).abs().max()) / upd
    print(f"three steps {'fused' if fused else 'layer-wise'} {shape_id(shape)}: tables {e_t:.3e} of the largest update")
    assert upd > 0 and e_t <= TOL_ORDER


# ---- 7. one optimiser step ------------------------------------------------------------------------------------------------------------------
class WeightedStepCase(R.StepCase):
    """``StepCase`` at points with the mixed weights: the reference's gradients are the weighted step's, the pass is ``train_points_weighted``'s"""

    def weight(self, k):
        w = W.weights(self.inps[0].points.shape[0], "mixed")
        return w[:self.sizes[0]] if k == 0 else w[self.sizes[0]:]

    def reference(self):
        i = self.inps[0]
        keys = [(R.NUM_BITS, C.NOISE_SEED, R.ADAM_STEP, sum(self.sizes[:k])) for k in range(2)]
        self.refs = [[W.step(i.geo, self.tables[0], self.params[0], weight=self.weight(k), loss_scale=0.5, noise_key=keys[k], **self.chunk_kw(i, k))
                      for k in range(2)]]
        self.grads_t = [[sum(r.table_grad[l] for r in self.refs[0]) for l in range(self.L)]]
        self.grads_d = [[sum(r.decoder_grads[k] for r in self.refs[0]) for k in range(6)]]

    def run_pass(self):
        f, dev = self.field, self.dev
        for k in range(2):
            kw = self.chunk_kw(self.inps[0], k)
            loss = f.train_points_weighted(torch.from_numpy(kw["points"]).to(dev), kw["target"].to(dev), torch.from_numpy(self.weight(k)).to(dev),
                                           accumulate=k > 0, scale=0.5, step=k == 1, fused=self.fused)
            err = abs(float(loss) - float(self.refs[0][k].loss)) / abs(float(self.refs[0][k].loss))
            print(f"MEASURED {self.what} | loss chunk {k} | {err:.3e} | {TOL_Y:.0e}")
            assert err <= TOL_Y, (self.what, k, err)
        assert f.steps == R.ADAM_STEP + 1


@pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])
@pytest.mark.parametrize("shape", R.STEP_SHAPES, ids=shape_id)
def test_optimiser_step(dev, shape, fused):
    case = WeightedStepCase(dev, shape, "points", fused, False)
    case.what = "weighted " + case.what
    case.run()


# ---- 8. the autograd op ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])
def test_train_points_weighted_differentiable(dev, fused):
    shape = (2, 2, 16)
    inp = C.inputs(*shape)
    kw = C.runs(inp)["points_lod"]
    n = kw["points"].shape[0]
    pts = torch.from_numpy(np.nan_to_num(kw["points"], nan=1.0, posinf=50.0, neginf=-5.0)).to(dev)
    target, wt = kw["target"].to(dev), torch.from_numpy(W.weights(n, "mixed")).to(dev)
    upstream = 3.0
    for lod0 in (torch.from_numpy(kw["lod"][1]).to(dev), torch.tensor(1.25, device=dev), None):
        a, b = (_field_of(dev, shape, fused, kw["table"], inp.params) for _ in range(2))
        dp = torch.full((n, 2), 7.0, device=dev)
        dl = None if lod0 is None else torch.full((n,), 7.0, device=dev)
        lb = b.train_points_weighted(pts, target, wt, lod=lod0, dpoints=dp, dlod=dl, fused=fused)
        p = pts.clone().requires_grad_(True)
        lod = None if lod0 is None else lod0.clone().requires_grad_(True)
        la = a.train_points_weighted_differentiable(p, target, wt, lod, fused=fused)
        assert la.requires_grad and torch.equal(la.detach(), lb) and a.steps == b.steps == 1
        (upstream * la).sum().backward()
        assert torch.equal(p.grad, torch.tensor(upstream, device=dev) * dp) and bool((p.grad != 0).any())
        if lod is not None:
            want = torch.tensor(upstream, device=dev) * (dl if lod.dim() > 0 else dl.sum())
            assert lod.grad.shape == lod.shape and torch.equal(lod.grad, want.reshape(lod.shape)) and bool((lod.grad != 0).any())
        assert wt.grad is None
        # nothing requires a gradient: the plain call
        c = _field_of(dev, shape, fused, kw["table"], inp.params)
        lc = c.train_points_weighted_differentiable(pts, target, wt, lod0, fused=fused)
        assert not lc.requires_grad and torch.equal(lc, lb)


# ---- 9. the fit loops -----------------------------------------------------------------------------------------------------------------------
def _fit_field(dev, fused, size=(32, 32)):
    return _hg().HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=21, fused=fused)


@pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])
def test_fit_loops_with_ones_are_the_unweighted_loops(dev, fused):
    from tests.test_gpu_hashgrid_lod import _striped
    size = (32, 32)
    image = _striped(size, dev)
    a, b = _fit_field(dev, fused), _fit_field(dev, fused)
    assert torch.equal(a.table.detach(), b.table.detach())
    pts = a._resample_points(size, [0, 0], size)
    cols = image.reshape(-1, 3).contiguous()
    ha = a.fit_points_weighted(pts, cols, torch.ones(pts.shape[0], device=dev), 1)
    hb = b.fit_points(pts, cols, 1)
    assert ha == hb and len(ha) == 1 and a.steps == b.steps == 1
    # in chunks: a chunk's scale is its share of the points by count
    a, b = _fit_field(dev, fused), _fit_field(dev, fused)
    assert a.fit_points_weighted(pts, cols, torch.ones(pts.shape[0], device=dev), 1, batch=300) == b.fit_points(pts, cols, 1, batch=300)
    a, b = _fit_field(dev, fused), _fit_field(dev, fused)
    assert a.fit_mips_weighted(image, 1, mip_weights=None) == b.fit_mips(image, 1) and a.steps == b.steps == 1


@pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])
def test_balanced_mips_weigh_every_mip_alike(dev, fused):
    """with "balanced" the first pass's loss is the mean of the three per-mip mean squared errors of the initial field (``decode_mip``)"""
    from tests.test_gpu_hashgrid_lod import _box, _striped
    image = _striped((32, 32), dev)
    a, b = _fit_field(dev, fused), _fit_field(dev, fused)
    mses = [float(((b.decode_mip(m).double() - _box(image, m).double()) ** 2).mean()) for m in range(3)]
    got = a.fit_mips_weighted(image, 1, mips=2, mip_weights="balanced")[0]
    want = sum(mses) / 3
    plain = _fit_field(dev, fused).fit_mips(image, 1)[0]
    err = abs(got - want) / want
    print(f"balanced mips {'fused' if fused else 'layer-wise'}: per-mip MSE {mses}, loss {got:.6e} against their mean {want:.6e} ({err:.2e}); fit_mips {plain:.6e}")
    assert err <= TOL_Y and abs(plain - want) / want > 100 * TOL_Y
