"""GPU tests of the training step that also returns the gradient with respect to the point coordinates (nic_hash_fused_forward_backward_points_grad,
csrc/hashgrid_points_joint.hip; HashGridField.train_points(dpoints=) / train_points_differentiable).

Single calls, on the smallest shapes that reach every branch of the kernel (dense and hashed levels, L F <= 32 and > 32, one lane, a ragged
wave, thirteen waves in more than one workgroup, points outside the field, a NaN row, three orders, three levels of detail):
1. against the siblings from the same state: loss, y and the six decoder gradients bit for bit, the table gradient within TOL_ORDER (the order of
   the atomics), dpoints bit for bit nic_hash_fused_points_grad's with the target;
2. dpoints against the float64 oracle of test_gpu_hashgrid_pointgrad.py end to end within TOL_G, a clamped axis exactly 0.0;
3. with codec noise, against the layer-wise composition under the same keys; the noise is there;
4. a frozen table (table_grad None): the same dpoints, nothing scattered;   5. the same call twice gives the same bits;
6. rows follow the caller's numbering: any order gives the unordered call's dpoints bit for bit.
The surface: 7. train_points(dpoints=) on both routes against a twin field that trains without it;  8. train_points_differentiable.
And what it is for: 9. two views of one scene, the second one's positions off by a shift, field and shift trained together."""
import copy

import pytest
import torch

from test_gpu_hashgrid_pointgrad import TOL_G, TOL_ORDER, TOL_Y, _decoder, level_weights, oracle_point_gradient, oracle_row_jacobian
from test_gpu_hashgrid_points import _table
from test_gpu_hashgrid_points_train import NAMES, _field, _rand_points, _twin, relmax

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- shapes -------------------------------------------------------------------------------------------------------------------------------------
SIZES = {2: (44, 37), 3: (20, 13, 17)}
SHAPES = [(1, 8), (2, 8), (4, 8), (8, 4), (4, 9), (8, 5)]                         # (F, L): L F = 8, 16, 32, 32 (KT = 1), 36, 40 (KT = 2)
COUNTS = (1, 63, 805)                                                              # one lane; a ragged wave; thirteen waves, the last ragged, four workgroups


def _small_geo(dim, F, L):
    """log2_table = 10: the coarse levels are dense, the fine ones hashed"""
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, level_resolutions
    size = SIZES[dim]
    geo = HashGeometry(size, tuple(level_resolutions(L, 16 if dim == 2 else 4, max(size))), F, 10)
    assert {(r + 1) ** dim <= 1024 for r in geo.resolutions} == {True, False}
    return geo


def _points(geo, dev, seed, n):
    """random fractional points; then rows outside the field on one axis, an infinite coordinate and one NaN row (n = 1: the point lies outside on axis 0)"""
    pts = _rand_points(geo, dev, seed, n)
    if n == 1:
        pts[0, 0] = -3.7
        return pts
    pts[3, 0] = -3.7
    pts[7, 1] = geo.field_size[1] + 10.25
    pts[11] = float("nan")
    pts[13, geo.dim - 1] = float("inf")
    pts[17, 0] = geo.field_size[0] - 0.5                                           # the upper edge itself is inside
    return pts


def _lods(geo, dev, n):
    """None, 0.0 and one value per point in [0, 4] - with thirteen waves, wave 1 lies above every fade[l] + 1, so it gathers no level at all"""
    from neural_image_compression_v2_amd import hashgrid as hg
    fade = hg.hash_lod_fade(geo)
    assert max(fade) + 1.0 < 4.0
    per = torch.rand(n, generator=torch.Generator(device=dev).manual_seed(n), device=dev) * 4.0
    if n >= 128:
        per[64:128] = 4.0
    return [None, (None, 0.0, fade), (per, 0.0, fade)]


def _orders(geo, pts):
    from neural_image_compression_v2_amd import hashgrid as hg
    n = pts.shape[0]
    return [None, hg.hash_point_order(geo, pts), torch.arange(n - 1, -1, -1, dtype=torch.int32, device=pts.device)]


def _run(fn, geo, table, pts, params, target, lod, frozen=False, **kw):
    """one call of a training entry from zeroed gradient buffers: (loss, y, decoder gradients, table gradient or None, whatever else it returns)"""
    gm = [torch.zeros_like(p) for p in params]
    tg = None if frozen else torch.zeros_like(table)
    lod_args = () if lod is None else lod
    out = fn(geo, table, pts, params, target, gm, *lod_args, table_grad=tg, want_y=True, **kw)
    return out[0], out[1], gm, tg, out[2:]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


# ---- 1, 2, 4, 5, 6: single calls ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,L", SHAPES)
@pytest.mark.parametrize("dim", [2, 3])
def test_single_calls_against_the_siblings_and_the_oracle(dev, dim, F, L):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _small_geo(dim, F, L)
    assert hg.hash_fused_supported(geo) and (geo.width > 32) == ((F, L) in SHAPES[4:])
    table, params = _table(geo, dev, 7 * dim + F, 0.45), _decoder(geo, dev, 3 + F)
    worst = {"table_grad": 0.0, "oracle": 0.0}
    for n in COUNTS:
        pts = _points(geo, dev, seed=n + F, n=n)
        target = torch.rand(n, 3, generator=torch.Generator(device=dev).manual_seed(n), device=dev)
        scale = float(n)                                                         # dy = 2 (y - t) / 3: gradients of the size of the values
        kept = (pts >= -0.5) & (pts <= torch.tensor([s - 0.5 for s in geo.field_size], device=dev))
        assert not bool(kept.all())
        for lod in _lods(geo, dev, n):
            lod_kw = {} if lod is None else dict(lod=lod[0], lod_uniform=lod[1], fade=lod[2])
            sibling = hg.hash_fused_forward_backward_points if lod is None else hg.hash_fused_forward_backward_points_lod
            # the fused point-gradient entry (no order: row n is point n) and the oracle, once per (n, lod)
            _, dp_g = hg.hash_fused_points_grad(geo, table, pts, params, target=target, loss_scale=scale, **lod_kw)
            wts = None if lod is None else level_weights(lod[2], lod[0], lod[1], n, dev)
            _, dp_o = oracle_point_gradient(table, geo, pts, params, target=target, scale=scale, weights=wts)
            for order in _orders(geo, pts):
                what = (n, None if lod is None else ("uniform" if lod[0] is None else "per point"), None if order is None else order[:2].tolist())
                loss_s, y_s, gm_s, tg_s, _ = _run(sibling, geo, table, pts, params, target, lod, order=order, loss_scale=scale)
                loss_j, y_j, gm_j, tg_j, (dp,) = _run(hg.hash_fused_forward_backward_points_grad, geo, table, pts, params, target,
                                                      (None, 0.0, None) if lod is None else lod, order=order, loss_scale=scale)
                # 1. the siblings, same state
                assert torch.equal(loss_j, loss_s) and torch.equal(y_j, y_s), what
                for name, a, b in zip(NAMES, gm_j, gm_s):
                    assert torch.equal(a, b), (what, name)
                e_t = relmax(tg_j, tg_s)
                worst["table_grad"] = max(worst["table_grad"], e_t)
                assert e_t <= TOL_ORDER and (n == 1 or bool((tg_j != 0).any())), (what, e_t)
                assert dp.shape == (n, dim) and bool(torch.isfinite(dp).all())
                assert torch.equal(dp, dp_g), what                                 # 1. and 6.: the caller's rows, whatever the order
                # 2. the oracle; a clamped axis is exactly 0.0 (also the NaN row's)
                assert bool((dp[~kept] == 0.0).all()), what
                if float(dp_o.abs().max()) > 0:
                    e_o = _rel(dp, dp_o)
                    worst["oracle"] = max(worst["oracle"], e_o)
                    assert e_o <= TOL_G, (what, e_o)
                else:
                    assert bool((dp == 0).all()), what
                # 4. a frozen table: the same position gradient and decoder gradients, nothing scattered
                loss_f, y_f, gm_f, tg_f, (dp_f,) = _run(hg.hash_fused_forward_backward_points_grad, geo, table, pts, params, target,
                                                        (None, 0.0, None) if lod is None else lod, frozen=True, order=order, loss_scale=scale)
                assert tg_f is None and torch.equal(dp_f, dp) and torch.equal(loss_f, loss_j) and all(torch.equal(a, b) for a, b in zip(gm_f, gm_j)), what
            # 5. the same call twice from the same state, with the last order of the loop: the same bits
            twice = [_run(hg.hash_fused_forward_backward_points_grad, geo, table, pts, params, target, (None, 0.0, None) if lod is None else lod,
                          order=order, loss_scale=scale)[4][0] for _ in range(2)]
            assert torch.equal(twice[0], twice[1]) and torch.equal(twice[0], dp)
            # dpoints is overwritten whatever the flags say, the decoder gradients add
            gm = [torch.ones_like(p) for p in params]
            dp2 = torch.full((n, dim), 5.0, device=dev)
            out = hg.hash_fused_forward_backward_points_grad(geo, table, pts, params, target, gm, *((None, 0.0, None) if lod is None else lod),
                                                             loss_scale=scale, add_grads=True, dpoints=dp2)
            assert out[2] is dp2 and torch.equal(dp2, dp_g) and not torch.equal(gm[0], gm_j[0])
    print(f"{dim}D F={F} L={L}: table gradient against the sibling {worst['table_grad']:.3e}, dpoints against the oracle {worst['oracle']:.3e}")


def test_a_wave_above_every_level_gathers_nothing(dev):
    """lod = 4 for every point of wave 1 (fade[l] + 1 < 4): the whole wave jumps over every level - its rows are zero, its position gradient is
    exactly 0 whatever the table holds there, and the other waves are untouched by it"""
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _small_geo(2, 2, 8)
    table, params = _table(geo, dev, 1, 0.45), _decoder(geo, dev, 2)
    pts = _rand_points(geo, dev, 3, 805)
    target = torch.rand(805, 3, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    lod = _lods(geo, dev, 805)[2]
    _, _, _, _, (dp,) = _run(hg.hash_fused_forward_backward_points_grad, geo, table, pts, params, target, lod, loss_scale=805.0)
    assert bool((dp[64:128] == 0).all()) and bool((dp[:64] != 0).any()) and bool((dp[128:] != 0).any())


# ---- 3. noise ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_noise_against_the_layerwise_composition(dev, dim):
    from neural_image_compression_v2_amd import fused, models
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _small_geo(dim, 2, 8)
    table = models.quantize_clamp(_table(geo, dev, 5 + dim, 0.45), 6)
    params = _decoder(geo, dev, 9)
    n = 805
    pts = _points(geo, dev, seed=dim, n=n)
    target = torch.rand(n, 3, generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    quant = (6, 11, 3, 1000)                                                     # num_bits, seed, offset, sample_base
    for lod in _lods(geo, dev, n)[::2]:
        lod_kw = {} if lod is None else dict(lod=lod[0], lod_uniform=lod[1], fade=lod[2])
        x = (hg.hash_encode_points(geo, table, pts, quant=quant) if lod is None else hg.hash_encode_points_lod(geo, table, pts, quant=quant, **lod_kw))
        x.requires_grad_(True)
        y_c = fused.DecoderFunction.apply(x, *params)
        dx, = torch.autograd.grad(((y_c - target) ** 2).mean() * float(n), x)
        tg_c = torch.zeros_like(table)
        if lod is None:
            hg.hash_encode_points_backward(geo, pts, dx, tg_c)
        else:
            hg.hash_encode_points_backward_lod(geo, pts, dx, tg_c, **lod_kw)
        dp_c = hg.hash_encode_points_grad(geo, table, pts, dx, **lod_kw)
        for order in (None, hg.hash_point_order(geo, pts)):
            _, y_j, _, tg_j, (dp,) = _run(hg.hash_fused_forward_backward_points_grad, geo, table, pts, params, target,
                                          (None, 0.0, None) if lod is None else lod, order=order, loss_scale=float(n), quant=quant)
            e_y, e_g, e_t = float((y_j - y_c.detach()).abs().max()), _rel(dp, dp_c), relmax(tg_j, tg_c)
            print(f"noise {dim}D lod={'none' if lod is None else 'per point'} order={'none' if order is None else 'cell'}: y {e_y:.3e}, dpoints {e_g:.3e}, table gradient {e_t:.3e}")
            assert e_y <= TOL_Y and e_g <= TOL_G and e_t <= TOL_G
        _, y_0, _, _, (dp_0,) = _run(hg.hash_fused_forward_backward_points_grad, geo, table, pts, params, target, (None, 0.0, None) if lod is None else lod,
                                     loss_scale=float(n))
        assert not torch.equal(dp, dp_0) and not torch.equal(y_j, y_0)            # the noise is there


# ---- 7. train_points(dpoints=) -----------------------------------------------------------------------------------------------------------------
def _decoder_of(f):
    return [p.detach().clone() for p in f.decoder.linear_params()]


@pytest.mark.parametrize("lod", [None, 1.25])
@pytest.mark.parametrize("fused_route", [False, True])
def test_train_points_with_dpoints_against_a_twin_without(dev, fused_route, lod):
    """the step is the step without dpoints - fused: loss and decoder bit for bit, the table within TOL_ORDER of the largest update (the bound of
    test_tail_is_optimizer_step_bit_for_bit: the atomics' order); layer-wise: the same launches, held to the same bounds - and dpoints is
    point_gradient's at the parameters before the step"""
    base = _field((200, 131), dev, 21, fused=fused_route)
    n = 1500
    pts = _rand_points(base.geo, dev, 5, n)
    pts[5, 0], pts[9] = -7.0, float("nan")
    target = torch.rand(n, 3, generator=torch.Generator(device=dev).manual_seed(8), device=dev)
    kw = dict(fused=fused_route, order="cell", lod=lod)
    base.train_points(pts, target, **kw)                                           # off the first Adam step
    a, b, c = (_twin(base, fused=fused_route) for _ in range(3))
    table0, dec0 = base.table.detach().clone(), _decoder_of(base)
    _, want = c.point_gradient(pts, target=target, lod=lod)
    dp = torch.full((n, 2), 9.0, device=dev)
    la, lb = a.train_points(pts, target, dpoints=dp, **kw), b.train_points(pts, target, **kw)
    torch.cuda.synchronize()
    assert a.steps == b.steps == base.steps + 1
    if fused_route:
        assert torch.equal(la, lb) and torch.equal(dp, want)
        for pa, pb, p0 in zip(a.decoder.linear_params(), b.decoder.linear_params(), dec0):
            assert torch.equal(pa, pb) and not torch.equal(pa, p0)
    else:
        assert abs(float(la) - float(lb)) <= TOL_Y * abs(float(lb)) and _rel(dp, want) <= TOL_G
        for pa, pb, p0 in zip(a.decoder.linear_params(), b.decoder.linear_params(), dec0):
            assert float((pa - pb).detach().abs().max()) <= TOL_ORDER * float((pb - p0).detach().abs().max())
    upd = float((b.table.detach() - table0).abs().max())
    e = float((a.table.detach() - b.table.detach()).abs().max()) / upd
    print(f"train_points(dpoints=) {'fused' if fused_route else 'layer-wise'} lod={lod}: table {e:.3e} of the largest update {upd:.3e}")
    assert upd > 0 and e <= TOL_ORDER
    assert bool((dp[5, 0] == 0) & (dp[9] == 0).all()) and bool(torch.isfinite(dp).all())
    # the chunks of an accumulate pass each fill their own dpoints, with their own share of the loss
    a, b = _twin(base, fused=fused_route), _twin(base, fused=fused_route)
    cuts, outs = [0, 400, 1000, n], []
    for k in range(3):
        sl = slice(cuts[k], cuts[k + 1])
        share = (cuts[k + 1] - cuts[k]) / n
        ck = dict(kw, accumulate=k > 0, scale=share, step=k == 2)
        out = torch.full((cuts[k + 1] - cuts[k], 2), 9.0, device=dev)
        la = a.train_points(pts[sl].contiguous(), target[sl].contiguous(), dpoints=out, **ck)
        lb = b.train_points(pts[sl].contiguous(), target[sl].contiguous(), **ck)
        _, want = c.point_gradient(pts[sl].contiguous(), target=target[sl].contiguous(), scale=share, lod=lod)
        assert (torch.equal(out, want) and torch.equal(la, lb)) if fused_route else _rel(out, want) <= TOL_G, k
        outs.append(out)
    torch.cuda.synchronize()
    assert a.steps == b.steps == base.steps + 1 and a._pass_samples == n
    for pa, pb in zip(a.decoder.linear_params(), b.decoder.linear_params()):
        assert torch.equal(pa, pb) if fused_route else float((pa - pb).detach().abs().max()) <= TOL_ORDER * float(pb.detach().abs().max())


@pytest.mark.parametrize("fused_route", [False, True])
def test_frozen_and_refused_calls(dev, fused_route, tmp_path):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    f = _field((96, 80), dev, 4, fused=fused_route, num_bits=6)
    n = 900
    pts = _rand_points(f.geo, dev, 2, n)
    target = torch.rand(n, 3, generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    kw = dict(fused=fused_route, order="cell")
    # refused calls leave a pass in progress as it was
    f.train_points(pts[:500].contiguous(), target[:500].contiguous(), scale=0.5, step=False, noise=False, **kw)
    grad, dec = f.table.grad.clone(), [p.grad.clone() for p in f.decoder.linear_params()]
    rest, trest = pts[500:].contiguous(), target[500:].contiguous()
    keep = torch.full((400, 2), 9.0, device=dev)
    for bad, err in ((torch.zeros(399, 2, device=dev), ValueError), (torch.zeros(400, 2, dtype=torch.float64, device=dev), ValueError),
                     (torch.zeros(2, 400, device=dev).t(), ValueError), (torch.zeros(400, 2), RuntimeError), (None, ValueError)):
        with pytest.raises(err):
            if bad is None:
                f.train_points(rest, target[501:].contiguous(), accumulate=True, dpoints=keep, **kw)      # a good dpoints, one target short
            else:
                f.train_points(rest, trest, accumulate=True, dpoints=bad, **kw)
    assert torch.equal(f.table.grad, grad) and f._pass_samples == 500 and f.steps == 0 and bool((keep == 9.0).all())
    for p, g in zip(f.decoder.linear_params(), dec):
        assert torch.equal(p.grad, g)
    mixed = HashGridField((96, 80), levels=8, features=2, log2_table=12, device=dev, seed=1, num_bits=[8, 8, 6, 6, 6, 4, 4, 4], fused=fused_route)
    with pytest.raises(NotImplementedError, match="bit depth per level"):
        mixed.train_points(rest, trest, dpoints=keep, **kw)
    assert mixed.steps == 0 and bool((mixed.table.grad == 0).all()) and bool((keep == 9.0).all())
    # a frozen table: dpoints is the unfrozen call's from the same parameters (no noise in either), the table and its gradient are untouched
    f.train_points(rest, trest, accumulate=True, scale=0.5, noise=False, **kw)     # finish the pass
    f.freeze()                                                                    # quantises the table in place, drops its gradient
    g = HashGridField((96, 80), levels=8, features=2, log2_table=12, device=dev, seed=1, num_bits=6, fused=fused_route)
    with torch.no_grad():
        g.table.copy_(f.table)
    g.decoder.load_state_dict(copy.deepcopy(f.decoder.state_dict()))
    dp_u, dp_f = torch.empty(n, 2, device=dev), torch.empty(n, 2, device=dev)
    g.train_points(pts, target, noise=False, step=False, dpoints=dp_u, **kw)
    t0 = f.table.detach().clone()
    f.train_points(pts, target, dpoints=dp_f, **kw)
    torch.cuda.synchronize()
    assert f.table.grad is None and torch.equal(f.table.detach(), t0) and f.steps == 2
    assert torch.equal(dp_f, dp_u) if fused_route else _rel(dp_f, dp_u) <= TOL_G
    assert bool((dp_f != 0).any())
    # a field from load_compressed decodes only
    path = tmp_path / "f.pt"
    f.save_compressed(path)
    loaded = HashGridField.load_compressed(path, dev, fused=fused_route)
    with pytest.raises(RuntimeError, match="decodes only"):
        loaded.train_points(pts, target, dpoints=dp_f, **kw)


# ---- 8. train_points_differentiable -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_route", [False, True])
def test_train_points_differentiable(dev, fused_route):
    base = _field((200, 131), dev, 31, fused=fused_route)
    n = 1200
    pts = _rand_points(base.geo, dev, 6, n)
    target = torch.rand(n, 3, generator=torch.Generator(device=dev).manual_seed(9), device=dev)
    kw = dict(fused=fused_route, order="cell")
    a, b, c, d, e = (_twin(base, fused=fused_route) for _ in range(5))
    dp = torch.empty(n, 2, device=dev)
    lb = b.train_points(pts, target, dpoints=dp, **kw)
    # points.grad = upstream * dpoints, and the field has stepped inside the call
    leaf = pts.clone().requires_grad_(True)
    loss = a.train_points_differentiable(leaf, target, **kw)
    assert loss.requires_grad and a.steps == base.steps + 1
    (2.5 * loss).sum().backward()
    torch.cuda.synchronize()
    if fused_route:
        assert torch.equal(loss.detach(), lb) and torch.equal(leaf.grad, 2.5 * dp)
        for pa, pb in zip(a.decoder.linear_params(), b.decoder.linear_params()):
            assert torch.equal(pa, pb)
    else:
        assert abs(float(loss.detach()) - float(lb)) <= TOL_Y * abs(float(lb)) and _rel(leaf.grad, 2.5 * dp) <= TOL_G
    # a shift behind p0 + theta receives the column sums
    theta = torch.zeros(2, device=dev, requires_grad=True)
    c.train_points_differentiable(pts + theta, target, **kw).sum().backward()
    # two fp32 sums of the same n terms in different orders: each within (n - 1) 2^-24 sum |term| < 1e-4 sum |term| of the exact sum
    assert float((theta.grad - dp.sum(dim=0)).abs().max()) <= 1e-4 * float(dp.abs().sum(dim=0).max()) and bool((theta.grad != 0).all())
    # nothing asks for a gradient: train_points itself
    plain = e.train_points_differentiable(pts, target, **kw)
    assert not plain.requires_grad and e.steps == base.steps + 1
    assert torch.equal(plain, lb) if fused_route else abs(float(plain) - float(lb)) <= TOL_Y * abs(float(lb))
    with torch.no_grad():
        if fused_route:
            out = d.train_points_differentiable(pts.clone().requires_grad_(True), target, **kw)
            assert not out.requires_grad and d.steps == base.steps + 1 and torch.equal(out, plain)
        else:                                                                    # the layer-wise step runs its own backward: it needs grad mode, as train_points does
            for call in (d.train_points_differentiable, e.train_points):
                with pytest.raises(RuntimeError, match="does not require grad"):
                    call(pts.clone().requires_grad_(True), target, **kw)


# ---- 9. does it do what it is for ----------------------------------------------------------------------------------------------------------------
JOINT = dict(size=(64, 64), steps=200, lr_shift=0.05, delta=(1.25, -0.75), n=2000, seed=5)


def joint_image(p):
    """a smooth analytic image at positions p [N, 2] in samples -> [N, 3] in (0, 1)"""
    x, y = p[:, 0] / 64.0, p[:, 1] / 64.0
    return torch.stack([0.5 + 0.3 * torch.sin(7 * x + 3 * y), 0.5 + 0.3 * torch.cos(5 * x - 4 * y), 0.5 + 0.2 * torch.sin(9 * y - 2 * x)], dim=1)


def joint_views(device, dtype=torch.float32):
    """view 1: positions and colours; view 2: colours taken at its true positions, handed over with positions that are off by delta.
    (positions of both views [2 n, 2] with theta = 0, colours [2 n, 3], delta)"""
    g = torch.Generator().manual_seed(JOINT["seed"])
    p1 = torch.rand(JOINT["n"], 2, generator=g, dtype=torch.float64) * 48.0 + 8.0
    p2 = torch.rand(JOINT["n"], 2, generator=g, dtype=torch.float64) * 48.0 + 8.0
    delta = torch.tensor(JOINT["delta"], dtype=torch.float64)
    colours = torch.cat([joint_image(p1), joint_image(p2)], dim=0)
    return torch.cat([p1, p2 - delta], dim=0).to(device, dtype), colours.to(device, dtype), delta.to(device, dtype)


def run_joint(train_step, device, dtype=torch.float32):
    """the loop both the field and the float64 restatement run: points = (view 1, view 2 + theta), theta from 0 by torch Adam; ``train_step(points,
    colours)`` steps the field and returns a loss whose backward reaches theta.  (first loss, last loss, theta)"""
    p0, colours, _ = joint_views(device, dtype)
    mask = torch.cat([torch.zeros(JOINT["n"], 1), torch.ones(JOINT["n"], 1)], dim=0).to(device, dtype)
    theta = torch.zeros(2, dtype=dtype, device=device, requires_grad=True)
    opt = torch.optim.Adam([theta], lr=JOINT["lr_shift"])
    losses = []
    for _ in range(JOINT["steps"]):
        opt.zero_grad()
        loss = train_step(p0 + mask * theta, colours)
        losses.append(float(loss.detach()))
        loss.sum().backward()
        opt.step()
    return losses[0], losses[-1], theta.detach()


class OracleJointStep(torch.autograd.Function):
    """one joint step in float64 (device-agnostic; the docstring figures of the test below come from this code on a CPU): the loss at the
    current parameters, its gradients into table and decoder by autograd through the oracle's row, d loss / d points through the oracle's
    Jacobian, then the field's Adam step (table lr 1e-2, decoder 5e-3: HashGridField's groups)"""

    @staticmethod
    def forward(ctx, points, state, target):
        geo, table, params, opt = state
        p32 = points.detach().float()
        with torch.enable_grad():
            row, jac = oracle_row_jacobian(table, geo.field_size, geo.resolutions, geo.log2_table, p32)
            row.retain_grad()
            h = torch.nn.functional.gelu(row @ params[0].T + params[1])
            h = torch.nn.functional.gelu(h @ params[2].T + params[3])
            loss = ((torch.sigmoid(h @ params[4].T + params[5]) - target) ** 2).mean()
            opt.zero_grad()
            loss.backward()
        ctx.save_for_backward(torch.einsum("nk,nka->na", row.grad, jac.detach()).to(points.dtype))
        opt.step()
        return loss.detach().to(points.dtype)

    @staticmethod
    def backward(ctx, g):
        dp, = ctx.saved_tensors
        return g * dp, None, None


def oracle_joint_state(geo, table, decoder_params, device):
    table = table.detach().to(device, torch.float64).requires_grad_(True)
    params = [p.detach().to(device, torch.float64).requires_grad_(True) for p in decoder_params]
    opt = torch.optim.Adam([{"params": [table], "lr": 0.01}, {"params": params, "lr": 0.005}])
    return geo, table, params, opt


@pytest.mark.parametrize("fused_route", [False, True])
def test_two_views_register_while_the_field_is_fitted(dev, fused_route):
    """Field (64, 64), four dense levels R = 4, 8, 16, 32, F = 2, log2_table = 12, at its own seeded init (table uniform +-1e-4, the decoder's
    nn.Linear init) and its own optimiser (FusedAdam, table lr 1e-2, decoder 5e-3); two views of 2000 points each in [8, 56]^2 with colours from
    joint_image, the second view's positions off by (1.25, -0.75); 200 steps of train_points_differentiable on all 4000 points (one call steps
    the field), the shift theta from 0 by torch Adam at 0.05 on the loss's backward.  Conditions: final loss <= 0.01 of the first,
    |theta - delta|_inf <= 0.1 samples.
    The float64 restatement of this loop (OracleJointStep above) on a CPU, from the field's own initial values (decoder of seed 5 through
    ColorDecoder's init, table uniform +-1e-4 from two seeds): loss 3.7864e-02 -> 5.870e-07 / 5.879e-07 (ratio 1.55e-05), theta (1.25021,
    -0.74877) / (1.25021, -0.74879), error 0.0012 samples - both conditions with far more than a factor 2 to spare."""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    f = HashGridField(JOINT["size"], levels=4, features=2, log2_table=12, base_resolution=4, finest_resolution=32, device=dev, seed=JOINT["seed"],
                      fused=fused_route)
    assert f.resolutions == (4, 8, 16, 32) and f.route == ("fused" if fused_route else "layerwise")
    kw = dict(fused=True, order="cell") if fused_route else {}
    first, last, theta = run_joint(lambda p, c: f.train_points_differentiable(p, c, **kw), dev)
    err = float((theta - torch.tensor(JOINT["delta"], device=dev)).abs().max())
    print(f"joint {f.route}: loss {first:.4e} -> {last:.4e} (ratio {last / first:.3e}), theta {theta.tolist()}, error {err:.4f} samples")
    assert f.steps == JOINT["steps"]
    assert last <= 0.01 * first and err <= 0.1, (first, last, err)
