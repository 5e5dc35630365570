"""GPU tests of the gradient with respect to the level of detail (nic_hash_encode_points_grad_lod / nic_hash_fused_points_grad_lod,
csrc/hashgrid_lodgrad.hip; HashGridField.point_gradient_lod / jacobian_lod / query_differentiable_lod).  Inputs and the float64
reference are tests/test_hashgrid_lodgrad_cpu.py's (built there from oracle/hashgrid_train_ref.py's pieces and held to differences of its own
loss); the bound is TOL_G of tests/test_gpu_hashgrid_pointgrad.py, 1e-4 of the largest magnitude of the compared tensor.

1. the layer-wise entry against the reference - dlod and dpoints -, every (dim, F, source), every launch length, the three ways to give lambda;
   dpoints bit for bit nic_hash_encode_points_grad's;
2. the fused entry with dy and with target: y bit for bit nic_hash_fused_forward_points_lod's, dpoints bit for bit nic_hash_fused_points_grad's,
   dlod against the reference end to end and against the layer-wise composition, L F on both sides of 32;
3. exact zeros (no level on the ramp, lambda_raw < 0, >= 32, NaN; checked in 1 and 2 on every launch) and points outside the field: dlod of the
   clamped point bit for bit, not zero;
4. an independent check that restates no formula: central differences of the forward in lambda (h = 1/8) where every weight stays inside one
   linear piece;
5. determinism and overwrite: two calls give equal bits, rows n < n_points of sentinel-filled outputs are overwritten, nothing past them is touched;
6. the surface on both routes and from load_compressed fields; the existing calls return what they returned before the new ones ran;
7. it can be descended on: a level of detail recovered by torch Adam on a 0-dim lod."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import hashgrid_train_ref as T
from tests import test_gpu_hashgrid_pointgrad as PG
from tests import test_hashgrid_lodgrad_cpu as L
from tests.test_hashgrid_lodgrad_cpu import MODES, N, TARGET_SCALE, rel
from tests.test_gpu_hashgrid_pointgrad import TOL_G

pytestmark = pytest.mark.gpu

SOURCES = [("f32", None), ("u8", 8), ("u8", 5), ("bits", 4), ("bits", 5)]          # packed: b = 4 tight, b = 5 straddling
LENGTHS = (1, 63, 64, 65, 130)
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _source(inp, dev, kind, bits):
    """(data on the device, kind, num_bits, the fp32 [L, T, F] values the forward blends, on the CPU)"""
    from neural_image_compression_v2_amd import hashgrid as hg
    from neural_image_compression_v2_amd import models
    table = inp.table.to(dev)
    if kind == "f32":
        return table, kind, None, inp.table
    clamped = models.quantize_clamp(table, bits)
    stored = hg.hash_pack_u8(inp.geo, clamped, bits)
    data = stored if kind == "u8" else hg.hash_pack_bits(inp.geo, clamped, bits)
    return data, kind, bits, hg._table_of_u8(inp.geo, stored, bits).cpu()


def _lod_kw(inp, mode, n, dev):
    """the level of detail of a launch of the first n rows: (keywords of the wrappers, (lod or None, lod_uniform) for the reference)"""
    lod, u = L.mode_lod(inp, mode, n)
    return dict(lod=None if lod is None else torch.from_numpy(lod).to(dev), lod_uniform=u, fade=inp.fade), (lod, u)


def _check_zeros(dlod, ref):
    """rows with no level on the ramp, or whose lambda_raw is < 0, >= 32 or NaN, are exactly 0"""
    flat = torch.from_numpy(~ref.passes | ~ref.ramp.any(axis=1))
    assert bool((dlod.cpu()[flat] == 0).all()) and bool(torch.isfinite(dlod).all())


def _compose(inp, data, kind, bits, pts, params, lod_kw, dy=None, target=None, scale=1.0):
    """the layer-wise composition: encode_lod -> general decoder -> its backward to the row -> nic_hash_encode_points_grad_lod"""
    from neural_image_compression_v2_amd import fused
    from neural_image_compression_v2_amd import hashgrid as hg
    x = hg.hash_encode_points_lod(inp.geo, data, pts, kind=kind, num_bits=bits, **lod_kw)
    x.requires_grad_(True)
    y = fused.DecoderFunction.apply(x, *params)
    g = dy if dy is not None else (y.detach() - target) * (2.0 * scale / (3.0 * pts.shape[0]))
    dx, = torch.autograd.grad(y, x, g)
    return (y.detach(),) + hg.hash_encode_points_grad_lod(inp.geo, data, pts, dx, kind, bits, **lod_kw)


# ---- 1. the layer-wise entry against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("dim", [2, 3])
def test_layerwise_entry_against_the_reference(dev, dim, F):
    from neural_image_compression_v2_amd import hashgrid as hg
    inp = L.inputs(dim, F)
    worst = {"dlod": 0.0, "dpoints": 0.0}
    for kind, bits in SOURCES:
        data, kind, bits, values = _source(inp, dev, kind, bits)
        for mode in MODES:
            for n in (LENGTHS if mode == "point" else (N,)):
                pts, dx = inp.points[:n].contiguous().to(dev), inp.dx[:n].contiguous().to(dev)
                kw, (lod, u) = _lod_kw(inp, mode, n, dev)
                ref = L.reference(inp.tgeo, values, inp.params, inp.points[:n], inp.fade, lod, u, dx=inp.dx[:n])
                dp, dl = hg.hash_encode_points_grad_lod(inp.geo, data, pts, dx, kind, bits, **kw)
                assert dp.shape == (n, dim) and dl.shape == (n,) and dl.dtype == torch.float32
                assert torch.equal(dp, hg.hash_encode_points_grad(inp.geo, data, pts, dx, kind, bits, **kw))       # the sibling's bits
                e_l, e_p = rel(dl, ref.dlod), rel(dp, ref.dpoints)
                worst = {"dlod": max(worst["dlod"], e_l), "dpoints": max(worst["dpoints"], e_p)}
                assert e_l < TOL_G and e_p < TOL_G, (kind, bits, mode, n, e_l, e_p)
                _check_zeros(dl, ref)
                on_start = torch.from_numpy((ref.a_raw == 1).any(axis=1) & ref.passes)                          # rows exactly on a_raw == 1: the right-hand value
                if bool(on_start.any()):
                    assert bool((ref.dlod[on_start] != 0).all())
                    assert float((dl.cpu().double() - ref.dlod)[on_start].abs().max()) < TOL_G * float(ref.dlod.abs().max())
    print(f"layer-wise {dim}D F={F}: dlod {worst['dlod']:.3e}, dpoints {worst['dpoints']:.3e} of the largest magnitude")
    e = hg.hash_encode_points_grad_lod(inp.geo, data, pts[:0].contiguous(), dx[:0].contiguous(), kind, bits, fade=inp.fade)
    assert e[0].shape == (0, dim) and e[1].shape == (0,)


# ---- 2. the fused entry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,F,levels", [(2, 1, 4), (3, 2, 4), (2, 4, 4), (3, 8, 4), (2, 8, 5), (3, 8, 5)])      # L F = 4, 8, 16, 32 (one k tile), 40 (two)
def test_fused_entry_against_the_reference_and_the_composition(dev, dim, F, levels):
    from neural_image_compression_v2_amd import hashgrid as hg
    inp = L.inputs(dim, F, levels)
    assert hg.hash_fused_supported(inp.geo) and (inp.geo.width > 32) == (levels == 5)
    params = [p.to(dev) for p in inp.params]
    worst = {"ref": 0.0, "compose": 0.0}
    for kind, bits in SOURCES:
        data, kind, bits, values = _source(inp, dev, kind, bits)
        for mode in MODES:
            for n in (LENGTHS if mode == "point" and kind != "u8" else (N,)):
                pts = inp.points[:n].contiguous().to(dev)
                kw, (lod, u) = _lod_kw(inp, mode, n, dev)
                y_fwd = hg.hash_fused_forward_points_lod(inp.geo, data, pts, params, kind=kind, num_bits=bits, **kw)
                for head in ("dy", "target"):
                    cpu = dict(dy=inp.dy[:n]) if head == "dy" else dict(target=inp.target[:n], loss_scale=TARGET_SCALE * n)
                    gpu = {k: (v.contiguous().to(dev) if isinstance(v, torch.Tensor) else v) for k, v in cpu.items()}
                    ref = L.reference(inp.tgeo, values, inp.params, inp.points[:n], inp.fade, lod, u, **cpu)
                    y, dp, dl = hg.hash_fused_points_grad_lod(inp.geo, data, pts, params, kind=kind, num_bits=bits, **gpu, **kw)
                    assert y.shape == (n, 3) and dp.shape == (n, dim) and dl.shape == (n,)
                    assert torch.equal(y, y_fwd)                                                                    # the forward's bits
                    y_s, dp_s = hg.hash_fused_points_grad(inp.geo, data, pts, params, kind=kind, num_bits=bits, **gpu, **kw)
                    assert torch.equal(dp, dp_s) and torch.equal(y, y_s)                                            # the sibling's bits
                    comp = {("scale" if k == "loss_scale" else k): v for k, v in gpu.items()}
                    _, dp_c, dl_c = _compose(inp, data, kind, bits, pts, params, kw, **comp)
                    e_r, e_c = rel(dl, ref.dlod), float((dl - dl_c).abs().max() / ref.dlod.abs().max())
                    worst = {"ref": max(worst["ref"], e_r), "compose": max(worst["compose"], e_c)}
                    assert e_r < TOL_G and e_c < TOL_G and rel(dp, ref.dpoints) < TOL_G, (kind, bits, mode, n, head, e_r, e_c)
                    _check_zeros(dl, ref)
                    none_y, dp_n, dl_n = hg.hash_fused_points_grad_lod(inp.geo, data, pts, params, want_y=False, kind=kind, num_bits=bits, **gpu, **kw)
                    assert none_y is None and torch.equal(dp_n, dp) and torch.equal(dl_n, dl)                       # the same bits, with and without y
    print(f"fused {dim}D L F = {inp.geo.width}: dlod against the reference {worst['ref']:.3e}, against the composition {worst['compose']:.3e}")
    e = hg.hash_fused_points_grad_lod(inp.geo, data, pts[:0].contiguous(), params, dy=gpu.get("dy", torch.zeros(n, 3, device=dev))[:0].contiguous(), kind=kind,
                                      num_bits=bits, fade=inp.fade)
    assert e[0].shape == (0, 3) and e[1].shape == (0, dim) and e[2].shape == (0,)


# ---- 3. points outside the field ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_a_point_outside_the_field_has_the_clamped_points_dlod(dev, dim):
    from neural_image_compression_v2_amd import hashgrid as hg
    inp = L.inputs(dim, 2)
    clamped, moved = T.clamp_points(inp.tgeo, inp.points.numpy())
    out = list(L.OUTSIDE_ROWS)
    assert moved[out].any(axis=1).all()
    pts, inside = inp.points.to(dev), torch.from_numpy(clamped.astype(np.float32)).contiguous().to(dev)
    params, dx, dy = [p.to(dev) for p in inp.params], inp.dx.to(dev), inp.dy.to(dev)
    kw, _ = _lod_kw(inp, "point", N, dev)
    for kind, bits in (("f32", None), ("bits", 5)):
        data, kind, bits, _ = _source(inp, dev, kind, bits)
        pairs = [(hg.hash_encode_points_grad_lod(inp.geo, data, p, dx, kind, bits, **kw) for p in (pts, inside)),
                 (hg.hash_fused_points_grad_lod(inp.geo, data, p, params, dy=dy, kind=kind, num_bits=bits, **kw)[1:] for p in (pts, inside))]
        for (dp, dl), (dp_in, dl_in) in pairs:
            assert torch.equal(dl, dl_in) and bool((dl[out] != 0).all())                                            # not zeroed
            assert bool((dp[torch.from_numpy(moved)] == 0).all())                                                   # the position gradient is, on those axes


# ---- 4. an independent check: central differences in lambda ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_central_differences_in_lambda_where_the_weights_are_affine(dev, dim):
    """lambda a multiple of 1/16, h = 1/8, rows where every a_raw stays off, on the ramp or at full weight over [lambda - h, lambda + h]
    (``affine_rows``; at least half of the rows, asserted on the CPU): the row is affine in lambda there and (y(lambda + h) - y(lambda - h)) . dy
    / 2 h is dlod up to the decoder's curvature - the GENTLE decoder keeps that below a third of the bound on the float64 reference (CPU file)"""
    from neural_image_compression_v2_amd import hashgrid as hg
    inp = L.inputs(dim, 2)
    lod = L.affine_lod()
    keep = torch.from_numpy(L.affine_rows(inp.fade, lod)).to(dev)
    assert int(keep.sum()) >= N // 2
    params = [p.to(dev) for p in L.decoder_params(inp.geo.width, 3, **L.GENTLE)]
    pts, dy, table = inp.points.to(dev), inp.dy.to(dev), inp.table.to(dev)
    lam = torch.from_numpy(lod).to(dev)
    up = hg.hash_fused_forward_points_lod(inp.geo, table, pts, params, lod=lam + L.H_GPU, fade=inp.fade)
    down = hg.hash_fused_forward_points_lod(inp.geo, table, pts, params, lod=lam - L.H_GPU, fade=inp.fade)
    want = (dy.double() * (up.double() - down.double())).sum(dim=1) / (2 * L.H_GPU)
    _, _, fused_dl = hg.hash_fused_points_grad_lod(inp.geo, table, pts, params, dy=dy, lod=lam, fade=inp.fade)
    _, _, comp_dl = _compose(inp, table, "f32", None, pts, params, dict(lod=lam, lod_uniform=0.0, fade=inp.fade), dy=dy)
    for name, got in (("fused", fused_dl), ("layer-wise", comp_dl)):
        err = float((got.double() - want)[keep].abs().max() / want[keep].abs().max())
        print(f"central differences in lambda {dim}D, {name}: {err:.3e} of {float(want[keep].abs().max()):.3e} at {int(keep.sum())} of {N} rows")
        assert err < TOL_G, (name, err)
    assert float(want[keep].abs().max()) > 1e-2                                  # the check is not vacuous


# ---- 5. determinism and overwrite -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 130])
def test_the_same_bits_twice_and_nothing_past_the_rows(dev, n):
    from neural_image_compression_v2_amd import _lib, fused
    from neural_image_compression_v2_amd import hashgrid as hg
    inp = L.inputs(3, 8, 5)
    geo, pad = inp.geo, 70
    params = [p.to(dev) for p in inp.params]
    pts, dx, dy = inp.points[:n].contiguous().to(dev), inp.dx[:n].contiguous().to(dev), inp.dy[:n].contiguous().to(dev)
    kw, _ = _lod_kw(inp, "point", n, dev)
    for kind, bits in (("f32", None), ("bits", 4)):
        data, kind, bits, _ = _source(inp, dev, kind, bits)
        a, b = (hg.hash_encode_points_grad_lod(geo, data, pts, dx, kind, bits, **kw) for _ in range(2))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        c, d = (hg.hash_fused_points_grad_lod(geo, data, pts, params, dy=dy, kind=kind, num_bits=bits, **kw) for _ in range(2))
        assert all(torch.equal(u, v) for u, v in zip(c, d))
        # the C entries on sentinel-filled outputs with room past the rows
        src, data = hg._point_source(geo, data, kind, bits)
        desc, lp, m = hg._point_desc(geo), hg._lod_struct(geo, inp.fade, 0.0), fused._mlp_struct(params)
        lib, stream = _lib.load(), _lib.stream_ptr(dev)
        dp, dl, y = (torch.full(shape, SENTINEL, device=dev) for shape in ((n + pad, geo.dim), (n + pad,), (n + pad, 3)))
        _lib.check(lib.nic_hash_encode_points_grad_lod(ctypes.byref(desc), ctypes.byref(lp), ctypes.byref(src), _lib.ptr(pts), _lib.ptr(kw["lod"]), n, _lib.ptr(dx),
                                                       _lib.ptr(dp), _lib.ptr(dl), stream))
        assert torch.equal(dp[:n], a[0]) and torch.equal(dl[:n], a[1]) and bool((dp[n:] == SENTINEL).all()) and bool((dl[n:] == SENTINEL).all())
        dp.fill_(SENTINEL), dl.fill_(SENTINEL)
        _lib.check(lib.nic_hash_fused_points_grad_lod(ctypes.byref(desc), ctypes.byref(lp), ctypes.byref(src), _lib.ptr(pts), _lib.ptr(kw["lod"]), n, ctypes.byref(m),
                                                      _lib.ptr(dy), None, 1.0, _lib.ptr(y), _lib.ptr(dp), _lib.ptr(dl), stream))
        assert torch.equal(y[:n], c[0]) and torch.equal(dp[:n], c[1]) and torch.equal(dl[:n], c[2])
        assert bool((y[n:] == SENTINEL).all()) and bool((dp[n:] == SENTINEL).all()) and bool((dl[n:] == SENTINEL).all())


# ---- 6. the surface -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_route", [False, True])
def test_the_surface(dev, fused_route, tmp_path):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    f = PG._field((40, 27), dev, 11, fused=fused_route, num_bits=6, levels=4, log2_table=10, base_resolution=4)
    assert f.route == ("fused" if fused_route else "layerwise")
    n = 200
    g = torch.Generator().manual_seed(2)
    pts_c = (torch.rand(n, 2, generator=g) * torch.tensor([42.0, 29.0]) - 1.5).contiguous()            # some outside the field
    lod_c = (torch.rand(n, generator=g) * 4.5).contiguous()
    lod_c[:4] = torch.tensor([0.0, -1.0, 40.0, float("nan")])
    dy_c, target_c = torch.rand(n, 3, generator=g) * 2 - 1, torch.rand(n, 3, generator=g)
    pts, lod, dy, target = pts_c.to(dev), lod_c.to(dev), dy_c.to(dev), target_c.to(dev)
    before = PG._training_state(f)
    # the existing calls, before any new one runs
    old_pg = [f.point_gradient(pts, dy=dy, lod=l) for l in (lod, 1.25)]
    leaf = pts.clone().requires_grad_(True)
    f.query_differentiable(leaf, lod=lod).backward(dy)
    old_qd = leaf.grad.clone()
    # point_gradient_lod: the sibling's y and dpoints bit for bit, dlod against the reference, both modes, per point and launch-wide
    tgeo = T.Geometry(f.geo.field_size, f.geo.resolutions, f.geo.features, f.geo.log2_table)
    params_c = [p.detach().cpu() for p in f.decoder.linear_params()]
    for l_gpu, l_ref in ((lod, (lod_c.numpy(), 0.0)), (1.25, (None, 1.25))):
        for gpu, cpu in ((dict(dy=dy), dict(dy=dy_c)), (dict(target=target, scale=3.0 * n), dict(target=target_c, loss_scale=3.0 * n))):
            y, dp, dl = f.point_gradient_lod(pts, l_gpu, **gpu)
            y_s, dp_s = f.point_gradient(pts, lod=l_gpu, **gpu)
            assert torch.equal(y, y_s) and torch.equal(dp, dp_s) and dl.shape == (n,)
            ref = L.reference(tgeo, f.table.detach().cpu(), params_c, pts_c, f.lod_fade, l_ref[0], l_ref[1], **cpu)
            assert rel(dl, ref.dlod) < TOL_G and float(ref.dlod.abs().max()) > 1e-2, (l_ref[1], list(gpu))
            _check_zeros(dl, ref)
    # jacobian_lod: three one-hot calls
    jac = f.jacobian_lod(pts, lod)
    assert jac.shape == (n, 3)
    for o in range(3):
        hot = torch.zeros(n, 3, device=dev)
        hot[:, o] = 1.0
        assert torch.equal(jac[:, o], f.point_gradient_lod(pts, lod, dy=hot)[2])
    # query_differentiable_lod: point_gradient_lod's gradients bit for bit, for the points, a [N] lod and - as the sum - a 0-dim lod
    _, dp, dl = f.point_gradient_lod(pts, lod, dy=dy)
    p_leaf, l_leaf = pts.clone().requires_grad_(True), lod.clone().requires_grad_(True)
    out = f.query_differentiable_lod(p_leaf, l_leaf)
    assert out.requires_grad and torch.equal(out.detach(), f.query(pts, lod=lod))
    out.backward(dy)
    assert torch.equal(p_leaf.grad, dp) and torch.equal(l_leaf.grad, dl)
    l_leaf = lod.clone().requires_grad_(True)
    f.query_differentiable_lod(pts, l_leaf).backward(dy)                          # the level of detail alone
    assert torch.equal(l_leaf.grad, dl)
    scalar = torch.tensor(1.25, device=dev, requires_grad=True)
    out = f.query_differentiable_lod(pts, scalar)
    assert torch.equal(out.detach(), f.query(pts, lod=1.25))
    out.backward(dy)
    assert scalar.grad.shape == () and torch.equal(scalar.grad, f.point_gradient_lod(pts, 1.25, dy=dy)[2].sum())
    # the plain path: query itself, bit for bit
    assert not f.query_differentiable_lod(pts, lod).requires_grad and torch.equal(f.query_differentiable_lod(pts, lod), f.query(pts, lod=lod))
    with torch.no_grad():
        plain = f.query_differentiable_lod(pts.clone().requires_grad_(True), lod.clone().requires_grad_(True))
    assert not plain.requires_grad and torch.equal(plain, f.query(pts, lod=lod))
    # nothing of the training state moved: no .grad, no optimiser state, no step count
    PG._same_state(before, PG._training_state(f))
    # the existing calls are unchanged
    for l, (y0, dp0) in zip((lod, 1.25), old_pg):
        y1, dp1 = f.point_gradient(pts, dy=dy, lod=l)
        assert torch.equal(y0, y1) and torch.equal(dp0, dp1)
    leaf = pts.clone().requires_grad_(True)
    f.query_differentiable(leaf, lod=lod).backward(dy)
    assert torch.equal(leaf.grad, old_qd)
    l_leaf = lod.clone().requires_grad_(True)
    assert not f.query_differentiable(pts, lod=l_leaf).requires_grad               # as before: no gradient for lod from query_differentiable
    # a field from load_compressed (uint8 and packed) answers point_gradient_lod from its stored table
    f.freeze()
    frozen = f.point_gradient_lod(pts, lod, dy=dy)
    for packed in (False, True):
        path = tmp_path / f"f{int(packed)}.pt"
        f.save_compressed(path, packed=packed)
        loaded = HashGridField.load_compressed(path, dev, fused=fused_route)
        assert loaded.table is None and loaded.route == f.route
        y_l, dp_l, dl_l = loaded.point_gradient_lod(pts, lod, dy=dy)
        assert float((y_l - frozen[0]).abs().max()) < PG.TOL_Y and rel(dp_l, frozen[1]) < TOL_G and rel(dl_l, frozen[2]) < TOL_G, packed
        assert bool((dl_l != 0).any()) and bool(torch.isfinite(dl_l).all())
        hot = torch.tensor([[0.0, 1.0, 0.0]] * 10, device=dev)
        assert torch.equal(loaded.jacobian_lod(pts[:10].contiguous(), 0.5)[:, 1], loaded.point_gradient_lod(pts[:10].contiguous(), 0.5, dy=hot)[2])
        l_leaf = lod.clone().requires_grad_(True)
        loaded.query_differentiable_lod(pts, l_leaf).backward(dy)
        assert torch.equal(l_leaf.grad, dl_l)
    # a bit depth per level: not built
    mixed = HashGridField((40, 27), levels=4, features=2, log2_table=10, base_resolution=4, device=dev, seed=3, num_bits=(8, 6, 5, 4), fused=fused_route)
    for call in (lambda: mixed.point_gradient_lod(pts, lod, dy=dy), lambda: mixed.jacobian_lod(pts, lod),
                 lambda: mixed.query_differentiable_lod(pts, lod.clone().requires_grad_(True))):
        with pytest.raises(NotImplementedError):
            call()


# ---- 7. it can be descended on --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_route", [False, True])
def test_a_level_of_detail_is_recovered_by_descent(dev, fused_route):
    """Field (64, 64), R = 4, 8, 16, 32 (fades 4, 3, 2, 1), F = 2, a table uniform in +- 0.5; 256 points, colours from query(p, lod = 1.25), a 0-dim
    lambda_hat from 2.0 - where the finest level sits exactly at its end and the next exactly at its start - by torch Adam (lr 0.02, 200 steps)
    through query_differentiable_lod.  Condition: |lambda_hat - 1.25| <= 0.075, a tenth of the initial 0.75.  The float64 reference's run of the
    same loop (CPU file): loss 2.2705e-04 -> 3.0377e-13, lambda_hat 1.25003, error 0.00003."""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    d = L.DESCENT
    geo, _, table, params, points = L.descent_inputs()
    f = HashGridField(d["size"], levels=4, features=d["features"], log2_table=d["log2_table"], base_resolution=4, finest_resolution=32, device=dev, seed=d["seed"],
                      fused=fused_route)
    assert f.resolutions == d["resolutions"] and f.lod_fade == (4.0, 3.0, 2.0, 1.0) and f.route == ("fused" if fused_route else "layerwise")
    with torch.no_grad():
        f.table.copy_(table.to(dev))
        for dst, src in zip(f.decoder.linear_params(), params):
            dst.copy_(src.to(dev))
    first, last, lam = L.run_descent(f.query_differentiable_lod, points.to(dev), dev)
    err = abs(lam - d["lam0"])
    print(f"descent on lambda ({f.route}): loss {first:.4e} -> {last:.4e}, lambda_hat {lam:.5f}, error {err:.5f}")
    assert err <= 0.075, (first, last, lam)
