"""GPU tests of the gradients with respect to the point coordinates (nic_hash_encode_points_grad / nic_hash_fused_points_grad,
csrc/hashgrid_pointgrad.hip; HashGridField.point_gradient / jacobian / query_differentiable).  The oracle is a float64 torch
restatement of the definition in include/nicv2_hip.h, written here: integer t and v, the fp32 weight w, the analytic signed-weight sum over the
corners, and an erf-GELU / sigmoid decoder in float64.

1. the row gradient against the oracle within 1e-5 of its largest magnitude (TOL_ORDER: the same sums in another order), dim 2 / 3, F 1 / 2 /
   4 / 8, all three sources, short launches;
2. an independent check that restates no formula: where the row is exactly affine along an axis, the central difference of hash_encode_points
   equals dpoints within 1e-4 (TOL_G);
3. a clamped axis is exactly 0.0 and the other axes are those of the clamped point, bit for bit;
4. level of detail: lambda = 0 is the plain entry bit for bit, lambda > 0 against the oracle, a faded level is not gathered;
5. the fused entry against the layer-wise composition (y within 5e-6, dpoints within 1e-4) and against the oracle end to end;
6. the surface: query_differentiable, jacobian, load_compressed fields, nothing of the field's training state moves;
7. it can be descended on: a shift recovered by torch Adam on the positions."""
import copy

import pytest
import torch

from test_gpu_hashgrid_points import _geo, _geo_for, _odd_points, _table, clamp_points, fixed_points

pytestmark = pytest.mark.gpu

M32 = (1 << 32) - 1
TOL_ORDER, TOL_G, TOL_Y = 1e-5, 1e-4, 5e-6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- the definition, restated in float64 (device-agnostic: test 7's figures come from this code on the CPU) -----------------------------------
def level_weights(fade, lod, lod_uniform, n, device):
    """[N, L] float64: a_l = min(max((fade[l] - lambda) + 1, 0), 1) in fp32, lambda = (lod or 0) + lod_uniform, NaN -> 0, clamped to [0, 32]"""
    lam = (torch.zeros(n, dtype=torch.float32, device=device) if lod is None else lod.float()) + torch.tensor(lod_uniform, dtype=torch.float32, device=device)
    lam = torch.where(lam == lam, lam, torch.zeros_like(lam)).clamp(0.0, 32.0)
    f = torch.tensor(list(fade), dtype=torch.float32, device=device)
    return ((f[None, :] - lam[:, None]) + 1.0).clamp(0.0, 1.0).double()


def oracle_row_jacobian(values, field_size, resolutions, log2_table, points, weights=None):
    """row [N, L F] and d row / d p [N, L F, dim] in float64 from ``values`` [L, T, F] (what the forward blends) at fp32 ``points``:
    t and v in int64, w = fp32(q mod 256 S_max) / fp32(256 S_max), the blend and the signed-weight sum in float64, a clamped axis 0"""
    dim, T = len(field_size), 1 << log2_table
    s_max = max(field_size)
    D = 256 * s_max
    values = values.double()
    t = fixed_points(points, field_size)
    hi = torch.tensor([float(s) - 0.5 for s in field_size], dtype=torch.float32, device=points.device)
    kept = ((points >= -0.5) & (points <= hi)).double()
    rows, jacs = [], []
    for l, R in enumerate(resolutions):
        q = t * R
        v = q // D
        w = ((q % D).float() / torch.tensor(float(D), dtype=torch.float32, device=points.device)).double()
        dense = (R + 1) ** dim <= T
        row, jac = 0, [0] * dim
        for c in range(1 << dim):
            vc = [v[:, a] + ((c >> a) & 1) for a in range(dim)] + [torch.zeros_like(v[:, 0])] * (3 - dim)
            if dense:
                h = vc[0] + (R + 1) * (vc[1] + (R + 1) * vc[2])
            else:
                h = (vc[0] & M32) ^ ((vc[1] * 2654435761) & M32) ^ ((vc[2] * 805459861) & M32)
            val = values[l][h & (T - 1)]
            cw = [w[:, a] if (c >> a) & 1 else 1 - w[:, a] for a in range(dim)]
            full = torch.ones_like(w[:, 0])
            for a in range(dim):
                full = full * cw[a]
            row = row + full[:, None] * val
            for a in range(dim):
                sw = torch.full_like(w[:, 0], 1.0 if (c >> a) & 1 else -1.0)
                for b in range(dim):
                    if b != a:
                        sw = sw * cw[b]
                jac[a] = jac[a] + sw[:, None] * val
        al = 1.0 if weights is None else weights[:, l][:, None]
        rows.append(al * row)
        jacs.append(torch.stack([al * (R / s_max) * jac[a] * kept[:, a][:, None] for a in range(dim)], dim=2))
    return torch.cat(rows, dim=1), torch.cat(jacs, dim=1)


def oracle_decoder(x, params):
    w1, b1, w2, b2, w3, b3 = [p.detach().double() for p in params]
    h = torch.nn.functional.gelu(x @ w1.T + b1)
    h = torch.nn.functional.gelu(h @ w2.T + b2)
    return torch.sigmoid(h @ w3.T + b3)


def oracle_point_gradient(values, geo, points, params, dy=None, target=None, scale=1.0, weights=None):
    """(y, dpoints) in float64, end to end"""
    row, jac = oracle_row_jacobian(values, geo.field_size, geo.resolutions, geo.log2_table, points, weights)
    with torch.enable_grad():                                                    # also when called from an autograd backward
        row = row.detach().requires_grad_(True)
        y = oracle_decoder(row, params)
        g = dy.double() if dy is not None else (y.detach() - target.double()) * (2.0 * scale / (3.0 * points.shape[0]))
        dx, = torch.autograd.grad(y, row, g)
    return y.detach(), torch.einsum("nk,nka->na", dx, jac)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


# ---- the sources ------------------------------------------------------------------------------------------------------------------------------
SOURCES = [("f32", None), ("u8", 8), ("u8", 5), ("bits", 4), ("bits", 5)]          # packed: b = 4 tight, b = 5 straddling


def _source(geo, dev, kind, bits, seed):
    """(data, kind, num_bits, the fp32 [L, T, F] values the forward blends)"""
    from neural_image_compression_v2_amd import hashgrid as hg
    from neural_image_compression_v2_amd import models
    if kind == "f32":
        table = _table(geo, dev, seed, 0.45)
        return table, kind, None, table
    clamped = models.quantize_clamp(_table(geo, dev, seed, 0.45), bits)
    stored = hg.hash_pack_u8(geo, clamped, bits)
    data = stored if kind == "u8" else hg.hash_pack_bits(geo, clamped, bits)
    return data, kind, bits, hg._table_of_u8(geo, stored, bits)


def _decoder(geo, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    def u(*shape, amp):
        return ((torch.rand(*shape, generator=g, device=dev) * 2 - 1) * amp).contiguous()
    k1, k2 = geo.width ** -0.5, 64 ** -0.5
    return [u(64, geo.width, amp=3 * k1), u(64, amp=k1), u(64, 64, amp=2 * k2), u(64, amp=k2), u(3, 64, amp=2 * k2), u(3, amp=k2)]


def _compose(geo, data, kind, bits, pts, params, dy=None, target=None, scale=1.0, lod=None):
    """the layer-wise composition: encode -> general decoder -> its backward to the row -> nic_hash_encode_points_grad"""
    from neural_image_compression_v2_amd import fused
    from neural_image_compression_v2_amd import hashgrid as hg
    lod_kw = {} if lod is None else dict(lod=lod[0], lod_uniform=lod[1], fade=lod[2])
    x = hg.hash_encode_points(geo, data, pts, kind, bits) if lod is None else hg.hash_encode_points_lod(geo, data, pts, kind=kind, num_bits=bits, **lod_kw)
    x.requires_grad_(True)
    y = fused.DecoderFunction.apply(x, *params)
    g = dy if dy is not None else (y.detach() - target) * (2.0 * scale / (3.0 * pts.shape[0]))
    dx, = torch.autograd.grad(y, x, g)
    return y.detach(), hg.hash_encode_points_grad(geo, data, pts, dx, kind, bits, **lod_kw)


# ---- 1. the row gradient against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("dim", [2, 3])
def test_row_gradient_against_the_oracle(dev, dim, F):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _geo_for(dim, F)
    pts = _odd_points(geo, dev, seed=10 * dim + F, n=3000)
    n = pts.shape[0]
    dx = torch.rand(n, geo.width, generator=torch.Generator(device=dev).manual_seed(F), device=dev) * 2 - 1
    for kind, bits in SOURCES:
        data, kind, bits, values = _source(geo, dev, kind, bits, seed=dim + F)
        _, jac = oracle_row_jacobian(values, geo.field_size, geo.resolutions, geo.log2_table, pts)
        want = torch.einsum("nk,nka->na", dx.double(), jac)
        got = hg.hash_encode_points_grad(geo, data, pts, dx, kind, bits)
        assert got.shape == (n, dim) and bool(torch.isfinite(got).all())
        e = float((got.double() - want).abs().max() / want.abs().max())
        print(f"row gradient {dim}D F={F} {kind} b={bits}: {e:.3e} of {float(want.abs().max()):.3e}")
        assert e < TOL_ORDER, (kind, bits, e)
        for m in (1, 63, 65):                                                    # part of a wave, one lane short of one, one lane into the next
            short = hg.hash_encode_points_grad(geo, data, pts[:m].contiguous(), dx[:m].contiguous(), kind, bits)
            assert float((short.double() - want[:m]).abs().max() / want.abs().max()) < TOL_ORDER, (kind, bits, m)
    assert hg.hash_encode_points_grad(geo, data, pts[:0].contiguous(), dx[:0].contiguous(), kind, bits).shape == (0, dim)


# ---- 2. an independent check: central differences where the row is affine ---------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_central_differences_where_the_row_is_affine(dev, dim):
    """p_a = 8 k + 3.5 + u, u a multiple of 1/256 in [-2, 2]: p +- 1 stays inside one cell of both levels (cells 16 and 8 samples wide), so the
    row is exactly affine along every axis and (row(p + e_a) - row(p - e_a)) / 2 is its derivative - no formula of the kernel is restated"""
    from neural_image_compression_v2_amd import hashgrid as hg
    from neural_image_compression_v2_amd.hashgrid import HashGeometry
    size, res = ((64, 64), (4, 8)) if dim == 2 else ((32, 32, 32), (2, 4))
    geo = HashGeometry(size, res, 2, 12)
    table = _table(geo, dev, 3, 0.5)
    g = torch.Generator(device=dev).manual_seed(dim)
    n = 2000
    k = torch.randint(0, size[0] // 8, (n, dim), generator=g, device=dev)
    u = torch.randint(-512, 513, (n, dim), generator=g, device=dev)
    pts = (8.0 * k + 3.5 + u / 256.0).float().contiguous()
    dx = torch.rand(n, geo.width, generator=g, device=dev) * 2 - 1
    got = hg.hash_encode_points_grad(geo, table, pts, dx)
    want = torch.empty(n, dim, dtype=torch.float64, device=dev)
    for a in range(dim):
        e = torch.zeros(dim, device=dev)
        e[a] = 1.0
        up, down = hg.hash_encode_points(geo, table, (pts + e).contiguous()), hg.hash_encode_points(geo, table, (pts - e).contiguous())
        want[:, a] = (dx.double() * (up.double() - down.double()) / 2).sum(dim=1)
    err = float((got.double() - want).abs().max() / want.abs().max())
    print(f"central differences {dim}D: {err:.3e} of {float(want.abs().max()):.3e}")
    assert err < TOL_G, err
    assert float(want.abs().max()) > 1e-2                                        # the check is not vacuous


# ---- 3. clamped axes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_clamped_axes_are_zero_and_the_others_the_clamped_points(dev, dim):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _geo_for(dim, 2)
    pts = _odd_points(geo, dev, seed=dim, n=500)
    inside = clamp_points(pts, geo.field_size).contiguous()
    moved = ~(inside == pts)                                                     # NaN included
    assert bool(moved.any()) and int(moved.all(dim=1).sum()) >= 3 and int((moved.any(dim=1) & ~moved.all(dim=1)).sum()) >= 10
    dx = torch.rand(pts.shape[0], geo.width, generator=torch.Generator(device=dev).manual_seed(2), device=dev) + 0.5
    params = _decoder(geo, dev, 4)
    dy = torch.rand(pts.shape[0], 3, generator=torch.Generator(device=dev).manual_seed(3), device=dev) + 0.5
    for kind, bits in (("f32", None), ("bits", 5)):
        data, kind, bits, _ = _source(geo, dev, kind, bits, seed=7)
        for got, at_clamped in ((hg.hash_encode_points_grad(geo, data, pts, dx, kind, bits), hg.hash_encode_points_grad(geo, data, inside, dx, kind, bits)),
                                (hg.hash_fused_points_grad(geo, data, pts, params, dy=dy, kind=kind, num_bits=bits)[1],
                                 hg.hash_fused_points_grad(geo, data, inside, params, dy=dy, kind=kind, num_bits=bits)[1])):
            assert bool((got[moved] == 0).all()) and not bool(torch.signbit(got[moved]).any())
            assert torch.equal(got[~moved], at_clamped[~moved])
            assert bool((at_clamped[~moved] != 0).any()) and bool(torch.isfinite(got).all())
    top = torch.tensor([[float(s) - 0.5 for s in geo.field_size]], device=dev)  # p = S - 1/2 is not clamped: the last cell's derivative
    assert bool((hg.hash_encode_points_grad(geo, data, top, dx[:1].contiguous(), kind, bits) != 0).all())


# ---- 4. level of detail ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_level_of_detail(dev, dim):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _geo_for(dim, 2)
    fade = hg.hash_lod_fade(geo)
    pts = _odd_points(geo, dev, seed=20 + dim, n=3000)
    n = pts.shape[0]
    g = torch.Generator(device=dev).manual_seed(dim)
    dx = torch.rand(n, geo.width, generator=g, device=dev) * 2 - 1
    dy = torch.rand(n, 3, generator=g, device=dev) * 2 - 1
    params = _decoder(geo, dev, 5)
    data, kind, bits, values = _source(geo, dev, "f32", None, seed=9)
    plain = hg.hash_encode_points_grad(geo, data, pts, dx)
    plain_y, plain_f = hg.hash_fused_points_grad(geo, data, pts, params, dy=dy)
    # lambda = 0, uniform and per point: the plain entry bit for bit
    for kw in (dict(fade=fade), dict(lod=torch.zeros(n, device=dev))):
        assert torch.equal(hg.hash_encode_points_grad(geo, data, pts, dx, **kw), plain)
        y0, f0 = hg.hash_fused_points_grad(geo, data, pts, params, dy=dy, **kw)
        assert torch.equal(f0, plain_f) and torch.equal(y0, plain_y)
    # lambda > 0 against the oracle
    per_point = torch.rand(n, generator=g, device=dev) * 4.0
    per_point[:8] = torch.tensor([float("nan"), -1.0, 0.0, 4.0, 40.0, float("inf"), 1.0, 2.5], device=dev)
    for lod_t, lod_u in ((None, 1.5), (per_point, 0.0), (per_point, 0.75)):
        wts = level_weights(fade, lod_t, lod_u, n, dev)
        _, jac = oracle_row_jacobian(values, geo.field_size, geo.resolutions, geo.log2_table, pts, wts)
        want = torch.einsum("nk,nka->na", dx.double(), jac)
        got = hg.hash_encode_points_grad(geo, data, pts, dx, lod=lod_t, lod_uniform=lod_u)
        e = float((got.double() - want).abs().max() / want.abs().max())
        print(f"row gradient {dim}D with a level of detail ({'per point' if lod_t is not None else 'uniform'} + {lod_u}): {e:.3e}")
        assert e < TOL_ORDER, e
        y_o, want_f = oracle_point_gradient(values, geo, pts, params, dy=dy, weights=wts)
        y_f, got_f = hg.hash_fused_points_grad(geo, data, pts, params, dy=dy, lod=lod_t, lod_uniform=lod_u)
        e_y, e_f = float((y_f.double() - y_o).abs().max()), float((got_f.double() - want_f).abs().max() / want_f.abs().max())
        print(f"fused with a level of detail: y {e_y:.3e}, dpoints {e_f:.3e}")
        assert e_f < TOL_G, (e_y, e_f)
    # a faded level is not gathered: NaN in the levels lambda weighs 0 changes nothing
    for lam in (1.5, 3.0):
        off = [l for l, f in enumerate(fade) if (f - lam) + 1.0 <= 0.0]
        assert off and len(off) < geo.levels
        poisoned = data.clone()
        poisoned[off] = float("nan")
        a, b = hg.hash_encode_points_grad(geo, data, pts, dx, lod_uniform=lam), hg.hash_encode_points_grad(geo, poisoned, pts, dx, lod_uniform=lam)
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b), lam
        (ya, fa), (yb, fb) = (hg.hash_fused_points_grad(geo, t, pts, params, dy=dy, lod_uniform=lam) for t in (data, poisoned))
        assert bool(torch.isfinite(fb).all()) and torch.equal(fa, fb) and torch.equal(ya, yb), lam


# ---- 5. the fused entry against the layer-wise composition and the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 4, 8])                                           # L F = 16, 32 (one k tile), 64 (two)
@pytest.mark.parametrize("dim", [2, 3])
def test_fused_against_the_composition_and_the_oracle(dev, dim, F):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _geo_for(dim, F)
    assert geo.width == 8 * F and hg.hash_fused_supported(geo)
    pts = _odd_points(geo, dev, seed=30 + dim + F, n=3000)
    n = pts.shape[0]
    g = torch.Generator(device=dev).manual_seed(dim * F)
    dy = torch.rand(n, 3, generator=g, device=dev) * 2 - 1
    target = torch.rand(n, 3, generator=g, device=dev)
    params = _decoder(geo, dev, 6 + F)
    fade = hg.hash_lod_fade(geo)
    lod_t = torch.rand(n, generator=g, device=dev) * 4.0
    worst = {"y": 0.0, "g": 0.0, "oracle": 0.0}
    for kind, bits in SOURCES:
        data, kind, bits, values = _source(geo, dev, kind, bits, seed=dim + F)
        for mode in (dict(dy=dy), dict(target=target, scale=float(n))):           # scale n: dy = 2 (y - t) / 3, of the size of the dy mode's
            for lod in (None, (lod_t, 0.5, fade)):
                if lod is not None and (kind, bits) not in (("f32", None), ("bits", 5)):
                    continue
                fkw = {k if k != "scale" else "loss_scale": v for k, v in mode.items()}
                if lod is not None:
                    fkw.update(lod=lod[0], lod_uniform=lod[1], fade=lod[2])
                y_f, g_f = hg.hash_fused_points_grad(geo, data, pts, params, kind=kind, num_bits=bits, **fkw)
                y_c, g_c = _compose(geo, data, kind, bits, pts, params, lod=lod, **mode)
                wts = None if lod is None else level_weights(fade, lod[0], lod[1], n, dev)
                y_o, g_o = oracle_point_gradient(values, geo, pts, params, weights=wts, **mode)
                e_y, e_g, e_o = float((y_f - y_c).abs().max()), rel(g_f, g_c), rel(g_f, g_o)
                worst = {"y": max(worst["y"], e_y), "g": max(worst["g"], e_g), "oracle": max(worst["oracle"], e_o)}
                assert y_f.shape == (n, 3) and g_f.shape == (n, dim) and bool(torch.isfinite(g_f).all())
                worst["y_oracle"] = max(worst.get("y_oracle", 0.0), float((y_f.double() - y_o).abs().max()))
                assert e_y < TOL_Y and e_g < TOL_G and e_o < TOL_G, (kind, bits, list(mode), e_y, e_g, e_o)
                if lod is None and "dy" in mode:
                    for m in (1, 31, 33, 65):                                   # half tiles with and without a live sample, a ragged second wave
                        y_s, g_s = hg.hash_fused_points_grad(geo, data, pts[:m].contiguous(), params, dy=dy[:m].contiguous(), kind=kind, num_bits=bits)
                        assert float((y_s - y_c[:m]).abs().max()) < TOL_Y and float((g_s.double() - g_c[:m].double()).abs().max() / g_c.abs().max()) < TOL_G, m
                    bit_equal = torch.equal(y_f, hg.hash_fused_forward_points(geo, data, pts, params, kind, bits))
                    print(f"{dim}D F={F} {kind} b={bits}: y bit-equal to nic_hash_fused_forward_points: {bit_equal}")
                    none_y, g_n = hg.hash_fused_points_grad(geo, data, pts, params, dy=dy, want_y=False, kind=kind, num_bits=bits)
                    assert none_y is None and torch.equal(g_n, g_f)               # deterministic, with and without y
    print(f"fused {dim}D L F = {geo.width}: y against the composition {worst['y']:.3e}, dpoints {worst['g']:.3e}, dpoints against the oracle {worst['oracle']:.3e} "
          f"(y against the oracle {worst['y_oracle']:.3e}, not asserted)")
    y_e, g_e = hg.hash_fused_points_grad(geo, data, pts[:0].contiguous(), params, dy=dy[:0].contiguous(), kind=kind, num_bits=bits)
    assert y_e.shape == (0, 3) and g_e.shape == (0, dim)


# ---- 6. the surface -------------------------------------------------------------------------------------------------------------------------
def _field(size, dev, seed, fused=False, num_bits=None, **kw):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    kw = dict(dict(levels=8, features=2, log2_table=12), **kw)
    f = HashGridField(size, device=dev, seed=seed, num_bits=num_bits, fused=fused, **kw)
    with torch.no_grad():
        f.table.uniform_(-0.4, 0.4, generator=torch.Generator(device=dev).manual_seed(seed))
        for p in f.decoder.parameters():
            p.mul_(3.0)                                                          # a decoder that does something with its input
    return f


def _training_state(f):
    return (None if f.table is None else f.table.grad.clone(), [None if p.grad is None else p.grad.clone() for p in f.decoder.parameters()],
            copy.deepcopy(f.optimizer.state_dict()), f.steps, f._grad_clean, None if f.table is None else f.table.detach().clone(),
            [p.detach().clone() for p in f.decoder.parameters()])


def _same_state(a, b):
    def eq(x, y):
        return (x is None and y is None) or torch.equal(x, y)
    assert eq(a[0], b[0]) and all(eq(x, y) for x, y in zip(a[1], b[1])) and a[3:5] == b[3:5] and eq(a[5], b[5]) and all(eq(x, y) for x, y in zip(a[6], b[6]))
    sa, sb = a[2], b[2]
    assert sa["param_groups"] == sb["param_groups"] and sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        for name, v in sa["state"][k].items():
            w = sb["state"][k][name]
            assert torch.equal(v, w) if isinstance(v, torch.Tensor) else v == w, (k, name)


@pytest.mark.parametrize("fused_route", [False, True])
def test_the_surface(dev, fused_route, tmp_path):
    from neural_image_compression_v2_amd import hashgrid as hg
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    f = _field((200, 131), dev, 11, fused=fused_route, num_bits=6)
    assert f.route == ("fused" if fused_route else "layerwise")
    pts = _odd_points(f.geo, dev, seed=1, n=1000)
    n = pts.shape[0]
    g = torch.Generator(device=dev).manual_seed(1)
    dy, target = torch.rand(n, 3, generator=g, device=dev) * 2 - 1, torch.rand(n, 3, generator=g, device=dev)
    before = _training_state(f)
    y, dp = f.point_gradient(pts, dy=dy)
    assert torch.equal(y, f.query(pts)) or float((y - f.query(pts)).abs().max()) < TOL_Y
    # against the oracle, both modes, with and without a level of detail
    params = [p.detach() for p in f.decoder.linear_params()]
    for lod in (None, 1.25):
        wts = None if lod is None else level_weights(f.lod_fade, None, lod, n, dev)
        for mode in (dict(dy=dy), dict(target=target, scale=float(n))):
            y_g, dp_g = f.point_gradient(pts, lod=lod, **mode)
            y_o, dp_o = oracle_point_gradient(f.table.detach(), f.geo, pts, params, weights=wts, **mode)
            assert rel(dp_g, dp_o) < TOL_G, (lod, list(mode))
    # query_differentiable: point_gradient's dpoints bit for bit, through any torch graph on the positions
    for lod in (None, 1.25):
        leaf = pts.clone().requires_grad_(True)
        out = f.query_differentiable(leaf, lod=lod)
        assert out.requires_grad and torch.equal(out.detach(), f.query(pts, lod=lod))
        out.backward(dy)
        assert torch.equal(leaf.grad, f.point_gradient(pts, dy=dy, lod=lod)[1])
    shift = torch.zeros(2, device=dev, requires_grad=True)
    ((f.query_differentiable(pts + shift) - target) ** 2).mean().backward()
    terms = f.point_gradient((pts + shift).detach(), target=target)[1]
    # two fp32 sums of the same n terms in different orders: each within (n - 1) 2^-24 sum |term| < 1e-4 sum |term| of the exact sum
    assert float((shift.grad - terms.sum(dim=0)).abs().max()) <= 1e-4 * float(terms.abs().sum(dim=0).max())
    assert not f.query_differentiable(pts).requires_grad                         # nothing asks for a gradient: query itself
    # jacobian: three one-hot calls
    jac = f.jacobian(pts[:300].contiguous(), lod=0.5)
    assert jac.shape == (300, 3, 2)
    for o in range(3):
        hot = torch.zeros(300, 3, device=dev)
        hot[:, o] = 1.0
        assert torch.equal(jac[:, o], f.point_gradient(pts[:300].contiguous(), dy=hot, lod=0.5)[1])
    # nothing of the training state moved: no .grad, no optimiser state, no step count
    _same_state(before, _training_state(f))
    # HashEncodePointsFunction still returns nothing for its points
    leaf = pts.clone().requires_grad_(True)
    x = hg.HashEncodePointsFunction.apply(f.table, f.geo, leaf)
    grads = torch.autograd.grad(x.sum(), [f.table, leaf], allow_unused=True)
    assert grads[0] is not None and grads[1] is None
    # a field from load_compressed (uint8 and packed) answers point_gradient
    f.freeze()
    frozen = f.point_gradient(pts, dy=dy)
    for packed in (False, True):
        path = tmp_path / f"f{int(packed)}.pt"
        f.save_compressed(path, packed=packed)
        loaded = HashGridField.load_compressed(path, dev, fused=fused_route)
        assert loaded.table is None and loaded.route == f.route
        y_l, dp_l = loaded.point_gradient(pts, dy=dy)
        assert float((y_l - frozen[0]).abs().max()) < TOL_Y and rel(dp_l, frozen[1]) < TOL_G, packed
        assert bool((dp_l != 0).any()) and bool(torch.isfinite(dp_l).all())
        assert torch.equal(loaded.jacobian(pts[:10].contiguous())[:, 1], loaded.point_gradient(pts[:10].contiguous(), dy=torch.tensor([[0.0, 1.0, 0.0]] * 10, device=dev))[1])


# ---- 7. it can be descended on --------------------------------------------------------------------------------------------------------------
DESCENT = dict(size=(64, 64), steps=120, lr=0.05, delta=(1.25, -0.75), n=2000, seed=5)


def descent_table(geo, device):
    """entry of vertex x at level l: 0.5 sin / 0.5 cos of a fixed low frequency of its position in samples (all four levels are dense)"""
    table = torch.zeros(geo.table_shape(), dtype=torch.float64, device=device)
    for l, R in enumerate(geo.resolutions):
        assert (R + 1) ** 2 <= geo.table_size
        v = torch.arange(R + 1, dtype=torch.float64, device=device) * (geo.s_max / R)
        vx, vy = torch.meshgrid(v, v, indexing="ij")                             # entry vx + (R + 1) vy
        phase = 0.11 * vx + 0.07 * vy + 0.9 * l
        e = (torch.arange(R + 1, device=device)[:, None] + (R + 1) * torch.arange(R + 1, device=device)[None, :]).reshape(-1)
        table[l, e, 0] = (0.5 * torch.sin(phase)).reshape(-1)
        table[l, e, 1] = (0.5 * torch.cos(0.13 * vx - 0.05 * vy + 0.4 * l)).reshape(-1)
    return table


def descent_points(device):
    g = torch.Generator().manual_seed(DESCENT["seed"])
    return (torch.rand(DESCENT["n"], 2, generator=g) * 48.0 + 8.0).to(device)


def run_descent(query_with_grad, points, device):
    """the loop both the field and the oracle run: colours from query(p + delta), delta_hat from 0 by torch Adam; (first loss, last loss, delta_hat)"""
    delta = torch.tensor(DESCENT["delta"], dtype=points.dtype, device=device)
    with torch.no_grad():
        colours = query_with_grad(points + delta).detach()
    hat = torch.zeros(2, dtype=points.dtype, device=device, requires_grad=True)
    opt = torch.optim.Adam([hat], lr=DESCENT["lr"])
    losses = []
    for _ in range(DESCENT["steps"] + 1):
        opt.zero_grad()
        loss = ((query_with_grad(points + hat) - colours) ** 2).mean()
        losses.append(float(loss.detach()))
        if len(losses) <= DESCENT["steps"]:
            loss.backward()
            opt.step()
    return losses[0], losses[-1], hat.detach()


class OracleQuery(torch.autograd.Function):
    """the float64 oracle as the same differentiable op of the points (positions rounded to fp32 first, as the field receives them)"""

    @staticmethod
    def forward(ctx, points, values, geo, params):
        p32 = points.detach().float()
        row, jac = oracle_row_jacobian(values, geo.field_size, geo.resolutions, geo.log2_table, p32)
        ctx.geo, ctx.values, ctx.params = geo, values, params
        ctx.save_for_backward(p32)
        return oracle_decoder(row, params).to(points.dtype)

    @staticmethod
    def backward(ctx, dy):
        p32, = ctx.saved_tensors
        return oracle_point_gradient(ctx.values, ctx.geo, p32, ctx.params, dy=dy)[1].to(dy.dtype), None, None, None


def test_a_shift_is_recovered_by_descent_on_the_positions(dev):
    """Field (64, 64), four dense levels R = 4, 8, 16, 32, F = 2, the table a low-frequency sin / cos of the vertex position, the decoder at its
    seeded default init; 2000 points in [8, 56]^2, colours from query(p + (1.25, -0.75)), delta_hat from 0 by torch Adam (lr 0.05, 120 steps)
    through query_differentiable(p + delta_hat).  Conditions: final loss <= 0.1 of the initial loss, |delta_hat - delta|_inf <= 0.25 samples.
    The float64 oracle's run of the same loop on a CPU (OracleQuery above): loss 3.0764e-07 -> 2.5418e-12 (ratio 8.3e-06), delta_hat
    (1.25254, -0.75268), error 0.0027 samples - both conditions with far more than a factor 2 to spare (200 steps: ratio 1.7e-07, error 0.0001)."""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    f = HashGridField(DESCENT["size"], levels=4, features=2, log2_table=12, base_resolution=4, finest_resolution=32, device=dev, seed=DESCENT["seed"])
    assert f.resolutions == (4, 8, 16, 32) and f.route == "layerwise"
    with torch.no_grad():
        f.table.copy_(descent_table(f.geo, dev).float())
    first, last, hat = run_descent(f.query_differentiable, descent_points(dev), dev)
    err = float((hat - torch.tensor(DESCENT["delta"], device=dev)).abs().max())
    print(f"descent: loss {first:.4e} -> {last:.4e} (ratio {last / first:.3e}), delta_hat {hat.tolist()}, error {err:.4f} samples")
    assert last <= 0.1 * first and err <= 0.25, (first, last, err)
