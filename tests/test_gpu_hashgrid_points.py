"""GPU tests of the hash-grid field at arbitrary points (nic_hash_encode_points / _backward / nic_hash_fused_forward_points, csrc/hash_points.hip;
HashGridField.query / resample / train_points).  The semantics of include/nicv2_hip.h are restated here in torch, independently of the kernels:
the fixed-point position in int64, the cell in int64, weights and sums in float64, the backward by autograd through the gathers.

1. sample centres give the rows of hash_encode / _u8 / _bits / _noisy bit for bit, in raster order and permuted;
2. off-lattice, edge, outside, NaN and infinite points: forward within 1e-6 of the largest magnitude, backward within 1e-5 of the largest gradient
   entry (the tolerances of tests/test_gpu_hashgrid.py for the same arithmetic), finite, and clamped exactly;
3. the backward adds, leaves untouched entries alone, sums coinciding points, and does not depend on the point order beyond 1e-5;
4. the fused query against the layer-wise one within 5e-6, all three table sources, 2D and 3D;
5. resample at the field size against decode() within 5e-6, a 2x resample against the restatement through the same decoder within 1e-6;
6. a stored file (uint8 and packed) answers query() exactly like the frozen field, in a fresh process too;
7. train_points on a crop's centres against train_step on the crop within 1e-5 of the largest update, with noise, and in accumulate chunks."""
import copy
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- the semantics, restated ---------------------------------------------------------------------------------------------------------------
def clamp_points(points, field_size):
    """fp32 [N, d]: NaN -> the low edge, everything else into [-1/2, S_a - 1/2]"""
    lo = torch.full((len(field_size),), -0.5, dtype=torch.float32, device=points.device)
    hi = torch.tensor([float(s) - 0.5 for s in field_size], dtype=torch.float32, device=points.device)
    p = torch.where(points >= lo, points, lo)
    return torch.where(p <= hi, p, hi)


def fixed_points(points, field_size):
    """int64 [N, d]: t = rint(256 p) + 128 (half to even; 256 p is exact in fp32), clamped to [0, 256 S_a - 1]"""
    t = torch.round(clamp_points(points, field_size) * 256.0).to(torch.int64) + 128
    top = torch.tensor([256 * int(s) - 1 for s in field_size], dtype=torch.int64, device=points.device)
    return torch.minimum(torch.clamp(t, min=0), top)


def ref_encode_points(table, field_size, resolutions, log2_table, points):
    """int64 cell math, float64 weights and sums; differentiable w.r.t. ``table`` [L, T, F] (float64).  w = fp32(q mod D) / fp32(D), D = 256 S_max"""
    dim, T = len(field_size), 1 << log2_table
    D = 256 * max(field_size)
    t = fixed_points(points, field_size)
    cols = []
    for l, R in enumerate(resolutions):
        q = t * R
        v, w = q // D, (q % D).float().double() / D
        assert int(v.max()) <= R - 1                                            # corner v + 1 never leaves the level
        dense = (R + 1) ** dim <= T
        acc = 0
        for c in range(1 << dim):
            vc = [v[:, a] + ((c >> a) & 1) for a in range(dim)] + [torch.zeros_like(v[:, 0])] * (3 - dim)
            if dense:
                h = vc[0] + (R + 1) * (vc[1] + (R + 1) * vc[2])
            else:
                h = (vc[0] & M32) ^ ((vc[1] * 2654435761) & M32) ^ ((vc[2] * 805459861) & M32)
            h = h & (T - 1)
            cw = torch.ones_like(w[:, 0])
            for a in range(dim):
                cw = cw * (w[:, a] if (c >> a) & 1 else 1 - w[:, a])
            acc = acc + cw[:, None] * table[l][h]
        cols.append(acc)
    return torch.cat(cols, dim=1)


def centres(extent, dev, origin=None):
    """fp32 [N, d] sample centres of a crop in nic_encode order (the last axis fastest)"""
    origin = [0] * len(extent) if origin is None else origin
    grids = torch.meshgrid(*[torch.arange(int(o), int(o) + int(e), device=dev) for o, e in zip(origin, extent)], indexing="ij")
    return torch.stack([g.reshape(-1) for g in grids], dim=1).to(torch.float32).contiguous()


def _geo(field_size, levels, F, log2_table, n_min=16):
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, level_resolutions
    return HashGeometry(tuple(field_size), tuple(level_resolutions(levels, n_min, max(field_size))), F, log2_table)


def _geo_for(dim, F, log2_table=12):
    """coarse levels dense, fine ones hashed; non-square, not a power of two"""
    geo = _geo((200, 131), 8, F, log2_table) if dim == 2 else _geo((40, 27, 33), 8, F, log2_table, n_min=4)
    kinds = {(r + 1) ** dim <= (1 << log2_table) for r in geo.resolutions}
    assert kinds == {True, False}
    return geo


def _table(geo, dev, seed, amp=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand(geo.table_shape(), generator=g, device=dev) * 2 - 1) * amp


def _odd_points(geo, dev, seed, n=5000):
    """random fractional points over the whole field, then both edges, points outside, huge, NaN and infinite coordinates"""
    g = torch.Generator(device=dev).manual_seed(seed)
    S = torch.tensor([float(s) for s in geo.field_size], device=dev)
    inside = torch.rand(n, geo.dim, generator=g, device=dev) * S - 0.5
    special = [-0.5, float("nan"), float("inf"), float("-inf"), -3.7, -1e30, 1e30, 0.0, 0.001953125, 0.00390625 * 1.5]
    rows = []
    for a in range(geo.dim):
        for val in special + [geo.field_size[a] - 0.5, geo.field_size[a] + 10.25, geo.field_size[a] - 0.5 - 2.0 ** -9, geo.field_size[a] - 1.0]:
            r = inside[len(rows) % n].clone()
            r[a] = val
            rows.append(r)
    rows.append(torch.full((geo.dim,), float("nan"), device=dev))
    rows.append(torch.full((geo.dim,), float("inf"), device=dev))
    rows.append(torch.full((geo.dim,), float("-inf"), device=dev))
    rows.append(S - 0.5)
    rows.append(torch.full((geo.dim,), -0.5, device=dev))
    return torch.cat([inside, torch.stack(rows)], dim=0).contiguous()


# ---- 1. sample centres: the lattice rows, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("dim", [2, 3])
def test_centres_equal_the_lattice_rows(dev, dim, F):
    from neural_image_compression_v2_amd import hashgrid as hg
    from neural_image_compression_v2_amd import models
    geo = _geo_for(dim, F)
    size, org = geo.field_size, [[0] * dim]
    table = _table(geo, dev, 10 * dim + F)
    pts = centres(size, dev)
    perm = torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(F)).to(dev)
    want = hg.hash_encode(geo, table, org, size)
    assert torch.equal(hg.hash_encode_points(geo, table, pts), want)
    assert torch.equal(hg.hash_encode_points(geo, table, pts[perm].contiguous()), want[perm])
    for b in (8, 3):                                                             # F b = 3 F straddles dwords, 8 F does not
        clamped = models.quantize_clamp(table * 0.45, b)
        stored, packed = hg.hash_pack_u8(geo, clamped, b), hg.hash_pack_bits(geo, clamped, b)
        want_u8 = hg.hash_encode_u8(geo, stored, org, size, b)
        assert torch.equal(hg.hash_encode_bits(geo, packed, org, size, b), want_u8)
        assert torch.equal(hg.hash_encode_points(geo, stored, pts, "u8", b), want_u8)
        assert torch.equal(hg.hash_encode_points(geo, packed, pts, "bits", b), want_u8)
        assert torch.equal(hg.hash_encode_points(geo, stored, pts[perm].contiguous(), "u8", b), want_u8[perm])
        assert torch.equal(hg.hash_encode_points(geo, packed, pts[perm].contiguous(), "bits", b), want_u8[perm])
    # noise: the keys are (seed, offset, sample_base + row, column), so raster order with the same sample_base gives the same rows
    want_n = hg.hash_encode_noisy(geo, table, org, size, 6, seed=77, offset=5, sample_base=12345)
    assert not torch.equal(want_n, want)
    assert torch.equal(hg.hash_encode_points(geo, table, pts, quant=(6, 77, 5, 12345)), want_n)


def test_centres_of_a_crop_inside_a_larger_field(dev):
    """S_x != S_y = S_max and a crop away from the origin: the divisor is 256 S_max on every axis"""
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _geo((131, 200), 8, 2, 12)
    table = _table(geo, dev, 3)
    want = hg.hash_encode(geo, table, [[131 - 37, 200 - 21]], (37, 21))
    assert torch.equal(hg.hash_encode_points(geo, table, centres((37, 21), dev, [131 - 37, 200 - 21])), want)


# ---- 2. off the lattice ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("dim", [2, 3])
def test_off_lattice_forward_backward(dev, dim, F):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _geo_for(dim, F)
    table = _table(geo, dev, 20 * dim + F)
    pts = _odd_points(geo, dev, seed=dim * 7 + F)
    out = hg.hash_encode_points(geo, table, pts)
    assert bool(torch.isfinite(out).all())
    t64 = table.double().requires_grad_(True)
    ref = ref_encode_points(t64, geo.field_size, geo.resolutions, geo.log2_table, pts)
    assert out.shape == ref.shape
    e = float((out.double() - ref.detach()).abs().max() / ref.detach().abs().max())
    print(f"points forward {dim}D F={F}: {e:.3e}")
    assert e < 1e-6, (geo, e)
    # a point outside the field (or not finite) gives exactly the row of the clamped point
    assert torch.equal(hg.hash_encode_points(geo, table, clamp_points(pts, geo.field_size).contiguous()), out)
    g = torch.Generator(device=dev).manual_seed(99)
    dx = torch.rand(out.shape, generator=g, device=dev) * 2 - 1
    ref.backward(dx.double())
    base = torch.rand(geo.table_shape(), generator=g, device=dev)                # the call ADDS to what is there
    grad = base.clone()
    hg.hash_encode_points_backward(geo, pts, dx, grad)
    torch.cuda.synchronize()
    gref = t64.grad
    eb = float(((grad.double() - base.double()) - gref).abs().max() / gref.abs().max())
    print(f"points backward {dim}D F={F}: {eb:.3e}")
    assert eb < 1e-5, (geo, eb)
    assert bool(torch.isfinite(grad).all())
    # the autograd Function is that backward into a zero buffer
    tq = table.clone().requires_grad_(True)
    hg.hash_encode_points_differentiable(geo, tq, pts).backward(dx)
    assert float((tq.grad.double() - gref).abs().max() / gref.abs().max()) < 1e-5


def test_off_lattice_from_the_stored_tables(dev):
    """the uint8 and the packed source off the lattice: bit for bit the fp32 route on the dequantised table; 3D, dense levels read to their last entry"""
    from neural_image_compression_v2_amd import hashgrid as hg
    from neural_image_compression_v2_amd import models
    for dim, F, b in ((2, 2, 8), (3, 4, 5), (2, 8, 3), (3, 1, 1)):
        geo = _geo_for(dim, F)
        clamped = models.quantize_clamp(_table(geo, dev, dim + F + b, 0.45), b)
        stored, packed = hg.hash_pack_u8(geo, clamped, b), hg.hash_pack_bits(geo, clamped, b)
        pts = _odd_points(geo, dev, seed=b)
        want = hg.hash_encode_points(geo, hg._table_of_u8(geo, stored, b), pts)
        assert torch.equal(hg.hash_encode_points(geo, stored, pts, "u8", b), want), (dim, F, b)
        assert torch.equal(hg.hash_encode_points(geo, packed, pts, "bits", b), want), (dim, F, b)


# ---- 3. the backward ---------------------------------------------------------------------------------------------------------------------
def test_backward_adds_and_leaves_untouched_entries_alone(dev):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _geo((200, 131), 8, 2, 19)
    g = torch.Generator(device=dev).manual_seed(4)
    pts = (torch.rand(3000, 2, generator=g, device=dev) * torch.tensor([60.0, 40.0], device=dev) + 20.25).contiguous()    # a corner of the field
    dx = torch.rand(3000, geo.width, generator=g, device=dev) + 0.5              # positive: a touched entry moves
    touched = torch.zeros(geo.table_shape(), dtype=torch.float64, device=dev).requires_grad_(True)
    ref_encode_points(touched, geo.field_size, geo.resolutions, geo.log2_table, pts).backward(dx.double())
    untouched = touched.grad == 0
    assert bool(untouched.any()) and not bool(untouched.all())
    base = torch.rand(geo.table_shape(), generator=g, device=dev)
    grad = base.clone()
    hg.hash_encode_points_backward(geo, pts, dx, grad)
    assert torch.equal(grad[untouched], base[untouched])
    assert bool((grad[~untouched] != base[~untouched]).any())
    assert float(((grad.double() - base.double()) - touched.grad).abs().max() / touched.grad.abs().max()) < 1e-5
    twice = grad.clone()
    hg.hash_encode_points_backward(geo, pts, dx, twice)                         # a second call adds the same again
    assert float(((twice.double() - grad.double()) - touched.grad).abs().max() / touched.grad.abs().max()) < 1e-5


@pytest.mark.parametrize("dim", [2, 3])
def test_backward_of_coinciding_points(dev, dim):
    """every point the same: each wave is one run, the sum must still be right (and with a second point mixed in, runs of two kinds)"""
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _geo_for(dim, 2)
    one = torch.tensor([17.3, 101.77, 5.5][:dim], device=dev)
    for n, mixed in ((1000, False), (777, True)):
        pts = one.repeat(n, 1)
        if mixed:
            pts[100:350] = torch.tensor([3.25, 8.0, 30.125][:dim], device=dev)
        pts = pts.contiguous()
        g = torch.Generator(device=dev).manual_seed(n)
        dx = torch.rand(n, geo.width, generator=g, device=dev)
        t64 = torch.zeros(geo.table_shape(), dtype=torch.float64, device=dev).requires_grad_(True)
        ref_encode_points(t64, geo.field_size, geo.resolutions, geo.log2_table, pts).backward(dx.double())
        grad = torch.zeros(geo.table_shape(), device=dev)
        hg.hash_encode_points_backward(geo, pts, dx, grad)
        e = float((grad.double() - t64.grad).abs().max() / t64.grad.abs().max())
        assert e < 1e-5, (dim, n, e)
        assert torch.equal(grad == 0, t64.grad == 0)


def test_backward_sorted_and_shuffled_orders_agree(dev):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _geo((200, 131), 8, 2, 12)
    pts = centres(geo.field_size, dev) + 0.3                                     # raster order: long runs at the coarse levels
    g = torch.Generator(device=dev).manual_seed(8)
    dx = torch.rand(pts.shape[0], geo.width, generator=g, device=dev) * 2 - 1
    perm = torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(1)).to(dev)
    a, b = torch.zeros(geo.table_shape(), device=dev), torch.zeros(geo.table_shape(), device=dev)
    hg.hash_encode_points_backward(geo, pts.contiguous(), dx, a)
    hg.hash_encode_points_backward(geo, pts[perm].contiguous(), dx[perm].contiguous(), b)
    e = float((a.double() - b.double()).abs().max() / a.double().abs().max())
    print(f"sorted against shuffled: {e:.3e}")
    assert e < 1e-5, e


def test_empty_point_set(dev):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _geo((64, 64), 4, 2, 12)
    table = _table(geo, dev, 1)
    none = torch.empty(0, 2, device=dev)
    assert hg.hash_encode_points(geo, table, none).shape == (0, geo.width)
    grad = torch.ones(geo.table_shape(), device=dev)
    hg.hash_encode_points_backward(geo, none, torch.empty(0, geo.width, device=dev), grad)
    assert bool((grad == 1).all())


# ---- 4. fused query against layer-wise query ----------------------------------------------------------------------------------------------
def _field(size, dev, seed, fused=False, num_bits=None, **kw):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    kw = dict(dict(levels=8, features=2, log2_table=12), **kw)
    f = HashGridField(size, device=dev, seed=seed, num_bits=num_bits, fused=fused, **kw)
    with torch.no_grad():
        f.table.uniform_(-0.4, 0.4, generator=torch.Generator(device=dev).manual_seed(seed))
    return f


def _twin(f, fused=False):
    """a deep copy of a trainable field: its own table, decoder and optimiser state with the same values and step counts, on the asked route"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    g = HashGridField(f.field_size, levels=f.geo.levels, features=f.geo.features, log2_table=f.geo.log2_table, hidden=f.hidden, n_linear=f.n_linear,
                      device=f.device, num_bits=f.num_bits, noise_seed=f.noise_seed)
    assert not f.frozen and g.geo.table_shape() == f.geo.table_shape()
    g.geo = f.geo
    g._set_route(fused)
    with torch.no_grad():
        g.table.copy_(f.table)
    g.decoder.load_state_dict(copy.deepcopy(f.decoder.state_dict()))
    g.optimizer.load_state_dict(copy.deepcopy(f.optimizer.state_dict()))
    g.steps = f.steps
    return g


@pytest.mark.parametrize("dim", [2, 3])
def test_fused_query_against_layerwise_query(dev, dim, tmp_path):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (200, 131) if dim == 2 else (40, 27, 33)
    kw = dict(base_resolution=16 if dim == 2 else 4)
    layer = _field(size, dev, 5, num_bits=6, **kw)
    both = _twin(layer, fused=True)
    assert layer.route == "layerwise" and both.route == "fused"
    pts = _odd_points(layer.geo, dev, seed=dim, n=4099)                          # not a multiple of 64: the last wave is ragged
    y_l, y_f = layer.query(pts), both.query(pts)
    assert y_l.shape == y_f.shape == (pts.shape[0], 3)
    e = float((y_l - y_f).abs().max())
    print(f"fused query {dim}D fp32 table: {e:.3e}")
    assert e < 5e-6, e
    assert bool(torch.isfinite(y_f).all())
    for n in (1, 63, 64, 65, 257):                                               # short launches: part of one wave, one wave, two, five
        assert float((layer.query(pts[:n].contiguous()) - both.query(pts[:n].contiguous())).abs().max()) < 5e-6, n
    assert both.query(torch.empty(0, dim, device=dev)).shape == (0, 3) == layer.query(torch.empty(0, dim, device=dev)).shape
    layer.freeze()
    for packed in (False, True):
        path = tmp_path / f"f{int(packed)}.pt"
        layer.save_compressed(path, packed=packed)
        a, b = HashGridField.load_compressed(path, dev), HashGridField.load_compressed(path, dev, fused=True)
        assert a.table is None and b.table is None and b.route == "fused"
        e = float((a.query(pts) - b.query(pts)).abs().max())
        print(f"fused query {dim}D {'packed' if packed else 'uint8'} table: {e:.3e}")
        assert e < 5e-6, (packed, e)


# ---- 5. resample -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_route", [False, True])
def test_resample_at_the_field_size_is_decode(dev, fused_route):
    for size, kw in (((200, 131), {}), ((40, 27, 33), dict(base_resolution=4))):
        f = _field(size, dev, 6, fused=fused_route, **kw)
        e = float((f.resample(size, tile=64) - f.decode()).abs().max())
        assert e < 5e-6, (size, e)
        assert f.resample(size[0]).shape == (*([size[0]] * len(size)), 3)


def test_resample_2x_against_the_restatement(dev):
    from neural_image_compression_v2_amd import fused
    for size, kw in (((200, 131), {}), ((40, 27, 33), dict(base_resolution=4))):
        f = _field(size, dev, 7, **kw)
        big = tuple(2 * s for s in size)
        got = f.resample(big, tile=96)
        assert got.shape == (*big, 3)
        axes = [((torch.arange(n, dtype=torch.float64, device=dev) + 0.5) * s / n - 0.5).float() for s, n in zip(size, big)]
        pts = torch.stack([g.reshape(-1) for g in torch.meshgrid(*axes, indexing="ij")], dim=1).contiguous()
        assert float(pts.min()) == -0.25 and float(pts[:, 0].max()) == size[0] - 0.75
        x = ref_encode_points(f.table.detach().double(), size, f.geo.resolutions, f.geo.log2_table, pts).float()
        with torch.no_grad():
            want = fused.DecoderFunction.apply(x, *[p.detach() for p in f.decoder.linear_params()]).reshape(*big, 3)
        e = float((got - want).abs().max())
        print(f"2x resample {len(size)}D: {e:.3e}")
        assert e < 1e-6, (size, e)
    # a non-integer ratio, smaller than the field
    f = _field((200, 131), dev, 7)
    assert f.resample((77, 50)).shape == (77, 50, 3)


# ---- 6. stored files ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_route", [False, True])
def test_stored_file_answers_query_like_the_frozen_field(dev, fused_route, tmp_path):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    for size, kw, b in (((96, 80), {}, 6), ((40, 27, 33), dict(base_resolution=4), 3)):
        f = _field(size, dev, 8, fused=fused_route, num_bits=b, **kw)
        f.freeze()
        pts = _odd_points(f.geo, dev, seed=3, n=3001)
        want = f.query(pts)
        for packed in (False, True):
            path = tmp_path / f"s{len(size)}{int(packed)}.pt"
            f.save_compressed(path, packed=packed)
            g = HashGridField.load_compressed(path, dev, fused=fused_route)
            assert g.table is None and (g.packed is not None) == packed and g.route == f.route
            assert torch.equal(g.query(pts), want), (size, packed)
            assert g.table is None and (g.stored is None) == packed             # nothing was converted


def test_stored_file_answers_query_in_a_fresh_process(dev, tmp_path):
    f = _field((96, 80), dev, 9, fused=True, num_bits=5)
    f.freeze()
    pts = _odd_points(f.geo, dev, seed=4, n=2000)
    want = f.query(pts).cpu()
    torch.save(pts.cpu(), tmp_path / "pts.pt")
    for packed in (False, True):
        path, out = tmp_path / f"f{int(packed)}.pt", tmp_path / f"y{int(packed)}.pt"
        f.save_compressed(path, packed=packed)
        code = ("import sys, torch\n"
                f"sys.path.insert(0, {ROOT!r})\n"
                "from neural_image_compression_v2_amd.hashgrid import HashGridField\n"
                f"f = HashGridField.load_compressed({str(path)!r}, 'cuda:0', fused=True)\n"
                "assert f.route == 'fused' and f.table is None\n"
                f"pts = torch.load({str(tmp_path / 'pts.pt')!r}).to('cuda:0')\n"
                f"torch.save(f.query(pts).cpu(), {str(out)!r})\n")
        subprocess.run([sys.executable, "-c", code], check=True, timeout=300)
        assert torch.equal(torch.load(out), want), packed


# ---- 7. training -------------------------------------------------------------------------------------------------------------------------
def _image(size, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.linspace(0, 1, size[0], device=dev)[:, None]
    y = torch.linspace(0, 1, size[1], device=dev)[None, :]
    base = torch.stack([0.5 + 0.3 * torch.sin(7 * x + 3 * y), 0.5 + 0.3 * torch.cos(5 * x * y * 4), 0.5 + 0.2 * torch.sin(13 * y - 2 * x)], dim=-1)
    return (base + 0.05 * torch.rand(*size, 3, generator=g, device=dev)).clamp(0, 1)


def _compare_updates(a, b, before_table, before_dec, what):
    """a, b: two fields after the same step by different calls: table and decoder within 1e-5 of the largest update of either"""
    upd = float((a.table.detach() - before_table).abs().max())
    assert upd > 0
    e = float((a.table.detach() - b.table.detach()).abs().max()) / upd
    print(f"{what}: table {e:.3e} of the largest update {upd:.3e}")
    assert e < 1e-5, (what, e)
    for (pa, pb, p0) in zip(a.decoder.linear_params(), b.decoder.linear_params(), before_dec):
        u = float((pa.detach() - p0).abs().max())
        assert u > 0
        ed = float((pa.detach() - pb.detach()).abs().max()) / u
        print(f"{what}: decoder tensor {tuple(pa.shape)} {ed:.3e}")
        assert ed < 1e-5, (what, ed)


@pytest.mark.parametrize("num_bits", [None, 6])
@pytest.mark.parametrize("fused_route", [False, True])
def test_train_points_on_centres_is_train_step(dev, num_bits, fused_route):
    """two deep copies (``_twin``) of one field: train_step on a crop, train_points on that crop's centres - only the order of the atomics differs.  The
    first copy runs the layer-wise train_step; the second is layer-wise or fused (train_points takes the layer-wise route either way)."""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size, org, ext = (256, 192), [40, 24], (64, 48)
    image = _image(size, dev)
    base = HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=3, num_bits=num_bits)
    target = image[org[0]:org[0] + ext[0], org[1]:org[1] + ext[1]].reshape(-1, 3).contiguous()
    for _ in range(2):                                                           # off the symmetric start; the noise offset is no longer 0
        base.train_step([org], ext, target)
    a, b = _twin(base), _twin(base, fused=fused_route)
    assert a.route == "layerwise" and b.route == ("fused" if fused_route else "layerwise")
    t0, d0 = base.table.detach().clone(), [p.detach().clone() for p in base.decoder.linear_params()]
    la = a.train_step([org], ext, target)
    lb = b.train_points(centres(ext, dev, org), target)
    assert a.steps == b.steps == 3
    assert abs(float(la) - float(lb)) <= 1e-5 * abs(float(la)), (float(la), float(lb))
    _compare_updates(a, b, t0, d0, f"one step, num_bits {num_bits}")
    # a pass in accumulate chunks against the single call: the same samples, the same noise keys (sample_base = the samples before the chunk)
    c = _twin(base)
    pts = centres(ext, dev, org)
    n, cut = pts.shape[0], [0, 1000, 2048, pts.shape[0]]
    tot = 0.0
    for k in range(3):
        s = slice(cut[k], cut[k + 1])
        tot = tot + c.train_points(pts[s].contiguous(), target[s].contiguous(), accumulate=k > 0, scale=(cut[k + 1] - cut[k]) / n, step=k == 2)
    assert c.steps == 3
    assert abs(float(tot) - float(lb)) <= 1e-5 * abs(float(lb)), (float(tot), float(lb))
    _compare_updates(b, c, t0, d0, f"three chunks, num_bits {num_bits}")
    # the fused field goes on training on its own route afterwards
    if fused_route:
        b.train_step([org], ext, target)
        assert b.steps == 4


def test_train_points_frozen_trains_the_decoder_alone(dev):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size, ext = (96, 80), (96, 80)
    image = _image(size, dev, seed=2)
    f = HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=4, num_bits=6)
    pts, target = centres(ext, dev), image.reshape(-1, 3).contiguous()
    f.train_points(pts, target)
    a = _twin(f)
    f.freeze()
    a.freeze()
    table = f.table.detach().clone()
    assert torch.equal(a.table.detach(), table)
    la, lf = a.train_step([[0, 0]], ext, target), f.train_points(pts, target)
    assert torch.equal(f.table.detach(), table) and f.table.grad is None
    assert abs(float(la) - float(lf)) <= 1e-5 * abs(float(la))
    for pa, pf in zip(a.decoder.linear_params(), f.decoder.linear_params()):
        assert torch.equal(pa, pf)                                               # no atomics on this path: the same launches


def test_train_points_fits_scattered_samples(dev):
    """what the entry is for: fit an image from random (point, colour) samples that never form a raster, then decode the lattice"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (128, 128)
    image = _image(size, dev, seed=5)
    f = HashGridField(size, levels=8, features=2, log2_table=14, device=dev, seed=5)
    g = torch.Generator(device=dev).manual_seed(6)
    first = None
    for it in range(200):
        idx = torch.randint(0, size[0] * size[1], (8192,), generator=g, device=dev)
        pts = torch.stack([idx // size[1], idx % size[1]], dim=1).float().contiguous()
        loss = float(f.train_points(pts, image.reshape(-1, 3)[idx].contiguous()))
        first = loss if first is None else first
    assert loss < 0.1 * first, (first, loss)
    assert float(((f.decode() - image) ** 2).mean()) < 0.1 * first


def test_refused_train_points_leaves_the_pass_alone(dev):
    """the checks come before the first write: a call refused for its arguments does not clear the gradients of a pass in progress"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (96, 80)
    image = _image(size, dev, seed=2)
    f = HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=4)
    pts, target = centres(size, dev), image.reshape(-1, 3).contiguous()
    f.train_points(pts[:4000].contiguous(), target[:4000].contiguous(), scale=0.5, step=False)
    grad = f.table.grad.clone()
    dec = [p.grad.clone() for p in f.decoder.linear_params()]
    assert bool((grad != 0).any()) and f._pass_samples == 4000
    with pytest.raises(ValueError):
        f.train_points(pts[4000:].contiguous(), target[4001:].contiguous())      # one target short
    with pytest.raises(ValueError):
        f.train_points(torch.empty(0, 2, device=dev), torch.empty(0, 3, device=dev))
    with pytest.raises(ValueError):
        f.train_points(pts[:10, :1].contiguous(), target[:10].contiguous())
    assert torch.equal(f.table.grad, grad) and f._pass_samples == 4000 and f.steps == 0
    for p, g in zip(f.decoder.linear_params(), dec):
        assert p.grad is not None and torch.equal(p.grad, g)
