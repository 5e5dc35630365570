"""GPU tests of the hash-grid codec with a bit depth per level (nic_hash_*_levels, csrc/hash_mixed.hip; HashGridField(num_bits=[..]);
DESIGN 4.7.6).  The reference is the pinned uniform-depth code applied level by level: level l of a mixed launch must equal, bit for bit,
level l of the uniform launch at depth b_l.  Fused against layer-wise keeps the project's margins for that comparison (TOL_Y = 5e-6,
TOL_G = 1e-4 of the reference's largest magnitude, tests/test_gpu_hashgrid_fused.py)."""
import os
import statistics
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_Y, TOL_G, TOL_ORDER = 5e-6, 1e-4, 1e-5
NAMES = ["dW1", "db1", "dW2", "db2", "dW3", "db3"]
# tight (F b divides 32 or is 64) and straddling depths, 1 and 8 included
BITS = {2: (8, 5, 3, 4), 3: (7, 2, 6, 1)}
CASES = [(dim, F) for dim in (2, 3) for F in (1, 2, 4, 8)]
# the seed-to-seed spread of the uniform b = 4 fit on the structured image (38.15 / 38.04 dB on seeds 1 / 2, DESIGN 4.7.1: 0.11 dB); the margin
# is a little over twice that, since two samples underestimate a range - fixed before the mixed fit was first run
QUALITY_MARGIN_DB = 0.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def relmax(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def check(a, b, tol, what):
    e = relmax(a, b)
    print(f"{what}: {e:.3e}")
    assert e <= tol, f"{what}: max error over the reference's largest magnitude {e:.3e} > {tol:.1e}"


def psnr(a, b):
    return float(10 * torch.log10(1.0 / ((a - b) ** 2).mean()))


def _geo(dim, F, levels=4):
    """dense coarse levels and a hashed fine one in a 2^10 table; non-square, not a multiple of the patch"""
    from neural_image_compression_v2_amd.hashgrid import HashGeometry
    if dim == 2:
        geo = HashGeometry((52, 37), (4, 9, 20, 45, 51)[:levels], F, 10)
    else:
        geo = HashGeometry((21, 13, 18), (2, 5, 9, 14, 20)[:levels], F, 10)
    dense = {(r + 1) ** dim <= 1024 for r in geo.resolutions}
    assert dense == {True, False}
    return geo


def _entries(geo):
    return [min((r + 1) ** geo.dim, geo.table_size) for r in geo.resolutions]


def _offsets(geo, bits):
    """byte offset of every level and of the tail: 4 sum_{k<l} ceil(E_k F b_k / 32), restated"""
    off = [0]
    for e, b in zip(_entries(geo), bits):
        off.append(off[-1] + 4 * (-(-(e * geo.features * b) // 32)))
    return off


def _table(geo, bits, dev, seed=0):
    """random values, level l inside its own range (and on both of its edges)"""
    from neural_image_compression_v2_amd import models
    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.rand(geo.table_shape(), generator=g, device=dev) * 1.2 - 0.6
    for l, b in enumerate(bits):
        t[l] = torch.clamp(t[l], *models._q_range(b))
    return t.contiguous()


def _crops(geo):
    """two crops that leave patches half empty"""
    if geo.dim == 2:
        return [[3, 1], [21, 17]], (27, 19)
    return [[1, 0, 2], [8, 3, 5]], (11, 9, 10)


def _points(geo, dev, seed=1, n=1500):
    g = torch.Generator(device=dev).manual_seed(seed)
    S = torch.tensor([float(s) for s in geo.field_size], device=dev)
    inside = torch.rand(n, geo.dim, generator=g, device=dev) * S - 0.5
    grids = torch.meshgrid(*[torch.arange(min(s, 9), device=dev) for s in geo.field_size], indexing="ij")
    centres = torch.stack([x.reshape(-1) for x in grids], dim=1).to(torch.float32)
    rows = []
    for a in range(geo.dim):
        for val in [-0.5, float("nan"), float("inf"), float("-inf"), -3.7, 1e30, geo.field_size[a] - 0.5, geo.field_size[a] + 10.25]:
            r = inside[len(rows)].clone()
            r[a] = val
            rows.append(r)
    rows.append(torch.full((geo.dim,), float("nan"), device=dev))
    return torch.cat([inside, centres, torch.stack(rows)], dim=0).contiguous()


def _decoder(geo, dev, seed=3):
    g = torch.Generator(device=dev).manual_seed(seed)
    shapes = [(64, geo.width), (64,), (64, 64), (64,), (3, 64), (3,)]
    return [((torch.rand(*s, generator=g, device=dev) * 2 - 1) * (1.0 / max(s[-1], 8)) ** 0.5).contiguous() for s in shapes]


# ---- pack ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,F", CASES)
def test_pack_holds_each_levels_uniform_bytes(dev, dim, F):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo, bits = _geo(dim, F), BITS[dim]
    table = _table(geo, bits, dev, seed=dim + F)
    mixed = hg.hash_pack_bits_levels(geo, table, bits)
    off = _offsets(geo, bits)
    assert mixed.numel() == off[-1] + 8 == hg.hash_packed_bytes(geo, bits)
    for l, b in enumerate(bits):
        ref, roff = hg.hash_pack_bits(geo, table, b), _offsets(geo, [b] * geo.levels)
        assert roff[l + 1] - roff[l] == off[l + 1] - off[l]
        assert torch.equal(mixed[off[l]:off[l + 1]], ref[roff[l]:roff[l + 1]]), (l, b)
    assert int(mixed[off[-1]:].max()) == 0                                        # the tail
    for b in (3, 4, 8):                                                           # equal depths: the /1 buffer
        assert torch.equal(hg.hash_pack_bits_levels(geo, table, [b] * geo.levels), hg.hash_pack_bits(geo, table, b)), b


# ---- rows from the packed table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,F", CASES)
def test_packed_rows_are_the_uniform_rows_per_level(dev, dim, F):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo, bits = _geo(dim, F), BITS[dim]
    table = _table(geo, bits, dev, seed=10 + dim + F)
    mixed = hg.hash_pack_bits_levels(geo, table, bits)
    coord, extent = _crops(geo)
    pts = _points(geo, dev)
    lat = hg.hash_encode_levels(geo, mixed, bits, coord=coord, extent=extent, kind="bits")
    at = hg.hash_encode_levels(geo, mixed, bits, points=pts, kind="bits")
    assert lat.shape == (2 * torch.tensor(extent).prod().item(), geo.width) and at.shape == (pts.shape[0], geo.width)
    for l, b in enumerate(bits):
        ref = hg.hash_pack_bits(geo, table, b)
        cols = slice(l * F, l * F + F)
        assert torch.equal(lat[:, cols], hg.hash_encode_bits(geo, ref, coord, extent, b)[:, cols]), (l, b)
        assert torch.equal(at[:, cols], hg.hash_encode_points(geo, ref, pts, "bits", b)[:, cols]), (l, b)
    assert bool(torch.isfinite(at).all())
    # the fp32 source without noise is nic_hash_encode's row
    assert torch.equal(hg.hash_encode_levels(geo, table, bits, coord=coord, extent=extent), hg.hash_encode(geo, table, coord, extent))
    assert torch.equal(hg.hash_encode_levels(geo, table, bits, points=pts), hg.hash_encode_points(geo, table, pts))


# ---- noisy rows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,F", CASES)
def test_noisy_rows_are_the_uniform_rows_per_level(dev, dim, F):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo, bits = _geo(dim, F), BITS[dim]
    table = _table(geo, bits, dev, seed=20 + dim + F)
    coord, extent = _crops(geo)
    pts = _points(geo, dev, seed=2)
    seed, offset, base = 0x1234_5678_9ABC, 41, (1 << 33) + 5
    lat = hg.hash_encode_levels(geo, table, bits, coord=coord, extent=extent, quant=(seed, offset, base))
    at = hg.hash_encode_levels(geo, table, bits, points=pts, quant=(seed, offset, base))
    for l, b in enumerate(bits):
        cols = slice(l * F, l * F + F)
        assert torch.equal(lat[:, cols], hg.hash_encode_noisy(geo, table, coord, extent, b, seed, offset, base)[:, cols]), (l, b)
        assert torch.equal(at[:, cols], hg.hash_encode_points(geo, table, pts, quant=(b, seed, offset, base))[:, cols]), (l, b)
    same = hg.hash_encode_levels(geo, table, [5] * geo.levels, coord=coord, extent=extent, quant=(seed, offset, base))
    assert torch.equal(same, hg.hash_encode_noisy(geo, table, coord, extent, 5, seed, offset, base))
    assert not torch.equal(lat, hg.hash_encode(geo, table, coord, extent))


# ---- clamp -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,F", [(2, 1), (2, 8), (3, 2), (3, 4)])
def test_clamp_levels_is_torch_clamp_per_level(dev, dim, F):
    from neural_image_compression_v2_amd import hashgrid as hg, models
    geo, bits = _geo(dim, F), BITS[dim]
    t = (torch.rand(geo.table_shape(), generator=torch.Generator(device=dev).manual_seed(4), device=dev) * 1.4 - 0.7).contiguous()
    t[0, 3, 0] = float("nan")
    t[geo.levels - 1, 1023, F - 1] = float("nan")
    t[1, 5, 0], t[2, 6, 0] = float("inf"), float("-inf")
    want = torch.stack([torch.clamp(t[l], *models._q_range(b)) for l, b in enumerate(bits)])
    got = hg.hash_clamp_levels(geo, t.clone(), bits)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))               # bit for bit, the NaNs included
    assert bool(torch.isnan(got[0, 3, 0])) and int(torch.isnan(got).sum()) == 2


# ---- fused against layer-wise ----------------------------------------------------------------------------------------------------------------
FUSED_CASES = CASES + [(2, 8, 5), (3, 8, 5)]                                          # L F = 40: two column tiles of the weight gradient


@pytest.mark.parametrize("case", FUSED_CASES)
def test_fused_forward_is_the_layerwise_decode(dev, case):
    from neural_image_compression_v2_amd import hashgrid as hg
    from neural_image_compression_v2_amd.fused import DecoderFunction
    dim, F = case[:2]
    geo = _geo(dim, F, *case[2:])
    bits = (BITS[dim] + (4,))[:geo.levels]
    table = _table(geo, bits, dev, seed=30 + dim + F)
    mixed = hg.hash_pack_bits_levels(geo, table, bits)
    params = _decoder(geo, dev)
    coord, extent = _crops(geo)
    pts = _points(geo, dev, seed=3)
    for data, kind in ((mixed, "bits"), (table, "f32")):
        for pos in (dict(coord=coord, extent=extent), dict(points=pts)):
            ref = DecoderFunction.apply(hg.hash_encode_levels(geo, data, bits, kind=kind, **pos), *params)
            got = hg.hash_fused_forward_levels(geo, data, bits, params, kind=kind, **pos)
            check(got, ref, TOL_Y, f"fused forward {dim}D F={F} L={geo.levels} {kind} {'points' if 'points' in pos else 'lattice'}")


def _layerwise_step(geo, table, bits, params, target, quant, scale, pos):
    from neural_image_compression_v2_amd import hashgrid as hg
    from neural_image_compression_v2_amd.fused import DecoderFunction
    x = hg.hash_encode_levels(geo, table, bits, quant=quant, **pos).requires_grad_(True)
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    y = DecoderFunction.apply(x, *ps)
    loss = ((y - target) ** 2).mean() * scale
    loss.backward()
    grad = torch.zeros(geo.table_shape(), device=table.device)
    if "points" in pos:
        hg.hash_encode_points_backward(geo, pos["points"], x.grad, grad)
    else:
        org = geo.upload_origins(pos["coord"], pos["extent"], table.device)
        hg.hash_encode_backward(geo, org, pos["extent"], x.grad, grad)
    return y.detach(), loss.detach(), grad, [p.grad for p in ps]


@pytest.mark.parametrize("case", FUSED_CASES)
def test_fused_forward_backward_is_the_layerwise_step(dev, case):
    from neural_image_compression_v2_amd import hashgrid as hg
    dim, F = case[:2]
    geo = _geo(dim, F, *case[2:])
    bits = (BITS[dim] + (4,))[:geo.levels]
    table = _table(geo, bits, dev, seed=40 + dim + F)
    params = _decoder(geo, dev, seed=5)
    coord, extent = _crops(geo)
    pts = _points(geo, dev, seed=4)
    quant, scale = (77, 3, 1000), 0.75
    for pos in (dict(coord=coord, extent=extent), dict(points=pts)):
        n = pts.shape[0] if "points" in pos else 2 * int(torch.tensor(extent).prod())
        tag = f"{dim}D F={F} L={geo.levels} {'points' if 'points' in pos else 'lattice'}"
        target = torch.rand(n, 3, generator=torch.Generator(device=dev).manual_seed(6), device=dev)
        for q in (quant, None):
            y0, l0, g0, gm0 = _layerwise_step(geo, table, bits, params, target, q, scale, pos)
            orders = [None]
            if "points" in pos:
                orders += [hg.hash_point_order(geo, pts), torch.randperm(n, generator=torch.Generator().manual_seed(2)).to(torch.int32).to(dev)]
            for order in orders:
                gm = [torch.full_like(p, 7.0) for p in params]                       # overwritten
                grad = torch.zeros(geo.table_shape(), device=dev)
                kw = dict(order=order) if order is not None else {}
                loss, y = hg.hash_fused_forward_backward_levels(geo, table, bits, params, target, gm, table_grad=grad, loss_scale=scale, want_y=True,
                                                                quant=q, **pos, **kw)
                what = f"{tag} noise={q is not None} order={order is not None}"
                check(y, y0, TOL_Y, what + " y")
                check(loss, l0.reshape(1), TOL_Y, what + " loss")
                check(grad, g0, TOL_G, what + " table grad")
                for name, a, b in zip(NAMES, gm, gm0):
                    check(a, b, TOL_G, what + " " + name)
        # ADD_GRADS / ADD_LOSS add to what the buffers hold; a null table_grad forms no table gradient
        gm = [0.5 * g for g in gm0]                                                  # of the gradients' own size: no cancellation in the check
        loss = torch.full((1,), 2.0, device=dev)
        hg.hash_fused_forward_backward_levels(geo, table, bits, params, target, gm, table_grad=None, loss=loss, loss_scale=scale, quant=None,
                                              add_grads=True, add_loss=True, **pos)
        check(loss, (l0 + 2.0).reshape(1), TOL_Y, tag + " ADD_LOSS")
        for name, a, b in zip(NAMES, gm, gm0):
            check(a, 1.5 * b, TOL_G, tag + " ADD_GRADS " + name)


# ---- field level ---------------------------------------------------------------------------------------------------------------------------------
def _image(size, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.linspace(0, 1, size[0], device=dev)[:, None]
    y = torch.linspace(0, 1, size[1], device=dev)[None, :]
    base = torch.stack([0.5 + 0.3 * torch.sin(7 * x + 3 * y), 0.5 + 0.3 * torch.cos(5 * x * y * 4), 0.5 + 0.2 * torch.sin(13 * y - 2 * x)], dim=-1)
    return (base + 0.05 * torch.rand(*size, 3, generator=g, device=dev)).clamp(0, 1)


def _structured_image(size, dev):
    """tests/test_gpu_hashgrid_codec.py's structured image, imported so that the two cannot drift apart"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import test_gpu_hashgrid_codec as codec
    finally:
        sys.path.pop(0)
    return codec._structured_image(size, dev)


FIELD_BITS = (8, 8, 7, 6, 5, 4, 3, 4)

CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
from neural_image_compression_v2_amd.hashgrid import HashGridField
f = HashGridField.load_compressed({path!r}, "cuda:0", fused={fused})
want = torch.load({want!r}).cuda()
assert f.level_bits == {bits!r} and f.num_bits is None and f.table is None
assert torch.equal(f.decode(tile=64), want)
print("child ok")
"""


@pytest.mark.parametrize("fused", [False, True])
def test_fit_freeze_save_load_decode(dev, tmp_path, fused):
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import HashGridField, hash_packed_bytes
    size = (120, 72)
    image = _image(size, dev, seed=2)
    field = HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=5, num_bits=list(FIELD_BITS), fused=fused)
    assert field.level_bits == FIELD_BITS and field.num_bits is None and field.route == ("fused" if fused else "layerwise")
    # while the table trains every level stays inside its own range
    for k in range(6):
        field.train_step([[0, 0]], size, image.reshape(-1, 3))
        t = field.table.detach()
        for l, b in enumerate(FIELD_BITS):
            lo, hi = models._q_range(b)
            assert float(t[l].min()) >= lo and float(t[l].max()) <= hi, (k, l, b)
    hist = field.fit(image, 40, chunk=50)
    assert field.frozen and field.table.grad is None and hist[-1] < hist[0]
    t = field.table.detach()
    for l, b in enumerate(FIELD_BITS):
        lo, hi = models._q_range(b)
        assert float(t[l].min()) >= lo and float(t[l].max()) <= hi
        assert torch.equal(t[l], models.quantize4fp(t[l], b))                       # frozen: each level nic_quantize'd with its depth
    mem = field.decode(tile=64)
    path = tmp_path / "mixed.pt"
    field.save_compressed(path, packed=True)
    with pytest.raises(ValueError):
        field.save_compressed(tmp_path / "u8.pt")
    d = torch.load(path, weights_only=True)
    assert d["format"] == "nicv2-hashgrid-bits/2" and d["level_bits"] == list(FIELD_BITS)
    assert d["table"].numel() == field.stored_bytes(packed=True)["table"] == hash_packed_bytes(field.geo, FIELD_BITS)
    for route in (False, True):
        loaded = HashGridField.load_compressed(path, dev, fused=route)
        assert loaded.table is None and loaded.stored is None and loaded.packed is not None and loaded.level_bits == FIELD_BITS
        dec = loaded.decode(tile=64)
        if route == fused:
            assert torch.equal(dec, mem)                                          # the frozen field's image, bit for bit
        else:
            check(dec, mem, TOL_Y, "the other route's decode")
        # query at the sample centres is decode
        grids = torch.meshgrid(*[torch.arange(s, device=dev) for s in size], indexing="ij")
        centres = torch.stack([g.reshape(-1) for g in grids], dim=1).to(torch.float32).contiguous()
        assert torch.equal(loaded.query(centres).reshape(*size, 3), dec)
        assert torch.equal(loaded.resample(size, tile=64), dec)
        # a decode-only field re-saves its buffer as it is
        loaded.save_compressed(tmp_path / "again.pt", packed=True)
        assert torch.equal(torch.load(tmp_path / "again.pt", weights_only=True)["table"], d["table"])
    # the same in a fresh process
    torch.save(mem.cpu(), tmp_path / "want.pt")
    code = CHILD.format(root=ROOT, path=str(path), want=str(tmp_path / "want.pt"), fused=fused, bits=FIELD_BITS)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("fused", [False, True])
def test_equal_depths_and_int_fields_agree(dev, tmp_path, fused):
    """[b] * L against b: the same loss sequence and the same stored bytes (the int field makes the calls it always made; the list takes the
    mixed path, whose rows and packed levels are the uniform ones bit for bit).  The table gradient is a sum of atomics, so the layer-wise
    later losses agree like two runs of one field, the first loss bit for bit on the layer-wise route."""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (64, 48)
    image = _image(size, dev, seed=3)
    kw = dict(levels=6, features=2, log2_table=11, device=dev, seed=9, fused=fused)
    a, b = HashGridField(size, num_bits=4, **kw), HashGridField(size, num_bits=[4] * 6, **kw)
    assert a.level_bits is None and a.num_bits == 4 and b.level_bits == (4,) * 6
    assert torch.equal(a.table, b.table)
    la = [a.train_step([[0, 0]], size, image.reshape(-1, 3)) for _ in range(5)]
    lb = [b.train_step([[0, 0]], size, image.reshape(-1, 3)) for _ in range(5)]
    if not fused:
        assert torch.equal(la[0], lb[0])                                            # the same noisy rows into the same decoder code
    check(lb[0].reshape(1), la[0].reshape(1), TOL_Y, "first loss of [4] * L against 4")
    for x, y in zip(la, lb):                 # later steps inherit the order of the table-gradient atomics through Adam, like two runs of one field
        check(y.reshape(1), x.reshape(1), 1e-3, "loss of [4] * L against 4")
    # stored bytes of one and the same table
    with torch.no_grad():
        b.table.copy_(a.table)
    a.save_compressed(tmp_path / "a.pt", packed=True)
    b.save_compressed(tmp_path / "b.pt", packed=True)
    ta, tb = torch.load(tmp_path / "a.pt", weights_only=True), torch.load(tmp_path / "b.pt", weights_only=True)
    assert ta["format"].endswith("/1") and tb["format"].endswith("/2") and torch.equal(ta["table"], tb["table"])
    assert a.stored_bytes(packed=True) == b.stored_bytes(packed=True)


@pytest.mark.parametrize("points", [False, True])
def test_tail_step_is_a_separate_optimizer_step(dev, points):
    """the fused mixed step with the optimiser tail (and the level clamp after it) against the same call without the tail followed by
    optimizer.step() and the clamp: the decoder bit for bit (fixed-order sums), the table within the order-of-atomics bound"""
    from neural_image_compression_v2_amd import hashgrid as hg
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (64, 48)
    image = _image(size, dev, seed=4).reshape(-1, 3).contiguous()
    kw = dict(levels=6, features=2, log2_table=11, device=dev, seed=11, fused=True, num_bits=[8, 7, 5, 4, 3, 2])
    a, b = HashGridField(size, **kw), HashGridField(size, **kw)
    grids = torch.meshgrid(*[torch.arange(s, device=dev) for s in size], indexing="ij")
    pts = (torch.stack([g.reshape(-1) for g in grids], dim=1).to(torch.float32) + 0.25).contiguous()

    def step(f, **k):
        return f.train_points(pts, image, fused=True, order="cell", **k) if points else f.train_step([[0, 0]], size, image, **k)
    assert torch.equal(a.table, b.table)                                         # twins: the same seed
    table = a.table.detach().clone()
    p0 = [p.detach().clone() for p in a.decoder.linear_params()]
    la = step(a)
    lb = step(b, step=False)
    b.optimizer.step()
    b._clamp_levels()
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    for pa, pb, p in zip(a.decoder.linear_params(), b.decoder.linear_params(), p0):
        assert torch.equal(pa, pb) and not torch.equal(pa, p)
    upd = float((a.table.detach() - table).abs().max())
    e = float((a.table.detach() - b.table.detach()).abs().max()) / upd
    print(f"tail against optimizer.step(): table {e:.3e} of the largest update {upd:.3e}")
    assert upd > 0 and e <= TOL_ORDER
    from neural_image_compression_v2_amd import models
    for l, bb in enumerate(a.level_bits):
        lo, hi = models._q_range(bb)
        assert float(a.table.detach()[l].min()) >= lo and float(a.table.detach()[l].max()) <= hi


def test_fit_points_mixed(dev):
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (64, 48)
    image = _image(size, dev, seed=5)
    grids = torch.meshgrid(*[torch.arange(s, device=dev) for s in size], indexing="ij")
    pts = torch.stack([g.reshape(-1) for g in grids], dim=1).to(torch.float32).contiguous()
    for fused in (False, True):
        f = HashGridField(size, levels=6, features=2, log2_table=11, device=dev, seed=2, fused=fused, num_bits=[8, 8, 6, 5, 4, 3])
        hist = f.fit_points(pts, image.reshape(-1, 3).contiguous(), 30, batch=1000)
        assert f.frozen and hist[-1] < 0.5 * hist[0], hist
        for l, b in enumerate(f.level_bits):
            assert torch.equal(f.table[l], models.quantize4fp(f.table[l].detach(), b))


# ---- quality ---------------------------------------------------------------------------------------------------------------------------------------
def test_mixed_allocation_quality(dev, tmp_path):
    """the structured 256^2 image of DESIGN 4.7.1 at log2_table 12 with test_fit_quality_2d_qat's shape and epochs: 8 bits for every level
    whose E_l lies below the median E_l and 4 for the rest must decode from its file no worse than the uniform b = 4 fit minus the seed-to-seed
    spread margin (QUALITY_MARGIN_DB), in a table smaller than the uniform b = 8 one"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size, epochs = (256, 256), 300
    image = _structured_image(size, dev)
    kw = dict(levels=8, features=2, log2_table=12, device=dev, seed=1)
    probe = HashGridField(size, num_bits=4, **kw)
    entries = [min((r + 1) ** 2, 1 << 12) for r in probe.resolutions]
    med = statistics.median(entries)
    alloc = [8 if e < med else 4 for e in entries]
    assert 8 in alloc and 4 in alloc, (entries, alloc)
    res, nbytes = {}, {}
    for name, b in (("b4", 4), ("mixed", alloc)):
        f = HashGridField(size, num_bits=b, **kw)
        f.set_schedule(epochs)
        f.fit(image, epochs)
        f.save_compressed(tmp_path / f"{name}.pt", packed=True)
        nbytes[name] = f.stored_bytes(packed=True)["table"]
        res[name] = psnr(HashGridField.load_compressed(tmp_path / f"{name}.pt", dev).decode(), image)
    b8 = HashGridField(size, num_bits=8, **kw).stored_bytes(packed=True)["table"]
    print(f"allocation {alloc} (E_l {entries}): {res['mixed']:.2f} dB in {nbytes['mixed']} B; uniform b=4 {res['b4']:.2f} dB in {nbytes['b4']} B; "
          f"uniform b=8 table {b8} B")
    assert nbytes["mixed"] < b8
    assert res["mixed"] >= res["b4"] - QUALITY_MARGIN_DB, res
