"""GPU tests of the batched decode from stored tables and at points (nic_hash_batch_forward_source, csrc/hashgrid_batch.hip;
HashGridFieldBatch.load_compressed / decode / query / resample).

The yardstick is always the existing SINGLE-field entries, called once per field on slices of the same stacked tensors - hash_fused_forward /
_u8 / _bits on the lattice, hash_fused_forward_points(kind=...) at points, which tests/test_gpu_hashgrid_fused.py, _packed.py and _points.py pin -
and never the code under test.  The bound is that suite's fp32 against fp32, TOL_Y = 5e-6 (max error over the reference's largest magnitude).
On the lattice the batched kernel runs the single kernel's operations in its order, so bit equality is asserted as well; the single-field POINT
kernel still carries its own decoder body, so at points the bound is asserted and whether the bits are equal is printed.  Values differ per field
(tables +-0.6 clamped to the quantiser's range and pushed through hash_pack_u8 / hash_pack_bits, decoders at twice nn.Linear's init): a shared or
swapped field cannot pass.  Shapes are the smallest at which each thing can go wrong."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_Y = 5e-6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def relmax(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def check(a, b, what, bits=True):
    e, same = relmax(a, b), torch.equal(a, b)
    print(f"{what}: {e:.3e} bits {'equal' if same else 'differ'}")
    assert e <= TOL_Y, f"{what}: max error over the reference's largest magnitude {e:.3e} > {TOL_Y:.1e}"
    if bits:
        assert same, f"{what}: not bit for bit ({e:.3e})"


def _geo(field_size, levels, F, log2_table, n_min=16):
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, level_resolutions
    return HashGeometry(tuple(field_size), tuple(level_resolutions(levels, n_min, max(field_size))), F, log2_table)


def _tight(F, b):
    """hash_bits_tight (csrc/hash_common.hpp): no entry of F b bits straddles a dword"""
    return 32 % (F * b) == 0 or F * b == 64


def _depth(F, tight):
    """a packed depth at which the gather takes the tight (one dword) or the straddling (funnel shift) window"""
    b = next(b for b in (4, 5, 3, 6, 7) if _tight(F, b) == tight)
    assert _tight(F, b) == tight
    return b


def _stacked(geo, dev, B, seed):
    """tables [B, L, T, F] in +-0.6 and the six stacked decoder tensors at twice nn.Linear's init, every field its own values"""
    from neural_image_compression_v2_amd.image_compression import ColorDecoder
    g = torch.Generator(device=dev).manual_seed(seed)
    tables = (torch.rand(B, *geo.table_shape(), generator=g, device=dev) * 2 - 1) * 0.6
    torch.manual_seed(seed + 1)
    decs = [ColorDecoder(geo.width, 64, 3).linear_params() for _ in range(B)]
    params = [(2.0 * torch.stack([d[k].detach() for d in decs])).to(dev).contiguous() for k in range(6)]
    return tables, params


def _source(geo, tables, kind, bits):
    """the stacked tables as the source ``kind``: fp32 as they are, or every field through hash_pack_u8 / hash_pack_bits -> uint8 [B, bytes]"""
    from neural_image_compression_v2_amd import hashgrid, models
    if kind == "f32":
        return tables
    pack = hashgrid.hash_pack_u8 if kind == "u8" else hashgrid.hash_pack_bits
    return torch.stack([pack(geo, models.quantize_clamp(tables[b], bits), bits) for b in range(tables.shape[0])]).contiguous()


def _origins(geo, extent, B, num_crops, dev, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.stack([torch.randint(0, s - e + 1, (B, num_crops), generator=g) for s, e in zip(geo.field_size, extent)], dim=-1)
    return o.to(torch.int32).to(dev)


def _points(geo, B, n, dev, seed):
    """[B, n, dim] fp32, every field its own, a third of them outside the field (they read its edge)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    size = torch.tensor(geo.field_size, dtype=torch.float32, device=dev)
    p = torch.rand(B, n, geo.dim, generator=g, device=dev) * size - 0.5
    out = torch.rand(B, n, generator=g, device=dev) < 1 / 3
    far = (torch.rand(B, n, geo.dim, generator=g, device=dev) * 3 - 1) * size
    return torch.where(out.unsqueeze(-1), far, p).contiguous()


def _single_lattice(geo, data, kind, bits, org, extent, params):
    from neural_image_compression_v2_amd import hashgrid
    out = []
    for b in range(data.shape[0]):
        ps = [p[b] for p in params]
        if kind == "f32":
            out.append(hashgrid.hash_fused_forward(geo, data[b], org[b], extent, ps))
        elif kind == "u8":
            out.append(hashgrid.hash_fused_forward_u8(geo, data[b], org[b], extent, bits, ps))
        else:
            out.append(hashgrid.hash_fused_forward_bits(geo, data[b], org[b], extent, bits, ps))
    return torch.stack(out)


def _single_points(geo, data, kind, bits, pts, params):
    from neural_image_compression_v2_amd import hashgrid
    return torch.stack([hashgrid.hash_fused_forward_points(geo, data[b], pts[b], [p[b] for p in params], kind, bits) for b in range(data.shape[0])])


# field size, levels, F, log2_table, n_min, crop extent, crops, B, groups_per_field, the sources ("tight" / "loose": a packed depth of that window)
CASES = {
    "2d": ((40, 36), 4, 2, 10, 16, (20, 12), 2, 3, 0, [("f32", None), ("u8", 8), ("bits", "tight"), ("bits", "loose")]),      # patch rims, two crops
    "2d_lf48": ((40, 36), 12, 4, 10, 16, (20, 12), 2, 3, 0, [("bits", "tight"), ("bits", "loose")]),                          # L F = 48
    "3d": ((12, 10, 9), 4, 1, 10, 4, (7, 10, 5), 2, 3, 0, [("u8", 8), ("bits", "tight"), ("bits", "loose")]),                 # 4 x 4 x 4 patches with rims
    "single": ((40, 36), 4, 2, 10, 16, (20, 12), 2, 1, 0, [("u8", 8), ("bits", "loose")]),                                    # B = 1
    "many": ((40, 36), 4, 2, 10, 16, (20, 12), 1, 40, 8, [("u8", 8), ("bits", "tight")]),                                     # 320 workgroups, 6 patches a field
}
LATTICE = [(name, k) for name, c in CASES.items() for k in range(len(c[9]))]
_cache = {}


def _case(name, k, dev):
    """the inputs of a case and source, built once per module and left unchanged"""
    if (name, k) not in _cache:
        size, levels, F, log2_table, n_min, extent, crops, B, groups, sources = CASES[name]
        geo = _geo(size, levels, F, log2_table, n_min)
        i = list(CASES).index(name)
        if ("base", name) not in _cache:
            _cache[("base", name)] = (*_stacked(geo, dev, B, 500 + i), _origins(geo, extent, B, crops, dev, 600 + i))
        tables, params, org = _cache[("base", name)]
        kind, bits = sources[k]
        if isinstance(bits, str):
            bits = _depth(F, bits == "tight")
        _cache[(name, k)] = (geo, _source(geo, tables, kind, bits), kind, bits, org, extent, params, groups)
    return _cache[(name, k)]


@pytest.mark.parametrize("name,k", LATTICE, ids=[f"{n}-{CASES[n][9][k][0]}-{CASES[n][9][k][1]}" for n, k in LATTICE])
def test_lattice_route_equals_the_single_field_entries(dev, name, k):
    from neural_image_compression_v2_amd.hashgrid import hash_batch_forward_source
    geo, data, kind, bits, org, extent, params, groups = _case(name, k, dev)
    if kind == "bits":
        print(f"packed depth {bits}: tight {_tight(geo.features, bits)}")
    ref = _single_lattice(geo, data, kind, bits, org, extent, params)
    y = hash_batch_forward_source(geo, data, params, kind, bits, coord=org, extent=extent, groups_per_field=groups)
    assert y.shape == ref.shape
    for b in range(data.shape[0]):
        check(y[b], ref[b], f"{name} {kind} {bits} field {b}")
    # the same launch twice: the same bits; and into a buffer of the caller's
    out = torch.full_like(y, 7.0)
    assert hash_batch_forward_source(geo, data, params, kind, bits, coord=org, extent=extent, groups_per_field=groups, out=out) is out
    assert torch.equal(out, y)


def test_fp32_source_equals_the_batched_forward(dev):
    from neural_image_compression_v2_amd.hashgrid import hash_batch_forward, hash_batch_forward_source
    geo, data, kind, bits, org, extent, params, _ = _case("2d", 0, dev)
    assert kind == "f32"
    assert torch.equal(hash_batch_forward_source(geo, data, params, coord=org, extent=extent), hash_batch_forward(geo, data, org, extent, params))


@pytest.mark.parametrize("name,k", [("2d", 1), ("2d", 3), ("3d", 1)], ids=["2d-u8", "2d-bits-loose", "3d-bits-tight"])
def test_a_field_alone_and_among_others_gives_the_same_bits(dev, name, k):
    from neural_image_compression_v2_amd.hashgrid import hash_batch_forward_source
    geo, data, kind, bits, org, extent, params, _ = _case(name, k, dev)
    pts = _points(geo, data.shape[0], 130, dev, 40)
    y = hash_batch_forward_source(geo, data, params, kind, bits, coord=org, extent=extent)
    yp = hash_batch_forward_source(geo, data, params, kind, bits, points=pts)
    for b in range(data.shape[0]):
        one = [p[b:b + 1].contiguous() for p in params]
        d1 = data[b:b + 1].clone()
        assert torch.equal(hash_batch_forward_source(geo, d1, one, kind, bits, coord=org[b:b + 1].contiguous(), extent=extent)[0], y[b]), b
        assert torch.equal(hash_batch_forward_source(geo, d1, one, kind, bits, points=pts[b:b + 1].contiguous())[0], yp[b]), b


POINT_CASES = [("2d", 0), ("2d", 1), ("2d", 2), ("2d", 3), ("2d_lf48", 1), ("3d", 0), ("3d", 2), ("single", 1), ("many", 1)]


@pytest.mark.parametrize("name,k", POINT_CASES, ids=[f"{n}-{CASES[n][9][k][0]}-{CASES[n][9][k][1]}" for n, k in POINT_CASES])
def test_points_route_against_the_single_field_point_entry(dev, name, k):
    from neural_image_compression_v2_amd.hashgrid import hash_batch_forward_source
    geo, data, kind, bits, _, _, params, groups = _case(name, k, dev)
    B = data.shape[0]
    for n in (130, 1):                            # three wave items with a ragged tail (most workgroups have none); one point
        pts = _points(geo, B, n, dev, 700 + n)
        ref = _single_points(geo, data, kind, bits, pts, params)
        y = hash_batch_forward_source(geo, data, params, kind, bits, points=pts, groups_per_field=groups)
        assert y.shape == (B, n, 3)
        for b in range(B):
            check(y[b], ref[b], f"points {name} {kind} {bits} N {n} field {b}", bits=False)
        assert torch.equal(hash_batch_forward_source(geo, data, params, kind, bits, points=pts, groups_per_field=groups), y)      # the same bits again
    # shared [N, dim] points are the same points stacked
    shared = _points(geo, 1, 130, dev, 77)[0]
    assert torch.equal(hash_batch_forward_source(geo, data, params, kind, bits, points=shared),
                       hash_batch_forward_source(geo, data, params, kind, bits, points=shared.unsqueeze(0).expand(B, -1, -1).contiguous()))
    # no points: an empty result, nothing launched
    y0 = hash_batch_forward_source(geo, data, params, kind, bits, points=torch.empty(B, 0, geo.dim, device=dev))
    assert y0.shape == (B, 0, 3)
    assert hash_batch_forward_source(geo, data, params, kind, bits, points=torch.empty(0, geo.dim, device=dev)).shape == (B, 0, 3)


def test_points_at_sample_centres_are_the_lattice(dev):
    """a point at the centre of a sample takes the lattice route's position bit for bit, and both routes share the decoder: the same bits"""
    from neural_image_compression_v2_amd.hashgrid import hash_batch_forward_source
    geo, data, kind, bits, _, _, params, _ = _case("2d", 3, dev)
    size = geo.field_size
    y = hash_batch_forward_source(geo, data, params, kind, bits, coord=[[0, 0]], extent=size)
    ax = [torch.arange(s, dtype=torch.float32, device=dev) for s in size]
    pts = torch.stack([g.reshape(-1) for g in torch.meshgrid(*ax, indexing="ij")], dim=1).contiguous()
    assert torch.equal(hash_batch_forward_source(geo, data, params, kind, bits, points=pts), y)


def test_end_to_end_files_batch_against_single_fields(dev, tmp_path, monkeypatch):
    from neural_image_compression_v2_amd import hashgrid
    from neural_image_compression_v2_amd.hashgrid import HashGridField, HashGridFieldBatch
    B = 3
    batch = HashGridFieldBatch(B, (64, 64), levels=8, log2_table=12, num_bits=4, device=dev, seed=11)
    g = torch.Generator(device=dev).manual_seed(12)
    x = torch.linspace(0, 1, 64, device=dev)
    images = torch.stack([torch.stack([torch.outer(torch.sin((b + 2) * x) ** 2, torch.cos((c + 1) * x) ** 2) for c in range(3)], dim=-1) for b in range(B)])
    images = (images + 0.05 * torch.rand(B, 64, 64, 3, generator=g, device=dev)).clamp(0, 1).contiguous()
    batch.fit(images, 6, freeze_at=0.5)           # three noisy epochs, then frozen: the decoders train alone
    assert batch.frozen and not batch.decode_only
    # a trained batch decodes with the launches it always made
    calls = []
    real = hashgrid.hash_batch_forward
    monkeypatch.setattr(hashgrid, "hash_batch_forward", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    monkeypatch.setattr(hashgrid, "hash_batch_forward_source", lambda *a, **kw: pytest.fail("a trained batch decodes through hash_batch_forward"))
    trained = batch.decode()
    assert len(calls) == 1 and len(batch.decode(tile=32)) == B and len(calls) == 1 + 4
    monkeypatch.undo()
    # ... and can be queried and resampled from its fp32 tables
    f0 = batch.extract(0)
    check(batch.resample((32, 32))[0], f0.resample((32, 32)), "trained batch resample field 0", bits=False)
    files = {}
    for packed in (False, True):
        paths = [str(tmp_path / f"f{b}_{int(packed)}.pt") for b in range(B)]
        batch.save_compressed(paths, packed=packed)
        files[packed] = paths
        loaded = HashGridFieldBatch.load_compressed(paths, device=dev)
        assert loaded.decode_only and loaded.frozen and loaded.tables is None and loaded.optimizer is None and loaded.n_fields == B
        held = loaded.packed if packed else loaded.stored
        assert (loaded.stored is None) == packed and (loaded.packed is None) != packed and held.dtype == torch.uint8 and held.shape[0] == B
        dec, dec_t, res = loaded.decode(), loaded.decode(tile=48), loaded.resample((32, 32))
        pts = _points(loaded.geo, B, 130, dev, 5)
        q = loaded.query(pts)
        assert dec.shape == (B, 64, 64, 3) and res.shape == (B, 32, 32, 3) and q.shape == (B, 130, 3)
        for b in range(B):
            single = HashGridField.load_compressed(paths[b], device=dev, fused=True)
            check(dec[b], single.decode(), f"packed {packed} decode field {b}")
            check(dec_t[b], dec[b], f"packed {packed} decode in tiles field {b}")
            check(res[b], single.resample((32, 32)), f"packed {packed} resample field {b}", bits=False)
            check(q[b], single.query(pts[b]), f"packed {packed} query field {b}", bits=False)
            ex = loaded.extract(b)
            assert ex.table is None and ex.frozen and ex.route == "fused" and ex.num_bits == 4 and (ex.packed is None) != packed
            check(ex.decode(), dec[b], f"packed {packed} extract({b}).decode()")
        # re-saved in the other format and back: the bytes of the table are the file's
        other = [str(tmp_path / f"o{b}_{int(packed)}.pt") for b in range(B)]
        back = [str(tmp_path / f"b{b}_{int(packed)}.pt") for b in range(B)]
        loaded.save_compressed(other, packed=not packed)
        HashGridFieldBatch.load_compressed(other, device=dev).save_compressed(back, packed=packed)
        for b in range(B):
            a, c = torch.load(paths[b], weights_only=True), torch.load(back[b], weights_only=True)
            assert a["format"] == c["format"] and torch.equal(a["table"], c["table"]) and a["num_bits"] == c["num_bits"] == 4
            assert all(torch.equal(a["decoder"][k], c["decoder"][k]) for k in a["decoder"])
    with pytest.raises(RuntimeError, match="decode-only"):
        loaded.fit(images, 1)
