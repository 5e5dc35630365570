"""GPU tests of the hash-grid decode and query with the decoder on the 16-bit matrix pipe (nic_hash_fused_forward_p16,
csrc/hashgrid_fused16.hip; HashGridField.decode / query / resample (precision="split" | "bf16")).

The oracle is a torch restatement of the header's contract on the device: the row comes from the EXISTING encode entry of the same source
(nic_hash_encode / _u8 / _bits on the lattice, nic_hash_encode_points at points - not the code under test), then per layer the bf16-rounded
operands (``.to(torch.bfloat16)`` rounds to nearest even) are multiplied and summed in float64, rounded to fp32 once, the bias added in fp32,
``torch.nn.functional.gelu`` and ``torch.sigmoid`` in fp32.

Bounds are absolute (y is a sigmoid output) and the project's own: ``split`` against its oracle and against the fp32 fused route 5e-6 (TOL_Y of
tests/test_gpu_hashgrid_fused.py; the README's split row), ``bf16`` against its oracle and - default initialisation only - against the fp32
route 1e-3 (the README's bf16 row).  The doubled decoder's ``bf16`` against fp32 is printed, not asserted (a CPU emulation of the reference
arithmetic alone gives 1.3e-3 there).

Shapes: 44 x 37 (partial 8 x 8 patches) and 12 x 10 x 9 (partial 4 x 4 x 4 patches), both with the smallest table the library accepts
(log2_table 10: 9 is outside the accepted 10 .. 24) so that dense and hashed levels both occur; L F = 8, 24, 32, 40, 64 (below one K = 16
step, a ragged step, the 32 boundary between the two LDS layouts, across it, the maximum); N = 209 points (a ragged last wave whose second
half tile is partly dead) and N = 5 (a wholly dead half tile), both with points outside the field and NaN / infinite coordinates."""
import ctypes
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_SPLIT, TOL_BF16 = 5e-6, 1e-3
FIELDS = {"2d": dict(size=(44, 37), log2_table=10, base=16), "3d": dict(size=(12, 10, 9), log2_table=10, base=4)}
SHAPES = [(8, 1), (12, 2), (16, 2), (10, 4), (8, 8)]                  # (L, F): L F = 8, 24, 32, 40, 64
SOURCES = [("f32", None), ("u8", 8), ("u8", 5), ("bits", 4), ("bits", 5)]     # packed: 4 tight, 5 straddling
MODES = ("split", "bf16")
CASES = [(f, L, F) for f in FIELDS for (L, F) in SHAPES]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def absmax(a, b):
    return float((a.double() - b.double()).abs().max())


def _points(size, n, dev, seed):
    """[n, dim] points: most inside the field, some outside on either side, and NaN / +-inf coordinates in the first rows"""
    g = torch.Generator().manual_seed(seed)
    s = torch.tensor([float(v) for v in size])
    pts = (torch.rand(n, len(size), generator=g) * 1.4 - 0.2) * s - 0.5           # [-0.2 S - 1/2, 1.2 S - 1/2]
    pts[0, 0], pts[1, -1], pts[2, 0], pts[3, -1] = float("nan"), float("inf"), float("-inf"), -7.25
    pts[4] = s + 3.0
    return pts.to(dev).contiguous()


def _clamped(size, pts):
    """the point the kernel reads for each point: NaN -> the low edge, everything else clamped into [-1/2, S - 1/2]"""
    out = torch.nan_to_num(pts, nan=-0.5)
    for a, s in enumerate(size):
        out[:, a] = out[:, a].clamp(-0.5, float(s) - 0.5)
    return out.contiguous()


class World:
    """one field shape: geometry, an fp32 table uniform in [-1/2, 1/2], its stored forms, the two decoders, the points, and the reference rows
    (each computed once by the existing encode entries and never written again)"""

    def __init__(self, field, L, F, dev):
        from neural_image_compression_v2_amd import hashgrid
        from neural_image_compression_v2_amd.image_compression import ColorDecoder
        spec = FIELDS[field]
        self.size, self.dev = spec["size"], dev
        self.geo = hashgrid.HashGeometry(self.size, tuple(hashgrid.level_resolutions(L, spec["base"], max(self.size))), F, spec["log2_table"])
        dense = [hashgrid.level_is_dense(r, self.geo.dim, self.geo.log2_table) for r in self.geo.resolutions]
        assert any(dense) and not all(dense), (self.geo.resolutions, dense)
        g = torch.Generator(device=dev).manual_seed(1000 + 10 * L + F)
        self.table = torch.rand(self.geo.table_shape(), generator=g, device=dev) - 0.5
        torch.manual_seed(7 + L * F)
        dec = ColorDecoder(self.geo.width, 64, 3).to(dev)
        default = [p.detach().clone() for p in dec.linear_params()]
        self.decoders = {"default": default, "doubled": [2.0 * p for p in default]}
        self.points = {209: _points(self.size, 209, dev, 11), 5: _points(self.size, 5, dev, 12)}
        self.origin, self.extent = [[0] * self.geo.dim], list(self.size)
        self._data, self._rows = {}, {}

    def data(self, kind, bits):
        """(tensor, kind, num_bits) of a source"""
        from neural_image_compression_v2_amd import hashgrid, models
        if (kind, bits) not in self._data:
            if kind == "f32":
                d = self.table
            else:
                clamped = models.quantize_clamp(self.table, bits)
                d = hashgrid.hash_pack_u8(self.geo, clamped, bits) if kind == "u8" else hashgrid.hash_pack_bits(self.geo, clamped, bits)
            self._data[(kind, bits)] = d
        return self._data[(kind, bits)], kind, bits

    def rows(self, kind, bits, where):
        """the [N, L F] reference row of the existing encode entry; ``where``: "lattice" (the whole field as one crop) or a point count"""
        from neural_image_compression_v2_amd import hashgrid
        key = (kind, bits, where)
        if key not in self._rows:
            d = self.data(kind, bits)[0]
            if where != "lattice":
                x = hashgrid.hash_encode_points(self.geo, d, self.points[where], kind, bits)
            elif kind == "f32":
                x = hashgrid.hash_encode(self.geo, d, self.origin, self.extent)
            elif kind == "u8":
                x = hashgrid.hash_encode_u8(self.geo, d, self.origin, self.extent, bits)
            else:
                x = hashgrid.hash_encode_bits(self.geo, d, self.origin, self.extent, bits)
            self._rows[key] = x
        return self._rows[key]

    def fp32(self, kind, bits, where, params):
        """y of the existing fp32 fused route"""
        from neural_image_compression_v2_amd import hashgrid
        d = self.data(kind, bits)[0]
        if where != "lattice":
            return hashgrid.hash_fused_forward_points(self.geo, d, self.points[where], params, kind, bits)
        if kind == "f32":
            return hashgrid.hash_fused_forward(self.geo, d, self.origin, self.extent, params)
        if kind == "u8":
            return hashgrid.hash_fused_forward_u8(self.geo, d, self.origin, self.extent, bits, params)
        return hashgrid.hash_fused_forward_bits(self.geo, d, self.origin, self.extent, bits, params)

    def p16(self, kind, bits, where, params, mode):
        from neural_image_compression_v2_amd import hashgrid
        d = self.data(kind, bits)[0]
        if where != "lattice":
            return hashgrid.hash_fused_forward_p16(self.geo, d, params, mode, points=self.points[where], kind=kind, num_bits=bits)
        return hashgrid.hash_fused_forward_p16(self.geo, d, params, mode, coord=self.origin, extent=self.extent, kind=kind, num_bits=bits)


@functools.lru_cache(maxsize=None)
def _world(field, L, F, dev):
    return World(field, L, F, dev)


def _bf(v):
    return v.to(torch.bfloat16).to(torch.float32)


def _layer(a, w, b, mode):
    a_hi, w_hi = _bf(a), _bf(w)
    z = a_hi.double() @ w_hi.double().T
    if mode == "split":
        a_lo, w_lo = _bf(a - a_hi), _bf(w - w_hi)
        z = a_lo.double() @ w_hi.double().T + a_hi.double() @ w_lo.double().T + z
    return z.to(torch.float32) + b


def oracle(x, params, mode):
    w1, b1, w2, b2, w3, b3 = params
    a = torch.nn.functional.gelu(_layer(x, w1, b1, mode))
    a = torch.nn.functional.gelu(_layer(a, w2, b2, mode))
    return torch.sigmoid(_layer(a, w3, b3, mode))


@pytest.mark.parametrize("field,L,F", CASES)
def test_against_the_oracle_and_the_fp32_route(dev, field, L, F):
    """every source x decoder x mode, on the lattice and at both point sets: the four bounds of the module docstring; every y finite"""
    w = _world(field, L, F, dev)
    worst = {}
    for kind, bits in SOURCES:
        for where in ("lattice", 209, 5):
            x = w.rows(kind, bits, where)
            for dname, params in w.decoders.items():
                y32 = w.fp32(kind, bits, where, params)
                for mode in MODES:
                    y = w.p16(kind, bits, where, params, mode)
                    assert y.shape == y32.shape and bool(torch.isfinite(y).all()), (kind, bits, where, dname, mode)
                    e_or, e_32 = absmax(y, oracle(x, params, mode)), absmax(y, y32)
                    for k, e in ((("oracle", mode, dname), e_or), (("fp32", mode, dname), e_32)):
                        worst[k] = max(worst.get(k, 0.0), e)
                    tag = f"{field} L={L} F={F} {kind}/{bits} {where} {dname} {mode}"
                    print(f"{tag}: vs oracle {e_or:.3e}, vs fp32 route {e_32:.3e}")
                    if mode == "split":
                        assert e_or <= TOL_SPLIT, f"{tag}: split against its oracle {e_or:.3e} > {TOL_SPLIT:.0e}"
                        assert e_32 <= TOL_SPLIT, f"{tag}: split against the fp32 route {e_32:.3e} > {TOL_SPLIT:.0e}"
                    else:
                        assert e_or <= TOL_BF16, f"{tag}: bf16 against its oracle {e_or:.3e} > {TOL_BF16:.0e}"
                        if dname == "default":
                            assert e_32 <= TOL_BF16, f"{tag}: bf16 against the fp32 route {e_32:.3e} > {TOL_BF16:.0e}"
    print(f"worst {field} L={L} F={F}:", {" ".join(k): f"{v:.3e}" for k, v in sorted(worst.items())})


@pytest.mark.parametrize("field,L,F", CASES)
def test_exact_pins_of_the_entry(dev, field, L, F):
    """the same call twice (no atomics); the uint8 source against an f32 table of its dequantised values; a y with 64 extra sentinel rows:
    rows >= N stay untouched, and points outside the field (NaN included) give the rows of the clamped points"""
    from neural_image_compression_v2_amd import _lib, fused, hashgrid
    w = _world(field, L, F, dev)
    params = w.decoders["default"]
    for mode in MODES:
        for kind, bits in SOURCES:
            for where in ("lattice", 209):
                assert torch.equal(w.p16(kind, bits, where, params, mode), w.p16(kind, bits, where, params, mode)), (mode, kind, bits, where)
        for bits in (8, 5):
            stored = w.data("u8", bits)[0]
            deq = hashgrid._table_of_u8(w.geo, stored, bits)
            for where in ("lattice", 209, 5):
                y_u8 = w.p16("u8", bits, where, params, mode)
                if where == "lattice":
                    y_f = hashgrid.hash_fused_forward_p16(w.geo, deq, params, mode, coord=w.origin, extent=w.extent)
                else:
                    y_f = hashgrid.hash_fused_forward_p16(w.geo, deq, params, mode, points=w.points[where])
                assert torch.equal(y_u8, y_f), (mode, bits, where)
        for n in (209, 5):
            pts = w.points[n]
            y = torch.full((n + 64, 3), -77.0, dtype=torch.float32, device=dev)
            src, data = hashgrid._point_source(w.geo, w.table, "f32", None)
            d, m = hashgrid._point_desc(w.geo), fused._mlp_struct(params)
            with torch.cuda.device(dev):
                _lib.check(_lib.load().nic_hash_fused_forward_p16(ctypes.byref(d), ctypes.byref(src), None, _lib.ptr(pts), n, ctypes.byref(m),
                                                                  hashgrid.PRECISIONS[mode], _lib.ptr(y), _lib.stream_ptr(dev)), "p16")
            assert bool((y[n:] == -77.0).all()), (mode, n)
            assert torch.equal(y[:n], w.p16("f32", None, n, params, mode))
            y_clamped = hashgrid.hash_fused_forward_p16(w.geo, w.table, params, mode, points=_clamped(w.size, pts))
            assert torch.equal(y[:n], y_clamped), (mode, n)
    assert hashgrid.hash_fused_forward_p16(w.geo, w.table, params, "split", points=torch.zeros(0, w.geo.dim, device=dev)).shape == (0, 3)


def _field(field, L, F, dev, num_bits=None, fused_route=False):
    """a HashGridField of the shape with a table uniform in [-1/2, 1/2] (clamped into the quantiser's range with ``num_bits``)"""
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    spec = FIELDS[field]
    f = HashGridField(spec["size"], levels=L, features=F, log2_table=spec["log2_table"], base_resolution=spec["base"], device=dev, seed=5,
                      num_bits=num_bits, fused=fused_route)
    with torch.no_grad():
        g = torch.Generator(device=dev).manual_seed(99)
        f.table.copy_(torch.rand(f.table.shape, generator=g, device=dev) - 0.5)
        if num_bits is not None:
            f.table.copy_(models.quantize_clamp(f.table, num_bits))
    return f


def _centres(size, dev):
    axes = [torch.arange(s, dtype=torch.float32, device=dev) for s in size]
    return torch.stack([g.reshape(-1) for g in torch.meshgrid(*axes, indexing="ij")], dim=1).contiguous()


@pytest.mark.parametrize("field,L,F", [("2d", 16, 2), ("2d", 10, 4), ("3d", 12, 2), ("3d", 8, 8)])
def test_exact_pins_of_the_field(dev, tmp_path, field, L, F):
    """decode against query at the sample centres, decode in tiles of 16, resample at the field size; a packed /1 file against the uint8 file
    of the same field (b = 5: straddling entries), both decoded from the loaded table; on both routes of the field"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    for route in (False, True):
        f = _field(field, L, F, dev, num_bits=5, fused_route=route)
        size = f.field_size
        p_u8, p_bits = os.path.join(str(tmp_path), f"u8_{route}.pt"), os.path.join(str(tmp_path), f"bits_{route}.pt")
        f.save_compressed(p_u8)
        f.save_compressed(p_bits, packed=True)
        f_u8 = HashGridField.load_compressed(p_u8, device=dev, fused=route)
        f_bits = HashGridField.load_compressed(p_bits, device=dev, fused=route)
        assert f_u8.stored is not None and f_bits.packed is not None and f_u8.table is None and f_bits.table is None
        for mode in MODES:
            for g in (f, f_u8, f_bits):
                full = g.decode(precision=mode)
                assert full.shape == (*size, 3) and bool(torch.isfinite(full).all())
                assert torch.equal(full, g.query(_centres(size, dev), precision=mode).reshape(*size, 3)), (route, mode)
                assert torch.equal(full, g.decode(tile=16, precision=mode)), (route, mode)
                assert torch.equal(full, g.resample(size, precision=mode)), (route, mode)
                assert torch.equal(full, g.resample(size, tile=16, precision=mode)), (route, mode)
            assert torch.equal(f_u8.decode(precision=mode), f_bits.decode(precision=mode)), (route, mode)


@pytest.mark.parametrize("field,L,F", [("2d", 16, 2), ("3d", 10, 4)])
def test_the_default_is_todays_routes(dev, field, L, F):
    """without the argument every method makes the launches it made: decode / query / resample against the entry points they always called"""
    from neural_image_compression_v2_amd import fused, hashgrid
    for route in (False, True):
        f = _field(field, L, F, dev, fused_route=route)
        size, geo, table = f.field_size, f.geo, f.table.detach()
        params = [p.detach() for p in f.decoder.linear_params()]
        pts = _points(size, 209, dev, 3)
        org, ext = [[0] * geo.dim], list(size)
        if route:
            want_dec = hashgrid.hash_fused_forward(geo, table, org, ext, params).reshape(*size, 3)
            want_q = hashgrid.hash_fused_forward_points(geo, table, pts, params)
        else:
            want_dec = fused.DecoderFunction.apply(hashgrid.hash_encode(geo, table, org, ext), *params).reshape(*size, 3)
            want_q = fused.DecoderFunction.apply(hashgrid.hash_encode_points(geo, table, pts), *params)
        assert f.route == ("fused" if route else "layerwise")
        assert torch.equal(f.decode(), want_dec) and torch.equal(f.query(pts), want_q)
        assert torch.equal(f.resample(size), f.query(_centres(size, dev)).reshape(*size, 3))


def test_precision_none_is_the_default(dev):
    f = _field("2d", 16, 2, dev, fused_route=True)
    pts = _points(f.field_size, 209, dev, 3)
    assert torch.equal(f.decode(precision=None), f.decode()) and torch.equal(f.query(pts, precision=None), f.query(pts))
    assert torch.equal(f.resample((20, 30), precision=None), f.resample((20, 30)))
    assert torch.equal(f.query(pts, lod=1.0, precision=None), f.query(pts, lod=1.0))


def test_refusals_leave_the_field_untouched(dev):
    """an unknown precision, a level of detail, a bit depth per level, a geometry outside the fused set: raised before anything is launched,
    with the table, its gradient, the step count and a pass in progress as they were"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    f = _field("2d", 16, 2, dev)
    size = f.field_size
    g = torch.Generator(device=dev).manual_seed(4)
    target = torch.rand(16 * size[1], 3, generator=g, device=dev)
    f.train_step([[0, 0]], (16, size[1]), target)                                              # one whole step
    f.train_step([[0, 0]], (16, size[1]), target, scale=0.5, step=False)                      # a pass in progress
    torch.cuda.synchronize()
    state = (f.table.detach().clone(), f.table.grad.clone(), f.steps, f._pass_samples, [p.detach().clone() for p in f.decoder.parameters()])
    assert state[2] == 1 and state[3] == 16 * size[1] and float(state[1].abs().max()) > 0
    pts = _points(size, 209, dev, 3)
    for bad in ("fp16", "SPLIT", "", 1):
        for call in (lambda: f.decode(precision=bad), lambda: f.query(pts, precision=bad), lambda: f.resample(size, precision=bad)):
            with pytest.raises(ValueError, match="precision"):
                call()
    for mode in MODES:
        for call in (lambda: f.query(pts, lod=1.0, precision=mode), lambda: f.resample((22, 18), lod="auto", precision=mode),
                     lambda: f.resample((22, 18), lod=1.0, precision=mode)):
            with pytest.raises(NotImplementedError):
                call()
    torch.cuda.synchronize()
    assert torch.equal(f.table.detach(), state[0]) and torch.equal(f.table.grad, state[1]) and (f.steps, f._pass_samples) == state[2:4]
    assert all(torch.equal(a.detach(), b) for a, b in zip(f.decoder.parameters(), state[4]))
    mixed = HashGridField((44, 37), levels=4, features=2, log2_table=10, device=dev, seed=5, num_bits=[8, 5, 3, 4])
    wide = HashGridField((44, 37), levels=9, features=8, log2_table=10, device=dev, seed=5)
    deep = HashGridField((44, 37), levels=4, features=2, log2_table=10, device=dev, seed=5, n_linear=5)
    for mode in MODES:
        before = mixed.table.detach().clone()
        with pytest.raises(NotImplementedError):
            mixed.decode(precision=mode)
        with pytest.raises(NotImplementedError):
            mixed.query(pts, precision=mode)
        assert torch.equal(mixed.table.detach(), before) and mixed.steps == 0
        for h in (wide, deep):
            with pytest.raises(ValueError, match="fused set"):
                h.decode(precision=mode)
            with pytest.raises(ValueError, match="fused set"):
                h.query(pts, precision=mode)
            with pytest.raises(ValueError, match="fused set"):
                h.resample((8, 8), precision=mode)
    with pytest.raises(NotImplementedError):
        HashGridField((64, 48), levels=4, features=2, log2_table=10, device=dev, seed=5).decode_mip(1, precision="split")
