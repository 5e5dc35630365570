"""CPU-only tests of the batched decode from stored tables and at points (run with -m "not gpu"): nic_hash_batch_forward_source is
exported, declared and mirrored with the same argument list and the ABI version stays 9; every argument error of the entry is decided on the host
in the documented order (fake pointers and refusals only: nothing launches; a launch at no points is NIC_OK); a packed table is a whole number of
dwords at every depth, so every field of an aligned stack is aligned; and ``hash_batch_forward_source`` / ``HashGridFieldBatch.load_compressed``
and a decode-only batch refuse on the host, before a device is touched and before anything is set."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
NAME = "nic_hash_batch_forward_source"
OK, NULL, UNSUP, SHAPE, WORKSPACE, ARG = 0, -1, -2, -3, -4, -5
F32, U8, BITS = 0, 1, 2
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_v2_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.load()


def _desc(dim=2, resolutions=(16,) * 8, features=2, log2_table=12, s_max=256, num_crops=1, extent=(256, 256, 1)):
    from neural_image_compression_v2_amd._lib import NicHashDesc
    d = NicHashDesc()
    d.dim, d.levels, d.features, d.log2_table, d.S_max, d.num_crops = dim, len(resolutions), features, log2_table, s_max, num_crops
    for a in range(3):
        d.extent[a] = extent[a]
    for l, r in enumerate(resolutions):
        d.resolution[l] = r
    return d


def _mlp(n_linear=3, layers=3):
    from neural_image_compression_v2_amd._lib import NicMlp
    m = NicMlp()
    m.n_linear = n_linear
    for i in range(layers):
        m.w[i] = m.b[i] = 16
    return m


def _src(kind=U8, bits=8, data=16):
    from neural_image_compression_v2_amd._lib import NicHashSource
    return NicHashSource(kind, bits, data)


def _ref(x):
    return None if x is None else ctypes.byref(x)


def _call(lib, d, n_fields=2, groups=0, src="default", origins=0, points=16, n_points=0, m="default", y=16):
    """the return code of the entry; every pointer is a dummy that is never dereferenced.  An accepted call with origins, or with points and
    n_points > 0, would launch: only refusals and n_points == 0 are tried"""
    m = _mlp() if m == "default" else m
    src = _src() if src == "default" else src
    return lib.nic_hash_batch_forward_source(_ref(d), n_fields, groups, _ref(src), P(origins), P(points), n_points, _ref(m), P(y), None)


def test_the_entry_is_exported_declared_and_mirrored(lib):
    from neural_image_compression_v2_amd import _lib, hashgrid
    import neural_image_compression_v2_amd as pkg
    header = open(HEADER).read()
    assert hasattr(lib, NAME) and NAME in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[NAME]
    m = re.search(rf"\b{NAME}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m
    cargs = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(cargs) == len(args) == 10 and res is ctypes.c_int, cargs
    for c, a in zip(cargs, args):
        if "*" in c:
            assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), c
        else:
            assert a is {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[c.split()[0]], c
    assert _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version() and re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)      # additive
    assert len(_lib.SIGNATURES) == 86 and all(re.search(rf"\b{n}\s*\(", header) and hasattr(lib, n) for n in _lib.SIGNATURES)      # 85 + this one
    assert pkg.hash_batch_forward_source is hashgrid.hash_batch_forward_source
    import inspect
    assert list(inspect.signature(hashgrid.hash_batch_forward_source).parameters) == [
        "geo", "data", "params", "kind", "num_bits", "coord", "extent", "points", "groups_per_field", "out"]
    assert list(inspect.signature(hashgrid.HashGridFieldBatch.load_compressed).parameters) == ["paths", "device", "groups_per_field"]
    for name in ("query", "resample", "decode", "extract", "save_compressed"):
        assert callable(getattr(hashgrid.HashGridFieldBatch, name))


def test_argument_errors_in_the_documented_order(lib):
    d = _desc()
    assert _call(lib, d) == OK                                           # points, n_points == 0: every check passes, nothing launches
    # 1. null desc / mlp, whatever else is wrong
    assert _call(lib, None) == NULL and _call(lib, d, m=None) == NULL
    assert _call(lib, None, n_fields=0, groups=3, src=None, origins=16) == NULL
    # 2. the fused set: before the position pair, n_fields, the groups and every pointer
    bad = _desc()
    bad.flags = 1
    wide = _desc(resolutions=(16,) * 9, features=8)                       # L F = 72
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (_desc(extent=(257, 8, 1)), SHAPE),
                       (_desc(num_crops=0), SHAPE), (wide, UNSUP)]:
        assert _call(lib, desc) == want
        assert _call(lib, desc, origins=16) == want and _call(lib, desc, points=0) == want
        assert _call(lib, desc, n_fields=0, groups=3, src=None, y=0) == want
    assert _call(lib, d, m=_mlp(5, 5)) == UNSUP and _call(lib, d, m=_mlp(5, 5), origins=16, n_fields=0) == UNSUP
    # 3. exactly one of origins / points: before the descriptor of the position, n_fields, the groups, the pointers and the source
    two = _desc(num_crops=2)
    for kw in (dict(origins=16, points=16), dict(origins=0, points=0)):
        assert _call(lib, d, **kw) == ARG
        assert _call(lib, two, **kw) == ARG
        assert _call(lib, d, n_fields=0, groups=3, src=None, y=0, n_points=-1, **kw) == ARG
    # 4. the descriptor of that position: points need one crop (SHAPE); both routes need 256 S_max < 2^30 (ARG)
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    assert _call(lib, two) == SHAPE and _call(lib, two, n_fields=0, groups=3, src=None) == SHAPE
    assert _call(lib, two, origins=16, points=0, src=None) == NULL       # the lattice takes several crops: on to the pointers
    assert _call(lib, big) == ARG and _call(lib, big, origins=16, points=0) == ARG
    # 5. n_fields
    for n in (0, -1, 65536, 1 << 30):
        assert _call(lib, d, n_fields=n) == ARG and _call(lib, d, n_fields=n, groups=3, src=None, y=0) == ARG
        assert _call(lib, d, n_fields=n, origins=16, points=0) == ARG
    assert _call(lib, d, n_fields=65535) == OK
    # 6. groups_per_field: 0, or a multiple of 8 up to the grid of one field's wave items - its patches, or ceil(n_points / 64)
    for g in (-8, -1, 1, 4, 12, 1 << 20):
        assert _call(lib, d, groups=g) == ARG and _call(lib, d, groups=g, src=None, y=0) == ARG, g
        assert _call(lib, d, groups=g, origins=16, points=0, src=None) == ARG, g
    small = _desc(extent=(16, 16, 1))                                     # 4 patches: one group of four, a grid of 8
    assert _call(lib, small, groups=16, origins=16, points=0, src=None) == ARG
    assert _call(lib, small, groups=8, origins=16, points=0, src=None) == NULL
    assert _call(lib, d, groups=16, n_points=130, src=None) == ARG        # 3 wave items: a grid of 8
    assert _call(lib, d, groups=8, n_points=130, src=None) == NULL
    assert _call(lib, d, groups=16, n_points=64 * 4 * 9, src=None) == NULL      # 9 groups of four: a grid of 16
    assert _call(lib, d, groups=8, n_points=0) == OK and _call(lib, d, groups=16, n_points=0) == ARG      # no points count as one item here
    # 7. null pointers: the source, its data, a decoder layer, y - before the source's own rules and n_points
    for kw in (dict(src=None), dict(src=_src(data=0)), dict(y=0), dict(m=_mlp(3, 2))):
        assert _call(lib, d, **kw) == NULL, kw
        assert _call(lib, d, n_points=-1, **kw) == NULL, kw
        assert _call(lib, d, origins=16, points=0, **kw) == NULL, kw
    assert _call(lib, d, src=_src(U8, 0, 0)) == NULL and _call(lib, d, src=_src(BITS, 9, 0)) == NULL
    # 8. the source: nic_hash_encode_points' rules, before n_points (a bad source at no points is still refused)
    for s in (_src(U8, 0), _src(U8, 9), _src(BITS, 0), _src(BITS, 9), _src(U8, -1), _src(F32, 8), _src(F32, 1), _src(7, 8), _src(-1, 0), _src(BITS, 4, 18),
              _src(BITS, 8, 17)):
        assert _call(lib, d, src=s) == ARG, (s.kind, s.num_bits, s.data)
        assert _call(lib, d, src=s, origins=16, points=0) == ARG, (s.kind, s.num_bits, s.data)
    for s in (_src(U8, 1), _src(U8, 8, 17), _src(BITS, 1), _src(BITS, 8, 20), _src(F32, 0), _src(F32, 0, 18)):
        assert _call(lib, d, src=s) == OK, (s.kind, s.num_bits, s.data)
    # 9. n_points < 0, then n_points == 0: NIC_OK with no launch (the pointers are fakes: a launch would fault)
    for n in (-1, -64, -(1 << 40)):
        assert _call(lib, d, n_points=n) == ARG
    for desc in (d, _desc(dim=3, resolutions=(4, 6, 9, 12), features=1, s_max=12, extent=(12, 10, 9))):
        for s in (_src(F32, 0), _src(U8, 8), _src(BITS, 3)):
            assert _call(lib, desc, src=s, n_points=0) == OK


def test_every_field_of_an_aligned_packed_stack_is_aligned(lib):
    for desc in (_desc(resolutions=(16, 21, 27, 36), features=2, log2_table=10, s_max=40, extent=(40, 36, 1)),
                 _desc(resolutions=(16, 23, 33, 47, 68, 97, 139, 200), features=1),
                 _desc(dim=3, resolutions=(4, 6, 9, 12), features=1, log2_table=10, s_max=12, extent=(12, 10, 9)),
                 _desc(dim=3, resolutions=(4, 7, 13, 24), features=8, log2_table=11, s_max=24, extent=(24, 24, 24))):
        for b in range(1, 9):
            n = lib.nic_hash_packed_bytes(_ref(desc), b)
            assert n > 8 and n % 4 == 0, (desc.dim, desc.features, b, n)      # the stride of a stack: field b starts on a dword


def _geo(size=(40, 36), levels=4, features=2, log2_table=10):
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, level_resolutions
    return HashGeometry(size, tuple(level_resolutions(levels, 16, max(size))), features, log2_table)


def _params(geo, b=3):
    lf = geo.width
    return [torch.zeros(b, 64, lf), torch.zeros(b, 64), torch.zeros(b, 64, 64), torch.zeros(b, 64), torch.zeros(b, 3, 64), torch.zeros(b, 3)]


def test_the_wrapper_checks_shapes_and_dtypes_before_a_device():
    from neural_image_compression_v2_amd import hashgrid
    geo = _geo()
    params = _params(geo)
    nu8, nb4 = hashgrid.hash_stored_bytes(geo), hashgrid.hash_packed_bytes(geo, 4)
    tables, stored, packed = torch.zeros(3, *geo.table_shape()), torch.zeros(3, nu8, dtype=torch.uint8), torch.zeros(3, nb4, dtype=torch.uint8)
    coord, extent = [[0, 0], [20, 24]], (20, 12)
    fs = hashgrid.hash_batch_forward_source
    # the source kind and its num_bits
    with pytest.raises(ValueError, match="source"):
        fs(geo, tables, params, "fp16", coord=coord, extent=extent)
    with pytest.raises(ValueError, match="num_bits"):
        fs(geo, tables, params, "f32", 8, coord=coord, extent=extent)
    for kind, data in (("u8", stored), ("bits", packed)):
        for bits in (None, 0, 9, [4] * 4):
            with pytest.raises(ValueError, match="num_bits"):
                fs(geo, data, params, kind, bits, coord=coord, extent=extent)
    with pytest.raises(TypeError):
        fs(geo, None, params, "u8", 8, coord=coord, extent=extent)
    # data: fp32 [B, L, T, F], or uint8 [B, bytes of one field at this depth]
    for bad in (tables[0], torch.zeros(3, 4, 512, 2), torch.zeros(0, 4, 1024, 2), tables.double(), stored):
        with pytest.raises(ValueError, match="data"):
            fs(geo, bad, params, "f32", coord=coord, extent=extent)
    for bad in (stored[0], stored[:, :-1], torch.zeros(3, nu8 + 1, dtype=torch.uint8), stored.to(torch.int8), stored.float(), torch.zeros(0, nu8, dtype=torch.uint8),
                packed):
        with pytest.raises(ValueError, match="data"):
            fs(geo, bad, params, "u8", 8, coord=coord, extent=extent)
    for bad in (packed[0], packed.reshape(-1), stored, torch.zeros(3, hashgrid.hash_packed_bytes(geo, 5), dtype=torch.uint8), packed.to(torch.int32)):
        with pytest.raises(ValueError, match="data"):
            fs(geo, bad, params, "bits", 4, coord=coord, extent=extent)
    # the decoder: six fp32 tensors stacked like the tables
    for k, shape in enumerate([(3, 64, 9), (3, 32), (3, 64, 32), (2, 64), (3, 64, 3), (3,)]):
        bad = list(params)
        bad[k] = torch.zeros(*shape)
        with pytest.raises(ValueError, match="params"):
            fs(geo, stored, bad, "u8", 8, coord=coord, extent=extent)
    with pytest.raises(ValueError, match="params"):
        fs(geo, stored, [p[:1] for p in params], "u8", 8, coord=coord, extent=extent)
    with pytest.raises(ValueError, match="params"):
        fs(geo, stored, [p.double() for p in params], "u8", 8, coord=coord, extent=extent)
    # exactly one position source
    pts = torch.zeros(7, 2)
    with pytest.raises(ValueError, match="exactly one"):
        fs(geo, stored, params, "u8", 8)
    with pytest.raises(ValueError, match="exactly one"):
        fs(geo, stored, params, "u8", 8, coord=coord, extent=extent, points=pts)
    with pytest.raises(ValueError, match="extent"):
        fs(geo, stored, params, "u8", 8, coord=coord)
    with pytest.raises(ValueError, match="extent"):
        fs(geo, stored, params, "u8", 8, points=pts, extent=extent)
    with pytest.raises(IndexError):
        fs(geo, stored, params, "u8", 8, coord=[[21, 0]], extent=extent)
    with pytest.raises(ValueError, match="origins"):
        fs(geo, stored, params, "u8", 8, coord=torch.zeros(2, 1, 2, dtype=torch.int64), extent=extent)
    for bad in (torch.zeros(7), torch.zeros(7, 3), torch.zeros(2, 7, 2), torch.zeros(3, 7, 3), torch.zeros(7, 2, dtype=torch.float64), torch.zeros(1, 3, 7, 2),
                [[0.0, 0.0]]):
        with pytest.raises(ValueError, match="points"):
            fs(geo, stored, params, "u8", 8, points=bad)
    # out: [B, N, 3] fp32 contiguous
    for bad in (torch.zeros(3, 7, 4), torch.zeros(2, 7, 3), torch.zeros(3, 7, 3, dtype=torch.float64), torch.zeros(7, 3)):
        with pytest.raises(ValueError, match="out"):
            fs(geo, stored, params, "u8", 8, points=pts, out=bad)
    with pytest.raises(ValueError, match="out"):
        fs(geo, stored, params, "u8", 8, coord=coord, extent=extent, out=torch.zeros(3, 7, 3))
    # with everything shaped right the refusal is the device's: nothing was launched
    for kind, data, bits in (("f32", tables, None), ("u8", stored, 8), ("bits", packed, 4)):
        with pytest.raises(RuntimeError, match="HIP device"):
            fs(geo, data, params, kind, bits, coord=coord, extent=extent)
        with pytest.raises(RuntimeError, match="HIP device"):
            fs(geo, data, params, kind, bits, points=torch.zeros(3, 7, 2))


def _file(path, size=(40, 36), levels=4, features=2, log2_table=10, num_bits=8, packed=False, hidden=64, n_linear=3, fmt=None, table=None, level_bits=None):
    """a save_compressed file made by hand on the CPU (zero table, default decoder)"""
    from neural_image_compression_v2_amd import hashgrid
    from neural_image_compression_v2_amd.image_compression import ColorDecoder
    geo = _geo(size, levels, features, log2_table)
    need = hashgrid.hash_packed_bytes(geo, level_bits if level_bits is not None else num_bits) if packed else hashgrid.hash_stored_bytes(geo)
    d = {"format": fmt if fmt is not None else (hashgrid.PACKED_FORMAT if packed else hashgrid.COMPRESSED_FORMAT), "field_size": list(size),
         "resolutions": list(geo.resolutions), "features": features, "log2_table": log2_table, "num_bits": num_bits, "hidden": hidden, "n_linear": n_linear,
         "table": torch.zeros(need, dtype=torch.uint8) if table is None else table,
         "decoder": {k: v.detach() for k, v in ColorDecoder(geo.width, hidden, n_linear).state_dict().items()}}
    if level_bits is not None:
        d["level_bits"] = list(level_bits)
    torch.save(d, path)
    return str(path)


def test_load_compressed_refuses_on_the_host(tmp_path):
    from neural_image_compression_v2_amd import hashgrid
    load = hashgrid.HashGridFieldBatch.load_compressed
    a, a2 = _file(tmp_path / "a.pt"), _file(tmp_path / "a2.pt")
    with pytest.raises(ValueError, match="no paths"):
        load([], device="cpu")
    for g in (4, -8, 12):
        with pytest.raises(ValueError, match="groups_per_field"):
            load([a, a2], device="cpu", groups_per_field=g)
    # every file must agree with the first: the error names the first path that differs
    others = {"geometry": [_file(tmp_path / "size.pt", size=(40, 40)), _file(tmp_path / "t.pt", log2_table=11), _file(tmp_path / "lv.pt", levels=5),
                           _file(tmp_path / "f.pt", features=4)],
              "num_bits": [_file(tmp_path / "bits.pt", num_bits=4)],
              "format": [_file(tmp_path / "packed.pt", packed=True)],
              "decoder shape": [_file(tmp_path / "h.pt", hidden=32), _file(tmp_path / "n.pt", n_linear=5)]}
    for what, files in others.items():
        for other in files:
            with pytest.raises(ValueError, match=f"its {what}") as e:
                load([a, a2, other, _file(tmp_path / "later.pt", size=(8, 8))], device="cpu")
            assert os.path.basename(other) in str(e.value) and "later.pt" not in str(e.value)
    # a bit depth per level: read, and not built
    mixed = _file(tmp_path / "mixed.pt", packed=True, num_bits=None, level_bits=(4, 4, 8, 8), fmt=hashgrid.MIXED_FORMAT)
    for paths in ([mixed], [a, mixed]):
        with pytest.raises(NotImplementedError, match="mixed.pt"):
            load(paths, device="cpu")
    # outside what the batched kernels decode
    with pytest.raises(ValueError, match="hidden"):
        load([_file(tmp_path / "h32.pt", hidden=32)], device="cpu")
    with pytest.raises(ValueError, match="n_linear"):
        load([_file(tmp_path / "n5.pt", n_linear=5)], device="cpu")
    with pytest.raises(ValueError, match="fused set"):
        load([_file(tmp_path / "wide.pt", levels=9, features=8, log2_table=12)], device="cpu")            # L F = 72
    # not such a file, a bad depth, a table of the wrong size
    torch.save({"format": "something/1"}, tmp_path / "other.pt")
    with pytest.raises(ValueError, match="other.pt"):
        load([a, str(tmp_path / "other.pt")], device="cpu")
    with pytest.raises(ValueError, match="num_bits"):
        load([_file(tmp_path / "b9.pt", num_bits=9)], device="cpu")
    with pytest.raises(ValueError, match="short.pt"):
        load([a, _file(tmp_path / "short.pt", table=torch.zeros(5, dtype=torch.uint8))], device="cpu")
    # files that agree: the refusal is the device's
    with pytest.raises(RuntimeError, match="HIP device"):
        load([a, a2], device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        load([_file(tmp_path / "p1.pt", packed=True, num_bits=4), _file(tmp_path / "p2.pt", packed=True, num_bits=4)], device="cpu", groups_per_field=8)


def test_a_decode_only_batch_refuses_to_train():
    from neural_image_compression_v2_amd.hashgrid import HashGridField, HashGridFieldBatch, hash_stored_bytes
    geo = _geo()
    f = HashGridFieldBatch.__new__(HashGridFieldBatch)
    f.n_fields, f.field_size, f.device, f.num_bits, f.frozen, f.geo = 3, (40, 36), torch.device("cpu"), 8, True, geo
    f.groups_per_field, f.steps, f.noise_seed, f._pass_samples, f._grad_clean = 0, 0, 0, 0, True
    f.tables, f.packed, f.stored = None, None, torch.zeros(3, hash_stored_bytes(geo), dtype=torch.uint8)
    f.params, f.optimizer, f.scheduler, f._gm = _params(geo), None, None, None
    assert f.decode_only
    before = dict(f.__dict__)
    n = 20 * 12
    single = HashGridField.__new__(HashGridField)
    with pytest.raises(RuntimeError, match="decode-only"):
        f.train_step([[0, 0]], (20, 12), torch.zeros(3, n, 3))
    with pytest.raises(RuntimeError, match="decode-only"):
        f.train_step([[99, 0]], (20, 12), None)                          # before the crops and the target are looked at
    with pytest.raises(RuntimeError, match="decode-only"):
        f.fit(torch.zeros(3, 40, 36, 3), 3)
    with pytest.raises(RuntimeError, match="decode-only"):
        f.freeze()
    for b in (0, 7):
        with pytest.raises(RuntimeError, match="decode-only"):
            f.insert(b, single)
    with pytest.raises(RuntimeError, match="decode-only"):
        f.apply_step()
    for b in (-1, 3):
        with pytest.raises(IndexError):
            f.extract(b)
    with pytest.raises(ValueError, match="paths"):
        f.save_compressed(["a", "b"])
    with pytest.raises(ValueError, match="size"):
        f.resample((32, 32, 32))
    assert f.__dict__.keys() == before.keys() and all(f.__dict__[k] is before[k] for k in before)       # nothing was set on the way to a refusal
    # a batch that holds fp32 tables is not decode-only: the refusals it always made come first
    f.tables, f.num_bits = torch.zeros(1), None
    assert not f.decode_only
    with pytest.raises(RuntimeError, match="num_bits"):
        f.freeze()
