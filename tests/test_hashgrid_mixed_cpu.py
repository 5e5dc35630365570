"""CPU-only tests of the hash-grid codec with a bit depth per level (run with -m "not gpu"): the six new C ABI symbols are exported, declared
and mirrored, the ABI version stays 9, ``nic_hash_packed_bytes_levels`` is the header's formula, every argument error of the new entry points is
decided on the host (fake pointers, nothing launches), and ``load_compressed`` refuses a bad format /2 file before it touches a device."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
NEW_SYMBOLS = ("nic_hash_packed_bytes_levels", "nic_hash_pack_bits_levels", "nic_hash_clamp_levels", "nic_hash_encode_levels",
               "nic_hash_fused_forward_levels", "nic_hash_fused_forward_backward_levels")
OK, NULL, UNSUP, SHAPE, WORKSPACE, ARG = 0, -1, -2, -3, -4, -5
P = ctypes.c_void_p
F32, U8, BITS = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_v2_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.load()


def _desc(dim=2, resolutions=(16, 64), features=2, log2_table=12, s_max=256, num_crops=1, extent=(256, 256, 1)):
    from neural_image_compression_v2_amd._lib import NicHashDesc
    d = NicHashDesc()
    d.dim, d.levels, d.features, d.log2_table, d.S_max, d.num_crops = dim, len(resolutions), features, log2_table, s_max, num_crops
    for a in range(3):
        d.extent[a] = extent[a]
    for l, r in enumerate(resolutions):
        d.resolution[l] = r
    return d


def _lb(bits):
    from neural_image_compression_v2_amd._lib import NicHashLevelBits
    lb = NicHashLevelBits()
    for l, b in enumerate(bits):
        lb.bits[l] = b
    return lb


def _src(kind=F32, num_bits=0, data=16):
    from neural_image_compression_v2_amd._lib import NicHashSource
    return NicHashSource(kind, num_bits, data)


def _quant(mode=2, base=0):
    from neural_image_compression_v2_amd._lib import NicHashQuant
    return NicHashQuant(0, mode, 1, 2, base)


def _mlp(n_linear=3, layers=3):
    from neural_image_compression_v2_amd._lib import NicMlp
    m = NicMlp()
    m.n_linear = n_linear
    for i in range(layers):
        m.w[i] = m.b[i] = 16
    return m


def _grads(base=0x1000):
    from neural_image_compression_v2_amd._lib import NicMlpGrads
    g = NicMlpGrads()
    for i in range(3):
        g.w[i], g.b[i] = base + 0x100 * i, base + 0x100 * i + 0x80
    return g


def _ref(x):
    return None if x is None else ctypes.byref(x)


def _enc(lib, d, lb, src="default", q=None, origins=0, points=16, n=0, out=16):
    src = _src() if src == "default" else src
    return lib.nic_hash_encode_levels(_ref(d), _ref(lb), _ref(src), _ref(q), P(origins), P(points), n, P(out), None)


def _fwd(lib, d, lb, src="default", origins=0, points=16, n=0, m="default", y=16):
    src = _src() if src == "default" else src
    m = _mlp() if m == "default" else m
    return lib.nic_hash_fused_forward_levels(_ref(d), _ref(lb), _ref(src), P(origins), P(points), n, _ref(m), P(y), None)


def _fb(lib, d, lb, q=None, table=16, origins=0, points=16, n=0, order=0, m="default", target=16, tg=16, gs="default", loss=16, y=0, flags=0, ws=16,
        ws_bytes=1 << 30, tail=None):
    m = _mlp() if m == "default" else m
    gs = _grads() if gs == "default" else gs
    return lib.nic_hash_fused_forward_backward_levels(_ref(d), _ref(lb), _ref(q), P(table), P(origins), P(points), n, P(order), _ref(m), P(target), 1.0,
                                                      P(tg), _ref(gs), P(loss), P(y), flags, P(ws), ws_bytes, _ref(tail), None)


def _pack(lib, d, lb, table=16, packed=16):
    return lib.nic_hash_pack_bits_levels(_ref(d), _ref(lb), P(table), P(packed), None)


def _clamp(lib, d, lb, table=16):
    return lib.nic_hash_clamp_levels(_ref(d), _ref(lb), P(table), None)


def _c_args(header, name):
    m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        out.append(re.sub(r"\s*\w+$", "", a) if not a.endswith("*") else a)
    return out


def test_new_symbols_are_exported_declared_and_mirrored(lib):
    from neural_image_compression_v2_amd import _build, _lib, hashgrid
    header = open(HEADER).read()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
        assert re.search(rf"\b{n}\s*\(", header), n
    assert _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version()                  # additive: the version stays
    assert re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)
    assert "hash_mixed.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "hash_mixed.hip"))
    assert ctypes.sizeof(_lib.NicHashLevelBits) == 128
    assert re.search(r"typedef struct nic_hash_level_bits \{\s*int32_t bits\[NIC_HASH_MAX_LEVELS\];\s*\} nic_hash_level_bits;", header)
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    structs = {"nic_hash_desc": _lib.NicHashDesc, "nic_hash_quant": _lib.NicHashQuant, "nic_mlp": _lib.NicMlp, "nic_mlp_grads": _lib.NicMlpGrads,
               "nic_step_tail": _lib.NicStepTail, "nic_hash_level_bits": _lib.NicHashLevelBits, "nic_hash_source": _lib.NicHashSource}
    for n in NEW_SYMBOLS:
        res, args = _lib.SIGNATURES[n]
        cargs = _c_args(header, n)
        assert len(cargs) == len(args), (n, cargs)
        for c, a in zip(cargs, args):
            if c.endswith("*"):
                base = c.replace("const", "").replace("*", "").strip()
                want = ctypes.POINTER(structs[base]) if base in structs else ctypes.c_void_p
                assert a is want or a == want, (n, c, a)
            else:
                assert a is kinds[c], (n, c, a)
        assert res is (ctypes.c_int64 if n == "nic_hash_packed_bytes_levels" else ctypes.c_int)
    assert "nicv2-hashgrid-bits/2" in header and hashgrid.MIXED_FORMAT == "nicv2-hashgrid-bits/2"
    for n in ("hash_pack_bits_levels", "hash_clamp_levels", "hash_encode_levels", "hash_fused_forward_levels", "hash_fused_forward_backward_levels"):
        assert callable(getattr(hashgrid, n)), n


def _formula(dim, resolutions, features, log2_table, bits):
    """the header's size, restated: 4 sum_l ceil(E_l F b_l / 32) + 8, E_l = (R_l + 1)^dim if that fits the table, else T"""
    total = 0
    for r, b in zip(resolutions, bits):
        e = (r + 1) ** dim
        e = e if e <= (1 << log2_table) else 1 << log2_table
        total += -(-(e * features * b) // 32)
    return 4 * total + 8


@pytest.mark.parametrize("dim,resolutions,features,log2_table,bits", [
    (2, (4, 9, 20, 45, 100), 2, 10, (8, 7, 5, 3, 4)),
    (2, (16, 33, 70, 150), 1, 12, (3, 5, 7, 1)),
    (2, (5, 11, 300), 4, 12, (7, 2, 5)),
    (3, (3, 7, 15, 40), 2, 11, (8, 5, 3, 6)),
    (3, (2, 9, 30), 8, 10, (5, 7, 3)),
])
def test_packed_bytes_levels_is_the_formula(lib, dim, resolutions, features, log2_table, bits):
    ext = (64, 64, 64 if dim == 3 else 1)
    d = _desc(dim, resolutions, features, log2_table, 512, 1, ext)
    dense = [(r + 1) ** dim <= (1 << log2_table) for r in resolutions]
    assert any(dense) and not all(dense)                          # the geometry mixes dense and hashed levels
    assert lib.nic_hash_packed_bytes_levels(ctypes.byref(d), ctypes.byref(_lb(bits))) == _formula(dim, resolutions, features, log2_table, bits)
    for b in range(1, 9):                                         # equal depths: format /1's size
        got = lib.nic_hash_packed_bytes_levels(ctypes.byref(d), ctypes.byref(_lb([b] * len(resolutions))))
        assert got == lib.nic_hash_packed_bytes(ctypes.byref(d), b) == _formula(dim, resolutions, features, log2_table, [b] * len(resolutions))
    # entries past desc->levels are ignored
    assert lib.nic_hash_packed_bytes_levels(ctypes.byref(d), ctypes.byref(_lb(list(bits) + [0, 99]))) == _formula(dim, resolutions, features, log2_table, bits)


def test_packed_bytes_levels_refuses_bad_input(lib):
    d = _desc()
    pb = lib.nic_hash_packed_bytes_levels
    assert pb(ctypes.byref(d), ctypes.byref(_lb([0, 4]))) == ARG
    assert pb(ctypes.byref(d), ctypes.byref(_lb([4, 9]))) == ARG
    assert pb(ctypes.byref(d), None) == NULL
    assert pb(None, ctypes.byref(_lb([4, 4]))) == NULL
    assert pb(ctypes.byref(_desc(features=3)), ctypes.byref(_lb([4, 4]))) == UNSUP
    assert pb(ctypes.byref(_desc(log2_table=9)), ctypes.byref(_lb([4, 4]))) == ARG
    assert pb(ctypes.byref(_desc(extent=(257, 8, 1))), ctypes.byref(_lb([4, 4]))) == SHAPE
    from neural_image_compression_v2_amd import hashgrid
    geo = hashgrid.HashGeometry((256, 256), (16, 64), 2, 12)
    assert hashgrid.hash_packed_bytes(geo, [8, 3]) == _formula(2, (16, 64), 2, 12, (8, 3))
    assert hashgrid.hash_packed_bytes(geo, 4) == hashgrid.hash_packed_bytes(geo, (4, 4))
    for bad in ([8], [8, 3, 3], [0, 4], [4, 9], [4.0, 4]):
        with pytest.raises(ValueError):
            hashgrid.hash_packed_bytes(geo, bad)


def test_descriptor_errors_come_first(lib):
    lb = _lb([8, 3])
    good = _desc()
    assert (_enc(lib, good, lb), _fwd(lib, good, lb), _fb(lib, good, lb)) == (OK, OK, OK)          # n_points == 0: no launch
    bad = _desc()
    bad.flags = 1
    for desc, want in [(None, NULL), (bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG),
                       (_desc(extent=(257, 8, 1)), SHAPE), (_desc(num_crops=0), SHAPE)]:
        assert (_pack(lib, desc, lb), _clamp(lib, desc, lb), _enc(lib, desc, lb), _fwd(lib, desc, lb), _fb(lib, desc, lb)) == (want,) * 5
    # the point route wants one field, both routes 256 S_max < 2^30 (the lattice goes through the fixed-point cell too)
    two = _desc(num_crops=2)
    assert (_enc(lib, two, lb), _fwd(lib, two, lb), _fb(lib, two, lb)) == (SHAPE, SHAPE, SHAPE)
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for kw in (dict(origins=0, points=16), dict(origins=16, points=0)):
        assert (_enc(lib, big, lb, **kw), _fwd(lib, big, lb, **kw), _fb(lib, big, lb, **kw)) == (ARG, ARG, ARG)
    # the fused entries answer nic_hash_fused_supported first: L F > 64, 5 layers
    wide = _desc(resolutions=(16,) * 9, features=8)
    lb9 = _lb([4] * 9)
    assert _enc(lib, wide, lb9) == OK and _fwd(lib, wide, lb9) == UNSUP and _fb(lib, wide, lb9) == UNSUP
    assert _fwd(lib, good, lb, m=_mlp(5, 5)) == UNSUP and _fb(lib, good, lb, m=_mlp(5, 5)) == UNSUP


def test_position_pair_and_argument_errors_stay_on_the_host(lib):
    d, lb = _desc(), _lb([8, 3])
    # both or neither of origins / points
    for kw in (dict(origins=16, points=16), dict(origins=0, points=0)):
        assert (_enc(lib, d, lb, **kw), _fwd(lib, d, lb, **kw), _fb(lib, d, lb, **kw)) == (ARG, ARG, ARG)
    # an order goes with points only
    assert _fb(lib, d, lb, origins=16, points=0, order=16) == ARG
    assert _fb(lib, d, lb, order=16, n=1 << 31) == ARG and _fb(lib, d, lb, n=-1) == ARG
    assert _enc(lib, d, lb, n=-1) == ARG and _fwd(lib, d, lb, n=-1) == ARG
    # null pointers
    assert _enc(lib, d, None) == NULL and _fwd(lib, d, None) == NULL and _fb(lib, d, None) == NULL
    assert _pack(lib, d, None) == NULL and _clamp(lib, d, None) == NULL
    assert _pack(lib, d, lb, table=0) == NULL and _pack(lib, d, lb, packed=0) == NULL and _clamp(lib, d, lb, table=0) == NULL
    assert _enc(lib, d, lb, src=None) == NULL and _enc(lib, d, lb, src=_src(data=0)) == NULL and _enc(lib, d, lb, out=0) == NULL
    assert _fwd(lib, d, lb, src=None) == NULL and _fwd(lib, d, lb, y=0) == NULL and _fwd(lib, d, lb, m=None) == NULL
    assert _fwd(lib, d, lb, m=_mlp(3, 2)) == NULL
    for kw in (dict(table=0), dict(target=0), dict(gs=None), dict(loss=0), dict(ws=0), dict(m=None), dict(m=_mlp(3, 2))):
        assert _fb(lib, d, lb, **kw) == NULL, kw
    assert _fb(lib, d, lb, tg=0, y=0) == OK                                  # a frozen table, no y
    # depths outside 1 .. 8
    for bits in ([0, 4], [4, 9], [-1, 4]):
        b = _lb(bits)
        assert (_pack(lib, d, b), _clamp(lib, d, b), _enc(lib, d, b), _fwd(lib, d, b), _fb(lib, d, b)) == (ARG,) * 5
    # the source: no uint8 form, num_bits 0, a packed table on a dword boundary; noise only with the fp32 table
    for s in (_src(U8), _src(U8, 4), _src(3), _src(F32, 4), _src(BITS, 4), _src(BITS, 0, 18)):
        assert _enc(lib, d, lb, src=s) == ARG and _fwd(lib, d, lb, src=s) == ARG
    assert _enc(lib, d, lb, src=_src(BITS)) == OK and _fwd(lib, d, lb, src=_src(BITS)) == OK
    assert _pack(lib, d, lb, packed=18) == ARG
    assert _enc(lib, d, lb, src=_src(BITS), q=_quant()) == ARG
    assert _enc(lib, d, lb, q=_quant()) == OK and _fb(lib, d, lb, q=_quant()) == OK
    assert _enc(lib, d, lb, q=_quant(mode=1)) == UNSUP and _fb(lib, d, lb, q=_quant(mode=1)) == UNSUP
    assert _enc(lib, d, lb, q=_quant(mode=7)) == ARG and _enc(lib, d, lb, q=_quant(base=-1)) == ARG and _fb(lib, d, lb, q=_quant(base=-1)) == ARG
    # flags, workspace
    assert _fb(lib, d, lb, flags=4) == ARG
    need = lib.nic_hash_fused_points_workspace_bytes(ctypes.byref(d), ctypes.byref(_mlp()))
    assert need > 0 and _fb(lib, d, lb, ws_bytes=need) == OK and _fb(lib, d, lb, ws_bytes=need - 1) == WORKSPACE
    # all of the above with the lattice as the position source, where an accepted call would launch: only refusals are tried
    lat = dict(origins=16, points=0)
    assert _enc(lib, d, _lb([0, 4]), **lat) == ARG and _enc(lib, d, lb, src=_src(U8, 4), **lat) == ARG
    assert _enc(lib, d, lb, src=_src(BITS), q=_quant(), **lat) == ARG and _fwd(lib, d, lb, src=_src(BITS, 0, 18), **lat) == ARG
    assert _fb(lib, d, lb, ws_bytes=need - 1, **lat) == WORKSPACE and _fb(lib, d, lb, flags=4, **lat) == ARG


def _mixed_file(tmp_path, name, **over):
    from neural_image_compression_v2_amd import hashgrid
    from neural_image_compression_v2_amd.image_compression import ColorDecoder
    res, feats, log2 = (4, 9, 20, 45), 2, 10
    bits = [8, 5, 3, 4]
    geo = hashgrid.HashGeometry((64, 48), res, feats, log2)
    d = {"format": hashgrid.MIXED_FORMAT, "field_size": [64, 48], "resolutions": list(res), "features": feats, "log2_table": log2, "num_bits": None,
         "level_bits": bits, "hidden": 64, "n_linear": 3, "table": torch.zeros(hashgrid.hash_packed_bytes(geo, bits), dtype=torch.uint8),
         "decoder": {k: v.detach() for k, v in ColorDecoder(geo.width, 64, 3).state_dict().items()}}
    d.update(over)
    path = os.path.join(tmp_path, name)
    torch.save(d, path)
    return path


def test_load_compressed_refuses_a_bad_mixed_file_without_a_device(tmp_path):
    from neural_image_compression_v2_amd import hashgrid
    need = _formula(2, (4, 9, 20, 45), 2, 10, (8, 5, 3, 4))
    cases = {"short.pt": dict(table=torch.zeros(need - 4, dtype=torch.uint8)), "long.pt": dict(table=torch.zeros(need + 4, dtype=torch.uint8)),
             "uniform_size.pt": dict(table=torch.zeros(_formula(2, (4, 9, 20, 45), 2, 10, (4,) * 4), dtype=torch.uint8)),
             "dtype.pt": dict(table=torch.zeros(need, dtype=torch.int8)), "few.pt": dict(level_bits=[8, 5, 3]),
             "many.pt": dict(level_bits=[8, 5, 3, 4, 4]), "zero.pt": dict(level_bits=[8, 5, 0, 4]), "nine.pt": dict(level_bits=[9, 5, 3, 4]),
             "none.pt": dict(level_bits=None), "float.pt": dict(level_bits=[8.0, 5.0, 3.0, 4.0])}
    for name, over in cases.items():
        with pytest.raises(ValueError):
            hashgrid.HashGridField.load_compressed(_mixed_file(str(tmp_path), name, **over), device="cpu")
    # a well-formed file passes every check and only then asks for the device
    with pytest.raises(RuntimeError, match="HIP device"):
        hashgrid.HashGridField.load_compressed(_mixed_file(str(tmp_path), "good.pt"), device="cpu")


def test_constructor_refuses_bad_depth_lists_before_a_device():
    from neural_image_compression_v2_amd import hashgrid
    for bad in ([8, 4], [8] * 5, [8, 4, 0, 4], [8, 4, 9, 4], [8, 4, 4.5, 4], [8, 4, "4", 4], []):
        with pytest.raises(ValueError):
            hashgrid.HashGridField((64, 48), levels=4, num_bits=bad, device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):                     # a good list gets as far as the device check
        hashgrid.HashGridField((64, 48), levels=4, num_bits=[8, 4, 3, 4], device="cpu")
