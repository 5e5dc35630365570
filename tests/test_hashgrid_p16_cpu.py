"""CPU-only tests of the hash-grid decode on the 16-bit matrix pipe (run with -m "not gpu"): nic_hash_fused_forward_p16 is
exported, declared and mirrored with the same argument list, the ABI version stays 9, its translation unit is in the build and restates none
of the shared helpers, every argument error is decided on the host in the order of nic_hash_fused_forward_levels (fake pointers, nothing
launches), and ``HashGridField`` refuses a bad ``precision=`` before it touches a device."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
SYMBOL = "nic_hash_fused_forward_p16"
UNIT = "hashgrid_fused16.hip"
OK, NULL, UNSUP, SHAPE, ARG = 0, -1, -2, -3, -5
P = ctypes.c_void_p
F32, U8, BITS = 0, 1, 2
SPLIT, BF16 = 1, 2


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


def _src(kind=F32, num_bits=0, data=16):
    from neural_image_compression_v2_amd._lib import NicHashSource
    return NicHashSource(kind, num_bits, data)


def _mlp(n_linear=3, layers=3):
    from neural_image_compression_v2_amd._lib import NicMlp
    m = NicMlp()
    m.n_linear = n_linear
    for i in range(layers):
        m.w[i] = m.b[i] = 16
    return m


def _ref(x):
    return None if x is None else ctypes.byref(x)


def _p16(lib, d, src="default", origins=0, points=16, n=0, m="default", precision=SPLIT, y=16):
    """the return code.  Every pointer is a dummy that is never dereferenced; the default call is at points with n_points = 0, which returns
    NIC_OK without a launch after every check has passed"""
    src = _src() if src == "default" else src
    m = _mlp() if m == "default" else m
    return lib.nic_hash_fused_forward_p16(_ref(d), _ref(src), P(origins), P(points), n, _ref(m), precision, P(y), None)


def _c_args(header, name):
    m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        out.append(re.sub(r"\s*\w+$", "", a) if not a.endswith("*") else a)
    return out


def test_the_symbol_is_exported_declared_and_mirrored(lib):
    from neural_image_compression_v2_amd import _build, _lib, hashgrid
    header = open(HEADER).read()
    assert hasattr(lib, SYMBOL) and SYMBOL in _lib.SIGNATURES and re.search(rf"\b{SYMBOL}\s*\(", header)
    assert _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version()                  # additive: the version stays
    assert re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)
    assert re.search(r"#define\s+NIC_HASH_PREC_SPLIT\s+1\b", header) and re.search(r"#define\s+NIC_HASH_PREC_BF16\s+2\b", header)
    assert (_lib.NIC_HASH_PREC_SPLIT, _lib.NIC_HASH_PREC_BF16) == (1, 2) and hashgrid.PRECISIONS == {"split": 1, "bf16": 2}
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int}
    structs = {"nic_hash_desc": _lib.NicHashDesc, "nic_mlp": _lib.NicMlp, "nic_hash_source": _lib.NicHashSource}
    res, args = _lib.SIGNATURES[SYMBOL]
    cargs = _c_args(header, SYMBOL)
    assert res is ctypes.c_int and len(cargs) == len(args) == 9, cargs
    for c, a in zip(cargs, args):
        if c.endswith("*"):
            base = c.replace("const", "").replace("*", "").strip()
            want = ctypes.POINTER(structs[base]) if base in structs else ctypes.c_void_p
            assert a is want or a == want, (c, a)
        else:
            assert a is kinds[c], (c, a)
    assert args[4] is ctypes.c_int64 and args[6] is ctypes.c_int              # n_points, precision
    assert callable(hashgrid.hash_fused_forward_p16)
    import inspect
    assert list(inspect.signature(hashgrid.hash_fused_forward_p16).parameters) == ["geo", "data", "params", "precision", "coord", "extent", "points",
                                                                                   "kind", "num_bits"]
    for name in ("decode", "query", "resample"):
        assert inspect.signature(getattr(hashgrid.HashGridField, name)).parameters["precision"].default is None, name


def test_the_unit_is_in_the_build_and_restates_no_shared_helper():
    """the kernel's translation unit is compiled, includes the two headers it builds on, and defines none of the helpers
    tests/test_hashgrid_common_cpu.py holds to one definition, nor the split / fragment helpers of fused_kernel.hpp"""
    from neural_image_compression_v2_amd import _build
    import test_hashgrid_common_cpu as common
    assert UNIT in _build.SOURCES and len(set(_build.SOURCES)) == len(_build.SOURCES)
    lines = open(os.path.join(_build.CSRC, UNIT)).read().splitlines()
    for h in ("hash_common.hpp", "fused_kernel.hpp"):
        assert any(re.match(rf'\s*#include\s+"{re.escape(h)}"', ln) for ln in lines), h
    for name in common.FUNCTIONS + list(common.OVERLOADS) + ["split8", "split_acc", "mfma_bf", "mfma_split", "frag_row", "sample_position"]:
        assert not any(common._function_re(name).match(ln) for ln in lines), name
    for name in common.STRUCTS + ["Frag2", "DecoderSmem"]:
        assert not any(common._struct_re(name).match(ln) for ln in lines), name
    text = "\n".join(lines)
    assert "encode_point<D, F, SRC, false, false, false>" in text and "__builtin_amdgcn_mfma_f32_32x32x16_bf16" in open(
        os.path.join(_build.CSRC, "fused_kernel.hpp")).read()
    assert "mfma_split(" in text and "mfma_bf(" in text and "split_acc(" in text and "split8(" in text


def test_argument_errors_in_the_order_of_the_levels_entry(lib):
    d = _desc()
    lat = dict(origins=16, points=0)
    for prec in (SPLIT, BF16):
        assert _p16(lib, d, precision=prec) == OK                                # n_points == 0: no launch
    # 1. null desc / mlp
    assert _p16(lib, None) == NULL and _p16(lib, d, m=None) == NULL
    assert _p16(lib, None, src=None, origins=0, points=0, precision=7, y=0) == NULL
    # 2. nic_hash_fused_supported: before the position pair and every pointer
    bad = _desc()
    bad.flags = 1
    wide = _desc(resolutions=(16,) * 9, features=8)                               # L F = 72
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (_desc(extent=(257, 8, 1)), SHAPE),
                       (_desc(num_crops=0), SHAPE), (wide, UNSUP)]:
        assert _p16(lib, desc) == want
        assert _p16(lib, desc, src=None, origins=0, points=0, precision=7, y=0, n=-1) == want
    assert _p16(lib, d, m=_mlp(5, 5)) == UNSUP and _p16(lib, d, m=_mlp(5, 5), origins=16) == UNSUP
    # 3. the position pair: both or neither
    for kw in (dict(origins=16, points=16), dict(origins=0, points=0)):
        assert _p16(lib, d, **kw) == ARG
        assert _p16(lib, d, src=None, y=0, precision=7, **kw) == ARG
    # 4. the descriptor of the position source: one field at points, 256 S_max < 2^30 on both routes
    two = _desc(num_crops=2)
    assert _p16(lib, two) == SHAPE and _p16(lib, two, src=None, y=0) == SHAPE
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    assert _p16(lib, big) == ARG and _p16(lib, big, **lat) == ARG and _p16(lib, big, src=None, **lat) == ARG
    # 5. null pointers: before the source, the precision and n_points
    assert _p16(lib, d, src=None) == NULL and _p16(lib, d, src=_src(data=0)) == NULL and _p16(lib, d, y=0) == NULL
    assert _p16(lib, d, m=_mlp(3, 2)) == NULL
    assert _p16(lib, d, src=_src(U8, 0, 0), precision=7, n=-1) == NULL and _p16(lib, d, y=0, src=_src(3, 8), precision=0, **lat) == NULL
    # 6. the source: the rules of the point entries, before the precision
    for s in (_src(F32, 8), _src(U8, 0), _src(U8, 9), _src(BITS, 0), _src(3, 8), _src(-1, 0), _src(BITS, 4, 18)):
        assert _p16(lib, d, src=s) == ARG and _p16(lib, d, src=s, **lat) == ARG, (s.kind, s.num_bits)
    for s in (_src(U8, 1), _src(U8, 8, 18), _src(BITS, 1), _src(BITS, 8), _src(BITS, 5)):
        assert _p16(lib, d, src=s) == OK, (s.kind, s.num_bits)
    # 7. the precision: 1 or 2, before n_points
    for prec in (0, 3, -1, 1 << 16):
        assert _p16(lib, d, precision=prec) == ARG and _p16(lib, d, precision=prec, **lat) == ARG
        assert _p16(lib, d, precision=prec, n=-1) == ARG
    # 8. n_points
    assert _p16(lib, d, n=-1) == ARG and _p16(lib, d, n=-(1 << 40)) == ARG
    # with the lattice as the position source an accepted call would launch: only refusals are tried
    assert _p16(lib, d, src=_src(U8, 0), **lat) == ARG and _p16(lib, d, y=0, **lat) == NULL and _p16(lib, two, precision=7, **lat) == ARG


def test_the_field_refuses_a_bad_precision_on_the_host():
    from neural_image_compression_v2_amd import hashgrid
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, HashGridField, level_resolutions

    def bare(size=(96, 80), level_bits=None, levels=8, features=2, hidden=64, n_linear=3):
        f = HashGridField.__new__(HashGridField)
        f.field_size, f.device, f.level_bits, f.table = size, torch.device("cpu"), level_bits, None
        f.geo = HashGeometry(size, tuple(level_resolutions(levels, 16, max(size))), features, 12)
        f.hidden, f.n_linear = hidden, n_linear
        return f
    pts = torch.zeros(5, 2)
    f = bare()
    before = dict(f.__dict__)
    calls = (lambda **kw: f.decode(**kw), lambda **kw: f.query(pts, **kw), lambda **kw: f.resample((48, 40), **kw))
    # an unknown string (or anything that is not one of the two)
    for bad in ("fp16", "f32", "SPLIT", "", 1, True, ("split",)):
        for call in calls:
            with pytest.raises(ValueError, match="precision"):
                call(precision=bad)
        with pytest.raises(ValueError, match="precision"):
            hashgrid.hash_fused_forward_p16(f.geo, torch.zeros(1), [], bad, points=pts)
    # with a level of detail
    for p in ("split", "bf16"):
        with pytest.raises(NotImplementedError):
            f.query(pts, lod=1.0, precision=p)
        with pytest.raises(NotImplementedError):
            f.query(pts, lod=torch.zeros(5), precision=p)
        with pytest.raises(NotImplementedError):
            f.resample((48, 40), lod="auto", precision=p)
        with pytest.raises(NotImplementedError):
            f.resample((48, 40), lod=0.0, precision=p)
        with pytest.raises(NotImplementedError):
            f.decode_mip(1, precision=p)
    # on a field with a bit depth per level
    g = bare(level_bits=(8,) * 8)
    for p in ("split", "bf16"):
        for call in (lambda **kw: g.decode(**kw), lambda **kw: g.query(pts, **kw), lambda **kw: g.resample((48, 40), **kw)):
            with pytest.raises(NotImplementedError):
                call(precision=p)
    # a geometry or decoder outside the fused set
    for h in (bare(levels=9, features=8), bare(hidden=32), bare(n_linear=5)):
        for p in ("split", "bf16"):
            for call in (lambda **kw: h.decode(**kw), lambda **kw: h.query(pts, **kw), lambda **kw: h.resample((48, 40), **kw)):
                with pytest.raises(ValueError, match="fused set"):
                    call(precision=p)
    with pytest.raises(ValueError, match="fused set"):
        hashgrid.hash_fused_forward_p16(bare(levels=9, features=8).geo, torch.zeros(1), [torch.zeros(64, 72)] + [torch.zeros(1)] * 5, "split", points=pts)
    assert f.__dict__ == before                                   # nothing was set on the way to a refusal
