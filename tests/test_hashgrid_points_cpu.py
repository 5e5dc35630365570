"""CPU-only tests of the hash-grid field at arbitrary points (run with -m "not gpu"): the three new C ABI symbols and nic_hash_source are
exported, declared and mirrored, the struct layout matches gcc's, the ABI version stays 9, every argument error of the new entry points is
decided on the host (no device touched, in the order of the crop siblings), and the Python wrappers refuse bad input before the library."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
NEW_SYMBOLS = ("nic_hash_encode_points", "nic_hash_encode_points_backward", "nic_hash_fused_forward_points")
NULL, UNSUP, SHAPE, ARG = -1, -2, -3, -5
F32, U8, BITS = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_v2_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.load()


def _desc(dim=2, resolutions=(16,), features=2, log2_table=19, s_max=3840, num_crops=1, extent=(3840, 2160, 1)):
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


def test_new_symbols_are_exported_declared_and_mirrored(lib):
    from neural_image_compression_v2_amd import _build, _lib, hashgrid
    header = open(HEADER).read()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
        assert re.search(rf"\b{n}\s*\(", header), n
    assert re.search(r"\}\s*nic_hash_source\s*;", header)
    assert (_lib.NIC_HASH_SRC_F32, _lib.NIC_HASH_SRC_U8, _lib.NIC_HASH_SRC_BITS) == (F32, U8, BITS)
    for name, val in (("NIC_HASH_SRC_F32", 0), ("NIC_HASH_SRC_U8", 1), ("NIC_HASH_SRC_BITS", 2)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", header), name
    assert _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version()                  # additive: the version stays
    assert "hash_points.hip" in _build.SOURCES
    for n in ("hash_encode_points", "hash_encode_points_backward", "hash_fused_forward_points", "HashEncodePointsFunction"):
        assert callable(getattr(hashgrid, n)), n
    for n in ("query", "resample", "train_points"):
        assert callable(getattr(hashgrid.HashGridField, n)), n
    # n_points travels as int64
    assert _lib.SIGNATURES["nic_hash_encode_points"][1][4] is ctypes.c_int64
    assert _lib.SIGNATURES["nic_hash_encode_points_backward"][1][2] is ctypes.c_int64
    assert _lib.SIGNATURES["nic_hash_fused_forward_points"][1][3] is ctypes.c_int64


def test_hash_source_layout_matches_the_c_header():
    from neural_image_compression_v2_amd._lib import NicHashSource
    fields = [f[0] for f in NicHashSource._fields_]
    assert fields == ["kind", "num_bits", "data"]
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){", 'printf("%zu\\n", sizeof(nic_hash_source));']
    prog += [f'printf("%zu %zu\\n", offsetof(nic_hash_source, {f}), sizeof(((nic_hash_source*)0)->{f}));' for f in fields]
    prog += ["return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-std=c11", src, "-o", exe], check=True)
        vals = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(NicHashSource) == 16
    assert len(vals) == 1 + 2 * len(fields)
    for k, f in enumerate(fields):
        assert getattr(NicHashSource, f).offset == vals[1 + 2 * k], f
        assert getattr(NicHashSource, f).size == vals[2 + 2 * k], f


def _calls(lib, d, s, q=None, m=None, pts=16, n=0, out=16, dx=16, grad=16):
    """(encode, backward, fused) return codes on one (desc, source).  Every pointer is a dummy that is never dereferenced: n_points = 0 unless
    the case is about it, so that a call with nothing wrong returns NIC_OK without a launch - every error is still decided before that"""
    P = ctypes.c_void_p
    db = None if d is None else ctypes.byref(d)
    sb = None if s is None else ctypes.byref(s)
    mb = ctypes.byref(_mlp() if m is None else m)
    return (lib.nic_hash_encode_points(db, sb, None if q is None else ctypes.byref(q), P(pts), n, P(out), None),
            lib.nic_hash_encode_points_backward(db, P(pts), n, P(dx), P(grad), None),
            lib.nic_hash_fused_forward_points(db, sb, P(pts), n, mb, P(out), None))


def test_point_argument_errors_are_reported_before_any_gpu_work(lib):
    from neural_image_compression_v2_amd._lib import NicHashQuant
    d, s = _desc(), _src()
    P = ctypes.c_void_p
    OK = 0
    assert _calls(lib, d, s) == (OK, OK, OK)
    # null pointers (the backward takes no source)
    assert _calls(lib, None, s) == (NULL, NULL, NULL)
    assert _calls(lib, d, None) == (NULL, OK, NULL)
    assert _calls(lib, d, _src(data=0)) == (NULL, OK, NULL)
    assert _calls(lib, d, s, pts=0) == (NULL, NULL, NULL)
    assert _calls(lib, d, s, out=0) == (NULL, OK, NULL)
    assert _calls(lib, d, s, dx=0) == (OK, NULL, OK)
    assert _calls(lib, d, s, grad=0) == (OK, NULL, OK)
    assert lib.nic_hash_fused_forward_points(ctypes.byref(d), ctypes.byref(s), P(16), 0, None, P(16), None) == NULL
    assert _calls(lib, d, s, m=_mlp(layers=1)) == (OK, OK, NULL)
    # kind / num_bits mismatches
    for bad in (_src(F32, 8), _src(F32, -1), _src(U8, 0), _src(U8, 9), _src(BITS, 0), _src(BITS, 9), _src(BITS, -3), _src(3, 8), _src(-1, 0)):
        assert _calls(lib, d, bad) == (ARG, OK, ARG), (bad.kind, bad.num_bits)
    for ok in (_src(U8, 1), _src(U8, 8), _src(BITS, 1), _src(BITS, 8)):
        assert _calls(lib, d, ok) == (OK, OK, OK)
    # a null pointer is reported before a bad source, like the _u8 / _bits siblings
    assert _calls(lib, d, _src(U8, 0), pts=0) == (NULL, NULL, NULL)
    assert lib.nic_hash_encode_u8(ctypes.byref(_desc(extent=(8, 8, 1))), 0, None, P(16), P(16), None) == NULL
    # the packed table is read as aligned dwords; the uint8 one is bytes
    assert _calls(lib, d, _src(BITS, 4, 18)) == (ARG, OK, ARG)
    assert _calls(lib, d, _src(U8, 4, 18)) == (OK, OK, OK)
    # quant: only with an fp32 source; its own checks are nic_hash_encode_noisy's
    q = NicHashQuant(8, 2, 1, 2, 0)
    assert _calls(lib, d, _src(U8, 8), q=q)[0] == ARG
    assert _calls(lib, d, _src(BITS, 8), q=q)[0] == ARG
    assert _calls(lib, d, s, q=q)[0] == OK
    assert _calls(lib, d, s, q=NicHashQuant(0, 2, 1, 2, 0))[0] == ARG
    assert _calls(lib, d, s, q=NicHashQuant(8, 2, 1, 2, -1))[0] == ARG
    assert _calls(lib, d, s, q=NicHashQuant(8, 1, 1, 2, 0))[0] == UNSUP          # NIC_NOISE_TENSOR
    assert _calls(lib, d, s, q=NicHashQuant(8, 7, 1, 2, 0))[0] == ARG
    assert _calls(lib, d, s, q=NicHashQuant(8, 0, 1, 2, 0))[0] == OK             # NIC_NOISE_NONE: the plain kernel
    # n_points: negative is an error, zero is NIC_OK with nothing launched (there is no device here, and the pointers are dummies)
    assert _calls(lib, d, s, n=-1) == (ARG, ARG, ARG)
    assert _calls(lib, d, s, n=-(1 << 40)) == (ARG, ARG, ARG)
    # one field per launch
    assert _calls(lib, _desc(num_crops=2), s) == (SHAPE, SHAPE, SHAPE)
    assert _calls(lib, _desc(num_crops=0), s) == (SHAPE, SHAPE, SHAPE)
    # 256 S_max < 2^30
    big = 1 << 22
    assert _calls(lib, _desc(s_max=big, extent=(big, 8, 1)), s) == (ARG, ARG, ARG)
    assert _calls(lib, _desc(s_max=big - 1, extent=(big - 1, 8, 1)), s) == (OK, OK, OK)
    assert lib.nic_hash_stored_bytes(ctypes.byref(_desc(s_max=big, extent=(8, 8, 1)))) > 0      # the crop route takes that field
    # every field the descriptor accepts at 4K or 256^3 passes
    from neural_image_compression_v2_amd.hashgrid import level_resolutions
    assert _calls(lib, _desc(resolutions=tuple(level_resolutions(16, 16, 3840))), s) == (OK, OK, OK)
    assert _calls(lib, _desc(dim=3, resolutions=tuple(level_resolutions(16, 16, 256)), s_max=256, extent=(256, 256, 256)), s) == (OK, OK, OK)
    # the descriptor checks of nic_hash_encode, flags != 0 included, with the siblings' codes
    bad = _desc()
    bad.flags = 1
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (_desc(resolutions=()), ARG),
                       (_desc(resolutions=(1 << 20,), s_max=1 << 11, extent=(8, 8, 1)), ARG), (_desc(extent=(3841, 8, 1)), SHAPE),
                       (_desc(extent=(8, 0, 1)), SHAPE)]:
        assert _calls(lib, desc, s) == (want, want, want)
        assert lib.nic_hash_encode(ctypes.byref(desc), P(16), P(16), P(16), None) == want
    # the descriptor comes before the pointers, the pointers before the arguments
    assert _calls(lib, bad, None, pts=0) == (ARG, ARG, ARG)
    assert _calls(lib, d, _src(U8, 0), pts=0, n=-1) == (NULL, NULL, NULL)
    # the fused kernel's own set: L F <= 64, 3 Linear layers - the answer of nic_hash_fused_supported
    wide = _desc(resolutions=tuple(range(16, 33)), features=4)                   # 17 x 4 = 68 columns
    assert lib.nic_hash_fused_supported(ctypes.byref(wide), 64, 3) == UNSUP
    assert _calls(lib, wide, s) == (OK, OK, UNSUP)
    assert _calls(lib, d, s, m=_mlp(n_linear=5, layers=5)) == (OK, OK, UNSUP)
    assert _calls(lib, d, s, m=_mlp(n_linear=0)) == (OK, OK, OK)


def test_python_side_checks_on_the_host():
    from neural_image_compression_v2_amd import hashgrid
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, HashGridField, level_resolutions
    geo = HashGeometry((256, 256), tuple(level_resolutions(8, 16, 256)), 2, 12)
    pts = torch.zeros(5, 2)
    table = torch.zeros(geo.table_shape())
    # nothing on the CPU: no fallback
    with pytest.raises(RuntimeError, match="HIP device"):
        hashgrid.hash_encode_points(geo, table, pts)
    with pytest.raises(RuntimeError, match="HIP device"):
        hashgrid.hash_encode_points_backward(geo, pts, torch.zeros(5, geo.width), table)
    with pytest.raises(ValueError):
        hashgrid.hash_encode_points(geo, table, pts, kind="f16")
    with pytest.raises(ValueError):
        hashgrid.hash_encode_points(geo, table, pts, kind="f32", num_bits=8)
    for kind in ("u8", "bits"):
        for bits in (None, 0, 9):
            with pytest.raises(ValueError):
                hashgrid.hash_encode_points(geo, torch.zeros(16, dtype=torch.uint8), pts, kind=kind, num_bits=bits)
        with pytest.raises(ValueError):                                          # host tensor, wrong size
            hashgrid.hash_fused_forward_points(geo, torch.zeros(16, dtype=torch.uint8), pts, [], kind=kind, num_bits=4)
    # a field too large for 8 fractional bits is refused by name, before the library
    huge = HashGeometry((1 << 22, 8), (16,), 2, 12)
    with pytest.raises(ValueError, match="2\\^30"):
        hashgrid._point_desc(huge)
    assert hashgrid._point_desc(geo).num_crops == 1 and list(hashgrid._point_desc(geo).extent)[:2] == [256, 256]
    # a decode-only field does not train
    f = HashGridField.__new__(HashGridField)
    f.table = None
    with pytest.raises(RuntimeError, match="decodes only"):
        f.train_points(pts, torch.zeros(5, 3))
