"""CPU-only tests of the hash-grid field's per-point level of detail (run with -m "not gpu"): the four _lod entry points and nic_hash_lod are
exported, declared and mirrored, the struct layout matches gcc's, the ABI version stays 9, every argument error is decided on the host (no
device touched, in the order of the siblings), hash_lod_fade is its float64 definition, and the Python side refuses bad input before the library."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
NEW_SYMBOLS = ("nic_hash_encode_points_lod", "nic_hash_encode_points_backward_lod", "nic_hash_fused_forward_points_lod",
               "nic_hash_fused_forward_backward_points_lod")
OK, NULL, UNSUP, SHAPE, ARG = 0, -1, -2, -3, -5
F32, U8, BITS = 0, 1, 2
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_v2_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.load()


def _desc(dim=2, resolutions=(16, 64), features=2, log2_table=19, s_max=3840, num_crops=1, extent=(3840, 2160, 1)):
    from neural_image_compression_v2_amd._lib import NicHashDesc
    d = NicHashDesc()
    d.dim, d.levels, d.features, d.log2_table, d.S_max, d.num_crops = dim, len(resolutions), features, log2_table, s_max, num_crops
    for a in range(3):
        d.extent[a] = extent[a]
    for l, r in enumerate(resolutions):
        d.resolution[l] = r
    return d


def _lod(fade=(), uniform=0.0, reserved=0):
    from neural_image_compression_v2_amd._lib import NicHashLod
    lp = NicHashLod()
    for l, v in enumerate(fade):
        lp.fade[l] = v
    lp.lod_uniform, lp.reserved = uniform, reserved
    return lp


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
    assert re.search(r"\}\s*nic_hash_lod\s*;", header)
    assert _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version()                  # additive: the version stays
    assert re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)
    assert all(os.path.isfile(os.path.join(_build.CSRC, src)) for src in _build.SOURCES)
    for n in ("hash_lod_fade", "hash_encode_points_lod", "hash_encode_points_backward_lod", "hash_fused_forward_points_lod",
              "hash_fused_forward_backward_points_lod"):
        assert callable(getattr(hashgrid, n)), n
    for n in ("decode_mip", "fit_mips"):
        assert callable(getattr(hashgrid.HashGridField, n)), n
    # n_points travels as int64, right after the lod pointer
    for n, at in (("nic_hash_encode_points_lod", 6), ("nic_hash_encode_points_backward_lod", 4), ("nic_hash_fused_forward_points_lod", 5),
                  ("nic_hash_fused_forward_backward_points_lod", 6)):
        assert _lib.SIGNATURES[n][1][at] is ctypes.c_int64, n
        assert _lib.SIGNATURES[n][1][1] == ctypes.POINTER(_lib.NicHashLod), n


def test_the_lod_kernels_live_in_the_point_units():
    """there is no translation unit of their own any more: no csrc/lod_* file, and the build names only files that exist (the point units, with
    every other csrc/hash_* file, are held to one copy of the shared helpers by tests/test_hashgrid_common_cpu.py)"""
    import glob
    from neural_image_compression_v2_amd import _build
    assert glob.glob(os.path.join(_build.CSRC, "lod_*")) == []
    missing = [src for src in _build.SOURCES if not os.path.isfile(os.path.join(_build.CSRC, src))]
    assert missing == [] and len(set(_build.SOURCES)) == len(_build.SOURCES)


def test_hash_lod_layout_matches_the_c_header():
    from neural_image_compression_v2_amd._lib import NIC_HASH_MAX_LEVELS, NicHashLod
    fields = [f[0] for f in NicHashLod._fields_]
    assert fields == ["fade", "lod_uniform", "reserved"]
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){", 'printf("%zu\\n", sizeof(nic_hash_lod));']
    prog += [f'printf("%zu %zu\\n", offsetof(nic_hash_lod, {f}), sizeof(((nic_hash_lod*)0)->{f}));' for f in fields]
    prog += ["return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-std=c11", src, "-o", exe], check=True)
        vals = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(NicHashLod) == 4 * NIC_HASH_MAX_LEVELS + 8
    assert len(vals) == 1 + 2 * len(fields)
    for k, f in enumerate(fields):
        assert getattr(NicHashLod, f).offset == vals[1 + 2 * k], f
        assert getattr(NicHashLod, f).size == vals[2 + 2 * k], f


def _calls(lib, d, lp, s, q=None, m=None, pts=16, lod=0, n=0, out=16, dx=16, grad=16, order=0, table=16, target=16, gm=True, loss=16, ws=16,
           ws_bytes=1 << 30, flags=0):
    """(encode, backward, fused query, fused step) return codes.  Every pointer is a dummy that is never dereferenced: n_points = 0 unless the
    case is about it, so that a call with nothing wrong returns NIC_OK without a launch - every error is still decided before that"""
    from neural_image_compression_v2_amd._lib import NicMlpGrads
    db = None if d is None else ctypes.byref(d)
    lb = None if lp is None else ctypes.byref(lp)
    sb = None if s is None else ctypes.byref(s)
    qb = None if q is None else ctypes.byref(q)
    mb = ctypes.byref(_mlp() if m is None else m)
    g = NicMlpGrads()
    table = None if s is None else (table if s.kind == F32 else 16)
    return (lib.nic_hash_encode_points_lod(db, lb, sb, qb, P(pts), P(lod), n, P(out), None),
            lib.nic_hash_encode_points_backward_lod(db, lb, P(pts), P(lod), n, P(dx), P(order), P(grad), None),
            lib.nic_hash_fused_forward_points_lod(db, lb, sb, P(pts), P(lod), n, mb, P(out), None),
            lib.nic_hash_fused_forward_backward_points_lod(db, lb, qb, P(table), P(pts), P(lod), n, P(order), mb, P(target), 1.0, P(grad),
                                                           ctypes.byref(g) if gm else None, P(loss), None, flags, P(ws), ws_bytes, None, None))


def test_lod_argument_errors_are_reported_before_any_gpu_work(lib):
    from neural_image_compression_v2_amd._lib import NicHashQuant
    d, lp, s = _desc(), _lod((7.9, 5.9)), _src()
    inf, nan = float("inf"), float("nan")
    assert _calls(lib, d, lp, s) == (OK, OK, OK, OK)
    assert _calls(lib, d, lp, s, lod=16) == (OK, OK, OK, OK)                     # lod is nullable, and never read on the host
    assert _calls(lib, d, lp, s, order=16) == (OK, OK, OK, OK)
    # the descriptor of the level of detail
    assert _calls(lib, d, None, s) == (NULL,) * 4
    for bad in (_lod((-1.0, 0.0)), _lod((0.0, -1e-30)), _lod((nan, 0.0)), _lod((0.0, inf)), _lod((0.0, -inf)), _lod((1.0, 1.0), uniform=nan),
                _lod((1.0, 1.0), uniform=inf), _lod((1.0, 1.0), uniform=-inf), _lod((1.0, 1.0), reserved=1), _lod((1.0, 1.0), reserved=-7)):
        assert _calls(lib, d, bad, s) == (ARG,) * 4, (list(bad.fade)[:2], bad.lod_uniform, bad.reserved)
    for ok in (_lod((0.0, 0.0)), _lod((-0.0, 31.5)), _lod((1e30, 0.0)), _lod((1.0, 1.0), uniform=-5.0), _lod((1.0, 1.0), uniform=1e30),
               _lod((1.0, 1.0, -1.0, nan))):                                     # entries past desc->levels are ignored
        assert _calls(lib, d, ok, s) == (OK,) * 4
    # the siblings' null pointers (the backward takes no source, the fused step takes the fp32 table itself)
    assert _calls(lib, None, lp, s) == (NULL,) * 4
    assert _calls(lib, d, lp, None) == (NULL, OK, NULL, NULL)
    assert _calls(lib, d, lp, _src(data=0))[::2] == (NULL, NULL)
    assert _calls(lib, d, lp, s, pts=0) == (NULL,) * 4
    assert _calls(lib, d, lp, s, out=0) == (NULL, OK, NULL, OK)
    assert _calls(lib, d, lp, s, dx=0) == (OK, NULL, OK, OK)
    assert _calls(lib, d, lp, s, grad=0) == (OK, NULL, OK, OK)                   # a null table_grad is the fused step's frozen table
    assert _calls(lib, d, lp, s, table=0)[3] == NULL
    assert _calls(lib, d, lp, s, target=0)[3] == NULL
    assert _calls(lib, d, lp, s, gm=False)[3] == NULL
    assert _calls(lib, d, lp, s, loss=0)[3] == NULL
    assert _calls(lib, d, lp, s, ws=0)[3] == NULL
    assert _calls(lib, d, lp, s, m=_mlp(layers=1)) == (OK, OK, NULL, NULL)
    # a null pointer comes before a bad lod descriptor, the lod descriptor before the siblings' arguments
    assert _calls(lib, d, _lod((-1.0, 0.0)), s, pts=0) == (NULL,) * 4
    assert _calls(lib, d, _lod((-1.0, 0.0)), _src(U8, 0), n=-1, flags=4) == (ARG,) * 4
    # the descriptor comes before everything
    bad = _desc()
    bad.flags = 1
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (_desc(resolutions=()), ARG),
                       (_desc(extent=(3841, 8, 1)), SHAPE), (_desc(num_crops=2), SHAPE)]:
        assert _calls(lib, desc, None, None, pts=0) == (want,) * 4
    big = 1 << 22
    assert _calls(lib, _desc(s_max=big, extent=(big, 8, 1)), lp, s) == (ARG,) * 4
    # the source, quant, n_points, flags, workspace: the siblings' checks with their codes
    for bs in (_src(F32, 8), _src(U8, 0), _src(U8, 9), _src(BITS, 0), _src(3, 8), _src(BITS, 4, 18)):
        assert _calls(lib, d, lp, bs)[:3] == (ARG, OK, ARG), (bs.kind, bs.num_bits)
    for gs in (_src(U8, 1), _src(U8, 8, 18), _src(BITS, 1), _src(BITS, 8)):
        assert _calls(lib, d, lp, gs)[:3] == (OK, OK, OK)
    q = NicHashQuant(8, 2, 1, 2, 0)
    assert _calls(lib, d, lp, s, q=q) == (OK, OK, OK, OK)
    assert _calls(lib, d, lp, _src(U8, 8), q=q)[0] == ARG
    assert _calls(lib, d, lp, _src(BITS, 8), q=q)[0] == ARG
    assert _calls(lib, d, lp, s, q=NicHashQuant(0, 2, 1, 2, 0))[::3] == (ARG, ARG)
    assert _calls(lib, d, lp, s, q=NicHashQuant(8, 2, 1, 2, -1))[::3] == (ARG, ARG)
    assert _calls(lib, d, lp, s, q=NicHashQuant(8, 1, 1, 2, 0))[::3] == (UNSUP, UNSUP)      # NIC_NOISE_TENSOR
    assert _calls(lib, d, lp, s, n=-1) == (ARG,) * 4
    assert _calls(lib, d, lp, s, n=1 << 31, order=16, dx=0, table=0)[1::2] == (NULL, NULL)  # pointers first
    assert _calls(lib, d, lp, s, flags=4)[3] == ARG
    assert _calls(lib, d, lp, s, ws_bytes=16)[3] == -4                           # NIC_E_WORKSPACE
    need = lib.nic_hash_fused_points_workspace_bytes(ctypes.byref(d), ctypes.byref(_mlp()))
    assert need > 0
    assert _calls(lib, d, lp, s, ws_bytes=need)[3] == OK and _calls(lib, d, lp, s, ws_bytes=need - 1)[3] == -4
    # the fused kernels' own set
    wide = _desc(resolutions=tuple(range(16, 33)), features=4)                   # 17 x 4 = 68 columns
    assert _calls(lib, wide, _lod((0.0,) * 17), s) == (OK, OK, UNSUP, UNSUP)
    assert _calls(lib, d, lp, s, m=_mlp(n_linear=5, layers=5)) == (OK, OK, UNSUP, UNSUP)


def test_an_order_indexes_fewer_than_2_31_points(lib):
    """with an order n_points >= 2^31 is NIC_E_ARG, decided on the host"""
    d, lp = _desc(), _lod((7.9, 5.9))
    from neural_image_compression_v2_amd._lib import NicMlpGrads
    g = NicMlpGrads()
    assert lib.nic_hash_encode_points_backward_lod(ctypes.byref(d), ctypes.byref(lp), P(16), None, 1 << 31, P(16), P(16), P(16), None) == ARG
    assert lib.nic_hash_fused_forward_backward_points_lod(ctypes.byref(d), ctypes.byref(lp), None, P(16), P(16), None, 1 << 31, P(16),
                                                          ctypes.byref(_mlp()), P(16), 1.0, P(16), ctypes.byref(g), P(16), None, 0, P(16), 1 << 30,
                                                          None, None) == ARG


def test_hash_lod_fade_is_its_float64_definition():
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, hash_lod_fade, level_resolutions
    for size, levels, n_min, n_max in (((3840, 2160), 16, 16, 3840), ((96, 80), 8, 16, 96), ((40, 36, 28), 8, 4, 40), ((64, 64), 6, 16, 256)):
        geo = HashGeometry(size, tuple(level_resolutions(levels, n_min, n_max)), 2, 12)
        fade = hash_lod_fade(geo)
        assert isinstance(fade, tuple) and len(fade) == levels
        for r, f in zip(geo.resolutions, fade):
            want = float(torch.tensor(max(0.0, math.log2(max(size) / r)), dtype=torch.float64).to(torch.float32))
            assert f == want and f >= 0 and math.isfinite(f), (r, f, want)
            if r >= max(size):
                assert f == 0.0
        assert list(fade) == sorted(fade, reverse=True)
    geo = HashGeometry((96, 80), (12, 96, 200), 2, 12)
    assert hash_lod_fade(geo) == (3.0, 0.0, 0.0)                                 # R_l = S_max: 0; finer than a sample: still 0


def test_python_side_checks_on_the_host():
    from neural_image_compression_v2_amd import hashgrid
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, HashGridField, level_resolutions
    geo = HashGeometry((96, 80), tuple(level_resolutions(8, 16, 96)), 2, 12)
    pts, table = torch.zeros(5, 2), torch.zeros(geo.table_shape())
    # nothing on the CPU: no fallback
    with pytest.raises(RuntimeError, match="HIP device"):
        hashgrid.hash_encode_points_lod(geo, table, pts)
    with pytest.raises(RuntimeError, match="HIP device"):
        hashgrid.hash_encode_points_backward_lod(geo, pts, torch.zeros(5, geo.width), table)
    # the fade: `levels` finite values >= 0
    for bad in ([0.0] * 7, [0.0] * 9, [0.0] * 7 + [-1.0], [0.0] * 7 + [float("nan")], [0.0] * 7 + [float("inf")], "01234567", 3.0, [None] * 8):
        with pytest.raises(ValueError):
            hashgrid._check_fade(8, bad)
        with pytest.raises(ValueError):
            HashGridField((96, 80), levels=8, log2_table=12, lod_fade=bad)       # before anything is allocated
    assert hashgrid._check_fade(3, [0, 1.5, 2]) == (0.0, 1.5, 2.0)
    assert list(hashgrid._lod_struct(geo, None, 1.25).fade)[:8] == list(hashgrid.hash_lod_fade(geo))
    assert hashgrid._lod_struct(geo, [1.0] * 8, 1.25).lod_uniform == 1.25
    with pytest.raises(ValueError):
        hashgrid._lod_struct(geo, None, float("nan"))

    def bare(size=(96, 80), level_bits=None):
        f = HashGridField.__new__(HashGridField)
        f.field_size, f.device, f.level_bits, f.table = size, torch.device("cpu"), level_bits, None
        f.geo = HashGeometry(size, tuple(level_resolutions(8, 16, max(size))), 2, 12)
        return f
    f = bare()
    assert f.lod_fade == hashgrid.hash_lod_fade(f.geo)
    # mips: every axis divisible by 2^m
    assert f._mip_size(0) == (96, 80) and f._mip_size(4) == (6, 5)
    for m in (5, 6, -1):
        with pytest.raises(ValueError, match="divisible"):
            f.decode_mip(m)
    with pytest.raises(ValueError, match="divisible"):
        f.fit_mips(torch.zeros(96, 80, 3), 1, mips=5)
    with pytest.raises(ValueError):
        f.fit_mips(torch.zeros(96, 81, 3), 1, mips=1)
    with pytest.raises(ValueError):
        bare((40, 36, 28)).decode_mip(3)
    # lod: a finite float or a [N] tensor; resample: None, "auto" or a float
    for bad in (float("nan"), float("inf"), "coarse", [1.0]):
        with pytest.raises(ValueError):
            f.query(pts, lod=bad)
    with pytest.raises(ValueError):
        f.resample((48, 40), lod="best")
    with pytest.raises(ValueError):
        f.resample((48, 40), lod=torch.zeros(3))
    # a bit depth per level has no level of detail
    g = bare(level_bits=(8,) * 8)
    with pytest.raises(NotImplementedError):
        g.query(pts, lod=1.0)
    with pytest.raises(NotImplementedError):
        g.resample((48, 40), lod="auto")
    with pytest.raises(NotImplementedError):
        g.decode_mip(1)
    with pytest.raises(NotImplementedError):
        g.fit_mips(torch.zeros(96, 80, 3), 1, mips=1)
    g.table = torch.zeros(1)
    with pytest.raises(NotImplementedError):
        g.train_points(pts, torch.zeros(5, 3), lod=1.0)
    with pytest.raises(NotImplementedError):
        g.fit_points(pts, torch.zeros(5, 3), 1, lod=torch.zeros(5))
