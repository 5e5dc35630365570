"""CPU-only tests of the hash-grid field (run with -m "not gpu"): the level-resolution formula, the dense / hashed split, the entry index the
kernels use (its host build, nic_hash_index_host) against Python-int known answers, the argument errors of the C ABI (decided on the host, no
device touched), the ctypes mirror of nic_hash_desc against the C layout, and that no product path runs without a HIP device."""
import ctypes
import math
import os
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
M32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_v2_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.load()


def _desc(dim=2, resolutions=(16,), features=2, log2_table=19, s_max=3840, num_crops=1, extent=(8, 8, 1)):
    from neural_image_compression_v2_amd._lib import NicHashDesc
    d = NicHashDesc()
    d.dim, d.levels, d.features, d.log2_table, d.S_max, d.num_crops = dim, len(resolutions), features, log2_table, s_max, num_crops
    for a in range(3):
        d.extent[a] = extent[a]
    for l, r in enumerate(resolutions):
        d.resolution[l] = r
    return d


def _index_py(dim, R, log2_table, vx, vy, vz=0):
    """the semantics of include/nicv2_hip.h in Python ints"""
    T = 1 << log2_table
    if (R + 1) ** dim <= T:
        h = vx + (R + 1) * (vy + (R + 1) * vz)
    else:
        h = (vx & M32) ^ ((vy * 2654435761) & M32) ^ ((vz * 805459861) & M32)
    return h & (T - 1)


def test_level_resolutions_formula_and_hand_values():
    from neural_image_compression_v2_amd.hashgrid import level_resolutions
    # L 16, N_min 16, N_max 3840: b = 240^(1/15); the last level rounds down to 3839 (16 b^15 = 3839.999.. in float64)
    assert level_resolutions(16, 16, 3840) == [16, 23, 33, 47, 68, 99, 143, 206, 297, 428, 617, 890, 1283, 1849, 2664, 3839]
    for L, lo, hi in [(5, 16, 256), (16, 2, 512), (8, 16, 2160), (32, 4, 4096), (2, 16, 64)]:
        b = math.exp((math.log(hi) - math.log(lo)) / (L - 1))
        assert level_resolutions(L, lo, hi) == [math.floor(lo * b ** l) for l in range(L)]
    assert level_resolutions(1, 16, 3840) == [16]
    with pytest.raises(ValueError):
        level_resolutions(33, 16, 3840)


def test_dense_and_hashed_levels():
    from neural_image_compression_v2_amd.hashgrid import level_is_dense, level_resolutions
    res = level_resolutions(16, 16, 3840)
    dense = [level_is_dense(r, 2, 19) for r in res]
    assert dense == [True] * 11 + [False] * 5                  # (617 + 1)^2 <= 2^19 < (890 + 1)^2
    assert level_is_dense(723, 2, 19) and not level_is_dense(724, 2, 19)
    assert level_is_dense(63, 3, 18) and not level_is_dense(64, 3, 18)       # 64^3 = 2^18
    assert [level_is_dense(r, 3, 19) for r in level_resolutions(16, 16, 256)] == [(r + 1) ** 3 <= 2 ** 19 for r in level_resolutions(16, 16, 256)]


def test_host_index_matches_python_ints(lib):
    assert lib.nic_hash_index_host(ctypes.byref(_desc(resolutions=(3839,))), 0, 3, 5, 0) == (3 ^ (5 * 2654435761 % 2 ** 32)) & (2 ** 19 - 1)
    cases = [
        (2, (100,), 19, [(0, 0, 0), (3, 5, 0), (100, 100, 0), (57, 99, 0)]),                      # dense 2D
        (2, (3839, 890), 19, [(3, 5, 0), (3839, 3839, 0), (0, 1, 0), (1234, 2345, 0)]),           # hashed 2D
        (2, (40,), 10, [(40, 40, 0), (7, 31, 0)]),                                               # hashed 2D, small table
        (3, (30,), 19, [(0, 0, 0), (30, 30, 30), (1, 2, 3)]),                                    # dense 3D
        (3, (255, 128), 19, [(255, 255, 255), (17, 200, 3), (0, 0, 1)]),                          # hashed 3D
        (3, (9,), 10, [(9, 9, 9), (1, 2, 3)]),                                                   # 10^3 <= 2^10: dense
    ]
    for dim, res, lg, verts in cases:
        d = _desc(dim=dim, resolutions=res, log2_table=lg, s_max=4096)
        for l, R in enumerate(res):
            for vx, vy, vz in verts:
                got = lib.nic_hash_index_host(ctypes.byref(d), l, vx, vy, vz)
                assert got == _index_py(dim, R, lg, vx, vy, vz), (dim, R, lg, vx, vy, vz)
                assert 0 <= got < 1 << lg
    # 2D ignores vz
    d = _desc(resolutions=(3839,))
    assert lib.nic_hash_index_host(ctypes.byref(d), 0, 7, 9, 123) == _index_py(2, 3839, 19, 7, 9)


def test_argument_errors_are_reported_before_any_gpu_work(lib):
    from neural_image_compression_v2_amd import _lib
    NULL, UNSUP, SHAPE, ARG = -1, -2, -3, -5
    dummy = ctypes.c_void_p(16)                       # never dereferenced: every case fails on the host first

    def rc(d):
        e = lib.nic_hash_encode(ctypes.byref(d), dummy, dummy, dummy, None)
        b = lib.nic_hash_encode_backward(ctypes.byref(d), dummy, dummy, dummy, None)
        i = lib.nic_hash_index_host(ctypes.byref(d), 0, 0, 0, 0)
        assert e == b == i, (e, b, i)
        return e

    assert lib.nic_hash_encode(None, dummy, dummy, dummy, None) == NULL
    assert lib.nic_hash_encode_backward(None, dummy, dummy, dummy, None) == NULL
    assert lib.nic_hash_index_host(None, 0, 0, 0, 0) == NULL
    d = _desc()
    assert lib.nic_hash_encode(ctypes.byref(d), None, dummy, dummy, None) == NULL
    assert lib.nic_hash_encode(ctypes.byref(d), dummy, None, dummy, None) == NULL
    assert lib.nic_hash_encode(ctypes.byref(d), dummy, dummy, None, None) == NULL
    assert lib.nic_hash_encode_backward(ctypes.byref(d), None, dummy, dummy, None) == NULL
    assert lib.nic_hash_encode_backward(ctypes.byref(d), dummy, None, dummy, None) == NULL
    assert lib.nic_hash_encode_backward(ctypes.byref(d), dummy, dummy, None, None) == NULL
    for f in (0, 3, 5, 16):
        assert rc(_desc(features=f)) == UNSUP
    for dim in (1, 4):
        assert rc(_desc(dim=dim)) == UNSUP
    assert rc(_desc(resolutions=())) == ARG                                           # levels 0
    too_many = _desc(resolutions=(16,) * 32)
    too_many.levels = 33
    assert rc(too_many) == ARG
    for lg in (9, 25):
        assert rc(_desc(log2_table=lg)) == ARG
    assert rc(_desc(resolutions=(16, 0, 32))) == ARG                                  # R_l < 1
    assert rc(_desc(resolutions=(1 << 20,), s_max=1 << 10)) == ARG                    # 2 S_max R = 2^31
    assert rc(_desc(num_crops=0)) == SHAPE
    assert rc(_desc(extent=(0, 8, 1))) == SHAPE
    assert rc(_desc(extent=(8, 4000, 1))) == SHAPE                                    # wider than the field
    bad = _desc()
    bad.flags = 1
    assert rc(bad) == ARG
    assert lib.nic_hash_index_host(ctypes.byref(_desc(resolutions=(16, 32))), 2, 0, 0, 0) == ARG   # level out of range
    assert lib.nic_hash_index_host(ctypes.byref(_desc(resolutions=(16, 32))), -1, 0, 0, 0) == ARG
    assert _lib.NIC_HASH_MAX_LEVELS == 32


def test_hash_desc_layout_matches_the_c_header():
    from neural_image_compression_v2_amd._lib import NicHashDesc
    fields = [f[0] for f in NicHashDesc._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){",
            'printf("%zu %d\\n", sizeof(nic_hash_desc), NIC_HASH_MAX_LEVELS);']
    prog += [f'printf("%zu\\n", offsetof(nic_hash_desc, {f}));' for f in fields]
    prog += ["return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-std=c11", src, "-o", exe], check=True)
        vals = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(NicHashDesc)
    assert vals[1] == 32
    for f, off in zip(fields, vals[2:]):
        assert getattr(NicHashDesc, f).offset == off, f
    assert len(vals) == 2 + len(fields)


def test_geometry_validation_and_descriptor():
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, level_resolutions
    geo = HashGeometry((3840, 2160), tuple(level_resolutions(16, 16, 3840)), 2, 19)
    assert geo.dim == 2 and geo.levels == 16 and geo.s_max == 3840 and geo.width == 32 and geo.table_shape() == (16, 1 << 19, 2)
    d = geo.to_desc(3, (64, 32))
    assert (d.dim, d.levels, d.features, d.log2_table, d.S_max, d.num_crops) == (2, 16, 2, 19, 3840, 3)
    assert list(d.extent) == [64, 32, 1] and list(d.resolution)[:16] == list(geo.resolutions) and d.flags == 0
    assert geo.check_crops([[0, 0], [3776, 2128]], (64, 32)).tolist() == [[0, 0], [3776, 2128]]
    with pytest.raises(IndexError):
        geo.check_crops([[3777, 0]], (64, 32))                      # one sample past the far edge
    with pytest.raises(IndexError):
        geo.check_crops([[0, -1]], (64, 32))
    with pytest.raises(ValueError):
        geo.check_crops([[0, 0]], (64, 32, 4))
    for bad in [dict(features=3), dict(log2_table=9), dict(log2_table=25)]:
        with pytest.raises(ValueError):
            HashGeometry((64, 64), (16,), **{**dict(features=2, log2_table=19), **bad})
    with pytest.raises(ValueError):
        HashGeometry((64, 64), (0,))
    with pytest.raises(ValueError):
        HashGeometry((64,), (16,))


def test_hash_grid_field_refuses_cpu():
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    with pytest.raises(RuntimeError):
        HashGridField((64, 48), device="cpu")
    with pytest.raises(RuntimeError):
        HashGridField((32, 32, 32), levels=4, device=torch.device("cpu"))
