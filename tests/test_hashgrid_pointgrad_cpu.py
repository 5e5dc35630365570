"""CPU-only tests of the gradients with respect to the point coordinates (run with -m "not gpu"): nic_hash_encode_points_grad and
nic_hash_fused_points_grad are exported, declared and mirrored with the same argument lists, the ABI version stays 9, their translation unit is
in the build and restates none of the shared helpers, every argument error of both entries is decided on the host in the documented order (fake
pointers, nothing launches), and ``HashGridField.point_gradient`` / ``jacobian`` / ``query_differentiable`` refuse before they touch a device."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
ENCODE, FUSED = "nic_hash_encode_points_grad", "nic_hash_fused_points_grad"
UNIT = "hashgrid_pointgrad.hip"
OK, NULL, UNSUP, SHAPE, ARG = 0, -1, -2, -3, -5
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


def _lod(levels=2, fade=None, lod_uniform=0.0, reserved=0):
    from neural_image_compression_v2_amd._lib import NicHashLod
    lp = NicHashLod()
    for l in range(levels):
        lp.fade[l] = 1.0 if fade is None else fade[l]
    lp.lod_uniform, lp.reserved = lod_uniform, reserved
    return lp


def _ref(x):
    return None if x is None else ctypes.byref(x)


def _enc(lib, d, lodp=None, src="default", points=16, lod=0, n=0, dx=16, dpoints=16):
    """the return code of the layer-wise entry.  Every pointer is a dummy that is never dereferenced; the default call has n_points = 0, which
    returns NIC_OK without a launch after every check has passed"""
    src = _src() if src == "default" else src
    return lib.nic_hash_encode_points_grad(_ref(d), _ref(lodp), _ref(src), P(points), P(lod), n, P(dx), P(dpoints), None)


def _fus(lib, d, lodp=None, src="default", points=16, lod=0, n=0, m="default", dy=16, target=0, loss_scale=1.0, y=0, dpoints=16):
    src = _src() if src == "default" else src
    m = _mlp() if m == "default" else m
    return lib.nic_hash_fused_points_grad(_ref(d), _ref(lodp), _ref(src), P(points), P(lod), n, _ref(m), P(dy), P(target), loss_scale, P(y), P(dpoints),
                                          None)


def _c_args(header, name):
    m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        out.append(re.sub(r"\s*\w+$", "", a) if not a.endswith("*") else a)
    return out


def test_the_symbols_are_exported_declared_and_mirrored(lib):
    from neural_image_compression_v2_amd import _lib, hashgrid
    header = open(HEADER).read()
    assert _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version()                  # additive: the version stays
    assert re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
    structs = {"nic_hash_desc": _lib.NicHashDesc, "nic_mlp": _lib.NicMlp, "nic_hash_source": _lib.NicHashSource, "nic_hash_lod": _lib.NicHashLod}
    for name, count in ((ENCODE, 9), (FUSED, 13)):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(rf"\bint\s+{name}\s*\(", header), name
        res, args = _lib.SIGNATURES[name]
        cargs = _c_args(header, name)
        assert res is ctypes.c_int and len(cargs) == len(args) == count, (name, cargs)
        for c, a in zip(cargs, args):
            if c.endswith("*"):
                base = c.replace("const", "").replace("*", "").strip()
                want = ctypes.POINTER(structs[base]) if base in structs else ctypes.c_void_p
                assert a is want or a == want, (name, c, a)
            else:
                assert a is kinds[c], (name, c, a)
    assert list(inspect.signature(hashgrid.hash_encode_points_grad).parameters) == ["geo", "data", "points", "dx", "kind", "num_bits", "lod", "lod_uniform",
                                                                                    "fade"]
    assert list(inspect.signature(hashgrid.hash_fused_points_grad).parameters) == ["geo", "data", "points", "params", "dy", "target", "loss_scale", "want_y",
                                                                                   "kind", "num_bits", "lod", "lod_uniform", "fade"]
    assert list(inspect.signature(hashgrid.HashGridField.point_gradient).parameters) == ["self", "points", "dy", "target", "scale", "lod"]
    assert list(inspect.signature(hashgrid.HashGridField.jacobian).parameters) == ["self", "points", "lod"]
    assert list(inspect.signature(hashgrid.HashGridField.query_differentiable).parameters) == ["self", "points", "lod"]


def test_the_unit_is_in_the_build_and_restates_no_shared_helper():
    """the translation unit is compiled, lies outside the hash_* glob that pins the five older units, includes the shared header and defines none
    of the helpers tests/test_hashgrid_common_cpu.py holds to one definition"""
    from neural_image_compression_v2_amd import _build
    import test_hashgrid_common_cpu as common
    assert UNIT in _build.SOURCES and len(set(_build.SOURCES)) == len(_build.SOURCES)
    assert not UNIT.startswith("hash_") and UNIT not in common.UNITS
    lines = open(os.path.join(_build.CSRC, UNIT)).read().splitlines()
    assert any(re.match(r'\s*#include\s+"hash_common\.hpp"', ln) for ln in lines)
    for name in common.FUNCTIONS + list(common.OVERLOADS) + ["load_decoder", "decoder_forward_half", "decoder_train_half", "write_record", "lattice_fixed",
                                                             "persistent_grid", "strided_grid"]:
        assert not any(common._function_re(name).match(ln) for ln in lines), name
    for name in common.STRUCTS + ["DecoderSmem", "TrainSmem", "TrainAcc"]:
        assert not any(common._struct_re(name).match(ln) for ln in lines), name
    text = "\n".join(lines)
    assert "encode_point<D, F, SRC, false, false, LOD>" in text and "point_cell<D>(" in text and "decoder_dx_half" in text
    assert "atomicAdd" not in text                                             # nothing is added anywhere


def test_argument_errors_of_the_layerwise_entry(lib):
    d = _desc()
    assert _enc(lib, d) == OK and _enc(lib, d, lodp=_lod()) == OK and _enc(lib, d, lodp=_lod(), lod=16) == OK      # n_points == 0: no launch
    # 1. the descriptor: before every pointer
    bad = _desc()
    bad.flags = 1
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(None, NULL), (bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG),
                       (_desc(extent=(257, 8, 1)), SHAPE), (_desc(num_crops=0), SHAPE), (_desc(num_crops=2), SHAPE), (big, ARG)]:
        assert _enc(lib, desc) == want
        assert _enc(lib, desc, src=None, points=0, dx=0, dpoints=0, n=-1) == want
    # 2. null pointers: before the source, the level of detail and n_points
    for kw in (dict(src=None), dict(src=_src(data=0)), dict(points=0), dict(dx=0), dict(dpoints=0)):
        assert _enc(lib, d, **kw) == NULL, kw
        assert _enc(lib, d, lodp=_lod(fade=(-1.0, 1.0)), n=-1, **kw) == NULL, kw
    assert _enc(lib, d, src=_src(U8, 0, 0), n=-1) == NULL
    # 3. the source: the rules of nic_hash_encode_points, before the level of detail
    for s in (_src(F32, 8), _src(U8, 0), _src(U8, 9), _src(BITS, 0), _src(3, 8), _src(-1, 0), _src(BITS, 4, 18)):
        assert _enc(lib, d, src=s) == ARG and _enc(lib, d, src=s, lodp=_lod(reserved=1), n=-1) == ARG, (s.kind, s.num_bits)
    for s in (_src(U8, 1), _src(U8, 8, 18), _src(BITS, 1), _src(BITS, 8), _src(BITS, 5)):
        assert _enc(lib, d, src=s) == OK, (s.kind, s.num_bits)
    # 4. the level of detail: check_lod's rules; a per-point array without the struct
    for lp in (_lod(fade=(-1.0, 1.0)), _lod(fade=(1.0, float("nan"))), _lod(fade=(float("inf"), 0.0)), _lod(lod_uniform=float("nan")),
               _lod(lod_uniform=float("inf")), _lod(reserved=1)):
        assert _enc(lib, d, lodp=lp) == ARG and _enc(lib, d, lodp=lp, n=-1) == ARG
    assert _enc(lib, d, lodp=None, lod=16) == ARG
    assert _enc(lib, _desc(resolutions=(16,)), lodp=_lod(fade=(1.0, -1.0))) == OK       # fade entries past desc->levels are ignored
    # 5. n_points
    assert _enc(lib, d, n=-1) == ARG and _enc(lib, d, n=-(1 << 40)) == ARG and _enc(lib, d, lodp=_lod(), n=-1) == ARG


def test_argument_errors_of_the_fused_entry(lib):
    d = _desc()
    assert _fus(lib, d) == OK and _fus(lib, d, dy=0, target=16, y=16) == OK and _fus(lib, d, lodp=_lod(), lod=16) == OK
    # 1. null desc / mlp
    assert _fus(lib, None) == NULL and _fus(lib, d, m=None) == NULL
    assert _fus(lib, None, src=None, points=0, dy=0, target=0, dpoints=0, n=-1) == NULL
    # 2. nic_hash_fused_supported: before every pointer
    bad = _desc()
    bad.flags = 1
    wide = _desc(resolutions=(16,) * 9, features=8)                               # L F = 72
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (_desc(extent=(257, 8, 1)), SHAPE),
                       (_desc(num_crops=0), SHAPE), (wide, UNSUP)]:
        assert _fus(lib, desc) == want
        assert _fus(lib, desc, src=None, points=0, dy=0, target=0, dpoints=0, n=-1) == want
    assert _fus(lib, d, m=_mlp(5, 5)) == UNSUP and _fus(lib, d, m=_mlp(5, 5), src=None) == UNSUP
    # 3. the conditions of the point entries
    two = _desc(num_crops=2)
    assert _fus(lib, two) == SHAPE and _fus(lib, two, src=None, dpoints=0) == SHAPE
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    assert _fus(lib, big) == ARG and _fus(lib, big, src=None) == ARG
    # 4. null pointers: before the source, the level of detail, the dy / target pair and n_points
    for kw in (dict(src=None), dict(src=_src(data=0)), dict(points=0), dict(dpoints=0), dict(m=_mlp(3, 2))):
        assert _fus(lib, d, **kw) == NULL, kw
        assert _fus(lib, d, lodp=_lod(reserved=1), dy=0, target=0, n=-1, **kw) == NULL, kw
    # 5. the source
    for s in (_src(F32, 8), _src(U8, 0), _src(U8, 9), _src(BITS, 0), _src(3, 8), _src(-1, 0), _src(BITS, 4, 18)):
        assert _fus(lib, d, src=s) == ARG and _fus(lib, d, src=s, dy=0, target=0, n=-1) == ARG, (s.kind, s.num_bits)
    for s in (_src(U8, 1), _src(U8, 8, 18), _src(BITS, 1), _src(BITS, 8), _src(BITS, 5)):
        assert _fus(lib, d, src=s) == OK, (s.kind, s.num_bits)
    # 6. the level of detail
    for lp in (_lod(fade=(-1.0, 1.0)), _lod(lod_uniform=float("nan")), _lod(reserved=1)):
        assert _fus(lib, d, lodp=lp) == ARG and _fus(lib, d, lodp=lp, dy=0, target=0, n=-1) == ARG
    assert _fus(lib, d, lodp=None, lod=16) == ARG
    # 7. exactly one of dy / target: before n_points
    assert _fus(lib, d, dy=16, target=16) == ARG and _fus(lib, d, dy=0, target=0) == ARG
    assert _fus(lib, d, dy=16, target=16, n=-1) == ARG and _fus(lib, d, dy=0, target=0, y=16, n=5) == ARG
    # 8. n_points
    assert _fus(lib, d, n=-1) == ARG and _fus(lib, d, dy=0, target=16, n=-(1 << 40)) == ARG


def test_the_field_refuses_on_the_host():
    from neural_image_compression_v2_amd import hashgrid
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, HashGridField, level_resolutions

    def bare(size=(96, 80), level_bits=None, levels=8, features=2):
        f = HashGridField.__new__(HashGridField)
        f.field_size, f.device, f.level_bits, f.table = size, torch.device("cpu"), level_bits, None
        f.geo = HashGeometry(size, tuple(level_resolutions(levels, 16, max(size))), features, 12)
        f.hidden, f.n_linear, f.route = 64, 3, "fused"
        return f
    pts, dy = torch.zeros(5, 2), torch.zeros(5, 3)
    # a bit depth per level: before everything else
    g = bare(level_bits=(8,) * 8)
    before = dict(g.__dict__)
    for call in (lambda: g.point_gradient(pts, dy=dy), lambda: g.point_gradient(pts), lambda: g.point_gradient(pts, dy=dy, target=dy),
                 lambda: g.jacobian(pts), lambda: g.query_differentiable(pts), lambda: g.query_differentiable(pts.clone().requires_grad_()),
                 lambda: g.point_gradient(pts, target=dy, lod=1.0)):
        with pytest.raises(NotImplementedError):
            call()
    assert g.__dict__ == before
    f = bare()
    before = dict(f.__dict__)
    # both or neither of dy / target
    for kw in (dict(), dict(dy=dy, target=dy), dict(lod=1.0), dict(dy=dy, target=dy, scale=2.0)):
        with pytest.raises(ValueError, match="exactly one"):
            f.point_gradient(pts, **kw)
    # shapes
    for kw in (dict(dy=torch.zeros(4, 3)), dict(dy=torch.zeros(5, 2)), dict(dy=torch.zeros(15)), dict(target=torch.zeros(6, 3)), dict(target=torch.zeros(5, 3, 1)),
               dict(dy=[[0.0] * 3] * 5)):
        with pytest.raises(ValueError, match=r"must be \[5, 3\]"):
            f.point_gradient(pts, **kw)
    for bad in (torch.zeros(5, 3), torch.zeros(5), torch.zeros(2, 5, 2)):
        with pytest.raises(ValueError, match="points must be"):
            f.point_gradient(bad, dy=dy)
    assert f.__dict__ == before                                   # nothing was set on the way to a refusal
    # the functions: the pair is decided before the table, the decoder or a device is looked at
    for kw in (dict(), dict(dy=dy, target=dy)):
        with pytest.raises(ValueError, match="exactly one"):
            hashgrid.hash_fused_points_grad(f.geo, torch.zeros(1), pts, [], **kw)
    with pytest.raises(ValueError, match=r"must be \[5, 3\]"):
        hashgrid.hash_fused_points_grad(f.geo, torch.zeros(1), pts, [], dy=torch.zeros(4, 3))
