"""CPU-only tests of the training step that also returns the gradient with respect to the point coordinates (run with -m "not gpu"; DESIGN
4.7.12): nic_hash_fused_forward_backward_points_grad is exported, declared and mirrored with the same argument list, the ABI version stays 9, its
translation unit is in the build, lies outside the hash_* glob and shares the walk with hashgrid_pointgrad.hip through one header, every
argument error of the entry is decided on the host in the order the header states (fake pointers; n_points = 0 or an error, so nothing
launches), and ``HashGridField.train_points(dpoints=)`` / ``train_points_differentiable`` refuse before they touch a device or the field."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
ENTRY = "nic_hash_fused_forward_backward_points_grad"
UNIT, SHARED = "hashgrid_points_joint.hip", "hashgrid_pointgrad.hpp"
OK, NULL, UNSUP, SHAPE, WORKSPACE, ARG = 0, -1, -2, -3, -4, -5
P = ctypes.c_void_p


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


def _lod(levels=2, fade=None, lod_uniform=0.0, reserved=0):
    from neural_image_compression_v2_amd._lib import NicHashLod
    lp = NicHashLod()
    for l in range(levels):
        lp.fade[l] = 1.0 if fade is None else fade[l]
    lp.lod_uniform, lp.reserved = lod_uniform, reserved
    return lp


def _ref(x):
    return None if x is None else ctypes.byref(x)


def _call(lib, d, lodp=None, q=None, table=16, pts=16, lod=0, n=0, order=0, m="default", target=16, tg=16, gs="default", loss=16, y=0, dpoints=16,
          flags=0, ws=16, ws_bytes=1 << 30, tail=None):
    """the return code of the entry.  Every pointer is a dummy that is never dereferenced: the default call has n_points = 0, which returns
    NIC_OK without a launch after every check has passed"""
    m = _mlp() if m == "default" else m
    gs = _grads() if gs == "default" else gs
    return getattr(lib, ENTRY)(_ref(d), _ref(lodp), _ref(q), P(table), P(pts), P(lod), n, P(order), _ref(m), P(target), 1.0, P(tg), _ref(gs), P(loss),
                               P(y), P(dpoints), flags, P(ws), ws_bytes, _ref(tail), None)


def _c_args(header, name):
    m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        out.append(re.sub(r"\s*\w+$", "", a) if not a.endswith("*") else a)
    return out


def test_the_symbol_is_exported_declared_and_mirrored(lib):
    from neural_image_compression_v2_amd import _lib, hashgrid
    header = open(HEADER).read()
    assert _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version()                  # additive: the version stays
    assert re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)
    assert hasattr(lib, ENTRY) and ENTRY in _lib.SIGNATURES and re.search(rf"\bint\s+{ENTRY}\s*\(", header)
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    structs = {"nic_hash_desc": _lib.NicHashDesc, "nic_hash_lod": _lib.NicHashLod, "nic_hash_quant": _lib.NicHashQuant, "nic_mlp": _lib.NicMlp,
               "nic_mlp_grads": _lib.NicMlpGrads, "nic_step_tail": _lib.NicStepTail}
    res, args = _lib.SIGNATURES[ENTRY]
    cargs = _c_args(header, ENTRY)
    assert res is ctypes.c_int and len(cargs) == len(args) == 21, cargs
    for c, a in zip(cargs, args):
        if c.endswith("*"):
            base = c.replace("const", "").replace("*", "").strip()
            want = ctypes.POINTER(structs[base]) if base in structs else ctypes.c_void_p
            assert a is want or a == want, (c, a)
        else:
            assert a is kinds[c], (c, a)
    # the lod sibling's list with dpoints after y
    sib = list(_lib.SIGNATURES["nic_hash_fused_forward_backward_points_lod"][1])
    assert list(args) == sib[:15] + [ctypes.c_void_p] + sib[15:]
    want = list(inspect.signature(hashgrid.hash_fused_forward_backward_points_lod).parameters) + ["dpoints"]
    assert list(inspect.signature(hashgrid.hash_fused_forward_backward_points_grad).parameters) == want
    tp = inspect.signature(hashgrid.HashGridField.train_points).parameters
    assert list(tp)[-1] == "dpoints" and tp["dpoints"].default is None
    assert list(tp)[:-1] == ["self", "points", "target", "accumulate", "scale", "step", "noise", "order", "fused", "lod"]      # as they were
    assert list(inspect.signature(hashgrid.HashGridField.train_points_differentiable).parameters) == ["self", "points", "target", "kwargs"]
    for method in ("fit_points", "fit_mips"):                                  # not extended
        assert "dpoints" not in inspect.signature(getattr(hashgrid.HashGridField, method)).parameters


def test_the_unit_is_in_the_build_and_the_walk_exists_once():
    from neural_image_compression_v2_amd import _build
    import test_hashgrid_common_cpu as common
    assert UNIT in _build.SOURCES and len(set(_build.SOURCES)) == len(_build.SOURCES) and SHARED in _build.HEADERS
    for name in (UNIT, SHARED):
        assert not name.startswith("hash_") and name not in common.UNITS
    text = {name: open(os.path.join(_build.CSRC, name)).read() for name in (UNIT, SHARED, "hashgrid_pointgrad.hip")}
    for name in (UNIT, "hashgrid_pointgrad.hip"):
        lines = text[name].splitlines()
        assert any(re.match(r'\s*#include\s+"hash_common\.hpp"', ln) for ln in lines) and any(re.match(rf'\s*#include\s+"{SHARED}"', ln) for ln in lines)
        # none of the helpers tests/test_hashgrid_common_cpu.py holds to one definition is restated
        for helper in common.FUNCTIONS + list(common.OVERLOADS) + ["load_decoder", "decoder_forward_half", "decoder_train_half", "write_record",
                                                                   "persistent_grid", "strided_grid"]:
            assert not any(common._function_re(helper).match(ln) for ln in lines), (name, helper)
        for struct in common.STRUCTS + ["DecoderSmem", "TrainSmem", "TrainAcc"]:
            assert not any(common._struct_re(struct).match(ln) for ln in lines), (name, struct)
    # the walk: defined in the shared header, once, as templates on the struct they read, and in neither unit
    for helper in ("kept_axes", "point_walk_levels", "point_walk", "point_grad", "store_point_grad", "lambda_passes"):
        found = {name: sum(bool(common._function_re(helper).match(ln)) for ln in t.splitlines()) for name, t in text.items()}
        assert found == {UNIT: 0, SHARED: 1, "hashgrid_pointgrad.hip": 0}, (helper, found)
    assert text[SHARED].count("const Src& s") == 3                             # the walk, its q_tight dispatcher, the position-gradient wrapper
    joint = text[UNIT]
    for piece in ("hash_points_joint_train_kernel", "load_decoder(", "encode_point<", "decoder_train_half<KT>(", "scatter_point<", "write_record<KT>(",
                  "xcd_range(", "ordered_row(", "point_lambda(", "point_grad<", "store_point_grad<D>(", "kept_axes<D>(", "open_fused_points(",
                  "fill_fused_points(", "points_fused_step("):
        assert piece in joint, piece
    # the host path of the step is hash_common.hpp's: the tail and the end of the step are called from there, in that order
    step = open(os.path.join(_build.CSRC, common.HEADER)).read()
    step = step[step.index("inline int points_fused_step("):]
    assert 0 < step.index("set_noise(") < step.index("NIC_E_WORKSPACE") < step.index("check_fused_tail(") < step.index("finish_fused_step(")
    assert "check_fused_tail(" not in joint and "finish_fused_step(" not in joint
    assert "atomicAdd" not in joint                                            # the only atomics are scatter_point's, in the shared header


def test_argument_errors_in_the_order_the_header_states(lib):
    from neural_image_compression_v2_amd import _lib
    from neural_image_compression_v2_amd._lib import NicHashQuant
    d = _desc()
    for kw in (dict(), dict(lodp=_lod()), dict(lodp=_lod(), lod=16), dict(tg=0), dict(y=16), dict(order=16), dict(flags=3)):
        assert _call(lib, d, **kw) == OK, kw                                   # n_points == 0: NIC_OK, nothing written
    # 1. null desc / mlp
    assert _call(lib, None) == NULL and _call(lib, d, m=None) == NULL and _call(lib, None, pts=0, dpoints=0, n=-1, ws_bytes=16) == NULL
    # 2. the fused set, then the conditions of the point entries: before every pointer
    bad = _desc()
    bad.flags = 1
    wide = _desc(resolutions=(16,) * 9, features=8)                               # L F = 72
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (_desc(extent=(257, 8, 1)), SHAPE),
                       (_desc(num_crops=0), SHAPE), (wide, UNSUP), (_desc(num_crops=2), SHAPE), (big, ARG)]:
        assert _call(lib, desc) == want
        assert _call(lib, desc, table=0, pts=0, dpoints=0, flags=4, n=-1, ws_bytes=16) == want
        assert want == lib.nic_hash_fused_forward_backward_points(ctypes.byref(desc), None, P(16), P(16), 0, None, ctypes.byref(_mlp()), P(16), 1.0, P(16),
                                                                  ctypes.byref(_grads()), P(16), None, 0, P(16), 1 << 30, None, None)   # the sibling's code
    assert _call(lib, d, m=_mlp(5, 5)) == UNSUP and _call(lib, d, m=_mlp(5, 5), dpoints=0) == UNSUP
    # 3. null pointers, dpoints among them: before flags, the level of detail, quant, n_points, the workspace and the tail
    for kw in (dict(table=0), dict(pts=0), dict(target=0), dict(loss=0), dict(dpoints=0), dict(ws=0), dict(gs=None), dict(m=_mlp(3, 2))):
        assert _call(lib, d, **kw) == NULL, kw
        assert _call(lib, d, flags=4, lodp=_lod(reserved=1), q=NicHashQuant(0, 2, 1, 2, 0), n=-1, ws_bytes=16, **kw) == NULL, kw
    # 4. flags: before the level of detail
    assert _call(lib, d, flags=4) == ARG and _call(lib, d, flags=-1) == ARG
    assert _call(lib, d, flags=4, lodp=_lod(reserved=1), n=-1, ws_bytes=16) == ARG
    # 5. the nic_hash_lod's rules, 6. a per-point array without the struct: before quant (whose NIC_E_UNSUPPORTED tells the two apart)
    tensor_noise = NicHashQuant(8, 1, 1, 2, 0)
    assert _call(lib, d, q=tensor_noise) == UNSUP
    for lp in (_lod(fade=(-1.0, 1.0)), _lod(fade=(1.0, float("nan"))), _lod(fade=(float("inf"), 0.0)), _lod(lod_uniform=float("nan")),
               _lod(lod_uniform=float("inf")), _lod(reserved=1)):
        assert _call(lib, d, lodp=lp) == ARG and _call(lib, d, lodp=lp, q=tensor_noise, n=-1, ws_bytes=16) == ARG
    assert _call(lib, d, lodp=None, lod=16) == ARG and _call(lib, d, lodp=None, lod=16, q=tensor_noise, ws_bytes=16) == ARG
    assert _call(lib, _desc(resolutions=(16,)), lodp=_lod(fade=(1.0, -1.0))) == OK   # fade entries past desc->levels are ignored
    # 7. quant: before n_points
    assert _call(lib, d, q=NicHashQuant(8, 2, 1, 2, 0)) == OK
    for q in (NicHashQuant(0, 2, 1, 2, 0), NicHashQuant(9, 2, 1, 2, 0), NicHashQuant(8, 2, 1, 2, -1), NicHashQuant(8, 7, 1, 2, 0)):
        assert _call(lib, d, q=q) == ARG
    assert _call(lib, d, q=tensor_noise, n=-1, ws_bytes=16) == UNSUP
    # 8. n_points: before the workspace
    assert _call(lib, d, n=-1) == ARG and _call(lib, d, n=-(1 << 40)) == ARG and _call(lib, d, n=1 << 31, order=16) == ARG
    assert _call(lib, d, n=-1, ws_bytes=16) == ARG and _call(lib, d, lodp=_lod(), n=-1, ws_bytes=16) == ARG
    # 9. the workspace: nic_hash_fused_points_workspace_bytes, whatever n_points is; before the tail
    need = lib.nic_hash_fused_points_workspace_bytes(ctypes.byref(d), ctypes.byref(_mlp()))
    assert need > 16
    assert _call(lib, d, ws_bytes=need) == OK and _call(lib, d, ws_bytes=need - 1) == WORKSPACE and _call(lib, d, ws_bytes=16) == WORKSPACE
    # 10. the tail: its decoder entries must carry this call's gradient buffers
    gs = _grads()

    def tail_of(grad, count=1, n_stream=0, tensors="own"):
        arr = (_lib.NicAdamTensor * 1)(_lib.NicAdamTensor(0x2000, grad, 0x3000, 0x4000, 64, 1, 0.005, 1.0, -1.0, 0, 0, 0))
        t = _lib.NicStepTail()
        t.tensors = ctypes.cast(arr, ctypes.c_void_p).value if tensors == "own" else tensors
        t.count, t.n_stream, t.beta1, t.beta2, t.eps = count, n_stream, 0.9, 0.999, 1e-8
        t._keep = arr
        return t

    assert _call(lib, d, gs=gs, tail=tail_of(gs.w[0])) == OK and _call(lib, d, gs=gs, lodp=_lod(), tail=tail_of(gs.b[2])) == OK
    assert _call(lib, d, gs=gs, tail=tail_of(0x7000)) == ARG and _call(lib, d, gs=gs, tail=tail_of(0)) == ARG
    assert _call(lib, d, gs=gs, tail=tail_of(gs.w[0], tensors=0)) == NULL
    assert _call(lib, d, gs=gs, tail=tail_of(gs.w[0], count=0)) == ARG and _call(lib, d, gs=gs, tail=tail_of(gs.w[0], n_stream=2)) == ARG
    assert _call(lib, d, gs=gs, tail=tail_of(0x7000), ws_bytes=16) == WORKSPACE


def test_the_field_refuses_on_the_host():
    from neural_image_compression_v2_amd import hashgrid
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, HashGridField, level_resolutions

    def bare(size=(96, 80), level_bits=None, table="present"):
        f = HashGridField.__new__(HashGridField)
        f.field_size, f.device, f.level_bits = size, torch.device("cpu"), level_bits
        f.geo = HashGeometry(size, tuple(level_resolutions(8, 16, max(size))), 2, 12)
        f.table = None if table is None else torch.zeros(1)
        f.hidden, f.n_linear, f.route, f.frozen, f.num_bits = 64, 3, "fused", False, None
        return f
    pts, target, dp = torch.zeros(5, 2), torch.zeros(5, 3), torch.full((5, 2), 7.0)
    # a field from load_compressed: the existing refusal
    g = bare(table=None)
    before = dict(g.__dict__)
    for call in (lambda: g.train_points(pts, target, dpoints=dp), lambda: g.train_points(pts, target, fused=True, order="cell", dpoints=dp),
                 lambda: g.train_points_differentiable(pts.clone().requires_grad_(), target), lambda: g.train_points_differentiable(pts, target)):
        with pytest.raises(RuntimeError, match="decodes only"):
            call()
    assert g.__dict__ == before
    # a bit depth per level: point_gradient's refusal
    g = bare(level_bits=(8,) * 8)
    before = dict(g.__dict__)
    for call in (lambda: g.train_points(pts, target, dpoints=dp), lambda: g.train_points(pts, target, fused=True, dpoints=torch.zeros(3)),
                 lambda: g.train_points(pts, target, lod=1.0, dpoints=dp), lambda: g.train_points_differentiable(pts.clone().requires_grad_(), target)):
        with pytest.raises(NotImplementedError, match="bit depth per level"):
            call()
    assert g.__dict__ == before
    # the tensor itself: type, shape, dtype, layout, then where it lives - before the points or the target are looked at
    f = bare()
    before = dict(f.__dict__)
    with pytest.raises(TypeError, match="dpoints"):
        f.train_points(pts, target, dpoints=[[0.0, 0.0]] * 5)
    for bad in (torch.zeros(4, 2), torch.zeros(5, 3), torch.zeros(10), torch.zeros(5, 2, 1)):
        with pytest.raises(ValueError, match=r"dpoints must be \[5, 2\]"):
            f.train_points(pts, target, dpoints=bad)
    for bad in (torch.zeros(5, 2, dtype=torch.float64), torch.zeros(5, 2, dtype=torch.float16)):
        with pytest.raises(ValueError, match="dtype"):
            f.train_points(pts, target, fused=True, dpoints=bad)
    with pytest.raises(ValueError, match="contiguous"):
        f.train_points(pts, target, dpoints=torch.zeros(2, 5).t())
    for bad in (torch.zeros(5, 3), torch.zeros(5), [[0.0, 0.0]] * 5):
        with pytest.raises(ValueError, match="points must be"):
            f.train_points(bad, target, dpoints=dp)
    with pytest.raises(RuntimeError, match="HIP device"):                       # a host tensor of the right shape: no CPU path
        f.train_points(pts, target, dpoints=dp)
    with pytest.raises(TypeError, match="dpoints"):
        f.train_points_differentiable(pts.clone().requires_grad_(), target, dpoints=dp)
    assert f.__dict__ == before and bool((dp == 7.0).all())                     # nothing was set or written on the way to a refusal
    # the function: the tensor is decided before the table, the decoder or a device is looked at
    with pytest.raises(ValueError, match=r"dpoints must be \[5, 2\]"):
        hashgrid.hash_fused_forward_backward_points_grad(f.geo, torch.zeros(1), pts, [], target, [], dpoints=torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        hashgrid.hash_fused_forward_backward_points_grad(f.geo, torch.zeros(1), pts, [], target, [])
