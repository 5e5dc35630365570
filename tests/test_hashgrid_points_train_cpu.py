"""CPU-only tests of cell-ordered and fused training at points (run with -m "not gpu"): the four new C ABI symbols are exported, declared and
mirrored with matching argument lists, the ABI version stays 9, the new source is part of the build, every argument error of the new entry points
is decided on the host (fake pointers, nothing launches, codes in the order of the siblings), the workspace query refuses what the entry refuses,
and the Python layer refuses bad input before the library."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
NEW_SYMBOLS = ("nic_hash_point_keys", "nic_hash_encode_points_backward_ordered", "nic_hash_fused_points_workspace_bytes",
               "nic_hash_fused_forward_backward_points")
OK, NULL, UNSUP, SHAPE, WORKSPACE, ARG = 0, -1, -2, -3, -4, -5
P = ctypes.c_void_p


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


def _c_args(header, name):
    """the parameter list of ``name``'s declaration in the header, one normalised C type per parameter"""
    m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        out.append(re.sub(r"\s*\w+$", "", a) if not a.endswith("*") else a)      # drop the parameter's name
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
    assert "hash_points_train.hip" in _build.SOURCES and "hash_common.hpp" in _build.HEADERS
    assert os.path.exists(os.path.join(_build.CSRC, "hash_points_train.hip")) and os.path.exists(os.path.join(_build.CSRC, "hash_common.hpp"))
    # the mirror against the header, argument by argument: pointers are void* / struct pointers, n_points int64, sizes size_t, the scale a float
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    structs = {"nic_hash_desc": _lib.NicHashDesc, "nic_hash_quant": _lib.NicHashQuant, "nic_mlp": _lib.NicMlp, "nic_mlp_grads": _lib.NicMlpGrads,
               "nic_step_tail": _lib.NicStepTail}
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
        assert res is (ctypes.c_size_t if n.endswith("workspace_bytes") else ctypes.c_int)
    assert "There is no fused training at points" not in header
    # the key's definition is stated in the header
    for word in ("Morton", "j dim + a", "max(0, b - k)"):
        assert word in header, word
    for n in ("hash_point_keys", "hash_point_order", "hash_encode_points_backward", "hash_fused_forward_backward_points"):
        assert callable(getattr(hashgrid, n)), n
    for n in ("train_points", "fit_points"):
        assert callable(getattr(hashgrid.HashGridField, n)), n


def _keys(lib, d, pts=16, n=0, keys=16):
    return lib.nic_hash_point_keys(None if d is None else ctypes.byref(d), P(pts), n, P(keys), None)


def _bwd(lib, d, pts=16, n=0, dx=16, order=16, grad=16):
    return lib.nic_hash_encode_points_backward_ordered(None if d is None else ctypes.byref(d), P(pts), n, P(dx), P(order), P(grad), None)


def _full_ws(lib, d, m=None):
    m = _mlp() if m is None else m
    return lib.nic_hash_fused_points_workspace_bytes(ctypes.byref(d), ctypes.byref(m))


def _fb(lib, d, m="default", q=None, table=16, pts=16, n=0, order=0, target=16, tg=16, gs="default", loss=16, y=0, flags=0, ws=16, ws_bytes=1 << 30,
        tail=None):
    m = _mlp() if m == "default" else m
    gs = _grads() if gs == "default" else gs
    return lib.nic_hash_fused_forward_backward_points(None if d is None else ctypes.byref(d), None if q is None else ctypes.byref(q), P(table), P(pts), n,
                                                      P(order), None if m is None else ctypes.byref(m), P(target), 1.0, P(tg),
                                                      None if gs is None else ctypes.byref(gs), P(loss), P(y), flags, P(ws), ws_bytes,
                                                      None if tail is None else ctypes.byref(tail), None)


def _all(lib, d):
    return (_keys(lib, d), _bwd(lib, d), _fb(lib, d))


def test_descriptor_errors_come_first_with_the_siblings_codes(lib):
    d = _desc()
    assert _all(lib, d) == (OK, OK, OK)
    assert _all(lib, None) == (NULL, NULL, NULL)
    bad = _desc()
    bad.flags = 1
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (_desc(resolutions=()), ARG),
                       (_desc(resolutions=(1 << 20,), s_max=1 << 11, extent=(8, 8, 1)), ARG), (_desc(extent=(3841, 8, 1)), SHAPE),
                       (_desc(extent=(8, 0, 1)), SHAPE), (_desc(num_crops=2), SHAPE), (_desc(num_crops=0), SHAPE)]:
        assert _all(lib, desc) == (want, want, want)
        assert lib.nic_hash_encode_points_backward(ctypes.byref(desc), P(16), 0, P(16), P(16), None) == want        # the sibling's code
        assert _full_ws(lib, desc) == 0
    # 256 S_max < 2^30
    big = 1 << 22
    assert _all(lib, _desc(s_max=big, extent=(big, 8, 1))) == (ARG, ARG, ARG)
    assert _full_ws(lib, _desc(s_max=big, extent=(big, 8, 1))) == 0
    assert _all(lib, _desc(s_max=big - 1, extent=(big - 1, 8, 1))) == (OK, OK, OK)
    # the descriptor comes before the pointers, the pointers before the arguments
    assert (_keys(lib, bad, pts=0), _bwd(lib, bad, pts=0), _fb(lib, bad, pts=0)) == (ARG, ARG, ARG)
    assert (_keys(lib, d, pts=0, n=-1), _bwd(lib, d, pts=0, n=-1), _fb(lib, d, pts=0, n=-1)) == (NULL, NULL, NULL)
    # 4K and 256^3 at the flagship settings pass
    from neural_image_compression_v2_amd.hashgrid import level_resolutions
    assert _all(lib, _desc(resolutions=tuple(level_resolutions(16, 16, 3840)))) == (OK, OK, OK)
    assert _all(lib, _desc(dim=3, resolutions=tuple(level_resolutions(16, 16, 256)), s_max=256, extent=(256, 256, 256))) == (OK, OK, OK)


def test_keys_and_ordered_scatter_argument_errors(lib):
    d = _desc()
    assert _keys(lib, d, pts=0) == NULL and _keys(lib, d, keys=0) == NULL
    assert _keys(lib, d, n=-1) == ARG and _keys(lib, d, n=-(1 << 40)) == ARG
    assert _bwd(lib, d, pts=0) == NULL and _bwd(lib, d, dx=0) == NULL and _bwd(lib, d, grad=0) == NULL
    assert _bwd(lib, d, n=-1) == ARG
    # n_points >= 2^31 needs int32 indices that do not exist: refused with an order.  (Without one the call IS the unordered entry, which
    # would launch; its own n_points checks are the sibling's and are swept in test_hashgrid_points_cpu.py.)
    assert _bwd(lib, d, n=1 << 31) == ARG and _bwd(lib, d, n=1 << 40) == ARG
    assert _bwd(lib, d, n=-1, order=0) == ARG and _bwd(lib, d, n=0, order=0) == OK and _bwd(lib, d, pts=0, order=0) == NULL


def test_fused_points_argument_errors(lib):
    from neural_image_compression_v2_amd import _lib
    from neural_image_compression_v2_amd._lib import NicHashQuant
    d = _desc()
    assert _fb(lib, d) == OK
    # null pointers: mlp, its layers, and every required buffer; table_grad, y, order, quant and tail may be null
    assert _fb(lib, d, m=None) == NULL
    assert _fb(lib, d, m=_mlp(layers=2)) == NULL
    for name in ("table", "pts", "target", "loss", "ws"):
        assert _fb(lib, d, **{name: 0}) == NULL, name
    assert _fb(lib, d, gs=None) == NULL
    assert _fb(lib, d, tg=0) == OK and _fb(lib, d, y=16) == OK and _fb(lib, d, order=16) == OK
    # the fused set first: nic_hash_fused_supported's answer, before the pointers
    wide = _desc(resolutions=tuple(range(16, 33)), features=4)                   # 17 x 4 = 68 columns
    assert lib.nic_hash_fused_supported(ctypes.byref(wide), 64, 3) == UNSUP
    assert _fb(lib, wide) == UNSUP and _fb(lib, wide, table=0) == UNSUP and _full_ws(lib, wide) == 0
    assert _fb(lib, d, m=_mlp(n_linear=5, layers=5)) == UNSUP and _full_ws(lib, d, _mlp(n_linear=5, layers=5)) == 0
    assert _fb(lib, d, m=_mlp(n_linear=0)) == OK
    assert (_keys(lib, wide), _bwd(lib, wide)) == (OK, OK)                       # the layer-wise entries take that shape
    # flags, quant: nic_hash_fused_forward_backward's checks
    assert _fb(lib, d, flags=4) == ARG and _fb(lib, d, flags=3) == OK
    assert _fb(lib, d, q=NicHashQuant(8, 2, 1, 2, 0)) == OK
    assert _fb(lib, d, q=NicHashQuant(0, 2, 1, 2, 0)) == ARG
    assert _fb(lib, d, q=NicHashQuant(8, 2, 1, 2, -1)) == ARG
    assert _fb(lib, d, q=NicHashQuant(8, 1, 1, 2, 0)) == UNSUP                   # NIC_NOISE_TENSOR
    assert _fb(lib, d, q=NicHashQuant(8, 7, 1, 2, 0)) == ARG
    # n_points
    assert _fb(lib, d, n=-1) == ARG
    assert _fb(lib, d, n=1 << 31, order=16) == ARG
    # the workspace: the query's size, whatever n_points is
    need = _full_ws(lib, d)
    assert need > 0 and need % 4 == 0
    assert _fb(lib, d, ws_bytes=need) == OK
    assert _fb(lib, d, ws_bytes=need - 1) == WORKSPACE and _fb(lib, d, ws_bytes=0) == WORKSPACE
    assert _fb(lib, d, ws_bytes=16, n=-1) == ARG                                 # the arguments come before the workspace
    assert need == lib.nic_hash_fused_workspace_bytes(ctypes.byref(d), ctypes.byref(_mlp()))      # the same records as the crop step
    # the tail: its decoder entries must carry this call's gradient buffers
    gs = _grads()

    def tail_of(grad, count=1, n_stream=0, tensors="own"):
        arr = (_lib.NicAdamTensor * 1)(_lib.NicAdamTensor(0x2000, grad, 0x3000, 0x4000, 64, 1, 0.005, 1.0, -1.0, 0, 0, 0))
        t = _lib.NicStepTail()
        t.tensors = ctypes.cast(arr, ctypes.c_void_p).value if tensors == "own" else tensors
        t.count, t.n_stream, t.beta1, t.beta2, t.eps = count, n_stream, 0.9, 0.999, 1e-8
        t._keep = arr
        return t

    assert _fb(lib, d, gs=gs, tail=tail_of(gs.w[0])) == OK                       # n_points = 0: nothing launches
    assert _fb(lib, d, gs=gs, tail=tail_of(gs.b[2])) == OK
    assert _fb(lib, d, gs=gs, tail=tail_of(0x7000)) == ARG                       # some other buffer
    assert _fb(lib, d, gs=gs, tail=tail_of(0)) == ARG
    assert _fb(lib, d, gs=gs, tail=tail_of(gs.w[0], tensors=0)) == NULL
    assert _fb(lib, d, gs=gs, tail=tail_of(gs.w[0], count=0)) == ARG
    assert _fb(lib, d, gs=gs, tail=tail_of(gs.w[0], n_stream=2)) == ARG
    assert _fb(lib, d, gs=gs, tail=tail_of(0x7000), ws_bytes=16) == WORKSPACE    # the workspace before the tail, as in the crop sibling


def test_python_side_checks_on_the_host():
    from neural_image_compression_v2_amd import hashgrid
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, HashGridField, level_resolutions
    geo = HashGeometry((256, 256), tuple(level_resolutions(8, 16, 256)), 2, 12)
    pts = torch.zeros(5, 2)
    table = torch.zeros(geo.table_shape())
    # nothing on the CPU: no fallback
    with pytest.raises(RuntimeError, match="HIP device"):
        hashgrid.hash_point_keys(geo, pts)
    with pytest.raises(RuntimeError, match="HIP device"):
        hashgrid.hash_point_order(geo, pts)
    with pytest.raises(RuntimeError, match="HIP device"):
        hashgrid.hash_fused_forward_backward_points(geo, table, pts, [], torch.zeros(5, 3), [])
    # the order: int32, one-dimensional, on the device, one index per point
    dev = torch.device("cuda:0")
    for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros(5, dtype=torch.int32), torch.zeros(5, 1, dtype=torch.int32), [0, 1, 2, 3, 4], "raster"):
        with pytest.raises(ValueError, match="order"):
            hashgrid._check_order(bad, 5, dev)
    # a field too large for 8 fractional bits is refused by name, before the library
    huge = HashGeometry((1 << 22, 8), (16,), 2, 12)
    with pytest.raises(ValueError, match="2\\^30"):
        hashgrid._point_desc(huge)
    # train_points / fit_points on a host-built stand-in: every refusal below is decided before the library or the device is touched
    f = HashGridField.__new__(HashGridField)
    f.table = None
    with pytest.raises(RuntimeError, match="decodes only"):
        f.train_points(pts, torch.zeros(5, 3), order="cell", fused=True)

    class _Dec:
        def linear_params(self):
            return []

    f.table, f.decoder, f.frozen, f.num_bits, f.geo, f.route = table.requires_grad_(True), _Dec(), False, None, geo, "layerwise"
    import neural_image_compression_v2_amd._lib as L
    real = L.require_cuda_f32
    L.require_cuda_f32 = lambda t, name: t                                       # let host tensors reach the argument checks
    try:
        with pytest.raises(ValueError, match="fused=True"):
            f.train_points(pts, torch.zeros(5, 3), fused=True)
        with pytest.raises(ValueError, match="fused=True"):
            f.fit_points(pts, torch.zeros(5, 3), epochs=1, fused=True)
        for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), "morton"):
            with pytest.raises(ValueError, match="order"):
                f.train_points(pts, torch.zeros(5, 3), order=bad)
        with pytest.raises(ValueError, match="target"):
            f.train_points(pts, torch.zeros(4, 3), order="cell")
        with pytest.raises(ValueError, match="batch"):
            f.fit_points(pts, torch.zeros(5, 3), epochs=1, batch=0, order=None, fused=False)
    finally:
        L.require_cuda_f32 = real
