"""Every fused-kernel instantiation the C ABI can dispatch to, each against the oracle (include/nicv2_hip.h, csrc/fused_capi.hip).

The dispatcher picks a kernel from the layout (2D triangular / sinusoidal, 3D method 3 / 4), the decoder depth, the arithmetic (fp32,
split-bf16, plain bf16, plain fp16), the grid storage (fp32, bf16, fp16), the channel counts (NIC_CP_LIST) and the level count (NIC_ML_LIST),
and every kernel has up to four modes: inference, MSE on a target tensor, MSE on the resident image, incoming dY.  ``enumerate_cells`` lists
every reachable combination: the fixed families are written down once from the routing of ``select_kernel`` (fused_capi.hip), the
channel-count and multi-level entries are read from the lists in csrc/fused_capi.hip, so a new entry there is a new case here.  What the C side
refuses with NIC_E_UNSUPPORTED is listed in ``REFUSED`` (tests/test_dispatch_lists_cpu.py asserts both lists through the C ABI).

Each cell runs one small case: several unaligned crops with ragged extents, one touching the far edge, in-kernel noise with a non-zero
``sample_base``; the MSE cell adds a single-sample crop in the far corner.  Tolerances are the suite's: the fp32 oracle via ``assert_rel`` for
the fp32 / split kernels (y 5e-6, loss 1e-5, gradients 1e-4); the precision-emulating oracle for the plain 16-bit kernels (bf16:
``check_step``, fp16: ``check_fp16``); ``_check`` of tests/test_gpu_multilevel.py for the multi-level kernels.  Image targets must give the
MSE step's y bit for bit and its loss and gradients within 1e-6; dY runs feed random signed values, not the MSE gradient, and check every
gradient against the oracle driven by the same dY (fp16: at three magnitudes, each with its own dZ scale)."""
import ctypes
import functools
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# layout id of pick_layout (fused_capi.hip) -> dim, method, triangular PE
LAYOUTS = {1: (2, 1, True), 2: (2, 1, False), 3: (3, 3, True), 4: (3, 4, False)}
MODES = ("infer", "mse", "img", "dy")
ML_MODES = ("infer", "mse")          # nic_fused_ml_forward / nic_fused_ml_forward_backward: the multi-level kernels have no image-target or dY entry
GRIDS = ("fp32", "bf16", "fp16")

# family -> (layouts, decoder depths, grid storages): the routing of fused_train / nic_fused_forward, written down once
#   fp32     no product flag: fused_kernel (32 samples x 4 waves), every layout, 3 Linear layers, fp32 grids
#   t16      NIC_FLAG_SPLIT_BF16, 2D: fused_train16 (16 samples x 8 waves); 16-bit grids train there too (their decode: fused_mlpn)
#   tile32   .. + NIC_FLAG_SPLIT_TILE32: 2D training back on fused_kernel
#   split3d  NIC_FLAG_SPLIT_BF16, 3D: fused_kernel
#   mlpn     NIC_FLAG_SPLIT_BF16, 2D, the depth-generic fused_mlpn: 5 Linear layers, or 3 with NIC_FLAG_MLPN; every grid storage
#   bf16     NIC_FLAG_BF16: the quarter kernels (fused_q16), every layout, 3 or 5 Linear layers, every grid storage
#   fp16     NIC_FLAG_FP16: the same kernels on IEEE half operands
FAMILIES = {
    "fp32": ((1, 2, 3, 4), (3,), ("fp32",)),
    "t16": ((1, 2), (3,), GRIDS),
    "tile32": ((1, 2), (3,), ("fp32",)),
    "split3d": ((3, 4), (3,), ("fp32",)),
    "mlpn": ((1, 2), (3, 5), GRIDS),
    "bf16": ((1, 2, 3, 4), (3, 5), GRIDS),
    "fp16": ((1, 2, 3, 4), (3, 5), GRIDS),
}

# family: the fixed families above, "cp" (NIC_CP_LIST on the plain-bf16 kernels) or "ml" (NIC_ML_LIST); levels = 1 off the multi-level kernels
Cell = namedtuple("Cell", "family layout C P nl grid levels mode")

# combinations the C side answers NIC_E_UNSUPPORTED for: not part of the matrix (training entry points; asserted on the CPU)
REFUSED = [
    Cell("fp32", 1, 12, 6, 5, "fp32", 1, "mse"),         # 5 Linear layers: the depth-generic kernel, split-bf16 products only
    Cell("fp32", 3, 12, 6, 5, "fp32", 1, "mse"),
    Cell("fp32", 1, 12, 6, 3, "bf16", 1, "mse"),         # 16-bit grid storage: not on the fp32 kernels
    Cell("fp32", 4, 12, 6, 3, "fp16", 1, "mse"),
    Cell("tile32", 1, 12, 6, 3, "bf16", 1, "mse"),       # .. nor on the 32-sample split kernel
    Cell("split3d", 3, 12, 6, 3, "bf16", 1, "mse"),      # .. nor on the 3D split kernels
    Cell("split3d", 4, 12, 6, 5, "fp32", 1, "mse"),      # 3D, 5 layers: plain 16-bit products only
    Cell("fp32", 1, 4, 6, 3, "fp32", 1, "mse"),          # other channel counts: the plain-bf16 kernels only
    Cell("t16", 2, 8, 6, 3, "fp32", 1, "mse"),
    Cell("fp16", 1, 4, 6, 3, "fp32", 1, "mse"),
    Cell("cp", 1, 4, 6, 5, "fp32", 1, "mse"),            # .. with 3 Linear layers
    Cell("ml", 1, 4, 6, 3, "bf16", 2, "mse"),            # the multi-level kernels read fp32 grids
]


def cp_list():
    """NIC_CP_LIST: (layout, C, P)"""
    from neural_image_compression_v2_amd import _build
    return _build.instance_list("NIC_CP_LIST")


def ml_list():
    """NIC_ML_LIST: (levels, C, n_linear)"""
    from neural_image_compression_v2_amd import _build
    return _build.instance_list("NIC_ML_LIST")


def enumerate_cells():
    cells = []
    for fam, (layouts, nls, grids) in FAMILIES.items():
        for layout in layouts:
            for nl in nls:
                for grid in grids:
                    cells += [Cell(fam, layout, 12, 6, nl, grid, 1, m) for m in MODES]
    for layout, C, P in cp_list():                           # the quarter kernels read every grid storage at every width
        for grid in GRIDS:
            cells += [Cell("cp", layout, C, P, 3, grid, 1, m) for m in MODES]
    for levels, C, nl in ml_list():
        for layout in (1, 2):                                # both positional encodings
            cells += [Cell("ml", layout, C, 6, nl, "fp32", levels, m) for m in ML_MODES]
    return cells


def cell_id(c: Cell) -> str:
    if c.family == "ml":
        return f"ml-L{c.levels}-C{c.C}-nl{c.nl}-{'tri' if c.layout == 1 else 'sin'}-{c.mode}"
    return f"{c.family}-lay{c.layout}-C{c.C}-P{c.P}-nl{c.nl}-{c.grid}-{c.mode}"


NOISE_SEED, NOISE_OFFSET, SAMPLE_BASE = 0x5EED1234ABCD, 42, 1000
SIZE = {2: (256, 256), 3: (64, 64, 64)}                    # the sampled image (base 64 / 16 pyramids at step 1/4)
EXTENT = {2: (37, 21), 3: (9, 6, 7)}
ORIGINS = {2: [(3, 5), (100, 60), (219, 235)], 3: [(3, 5, 9), (20, 0, 31), (55, 58, 57)]}     # the last crop ends at the far edge of every axis
ML_SIZE = {2: (128, 96), 3: (256, 192), 5: (1024, 1024)}
DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def geometry(c: Cell, extent, num_crops: int, **kw):
    """the PathGeometry of a cell (the product flags of its family; the grid storage is the grids' dtype)"""
    from neural_image_compression_v2_amd import _lib, fused
    dim, method, tri = LAYOUTS[c.layout]
    flags = {"fp32": {}, "t16": dict(split_bf16=True), "tile32": dict(split_bf16=True, split_tile32=True), "split3d": dict(split_bf16=True),
             "mlpn": dict(split_bf16=True, mlpn=c.nl == 3), "bf16": dict(bf16=True), "fp16": dict(fp16=True), "cp": dict(bf16=True),
             "ml": {}}[c.family]
    return fused.PathGeometry(dim=dim, method=method, step_number=0.25, mip_level=0, extent=tuple(extent), num_crops=num_crops, channels=c.C,
                              pe_channels=c.P, use_tri_pe=tri, noise_mode=_lib.NIC_NOISE_KERNEL, noise_seed=NOISE_SEED, noise_offset=NOISE_OFFSET,
                              sample_base=SAMPLE_BASE, **flags, **kw)


# ------------------------------------------------------------------------------------------------------------------------------ GPU part

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _quarter(c: Cell) -> bool:
    return c.family in ("bf16", "fp16", "cp")


def _noise(c: Cell, n: int, sample_base: int = SAMPLE_BASE):
    from oracle import nic_oracle as O
    dim, method, _ = LAYOUTS[c.layout]
    cin = O.decoder_input_channels(c.C, c.P, dim, method)
    if c.family == "cp":
        return O.kernel_noise(n, cin, 8, NOISE_SEED, NOISE_OFFSET, sample_base, layout=(dim, method, c.C, c.P))
    return O.kernel_noise(n, cin, 8, NOISE_SEED, NOISE_OFFSET, sample_base, quarter=_quarter(c))


@functools.lru_cache(maxsize=4)
def _setup(key: Cell):
    """grids (as stored and as the oracle sees them), decoder, image and the crop targets of a cell (mode-independent)"""
    from oracle import nic_oracle as O
    from tests.test_gpu_parity import _pyramid
    dim, method, _ = LAYOUTS[key.layout]
    fp, _ = _pyramid(dim, 64 if dim == 2 else 16, key.C, seed=9 + key.C + key.P)
    g0s, g1s = fp[0].to(DTYPE[key.grid]), fp[1].to(DTYPE[key.grid])
    cin = O.decoder_input_channels(key.C, key.P, dim, method)
    g = torch.Generator().manual_seed(1000 * key.layout + 10 * key.C + key.nl)
    mlp = O.init_mlp(cin, 64, generator=g, n_linear=key.nl)
    img8 = torch.randint(0, 256, (3, *SIZE[dim]), generator=g, dtype=torch.uint8)
    den = 255.0 if dim == 2 else 256.0
    imgf = img8.float() / den
    crops = [imgf[(slice(None), *(slice(o[a], o[a] + EXTENT[dim][a]) for a in range(dim)))].reshape(3, -1).T for o in ORIGINS[dim]]
    return g0s, g1s, g0s.float(), g1s.float(), mlp, img8, imgf, den, torch.cat(crops)


def _key(c: Cell) -> Cell:
    return c._replace(mode="")


@functools.lru_cache(maxsize=4)
def _oracle_mse(key: Cell, single: bool = False):
    """(emulating or None, fp32) oracle steps of the cell's MSE case, or of its single-sample crop in the far corner"""
    from oracle import nic_oracle as O
    dim, method, tri = LAYOUTS[key.layout]
    _, _, g0o, g1o, mlp, _, imgf, _, target = _setup(key)
    origins, extent = ORIGINS[dim], EXTENT[dim]
    if single:
        origins, extent = [tuple(s - 1 for s in SIZE[dim])], (1,) * dim
        target = imgf[(slice(None), *(slice(s - 1, s) for s in SIZE[dim]))].reshape(3, 1).T
    n = len(origins) * int(np.prod(extent))
    noise = _noise(key, n)
    emu = {"bf16": "bf16", "cp": "bf16", "fp16": "fp16"}.get(key.family)
    ref = O.forward_backward(g0o, g1o, mlp, origins, extent, 0.25, 0, target, noise, key.P, method=method, use_tri_pe=tri, emulate=emu) if emu else None
    ref32 = O.forward_backward(g0o, g1o, mlp, origins, extent, 0.25, 0, target, noise, key.P, method=method, use_tri_pe=tri)
    return ref, ref32, origins, extent, target


def _check_grads(c: Cell, got, ref, ref32, tag, with_outputs=True):
    """got / ref / ref32: (y, loss, g0, g1, [decoder gradients]) - y and loss None when ``with_outputs`` is False (the dY entry point)"""
    from tests.test_gpu_bf16 import check_step
    from tests.test_gpu_fp16 import check_fp16
    from tests.test_gpu_parity import assert_rel, relmax
    y, loss, g0, g1, gm = got
    names = [f"{k}{i + 1}" for i in range(c.nl) for k in ("W", "b")]
    if c.family in ("bf16", "cp", "fp16"):
        if with_outputs:
            (check_fp16 if c.family == "fp16" else check_step)(_Out(y, loss, g0, g1, gm), ref, ref32, c.nl, tag)
            return
        # the dY entry point has no y / loss: the gradients at check_step's (bf16) / check_fp16's (fp16) tolerances
        mine = dict(zip(["g0", "g1"] + names, [g0, g1] + list(gm)))
        errs = {k: relmax(a, b) for (k, a), b in zip(mine.items(), [ref.grad_g0, ref.grad_g1] + list(ref.grad_mlp))}
        e32 = {k: relmax(a, b) for (k, a), b in zip(mine.items(), [ref32.grad_g0, ref32.grad_g1] + list(ref32.grad_mlp))}
        print(f"\n[{tag}] vs emulating oracle: " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
        print(f"[{tag}] vs fp32 oracle:      " + " ".join(f"{k}={v:.1e}" for k, v in e32.items()))
        if c.family == "fp16":
            tol, tol32 = (lambda k: 1e-3), (lambda k: 3e-3)
        else:
            tol, tol32 = (lambda k: 3e-3 if k in ("g0", "g1") else 1e-3), (lambda k: 3e-2)
        bad = {k: v for k, v in errs.items() if not (np.isfinite(v) and v <= tol(k))}
        assert not bad, f"{tag}: against the emulating oracle {bad}"
        bad32 = {k: v for k, v in e32.items() if not (np.isfinite(v) and v <= tol32(k))}
        assert not bad32, f"{tag}: against the fp32 oracle {bad32}"
        return
    if with_outputs:
        assert_rel(y, ref32.y, 5e-6, f"{tag} y")
        assert_rel(loss, ref32.loss, 1e-5, f"{tag} loss")
    assert_rel(g0, ref32.grad_g0, 1e-4, f"{tag} grad G0")
    assert_rel(g1, ref32.grad_g1, 1e-4, f"{tag} grad G1")
    for nme, a, b in zip(names, gm, ref32.grad_mlp):
        assert_rel(a, b, 1e-4, f"{tag} {nme}")


_Out = namedtuple("_Out", "y loss grad_g0 grad_g1 grad_mlp")


def _backward_dy(geo, g0, g1, origins, params, dy):
    """nic_fused_backward_dy straight through the C ABI (any grid storage; PathGeometry.dz_scale_log2 as given)"""
    from neural_image_compression_v2_amd import _lib, fused
    lib = _lib.load()
    dev = g0.device
    org = fused.upload_origins(geo, origins, dev, g0, g1)
    d = geo.to_desc(g0, g1, fused.origins_aligned(geo, origins))
    gg0 = torch.zeros(g0.shape, dtype=torch.float32, device=dev)
    gg1 = torch.zeros(g1.shape, dtype=torch.float32, device=dev)
    gm = [torch.empty_like(p) for p in params]
    ws = _lib.workspace(dev, int(lib.nic_workspace_bytes(ctypes.byref(d))))
    m, gs = fused._mlp_struct(params), fused._grads_struct(gm)
    _lib.check(lib.nic_fused_backward_dy(ctypes.byref(d), _lib.ptr(g0), _lib.ptr(g1), _lib.ptr(org), ctypes.byref(m), _lib.ptr(None), _lib.ptr(dy),
                                         _lib.ptr(gg0), _lib.ptr(gg1), ctypes.byref(gs), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)),
               "nic_fused_backward_dy")
    return gg0, gg1, gm


def _run_single(dev, c: Cell):
    """one sample in the far corner: a launch with a single live lane.  One sample's gradients are that sample's products alone - nothing
    averages a rounding - so the per-row clause of ``assert_rel`` (a W1 row is dz_h x, dz_h a sum of three terms that may cancel) and, on the
    16-bit kernels, the emulating oracle's gradient bounds (one bf16 / fp16 rounding of dZ that falls the other way moves a whole tensor by
    ~2^-8) do not apply: there the outputs are held against the emulating oracle and the gradients against the fp32 oracle at 3e-2."""
    from neural_image_compression_v2_amd import fused
    from tests.test_gpu_parity import assert_rel, relmax
    key = _key(c)
    ref, ref32, origins, extent, target = _oracle_mse(key, True)
    g0s, g1s, _, _, mlp, *_ = _setup(key)
    geo = geometry(c, extent, 1)
    out = fused.fused_forward_backward(geo, g0s.to(dev), g1s.to(dev), origins, [q.to(dev) for q in mlp.tensors()], target.to(dev), want_y=True)
    tag = f"{cell_id(c)} single sample"
    names = ["G0", "G1"] + [f"{k}{i + 1}" for i in range(c.nl) for k in ("W", "b")]
    got = [out.grad_g0, out.grad_g1] + list(out.grad_mlp)
    want32 = [ref32.grad_g0, ref32.grad_g1] + list(ref32.grad_mlp)
    if c.family in ("bf16", "cp", "fp16"):
        tol_y = 2e-4 if c.family == "fp16" else 2e-3
        errs = {"y": relmax(out.y, ref.y), "loss": relmax(out.loss, ref.loss)}
        e32 = {n_: relmax(a, b) for n_, a, b in zip(names, got, want32)}
        print(f"\n[{tag}] vs emulating oracle: y={errs['y']:.1e} loss={errs['loss']:.1e}; vs fp32 oracle: " + " ".join(f"{k}={v:.1e}" for k, v in e32.items()))
        assert errs["y"] <= tol_y and errs["loss"] <= (2e-4 if c.family == "fp16" else 1e-3), (tag, errs)
        bad32 = {k: v for k, v in e32.items() if not (np.isfinite(v) and v <= 3e-2)}
        assert not bad32, f"{tag}: against the fp32 oracle {bad32}"
        return
    assert_rel(out.y, ref32.y, 5e-6, f"{tag} y", row_factor=float("inf"))
    assert_rel(out.loss, ref32.loss, 1e-5, f"{tag} loss", row_factor=float("inf"))
    for n_, a, b in zip(names, got, want32):
        assert_rel(a, b, 1e-4, f"{tag} {n_}", row_factor=float("inf"))


def _run_ml(dev, c: Cell):
    from neural_image_compression_v2_amd import fused
    from oracle import nic_oracle as O
    from tests.test_gpu_multilevel import _check, _field
    from tests.test_gpu_parity import relmax
    L, C, P, NL, tri = c.levels, c.C, c.P, c.nl, c.layout == 1
    size = ML_SIZE[L]
    fp = _field(size, L, C, 11)
    cin = L * (5 * C + 2 * P) + 1
    mlp = O.init_mlp(cin, 64, torch.Generator().manual_seed(5 + L + C + NL), n_linear=NL)
    params = [t.to(dev) for t in mlp.tensors()]
    fpd = [t.to(dev) for t in fp]
    ext = (37, 21)
    cases = [([(3, 5), (size[0] // 2 + 1, size[1] // 3), (size[0] - ext[0], size[1] - ext[1])], ext), ([(size[0] - 1, size[1] - 1)], (1, 1))]
    g = torch.Generator().manual_seed(9)
    for origins, extent in cases:
        n = len(origins) * extent[0] * extent[1]
        target = torch.rand(n, 3, generator=g)
        geo = geometry(c, extent, len(origins))
        tag = f"{cell_id(c)} {extent}"
        if c.mode == "mse":
            noise = O.kernel_noise(n, cin, 8, NOISE_SEED, NOISE_OFFSET, SAMPLE_BASE, layout=(2, 1, C, P, L))
            ref = O.multilevel_forward_backward(fp, mlp, origins, extent, target, noise, P, tri, emulate="bf16")
            ref32 = O.multilevel_forward_backward(fp, mlp, origins, extent, target, noise, P, tri)
            out = fused.fused_ml_forward_backward(geo, fpd, origins, params, target.to(dev), want_y=True)
            if n == 1:
                # one sample: bf16 arithmetic with nothing to average sits up to ~4e-2 from fp32 - the emulating oracle is the yardstick (_check's bounds)
                ref32 = ref
            _check(tag, out.y, out.loss, out.grad_fp, out.grad_mlp, ref, ref32, NL)
        else:
            ref = O.multilevel_forward_backward(fp, mlp, origins, extent, target, None, P, tri, emulate="bf16")
            ref32 = O.multilevel_forward_backward(fp, mlp, origins, extent, target, None, P, tri)
            y = fused.fused_ml_forward(geo, fpd, origins, params)
            e, e32 = relmax(y, ref[0]), relmax(y, ref32[0])
            print(f"\n[{tag}] y vs emulating oracle {e:.1e}, vs fp32 oracle {e32:.1e}")
            assert e <= 2e-3 and e32 <= 3e-2, (tag, e, e32)


@pytest.mark.parametrize("cell", enumerate_cells(), ids=cell_id)
def test_dispatch_cell(dev, cell):
    from neural_image_compression_v2_amd import fused
    from oracle import nic_oracle as O
    from tests.test_gpu_parity import relmax
    c = cell
    if c.family == "ml":
        _run_ml(dev, c)
        return
    key = _key(c)
    dim, method, tri = LAYOUTS[c.layout]
    g0s, g1s, g0o, g1o, mlp, img8, imgf, den, target = _setup(key)
    origins, extent = ORIGINS[dim], EXTENT[dim]
    n = len(origins) * int(np.prod(extent))
    g0d, g1d = g0s.to(dev), g1s.to(dev)
    params = [q.to(dev) for q in mlp.tensors()]
    geo = geometry(c, extent, len(origins))
    tag = cell_id(c)
    if c.mode in ("infer", "mse"):
        ref, ref32, *_ = _oracle_mse(key)
    if c.mode == "infer":
        y = fused.fused_forward(geo, g0d, g1d, origins, params)
        if c.family in ("bf16", "cp", "fp16"):
            e, e32 = relmax(y, ref.y), relmax(y, ref32.y)
            print(f"\n[{tag}] y vs emulating oracle {e:.1e}, vs fp32 oracle {e32:.1e}")
            tol, tol32 = (2e-4, 2e-4) if c.family == "fp16" else (2e-3, 3e-2)
            assert e <= tol and e32 <= tol32, (tag, e, e32)
        else:
            from tests.test_gpu_parity import assert_rel
            assert_rel(y, ref32.y, 5e-6, f"{tag} y")
        return
    if c.mode == "mse":
        out = fused.fused_forward_backward(geo, g0d, g1d, origins, params, target.to(dev), want_y=True)
        _check_grads(c, (out.y, out.loss, out.grad_g0, out.grad_g1, out.grad_mlp), ref, ref32, tag)
        _run_single(dev, c)
        return
    if c.mode == "img":
        base = fused.fused_forward_backward(geo, g0d, g1d, origins, params, target.to(dev), want_y=True)
        rgbx = (img8[0].int() | (img8[1].int() << 8) | (img8[2].int() << 16)).contiguous()
        for what, tgt in (("fp32 planar", fused.TargetImage(imgf.to(dev))), ("uint8 planar", fused.TargetImage(img8.to(dev), den=den)),
                          ("RGBX", fused.TargetImage(rgbx.to(dev), den=den, rgbx=True))):
            out = fused.fused_forward_backward(geo, g0d, g1d, origins, params, tgt, want_y=True)
            assert torch.equal(out.y, base.y), f"{tag} {what}: y differs from the MSE step's"
            errs = {"loss": relmax(out.loss, base.loss), "g0": relmax(out.grad_g0, base.grad_g0), "g1": relmax(out.grad_g1, base.grad_g1)}
            for i, (a, b) in enumerate(zip(out.grad_mlp, base.grad_mlp)):
                errs[f"p{i}"] = relmax(a, b)
            bad = {k: v for k, v in errs.items() if not v <= 1e-6}
            assert not bad, f"{tag} {what}: against the MSE step {bad}"
        return
    # dY: random signed values at the MSE gradient's scale (fp16: also 1e-3x and 1e3x, each with the dZ scale a caller would pick)
    noise = _noise(c, n)
    emu = {"bf16": "bf16", "cp": "bf16", "fp16": "fp16"}.get(c.family)
    gd = torch.Generator().manual_seed(31 * c.layout + c.C + c.nl)
    base_dy = (torch.rand(n, 3, generator=gd) * 2 - 1) * (2.0 / (3 * n))
    for factor in ((1.0, 1e-3, 1e3) if c.family == "fp16" else (1.0,)):
        dy = base_dy * factor
        k = int(round(np.log2(3.0 * n / factor))) + 1 if c.family == "fp16" else 0
        ref = O.forward_backward(g0o, g1o, mlp, origins, extent, 0.25, 0, None, noise, c.P, method=method, use_tri_pe=tri, emulate=emu, dy=dy,
                                 dz_scale_log2=k) if emu else None
        ref32 = O.forward_backward(g0o, g1o, mlp, origins, extent, 0.25, 0, None, noise, c.P, method=method, use_tri_pe=tri, dy=dy)
        gg0, gg1, gm = _backward_dy(geometry(c, extent, len(origins), dz_scale_log2=k), g0d, g1d, origins, params, dy.to(dev))
        _check_grads(c, (None, None, gg0, gg1, gm), ref, ref32, f"{tag} dy x{factor:g} k={k}", with_outputs=False)
