"""CPU-only tests of the gradient with respect to the level of detail (run with -m "not gpu"): nic_hash_encode_points_grad_lod and
nic_hash_fused_points_grad_lod are exported, declared in the companion header include/nicv2_hip_ext.h alone and mirrored in _lib.EXT_SIGNATURES
argument for argument (the ABI version stays 9, the main header's 86 entries stay); every argument error is decided on the host in the documented
order (fake pointers and refusals only: nothing launches); the unit and its header are in the build.

The float64 reference ``reference`` is built from oracle/hashgrid_train_ref.py's own pieces - ``rows``, ``encode`` and ``decoder``, with the [N, L]
weights of ``level_weights`` as a leaf: ``torch.autograd`` gives d loss / d weights, and dlod = - sum over the levels on the ramp of it, ramp
membership and the clamp of lambda decided in fp32 as the header defines them.  It is held to differences of its own float64 loss in lambda:
central ones (step 2^-10) away from the kinks and one-sided ones from the right exactly on them, both to 1e-9 - with the loss sum(dx * row), which
is affine in lambda inside a piece, so that a difference quotient is the derivative up to rounding (through the decoder a central difference of
step h is h^2 / 6 x the third derivative away from it, 1.6e-7 x: no test of 1e-9).

Teeth, on the inputs tests/test_gpu_hashgrid_lodgrad.py uses: the left-hand convention, a flipped sign and ``r`` taken weighed each move dlod by
far more than the GPU tests' bound.  The descent of test 7 and the central differences of test 4 of the GPU file are run here on the reference:
their conditions are met with room by the definition itself.

``inputs``, ``reference`` and the descent loop are shared with the GPU file: both sides see the same bytes."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import hashgrid_train_ref as T
from tests.test_hashgrid_batch_points_cpu import ARG, NULL, OK, SHAPE, UNSUP, HEADER, EXT_HEADER, _desc, _mlp, _ref, lib  # noqa: F401
from tests.test_hashgrid_batch_lod_cpu import _bad_lods, _lod, _src

ENC, FUSED = "nic_hash_encode_points_grad_lod", "nic_hash_fused_points_grad_lod"
ARGS = {ENC: ["desc", "lodp", "src", "points", "lod", "n_points", "dx", "dpoints", "dlod", "stream"],
        FUSED: ["desc", "lodp", "src", "points", "lod", "n_points", "mlp", "dy", "target", "loss_scale", "y", "dpoints", "dlod", "stream"]}
SIBLINGS = {ENC: "nic_hash_encode_points_grad", FUSED: "nic_hash_fused_points_grad"}
PTR = ctypes.c_void_p
UNIT, WALK = "hashgrid_lodgrad.hip", "hashgrid_pointgrad.hpp"
F32 = np.float32
TOL_G = 1e-4            # tests/test_gpu_hashgrid_pointgrad.py's: of the largest magnitude of the compared tensor

# ------------------------------------------------------------------------------------------------------------------ shared with the GPU file
N = 130                                                   # two waves and two lanes of a third
SIZES = {2: (13, 9), 3: (7, 6, 5)}
RESOLUTIONS = {2: (2, 5, 13, 34, 40), 3: (2, 4, 8, 16, 20)}   # the first `levels` of them: from 2 up to >= S_max; log2_table 10: dense, dense, dense, hashed ..
LOG2_TABLE = 10
FADES = {4: (3.0, 2.0, 0.5, 0.0), 5: (3.0, 2.0, 1.25, 0.5, 0.0)}
MAX_FADE = 3.0
# the level of detail of a launch: (per point?, lod_uniform)
MODES = {"point": (True, 0.0), "uniform": (False, 1.0), "both": (True, 0.5)}   # uniform 1.0: fade 0.0 exactly at its end, fade 0.5 half way down
TARGET_SCALE = 3.0                                        # loss_scale = 3 n with a target: the output gradient is 2 (y - target), of dy's size
OUTSIDE_ROWS = (20, 21, 22, 23, 129)                      # rows whose point lies outside the field (one of them a NaN), each with a level on the ramp
H_GPU = 0.125                                             # the step of the GPU file's central differences


def lod_rows(fade):
    """the 130 values of lambda: a row exactly at fade[l] (a_raw == 1) and at fade[l] + 1 (a_raw == 0) for every l; 0, -1, 32, 40 and NaN; random
    in [0, max fade + 1.5]; rows 64 .. 127, one whole wave, with every level off; rows 128, 129 (the third wave) at 2.5, where the levels of
    fade <= 1.5 are live for no lane of that wave"""
    g = torch.Generator().manual_seed(17)
    lod = (torch.rand(N, generator=g) * (MAX_FADE + 1.5)).numpy().astype(F32)
    k = 0
    for f in fade:
        lod[k], lod[k + 1] = f, f + 1.0
        k += 2
    lod[k:k + 5] = [0.0, -1.0, 32.0, 40.0, float("nan")]
    assert k + 5 <= 20
    lod[20:24] = [0.5, 2.75, 2.25, 3.5]
    lod[64:128] = MAX_FADE + 1.0 + (torch.rand(64, generator=g) * 2.0).numpy().astype(F32)
    lod[64] = MAX_FADE + 1.0
    lod[128:] = 2.5
    return lod


def decoder_params(width, seed, amps=(3.0, 2.0, 2.0), bias=1.0):
    """a 64-64-3 decoder, uniform in +- amp / sqrt(fan in) (biases +- ``bias`` / sqrt(fan in)): it does something with its input"""
    g = torch.Generator().manual_seed(seed)

    def u(*shape, amp):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * amp).contiguous()
    k1, k2 = width ** -0.5, 64 ** -0.5
    return [u(64, width, amp=amps[0] * k1), u(64, amp=bias * k1), u(64, 64, amp=amps[1] * k2), u(64, amp=bias * k2), u(3, 64, amp=amps[2] * k2),
            u(3, amp=bias * k2)]


@functools.lru_cache(maxsize=None)
def inputs(dim, features, levels=4):
    """everything a case reads, as fp32 CPU tensors (read-only: shared between tests): the geometry twice (the package's and the oracle's), a
    table uniform in +- 0.5, the decoder, 130 points (five of them outside the field), dx, dy, target, the fades and lambda per point"""
    from neural_image_compression_v2_amd.hashgrid import HashGeometry
    size, res = SIZES[dim], RESOLUTIONS[dim][:levels]
    geo = HashGeometry(size, res, features, LOG2_TABLE)
    tgeo = T.Geometry(size, res, features, LOG2_TABLE)
    dense = [T.level_dense(tgeo, l) for l in range(levels)]
    assert any(dense) and not all(dense) and res[0] == 2 and res[-1] >= max(size)
    g = torch.Generator().manual_seed(1000 * dim + 10 * features + levels)
    table = (torch.rand(levels, 1 << LOG2_TABLE, features, generator=g) - 0.5).contiguous()
    points = torch.rand(N, dim, generator=g) * torch.tensor([float(s) for s in size]) - 0.5
    points[20, 0] = -3.0
    points[21, 1] = size[1] + 2.0
    points[22] = torch.tensor([-1.0, size[1] + 0.25, 99.0][:dim])
    points[23, 0] = float("nan")
    points[129, 0] = size[0] + 1.0
    dx = torch.rand(N, levels * features, generator=g) * 2 - 1
    dy = torch.rand(N, 3, generator=g) * 2 - 1
    target = torch.rand(N, 3, generator=g)
    fade = FADES[levels]
    return types.SimpleNamespace(geo=geo, tgeo=tgeo, table=table, params=decoder_params(levels * features, 7 * dim + features), points=points.contiguous(),
                                 dx=dx, dy=dy, target=target, fade=fade, lod=lod_rows(fade))


def mode_lod(inp, mode, n=N):
    """(lod [n] or None, lod_uniform) of a launch of the first n rows"""
    per_point, u = MODES[mode]
    return (inp.lod[:n].copy() if per_point else None), u


def ramp_f32(fade, lod, lod_uniform, n):
    """(a_raw [n, L], on the ramp [n, L], the clamp of lambda passes [n]) in fp32, as the header defines them: lambda_raw = (lod or 0) +
    lod_uniform; passes iff 0 <= lambda_raw < 32 (a NaN does not); lambda = lambda_raw with NaN -> 0 clamped to [0, 32]; a_raw = (fade - lambda) + 1
    in that order; on the ramp iff 0 < a_raw <= 1"""
    with np.errstate(invalid="ignore"):
        raw = ((np.zeros(n, dtype=F32) if lod is None else np.asarray(lod, dtype=F32).reshape(n)) + F32(lod_uniform)).astype(F32)
        passes = (raw >= 0) & (raw < 32)
        lam = np.where(np.isnan(raw), F32(0), raw).astype(F32)
        lam = np.minimum(np.maximum(lam, F32(0)), F32(32))
    a_raw = ((np.asarray(fade, dtype=F32).reshape(1, -1) - lam[:, None]).astype(F32) + F32(1)).astype(F32)
    return a_raw, (a_raw > 0) & (a_raw <= 1), passes


def reference(tgeo, values, params, points, fade, lod, lod_uniform, dx=None, dy=None, target=None, loss_scale=1.0):
    """float64, from the oracle's own pieces.  ``values`` [L, T, F]: what the forward blends.  The loss is sum(dx * row) (the layer-wise entry),
    sum(dy * y), or mean((y - target)^2) * loss_scale - exactly one.  Returns y, row, dpoints (the oracle's own), dlod, and what the teeth need:
    d loss / d weights ``dW``, the weights ``W``, ``a_raw``, ``ramp`` and ``passes``"""
    assert sum(v is not None for v in (dx, dy, target)) == 1
    tab = T.as_f64(values)
    tables = [tab[l] for l in range(tgeo.levels)]
    ps = [T.as_f64(p) for p in params]
    n = points.shape[0]
    lod = None if lod is None else np.asarray(lod, dtype=F32)
    with torch.enable_grad():                                                # also when called from an autograd Function
        pos = T.rows(tgeo, points=points)
        W = torch.from_numpy(T.level_weights(tgeo, n, fade, lod, lod_uniform)).requires_grad_(True)
        row = T.encode(tgeo, tables, pos, None, W)
        y = T.decoder(row, ps)
        if dx is not None:
            loss = (row * T.as_f64(dx)).sum()
        elif dy is not None:
            loss = (y * T.as_f64(dy)).sum()
        else:
            loss = T.mse(y, T.as_f64(target)) * float(loss_scale)
        dW, dp = torch.autograd.grad(loss, [W, pos.points], allow_unused=True)
    dp = torch.zeros_like(pos.points) if dp is None else dp
    a_raw, ramp, passes = ramp_f32(fade, lod, lod_uniform, n)
    dlod = -(dW * torch.from_numpy(ramp)).sum(dim=1) * torch.from_numpy(passes)
    return types.SimpleNamespace(y=y.detach(), row=row.detach(), dpoints=dp, dlod=dlod, dW=dW, W=W.detach(), a_raw=a_raw, ramp=ramp, passes=passes)


def rel(a, b):
    """the largest difference as a share of the largest magnitude of the reference ``b``"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max())


# ---- the central differences of the GPU file (its test 4): lambda per row, and the rows whose weights stay inside one linear piece
def affine_lod():
    """130 multiples of 1/16 in [1/8, max fade + 1.5]"""
    g = torch.Generator().manual_seed(23)
    return (torch.randint(2, int(16 * (MAX_FADE + 1.5)) + 1, (N,), generator=g).double() / 16.0).numpy().astype(F32)


def affine_rows(fade, lod, h=H_GPU):
    """rows where every level keeps its piece over [lambda - h, lambda + h]: off (a_raw + h <= 0), on the ramp (0 <= a_raw - h and a_raw + h <= 1)
    or at full weight (a_raw - h >= 1), and lambda - h >= 0.  All of it is exact in fp32: fades and lambda are multiples of 1/16"""
    a_raw, _, _ = ramp_f32(fade, lod, 0.0, lod.shape[0])
    piece = (a_raw + h <= 0) | ((a_raw - h >= 0) & (a_raw + h <= 1)) | (a_raw - h >= 1)
    return piece.all(axis=1) & (lod - h >= 0)


# the decoder of the central differences: no biases, small hidden layers and a large output layer - close to linear over a step of 1/8 in
# lambda, with outputs that still move by a few 1e-2 per unit of lambda (both asserted below on the reference)
GENTLE = dict(amps=(0.25, 0.5, 48.0), bias=0.0)


# ---- the descent of the GPU file (its test 7)
DESCENT = dict(size=(64, 64), resolutions=(4, 8, 16, 32), features=2, log2_table=12, n=256, lam0=1.25, start=2.0, lr=0.02, steps=200, seed=5)


def descent_inputs():
    """(HashGeometry, oracle Geometry, table [4, 4096, 2] uniform in +- 0.5, decoder, 256 points inside the field); the default fades are 4, 3, 2, 1:
    at lambda0 = 1.25 the finest level is on the ramp, at the start 2.0 it is exactly at its end and the next one exactly at its start"""
    from neural_image_compression_v2_amd.hashgrid import HashGeometry
    d = DESCENT
    geo = HashGeometry(d["size"], d["resolutions"], d["features"], d["log2_table"])
    tgeo = T.Geometry(d["size"], d["resolutions"], d["features"], d["log2_table"])
    g = torch.Generator().manual_seed(d["seed"])
    table = (torch.rand(*geo.table_shape(), generator=g) - 0.5).contiguous()
    points = (torch.rand(d["n"], 2, generator=g) * 62.0 + 0.5).contiguous()
    return geo, tgeo, table, decoder_params(geo.width, d["seed"]), points


def run_descent(query_lod, points, device):
    """the loop the field and the reference both run: colours from query(p, lambda0), lambda_hat from ``start`` by torch Adam on a 0-dim fp32
    tensor; returns (first loss, last loss, lambda_hat)"""
    d = DESCENT
    with torch.no_grad():
        colours = query_lod(points, torch.tensor(d["lam0"], dtype=torch.float32, device=device)).detach()
    lam = torch.tensor(d["start"], dtype=torch.float32, device=device, requires_grad=True)
    opt = torch.optim.Adam([lam], lr=d["lr"])
    losses = []
    for _ in range(d["steps"] + 1):
        opt.zero_grad()
        loss = ((query_lod(points, lam) - colours) ** 2).mean()
        losses.append(float(loss.detach()))
        if len(losses) <= d["steps"]:
            loss.backward()
            opt.step()
    return losses[0], losses[-1], float(lam.detach())


class ReferenceQuery(torch.autograd.Function):
    """the float64 reference as the same differentiable op of a 0-dim lambda (rounded to fp32 first, as the field receives it)"""

    @staticmethod
    def forward(ctx, lam, tgeo, table, params, points, fade):
        ctx.args = (tgeo, table, params, points, fade, float(F32(float(lam))))
        n = points.shape[0]
        return reference(tgeo, table, params, points, fade, None, ctx.args[5], dy=torch.zeros(n, 3)).y.to(lam.dtype)

    @staticmethod
    def backward(ctx, dy):
        tgeo, table, params, points, fade, lam = ctx.args
        return reference(tgeo, table, params, points, fade, None, lam, dy=dy).dlod.sum().to(dy.dtype), None, None, None, None, None


# ------------------------------------------------------------------------------------------------------------------ the C entries
def _enc(lib, d, lodp="default", src="default", points=16, lod=0, n_points=0, dx=16, dpoints=16, dlod=16):
    """the return code of the layer-wise entry with dummy pointers; only calls a host check refuses, or n_points == 0, are made: nothing launches"""
    lodp = _lod() if lodp == "default" else lodp
    src = _src() if src == "default" else src
    assert n_points <= 0
    return lib.nic_hash_encode_points_grad_lod(_ref(d), _ref(lodp), _ref(src), PTR(points), PTR(lod), n_points, PTR(dx), PTR(dpoints), PTR(dlod), None)


def _fus(lib, d, lodp="default", src="default", points=16, lod=0, n_points=0, m="default", dy=16, target=0, y=16, dpoints=16, dlod=16):
    lodp = _lod() if lodp == "default" else lodp
    src = _src() if src == "default" else src
    m = _mlp() if m == "default" else m
    assert n_points <= 0
    return lib.nic_hash_fused_points_grad_lod(_ref(d), _ref(lodp), _ref(src), PTR(points), PTR(lod), n_points, _ref(m), PTR(dy), PTR(target), 1.0, PTR(y),
                                              PTR(dpoints), PTR(dlod), None)


def test_the_entries_are_exported_declared_in_the_companion_header_only_and_mirrored(lib):
    from neural_image_compression_v2_amd import _lib, hashgrid
    import neural_image_compression_v2_amd as pkg
    header, ext = open(HEADER).read(), open(EXT_HEADER).read()
    types_of = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    for name, names in ARGS.items():
        assert hasattr(lib, name)
        assert name not in header and name not in _lib.SIGNATURES and name in _lib.EXT_SIGNATURES
        res, args = _lib.EXT_SIGNATURES[name]
        m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", ext, re.S)
        assert m, name
        cargs = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert len(cargs) == len(args) == len(names), (name, cargs)
        assert res is ctypes.c_int
        for c, a in zip(cargs, args):
            if "*" in c:
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (name, c)
            else:
                assert a is types_of[c.split()[0]], (name, c)
        assert [c.split()[-1].lstrip("*") for c in cargs] == names
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        # the sibling argument for argument, with dlod after dpoints
        sib = re.search(rf"\b{SIBLINGS[name]}\s*\(([^;]*?)\)\s*;", header, re.S)
        sargs = [" ".join(a.split()) for a in sib.group(1).split(",")]
        k = [c.split()[-1].lstrip("*") for c in sargs].index("dpoints")
        assert cargs == sargs[:k + 1] + ["float *dlod"] + sargs[k + 1:], name
        sres, sig = _lib.SIGNATURES[SIBLINGS[name]]
        assert sres is res and args == sig[:k + 1] + [ctypes.c_void_p] + sig[k + 1:]
    declared = set(re.findall(r"\b(nic_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", ext, flags=re.S)))
    assert declared == set(_lib.EXT_SIGNATURES) and len(_lib.SIGNATURES) == 86 and _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version()
    assert re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)
    for name in ("hash_encode_points_grad_lod", "hash_fused_points_grad_lod"):
        assert getattr(pkg, name) is getattr(hashgrid, name)
    comment = ext[ext.index("LEVEL OF DETAIL of a point"):ext.index(f"int {ENC}(")]
    for words in ("ON THE RAMP iff 0 < a_raw <= 1", "right-hand derivative", "exactly 0.0f", "lambda_raw == 0 passes", "a clamped axis does not zero dlod",
                  "WRITTEN (never added to)", "sum of dlod"):
        assert words in " ".join(comment.replace("*", " ").split()), words


def test_the_python_signatures():
    import inspect
    from neural_image_compression_v2_amd import hashgrid
    sig = inspect.signature(hashgrid.hash_encode_points_grad_lod).parameters
    assert list(sig) == ["geo", "data", "points", "dx", "kind", "num_bits", "lod", "lod_uniform", "fade"] == list(
        inspect.signature(hashgrid.hash_encode_points_grad).parameters)
    sig = inspect.signature(hashgrid.hash_fused_points_grad_lod).parameters
    assert list(sig) == ["geo", "data", "points", "params", "dy", "target", "loss_scale", "want_y", "kind", "num_bits", "lod", "lod_uniform", "fade"] == list(
        inspect.signature(hashgrid.hash_fused_points_grad).parameters)
    cls = hashgrid.HashGridField
    sig = inspect.signature(cls.point_gradient_lod).parameters
    assert list(sig) == ["self", "points", "lod", "dy", "target", "scale"] and [sig[k].default for k in list(sig)[3:]] == [None, None, 1.0]
    assert list(inspect.signature(cls.jacobian_lod).parameters) == ["self", "points", "lod"] == list(inspect.signature(cls.query_differentiable_lod).parameters)
    # the existing methods keep their parameter lists
    assert list(inspect.signature(cls.point_gradient).parameters) == ["self", "points", "dy", "target", "scale", "lod"]
    assert list(inspect.signature(cls.jacobian).parameters) == ["self", "points", "lod"] == list(inspect.signature(cls.query_differentiable).parameters)
    assert list(inspect.signature(cls.query).parameters) == ["self", "points", "lod", "precision"]


def test_layerwise_entry_argument_errors_in_the_documented_order(lib):
    d = _desc()
    assert _enc(lib, d) == OK                                             # every check passes; no points: no launch
    # 1. the descriptor of a point source, whatever else is wrong
    bad = _desc()
    bad.flags = 1
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(None, NULL), (bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (_desc(num_crops=2), SHAPE),
                       (big, ARG)]:
        assert _enc(lib, desc) == want and _enc(lib, desc, lodp=None, src=None, dlod=0, n_points=-1) == want
    # 2. null pointers: lodp and dlod with the siblings' (lod may be null) - before the source, the nic_hash_lod and n_points
    for kw in (dict(lodp=None), dict(src=None), dict(src=_src(data=0)), dict(points=0), dict(dx=0), dict(dpoints=0), dict(dlod=0)):
        assert _enc(lib, d, **kw) == NULL and _enc(lib, d, n_points=-1, **kw) == NULL, kw
        if "src" not in kw and "lodp" not in kw:
            assert _enc(lib, d, **dict(kw, src=_src(kind=7), lodp=_lod(reserved=1))) == NULL, kw
    assert _enc(lib, d, lod=16) == OK and _enc(lib, d, lod=0) == OK
    # 3. the source: kind, num_bits, alignment - before the nic_hash_lod
    for src in (_src(kind=7), _src(kind=0, bits=4), _src(kind=1, bits=0), _src(kind=1, bits=9), _src(kind=2, bits=4, data=18)):
        assert _enc(lib, d, src=src) == ARG and _enc(lib, d, src=src, lodp=_lod(reserved=1), n_points=-1) == ARG
    for src in (_src(kind=1, bits=8), _src(kind=2, bits=4)):
        assert _enc(lib, d, src=src) == OK
    # 4. the nic_hash_lod - before n_points
    for lp in _bad_lods():
        assert _enc(lib, d, lodp=lp) == ARG and _enc(lib, d, lodp=lp, lod=16, n_points=-1) == ARG
    assert _enc(lib, _desc(resolutions=(16,) * 4), lodp=_lod((0.0,) * 4 + (-1.0, float("nan")))) == OK        # fade past the levels is ignored
    # 5. n_points < 0; 6. n_points == 0 is NIC_OK without a launch (the pointers are fakes: a launch would fault)
    for n_points in (-1, -(1 << 40)):
        assert _enc(lib, d, n_points=n_points) == ARG
    for desc in (d, _desc(dim=3, resolutions=(4, 6, 9, 12), features=1, s_max=12, extent=(12, 10, 9)), _desc(features=8)):
        assert _enc(lib, desc) == OK and _enc(lib, desc, lod=16, lodp=_lod(uniform=1.5)) == OK


def test_fused_entry_argument_errors_in_the_documented_order(lib):
    d = _desc()
    assert _fus(lib, d) == OK
    # 1. null desc / mlp, whatever else is wrong
    assert _fus(lib, None) == NULL and _fus(lib, d, m=None) == NULL and _fus(lib, None, lodp=None, src=None, n_points=-1) == NULL
    # 2. the fused set, then the descriptor of a point source: before every pointer
    bad = _desc()
    bad.flags = 1
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(resolutions=(16,) * 9, features=8), UNSUP), (_desc(num_crops=2), SHAPE),
                       (big, ARG)]:
        assert _fus(lib, desc) == want and _fus(lib, desc, lodp=None, src=None, dpoints=0, dlod=0, n_points=-1) == want
    assert _fus(lib, d, m=_mlp(5, 5)) == UNSUP
    # 3. null pointers: lodp and dlod with the siblings', then the decoder's layers (lod, dy, target and y may be null)
    for kw in (dict(lodp=None), dict(src=None), dict(src=_src(data=0)), dict(points=0), dict(dpoints=0), dict(dlod=0), dict(m=_mlp(3, 2))):
        assert _fus(lib, d, **kw) == NULL and _fus(lib, d, n_points=-1, dy=0, **kw) == NULL, kw
        if "src" not in kw and "lodp" not in kw:
            assert _fus(lib, d, **dict(kw, src=_src(kind=7), lodp=_lod(reserved=1))) == NULL, kw
    assert _fus(lib, d, y=0, lod=16) == OK
    # 4. the source; 5. the nic_hash_lod; 6. exactly one of dy / target; 7. n_points < 0
    for src in (_src(kind=7), _src(kind=0, bits=4), _src(kind=1, bits=0), _src(kind=1, bits=9), _src(kind=2, bits=4, data=18)):
        assert _fus(lib, d, src=src) == ARG and _fus(lib, d, src=src, lodp=_lod(reserved=1), dy=0, n_points=-1) == ARG
    for lp in _bad_lods():
        assert _fus(lib, d, lodp=lp) == ARG and _fus(lib, d, lodp=lp, dy=0, n_points=-1) == ARG
    assert _fus(lib, d, dy=16, target=16) == ARG and _fus(lib, d, dy=0, target=0) == ARG and _fus(lib, d, dy=0, target=16) == OK
    assert _fus(lib, d, dy=16, target=16, n_points=-1) == ARG
    for n_points in (-1, -(1 << 40)):
        assert _fus(lib, d, n_points=n_points) == ARG
    # 8. n_points == 0 is NIC_OK without a launch
    for desc in (d, _desc(dim=3, resolutions=(4, 6, 9, 12), features=1, s_max=12, extent=(12, 10, 9)), _desc(features=8), _desc(resolutions=(16,) * 5, features=8)):
        assert _fus(lib, desc) == OK and _fus(lib, desc, dy=0, target=16, lod=16, src=_src(kind=2, bits=4)) == OK


# ------------------------------------------------------------------------------------------------------------------ the unit
def test_the_unit_and_its_header_are_in_the_build_and_restate_no_shared_helper():
    from neural_image_compression_v2_amd import _build
    import test_hashgrid_common_cpu as common
    assert UNIT in _build.SOURCES and WALK in _build.HEADERS and len(set(_build.SOURCES)) == len(_build.SOURCES)
    for f in (UNIT, WALK):
        assert f.startswith("hashgrid_") and not f.startswith(("hash_", "lod_"))
    unit, walk = (open(os.path.join(_build.CSRC, f)).read() for f in (UNIT, WALK))
    assert re.search(r'^\s*#include\s+"hash_common\.hpp"', walk, re.M) and re.search(r'^\s*#include\s+"hashgrid_pointgrad\.hpp"', unit, re.M)
    walk_helpers = ["decoder_dx_half", "point_grad", "point_walk", "point_walk_levels", "kept_axes", "store_point_grad", "lambda_passes"]
    for text in (unit, walk):
        for name in common.FUNCTIONS + list(common.OVERLOADS) + walk_helpers:
            # the walk header defines its own helpers once each; nothing else is restated anywhere
            assert sum(bool(common._function_re(name).match(ln)) for ln in text.splitlines()) == (1 if text is walk and name in walk_helpers else 0), name
        for name in common.STRUCTS:
            assert not any(common._struct_re(name).match(ln) for ln in text.splitlines()), name
        assert "atomic" not in text
    for call in ("hash_points_grad_lod_kernel<D, F, SRC>", "hash_points_fused_grad_lod_kernel<D, F, SRC, 2>", "hash_points_fused_grad_lod_kernel<D, F, SRC, 1>",
                 "p.d.levels * F > 32", "decoder_dx_half<KT>(", "encode_point<D, F, SRC, false, false, true>(p, t, 0, lam, xrow)", "point_walk<D, F, SRC, true, true, false>("):
        assert call in unit, call
    assert "accl = fmaf(pw, dot, accl)" in walk and "glam = __fsub_rn(glam, accl)" in walk


# ------------------------------------------------------------------------------------------------------------------ the reference
CASES = [(2, 1, 4), (2, 2, 4), (3, 4, 4), (3, 8, 4), (2, 8, 5), (3, 8, 5)]


def _loss_rows(inp, lam64):
    """the float64 loss sum_k dx[n, k] row[n, k] of every row at the float64 level of detail ``lam64`` [n] (its clamp to [0, 32] included)"""
    fade = np.asarray(inp.fade, dtype=np.float64)
    lam = np.clip(lam64, 0.0, 32.0)
    W = torch.from_numpy(np.clip((fade[None, :] - lam[:, None]) + 1.0, 0.0, 1.0))
    tab = T.as_f64(inp.table)
    row = T.encode(inp.tgeo, [tab[l] for l in range(inp.tgeo.levels)], T.rows(inp.tgeo, points=inp.points), None, W)
    return (row * T.as_f64(inp.dx)).sum(dim=1).detach().numpy()


@pytest.mark.parametrize("case", CASES, ids=str)
def test_the_reference_against_differences_of_its_own_loss(case):
    inp = inputs(*case)
    h = 2.0 ** -10
    for mode in MODES:
        lod, u = mode_lod(inp, mode)
        ref = reference(inp.tgeo, inp.table, inp.params, inp.points, inp.fade, lod, u, dx=inp.dx)
        with np.errstate(invalid="ignore"):
            raw = ((np.zeros(N, dtype=F32) if lod is None else lod) + F32(u)).astype(F32)
        lam = raw.astype(np.float64)
        # central differences at rows whose every a_raw is at least 2^-6 from 0 and 1, lambda itself that far inside [0, 32]
        away = (np.minimum(np.abs(ref.a_raw), np.abs(ref.a_raw - 1)) >= 2.0 ** -6).all(axis=1) & (raw >= 2.0 ** -6) & (raw <= 32 - 2.0 ** -6)
        on_ramp = away & ref.ramp.any(axis=1)
        assert mode == "uniform" or (on_ramp.sum() >= 20 and (away & ~ref.ramp.any(axis=1)).sum() >= 20), (mode, on_ramp.sum())
        if away.any():
            safe = np.where(away, lam, 1.0)
            cd = (_loss_rows(inp, safe + h) - _loss_rows(inp, safe - h)) / (2 * h)
            want = ref.dlod.numpy()
            err = np.abs(cd - want)[away].max() / max(np.abs(want).max(), 1e-300)
            print(f"{case} {mode}: central differences at {int(away.sum())} rows ({int(on_ramp.sum())} with a level on the ramp): {err:.3e}")
            assert err <= 1e-9, (mode, err)
        # one-sided differences from the right at rows exactly on a_raw == 1 or a_raw == 0 (and 0 <= lambda_raw < 32)
        kink = ((ref.a_raw == 1) | (ref.a_raw == 0)).any(axis=1) & ref.passes
        if mode == "point":
            assert kink[:2 * len(inp.fade)].all() and (ref.a_raw[:2 * len(inp.fade)] == 1).any(axis=1).sum() >= len(inp.fade)
        if mode == "uniform":
            assert kink.all()                                             # lambda = 1.0: a level exactly at its end on every row
        if kink.any():
            safe = np.where(kink, lam, 1.0)
            right = (_loss_rows(inp, safe + h) - _loss_rows(inp, safe)) / h
            err = np.abs(right - ref.dlod.numpy())[kink].max() / np.abs(ref.dlod.numpy()).max()
            print(f"{case} {mode}: differences from the right at {int(kink.sum())} rows on a kink: {err:.3e}")
            assert err <= 1e-9, (mode, err)
        # the exact zeros of the definition
        flat = ~ref.passes | ~ref.ramp.any(axis=1)
        assert bool((ref.dlod[torch.from_numpy(flat)] == 0).all()) and bool((ref.dlod[torch.from_numpy(~flat)] != 0).any())


@pytest.mark.parametrize("case", CASES, ids=str)
def test_the_inputs_hold_every_kind_of_row(case):
    inp = inputs(*case)
    lod, fade = inp.lod, inp.fade
    a_raw, ramp, passes = ramp_f32(fade, lod, 0.0, N)
    for l, f in enumerate(fade):
        assert a_raw[2 * l, l] == 1 and a_raw[2 * l + 1, l] == 0
    k = 2 * len(fade)
    assert list(lod[k:k + 4]) == [0.0, -1.0, 32.0, 40.0] and np.isnan(lod[k + 4]) and list(passes[k:k + 5]) == [True, False, False, False, False]
    assert ramp[k].any()                                                  # lambda_raw == 0 passes a gradient through
    assert (a_raw[64:128] <= 0).all() and not ramp[64:128].any()           # one whole wave with every level off
    live = a_raw[128:] > 0
    assert live.any(axis=0).any() and not live.any(axis=0).all()           # a wave where some level is live for no lane
    assert ramp[list(OUTSIDE_ROWS)].any(axis=1).all()
    moved = T.clamp_points(inp.tgeo, inp.points.numpy())[1]
    assert moved[list(OUTSIDE_ROWS)].any(axis=1).all() and moved[22].all() and moved.any(axis=1).sum() == len(OUTSIDE_ROWS)
    for n in (1, 63, 64, 65, 130):                                         # every launch length has a row with a gradient
        assert ramp[:n].any()
    for mode in MODES:
        l_m, u = mode_lod(inp, mode)
        for head in (dict(dx=inp.dx), dict(dy=inp.dy), dict(target=inp.target, loss_scale=TARGET_SCALE * N)):
            ref = reference(inp.tgeo, inp.table, inp.params, inp.points, fade, l_m, u, **head)
            assert float(ref.dlod.abs().max()) >= 1e-2 and float(ref.dpoints.abs().max()) >= 1e-2, (mode, list(head))
            assert bool(torch.isfinite(ref.dlod).all())
            assert mode != "point" or bool((ref.dlod[list(OUTSIDE_ROWS)] != 0).all())


# ------------------------------------------------------------------------------------------------------------------ teeth
def _mistakes(ref):
    left = (ref.a_raw >= 0) & (ref.a_raw < 1)
    keep = torch.from_numpy(ref.passes)
    return {"the left-hand convention": -(ref.dW * torch.from_numpy(left)).sum(dim=1) * keep,
            "a sign flip": -ref.dlod,
            "r taken weighed": -(ref.dW * ref.W * torch.from_numpy(ref.ramp)).sum(dim=1) * keep}


@pytest.mark.parametrize("case", CASES, ids=str)
def test_teeth_three_mistakes_are_each_seen_on_the_gpu_tests_inputs(case):
    inp = inputs(*case)
    for mode in MODES:
        lod, u = mode_lod(inp, mode)
        for head in (dict(dx=inp.dx), dict(dy=inp.dy), dict(target=inp.target, loss_scale=TARGET_SCALE * N)):
            ref = reference(inp.tgeo, inp.table, inp.params, inp.points, inp.fade, lod, u, **head)
            for name, bad in _mistakes(ref).items():
                moved = rel(bad, ref.dlod) / TOL_G
                assert moved > 1000, (mode, list(head), name, moved)


# ------------------------------------------------------------------------------------------------------------------ what the GPU file asks of the definition
@pytest.mark.parametrize("dim", [2, 3])
def test_the_central_differences_of_the_gpu_file_hold_on_the_reference(dim):
    """(y(lambda + 1/8) - y(lambda - 1/8)) . dy / (1/4) on the rows ``affine_rows`` keeps, through the GENTLE decoder: at most half of the rows are
    left out, and the float64 reference meets the GPU test's bound with a factor 3 to spare.  What is left is the decoder's curvature, h^2 / 6 x
    the third derivative; a stronger decoder has more of it, a weaker one moves y too little for fp32 outputs (an error of 2^-23 in y is 2^-20 in
    the difference quotient, 1e-4 of 1e-2): the third of the bound the reference uses leaves the other two to that rounding"""
    inp = inputs(dim, 2)
    lod = affine_lod()
    keep = affine_rows(inp.fade, lod)
    assert keep.sum() >= N / 2, keep.sum()
    params = decoder_params(inp.geo.width, 3, **GENTLE)
    ref = reference(inp.tgeo, inp.table, params, inp.points, inp.fade, lod, 0.0, dy=inp.dy)
    up = reference(inp.tgeo, inp.table, params, inp.points, inp.fade, lod + F32(H_GPU), 0.0, dy=inp.dy).y
    down = reference(inp.tgeo, inp.table, params, inp.points, inp.fade, lod - F32(H_GPU), 0.0, dy=inp.dy).y
    cd = ((up - down) * T.as_f64(inp.dy)).sum(dim=1) / (2 * H_GPU)
    k = torch.from_numpy(keep)
    err = float((cd - ref.dlod)[k].abs().max() / ref.dlod[k].abs().max())
    print(f"{dim}D: {int(keep.sum())} of {N} rows kept; the reference against its own central differences {err:.3e} of {float(ref.dlod[k].abs().max()):.3e}")
    assert err < TOL_G / 3 and float(ref.dlod[k].abs().max()) > 1.5e-2
    assert bool((ref.dlod[k] != 0).sum() >= 20)


def test_descent_on_the_reference_recovers_lambda():
    """the float64 reference's run of the GPU file's loop: |lambda_hat - lambda0| at most a tenth of the initial 0.75, with a factor 4 to spare"""
    geo, tgeo, table, params, points = descent_inputs()
    fade = T.default_fade(tgeo)
    assert fade == (4.0, 3.0, 2.0, 1.0)
    first, last, lam = run_descent(lambda p, l: ReferenceQuery.apply(l, tgeo, table, params, p, fade), points, torch.device("cpu"))
    err = abs(lam - DESCENT["lam0"])
    print(f"descent on the reference: loss {first:.4e} -> {last:.4e}, lambda_hat {lam:.5f}, error {err:.5f}")
    assert DESCENT["steps"] <= 300 and err <= 0.075 / 4, (first, last, lam)
