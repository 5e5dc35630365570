"""CPU-only tests of the gradient with respect to the level of detail from the TRAINING STEP (run with -m "not gpu"):
nic_hash_fused_forward_backward_points_grad_lod and nic_hash_encode_points_grad_lod_noisy are exported, declared in the companion header
include/nicv2_hip_ext.h alone and mirrored in _lib.EXT_SIGNATURES with their argument lists held to the siblings' (dlod after dpoints; quant
after lodp); the ABI version stays 9 and the main header's 86 entries stay; the Python signatures are the documented ones and the existing ones
are as they were; every argument error is decided on the host in the documented order (fake pointers and refusals only, n_points == 0 for the
NIC_OK cases: nothing launches).

The float64 reference ``reference_step`` is built from oracle/hashgrid_train_ref.py's own pieces - ``rows``, ``level_weights`` as a leaf W,
``noise``, ``encode(geo, tables, pos, nz, W)``, ``decoder``, ``mse`` - through ONE ``torch.autograd.grad`` call that yields dW, dpoints, the
per-level table gradients and the decoder gradients; dlod = -(dW . ramp).sum(1) . passes with ``ramp_f32`` of tests/test_hashgrid_lodgrad_cpu.py.
In ``encode`` the noise is added before the weight, so dW[n, l] = sum_f g[n, l F + f] (r[n, l, f] + nz[n, l F + f]): the definition of the
header, with no formula restated.  It equals ``T.step(.., noise_key=, lod=)`` in y, loss, table and decoder gradients and dpoints to 1e-12, and is
held to differences of its own float64 loss in lambda with the noise held fixed (4.7.22's recipe: central, h = 2^-10, at rows at least 2^-6 from
every kink; from the right exactly on a_raw == 1 / a_raw == 0; loss sum(dx . row); bound 1e-9).

Teeth, on the inputs tests/test_gpu_hashgrid_lodtrain.py uses: the noise left out of r, noise keyed by the walk position under a non-identity
order, noise keyed without sample_base and a flipped sign each move dlod by more than 100 x TOL_G at num_bits = 4 on every case and mode.

``reference_step``, ``NOISE_KEYS`` and the joint loop are shared with the GPU file: both sides see the same bytes."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import hashgrid_train_ref as T
from tests.test_hashgrid_batch_points_cpu import ARG, NULL, OK, SHAPE, UNSUP, WORKSPACE, HEADER, EXT_HEADER, _desc, _mlp, _ref, lib  # noqa: F401
from tests.test_hashgrid_batch_lod_cpu import _bad_lods, _lod
from tests.test_hashgrid_lodgrad_cpu import CASES, F32, MODES, N, TARGET_SCALE, TOL_G, inputs, mode_lod, ramp_f32, rel
from tests.test_hashgrid_pointtrain_cpu import _grads

FUSED, ENC = "nic_hash_fused_forward_backward_points_grad_lod", "nic_hash_encode_points_grad_lod_noisy"
ARGS = {FUSED: ["desc", "lodp", "quant", "table", "points", "lod", "n_points", "order", "mlp", "target", "loss_scale", "table_grad", "mlp_grads", "loss", "y",
                "dpoints", "dlod", "flags", "workspace", "workspace_bytes", "tail", "stream"],
        ENC: ["desc", "lodp", "quant", "table", "points", "lod", "n_points", "dx", "dpoints", "dlod", "stream"]}
PTR = ctypes.c_void_p
UNIT, WALK = "hashgrid_lodtrain.hip", "hashgrid_pointgrad.hpp"

# ------------------------------------------------------------------------------------------------------------------ shared with the GPU file
# (bits, seed, offset, sample_base): sample_base != 0, a seed and an offset with both 32-bit halves in use
NOISE_KEYS = {4: (4, 0x1234567_89ABCDEF, (3 << 32) + 17, 1000), 8: (8, 0x0FEDCBA9_87654321, 5, 77), 2: (2, 99, 1, 5)}


def reference_step(tgeo, table, params, points, fade, lod, lod_uniform, target=None, loss_scale=1.0, noise_key=None, nz=None, dx=None):
    """float64, from the oracle's own pieces through one ``torch.autograd.grad`` call.  The loss is mean((y - target)^2) * loss_scale (the step),
    or sum(dx * row) (the layer-wise entry) - exactly one.  ``noise_key``: None or (bits, seed, offset, sample_base); ``nz`` [N, L F] overrides the
    values (the teeth).  Returns y, loss, row, dlod, dpoints, table_grad (per level), decoder_grads, and what the teeth need: dW, drow (d loss / d
    row, the gradient of the weighed column), nz, ramp, passes, a_raw"""
    assert (target is None) != (dx is None)
    tab = T.as_f64(table)
    tables = [tab[l].clone().requires_grad_(True) for l in range(tgeo.levels)]
    ps = [T.as_f64(p).clone().requires_grad_(True) for p in params]
    n = points.shape[0]
    lod = None if lod is None else np.asarray(lod, dtype=F32)
    with torch.enable_grad():
        pos = T.rows(tgeo, points=points)
        W = torch.from_numpy(T.level_weights(tgeo, n, fade, lod, lod_uniform)).requires_grad_(True)
        if nz is None and noise_key is not None:
            nz = torch.from_numpy(T.noise(n, tgeo.width, *noise_key))
        row = T.encode(tgeo, tables, pos, nz, W)
        y = T.decoder(row, ps)
        loss = (row * T.as_f64(dx)).sum() if dx is not None else T.mse(y, T.as_f64(target)) * float(loss_scale)
        leaves = [W, pos.points, row] + tables + ps
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]
    dW, dp, drow = grads[:3]
    a_raw, ramp, passes = ramp_f32(fade, lod, lod_uniform, n)
    dlod = -(dW * torch.from_numpy(ramp)).sum(dim=1) * torch.from_numpy(passes)
    return types.SimpleNamespace(y=y.detach(), loss=loss.detach(), row=row.detach(), dlod=dlod, dpoints=dp, table_grad=grads[3:3 + tgeo.levels],
                                 decoder_grads=grads[3 + tgeo.levels:], dW=dW, drow=drow, nz=nz, ramp=ramp, passes=passes, a_raw=a_raw)


def noise_term(tgeo, drow, nz):
    """[N, L]: sum_f drow[n, l F + f] nz[n, l F + f] - the part of dW that comes from the noise"""
    return (drow * nz).reshape(drow.shape[0], tgeo.levels, tgeo.features).sum(dim=2)


def orders(n):
    """the non-identity orders of the GPU file as int64 CPU tensors: reversed, and a fixed permutation"""
    return {"reversed": torch.arange(n - 1, -1, -1), "perm": torch.randperm(n, generator=torch.Generator().manual_seed(29))}


# ---- the joint loop of the GPU file (its test 7b): the field steps inside the call, one torch Adam steps a 0-dim lambda and a shift of the points
JOINT = dict(steps=20, lam_start=2.0, lam_true=1.25, lr=0.02, shift_true=(0.75, -0.5), table_lr=0.01, decoder_lr=0.005)


def joint_colours(tgeo, table, params, points, fade):
    """the colours the joint loop fits, as fp32: the float64 reference's query of the starting field at points + shift_true, lambda_true"""
    p = (points + torch.tensor(JOINT["shift_true"])).contiguous()
    return reference_step(tgeo, table, params, p, fade, None, JOINT["lam_true"], target=torch.zeros(p.shape[0], 3)).y.float()


def run_joint(step, points, colours, device):
    """the loop the field and the reference both run: ``step(points, lam, colours)`` trains the field by one step and returns its loss as a
    differentiable op of the points and of the 0-dim lambda; one torch Adam steps lambda from ``lam_start`` and a 2-vector shift of the points
    from 0.  Returns the trajectories (lambda [steps], shift [steps, 2], loss [steps]) as float64 CPU tensors"""
    lam = torch.tensor(JOINT["lam_start"], dtype=torch.float32, device=device, requires_grad=True)
    shift = torch.zeros(2, dtype=torch.float32, device=device, requires_grad=True)
    opt = torch.optim.Adam([lam, shift], lr=JOINT["lr"])
    lams, shifts, losses = [], [], []
    for _ in range(JOINT["steps"]):
        opt.zero_grad()
        loss = step(points + shift, lam, colours)
        loss.sum().backward()
        opt.step()
        lams.append(lam.detach().double().cpu().clone())
        shifts.append(shift.detach().double().cpu().clone())
        losses.append(loss.detach().double().cpu().reshape(()).clone())
    return torch.stack(lams), torch.stack(shifts), torch.stack(losses)


class ReferenceJoint:
    """the float64 reference's side of ``run_joint``: the step of ``reference_step`` at the fp32 points and lambda it is handed, the field's
    update held to ``T.adam_step`` (table lr 0.01, decoder lr 0.005, no clamp: the field has no codec), the state kept in float64"""

    def __init__(self, tgeo, table, params, fade):
        self.tgeo, self.fade, self.count = tgeo, fade, 0
        self.state = [[T.as_f64(torch.stack([table[l] for l in range(tgeo.levels)])), None, None, JOINT["table_lr"]]]
        self.state += [[T.as_f64(p), None, None, JOINT["decoder_lr"]] for p in params]
        for s in self.state:
            s[1], s[2] = torch.zeros_like(s[0]), torch.zeros_like(s[0])

    def step(self, points, lam, colours):
        ref_self = self

        class Step(torch.autograd.Function):
            @staticmethod
            def forward(ctx, pts, lam_):
                ref = reference_step(ref_self.tgeo, ref_self.state[0][0], [s[0] for s in ref_self.state[1:]], pts.detach().float().contiguous(), ref_self.fade,
                                     None, float(F32(float(lam_))), target=colours)
                ctx.save_for_backward(ref.dpoints, ref.dlod.sum())
                ref_self.count += 1
                grads = [torch.stack(list(ref.table_grad))] + list(ref.decoder_grads)
                for s, g in zip(ref_self.state, grads):
                    s[0], s[1], s[2] = T.adam_step(s[0], g, s[1], s[2], ref_self.count, s[3])
                return ref.loss.to(pts.dtype)

            @staticmethod
            def backward(ctx, g):
                dp, dl = ctx.saved_tensors
                return (g * dp).to(g.dtype), (g * dl).to(g.dtype)
        return Step.apply(points, lam)


# ------------------------------------------------------------------------------------------------------------------ the C entries
def _quant(bits=8, mode=2, seed=1, offset=2, base=0):
    from neural_image_compression_v2_amd._lib import NicHashQuant
    return NicHashQuant(bits, mode, seed, offset, base)


def _fus(lib, d, lodp="default", q=None, table=16, pts=16, lod=0, n=0, order=0, m="default", target=16, tg=16, gs="default", loss=16, y=0, dpoints=16,
         dlod=16, flags=0, ws=16, ws_bytes=1 << 30, tail=None):
    """the return code of the fused entry.  Every pointer is a dummy that is never dereferenced: n_points <= 0 only, so nothing launches"""
    lodp = _lod() if lodp == "default" else lodp
    m = _mlp() if m == "default" else m
    gs = _grads() if gs == "default" else gs
    assert n <= 0 or order
    return getattr(lib, FUSED)(_ref(d), _ref(lodp), _ref(q), PTR(table), PTR(pts), PTR(lod), n, PTR(order), _ref(m), PTR(target), 1.0, PTR(tg), _ref(gs),
                               PTR(loss), PTR(y), PTR(dpoints), PTR(dlod), flags, PTR(ws), ws_bytes, _ref(tail), None)


def _enc(lib, d, lodp="default", q=None, table=16, pts=16, lod=0, n=0, dx=16, dpoints=16, dlod=16):
    lodp = _lod() if lodp == "default" else lodp
    assert n <= 0
    return getattr(lib, ENC)(_ref(d), _ref(lodp), _ref(q), PTR(table), PTR(pts), PTR(lod), n, PTR(dx), PTR(dpoints), PTR(dlod), None)


def _c_args(text, name):
    m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_entries_are_exported_declared_in_the_companion_header_only_and_mirrored(lib):
    from neural_image_compression_v2_amd import _lib, hashgrid
    import neural_image_compression_v2_amd as pkg
    header, ext = open(HEADER).read(), open(EXT_HEADER).read()
    types_of = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    structs = {"nic_hash_desc": _lib.NicHashDesc, "nic_hash_lod": _lib.NicHashLod, "nic_hash_quant": _lib.NicHashQuant, "nic_mlp": _lib.NicMlp,
               "nic_mlp_grads": _lib.NicMlpGrads, "nic_step_tail": _lib.NicStepTail}
    for name, names in ARGS.items():
        assert hasattr(lib, name)
        assert name not in header and name not in _lib.SIGNATURES and name in _lib.EXT_SIGNATURES
        res, args = _lib.EXT_SIGNATURES[name]
        cargs = _c_args(ext, name)
        assert len(cargs) == len(args) == len(names), (name, cargs)
        assert res is ctypes.c_int
        for c, a in zip(cargs, args):
            if "*" in c:
                base = c.replace("const", "").split("*")[0].strip()
                want = ctypes.POINTER(structs[base]) if base in structs else ctypes.c_void_p
                assert a is want or a == want, (name, c, a)
            else:
                assert a is types_of[c.split()[0]], (name, c)
        assert [c.split()[-1].lstrip("*") for c in cargs] == names
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # the fused entry: the sibling of the main header argument for argument, with dlod after dpoints
    sargs = _c_args(header, "nic_hash_fused_forward_backward_points_grad")
    k = [c.split()[-1].lstrip("*") for c in sargs].index("dpoints")
    assert _c_args(ext, FUSED) == sargs[:k + 1] + ["float *dlod"] + sargs[k + 1:]
    sres, sig = _lib.SIGNATURES["nic_hash_fused_forward_backward_points_grad"]
    assert sres is ctypes.c_int and _lib.EXT_SIGNATURES[FUSED][1] == sig[:k + 1] + [ctypes.c_void_p] + sig[k + 1:]
    # the layer-wise entry: nic_hash_encode_points_grad_lod with quant after lodp and the fp32 table in the place of the source
    sargs = _c_args(ext, "nic_hash_encode_points_grad_lod")
    assert sargs[2] == "const nic_hash_source *src"
    assert _c_args(ext, ENC) == sargs[:2] + ["const nic_hash_quant *quant", "const float *table"] + sargs[3:]
    sig = _lib.EXT_SIGNATURES["nic_hash_encode_points_grad_lod"][1]
    assert _lib.EXT_SIGNATURES[ENC][1] == sig[:2] + [ctypes.POINTER(_lib.NicHashQuant), ctypes.c_void_p] + sig[3:]
    declared = set(re.findall(r"\b(nic_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", ext, flags=re.S)))
    assert declared == set(_lib.EXT_SIGNATURES) and len(_lib.SIGNATURES) == 86 and _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version()
    assert re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)
    for name in ("hash_fused_forward_backward_points_grad_lod", "hash_encode_points_grad_lod_noisy"):
        assert getattr(pkg, name) is getattr(hashgrid, name)
    comment = " ".join(ext[ext.index("from the TRAINING STEP"):ext.index(f"int {ENC}(")].replace("*", " ").split())
    for words in ("a_l (r[n, l, f] + nz[n, l F + f])", "the slope on the ramp is -(r + nz), not -r", "CALLER'S ROW", "the same generator block",
                  "right-hand derivative", "exactly 0.0f", "a clamped axis zeroes its dpoints and not dlod", "WRITTEN once by its lane",
                  "whatever NIC_HASH_FUSED_ADD_GRADS says", "n_points == 0 touches nothing", "table_grad == NULL (a frozen table) still produces dpoints, dlod",
                  "bit for bit"):
        assert words in comment, words


def test_the_python_signatures():
    from neural_image_compression_v2_amd import hashgrid
    sib = list(inspect.signature(hashgrid.hash_fused_forward_backward_points_grad).parameters)
    assert sib[-1] == "dpoints"
    assert list(inspect.signature(hashgrid.hash_fused_forward_backward_points_grad_lod).parameters) == sib + ["dlod"]
    sig = inspect.signature(hashgrid.hash_encode_points_grad_lod_noisy).parameters
    assert list(sig) == ["geo", "table", "points", "dx", "lod", "lod_uniform", "fade", "quant"] and sig["quant"].default is None
    cls = hashgrid.HashGridField
    sig = inspect.signature(cls.train_points_grad_lod).parameters
    assert list(sig) == ["self", "points", "target", "lod", "dpoints", "dlod", "accumulate", "scale", "step", "noise", "order", "fused"]
    assert [sig[k].default for k in list(sig)[4:]] == [None, None, False, 1.0, True, None, None, False]
    assert sig["lod"].default is inspect.Parameter.empty
    sig = inspect.signature(cls.train_points_differentiable_lod).parameters
    assert list(sig) == ["self", "points", "lod", "target", "kwargs"] and sig["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    # the existing ones are as they were
    tp = inspect.signature(cls.train_points).parameters
    assert list(tp) == ["self", "points", "target", "accumulate", "scale", "step", "noise", "order", "fused", "lod", "dpoints"]
    assert [tp[k].default for k in list(tp)[3:]] == [False, 1.0, True, None, None, False, None, None]
    assert list(inspect.signature(cls.train_points_differentiable).parameters) == ["self", "points", "target", "kwargs"]
    assert list(inspect.signature(cls.fit_points).parameters) == ["self", "points", "target", "epochs", "batch", "order", "fused", "freeze_at", "lod"]
    assert list(inspect.signature(cls.fit_mips).parameters) == ["self", "target", "epochs", "mips", "batch", "order", "fused", "freeze_at"]
    assert list(inspect.signature(hashgrid.hash_encode_points_grad_lod).parameters) == ["geo", "data", "points", "dx", "kind", "num_bits", "lod", "lod_uniform",
                                                                                        "fade"]


def test_fused_entry_argument_errors_in_the_documented_order(lib):
    from neural_image_compression_v2_amd import _lib
    d = _desc(resolutions=(16, 64))
    for kw in (dict(), dict(lod=16), dict(tg=0), dict(y=16), dict(order=16), dict(flags=3), dict(q=_quant())):
        assert _fus(lib, d, **kw) == OK, kw                                    # n_points == 0: NIC_OK, nothing written
    # 1. null desc / mlp
    assert _fus(lib, None) == NULL and _fus(lib, d, m=None) == NULL and _fus(lib, None, lodp=None, pts=0, dlod=0, n=-1, ws_bytes=16) == NULL
    # 2. the fused set, then the descriptor of a point source: before every pointer - the sibling's codes
    bad = _desc()
    bad.flags = 1
    wide = _desc(resolutions=(16,) * 9, features=8)
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (wide, UNSUP), (_desc(num_crops=2), SHAPE),
                       (big, ARG)]:
        assert _fus(lib, desc) == want and _fus(lib, desc, lodp=None, table=0, dpoints=0, dlod=0, flags=4, n=-1, ws_bytes=16) == want
        sib = lib.nic_hash_fused_forward_backward_points_grad(_ref(desc), _ref(_lod()), None, PTR(16), PTR(16), None, 0, None, _ref(_mlp()), PTR(16), 1.0,
                                                              PTR(16), _ref(_grads()), PTR(16), None, PTR(16), 0, PTR(16), 1 << 30, None, None)
        assert sib == want
    assert _fus(lib, d, m=_mlp(5, 5)) == UNSUP
    # 3. null pointers, lodp and dlod among them: before flags, the nic_hash_lod, quant, n_points, the workspace and the tail
    for kw in (dict(lodp=None), dict(table=0), dict(pts=0), dict(target=0), dict(loss=0), dict(dpoints=0), dict(dlod=0), dict(ws=0), dict(gs=None),
               dict(m=_mlp(3, 2))):
        assert _fus(lib, d, **kw) == NULL, kw
        extra = {} if "lodp" in kw else dict(lodp=_lod(reserved=1))
        assert _fus(lib, d, flags=4, q=_quant(bits=0), n=-1, ws_bytes=16, **extra, **kw) == NULL, kw
    # 4. flags: before the nic_hash_lod
    assert _fus(lib, d, flags=4) == ARG and _fus(lib, d, flags=-1) == ARG and _fus(lib, d, flags=4, lodp=_lod(reserved=1), n=-1, ws_bytes=16) == ARG
    # 5. the nic_hash_lod: before quant (whose NIC_E_UNSUPPORTED tells the two apart)
    tensor_noise = _quant(mode=1)
    assert _fus(lib, d, q=tensor_noise) == UNSUP
    for lp in _bad_lods():                                                     # eight levels: every fade of the list is inside
        assert _fus(lib, _desc(), lodp=lp) == ARG and _fus(lib, _desc(), lodp=lp, q=tensor_noise, n=-1, ws_bytes=16) == ARG
    assert _fus(lib, d, lodp=_lod((1.0, 1.0, -1.0, float("nan")))) == OK       # fade entries past desc->levels are ignored
    # 6. quant: before n_points
    for q in (_quant(bits=0), _quant(bits=9), _quant(base=-1), _quant(mode=7)):
        assert _fus(lib, d, q=q) == ARG
    assert _fus(lib, d, q=tensor_noise, n=-1, ws_bytes=16) == UNSUP and _fus(lib, d, q=_quant(mode=0, bits=8)) == OK
    # 7. n_points: before the workspace
    assert _fus(lib, d, n=-1) == ARG and _fus(lib, d, n=-(1 << 40)) == ARG and _fus(lib, d, n=1 << 31, order=16) == ARG and _fus(lib, d, n=-1, ws_bytes=16) == ARG
    # 8. the workspace: nic_hash_fused_points_workspace_bytes, whatever n_points is; before the tail
    need = lib.nic_hash_fused_points_workspace_bytes(ctypes.byref(d), ctypes.byref(_mlp()))
    assert need > 16 and _fus(lib, d, ws_bytes=need) == OK and _fus(lib, d, ws_bytes=need - 1) == WORKSPACE and _fus(lib, d, ws_bytes=16) == WORKSPACE
    # 9. the tail: its decoder entries must carry this call's gradient buffers
    gs = _grads()

    def tail_of(grad, count=1, n_stream=0):
        arr = (_lib.NicAdamTensor * 1)(_lib.NicAdamTensor(0x2000, grad, 0x3000, 0x4000, 64, 1, 0.005, 1.0, -1.0, 0, 0, 0))
        t = _lib.NicStepTail()
        t.tensors = ctypes.cast(arr, ctypes.c_void_p).value
        t.count, t.n_stream, t.beta1, t.beta2, t.eps = count, n_stream, 0.9, 0.999, 1e-8
        t._keep = arr
        return t

    assert _fus(lib, d, gs=gs, tail=tail_of(gs.w[0])) == OK and _fus(lib, d, gs=gs, tail=tail_of(0x7000)) == ARG
    assert _fus(lib, d, gs=gs, tail=tail_of(gs.w[0], count=0)) == ARG and _fus(lib, d, gs=gs, tail=tail_of(0x7000), ws_bytes=16) == WORKSPACE
    # 10. n_points == 0 is NIC_OK for every shape of the fused set
    for desc in (_desc(dim=3, resolutions=(4, 6, 9, 12), features=1, s_max=12, extent=(12, 10, 9)), _desc(features=8, resolutions=(16,) * 4),
                 _desc(resolutions=(16,) * 5, features=8)):
        assert _fus(lib, desc) == OK and _fus(lib, desc, q=_quant(bits=4, base=9), lod=16, order=16) == OK


def test_layerwise_entry_argument_errors_in_the_documented_order(lib):
    d = _desc()
    assert _enc(lib, d) == OK and _enc(lib, d, lod=16, q=_quant()) == OK
    # 1. the descriptor of a point source, whatever else is wrong
    bad = _desc()
    bad.flags = 1
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(None, NULL), (bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (_desc(num_crops=2), SHAPE),
                       (big, ARG)]:
        assert _enc(lib, desc) == want and _enc(lib, desc, lodp=None, table=0, dlod=0, n=-1) == want
    # 2. null pointers (quant and lod may be null): before the nic_hash_lod, quant and n_points
    for kw in (dict(lodp=None), dict(table=0), dict(pts=0), dict(dx=0), dict(dpoints=0), dict(dlod=0)):
        assert _enc(lib, d, **kw) == NULL and _enc(lib, d, n=-1, q=_quant(bits=0), **kw) == NULL, kw
        if "lodp" not in kw:
            assert _enc(lib, d, **dict(kw, lodp=_lod(reserved=1))) == NULL, kw
    # 3. the nic_hash_lod: before quant
    for lp in _bad_lods():
        assert _enc(lib, d, lodp=lp) == ARG and _enc(lib, d, lodp=lp, q=_quant(mode=1), n=-1) == ARG
    # 4. quant, as the training entries check it: before n_points
    assert _enc(lib, d, q=_quant(mode=1)) == UNSUP and _enc(lib, d, q=_quant(mode=1), n=-1) == UNSUP
    for q in (_quant(bits=0), _quant(bits=9), _quant(base=-1), _quant(mode=7)):
        assert _enc(lib, d, q=q) == ARG and _enc(lib, d, q=q, n=-1) == ARG
    assert _enc(lib, d, q=_quant(mode=0)) == OK
    # 5. n_points < 0; 6. n_points == 0 is NIC_OK without a launch
    for n in (-1, -(1 << 40)):
        assert _enc(lib, d, n=n) == ARG
    for desc in (_desc(dim=3, resolutions=(4, 6, 9, 12), features=1, s_max=12, extent=(12, 10, 9)), _desc(features=8), _desc(features=4)):
        assert _enc(lib, desc) == OK and _enc(lib, desc, q=_quant(bits=4, base=3), lod=16) == OK


# ------------------------------------------------------------------------------------------------------------------ the unit
def test_the_unit_and_its_header_are_in_the_build_and_restate_no_shared_helper():
    from neural_image_compression_v2_amd import _build
    import test_hashgrid_common_cpu as common
    assert UNIT in _build.SOURCES and WALK in _build.HEADERS and len(set(_build.SOURCES)) == len(_build.SOURCES)
    for f in (UNIT, WALK):
        assert f.startswith("hashgrid_") and not f.startswith("hash_") and f not in common.UNITS
    unit, walk = (open(os.path.join(_build.CSRC, f)).read() for f in (UNIT, WALK))
    assert re.search(r'^\s*#include\s+"hash_common\.hpp"', walk, re.M) and re.search(r'^\s*#include\s+"hashgrid_pointgrad\.hpp"', unit, re.M)
    shared = common.FUNCTIONS + list(common.OVERLOADS) + ["load_decoder", "decoder_train_half", "write_record", "persistent_grid", "strided_grid", "point_grad",
                                                          "point_walk", "point_walk_levels", "kept_axes", "store_point_grad", "lambda_passes", "noise_block",
                                                          "noise_from_block"]
    own = ["point_grad", "point_walk", "point_walk_levels", "kept_axes", "store_point_grad", "lambda_passes"]      # the walk header's: once each
    for text in (unit, walk):
        for name in shared:
            assert sum(bool(common._function_re(name).match(ln)) for ln in text.splitlines()) == (1 if text is walk and name in own else 0), name
        for name in common.STRUCTS + ["DecoderSmem", "TrainSmem", "TrainAcc"]:
            assert not any(common._struct_re(name).match(ln) for ln in text.splitlines()), name
        assert "atomicAdd" not in text                                         # the only atomics are scatter_point's, in the shared header
    for piece in ("hash_points_lod_train_kernel<D, F, 2, NOISE>", "hash_points_lod_train_kernel<D, F, 1, NOISE>", "hash_points_grad_lod_noisy_kernel<D, F, NOISE>",
                  "p.d.levels * F > 32", "load_decoder(", "encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, true>(s, t, row, lam, xrow)",
                  "decoder_train_half<KT>(", "scatter_point<D, F, true>(", "write_record<KT>(", "xcd_range(", "ordered_row(", "point_lambda(",
                  "store_point_grad<D>(p.dpoints, row,", "kept_axes<D>(", "open_fused_points(", "fill_fused_points(", "points_fused_step(", "p.dlod[row] = lambda_passes(",
                  "point_walk<D, F, NIC_HASH_SRC_F32, true, true, NOISE>(s, t, row, lam, grow, gp, gl)"):
        assert piece in unit, piece
    assert "check_fused_tail(" not in unit and "finish_fused_step(" not in unit      # the host path of the step is hash_common.hpp's
    # the walk regenerates the noise with the forward's key and subtracts it with the blend; without noise it is 4.7.22's walk itself: one body
    for piece in ("noise_block(s.noise, s.sample_base + (uint64_t)n, nblk_id)", "noise_from_block(s.noise, nblk, (c0 + f) & 15)",
                  "glam = __fsub_rn(glam, __fadd_rn(accl, nd))", "glam = __fsub_rn(glam, accl)", "if constexpr (NOISE) {"):
        assert piece in walk, piece


# ------------------------------------------------------------------------------------------------------------------ the reference
def _step_inputs(inp, mode, n=N):
    lod, u = mode_lod(inp, mode, n)
    return lod, u, dict(target=inp.target[:n], loss_scale=TARGET_SCALE * n)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_the_reference_is_the_oracles_step(case):
    """y, loss, table and decoder gradients and dpoints of ``reference_step`` equal ``T.step(.., noise_key=, lod=)``'s to 1e-12 of the largest
    magnitude, with and without noise: the leaf W changes nothing of the step"""
    inp = inputs(*case)
    for mode in MODES:
        lod, u, head = _step_inputs(inp, mode)
        for key in (None, NOISE_KEYS[4]):
            ref = reference_step(inp.tgeo, inp.table, inp.params, inp.points, inp.fade, lod, u, noise_key=key, **head)
            st = T.step(inp.tgeo, inp.table, inp.params, inp.target, points=inp.points, loss_scale=head["loss_scale"], noise_key=key, lod=(inp.fade, lod, u))
            pairs = [(ref.y, st.y), (ref.loss, st.loss), (ref.dpoints, st.dpoints), (ref.row, st.row)]
            pairs += list(zip(ref.table_grad, st.table_grad)) + list(zip(ref.decoder_grads, st.decoder_grads))
            for a, b in pairs:
                assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300), (mode, key)
            assert float(ref.dlod.abs().max()) > 1e-2 and bool(torch.isfinite(ref.dlod).all())
            # dW is sum_f g (r + nz): taking the noise term out leaves the noiseless blend's share
            if key is not None:
                assert float(noise_term(inp.tgeo, ref.drow, ref.nz).abs().max()) > 0


def _loss_rows(inp, lam64, nz):
    """the float64 loss sum_k dx[n, k] row[n, k] of every row at the float64 level of detail ``lam64`` [n] (its clamp to [0, 32] included), the
    noise ``nz`` held fixed"""
    fade = np.asarray(inp.fade, dtype=np.float64)
    lam = np.clip(lam64, 0.0, 32.0)
    W = torch.from_numpy(np.clip((fade[None, :] - lam[:, None]) + 1.0, 0.0, 1.0))
    tab = T.as_f64(inp.table)
    row = T.encode(inp.tgeo, [tab[l] for l in range(inp.tgeo.levels)], T.rows(inp.tgeo, points=inp.points), nz, W)
    return (row * T.as_f64(inp.dx)).sum(dim=1).detach().numpy()


@pytest.mark.parametrize("case", CASES, ids=str)
def test_the_reference_against_differences_of_its_own_loss_with_the_noise_held_fixed(case):
    inp = inputs(*case)
    h = 2.0 ** -10
    nz = torch.from_numpy(T.noise(N, inp.tgeo.width, *NOISE_KEYS[4]))
    for mode in MODES:
        lod, u = mode_lod(inp, mode)
        ref = reference_step(inp.tgeo, inp.table, inp.params, inp.points, inp.fade, lod, u, dx=inp.dx, noise_key=NOISE_KEYS[4])
        assert torch.equal(ref.nz, nz)
        want = ref.dlod.numpy()
        with np.errstate(invalid="ignore"):
            raw = ((np.zeros(N, dtype=F32) if lod is None else lod) + F32(u)).astype(F32)
        lam = raw.astype(np.float64)
        away = (np.minimum(np.abs(ref.a_raw), np.abs(ref.a_raw - 1)) >= 2.0 ** -6).all(axis=1) & (raw >= 2.0 ** -6) & (raw <= 32 - 2.0 ** -6)
        on_ramp = away & ref.ramp.any(axis=1)
        assert mode == "uniform" or on_ramp.sum() >= 20, (mode, on_ramp.sum())
        if away.any():
            safe = np.where(away, lam, 1.0)
            cd = (_loss_rows(inp, safe + h, nz) - _loss_rows(inp, safe - h, nz)) / (2 * h)
            err = np.abs(cd - want)[away].max() / np.abs(want).max()
            print(f"{case} {mode}: central differences at {int(away.sum())} rows ({int(on_ramp.sum())} with a level on the ramp): {err:.3e}")
            assert err <= 1e-9, (mode, err)
        kink = ((ref.a_raw == 1) | (ref.a_raw == 0)).any(axis=1) & ref.passes
        assert kink.any()
        safe = np.where(kink, lam, 1.0)
        right = (_loss_rows(inp, safe + h, nz) - _loss_rows(inp, safe, nz)) / h
        err = np.abs(right - want)[kink].max() / np.abs(want).max()
        print(f"{case} {mode}: differences from the right at {int(kink.sum())} rows on a kink: {err:.3e}")
        assert err <= 1e-9, (mode, err)
        flat = ~ref.passes | ~ref.ramp.any(axis=1)
        assert bool((ref.dlod[torch.from_numpy(flat)] == 0).all()) and bool((ref.dlod[torch.from_numpy(~flat)] != 0).any())


# ------------------------------------------------------------------------------------------------------------------ teeth
def mistakes(tgeo, ref, key, order):
    """dlod of four wrong kernels from the parts of the right one: dW = (blend part) + noise_term(nz), so another noise swaps the second term.
    ``order`` [N] int64: lane pos handles the caller's row order[pos]; the wrong key of that row is sample_base + pos"""
    n = ref.dW.shape[0]
    ramp, keep = torch.from_numpy(ref.ramp), torch.from_numpy(ref.passes)
    blend = ref.dW - noise_term(tgeo, ref.drow, ref.nz)

    def dlod(dW):
        return -(dW * ramp).sum(dim=1) * keep
    by_pos = torch.empty_like(ref.nz)
    by_pos[order] = ref.nz                                                    # row order[pos] gets the noise of key sample_base + pos
    no_base = torch.from_numpy(T.noise(n, tgeo.width, key[0], key[1], key[2], 0))
    return {"the noise left out of r": dlod(blend),
            "noise keyed by the walk position": dlod(blend + noise_term(tgeo, ref.drow, by_pos)),
            "noise keyed without sample_base": dlod(blend + noise_term(tgeo, ref.drow, no_base)),
            "the sign of the noise term flipped": dlod(blend - noise_term(tgeo, ref.drow, ref.nz)),
            "the sign of dlod flipped": -ref.dlod}


@pytest.mark.parametrize("case", CASES, ids=str)
def test_teeth_the_mistakes_are_each_seen_on_the_gpu_tests_inputs(case):
    inp = inputs(*case)
    key = NOISE_KEYS[4]
    assert key[0] == 4 and key[3] != 0
    for mode in MODES:
        lod, u, head = _step_inputs(inp, mode)
        ref = reference_step(inp.tgeo, inp.table, inp.params, inp.points, inp.fade, lod, u, noise_key=key, **head)
        for oname, order in orders(N).items():
            assert not torch.equal(order, torch.arange(N))
            for name, bad in mistakes(inp.tgeo, ref, key, order).items():
                moved = rel(bad, ref.dlod) / TOL_G
                assert moved > 100, (mode, oname, name, moved)
        # the figures of the other depths, printed: the noise term shrinks with 2^-b
        shares = {b: rel(mistakes(inp.tgeo, r, NOISE_KEYS[b], orders(N)["reversed"])["the noise left out of r"], r.dlod)
                  for b in (2, 4, 8) for r in [reference_step(inp.tgeo, inp.table, inp.params, inp.points, inp.fade, lod, u, noise_key=NOISE_KEYS[b], **head)]}
        print(f"{case} {mode}: leaving the noise out moves dlod by " + ", ".join(f"{v:.2e} (b = {b})" for b, v in shares.items()))


# ------------------------------------------------------------------------------------------------------------------ the joint loop of the GPU file
def test_the_joint_loop_on_the_reference_is_deterministic_and_moves():
    """the reference's run of the GPU file's test 7b, twice: the same trajectories, lambda and the shift leave their starts, the loss falls.  No
    recovery of lambda is claimed: a field that is fitted at the same time absorbs a free lambda"""
    from tests.test_hashgrid_lodgrad_cpu import descent_inputs
    geo, tgeo, table, params, points = descent_inputs()
    fade = T.default_fade(tgeo)
    colours = joint_colours(tgeo, table, params, points, fade)
    runs = [run_joint(ReferenceJoint(tgeo, table, params, fade).step, points, colours, torch.device("cpu")) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    lams, shifts, losses = runs[0]
    print(f"joint loop on the reference: lambda {float(lams[0]):.5f} -> {float(lams[-1]):.5f}, shift -> {shifts[-1].tolist()}, "
          f"loss {float(losses[0]):.4e} -> {float(losses[-1]):.4e}")
    assert lams.shape == (JOINT["steps"],) and shifts.shape == (JOINT["steps"], 2) and bool(torch.isfinite(losses).all())
    assert float(lams[-1]) < JOINT["lam_start"] - 0.1 and float(shifts[-1].abs().min()) > 0.05 and float(losses[-1]) < float(losses[0])


# ------------------------------------------------------------------------------------------------------------------ refusals on the host
def test_the_field_refuses_on_the_host():
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, HashGridField, level_resolutions

    def bare(size=(96, 80), level_bits=None, table="present"):
        f = HashGridField.__new__(HashGridField)
        f.field_size, f.device, f.level_bits = size, torch.device("cpu"), level_bits
        f.geo = HashGeometry(size, tuple(level_resolutions(8, 16, max(size))), 2, 12)
        f.table = None if table is None else torch.zeros(1)
        f.hidden, f.n_linear, f.route, f.frozen, f.num_bits, f._lod_fade = 64, 3, "fused", False, None, None
        return f
    pts, target, dp, dl = torch.zeros(5, 2), torch.zeros(5, 3), torch.full((5, 2), 7.0), torch.full((5,), 7.0)
    g = bare(table=None)
    before = dict(g.__dict__)
    for call in (lambda: g.train_points_grad_lod(pts, target, 1.0), lambda: g.train_points_grad_lod(pts, target, 1.0, dp, dl, fused=True),
                 lambda: g.train_points_differentiable_lod(pts, torch.tensor(1.0, requires_grad=True), target),
                 lambda: g.train_points_differentiable_lod(pts, 1.0, target)):
        with pytest.raises(RuntimeError, match="decodes only"):
            call()
    assert g.__dict__ == before
    g = bare(level_bits=(8,) * 8)
    before = dict(g.__dict__)
    for call in (lambda: g.train_points_grad_lod(pts, target, 1.0, dp, dl), lambda: g.train_points_grad_lod(pts, target, torch.zeros(5), fused=True),
                 lambda: g.train_points_differentiable_lod(pts, torch.zeros(5, requires_grad=True), target)):
        with pytest.raises(NotImplementedError, match="bit depth per level"):
            call()
    assert g.__dict__ == before
    f = bare()
    before = dict(f.__dict__)
    with pytest.raises(ValueError, match="lod is a float"):
        f.train_points_grad_lod(pts, target, None, dp, dl)
    with pytest.raises(TypeError):
        f.train_points_grad_lod(pts, target)                                   # lod is required
    for bad in (torch.zeros(5, 3), torch.zeros(5), [[0.0, 0.0]] * 5):
        with pytest.raises(ValueError, match="points must be"):
            f.train_points_grad_lod(bad, target, 1.0, dp, dl)
    with pytest.raises(TypeError, match="dlod"):
        f.train_points_grad_lod(pts, target, 1.0, dp, [0.0] * 5)
    for bad in (torch.zeros(4), torch.zeros(5, 1), torch.zeros(())):
        with pytest.raises(ValueError, match=r"dlod must be \[5\]"):
            f.train_points_grad_lod(pts, target, 1.0, dp, bad)
    with pytest.raises(ValueError, match="dtype"):
        f.train_points_grad_lod(pts, target, 1.0, dp, torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous"):
        f.train_points_grad_lod(pts, target, 1.0, dp, torch.zeros(10)[::2])
    with pytest.raises(ValueError, match=r"dpoints must be \[5, 2\]"):
        f.train_points_grad_lod(pts, target, 1.0, torch.zeros(5, 3), None)
    for kw in (dict(dpoints=dp, dlod=dl), dict(dpoints=None, dlod=None), dict(dpoints=dp, dlod=None)):
        with pytest.raises(RuntimeError, match="HIP device"):                   # host tensors of the right shape: no CPU path
            f.train_points_grad_lod(pts, target, 1.0, **kw)
    for kw in (dict(dpoints=dp), dict(dlod=dl)):
        with pytest.raises(TypeError, match="dpoints and dlod"):
            f.train_points_differentiable_lod(pts.clone().requires_grad_(), 1.0, target, **kw)
    assert f.__dict__ == before and bool((dp == 7.0).all()) and bool((dl == 7.0).all())
