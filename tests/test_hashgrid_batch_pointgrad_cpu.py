"""CPU-only tests of the batch's gradients with respect to the point positions (run with -m "not gpu"):
nic_hash_batch_points_grad and nic_hash_batch_forward_backward_points_grad are exported, declared in the companion header
include/nicv2_hip_ext.h alone and mirrored in _lib.EXT_SIGNATURES (the ABI version stays 9, the main header's 86 entries stay); every argument
error is decided on the host in the documented order (fake pointers and refusals only: nothing launches); the new Python functions and methods
have the specified signatures and the existing ones keep theirs; the wrappers and the class refuse before a device is touched; the kernels
call the shared helpers and restate none.

Teeth, with the float64 reference alone (oracle/hashgrid_train_ref.py) on the inputs tests/test_gpu_hashgrid_batch_pointgrad.py uses: field b
differentiated through field b + 1's table, the gradient scaled by the padded width N where the field's own count belongs, ``dpoints`` written
at the position in the order where the row belongs, and ``lod`` read at the position where the row belongs each move ``C.measure``'s
``dpoints`` entry by more than ``C.TEETH`` x its bound on every shape (smallest movements, x the bound, worst shape, field and count: 7.8e3,
6.9e3, 9.6e3 and 4.9e3; a one-point field has one order: it is left out of the two order cases).

``joint_reference`` / ``with_dpoints`` are shared with the GPU file: both sides see the same bytes."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import hashgrid_train_ref as T
from tests import test_hashgrid_batch_lod_cpu as L
from tests import test_hashgrid_batch_points_cpu as P
from tests import test_hashgrid_train_ref_cpu as C
from tests.test_hashgrid_batch_points_cpu import ARG, NULL, OK, SHAPE, UNSUP, WORKSPACE, REC, _cap, _desc, _mlp, _ref, lib  # noqa: F401
from tests.test_hashgrid_batch_lod_cpu import _bad_lods, _lod, _src

GRAD, JOINT = "nic_hash_batch_points_grad", "nic_hash_batch_forward_backward_points_grad"
ARGS = {GRAD: ["desc", "n_fields", "groups_per_field", "lodp", "src", "points", "lod", "n_points", "counts", "order", "mlp", "dy", "target", "loss_scale", "y",
               "dpoints", "stream"],
        JOINT: ["desc", "n_fields", "groups_per_field", "lodp", "quant", "tables", "points", "lod", "n_points", "counts", "order", "mlp", "target", "loss_scale",
                "table_grads", "mlp_grads", "loss", "y", "dpoints", "flags", "workspace", "workspace_bytes", "stream"]}
PTR = ctypes.c_void_p
N, B = P.N, C.N_FIELDS
GRAD_UNIT, JOINT_UNIT, WALK = "hashgrid_batch_grad.hip", "hashgrid_batch.hip", "hashgrid_pointgrad.hpp"


# ------------------------------------------------------------------------------------------------------------------ shared with the GPU file
def joint_reference(shape, b, n_b, noisy, mode=None):
    """the float64 step of field b on its first n_b points - plain (``mode`` None) or with its level of detail of ``mode`` (the lod file's
    modes) -, ``dpoints`` included; computed once by the files that own the inputs and shared read-only"""
    return P.point_reference(shape, b, n_b, noisy) if mode is None else L.lod_reference(shape, b, n_b, noisy, mode)


def with_dpoints(ref, dpoints):
    """``ref`` with another position gradient: what a mistake that touches ``dpoints`` alone returns"""
    return types.SimpleNamespace(**{**vars(ref), "dpoints": dpoints})


# ------------------------------------------------------------------------------------------------------------------ the C entries
def _grad(lib, d, n_fields=2, groups=0, lodp=None, src="default", points=16, lod=0, n_points=0, counts=0, order=0, m="default", dy=16, target=0, y=16,
          dpoints=16):
    """the return code of the gradient entry with dummy pointers; only calls a host check refuses, or n_points == 0, are made: nothing launches"""
    src = _src() if src == "default" else src
    m = _mlp() if m == "default" else m
    assert n_points <= 0 or n_points >= 1 << 31 or any(v is None for v in (d, src, m)) or not (points and dpoints)
    return lib.nic_hash_batch_points_grad(_ref(d), n_fields, groups, _ref(lodp), _ref(src), PTR(points), PTR(lod), n_points, PTR(counts), PTR(order), _ref(m),
                                          PTR(dy), PTR(target), 1.0, PTR(y), PTR(dpoints), None)


def _joint(lib, d, n_fields=2, groups=0, lodp=None, quant=None, tables=16, points=16, lod=0, n_points=130, counts=0, order=0, m="default", target=16,
           table_grads=16, grads="default", loss=16, y=16, dpoints=16, flags=0, ws=16, ws_bytes=16):
    """the return code of the joint entry; with the 16-byte workspace an accepted call stops at the workspace check"""
    from neural_image_compression_v2_amd._lib import NicMlpGrads
    m = _mlp() if m == "default" else m
    grads = NicMlpGrads() if grads == "default" else grads
    return lib.nic_hash_batch_forward_backward_points_grad(_ref(d), n_fields, groups, _ref(lodp), _ref(quant), PTR(tables), PTR(points), PTR(lod), n_points,
                                                           PTR(counts), PTR(order), _ref(m), PTR(target), 1.0, PTR(table_grads), _ref(grads), PTR(loss), PTR(y),
                                                           PTR(dpoints), flags, PTR(ws), ws_bytes, None)


def test_the_entries_are_exported_declared_in_the_companion_header_only_and_mirrored(lib):
    from neural_image_compression_v2_amd import _lib, hashgrid
    import neural_image_compression_v2_amd as pkg
    header, ext = open(P.HEADER).read(), open(P.EXT_HEADER).read()
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
        assert _lib.EXT_SIGNATURES[name][1][3]._type_ is _lib.NicHashLod          # the nullable nic_hash_lod, where the single-field entries have it
    declared = set(re.findall(r"\b(nic_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", ext, flags=re.S)))
    assert declared == set(_lib.EXT_SIGNATURES) and len(_lib.SIGNATURES) == 86 and _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version()
    assert re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)
    for name in ("hash_batch_points_grad", "hash_batch_forward_backward_points_grad"):
        assert getattr(pkg, name) is getattr(hashgrid, name)


def test_the_python_signatures():
    from neural_image_compression_v2_amd import hashgrid
    sig = inspect.signature(hashgrid.hash_batch_points_grad).parameters
    assert list(sig) == ["geo", "data", "points", "params", "dy", "target", "loss_scale", "counts", "order", "want_y", "kind", "num_bits", "lod", "lod_uniform",
                         "fade", "groups_per_field"]
    assert [sig[k].default for k in list(sig)[4:]] == [None, None, 1.0, None, None, True, "f32", None, None, 0.0, None, 0]
    sig = inspect.signature(hashgrid.hash_batch_forward_backward_points_grad).parameters
    assert list(sig)[:-1] == list(inspect.signature(hashgrid.hash_batch_forward_backward_points_lod).parameters) and list(sig)[-1] == "dpoints"
    assert set(sig) == set(inspect.signature(hashgrid.hash_batch_forward_backward_points).parameters) | {"lod", "lod_uniform", "fade", "dpoints"}
    assert sig["dpoints"].default is None and sig["lod"].default is None and sig["lod_uniform"].default == 0.0 and sig["fade"].default is None
    cls = hashgrid.HashGridFieldBatch
    sig = inspect.signature(cls.point_gradient).parameters
    assert list(sig) == ["self", "points", "dy", "target", "scale", "counts", "order", "lod"]
    assert [sig[k].default for k in list(sig)[2:]] == [None, None, 1.0, None, None, None]
    assert list(inspect.signature(cls.jacobian).parameters) == ["self", "points", "lod"] == list(inspect.signature(cls.query_differentiable).parameters)
    sig = inspect.signature(cls.train_points_grad).parameters
    assert list(sig) == ["self", "points", "target", "dpoints", "lod", "counts", "accumulate", "scale", "step", "noise", "order"]
    assert [sig[k].default for k in list(sig)[3:]] == [None, None, None, False, 1.0, True, None, None]
    sig = inspect.signature(cls.train_points_differentiable).parameters
    assert list(sig) == ["self", "points", "target", "kwargs"] and sig["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    # the existing methods keep their parameter lists
    assert list(inspect.signature(cls.train_points).parameters) == ["self", "points", "target", "counts", "accumulate", "scale", "step", "noise", "order"]
    assert list(inspect.signature(cls.train_points_lod).parameters) == ["self", "points", "target", "lod", "counts", "accumulate", "scale", "step", "noise", "order"]
    assert list(inspect.signature(cls.query).parameters) == ["self", "points", "precision"]
    assert list(inspect.signature(cls.fit_points).parameters) == ["self", "points", "target", "epochs", "counts", "order", "freeze_at"]
    assert list(inspect.signature(hashgrid.hash_batch_forward_backward_points).parameters) == [
        "geo", "tables", "points", "params", "target", "mlp_grads", "table_grads", "order", "counts", "loss", "loss_scale", "want_y", "quant", "add_grads",
        "add_loss", "groups_per_field"]
    doc = cls.__doc__
    assert "4.7.21" in doc and "train_points_grad" in doc and "point_gradient" in doc and "``dpoints`` and the 16-bit" not in doc


def test_gradient_entry_argument_errors_in_the_documented_order(lib):
    d = _desc()
    assert _grad(lib, d) == OK                                            # every check passes; no points: no launch
    # 1. null desc / mlp, whatever else is wrong
    assert _grad(lib, None) == NULL and _grad(lib, d, m=None) == NULL and _grad(lib, None, n_fields=0, groups=3, src=None, n_points=-1) == NULL
    # 2. the fused set, then the descriptor of a point source: before n_fields, the groups and every pointer
    bad = _desc()
    bad.flags = 1
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(resolutions=(16,) * 9, features=8), UNSUP), (_desc(num_crops=2), SHAPE),
                       (big, ARG)]:
        assert _grad(lib, desc) == want and _grad(lib, desc, n_fields=0, groups=3, src=None, dpoints=0, n_points=-1) == want
    assert _grad(lib, d, m=_mlp(5, 5)) == UNSUP
    # 3. n_fields
    for n in (0, -1, 65536):
        assert _grad(lib, d, n_fields=n) == ARG and _grad(lib, d, n_fields=n, groups=3, src=None, n_points=-1) == ARG
    # 4. groups_per_field on ceil(n_points / 64) wave items; no points count as one item
    for g in (-8, 1, 12, 16, 1 << 20):
        assert _grad(lib, d, groups=g) == ARG and _grad(lib, d, groups=g, src=None, dpoints=0, n_points=-1) == ARG
    assert _grad(lib, d, groups=8) == OK
    # 5. null pointers (lodp, lod, counts, order, dy, target and y may be null) - before the source, the level of detail, dy / target and n_points
    for kw in (dict(src=None), dict(src=_src(data=0)), dict(points=0), dict(dpoints=0), dict(m=_mlp(3, 2))):
        assert _grad(lib, d, **kw) == NULL and _grad(lib, d, n_points=-1, dy=0, **kw) == NULL, kw
        assert _grad(lib, d, lodp=_lod(reserved=1), lod=16, **kw) == NULL, kw
    assert _grad(lib, d, y=0, counts=16, order=16) == OK and _grad(lib, d, lodp=_lod(), lod=16) == OK and _grad(lib, d, lodp=_lod(), lod=0) == OK
    # 6. the source: kind, num_bits, alignment
    for src in (_src(kind=7), _src(kind=0, bits=4), _src(kind=1, bits=0), _src(kind=1, bits=9), _src(kind=2, bits=4, data=18)):
        assert _grad(lib, d, src=src) == ARG and _grad(lib, d, src=src, n_points=-1) == ARG
    for src in (_src(kind=1, bits=8), _src(kind=2, bits=4)):
        assert _grad(lib, d, src=src) == OK
    # 7. a per-point array without a nic_hash_lod, then the nic_hash_lod itself
    assert _grad(lib, d, lod=16) == ARG and _grad(lib, d, lod=16, n_points=-1) == ARG
    for lp in _bad_lods():
        assert _grad(lib, d, lodp=lp) == ARG and _grad(lib, d, lodp=lp, lod=16, n_points=-1) == ARG
    assert _grad(lib, _desc(resolutions=(16,) * 4), lodp=_lod((0.0,) * 4 + (-1.0, float("nan")))) == OK       # fade past the levels is ignored
    # 8. exactly one of dy / target
    assert _grad(lib, d, dy=16, target=16) == ARG and _grad(lib, d, dy=0, target=0) == ARG and _grad(lib, d, dy=0, target=16) == OK
    # 9. n_points < 0 or >= 2^31; 10. n_points == 0 is NIC_OK without a launch (the pointers are fakes: a launch would fault)
    for n_points in (-1, -(1 << 40), 1 << 31, 1 << 40):
        assert _grad(lib, d, n_points=n_points) == ARG
    for desc in (d, _desc(dim=3, resolutions=(4, 6, 9, 12), features=1, s_max=12, extent=(12, 10, 9)), _desc(features=8)):
        assert _grad(lib, desc) == OK and _grad(lib, desc, lodp=_lod(), dy=0, target=16, counts=16, order=16) == OK


def test_joint_entry_argument_errors_in_the_documented_order(lib):
    from neural_image_compression_v2_amd._lib import NicHashQuant, NIC_NOISE_KERNEL
    d = _desc()
    cap = _cap(lib)
    for lodp in (None, _lod()):
        assert _joint(lib, d, lodp=lodp) == WORKSPACE                     # every check up to the workspace passes, plain and with a level of detail
        # 1. null desc / mlp
        assert _joint(lib, None, lodp=lodp) == NULL and _joint(lib, d, lodp=lodp, m=None) == NULL
        assert _joint(lib, None, lodp=lodp, n_fields=0, groups=3, tables=0, n_points=-1) == NULL
        # 2. the fused set (then 256 S_max < 2^30)
        bad = _desc()
        bad.flags = 1
        big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
        for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(log2_table=9), ARG), (_desc(num_crops=0), SHAPE),
                           (_desc(resolutions=(16,) * 9, features=8), UNSUP), (big, ARG)]:
            assert _joint(lib, desc, lodp=lodp) == want and _joint(lib, desc, lodp=lodp, n_fields=0, groups=3, tables=0, dpoints=0, n_points=-1) == want
        # 3. n_fields; 4. groups_per_field
        for n in (0, -1, 65536):
            assert _joint(lib, d, lodp=lodp, n_fields=n) == ARG and _joint(lib, d, lodp=lodp, n_fields=n, groups=3, dpoints=0, n_points=-1) == ARG
        for g in (-8, 1, 12, 1 << 20):
            assert _joint(lib, d, lodp=lodp, groups=g) == ARG and _joint(lib, d, lodp=lodp, groups=g, tables=0, dpoints=0, n_points=-1) == ARG
        assert _joint(lib, d, lodp=lodp, groups=16, n_points=130) == ARG and _joint(lib, d, lodp=lodp, groups=8, n_points=130) == WORKSPACE
        # 5. null pointers: dpoints with the others (lodp, lod, counts, order, table_grads and y may be null), before the level of detail and the flags
        for kw in (dict(tables=0), dict(points=0), dict(target=0), dict(grads=None), dict(loss=0), dict(dpoints=0), dict(ws=0), dict(m=_mlp(3, 2))):
            assert _joint(lib, d, lodp=lodp, **kw) == NULL and _joint(lib, d, lodp=lodp, flags=4, n_points=-1, **kw) == NULL, kw
            assert _joint(lib, d, lodp=_lod(uniform=float("nan")), **kw) == NULL and _joint(lib, d, lodp=None, lod=16, **kw) == NULL, kw
        assert _joint(lib, d, lodp=lodp, table_grads=0, y=0) == WORKSPACE and _joint(lib, d, lodp=lodp, counts=16, order=16) == WORKSPACE
        # 7. flags; 8. the quantiser
        for flags in (4, 8, -1):
            assert _joint(lib, d, lodp=lodp, flags=flags) == ARG and _joint(lib, d, lodp=lodp, flags=flags, quant=NicHashQuant(8, 1, 1, 2, 0)) == ARG
        assert _joint(lib, d, lodp=lodp, flags=3) == WORKSPACE
        assert _joint(lib, d, lodp=lodp, quant=NicHashQuant(0, NIC_NOISE_KERNEL, 1, 2, 0)) == ARG
        assert _joint(lib, d, lodp=lodp, quant=NicHashQuant(8, 1, 1, 2, 0)) == UNSUP
        assert _joint(lib, d, lodp=lodp, quant=NicHashQuant(8, NIC_NOISE_KERNEL, 1, 2, 0)) == WORKSPACE
        # 9. the workspace (the siblings' query), before the point descriptor and n_points
        two = _desc(num_crops=2)
        need = lib.nic_hash_batch_points_workspace_bytes(_ref(d), 2, 8, 64 * 4 * 9, _ref(_mlp()))
        assert need == 2 * 8 * REC * 4
        assert _joint(lib, d, lodp=lodp, groups=8, n_points=64 * 4 * 9, ws_bytes=need - 1) == WORKSPACE
        assert _joint(lib, two, lodp=lodp) == WORKSPACE and _joint(lib, d, lodp=lodp, n_points=-1) == WORKSPACE
        # 10. one crop; 11. n_points < 0 or >= 2^31; 12. n_points == 0: NIC_OK with no launch
        enough = 2 * cap * REC * 4
        for n_points in (130, 0, -1):
            assert _joint(lib, two, lodp=lodp, n_points=n_points, ws_bytes=enough) == SHAPE
        for n_points in (-1, -(1 << 40), 1 << 31):
            assert _joint(lib, d, lodp=lodp, n_points=n_points, ws_bytes=enough) == ARG
        need0 = lib.nic_hash_batch_points_workspace_bytes(_ref(d), 2, 0, 0, _ref(_mlp()))
        for flags in (0, 3):
            assert _joint(lib, d, lodp=lodp, n_points=0, ws_bytes=need0, flags=flags, counts=16, order=16, quant=NicHashQuant(8, NIC_NOISE_KERNEL, 1, 2, 0)) == OK
        assert _joint(lib, d, lodp=lodp, n_points=0, ws_bytes=need0 - 1) == WORKSPACE
    # 6. the level of detail, right after the pointers: a per-point array without a nic_hash_lod, then the nic_hash_lod - before the flags, the
    # quantiser, the workspace and n_points
    assert _joint(lib, d, lod=16) == ARG and _joint(lib, d, lod=16, quant=NicHashQuant(8, 1, 1, 2, 0), n_points=-1) == ARG
    assert _joint(lib, d, lodp=_lod(), lod=16) == WORKSPACE
    for lp in _bad_lods():
        assert _joint(lib, d, lodp=lp) == ARG and _joint(lib, d, lodp=lp, flags=4, quant=NicHashQuant(8, 1, 1, 2, 0), n_points=-1) == ARG


# ------------------------------------------------------------------------------------------------------------------ the units
def _kernel(text, name):
    k = text[text.index(f"{name}(const"):]
    return k[:k.index("\n}\n")]


def test_the_kernels_call_the_shared_helpers_and_restate_none():
    from neural_image_compression_v2_amd import _build
    import test_hashgrid_common_cpu as common
    assert GRAD_UNIT in _build.SOURCES and JOINT_UNIT in _build.SOURCES and WALK in _build.HEADERS and len(set(_build.SOURCES)) == len(_build.SOURCES)
    assert not GRAD_UNIT.startswith("hash_")                              # outside the glob of the units hash_common.hpp was cut from
    texts = {f: open(os.path.join(_build.CSRC, f)).read() for f in _build.SOURCES + [h for h in _build.HEADERS if h.endswith(".hpp")]}
    grad, joint, walk = texts[GRAD_UNIT], texts[JOINT_UNIT], texts[WALK]
    for inc in ("hash_common.hpp", "hashgrid_pointgrad.hpp", "hashgrid_batch.hpp"):
        assert re.search(rf'^\s*#include\s+"{re.escape(inc)}"', grad, re.M) and re.search(rf'^\s*#include\s+"{re.escape(inc)}"', joint, re.M), inc
    assert re.search(r'^\s*#include\s+".*nicv2_hip_ext\.h"', grad, re.M)
    device = ["lattice_fixed", "load_decoder", "decoder_forward_half", "decoder_train_half", "write_record", "persistent_grid", "strided_grid", "field_range",
              "field_loss_mul", "field_count", "decoder_dx_half", "point_grad", "point_walk", "point_walk_levels", "kept_axes", "store_point_grad"]
    for name in common.FUNCTIONS + list(common.OVERLOADS) + device:
        assert not any(common._function_re(name).match(ln) for ln in grad.splitlines()), name
    for name in common.STRUCTS + ["DecoderSmem", "TrainSmem", "TrainAcc", "SParams", "StoredSrc"]:
        assert not any(common._struct_re(name).match(ln) for ln in grad.splitlines()), name
    # the walk and the decoder's backward to the input: one definition each, in the shared header
    for name in ("decoder_dx_half", "point_grad", "point_walk", "point_walk_levels", "kept_axes", "store_point_grad"):
        found = sorted(f for f, t in texts.items() if any(common._function_re(name).match(ln) for ln in t.splitlines()))
        assert found == [WALK], (name, found)
    assert "decoder_dx_half<KT>(" in texts["hashgrid_pointgrad.hip"]
    assert "(double)loss_scale / (3.0" not in grad
    # the gradient-only unit: constants in, one writer per row out
    assert "atomic" not in grad and "workspace" not in re.sub(r"//.*", "", grad)
    k = _kernel(grad, "hash_batch_points_grad_kernel")
    for call in ("load_decoder(", "DecoderSmem", "blockIdx.x / (unsigned)p.groups", "field_count(p.counts, b, p.n)", "field_loss_mul(p.loss_scale, n_b)",
                 "field_range(n_waves, lb, p.groups)", "ordered_row(order, n_b, live_lane ? pos : n_b - 1)", "point_lambda(lod_b, p.lod_uniform, row)",
                 "point_fixed<D>(p.d, points, row, t)", "encode_point<D, F, SRC, false, false, LOD>(src_b, t, row, lam, xrow)", "decoder_dx_half<KT>(",
                 "point_grad<D, F, SRC, LOD>(src_b, t, lam, grow, gp)", "if (live_lane) store_point_grad<D>(dpoints, row, kept_axes<D>(p.d, points, row), gp)"):
        assert call in k, call
    assert k.count("__syncthreads()") == 1 and k.index("__syncthreads()") < k.index("for (int64_t g")
    plain = k[k.index("} else {"):]                                        # the branch without d / d lambda, after the DLOD one
    assert k.index("encode_point<") < k.index("decoder_dx_half<KT>(") < k.index("} else {") and "point_walk<" not in plain
    assert plain.index("point_grad<") < plain.index("store_point_grad<D>(")
    # one kernel for this entry and its _lod sibling: the parameter struct a template argument, both KT behind the one launch
    assert "hash_batch_points_grad_kernel<D, F, SRC, 2, LOD, DLOD, P>" in grad and "hash_batch_points_grad_kernel<D, F, SRC, 1, LOD, DLOD, P>" in grad
    assert "p.d.levels * F > 32" in grad and grad.count("__global__") == 1 and "launch<SRC, true, false>(q," in grad and "launch<SRC, false, false>(q," in grad
    # the joint kernel: the training kernels' shape, the backward always to the row, the walk after the scatter
    k = _kernel(joint, "hash_batch_points_joint_kernel")
    for call in ("load_decoder(", "TrainSmem", "field_count(p.counts, b, p.n)", "field_loss_mul(p.loss_scale, n_b)", "field_range(n_waves, lb, p.groups)",
                 "ordered_row(order, n_b, live_lane ? pos : n_b - 1)", "point_lambda(lod_b, p.lod_uniform, row)", "point_fixed<D>(p.d, points, row, t)",
                 "encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, LOD>(src_b, t, row, lam, xrow)", "decoder_train_half<KT>(", "true, A);",
                 "scatter_point<D, F, LOD>(p.d, t, grad,", "point_grad<D, F, NIC_HASH_SRC_F32, LOD>(src_b, t, lam, grow, gp)",
                 "if (live_lane) store_point_grad<D>(dpoints, row, kept_axes<D>(p.d, points, row), gp)", "write_record<KT>("):
        assert call in k, call
    assert k.count("__syncthreads()") == 1 and k.index("__syncthreads()") < k.index("for (int64_t g")
    assert k.index("decoder_train_half<KT>(") < k.index("scatter_point<D, F, LOD>(") < k.index("point_grad<") < k.index("write_record<KT>(")
    assert "hash_batch_points_joint_kernel<D, F, 2, NOISE, LOD>" in joint and "hash_batch_points_joint_kernel<D, F, 1, NOISE, LOD>" in joint
    assert joint.index("hash_batch_points_joint_kernel(const") > joint.index("// ---- host side")          # outside the slices the older tests read
    e = joint[joint.index("int nic_hash_batch_forward_backward_points_grad("):]
    assert "const KernelEndDrop end;" in e and "batch_points_step(p," in e and "tail_block" not in joint
    # the step's host path, shared by the four entries: the launch, the end mark, the one reduction
    st = joint[joint.index("static int batch_points_step("):joint.index("}  // namespace hbatch")]
    assert st.index("launch(std::true_type{})") < st.index("kernel_end_mark((hipStream_t)stream);") < st.index("launch_batch_reduce(")
    assert "hash_batch_reduce_kernel" in joint[joint.index("static int launch_batch_reduce("):joint.index("static int open_batch_points(")]


# ------------------------------------------------------------------------------------------------------------------ the Python surface
def test_the_wrappers_refuse_before_a_device():
    from neural_image_compression_v2_amd import hashgrid
    geo = P._geo()
    tables, params = torch.zeros(3, *geo.table_shape()), P._params(geo)
    pts, target, gm = torch.zeros(3, 7, 2), torch.zeros(3, 7, 3), [torch.zeros_like(p) for p in params]

    def pg(data=tables, points=pts, params=params, dy=target, **kw):
        return hashgrid.hash_batch_points_grad(geo, data, points, params, dy=dy, **kw)

    def fb(tables=tables, points=pts, params=params, target=target, gm=gm, **kw):
        return hashgrid.hash_batch_forward_backward_points_grad(geo, tables, points, params, target, gm, **kw)
    # ---- the gradient entry
    for bad in (tables[0], torch.zeros(3, 4, 512, 2), torch.zeros(3, 100, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="data"):
            pg(data=bad)
    with pytest.raises(TypeError):
        pg(data=None)
    with pytest.raises(ValueError, match="num_bits"):
        pg(num_bits=4)
    with pytest.raises(ValueError, match="num_bits"):
        pg(data=torch.zeros(3, hashgrid.hash_stored_bytes(geo), dtype=torch.uint8), kind="u8")
    with pytest.raises(ValueError, match="table source"):
        pg(kind="f16")
    for k, shape in enumerate([(3, 64, 9), (3, 32), (3, 64, 32), (2, 64), (3, 64, 3), (3,)]):
        bad = list(params)
        bad[k] = torch.zeros(*shape)
        with pytest.raises(ValueError, match="params"):
            pg(params=bad)
    for bad in P.BAD_POINTS:
        with pytest.raises(ValueError, match="points"):
            pg(points=bad)
    with pytest.raises(ValueError, match="exactly one of dy and target"):
        pg(target=target)
    with pytest.raises(ValueError, match="exactly one of dy and target"):
        pg(dy=None)
    for bad in (torch.zeros(7, 3), torch.zeros(2, 7, 3), torch.zeros(3, 8, 3), torch.zeros(3, 7, 4), [[0.0] * 3] * 7):
        with pytest.raises(ValueError, match="dy"):
            pg(dy=bad)
        with pytest.raises(ValueError, match="target"):
            pg(dy=None, target=bad)
    for bad in P.BAD_COUNTS:
        with pytest.raises(ValueError, match="counts"):
            pg(counts=bad)
    for bad in P._bad_orders():
        with pytest.raises(ValueError, match="order"):
            pg(order=bad)
    for bad in L.BAD_LOD_TENSORS:
        with pytest.raises(ValueError, match="lod"):
            pg(lod=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lod_uniform"):
            pg(lod_uniform=bad)
    for bad in ((1.0,) * 3, (1.0, 1.0, -1.0, 1.0), "abcd"):
        with pytest.raises(ValueError, match="fade"):
            pg(fade=bad)
    for bad in (torch.zeros(3, 7, 4), torch.zeros(3, 7, 3, dtype=torch.float64), torch.zeros(3, 3, 7).transpose(1, 2)):
        with pytest.raises(ValueError, match="want_y"):
            pg(want_y=bad)
    with pytest.raises(ValueError, match="too large"):
        hashgrid.hash_batch_points_grad(hashgrid.HashGeometry((1 << 22, 8), (1, 1), 2, 10), torch.zeros(3, 2, 1024, 2), pts, P._params(P._geo(levels=2)), dy=target)
    # with everything shaped right the refusal is the device's: nothing was launched
    for counts in P.GOOD_COUNTS:
        with pytest.raises(RuntimeError, match="HIP device"):
            pg(counts=counts, order=torch.zeros(3, 7, dtype=torch.int32), lod=torch.zeros(7), lod_uniform=0.5, want_y=torch.zeros(3, 7, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        pg(points=torch.zeros(7, 2), dy=None, target=target, want_y=False)
    # ---- the joint entry: the sibling's refusals, then dpoints'
    with pytest.raises(ValueError, match="tables"):
        fb(tables=tables[0])
    for bad in P.BAD_POINTS:
        with pytest.raises(ValueError, match="points"):
            fb(points=bad)
    with pytest.raises(ValueError, match="target"):
        fb(target=torch.zeros(3, 8, 3))
    for bad in P.BAD_COUNTS:
        with pytest.raises(ValueError, match="counts"):
            fb(counts=bad)
    for bad in L.BAD_LOD_TENSORS:
        with pytest.raises(ValueError, match="lod"):
            fb(lod=bad)
    with pytest.raises(TypeError, match="dpoints"):
        fb(dpoints=[[0.0, 0.0]] * 7)
    for bad in (torch.zeros(7, 2), torch.zeros(2, 7, 2), torch.zeros(3, 7, 3), torch.zeros(3, 8, 2), torch.zeros(3, 7, 2, dtype=torch.float64),
                torch.zeros(3, 2, 7).transpose(1, 2)):
        with pytest.raises(ValueError, match="dpoints"):
            fb(dpoints=bad)
    for kw in (dict(), dict(dpoints=torch.zeros(3, 7, 2)), dict(lod=torch.zeros(3, 7), counts=(7, 0, 3), order=torch.zeros(3, 7, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match="HIP device"):
            fb(**kw)


def test_the_class_refuses_on_the_host():
    f = P._bare()
    before = dict(f.__dict__)
    pts, target = torch.zeros(3, 7, 2), torch.zeros(3, 7, 3)
    for bad in P.BAD_POINTS:
        for call in (lambda: f.point_gradient(bad, dy=target), lambda: f.train_points_grad(bad, target), lambda: f.jacobian(bad),
                     lambda: f.train_points_differentiable(bad, target)):
            with pytest.raises(ValueError, match="points"):
                call()
    with pytest.raises(ValueError, match="exactly one of dy and target"):
        f.point_gradient(pts)
    with pytest.raises(ValueError, match="exactly one of dy and target"):
        f.point_gradient(pts, dy=target, target=target)
    for bad in (torch.zeros(7, 3), torch.zeros(3, 8, 3), None):
        if bad is not None:
            with pytest.raises(ValueError, match="dy"):
                f.point_gradient(pts, dy=bad)
        with pytest.raises(ValueError, match="target"):
            f.train_points_grad(pts, bad)
    for bad in P.BAD_COUNTS:
        with pytest.raises(ValueError, match="counts"):
            f.point_gradient(pts, dy=target, counts=bad)
        with pytest.raises(ValueError, match="counts"):
            f.train_points_grad(pts, target, counts=bad)
    for bad in P._bad_orders() + ("morton", "Cell", ""):
        with pytest.raises(ValueError, match="order"):
            f.point_gradient(pts, target=target, order=bad)
        with pytest.raises(ValueError, match="order"):
            f.train_points_grad(pts, target, order=bad)
    for bad in L.BAD_LOD_TENSORS + L.BAD_LOD_VALUES:
        with pytest.raises(ValueError, match="lod"):
            f.point_gradient(pts, dy=target, lod=bad)
        with pytest.raises(ValueError, match="lod"):
            f.train_points_grad(pts, target, lod=bad)
    with pytest.raises(TypeError, match="dpoints"):
        f.train_points_grad(pts, target, dpoints=[[0.0, 0.0]] * 7)
    for bad in (torch.zeros(7, 2), torch.zeros(3, 7, 3), torch.zeros(3, 7, 2, dtype=torch.float64), torch.zeros(3, 2, 7).transpose(1, 2)):
        with pytest.raises(ValueError, match="dpoints"):
            f.train_points_grad(pts, target, dpoints=bad)
    with pytest.raises(TypeError, match="dpoints"):
        f.train_points_differentiable(pts, target, dpoints=torch.zeros(3, 7, 2))
    with pytest.raises(ValueError, match="noise"):
        f.train_points_grad(pts, target, noise=True)                      # no codec: no noise
    # everything right: the refusal is the device's
    for counts in (None, (7, 0, 3)):
        for order in (None, "cell", torch.zeros(3, 7, dtype=torch.int32)):
            for lod in (None, 0.5, torch.zeros(7)):
                with pytest.raises(RuntimeError, match="HIP device"):
                    f.point_gradient(pts, dy=target, counts=counts, order=order, lod=lod)
                with pytest.raises(RuntimeError, match="HIP device"):
                    f.train_points_grad(pts, target, counts=counts, order=order, lod=lod, dpoints=torch.zeros(3, 7, 2))
    with pytest.raises(RuntimeError, match="HIP device"):
        f.jacobian(torch.zeros(7, 2))
    with pytest.raises(RuntimeError, match="HIP device"):
        f.query_differentiable(pts.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="HIP device"):
        f.train_points_differentiable(pts.clone().requires_grad_(True), target)
    assert f.__dict__.keys() == before.keys() and all(f.__dict__[k] is before[k] for k in before)       # nothing was set on the way to a refusal
    # a decode-only batch: the training calls refuse before they look at an argument; the gradient reads the stored tables
    g = P._bare(decode_only=True, num_bits=8, frozen=True)
    with pytest.raises(RuntimeError, match="decode-only"):
        g.train_points_grad(None, None)
    with pytest.raises(RuntimeError, match="decode-only"):
        g.train_points_differentiable(pts.clone().requires_grad_(True), target)
    with pytest.raises(RuntimeError, match="HIP device"):
        g.point_gradient(pts, dy=target)


# ------------------------------------------------------------------------------------------------------------------ teeth
def _moved(bad_dpoints, ref):
    err, bound = C.measure(with_dpoints(ref, bad_dpoints), ref)["dpoints"]
    return err / bound


def test_every_fields_set_has_a_clamped_axis_and_a_gradient():
    """what "an axis whose clamp moved the point gets exactly 0" is tested on: every field's points - even its shortest prefixes but the
    one-point one - hold a clamped axis, and the reference's gradient is exactly zero there and not zero everywhere else"""
    for shape in C.SHAPES:
        for b in range(B):
            f = P.field_inputs(shape, b)
            for n_b in sorted({n for c in P.COUNTS[1:] for n in c if n > 1}):
                moved = T.clamp_points(f.geo, f.points[:n_b])[1]
                assert moved.any() and not moved.all(), (shape, b, n_b)
            ref = joint_reference(shape, b, N, False)
            moved = torch.from_numpy(T.clamp_points(f.geo, f.points)[1])
            assert ref.dpoints.shape == (N, shape[0]) and bool((ref.dpoints[moved] == 0).all()) and bool((ref.dpoints[~moved] != 0).any())
            assert bool(torch.isfinite(ref.dpoints).all())


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_teeth_a_field_through_its_neighbours_table(shape):
    """field b differentiated through field b + 1's table (its own points, decoder and targets)"""
    for b in range(B):
        f, nxt = P.field_inputs(shape, b), P.field_inputs(shape, (b + 1) % B)
        bad = T.step(f.geo, nxt.table, f.params, f.target, points=f.points, loss_scale=C.LOSS_SCALE)
        ratio = _moved(bad.dpoints, joint_reference(shape, b, N, False))
        print(f"{C.shape_id(shape)} field {b} through field {(b + 1) % B}'s table: dpoints moves by {ratio:.1f} x its bound")
        assert ratio > C.TEETH


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_teeth_the_gradient_is_scaled_by_the_fields_own_count(shape):
    """2 (y - target) loss_scale / (3 N) with the padded N = 209 where the field's n_b belongs: every count below 209 the GPU test uses"""
    for counts in P.COUNTS[1:]:
        for b, n_b in enumerate(counts):
            if n_b in (0, N):
                continue
            ref = joint_reference(shape, b, n_b, False)
            ratio = _moved(ref.dpoints * (n_b / N), ref)
            print(f"{C.shape_id(shape)} field {b}, {n_b} of {N} points: dpoints moves by {ratio:.1f} x its bound")
            assert ratio > C.TEETH


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_teeth_dpoints_is_written_at_the_row(shape):
    """with an order, lane ``pos`` handles row order[pos]: its gradient stored at ``pos`` where the row belongs"""
    for counts in P.COUNTS:
        for b in range(B):
            n_b = P.count_of(counts, b)
            if n_b < 2:                         # no point, or one point: one order
                continue
            perm = L.permutation(b, n_b)
            assert not torch.equal(perm, torch.arange(n_b))
            ref = joint_reference(shape, b, n_b, False)
            ratio = _moved(ref.dpoints[perm], ref)
            print(f"{C.shape_id(shape)} field {b}, {n_b} points, dpoints by position: moves by {ratio:.1f} x its bound")
            assert ratio > C.TEETH


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_teeth_lod_is_read_at_the_row(shape):
    """with an order and a level of detail per point, lane ``pos`` handles row order[pos] with lod[pos] where lod[order[pos]] belongs"""
    for counts in P.COUNTS:
        for b in range(B):
            n_b = P.count_of(counts, b)
            if n_b < 2:
                continue
            f = P.field_inputs(shape, b)
            fade, lod, u = L.lod_of(shape, b, "point")
            perm = L.permutation(b, n_b)
            at_pos = np.empty(n_b, dtype=np.float32)
            at_pos[perm.numpy()] = lod[:n_b]                                # row order[pos] gets lod[pos]
            bad = T.step(f.geo, f.table, f.params, f.target[:n_b], points=f.points[:n_b], loss_scale=C.LOSS_SCALE, lod=(fade, at_pos, u))
            ratio = _moved(bad.dpoints, joint_reference(shape, b, n_b, False, "point"))
            print(f"{C.shape_id(shape)} field {b}, {n_b} points, lod by position: dpoints moves by {ratio:.1f} x its bound")
            assert ratio > C.TEETH
