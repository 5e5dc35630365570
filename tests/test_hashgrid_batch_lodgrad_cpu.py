"""CPU-only tests of the batch's gradients with respect to the level of detail (run with -m "not gpu"):
nic_hash_batch_points_grad_lod and nic_hash_batch_forward_backward_points_grad_lod are exported, declared in the companion header
include/nicv2_hip_ext.h alone and mirrored in _lib.EXT_SIGNATURES with their argument lists held to the siblings' (one pointer, dlod, after
dpoints); the ABI version stays 9 and the main header's 86 entries stay; every argument error is decided on the host in the documented order
(fake pointers and refusals only: nothing launches); the wrappers and the class refuse before a device is touched; the two kernels call the
one shared walk and restate no helper.

The inputs are built from existing pieces: field 0 of a case is ``inputs(*case)`` of tests/test_hashgrid_lodgrad_cpu.py as it stands, fields 1
and 2 draw their own table, decoder, points and target from other seeds on the same geometry and carry ``lod_rows(fade)`` with the rows of
wave 0 that sit exactly on a kink moved to other lanes of that wave.  The reference of field b is ``reference_step`` of
tests/test_hashgrid_lodtrain_cpu.py on field b's own tensors and first n_b rows; it is never the code under test.

Teeth, on these inputs: reading the neighbour field's lod / table / decoder, storing dlod at the position in the order instead of at the row,
scaling by the padded N instead of n_b, dropping the noise term and keying the noise by position instead of by row each move the reference's
dlod of some field beyond TOL_G (the factors are printed).

``batch_inputs``, ``field_reference``, ``COUNTS`` and ``permutation`` are shared with the GPU file: both sides see the same bytes."""
import ctypes
import functools
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import hashgrid_train_ref as T
from tests import test_hashgrid_batch_points_cpu as P
from tests import test_hashgrid_lodgrad_cpu as G
from tests import test_hashgrid_lodtrain_cpu as S
from tests.test_hashgrid_batch_points_cpu import ARG, NULL, OK, SHAPE, UNSUP, WORKSPACE, REC, HEADER, EXT_HEADER, _cap, _desc, _mlp, _ref, lib  # noqa: F401
from tests.test_hashgrid_batch_lod_cpu import BAD_LOD_TENSORS, BAD_LOD_VALUES, _bad_lods, _lod, _src
from tests.test_hashgrid_lodgrad_cpu import CASES, MODES, N, TARGET_SCALE, TOL_G, inputs, lod_rows, ramp_f32, rel
from tests.test_hashgrid_lodtrain_cpu import NOISE_KEYS, reference_step

GRAD, JOINT = "nic_hash_batch_points_grad_lod", "nic_hash_batch_forward_backward_points_grad_lod"
SIBLINGS = {GRAD: "nic_hash_batch_points_grad", JOINT: "nic_hash_batch_forward_backward_points_grad"}
ARGS = {GRAD: ["desc", "n_fields", "groups_per_field", "lodp", "src", "points", "lod", "n_points", "counts", "order", "mlp", "dy", "target", "loss_scale", "y",
               "dpoints", "dlod", "stream"],
        JOINT: ["desc", "n_fields", "groups_per_field", "lodp", "quant", "tables", "points", "lod", "n_points", "counts", "order", "mlp", "target", "loss_scale",
                "table_grads", "mlp_grads", "loss", "y", "dpoints", "dlod", "flags", "workspace", "workspace_bytes", "stream"]}
PTR = ctypes.c_void_p
GRAD_UNIT, JOINT_UNIT, WALK = "hashgrid_batch_grad.hip", "hashgrid_batch.hip", "hashgrid_pointgrad.hpp"

# ------------------------------------------------------------------------------------------------------------------ shared with the GPU file
B = 3
COUNTS = [None, (130, 65, 1), (64, 0, 63)]                 # a full row; two waves and one lane, one point; a whole wave, nothing, one short of a wave
LOSS_SCALE = TARGET_SCALE * N                              # one value for the launch: field b's output gradient is 2 (y - target) LOSS_SCALE / (3 n_b)
KINK_ROWS = 20                                             # rows 0 .. 19 of lod_rows: the kinks, 0 / -1 / 32 / 40 / NaN and random values
MOVED_TO = {1: 24, 2: 44}                                  # fields 1 and 2: those rows swapped with rows 24 .. 43 / 44 .. 63 of the same wave


def count_of(counts, b):
    return N if counts is None else counts[b]


def field_lod_rows(fade, b):
    """``lod_rows(fade)``; for fields 1 and 2 with rows 0 .. 19 swapped with 20 other rows of wave 0.  Rows 20 .. 23 (the outside points), 64 ..
    127 (every level off) and 128 / 129 stay where they are"""
    lod = lod_rows(fade).copy()
    if b:
        k = MOVED_TO[b]
        head, other = lod[:KINK_ROWS].copy(), lod[k:k + KINK_ROWS].copy()
        lod[:KINK_ROWS], lod[k:k + KINK_ROWS] = other, head
    return lod


@functools.lru_cache(maxsize=None)
def batch_inputs(case):
    """the B = 3 fields of a case on its one geometry, as fp32 CPU tensors (read-only): field 0 is ``inputs(*case)``; fields 1 and 2 draw a
    table uniform in +- 0.5, a decoder, 130 points (rows 20 .. 23 and 129 outside the field, one of them a NaN) and a target of their own"""
    dim, features, levels = case
    f0 = inputs(*case)
    size = G.SIZES[dim]
    fields = [types.SimpleNamespace(table=f0.table, params=f0.params, points=f0.points, target=f0.target, dy=f0.dy, lod=f0.lod)]
    for b in (1, 2):
        g = torch.Generator().manual_seed(50000 * b + 1000 * dim + 10 * features + levels)
        table = (torch.rand(levels, 1 << G.LOG2_TABLE, features, generator=g) - 0.5).contiguous()
        points = torch.rand(N, dim, generator=g) * torch.tensor([float(s) for s in size]) - 0.5
        points[20, dim - 1] = -2.0 - b
        points[21, 0] = size[0] + 1.5 * b
        points[22] = torch.tensor([size[0] + 0.25, -1.0, -7.0][:dim])
        points[23, 1] = float("nan")
        points[129, 1] = size[1] + 3.0
        fields.append(types.SimpleNamespace(table=table, params=G.decoder_params(levels * features, 7 * dim + features + 31 * b), points=points.contiguous(),
                                            target=torch.rand(N, 3, generator=g), dy=torch.rand(N, 3, generator=g) * 2 - 1,
                                            lod=field_lod_rows(f0.fade, b)))
    return types.SimpleNamespace(geo=f0.geo, tgeo=f0.tgeo, fade=f0.fade, fields=fields)


def field_lod(bi, b, mode, n_b=N):
    """(lod [n_b] or None, lod_uniform) of field b in ``mode`` (MODES of tests/test_hashgrid_lodgrad_cpu.py)"""
    per_point, u = MODES[mode]
    return (bi.fields[b].lod[:n_b].copy() if per_point else None), u


def stacked(bi, name):
    """[B, ...]: the tensors ``name`` of the three fields, stacked"""
    if name == "params":
        return [torch.stack([f.params[k] for f in bi.fields]).contiguous() for k in range(6)]
    if name == "lod":
        return torch.from_numpy(np.stack([f.lod for f in bi.fields])).contiguous()
    return torch.stack([getattr(f, name) for f in bi.fields]).contiguous()


def permutation(b, n_b):
    """the fixed permutation of field b's own rows (the "perm" order)"""
    return torch.randperm(n_b, generator=torch.Generator().manual_seed(41 + b))


def field_reference(case, b, n_b, mode, bits=None, sample_base=None):
    """``reference_step`` of field b of a case on its own tensors and its first n_b rows with LOSS_SCALE (the mean is over n_b); ``bits``: None,
    or the noise of NOISE_KEYS[bits] (``sample_base`` overrides its last entry).  Computed once and shared (read-only)"""
    return _field_reference(tuple(case), int(b), int(n_b), str(mode), bits, sample_base)


@functools.lru_cache(maxsize=None)
def _field_reference(case, b, n_b, mode, bits, sample_base):
    bi = batch_inputs(case)
    f = bi.fields[b]
    lod, u = field_lod(bi, b, mode, n_b)
    key = None if bits is None else NOISE_KEYS[bits] if sample_base is None else NOISE_KEYS[bits][:3] + (sample_base,)
    return reference_step(bi.tgeo, f.table, f.params, f.points[:n_b], bi.fade, lod, u, target=f.target[:n_b], loss_scale=LOSS_SCALE, noise_key=key)


def close(got, want):
    """the largest difference as a share of the reference's largest magnitude; a reference that is zero everywhere is met by zeros alone"""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    top = float(want.abs().max())
    if top == 0.0:
        return 0.0 if bool((got == 0).all()) else float("inf")
    return float((got - want).abs().max() / top)


@pytest.fixture(autouse=True)
def the_feature_is_there():
    """everything in this file - the inputs and the teeth too - is about the two entries and the five methods: without them nothing here holds"""
    from neural_image_compression_v2_amd import _lib
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch
    assert GRAD in _lib.EXT_SIGNATURES and JOINT in _lib.EXT_SIGNATURES
    for name in ("point_gradient_lod", "jacobian_lod", "query_differentiable_lod", "train_points_grad_lod", "train_points_differentiable_lod"):
        assert callable(getattr(HashGridFieldBatch, name, None)), name


# ------------------------------------------------------------------------------------------------------------------ the C entries
def _grad(lib, d, n_fields=2, groups=0, lodp="default", src="default", points=16, lod=0, n_points=0, counts=0, order=0, m="default", dy=16, target=0, y=16,
          dpoints=16, dlod=16):
    """the return code of the gradient entry with dummy pointers; only calls a host check refuses, or n_points == 0, are made: nothing launches"""
    lodp = _lod() if lodp == "default" else lodp
    src = _src() if src == "default" else src
    m = _mlp() if m == "default" else m
    assert n_points <= 0 or n_points >= 1 << 31
    return getattr(lib, GRAD)(_ref(d), n_fields, groups, _ref(lodp), _ref(src), PTR(points), PTR(lod), n_points, PTR(counts), PTR(order), _ref(m), PTR(dy),
                              PTR(target), 1.0, PTR(y), PTR(dpoints), PTR(dlod), None)


def _joint(lib, d, n_fields=2, groups=0, lodp="default", quant=None, tables=16, points=16, lod=0, n_points=130, counts=0, order=0, m="default", target=16,
           table_grads=16, grads="default", loss=16, y=16, dpoints=16, dlod=16, flags=0, ws=16, ws_bytes=16):
    """the return code of the training entry; with the 16-byte workspace an accepted call stops at the workspace check, and with a workspace
    that passes only calls a LATER check refuses, or n_points == 0, are made: nothing launches"""
    from neural_image_compression_v2_amd._lib import NicMlpGrads
    lodp = _lod() if lodp == "default" else lodp
    m = _mlp() if m == "default" else m
    grads = NicMlpGrads() if grads == "default" else grads
    return getattr(lib, JOINT)(_ref(d), n_fields, groups, _ref(lodp), _ref(quant), PTR(tables), PTR(points), PTR(lod), n_points, PTR(counts), PTR(order),
                               _ref(m), PTR(target), 1.0, PTR(table_grads), _ref(grads), PTR(loss), PTR(y), PTR(dpoints), PTR(dlod), flags, PTR(ws), ws_bytes,
                               None)


def _c_args(text, name):
    m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_entries_are_exported_declared_in_the_companion_header_only_and_mirrored(lib):
    from neural_image_compression_v2_amd import _lib, hashgrid
    import neural_image_compression_v2_amd as pkg
    header, ext = open(HEADER).read(), open(EXT_HEADER).read()
    types_of = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    for name, names in ARGS.items():
        assert hasattr(lib, name)
        assert name not in header and name not in _lib.SIGNATURES and name in _lib.EXT_SIGNATURES
        res, args = _lib.EXT_SIGNATURES[name]
        cargs = _c_args(ext, name)
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
        # the sibling argument for argument, with one pointer - dlod - after dpoints
        sargs = _c_args(ext, SIBLINGS[name])
        k = [c.split()[-1].lstrip("*") for c in sargs].index("dpoints")
        assert cargs == sargs[:k + 1] + ["float *dlod"] + sargs[k + 1:], name
        sres, sig = _lib.EXT_SIGNATURES[SIBLINGS[name]]
        assert sres is res and args == sig[:k + 1] + [ctypes.c_void_p] + sig[k + 1:]
    declared = set(re.findall(r"\b(nic_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", ext, flags=re.S)))
    assert declared == set(_lib.EXT_SIGNATURES) and len(_lib.SIGNATURES) == 86 and _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version()
    assert re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)
    for name in ("hash_batch_points_grad_lod", "hash_batch_forward_backward_points_grad_lod"):
        assert getattr(pkg, name) is getattr(hashgrid, name)


def test_the_python_signatures():
    from neural_image_compression_v2_amd import hashgrid
    sig = inspect.signature(hashgrid.hash_batch_points_grad_lod).parameters
    assert list(sig)[:7] == ["geo", "data", "points", "params", "lod", "lod_uniform", "fade"] and list(sig)[-2:] == ["dpoints", "dlod"]
    assert set(sig) == set(inspect.signature(hashgrid.hash_batch_points_grad).parameters) | {"dpoints", "dlod"}
    sig = inspect.signature(hashgrid.hash_batch_forward_backward_points_grad_lod).parameters
    assert list(sig)[:-1] == list(inspect.signature(hashgrid.hash_batch_forward_backward_points_grad).parameters) and list(sig)[-1] == "dlod"
    assert sig["dlod"].default is None and sig["dpoints"].default is None
    cls = hashgrid.HashGridFieldBatch
    sig = inspect.signature(cls.point_gradient_lod).parameters
    assert list(sig) == ["self", "points", "lod", "dy", "target", "scale", "counts", "order"]
    assert [sig[k].default for k in list(sig)[3:]] == [None, None, 1.0, None, None]
    assert list(inspect.signature(cls.jacobian_lod).parameters) == ["self", "points", "lod"] == list(inspect.signature(cls.query_differentiable_lod).parameters)
    sig = inspect.signature(cls.train_points_grad_lod).parameters
    assert list(sig) == ["self", "points", "target", "lod", "dpoints", "dlod", "counts", "accumulate", "scale", "step", "noise", "order"]
    assert [sig[k].default for k in list(sig)[4:]] == [None, None, None, False, 1.0, True, None, None]
    sig = inspect.signature(cls.train_points_differentiable_lod).parameters
    assert list(sig) == ["self", "points", "lod", "target", "kwargs"] and sig["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    # the existing methods keep their parameter lists
    assert list(inspect.signature(cls.point_gradient).parameters) == ["self", "points", "dy", "target", "scale", "counts", "order", "lod"]
    assert list(inspect.signature(cls.train_points_grad).parameters) == ["self", "points", "target", "dpoints", "lod", "counts", "accumulate", "scale", "step",
                                                                         "noise", "order"]
    assert list(inspect.signature(cls.query_differentiable).parameters) == ["self", "points", "lod"]
    assert list(inspect.signature(cls.query_lod).parameters) == ["self", "points", "lod", "precision"]
    assert "4.7.25" in cls.__doc__ and "point_gradient_lod" in cls.__doc__ and "a gradient with respect to the level of detail;" not in cls.__doc__


def test_gradient_entry_argument_errors_in_the_documented_order(lib):
    d = _desc()
    assert _grad(lib, d) == OK                                            # every check passes; no points: no launch
    # 1. null desc / mlp, whatever else is wrong
    assert _grad(lib, None) == NULL and _grad(lib, d, m=None) == NULL and _grad(lib, None, n_fields=0, groups=3, src=None, lodp=None, n_points=-1) == NULL
    # 2. the fused set, then the descriptor of a point source: before n_fields, the groups and every pointer
    bad = _desc()
    bad.flags = 1
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(resolutions=(16,) * 9, features=8), UNSUP), (_desc(num_crops=2), SHAPE),
                       (big, ARG)]:
        assert _grad(lib, desc) == want and _grad(lib, desc, n_fields=0, groups=3, src=None, lodp=None, dpoints=0, dlod=0, n_points=-1) == want
    assert _grad(lib, d, m=_mlp(5, 5)) == UNSUP
    # 3. n_fields; 4. groups_per_field on ceil(n_points / 64) wave items, no points counting as one item
    for n in (0, -1, 65536):
        assert _grad(lib, d, n_fields=n) == ARG and _grad(lib, d, n_fields=n, groups=3, src=None, dlod=0, n_points=-1) == ARG
    for g in (-8, 1, 12, 16, 1 << 20):
        assert _grad(lib, d, groups=g) == ARG and _grad(lib, d, groups=g, lodp=None, dlod=0, n_points=-1) == ARG
    assert _grad(lib, d, groups=8) == OK
    # 5. null pointers: lodp and dlod with the sibling's (lod, counts, order, dy, target and y may be null) - before the source, the nic_hash_lod,
    #    dy / target and n_points
    for kw in (dict(lodp=None), dict(src=None), dict(src=_src(data=0)), dict(points=0), dict(dpoints=0), dict(dlod=0), dict(m=_mlp(3, 2))):
        assert _grad(lib, d, **kw) == NULL and _grad(lib, d, n_points=-1, dy=0, **kw) == NULL, kw
        if "src" not in kw and "lodp" not in kw:
            assert _grad(lib, d, **dict(kw, src=_src(kind=7), lodp=_lod(reserved=1))) == NULL, kw
    assert _grad(lib, d, y=0, counts=16, order=16, lod=16) == OK and _grad(lib, d, lod=0) == OK
    # 6. the source: kind, num_bits, alignment - before the nic_hash_lod
    for src in (_src(kind=7), _src(kind=0, bits=4), _src(kind=1, bits=0), _src(kind=1, bits=9), _src(kind=2, bits=4, data=18)):
        assert _grad(lib, d, src=src) == ARG and _grad(lib, d, src=src, lodp=_lod(reserved=1), n_points=-1) == ARG
    for src in (_src(kind=1, bits=8), _src(kind=2, bits=4)):
        assert _grad(lib, d, src=src) == OK
    # 7. the nic_hash_lod - before dy / target and n_points
    for lp in _bad_lods():
        assert _grad(lib, d, lodp=lp) == ARG and _grad(lib, d, lodp=lp, lod=16, dy=0, n_points=-1) == ARG
    assert _grad(lib, _desc(resolutions=(16,) * 4), lodp=_lod((0.0,) * 4 + (-1.0, float("nan")))) == OK       # fade past the levels is ignored
    # 8. exactly one of dy / target
    assert _grad(lib, d, dy=16, target=16) == ARG and _grad(lib, d, dy=0, target=0) == ARG and _grad(lib, d, dy=0, target=16) == OK
    assert _grad(lib, d, dy=16, target=16, n_points=-1) == ARG
    # 9. n_points < 0 or >= 2^31; 10. n_points == 0 is NIC_OK without a launch (the pointers are fakes: a launch would fault)
    for n_points in (-1, -(1 << 40), 1 << 31, 1 << 40):
        assert _grad(lib, d, n_points=n_points) == ARG
    for desc in (d, _desc(dim=3, resolutions=(4, 6, 9, 12), features=1, s_max=12, extent=(12, 10, 9)), _desc(features=8)):
        assert _grad(lib, desc) == OK and _grad(lib, desc, lodp=_lod(uniform=1.5), dy=0, target=16, counts=16, order=16, lod=16) == OK


def test_training_entry_argument_errors_in_the_documented_order(lib):
    from neural_image_compression_v2_amd._lib import NicHashQuant, NIC_NOISE_KERNEL
    d = _desc()
    cap = _cap(lib)
    assert _joint(lib, d) == WORKSPACE                                    # every check up to the workspace passes
    # 1. null desc / mlp
    assert _joint(lib, None) == NULL and _joint(lib, d, m=None) == NULL and _joint(lib, None, lodp=None, n_fields=0, groups=3, tables=0, n_points=-1) == NULL
    # 2. the fused set (then 256 S_max < 2^30)
    bad = _desc()
    bad.flags = 1
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(log2_table=9), ARG), (_desc(num_crops=0), SHAPE),
                       (_desc(resolutions=(16,) * 9, features=8), UNSUP), (big, ARG)]:
        assert _joint(lib, desc) == want and _joint(lib, desc, lodp=None, n_fields=0, groups=3, tables=0, dpoints=0, dlod=0, n_points=-1) == want
    # 3. n_fields; 4. groups_per_field
    for n in (0, -1, 65536):
        assert _joint(lib, d, n_fields=n) == ARG and _joint(lib, d, n_fields=n, groups=3, dlod=0, n_points=-1) == ARG
    for g in (-8, 1, 12, 1 << 20):
        assert _joint(lib, d, groups=g) == ARG and _joint(lib, d, groups=g, tables=0, lodp=None, dlod=0, n_points=-1) == ARG
    assert _joint(lib, d, groups=16, n_points=130) == ARG and _joint(lib, d, groups=8, n_points=130) == WORKSPACE
    # 5. null pointers: lodp and dlod with the sibling's (quant, lod, counts, order, table_grads and y may be null), before the nic_hash_lod and the flags
    for kw in (dict(lodp=None), dict(tables=0), dict(points=0), dict(target=0), dict(grads=None), dict(loss=0), dict(dpoints=0), dict(dlod=0), dict(ws=0),
               dict(m=_mlp(3, 2))):
        assert _joint(lib, d, **kw) == NULL and _joint(lib, d, flags=4, n_points=-1, **kw) == NULL, kw
        if "lodp" not in kw:
            assert _joint(lib, d, lodp=_lod(uniform=float("nan")), **kw) == NULL, kw
    assert _joint(lib, d, table_grads=0, y=0) == WORKSPACE and _joint(lib, d, counts=16, order=16, lod=16) == WORKSPACE
    # 6. the nic_hash_lod, right after the pointers - before the flags, the quantiser, the workspace and n_points
    for lp in _bad_lods():
        assert _joint(lib, d, lodp=lp) == ARG and _joint(lib, d, lodp=lp, flags=4, quant=NicHashQuant(8, 1, 1, 2, 0), n_points=-1) == ARG
    # 7. flags; 8. the quantiser
    for flags in (4, 8, -1):
        assert _joint(lib, d, flags=flags) == ARG and _joint(lib, d, flags=flags, quant=NicHashQuant(8, 1, 1, 2, 0)) == ARG
    assert _joint(lib, d, flags=3) == WORKSPACE
    assert _joint(lib, d, quant=NicHashQuant(0, NIC_NOISE_KERNEL, 1, 2, 0)) == ARG
    assert _joint(lib, d, quant=NicHashQuant(8, 1, 1, 2, 0)) == UNSUP
    assert _joint(lib, d, quant=NicHashQuant(8, NIC_NOISE_KERNEL, 1, 2, 0)) == WORKSPACE
    # 9. the workspace (the siblings' query), before the point descriptor and n_points
    two = _desc(num_crops=2)
    need = lib.nic_hash_batch_points_workspace_bytes(_ref(d), 2, 8, 64 * 4 * 9, _ref(_mlp()))
    assert need == 2 * 8 * REC * 4
    assert _joint(lib, d, groups=8, n_points=64 * 4 * 9, ws_bytes=need - 1) == WORKSPACE
    assert _joint(lib, two) == WORKSPACE and _joint(lib, d, n_points=-1) == WORKSPACE
    # 10. one crop; 11. n_points < 0 or >= 2^31; 12. n_points == 0: NIC_OK with no launch, nothing touched
    enough = 2 * cap * REC * 4
    for n_points in (130, 0, -1):
        assert _joint(lib, two, n_points=n_points, ws_bytes=enough) == SHAPE
    for n_points in (-1, -(1 << 40), 1 << 31):
        assert _joint(lib, d, n_points=n_points, ws_bytes=enough) == ARG
    need0 = lib.nic_hash_batch_points_workspace_bytes(_ref(d), 2, 0, 0, _ref(_mlp()))
    for flags in (0, 3):
        assert _joint(lib, d, n_points=0, ws_bytes=need0, flags=flags, lod=16, counts=16, order=16, quant=NicHashQuant(8, NIC_NOISE_KERNEL, 1, 2, 0)) == OK
    assert _joint(lib, d, n_points=0, ws_bytes=need0 - 1) == WORKSPACE


# ------------------------------------------------------------------------------------------------------------------ the units
def _kernel(text, name):
    k = text[text.index(f"{name}(const"):]
    return k[:k.index("\n}\n")]


def test_the_kernels_call_the_one_walk_and_restate_no_shared_helper():
    from neural_image_compression_v2_amd import _build
    import test_hashgrid_common_cpu as common
    assert GRAD_UNIT in _build.SOURCES and JOINT_UNIT in _build.SOURCES and WALK in _build.HEADERS and len(set(_build.SOURCES)) == len(_build.SOURCES)
    texts = {f: open(os.path.join(_build.CSRC, f)).read() for f in _build.SOURCES + [h for h in _build.HEADERS if h.endswith(".hpp")]}
    grad, joint = texts[GRAD_UNIT], texts[JOINT_UNIT]
    walk_helpers = ["decoder_dx_half", "point_grad", "point_walk", "point_walk_levels", "kept_axes", "store_point_grad", "lambda_passes"]
    device = ["lattice_fixed", "load_decoder", "decoder_forward_half", "decoder_train_half", "write_record", "persistent_grid", "strided_grid", "field_range",
              "field_loss_mul", "field_count"]
    for text in (grad, joint):
        for name in common.FUNCTIONS + list(common.OVERLOADS) + device + walk_helpers:
            assert not any(common._function_re(name).match(ln) for ln in text.splitlines()), name
        for name in common.STRUCTS + ["DecoderSmem", "TrainSmem", "TrainAcc", "SParams", "StoredSrc"]:
            assert not any(common._struct_re(name).match(ln) for ln in text.splitlines()), name
    for name in walk_helpers:                                             # the walk still has one definition
        found = sorted(f for f, t in texts.items() if any(common._function_re(name).match(ln) for ln in t.splitlines()))
        assert found == [WALK], (name, found)
    # the gradient-only kernel: the sibling's shape, the walk asked for d / d lambda, one writer per row, no atomics and no workspace
    assert "atomic" not in grad and "workspace" not in re.sub(r"//.*", "", grad)
    k = _kernel(grad, "hash_batch_points_grad_kernel")                     # the one kernel of the unit, its DLOD branch
    for call in ("load_decoder(", "DecoderSmem", "blockIdx.x / (unsigned)p.groups", "field_count(p.counts, b, p.n)", "field_loss_mul(p.loss_scale, n_b)",
                 "field_range(n_waves, lb, p.groups)", "ordered_row(order, n_b, live_lane ? pos : n_b - 1)", "point_lambda(lod_b, p.lod_uniform, row)",
                 "point_fixed<D>(p.d, points, row, t)", "encode_point<D, F, SRC, false, false, LOD>(src_b, t, row, lam, xrow)", "decoder_dx_half<KT>(",      # LOD is true under DLOD: the static_assert below
                 "point_walk<D, F, SRC, true, true, false>(src_b, t, row, lam, grow, gp, gl)",
                 "store_point_grad<D>(dpoints, row, kept_axes<D>(p.d, points, row), gp)", "dlod[row] = lambda_passes(lod_b, p.lod_uniform, row) ? gl : 0.0f"):
        assert call in k, call
    assert k.count("__syncthreads()") == 1 and k.index("__syncthreads()") < k.index("for (int64_t g")
    assert k.index("encode_point<") < k.index("decoder_dx_half<KT>(") < k.index("point_walk<") < k.index("if (live_lane) {") < k.index("dlod[row] =")
    assert "if constexpr (DLOD) dlod = p.dlod + (int64_t)b * p.n;" in k and k.index("if constexpr (DLOD) dlod =") < k.index("for (int64_t g")
    assert k.index("if constexpr (DLOD) {") < k.index("point_walk<") < k.index("} else {") < k.index(" point_grad<D, F, SRC, LOD>(")
    assert "static_assert(LOD || !DLOD" in k                               # a level of detail always on under DLOD
    assert "hash_batch_points_grad_kernel<D, F, SRC, 2, LOD, DLOD, P>" in grad and "hash_batch_points_grad_kernel<D, F, SRC, 1, LOD, DLOD, P>" in grad
    assert "launch<SRC, true, true>(p," in grad and "hash_batch_points_grad_lod_kernel" not in grad
    assert grad.index("hash_batch_points_grad_kernel(const") < grad.index("// ---- host side")
    # the training kernel: at the end of the device part, the sibling's shape, the walk after the scatter with the noise
    k = _kernel(joint, "hash_batch_points_joint_lod_kernel")
    for call in ("load_decoder(", "TrainSmem", "field_count(p.counts, b, p.n)", "field_loss_mul(p.loss_scale, n_b)", "field_range(n_waves, lb, p.groups)",
                 "ordered_row(order, n_b, live_lane ? pos : n_b - 1)", "point_lambda(lod_b, p.lod_uniform, row)", "point_fixed<D>(p.d, points, row, t)",
                 "encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, true>(src_b, t, row, lam, xrow)", "decoder_train_half<KT>(", "true, A);",
                 "scatter_point<D, F, true>(p.d, t, grad, p.fade, lam, live_lane, lane, grow)",
                 "point_walk<D, F, NIC_HASH_SRC_F32, true, true, NOISE>(src_b, t, row, lam, grow, gp, gl)",
                 "store_point_grad<D>(dpoints, row, kept_axes<D>(p.d, points, row), gp)", "dlod[row] = lambda_passes(lod_b, p.lod_uniform, row) ? gl : 0.0f",
                 "write_record<KT>(", "LodFieldSrc src_b{{p.d, p.tables + tab_off, p.noise, p.sample_base}, p.fade}"):
        assert call in k, call
    assert "atomic" not in k and k.count("__syncthreads()") == 1 and k.index("__syncthreads()") < k.index("for (int64_t g")
    assert k.index("decoder_train_half<KT>(") < k.index("scatter_point<D, F, true>(") < k.index("point_walk<") < k.index("dlod[row] =") < k.index("write_record<KT>(")
    assert "hash_batch_points_joint_lod_kernel<D, F, 2, NOISE>" in joint and "hash_batch_points_joint_lod_kernel<D, F, 1, NOISE>" in joint
    assert joint.index("hash_batch_points_joint_kernel(const") < joint.index("hash_batch_points_joint_lod_kernel(const") < joint.index("}  // namespace hbatch")
    e = joint[joint.index(f"int {JOINT}("):]
    e = e[:e.index("\n}\n")]
    assert "const KernelEndDrop end;" in e and e.index("open_batch_points(") < e.index("!lodp") < e.index("check_lod(desc, lodp)") < e.index("batch_points_step(p,")
    st = joint[joint.index("static int batch_points_step("):joint.index("}  // namespace hbatch")]     # the rest of the order, in the shared step
    assert st.index("flags & ~") < st.index("set_noise(") < st.index("NIC_E_WORKSPACE") < st.index("check_point_desc(desc)") < st.index("n_points == 0")
    assert st.index("n_points == 0") < st.index("kernel_end_mark((hipStream_t)stream);") < st.index("launch_batch_reduce(")
    e = grad[grad.index("static int batch_points_grad("):]                 # both gradient entries sit on it
    assert e.index("!lodp") < e.index("set_point_source(p, src)") < e.index("check_lod(desc, lodp)") < e.index("(dy != nullptr) == (target != nullptr)")
    for name, last in ((GRAD, "dlod, true, stream);"), ("nic_hash_batch_points_grad", "nullptr, false, stream);")):
        w = grad[grad.index(f"int {name}("):]
        assert "return batch_points_grad(" in w[:w.index("\n}\n")] and last in w[:w.index("\n}\n")], name


# ------------------------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("case", CASES, ids=str)
def test_every_fields_lod_holds_every_kind_of_row(case):
    bi = batch_inputs(case)
    fade = bi.fade
    assert len(bi.fields) == B and bi.fields[0].lod is inputs(*case).lod and bi.fields[0].table is inputs(*case).table
    assert (bi.geo.width > 32) == (case[2] == 5)                          # both KT
    for b, f in enumerate(bi.fields):
        a_raw, ramp, passes = ramp_f32(fade, f.lod, 0.0, N)
        wave0 = a_raw[:64]
        for l in range(len(fade)):                                        # a_raw == 1 and a_raw == 0 for every level, in wave 0
            assert (wave0[:, l] == 1).any() and (wave0[:, l] == 0).any(), (b, l)
        with np.errstate(invalid="ignore"):
            vals = f.lod[:64]
            for v in (0.0, -1.0, 32.0, 40.0):
                assert (vals == np.float32(v)).any(), (b, v)
            assert np.isnan(vals).any() and int((~passes).sum()) == 4
        assert ramp[f.lod == 0].any()                                     # lambda_raw == 0 passes a gradient through
        assert (a_raw[64:128] <= 0).all() and not ramp[64:128].any()       # one whole wave with every level off
        assert list(f.lod[128:]) == [2.5, 2.5]
        assert ramp[list(G.OUTSIDE_ROWS)].any(axis=1).all()                # outside points that have a level on the ramp
        moved = T.clamp_points(bi.tgeo, f.points.numpy())[1]
        assert moved[list(G.OUTSIDE_ROWS)].any(axis=1).all() and moved.any(axis=1).sum() == len(G.OUTSIDE_ROWS)
        if b:                                                             # the kink rows sit at other lanes than field 0's
            k = MOVED_TO[b]
            assert np.array_equal(f.lod[k:k + KINK_ROWS], bi.fields[0].lod[:KINK_ROWS], equal_nan=True)
            assert np.array_equal(f.lod[:KINK_ROWS], bi.fields[0].lod[k:k + KINK_ROWS]) and np.array_equal(f.lod[64:], bi.fields[0].lod[64:])
            assert not torch.equal(f.table, bi.fields[0].table) and not torch.equal(f.params[0], bi.fields[0].params[0])
        for counts in COUNTS:                                             # every count a field is launched at has a gradient to compare
            n_b = count_of(counts, b)
            if n_b:
                for mode in MODES:
                    ref = field_reference(case, b, n_b, mode)
                    assert float(ref.dpoints.abs().max()) > 0 and bool(torch.isfinite(ref.dlod).all()), (b, n_b, mode)
                    assert n_b == 1 or float(ref.dlod.abs().max()) >= 1e-3, (b, n_b, mode)


# ------------------------------------------------------------------------------------------------------------------ teeth
def _dlod_from(ref, dW):
    return -(dW * torch.from_numpy(ref.ramp)).sum(dim=1) * torch.from_numpy(ref.passes)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_teeth_five_mistakes_are_each_seen_on_these_inputs(case):
    bi = batch_inputs(case)
    moved = {}
    for b in range(B):
        f, nxt = bi.fields[b], bi.fields[(b + 1) % B]
        ref = field_reference(case, b, N, "point")
        lod, u = field_lod(bi, b, "point")

        def step(table=f.table, params=f.params, lod=lod):
            return reference_step(bi.tgeo, table, params, f.points, bi.fade, lod, u, target=f.target, loss_scale=LOSS_SCALE)
        # reading the neighbour field's lod / table / decoder
        moved[("neighbour's lod", b)] = rel(step(lod=field_lod(bi, (b + 1) % B, "point")[0]).dlod, ref.dlod)
        moved[("neighbour's table", b)] = rel(step(table=nxt.table).dlod, ref.dlod)
        moved[("neighbour's decoder", b)] = rel(step(params=nxt.params).dlod, ref.dlod)
        # storing dlod at the position in the order instead of at the row; scaling by the padded N instead of n_b
        for counts in COUNTS:
            n_b = count_of(counts, b)
            if n_b < 2:
                continue
            r = field_reference(case, b, n_b, "point")
            perm = permutation(b, n_b)
            assert not torch.equal(perm, torch.arange(n_b))
            key = ("dlod by position", b)
            moved[key] = min(moved.get(key, float("inf")), rel(r.dlod[perm], r.dlod))
            if n_b < N:
                key = ("scaled by the padded N", b)
                moved[key] = min(moved.get(key, float("inf")), rel(r.dlod * (n_b / N), r.dlod))
        # dropping the noise term; keying the noise by position instead of by row (under the fixed permutation)
        for bits in (4, 8):
            r = field_reference(case, b, N, "point", bits)
            term = S.noise_term(bi.tgeo, r.drow, r.nz)
            moved[(f"no noise term, b = {bits}", b)] = rel(_dlod_from(r, r.dW - term), r.dlod)
            perm = permutation(b, N)
            nz_pos = torch.empty_like(r.nz)
            nz_pos[perm] = r.nz                                           # row order[pos] gets the noise of key sample_base + pos
            moved[(f"noise keyed by position, b = {bits}", b)] = rel(_dlod_from(r, r.dW - term + S.noise_term(bi.tgeo, r.drow, nz_pos)), r.dlod)
    for name in sorted({k[0] for k in moved}):
        worst = max(v for k, v in moved.items() if k[0] == name)
        least = min(v for k, v in moved.items() if k[0] == name)
        print(f"{case} {name}: dlod moves by {least / TOL_G:.1f} .. {worst / TOL_G:.1f} x TOL_G over the fields")
        assert worst > TOL_G, (name, worst)                               # some field sees it ...
        assert least > TOL_G, (name, least)                               # ... and on these inputs every field does


# ------------------------------------------------------------------------------------------------------------------ the Python surface
def test_the_wrappers_refuse_before_a_device():
    from neural_image_compression_v2_amd import hashgrid
    geo = P._geo()
    tables, params = torch.zeros(3, *geo.table_shape()), P._params(geo)
    pts, target, gm = torch.zeros(3, 7, 2), torch.zeros(3, 7, 3), [torch.zeros_like(p) for p in params]

    def pg(data=tables, points=pts, params=params, dy=target, **kw):
        return hashgrid.hash_batch_points_grad_lod(geo, data, points, params, dy=dy, **kw)

    def fb(tables=tables, points=pts, params=params, target=target, gm=gm, **kw):
        return hashgrid.hash_batch_forward_backward_points_grad_lod(geo, tables, points, params, target, gm, **kw)
    for call in (pg, fb):
        with pytest.raises(TypeError, match="dlod"):
            call(dlod=[[0.0] * 7] * 3)
        for bad in (torch.zeros(7), torch.zeros(2, 7), torch.zeros(3, 8), torch.zeros(3, 7, 1), torch.zeros(3, 7, dtype=torch.float64),
                    torch.zeros(7, 3).transpose(0, 1)):
            with pytest.raises(ValueError, match="dlod"):
                call(dlod=bad)
        for bad in (torch.zeros(7, 2), torch.zeros(3, 7, 3), torch.zeros(3, 7, 2, dtype=torch.float64), torch.zeros(3, 2, 7).transpose(1, 2)):
            with pytest.raises(ValueError, match="dpoints"):
                call(dpoints=bad)
        for bad in BAD_LOD_TENSORS:
            with pytest.raises(ValueError, match="lod"):
                call(lod=bad)
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="lod_uniform"):
                call(lod_uniform=bad)
        for bad in ((1.0,) * 3, (1.0, 1.0, -1.0, 1.0), "abcd"):
            with pytest.raises(ValueError, match="fade"):
                call(fade=bad)
        for bad in P.BAD_POINTS:
            with pytest.raises(ValueError, match="points"):
                call(points=bad)
        for bad in P.BAD_COUNTS:
            with pytest.raises(ValueError, match="counts"):
                call(counts=bad)
        for bad in P._bad_orders():
            with pytest.raises(ValueError, match="order"):
                call(order=bad)
        # with everything shaped right the refusal is the device's: nothing was launched
        for kw in (dict(), dict(dlod=torch.zeros(3, 7), dpoints=torch.zeros(3, 7, 2)), dict(lod=torch.zeros(3, 7), counts=(7, 0, 3),
                                                                                           order=torch.zeros(3, 7, dtype=torch.int32)), dict(lod=torch.zeros(7))):
            with pytest.raises(RuntimeError, match="HIP device"):
                call(**kw)
    with pytest.raises(ValueError, match="exactly one of dy and target"):
        pg(target=target)
    with pytest.raises(ValueError, match="exactly one of dy and target"):
        pg(dy=None)
    with pytest.raises(ValueError, match="num_bits"):
        pg(num_bits=4)
    with pytest.raises(ValueError, match="tables"):
        fb(tables=tables[0])
    with pytest.raises(ValueError, match="target"):
        fb(target=torch.zeros(3, 8, 3))


def test_the_class_refuses_on_the_host():
    f = P._bare()
    before = dict(f.__dict__)
    pts, target, lod = torch.zeros(3, 7, 2), torch.zeros(3, 7, 3), torch.zeros(3, 7)
    for bad in P.BAD_POINTS:
        for call in (lambda: f.point_gradient_lod(bad, lod, dy=target), lambda: f.train_points_grad_lod(bad, target, lod), lambda: f.jacobian_lod(bad, lod),
                     lambda: f.train_points_differentiable_lod(bad, lod.clone().requires_grad_(True), target),
                     lambda: f.query_differentiable_lod(bad, lod.clone().requires_grad_(True))):
            with pytest.raises(ValueError, match="points"):
                call()
    # lod is required, and is a float or a [N] / [B, N] tensor
    for call in (lambda l: f.point_gradient_lod(pts, l, dy=target), lambda l: f.train_points_grad_lod(pts, target, l)):
        with pytest.raises(ValueError, match="lod"):
            call(None)
        for bad in BAD_LOD_TENSORS + BAD_LOD_VALUES:
            with pytest.raises(ValueError, match="lod"):
                call(bad)
    with pytest.raises(ValueError, match="lod"):
        f.jacobian_lod(pts, None)
    with pytest.raises(ValueError, match="lod"):
        f.query_differentiable_lod(pts.clone().requires_grad_(True), None)
    with pytest.raises(ValueError, match="exactly one of dy and target"):
        f.point_gradient_lod(pts, lod)
    with pytest.raises(ValueError, match="exactly one of dy and target"):
        f.point_gradient_lod(pts, lod, dy=target, target=target)
    with pytest.raises(ValueError, match="dy"):
        f.point_gradient_lod(pts, lod, dy=torch.zeros(3, 8, 3))
    with pytest.raises(ValueError, match="target"):
        f.train_points_grad_lod(pts, torch.zeros(3, 8, 3), lod)
    for bad in P.BAD_COUNTS:
        with pytest.raises(ValueError, match="counts"):
            f.point_gradient_lod(pts, lod, dy=target, counts=bad)
        with pytest.raises(ValueError, match="counts"):
            f.train_points_grad_lod(pts, target, lod, counts=bad)
    for bad in P._bad_orders() + ("morton", "Cell", ""):
        with pytest.raises(ValueError, match="order"):
            f.point_gradient_lod(pts, lod, target=target, order=bad)
        with pytest.raises(ValueError, match="order"):
            f.train_points_grad_lod(pts, target, lod, order=bad)
    # the two tensors
    with pytest.raises(TypeError, match="dlod"):
        f.train_points_grad_lod(pts, target, lod, dlod=[[0.0] * 7] * 3)
    for bad in (torch.zeros(7), torch.zeros(3, 8), torch.zeros(2, 7), torch.zeros(3, 7, dtype=torch.float64), torch.zeros(7, 3).transpose(0, 1)):
        with pytest.raises(ValueError, match="dlod"):
            f.train_points_grad_lod(pts, target, lod, dlod=bad)
    for bad in (torch.zeros(7, 2), torch.zeros(3, 7, 3), torch.zeros(3, 7, 2, dtype=torch.float64)):
        with pytest.raises(ValueError, match="dpoints"):
            f.train_points_grad_lod(pts, target, lod, dpoints=bad)
    with pytest.raises(TypeError, match="dlod"):
        f.train_points_differentiable_lod(pts.clone().requires_grad_(True), lod, target, dlod=torch.zeros(3, 7))
    with pytest.raises(TypeError, match="dpoints"):
        f.train_points_differentiable_lod(pts, lod.clone().requires_grad_(True), target, dpoints=torch.zeros(3, 7, 2))
    # precision= is refused as on the siblings: these calls have no 16-bit form and no such parameter
    for call in (lambda **kw: f.point_gradient_lod(pts, lod, dy=target, **kw), lambda **kw: f.train_points_grad_lod(pts, target, lod, **kw),
                 lambda **kw: f.jacobian_lod(pts, lod, **kw), lambda **kw: f.query_differentiable_lod(pts, lod, **kw),
                 lambda **kw: f.train_points_differentiable_lod(pts.clone().requires_grad_(True), lod, target, **kw)):
        with pytest.raises(TypeError, match="precision"):
            call(precision="bf16")
    with pytest.raises(ValueError, match="noise"):
        f.train_points_grad_lod(pts, target, lod, noise=True)             # no codec: no noise
    # everything right: the refusal is the device's
    for counts in (None, (7, 0, 3)):
        for order in (None, "cell", torch.zeros(3, 7, dtype=torch.int32)):
            for l in (0.5, torch.zeros(7), lod, torch.tensor(1.5)):
                with pytest.raises(RuntimeError, match="HIP device"):
                    f.point_gradient_lod(pts, l, dy=target, counts=counts, order=order)
                with pytest.raises(RuntimeError, match="HIP device"):
                    f.train_points_grad_lod(pts, target, l, counts=counts, order=order, dpoints=torch.zeros(3, 7, 2), dlod=torch.zeros(3, 7))
    with pytest.raises(RuntimeError, match="HIP device"):
        f.jacobian_lod(torch.zeros(7, 2), lod)
    with pytest.raises(RuntimeError, match="HIP device"):
        f.query_differentiable_lod(pts, torch.tensor(1.5, requires_grad=True))
    with pytest.raises(RuntimeError, match="HIP device"):
        f.train_points_differentiable_lod(pts.clone().requires_grad_(True), lod.clone().requires_grad_(True), target)
    assert f.__dict__.keys() == before.keys() and all(f.__dict__[k] is before[k] for k in before)       # nothing was set on the way to a refusal
    # a decode-only batch: the training calls refuse before they look at an argument; the gradient reads the stored tables
    g = P._bare(decode_only=True, num_bits=8, frozen=True)
    with pytest.raises(RuntimeError, match="decode-only"):
        g.train_points_grad_lod(None, None, None)
    with pytest.raises(RuntimeError, match="decode-only"):
        g.train_points_differentiable_lod(pts.clone().requires_grad_(True), lod, target)
    with pytest.raises(RuntimeError, match="HIP device"):
        g.point_gradient_lod(pts, lod, dy=target)
    # a bit depth per level has no batch at all
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch
    with pytest.raises(NotImplementedError, match="bit depth per level"):
        HashGridFieldBatch(3, (40, 36), levels=4, num_bits=(8, 6, 5, 4))
