"""CPU-only tests of the batch's level of detail per point (run with -m "not gpu"): nic_hash_batch_forward_points_lod and
nic_hash_batch_forward_backward_points_lod are exported, declared in the companion header include/nicv2_hip_ext.h alone and mirrored in
_lib.EXT_SIGNATURES; every argument error is decided on the host in the documented order (fake pointers and refusals only: nothing launches);
the wrappers and ``HashGridFieldBatch.query_lod`` / ``resample_lod`` / ``decode_mip`` / ``train_points_lod`` / ``fit_points_lod`` / ``fit_mips``
refuse before a device is touched and set nothing on the way; the two kernels sit in the batch unit outside the slices the older tests read
and restate no shared helper.

Teeth, with the float64 reference alone (oracle/hashgrid_train_ref.py) on the inputs tests/test_gpu_hashgrid_batch_lod.py uses: a step that
ignores ``lod``, one that reads the neighbour field's ``lod``, and one that reads ``lod`` at the position in the order instead of at the row
each move a compared quantity by more than ``C.TEETH`` x its bound on every shape (smallest movements, x the bound, worst shape and field: 1.1e4,
1.1e4 and 1.1e4); and the inputs reach a level of weight 1, of weight 0, of
a weight strictly between, and a level that a whole wave skips.

``lod_of`` / ``MODES`` / ``lod_reference`` / ``permutation`` are shared with the GPU file: both sides see the same bytes."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import hashgrid_train_ref as T
from tests import test_hashgrid_batch_points_cpu as P
from tests import test_hashgrid_train_ref_cpu as C
from tests.test_hashgrid_batch_points_cpu import ARG, NULL, OK, SHAPE, UNSUP, WORKSPACE, REC, _cap, _desc, _mlp, _ref, lib  # noqa: F401

FWD, TRAIN = "nic_hash_batch_forward_points_lod", "nic_hash_batch_forward_backward_points_lod"
ARGS = {FWD: ["desc", "n_fields", "groups_per_field", "lodp", "src", "points", "lod", "n_points", "mlp", "y", "stream"],
        TRAIN: ["desc", "n_fields", "groups_per_field", "lodp", "quant", "tables", "points", "lod", "n_points", "counts", "order", "mlp", "target", "loss_scale",
                "table_grads", "mlp_grads", "loss", "y", "flags", "workspace", "workspace_bytes", "stream"]}
PTR = ctypes.c_void_p
N, B = P.N, C.N_FIELDS

# ------------------------------------------------------------------------------------------------------------------ shared with the GPU file
# mode -> what the launch gets as (fade, per-point lod or None, lod_uniform), from the field's own inputs
#   point     the per-point lod of tests/test_hashgrid_train_ref_cpu.py (NaN, a negative, 40 and values up to max(fade) + 1.5), default fade
#   uniform   one launch-wide 1.25
#   skip      one launch-wide lambda just past (the largest fade below max(fade)) + 1: every level but the coarsest (and one of its resolution)
#             is off for every lane, so whole waves skip them, and the coarsest keeps a weight strictly between 0 and 1
#   off       one launch-wide 40 (clamped to 32): every level is off
#   boundary  a fade that is NOT monotone - level BOUNDARY_LEVEL fades at once, the others never - under a launch-wide 1.5: at F = 4 that
#             level opens a generator block of 16 noise columns, the whole wave skips it, and the next live level has to make the block
MODES = ("point", "uniform", "skip", "off", "boundary")
BOUNDARY_LEVEL = 4


def skip_lambda(fade):
    below = [v for v in fade if v < max(fade)]              # two coarse levels may share a resolution, and so the largest fade
    top = max(below) if below else max(fade) - 0.5
    return float(np.float32(top + 1.0 + 2.0 ** -6))


def lod_of(shape, b, mode):
    """(fade, lod [N] float32 numpy or None, lod_uniform) of field b of a shape in ``mode``"""
    inp = C.inputs(*shape, b)
    if mode == "point":
        return inp.fade, inp.lod, 0.0
    if mode == "uniform":
        return inp.fade, None, 1.25
    if mode == "skip":
        return inp.fade, None, skip_lambda(inp.fade)
    if mode == "off":
        return inp.fade, None, 40.0
    if mode == "boundary":
        return tuple(0.0 if l == BOUNDARY_LEVEL else 8.0 for l in range(shape[2])), None, 1.5
    raise KeyError(mode)


def lod_reference(shape, b, n_b, noisy, mode="point", base=C.NOISE_BASE, loss_scale=C.LOSS_SCALE):
    """``T.step`` of field b on its first n_b points with ITS level of detail, computed once and shared (read-only)"""
    return _lod_reference(tuple(int(v) for v in shape), int(b), int(n_b), bool(noisy), str(mode), int(base), float(loss_scale))


@functools.lru_cache(maxsize=None)
def _lod_reference(shape, b, n_b, noisy, mode, base, loss_scale):
    f = P.field_inputs(shape, b)
    fade, lod, u = lod_of(shape, b, mode)
    return T.step(f.geo, f.table_q if noisy else f.table, f.params, f.target[:n_b], points=f.points[:n_b], loss_scale=loss_scale,
                  noise_key=C.noise_key(base=base) if noisy else None, lod=(fade, None if lod is None else lod[:n_b], u))


def permutation(b, n_b):
    """the permutation of field b's own rows the GPU file's "perm" order uses"""
    return torch.randperm(n_b, generator=torch.Generator().manual_seed(11 + b))


# ------------------------------------------------------------------------------------------------------------------ the C entries
def _lod(fade=(1.0,) * 8, uniform=0.0, reserved=0):
    from neural_image_compression_v2_amd._lib import NicHashLod
    lp = NicHashLod()
    for l, v in enumerate(fade):
        lp.fade[l] = v
    lp.lod_uniform, lp.reserved = uniform, reserved
    return lp


def _src(kind=0, bits=0, data=16):
    from neural_image_compression_v2_amd._lib import NicHashSource
    return NicHashSource(kind, bits, data)


def _fwd(lib, d, n_fields=2, groups=0, lodp="default", src="default", points=16, lod=0, n_points=130, m="default", y=16):
    """the return code of the forward entry with dummy pointers; only calls a host check refuses, or n_points == 0, are made"""
    lodp = _lod() if lodp == "default" else lodp
    src = _src() if src == "default" else src
    m = _mlp() if m == "default" else m
    return lib.nic_hash_batch_forward_points_lod(_ref(d), n_fields, groups, _ref(lodp), _ref(src), PTR(points), PTR(lod), n_points, _ref(m), PTR(y), None)


def _train(lib, d, n_fields=2, groups=0, lodp="default", quant=None, tables=16, points=16, lod=0, n_points=130, counts=0, order=0, m="default", target=16,
           table_grads=16, grads="default", loss=16, y=16, flags=0, ws=16, ws_bytes=16):
    """the return code of the training entry; with the 16-byte workspace an accepted call stops at the workspace check"""
    from neural_image_compression_v2_amd._lib import NicMlpGrads
    lodp = _lod() if lodp == "default" else lodp
    m = _mlp() if m == "default" else m
    grads = NicMlpGrads() if grads == "default" else grads
    return lib.nic_hash_batch_forward_backward_points_lod(_ref(d), n_fields, groups, _ref(lodp), _ref(quant), PTR(tables), PTR(points), PTR(lod), n_points,
                                                          PTR(counts), PTR(order), _ref(m), PTR(target), 1.0, PTR(table_grads), _ref(grads), PTR(loss), PTR(y),
                                                          flags, PTR(ws), ws_bytes, None)


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
    assert _lib.EXT_SIGNATURES[FWD][1][3]._type_ is _lib.NicHashLod and _lib.EXT_SIGNATURES[TRAIN][1][3]._type_ is _lib.NicHashLod
    declared = set(re.findall(r"\b(nic_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", ext, flags=re.S)))
    assert declared == set(_lib.EXT_SIGNATURES) and len(_lib.SIGNATURES) == 86 and _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version()
    for name in ("hash_batch_forward_points_lod", "hash_batch_forward_backward_points_lod"):
        assert getattr(pkg, name) is getattr(hashgrid, name)
    assert list(inspect.signature(hashgrid.hash_batch_forward_points_lod).parameters) == [
        "geo", "data", "points", "params", "lod", "lod_uniform", "fade", "kind", "num_bits", "groups_per_field", "out"]
    assert list(inspect.signature(hashgrid.hash_batch_forward_backward_points_lod).parameters) == [
        "geo", "tables", "points", "params", "target", "mlp_grads", "lod", "lod_uniform", "fade", "table_grads", "order", "counts", "loss", "loss_scale",
        "want_y", "quant", "add_grads", "add_loss", "groups_per_field"]
    cls = hashgrid.HashGridFieldBatch
    assert list(inspect.signature(cls.query_lod).parameters) == ["self", "points", "lod", "precision"]
    assert list(inspect.signature(cls.resample_lod).parameters) == ["self", "size", "lod", "tile", "precision"]
    assert inspect.signature(cls.resample_lod).parameters["lod"].default == "auto"
    assert list(inspect.signature(cls.decode_mip).parameters) == ["self", "m", "tile"] and inspect.signature(cls.decode_mip).parameters["tile"].default == 1024
    assert list(inspect.signature(cls.train_points_lod).parameters) == ["self", "points", "target", "lod", "counts", "accumulate", "scale", "step", "noise", "order"]
    assert list(inspect.signature(cls.fit_points_lod).parameters) == ["self", "points", "target", "epochs", "lod", "counts", "order", "freeze_at"]
    sig = inspect.signature(cls.fit_mips).parameters
    assert list(sig) == ["self", "targets", "epochs", "mips", "order", "freeze_at"] and sig["mips"].default == 2 and sig["order"].default == "cell"
    assert sig["freeze_at"].default == 0.95 and isinstance(cls.lod_fade, property) and cls.lod_fade.fset is not None
    assert "4.7.20" in cls.__doc__ and "query_lod" in cls.__doc__


def _bad_lods():
    inf, nan = float("inf"), float("nan")
    return [_lod((1.0, -1.0)), _lod((-1e-30,)), _lod((0.0,) * 7 + (nan,)), _lod((inf,)), _lod((0.0, -inf)), _lod(uniform=nan), _lod(uniform=inf),
            _lod(uniform=-inf), _lod(reserved=1), _lod(reserved=-1)]


def test_forward_argument_errors_in_the_documented_order(lib):
    d = _desc()
    assert _fwd(lib, d, n_points=0) == OK                                 # every check passes; no points: no launch
    # 1. null desc / mlp, whatever else is wrong
    assert _fwd(lib, None) == NULL and _fwd(lib, d, m=None) == NULL and _fwd(lib, None, n_fields=0, groups=3, lodp=None, n_points=-1) == NULL
    # 2. the fused set, then the descriptor of a point source: before n_fields, the groups and every pointer
    bad = _desc()
    bad.flags = 1
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(resolutions=(16,) * 9, features=8), UNSUP), (_desc(num_crops=2), SHAPE),
                       (big, ARG)]:
        assert _fwd(lib, desc) == want and _fwd(lib, desc, n_fields=0, groups=3, lodp=None, src=None, y=0, n_points=-1) == want
    assert _fwd(lib, d, m=_mlp(5, 5)) == UNSUP
    # 3. n_fields
    for n in (0, -1, 65536):
        assert _fwd(lib, d, n_fields=n) == ARG and _fwd(lib, d, n_fields=n, groups=3, lodp=None, n_points=-1) == ARG
    # 4. groups_per_field on ceil(n_points / 64) wave items; no points count as one item
    for g in (-8, 1, 12, 1 << 20):
        assert _fwd(lib, d, groups=g) == ARG and _fwd(lib, d, groups=g, lodp=None, y=0, n_points=-1) == ARG
    assert _fwd(lib, d, groups=16, n_points=130) == ARG and _fwd(lib, d, groups=16, n_points=0) == ARG and _fwd(lib, d, groups=8, n_points=0) == OK
    # 5. null pointers - lodp with the others (lod may be null) - before the nic_hash_lod, the source and n_points
    for kw in (dict(lodp=None), dict(src=None), dict(src=_src(data=0)), dict(points=0), dict(y=0), dict(m=_mlp(3, 2))):
        assert _fwd(lib, d, **kw) == NULL and _fwd(lib, d, n_points=-1, **kw) == NULL, kw
        if "lodp" not in kw:
            assert _fwd(lib, d, lodp=_lod(reserved=1), **kw) == NULL, kw
    assert _fwd(lib, d, lod=16, n_points=0) == OK
    # 6. the nic_hash_lod, right after the pointers: before the source and n_points
    for lp in _bad_lods():
        assert _fwd(lib, d, lodp=lp) == ARG and _fwd(lib, d, lodp=lp, src=_src(kind=7), n_points=-1) == ARG
    assert _fwd(lib, _desc(resolutions=(16,) * 4), lodp=_lod((0.0,) * 4 + (-1.0, float("nan"))), n_points=0) == OK       # fade past the levels is ignored
    # 7. the source: kind, num_bits, alignment
    for src in (_src(kind=7), _src(kind=0, bits=4), _src(kind=1, bits=0), _src(kind=1, bits=9), _src(kind=2, bits=4, data=18)):
        assert _fwd(lib, d, src=src) == ARG and _fwd(lib, d, src=src, n_points=-1) == ARG
    for src in (_src(kind=1, bits=8), _src(kind=2, bits=4)):
        assert _fwd(lib, d, src=src, n_points=0) == OK
    # 8. n_points < 0; 9. n_points == 0 is NIC_OK without a launch (the pointers are fakes: a launch would fault)
    for n_points in (-1, -(1 << 40)):
        assert _fwd(lib, d, n_points=n_points) == ARG
    for desc in (d, _desc(dim=3, resolutions=(4, 6, 9, 12), features=1, s_max=12, extent=(12, 10, 9)), _desc(features=8)):
        assert _fwd(lib, desc, n_points=0) == OK


def test_training_argument_errors_in_the_documented_order(lib):
    from neural_image_compression_v2_amd._lib import NicHashQuant, NIC_NOISE_KERNEL
    d = _desc()
    cap = _cap(lib)
    assert _train(lib, d) == WORKSPACE                                   # every check up to the workspace passes
    # 1. null desc / mlp
    assert _train(lib, None) == NULL and _train(lib, d, m=None) == NULL and _train(lib, None, n_fields=0, groups=3, lodp=None, tables=0, n_points=-1) == NULL
    # 2. the fused set (then 256 S_max < 2^30)
    bad = _desc()
    bad.flags = 1
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(log2_table=9), ARG), (_desc(num_crops=0), SHAPE), (_desc(resolutions=(16,) * 9, features=8), UNSUP),
                       (big, ARG)]:
        assert _train(lib, desc) == want and _train(lib, desc, n_fields=0, groups=3, lodp=None, tables=0, n_points=-1) == want
    # 3. n_fields; 4. groups_per_field
    for n in (0, -1, 65536):
        assert _train(lib, d, n_fields=n) == ARG and _train(lib, d, n_fields=n, groups=3, lodp=None, n_points=-1) == ARG
    for g in (-8, 1, 12, 1 << 20):
        assert _train(lib, d, groups=g) == ARG and _train(lib, d, groups=g, lodp=None, tables=0, n_points=-1) == ARG
    assert _train(lib, d, groups=16, n_points=130) == ARG and _train(lib, d, groups=8, n_points=130) == WORKSPACE
    # 5. null pointers: lodp with the others (lod, counts, order, table_grads and y may be null), before the nic_hash_lod and the flags
    for kw in (dict(lodp=None), dict(tables=0), dict(points=0), dict(target=0), dict(grads=None), dict(loss=0), dict(ws=0), dict(m=_mlp(3, 2))):
        assert _train(lib, d, **kw) == NULL and _train(lib, d, flags=4, n_points=-1, **kw) == NULL, kw
        if "lodp" not in kw:
            assert _train(lib, d, lodp=_lod(uniform=float("nan")), **kw) == NULL, kw
    assert _train(lib, d, table_grads=0, y=0, lod=0) == WORKSPACE and _train(lib, d, lod=16, counts=16, order=16) == WORKSPACE
    # 6. the nic_hash_lod, right after the pointers: before the flags, the quantiser, the workspace and n_points
    for lp in _bad_lods():
        assert _train(lib, d, lodp=lp) == ARG
        assert _train(lib, d, lodp=lp, flags=4, quant=NicHashQuant(8, 1, 1, 2, 0), n_points=-1) == ARG
    # 7. flags; 8. the quantiser
    for flags in (4, 8, -1):
        assert _train(lib, d, flags=flags) == ARG and _train(lib, d, flags=flags, quant=NicHashQuant(8, 1, 1, 2, 0)) == ARG
    assert _train(lib, d, flags=3) == WORKSPACE
    assert _train(lib, d, quant=NicHashQuant(0, NIC_NOISE_KERNEL, 1, 2, 0)) == ARG and _train(lib, d, quant=NicHashQuant(8, 1, 1, 2, 0)) == UNSUP
    assert _train(lib, d, quant=NicHashQuant(8, NIC_NOISE_KERNEL, 1, 2, 0)) == WORKSPACE
    # 9. the workspace (the sibling's query), before the point descriptor and n_points
    two = _desc(num_crops=2)
    need = lib.nic_hash_batch_points_workspace_bytes(_ref(d), 2, 8, 64 * 4 * 9, _ref(_mlp()))
    assert need == 2 * 8 * REC * 4
    assert _train(lib, d, groups=8, n_points=64 * 4 * 9, ws_bytes=need - 1) == WORKSPACE
    assert _train(lib, two) == WORKSPACE and _train(lib, d, n_points=-1) == WORKSPACE
    # 10. one crop; 11. n_points < 0 or >= 2^31; 12. n_points == 0: NIC_OK with no launch
    enough = 2 * cap * REC * 4
    for n_points in (130, 0, -1):
        assert _train(lib, two, n_points=n_points, ws_bytes=enough) == SHAPE
    for n_points in (-1, -(1 << 40), 1 << 31):
        assert _train(lib, d, n_points=n_points, ws_bytes=enough) == ARG
    need0 = lib.nic_hash_batch_points_workspace_bytes(_ref(d), 2, 0, 0, _ref(_mlp()))
    for flags in (0, 3):
        assert _train(lib, d, n_points=0, ws_bytes=need0, flags=flags, lod=16, counts=16, order=16, quant=NicHashQuant(8, NIC_NOISE_KERNEL, 1, 2, 0)) == OK
    assert _train(lib, d, n_points=0, ws_bytes=need0 - 1) == WORKSPACE


# ------------------------------------------------------------------------------------------------------------------ the unit
def test_the_kernels_are_in_the_batch_unit_outside_the_older_slices_and_restate_no_shared_helper():
    from neural_image_compression_v2_amd import _build
    import test_hashgrid_common_cpu as common
    unit = open(os.path.join(_build.CSRC, P.UNIT)).read()
    shared = open(os.path.join(_build.CSRC, P.SHARED)).read()
    device = ["lattice_fixed", "load_decoder", "decoder_forward_half", "decoder_train_half", "write_record", "persistent_grid", "strided_grid", "field_range",
              "field_loss_mul", "field_count"]
    for name in common.FUNCTIONS + list(common.OVERLOADS) + device:
        assert not any(common._function_re(name).match(ln) for ln in unit.splitlines()), name
    for name in common.STRUCTS + ["DecoderSmem", "TrainSmem", "TrainAcc", "SParams", "StoredSrc"]:
        assert not any(common._struct_re(name).match(ln) for ln in unit.splitlines()), name
    assert any(common._struct_re("SParams").match(ln) for ln in shared.splitlines())
    # the older tests read hash_batch_points_kernel(const .. "// ---- forward only" and hash_batch_reduce_kernel( .. "// ---- host side"
    marks = [unit.index("hash_batch_points_kernel(const"), unit.index("// ---- forward only"), unit.index("hash_batch_decode_kernel(const"),
             unit.index("// ---- with a level of detail per point"), unit.index("hash_batch_points_lod_kernel(const"),
             unit.index("hash_batch_decode_lod_kernel(const"), unit.index("void __launch_bounds__(256) hash_batch_reduce_kernel("), unit.index("// ---- host side")]
    assert marks == sorted(marks)
    older = unit[marks[0]:marks[1]] + unit[marks[6]:marks[7]]
    assert "_lod" not in older and "fade" not in older and "point_lambda" not in older
    # the older kernels keep their calls
    assert "encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, false>(src_b, t, row, 0.f, xrow)" in unit[marks[0]:marks[1]]
    assert "encode_point<D, F, SRC, false, false, false>(src_b, t, row, 0.f, xrow)" in unit[marks[2]:marks[3]]
    # the new ones: the siblings' shape around the LOD level loop and scatter
    k = unit[marks[4]:marks[5]]
    for call in ("load_decoder(", "field_count(p.counts, b, p.n)", "field_loss_mul(p.loss_scale, n_b)", "field_range(n_waves, lb, p.groups)", "ordered_row(order, n_b,",
                 "point_lambda(lod_b, p.lod_uniform, row)", "point_fixed<D>(p.d, points, row, t)",
                 "encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, true>(src_b, t, row, lam, xrow)", "decoder_train_half<KT>(",
                 "scatter_point<D, F, true>(p.d, t, grad, p.fade, lam, live_lane, lane,", "write_record<KT>(", "TrainSmem"):
        assert call in k, call
    assert k.count("__syncthreads()") == 1 and k.index("__syncthreads()") < k.index("for (int64_t g")
    assert k.index("ordered_row(order, n_b,") < k.index("point_lambda(lod_b,") < k.index("encode_point<") < k.index("scatter_point<D, F, true>(")
    f = unit[marks[5]:marks[6]]
    for call in ("load_decoder(", "field_range(p.n_items, lb, p.groups)", "point_fixed<D>(p.d, points, row, t)",
                 "encode_point<D, F, SRC, false, false, true>(src_b, t, row, point_lambda(lod_b, p.lod_uniform, row), xrow)", "decoder_forward_half(", "DecoderSmem"):
        assert call in f, call
    assert "atomic" not in f and f.count("__syncthreads()") == 1
    assert "hash_batch_points_lod_kernel<D, F, 2, NOISE>" in unit and "hash_batch_points_lod_kernel<D, F, 1, NOISE>" in unit
    for entry in ("int nic_hash_batch_forward_points_lod(", "int nic_hash_batch_forward_backward_points_lod("):
        e = unit[unit.index(entry):]
        e = e[:e.index("\n}\n")]
        assert e.index("!lodp") < e.index("check_lod(desc, lodp)") < e.index("set_lod(p, lodp, lod)")
    e = unit[unit.index("int nic_hash_batch_forward_backward_points_lod("):]
    e = e[:e.index("\n}\n")]
    st = unit[unit.index("static int batch_points_step("):unit.index("}  // namespace hbatch")]       # the step's host path
    assert "const KernelEndDrop end;" in e and e.index("check_lod(desc, lodp)") < e.index("batch_points_step(p,") and "flags & ~" not in e
    assert st.index("{") < st.index("flags & ~") < st.index("p.d = *desc") and "kernel_end_mark((hipStream_t)stream);" in st


# ------------------------------------------------------------------------------------------------------------------ the Python surface
BAD_LOD_TENSORS = (torch.zeros(6), torch.zeros(2, 7), torch.zeros(3, 6), torch.zeros(3, 7, 1), torch.zeros(7, dtype=torch.float64),
                   torch.zeros(3, 7, dtype=torch.int32))
BAD_LOD_VALUES = (float("nan"), float("inf"), -float("inf"), "coarse", "1.5", "nan", [1.0], (0.0,) * 7, object())


def test_the_wrappers_refuse_before_a_device():
    from neural_image_compression_v2_amd import hashgrid
    geo = P._geo()
    tables, params = torch.zeros(3, *geo.table_shape()), P._params(geo)
    pts, target, gm = torch.zeros(3, 7, 2), torch.zeros(3, 7, 3), [torch.zeros_like(p) for p in params]

    def fb(points=pts, **kw):
        return hashgrid.hash_batch_forward_backward_points_lod(geo, tables, points, params, target, gm, **kw)

    def fw(points=pts, data=tables, **kw):
        return hashgrid.hash_batch_forward_points_lod(geo, data, points, params, **kw)
    for call in (fb, fw):
        for bad in BAD_LOD_TENSORS + ([0.0] * 7, 1.0):
            with pytest.raises(ValueError, match="lod"):
                call(lod=bad)
        for bad in ([0.0] * 3, [0.0] * 3 + [-1.0], [0.0] * 3 + [float("nan")], "0123", 3.0):
            with pytest.raises(ValueError):
                call(fade=bad)
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="lod_uniform"):
                call(lod_uniform=bad)
        for bad in P.BAD_POINTS:
            with pytest.raises(ValueError, match="points"):
                call(points=bad)
        # everything right - no lod, a shared one, one per field - the refusal is the device's: nothing was launched
        for lod in (None, torch.zeros(7), torch.zeros(3, 7)):
            with pytest.raises(RuntimeError, match="HIP device"):
                call(lod=lod, lod_uniform=1.25, fade=[3.0, 2.0, 1.0, 0.0])
    for bad in P.BAD_COUNTS:
        with pytest.raises(ValueError, match="counts"):
            fb(counts=bad)
    for bad in P._bad_orders():
        with pytest.raises(ValueError, match="order"):
            fb(order=bad)
    stored = torch.zeros(3, hashgrid.hash_stored_bytes(geo), dtype=torch.uint8)
    with pytest.raises(ValueError, match="num_bits"):
        fw(data=stored, kind="u8")
    with pytest.raises(RuntimeError, match="HIP device"):
        fw(data=stored, kind="u8", num_bits=8, lod=torch.zeros(7))


def test_the_class_refuses_on_the_host():
    f = P._bare()
    before = dict(f.__dict__)
    pts, target = torch.zeros(3, 7, 2), torch.zeros(3, 7, 3)
    calls = (lambda p, t, lod, **kw: f.train_points_lod(p, t, lod, **kw), lambda p, t, lod, **kw: f.fit_points_lod(p, t, 3, lod, **kw))
    for call in calls:
        for bad in BAD_LOD_TENSORS + BAD_LOD_VALUES + (None,):
            with pytest.raises(ValueError, match="lod"):
                call(pts, target, bad)
        for bad in P.BAD_POINTS:
            with pytest.raises(ValueError, match="points"):
                call(bad, target, 1.0)
        for bad in (torch.zeros(7, 3), torch.zeros(3, 8, 3), None):
            with pytest.raises(ValueError, match="target"):
                call(pts, bad, 1.0)
        for bad in P.BAD_COUNTS:
            with pytest.raises(ValueError, match="counts"):
                call(pts, target, torch.zeros(7), counts=bad)
        for bad in P._bad_orders() + ("morton",):
            with pytest.raises(ValueError, match="order"):
                call(pts, target, torch.zeros(3, 7), order=bad)
        for lod in (0.0, 1, 2.5, torch.tensor(1.5), torch.zeros(7), torch.zeros(3, 7)):
            for order in (None, "cell"):
                with pytest.raises(RuntimeError, match="HIP device"):
                    call(pts, target, lod, counts=(7, 0, 3), order=order)
    with pytest.raises(ValueError, match="noise"):
        f.train_points_lod(pts, target, 1.0, noise=True)                 # no codec: no noise
    # query / resample / decode_mip / fit_mips
    for bad in BAD_LOD_TENSORS + BAD_LOD_VALUES + (None,):
        with pytest.raises(ValueError, match="lod"):
            f.query_lod(pts, bad)
    for precision in ("split", "bf16"):
        with pytest.raises(NotImplementedError, match="level of detail"):
            f.query_lod(pts, 1.0, precision=precision)
        with pytest.raises(NotImplementedError, match="level of detail"):
            f.resample_lod((20, 18), "auto", precision=precision)
    with pytest.raises(ValueError):
        f.query_lod(pts, 1.0, precision="fp8")
    for lod in (1.0, torch.zeros(7), torch.zeros(3, 7)):
        with pytest.raises(RuntimeError, match="HIP device"):
            f.query_lod(pts, lod)
    for bad in ("best", torch.zeros(3), float("nan"), None, [1.0]):
        with pytest.raises(ValueError):
            f.resample_lod((20, 18), bad)
    with pytest.raises(ValueError, match="size"):
        f.resample_lod((20, 18, 4))
    assert f._mip_size(0) == (40, 36) and f._mip_size(2) == (10, 9)
    for m in (3, -1):
        with pytest.raises(ValueError, match="divisible"):
            f.decode_mip(m)
        with pytest.raises(ValueError, match="divisible"):
            f.fit_mips(torch.zeros(3, 40, 36, 3), 1, mips=max(m, 3))
    for bad in (torch.zeros(40, 36, 3), torch.zeros(2, 40, 36, 3), torch.zeros(3, 40, 35, 3), None):
        with pytest.raises(ValueError, match="targets"):
            f.fit_mips(bad, 1)
    with pytest.raises(ValueError, match="mips"):
        f.fit_mips(torch.zeros(3, 40, 36, 3), 1, mips=-1)
    with pytest.raises(RuntimeError, match="HIP device"):
        f.fit_mips(torch.zeros(3, 40, 36, 3), 1, mips=2)
    assert f.__dict__.keys() == before.keys() and all(f.__dict__[k] is before[k] for k in before)       # nothing was set on the way to a refusal
    # the fade: the geometry's unless one is assigned
    from neural_image_compression_v2_amd.hashgrid import hash_lod_fade
    assert f.lod_fade == hash_lod_fade(f.geo)
    for bad in ([0.0] * 3, [0.0] * 5, [0.0] * 3 + [-1.0], [0.0] * 3 + [float("inf")], "0123", 3.0):
        with pytest.raises(ValueError):
            f.lod_fade = bad
    assert "_lod_fade" not in f.__dict__
    f.lod_fade = [3, 2.5, 1, 0]
    assert f.lod_fade == (3.0, 2.5, 1.0, 0.0)
    f.lod_fade = None
    assert f.lod_fade == hash_lod_fade(f.geo)
    # a decode-only batch decodes with a level of detail and refuses to train with one, before it looks at an argument
    g = P._bare(decode_only=True, num_bits=8, frozen=True)
    for call in (lambda: g.train_points_lod(None, None, 1.0), lambda: g.fit_points_lod(None, None, 3, 1.0), lambda: g.fit_mips(None, 3)):
        with pytest.raises(RuntimeError, match="decode-only"):
            call()
    with pytest.raises(RuntimeError, match="HIP device"):
        g.query_lod(pts, 1.0)
    # a bit depth per level in a batch stays refused
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch
    with pytest.raises(NotImplementedError, match="bit depth per level"):
        HashGridFieldBatch(3, (40, 36), levels=4, log2_table=10, num_bits=(8, 6, 4, 2))


# ------------------------------------------------------------------------------------------------------------------ teeth
def _moved(bad, ref):
    return C.worst(C.measure(bad, ref))


def _step(shape, b, lod, noisy=False):
    f = P.field_inputs(shape, b)
    fade = C.inputs(*shape, b).fade
    return T.step(f.geo, f.table_q if noisy else f.table, f.params, f.target, points=f.points, loss_scale=C.LOSS_SCALE,
                  noise_key=C.noise_key() if noisy else None, lod=None if lod is None else (fade, lod, 0.0))


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_teeth_ignoring_the_level_of_detail(shape):
    """the plain kernel's result where the lod kernel's is asked for"""
    for b in range(B):
        q, ratio = _moved(_step(shape, b, None), lod_reference(shape, b, N, False))
        print(f"{C.shape_id(shape)} field {b} without its lod: {q} moves by {ratio:.1f} x its bound")
        assert ratio > C.TEETH


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_teeth_the_neighbour_fields_level_of_detail(shape):
    """field b weighed by field b + 1's slice of lod"""
    for b in range(B):
        mine, theirs = C.inputs(*shape, b).lod, C.inputs(*shape, (b + 1) % B).lod
        assert not np.array_equal(mine, theirs, equal_nan=True)
        q, ratio = _moved(_step(shape, b, theirs), lod_reference(shape, b, N, False))
        print(f"{C.shape_id(shape)} field {b} with field {(b + 1) % B}'s lod: {q} moves by {ratio:.1f} x its bound")
        assert ratio > C.TEETH


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_teeth_the_level_of_detail_is_read_at_the_row(shape):
    """with an order, lod read at the POSITION in the order: the lane at position pos handles row order[pos] and takes lod[pos]"""
    for b in range(B):
        lod = C.inputs(*shape, b).lod
        perm = permutation(b, N).numpy()
        wrong = np.empty_like(lod)
        wrong[perm] = lod                                                 # row perm[pos] gets lod[pos]
        assert not np.array_equal(wrong, lod, equal_nan=True)
        q, ratio = _moved(_step(shape, b, wrong), lod_reference(shape, b, N, False))
        print(f"{C.shape_id(shape)} field {b}, lod by position: {q} moves by {ratio:.1f} x its bound")
        assert ratio > C.TEETH


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_the_inputs_reach_every_weight(shape):
    """over the modes the GPU file runs on this shape: a level of weight 1, one of weight 0, one strictly between, and a level that all 64
    lanes of a wave weigh 0 while another level of that wave is live (the wave-wide skip)"""
    geo = C.inputs(*shape).geo
    for b in range(B):
        seen = set()
        for mode in ("point", "uniform", "skip"):
            fade, lod, u = lod_of(shape, b, mode)
            a = T.level_weights(geo, N, fade, lod, u)
            seen |= {"one"} if (a == 1).any() else set()
            seen |= {"zero"} if (a == 0).any() else set()
            seen |= {"between"} if ((a > 0) & (a < 1)).any() else set()
            for w0 in range(0, N, 64):
                wave = a[w0:w0 + 64]
                off, on = (wave == 0).all(axis=0), (wave > 0).any(axis=0)
                if off.any() and (on.any() or mode == "skip"):
                    seen.add("wave skip")
            if mode == "skip" and shape[2] > 1:
                top = np.array(fade) == max(fade)                             # only the coarsest resolution, at a fractional weight
                assert top[0] and (a[:, ~top] == 0).all() and ((a[:, top] > 0) & (a[:, top] < 1)).all() and (~top).sum() >= shape[2] - 2
        # a single level has no sibling to stay live beside it: its wave-wide skip is the "off" mode below
        assert seen == {"one", "zero", "between"} | ({"wave skip"} if shape[2] > 1 else set()), (b, seen)
    a = T.level_weights(geo, N, *lod_of(shape, 0, "off"))
    assert (a == 0).all()
    if shape[2] > BOUNDARY_LEVEL + 1:
        a = T.level_weights(geo, N, *lod_of(shape, 0, "boundary"))
        assert (a[:, BOUNDARY_LEVEL] == 0).all() and (np.delete(a, BOUNDARY_LEVEL, axis=1) == 1).all()
