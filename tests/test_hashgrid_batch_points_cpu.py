"""CPU-only tests of the batched training at points (run with -m "not gpu"): nic_hash_batch_points_workspace_bytes and
nic_hash_batch_forward_backward_points are exported, declared in the companion header include/nicv2_hip_ext.h and mirrored in
_lib.EXT_SIGNATURES with the same argument lists (the ABI version stays 9, the main header's 86 entries stay); every argument error is decided
on the host in the documented order (fake pointers and refusals only: nothing launches; a launch at no points is NIC_OK); the workspace follows
the groups rule on ceil(n / 64) wave items; the wrappers and ``HashGridFieldBatch.train_points`` / ``fit_points`` refuse before a device is
touched; the kernel sits in the batch unit and restates no shared helper.

Teeth, with the float64 reference alone (oracle/hashgrid_train_ref.py) on the inputs tests/test_gpu_hashgrid_batch_points.py uses: a field
evaluated at its neighbour's points, a loss normalised by the padded width instead of the field's own count, and noise keyed by the position
in the order instead of by the row each move a compared quantity by more than ``C.TEETH`` x its bound on every shape (smallest movements,
x the bound, worst shape and field: 1.4e4, 1.4e5 and 1.1e3).

``field_inputs`` / ``COUNTS`` / ``point_reference`` are shared with the GPU file: both sides see the same bytes."""
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
from tests import test_hashgrid_train_ref_cpu as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
EXT_HEADER = os.path.join(ROOT, "include", "nicv2_hip_ext.h")
UNIT = "hashgrid_batch.hip"
SHARED = "hashgrid_batch.hpp"
TRAIN, WS = "nic_hash_batch_forward_backward_points", "nic_hash_batch_points_workspace_bytes"
ARGS = {WS: ["desc", "n_fields", "groups_per_field", "n_points", "mlp"],
        TRAIN: ["desc", "n_fields", "groups_per_field", "quant", "tables", "points", "n_points", "counts", "order", "mlp", "target", "loss_scale", "table_grads",
                "mlp_grads", "loss", "y", "flags", "workspace", "workspace_bytes", "stream"]}
OK, NULL, UNSUP, SHAPE, WORKSPACE, ARG = 0, -1, -2, -3, -4, -5
P = ctypes.c_void_p
REC = 64 * 16 + 64 + 64 * 64 + 64 + 3 * 64 + 3 + 1          # one record at L F = 16: the decoder's gradients + the loss

# ------------------------------------------------------------------------------------------------------------------ shared with the GPU file
N = C.G.N_POINTS                                             # 209: three waves and a ragged fourth
COUNTS = [None, (209, 65, 1), (64, 0, 63)]                   # a full row, one point past a wave, one point; a whole wave, nothing, one short of a wave


def count_of(counts, b):
    return N if counts is None else counts[b]


def field_inputs(shape, b):
    """field b of a shape: ``C.inputs(*shape, b)`` with the field's OWN points, ``query_points(seed=b)`` (the seed moves the random rows)"""
    return _field_inputs(tuple(int(v) for v in shape), int(b))


@functools.lru_cache(maxsize=None)
def _field_inputs(shape, b):
    inp = C.inputs(*shape, b)
    pts = C.G.query_points(inp.geo.field_size, inp.geo.resolutions, seed=b)
    assert pts.shape == (N, inp.dim) and inp.target_points.shape == (N, 3)
    return types.SimpleNamespace(inp=inp, geo=inp.geo, points=pts, target=inp.target_points, params=inp.params, table=inp.table, table_q=inp.table_q)


def point_reference(shape, b, n_b, noisy, base=C.NOISE_BASE, loss_scale=C.LOSS_SCALE):
    """``T.step`` of field b on its first n_b points, computed once and shared (read-only)"""
    return _point_reference(tuple(int(v) for v in shape), int(b), int(n_b), bool(noisy), int(base), float(loss_scale))


@functools.lru_cache(maxsize=None)
def _point_reference(shape, b, n_b, noisy, base, loss_scale):
    f = field_inputs(shape, b)
    return T.step(f.geo, f.table_q if noisy else f.table, f.params, f.target[:n_b], points=f.points[:n_b], loss_scale=loss_scale,
                  noise_key=C.noise_key(base=base) if noisy else None)


# ------------------------------------------------------------------------------------------------------------------ the C entries
@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_v2_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.load()


def _desc(dim=2, resolutions=(16,) * 8, features=2, log2_table=12, s_max=256, num_crops=1, extent=(256, 256, 1)):
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


def _ref(x):
    return None if x is None else ctypes.byref(x)


def _train(lib, d, n_fields=2, groups=0, quant=None, tables=16, points=16, n_points=130, counts=0, order=0, m="default", target=16, table_grads=16,
           grads="default", loss=16, y=16, flags=0, ws=16, ws_bytes=16):
    """the return code of the entry; every pointer is a dummy that is never dereferenced.  With the 16-byte workspace an accepted call stops at
    the workspace check; with a workspace size that passes, only calls that a LATER check refuses, or n_points == 0, are tried: nothing launches"""
    from neural_image_compression_v2_amd._lib import NicMlpGrads
    m = _mlp() if m == "default" else m
    grads = NicMlpGrads() if grads == "default" else grads
    return lib.nic_hash_batch_forward_backward_points(_ref(d), n_fields, groups, _ref(quant), P(tables), P(points), n_points, P(counts), P(order), _ref(m),
                                                      P(target), 1.0, P(table_grads), _ref(grads), P(loss), P(y), flags, P(ws), ws_bytes, None)


def _cap(lib):
    cap = lib.nic_hash_fused_workspace_bytes(_ref(_desc()), _ref(_mlp())) // (REC * 4)      # one workgroup per CU, a multiple of 8
    assert cap >= 8 and cap % 8 == 0
    return cap


def test_the_entries_are_exported_declared_in_the_companion_header_and_mirrored(lib):
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
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int)
        for c, a in zip(cargs, args):
            if "*" in c:
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (name, c)
            else:
                assert a is types_of[c.split()[0]], (name, c)
        assert [c.split()[-1].lstrip("*") for c in cargs] == names
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args             # load() set them: a stale build fails there
    declared = set(re.findall(r"\b(nic_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", ext, flags=re.S)))
    assert declared == set(_lib.EXT_SIGNATURES) and not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES) == 86                                      # the main header's set is closed
    assert _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version() and re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)      # additive
    for name in ("hash_batch_forward_backward_points", "hash_batch_point_order"):
        assert getattr(pkg, name) is getattr(hashgrid, name)
    assert list(inspect.signature(hashgrid.hash_batch_forward_backward_points).parameters) == [
        "geo", "tables", "points", "params", "target", "mlp_grads", "table_grads", "order", "counts", "loss", "loss_scale", "want_y", "quant", "add_grads",
        "add_loss", "groups_per_field"]
    assert list(inspect.signature(hashgrid.hash_batch_point_order).parameters) == ["geo", "points", "counts"]
    assert list(inspect.signature(hashgrid.HashGridFieldBatch.train_points).parameters) == [
        "self", "points", "target", "counts", "accumulate", "scale", "step", "noise", "order"]
    sig = inspect.signature(hashgrid.HashGridFieldBatch.fit_points).parameters
    assert list(sig) == ["self", "points", "target", "epochs", "counts", "order", "freeze_at"] and sig["order"].default == "cell" and sig["freeze_at"].default == 0.95
    assert "train_points" in hashgrid.HashGridFieldBatch.__doc__ and "4.7.18" in hashgrid.HashGridFieldBatch.__doc__


def test_argument_errors_in_the_documented_order(lib):
    from neural_image_compression_v2_amd._lib import NicHashQuant, NIC_NOISE_KERNEL
    from neural_image_compression_v2_amd.hashgrid import hash_batch_groups
    d = _desc()
    cap = _cap(lib)
    assert _train(lib, d) == WORKSPACE                                   # every check up to the workspace passes
    # 1. null desc / mlp, whatever else is wrong
    assert _train(lib, None) == NULL and _train(lib, d, m=None) == NULL
    assert _train(lib, None, n_fields=0, groups=3, tables=0, n_points=-1) == NULL
    # 2. the fused set (then 256 S_max < 2^30): before n_fields, the groups and every pointer
    bad = _desc()
    bad.flags = 1
    wide = _desc(resolutions=(16,) * 9, features=8)                       # L F = 72
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (_desc(extent=(257, 8, 1)), SHAPE),
                       (_desc(num_crops=0), SHAPE), (wide, UNSUP), (big, ARG)]:
        assert _train(lib, desc) == want
        assert _train(lib, desc, n_fields=0, groups=3, tables=0, y=0, n_points=-1) == want
    assert _train(lib, d, m=_mlp(5, 5)) == UNSUP and _train(lib, d, m=_mlp(5, 5), n_fields=0) == UNSUP
    # 3. n_fields
    for n in (0, -1, 65536, 1 << 30):
        assert _train(lib, d, n_fields=n) == ARG and _train(lib, d, n_fields=n, groups=3, tables=0, n_points=-1) == ARG
    assert _train(lib, d, n_fields=65535, groups=8) == WORKSPACE
    # 4. groups_per_field: 0, or a multiple of 8 up to the grid of one field's wave items, ceil(n_points / 64); no points count as one item
    for g in (-8, -1, 1, 4, 12, 1 << 20):
        assert _train(lib, d, groups=g) == ARG and _train(lib, d, groups=g, tables=0, y=0, n_points=-1) == ARG, g
    assert _train(lib, d, groups=16, n_points=130) == ARG                 # 3 wave items: a grid of 8
    assert _train(lib, d, groups=8, n_points=130) == WORKSPACE
    assert _train(lib, d, groups=16, n_points=64 * 4 * 9) == WORKSPACE    # 9 groups of four: a grid of 16
    assert _train(lib, d, groups=24, n_points=64 * 4 * 9) == ARG
    assert _train(lib, d, groups=16, n_points=0) == ARG and _train(lib, d, groups=16, n_points=-5) == ARG
    assert _train(lib, d, groups=8, n_points=0) == WORKSPACE
    # 5. null pointers (counts, order, table_grads and y may be null), before the flags, the quantiser, the workspace and n_points
    for kw in (dict(tables=0), dict(points=0), dict(target=0), dict(grads=None), dict(loss=0), dict(ws=0), dict(m=_mlp(3, 2))):
        assert _train(lib, d, **kw) == NULL and _train(lib, d, flags=4, n_points=-1, **kw) == NULL, kw
    assert _train(lib, d, table_grads=0, y=0, counts=0, order=0) == WORKSPACE and _train(lib, d, counts=16, order=16) == WORKSPACE
    # 6. flags
    for flags in (4, 8, -1):
        assert _train(lib, d, flags=flags) == ARG
    assert _train(lib, d, flags=3) == WORKSPACE
    # 7. the quantiser: nic_hash_fused_forward_backward's rules
    for bits in (0, 9):
        assert _train(lib, d, quant=NicHashQuant(bits, NIC_NOISE_KERNEL, 1, 2, 0)) == ARG
    assert _train(lib, d, quant=NicHashQuant(8, NIC_NOISE_KERNEL, 1, 2, -1)) == ARG
    assert _train(lib, d, quant=NicHashQuant(8, 1, 1, 2, 0)) == UNSUP                     # NIC_NOISE_TENSOR
    assert _train(lib, d, quant=NicHashQuant(8, 3, 1, 2, 0)) == ARG
    assert _train(lib, d, quant=NicHashQuant(8, NIC_NOISE_KERNEL, 1, 2, 0)) == WORKSPACE
    # 8. the workspace: n_fields x G records - before the point descriptor and n_points
    two = _desc(num_crops=2)
    for n, g in ((1, 8), (2, 8), (5, 16)):
        need = lib.nic_hash_batch_points_workspace_bytes(_ref(d), n, g, 64 * 4 * 9, _ref(_mlp()))
        assert need == n * g * REC * 4
        assert _train(lib, d, n_fields=n, groups=g, n_points=64 * 4 * 9, ws_bytes=need - 1) == WORKSPACE
    assert _train(lib, two) == WORKSPACE and _train(lib, d, n_points=-1) == WORKSPACE and _train(lib, d, n_points=1 << 31) == WORKSPACE
    # 9. the descriptor of a point source: one crop (256 S_max < 2^30 was step 2's)
    enough = 2 * cap * REC * 4                                            # two fields, at most cap workgroups each
    for n_points in (130, 0, -1, 1 << 31):
        assert _train(lib, two, n_points=n_points, ws_bytes=enough) == SHAPE
    # 10. n_points < 0 or >= 2^31
    for n_points in (-1, -64, -(1 << 40), 1 << 31, 1 << 40):
        assert _train(lib, d, n_points=n_points, ws_bytes=enough) == ARG
    # 11. n_points == 0: NIC_OK with no launch (the pointers are fakes: a launch would fault)
    for desc in (d, _desc(dim=3, resolutions=(4, 6, 9, 12), features=1, s_max=12, extent=(12, 10, 9)), _desc(features=8)):
        rec = 64 * desc.levels * desc.features + 64 + 64 * 64 + 64 + 3 * 64 + 3 + 1
        need = lib.nic_hash_batch_points_workspace_bytes(_ref(desc), 2, 0, 0, _ref(_mlp()))
        assert need == 2 * hash_batch_groups(2, 1, cap) * rec * 4 == 2 * 8 * rec * 4
        for flags in (0, 3):
            assert _train(lib, desc, n_points=0, ws_bytes=need, flags=flags) == OK
            assert _train(lib, desc, n_points=0, ws_bytes=need, flags=flags, counts=16, order=16, quant=NicHashQuant(8, NIC_NOISE_KERNEL, 1, 2, 0)) == OK
        assert _train(lib, desc, n_points=0, ws_bytes=need - 1) == WORKSPACE


def test_the_workspace_follows_the_groups_rule_on_the_wave_items(lib):
    from neural_image_compression_v2_amd.hashgrid import hash_batch_groups
    d, m, cap = _desc(), _mlp(), _cap(lib)
    for n_points in (1, 63, 64, 65, 209, 64 * 4 * 8, 64 * 4 * 8 + 1, 1 << 14, 1 << 20, (1 << 31) - 1):
        items = (n_points + 63) // 64
        for b in (1, 3, 8, 40, 64):
            need = lib.nic_hash_batch_points_workspace_bytes(_ref(d), b, 0, n_points, _ref(m))
            assert need == b * hash_batch_groups(b, items, cap) * REC * 4, (n_points, b)
    assert lib.nic_hash_batch_points_workspace_bytes(_ref(d), 3, 16, 64 * 4 * 9, _ref(m)) == 3 * 16 * REC * 4
    # the query answers 0 for what the entry refuses
    wide, two = _desc(resolutions=(16,) * 9, features=8), _desc(num_crops=2)
    for args in ((None, 2, 0, 130, m), (d, 2, 0, 130, None), (wide, 2, 0, 130, m), (d, 0, 0, 130, m), (d, 65536, 0, 130, m), (d, 2, 4, 130, m), (d, 2, 16, 130, m),
                 (two, 2, 0, 130, m), (d, 2, 0, -1, m), (d, 2, 0, 1 << 31, m)):
        assert lib.nic_hash_batch_points_workspace_bytes(_ref(args[0]), args[1], args[2], args[3], _ref(args[4])) == 0


# ------------------------------------------------------------------------------------------------------------------ the unit
def test_the_kernel_is_in_the_batch_unit_and_restates_no_shared_helper():
    from neural_image_compression_v2_amd import _build
    import test_hashgrid_common_cpu as common
    assert UNIT in _build.SOURCES and SHARED in _build.HEADERS and len(set(_build.SOURCES)) == len(_build.SOURCES)
    texts = {f: open(os.path.join(_build.CSRC, f)).read() for f in (UNIT, SHARED, "hashgrid_fused16.hip")}
    lines = texts[UNIT].splitlines()
    assert any(re.match(r'\s*#include\s+"hashgrid_batch\.hpp"', ln) for ln in lines) and any(re.match(r'\s*#include\s+".*nicv2_hip_ext\.h"', ln) for ln in lines)
    device = ["lattice_fixed", "load_decoder", "decoder_forward_half", "decoder_train_half", "write_record", "persistent_grid", "strided_grid", "field_range"]
    for f in (UNIT, SHARED):
        for name in common.FUNCTIONS + list(common.OVERLOADS) + (device if f == UNIT else device[:-1]):
            assert not any(common._function_re(name).match(ln) for ln in texts[f].splitlines()), (f, name)
        for name in common.STRUCTS + ["DecoderSmem", "TrainSmem", "TrainAcc"]:
            assert not any(common._struct_re(name).match(ln) for ln in texts[f].splitlines()), (f, name)
    # the loss multiplier and the clamped count: one definition each, shared by the kernel and the reduction
    for name in ("field_loss_mul", "field_count"):
        found = [f for f, t in texts.items() if any(common._function_re(name).match(ln) for ln in t.splitlines())]
        assert found == [SHARED], (name, found)
    assert "__host__ __device__ inline float field_loss_mul(" in texts[SHARED]
    assert "(double)loss_scale / (3.0" not in texts[UNIT]                 # the expression lives in the helper alone
    # the kernel: hash_batch_kernel's training shape around the point source
    unit = texts[UNIT]
    k = unit[unit.index("hash_batch_points_kernel(const"):]
    k = k[:k.index("// ---- forward only")]
    for call in ("load_decoder(", "field_count(p.counts, b, p.n)", "field_loss_mul(p.loss_scale, n_b)", "field_range(n_waves, lb, p.groups)",
                 "ordered_row(order, n_b,", "point_fixed<D>(p.d, points, row, t)", "encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, false>(src_b, t, row,",
                 "decoder_train_half<KT>(", "scatter_point<D, F, false>(", "write_record<KT>(", "blockIdx.x / (unsigned)p.groups", "TrainSmem"):
        assert call in k, call
    assert k.count("__syncthreads()") == 1 and k.index("__syncthreads()") < k.index("for (int64_t g")      # the one barrier follows the prologue
    assert k.index("decoder_train_half<KT>(") < k.index("scatter_point<D, F, false>(") < k.index("write_record<KT>(")
    r = unit[unit.index("void __launch_bounds__(256) hash_batch_reduce_kernel("):]
    r = r[:r.index("// ---- host side")]
    assert "const int32_t* counts" in r and "float loss_scale" in r and "field_count(counts," in r and "field_loss_mul(loss_scale, n_b)" in r
    assert "tail_block" not in unit                                      # still no optimiser tail on the reduction
    assert "hash_batch_points_kernel<D, F, 2, NOISE>" in unit and "hash_batch_points_kernel<D, F, 1, NOISE>" in unit and "p.d.levels * F > 32" in unit
    e = unit[unit.index("int nic_hash_batch_forward_backward_points("):]
    e = e[:e.index("\n}\n")]
    assert "const KernelEndDrop end;" in e and e.index("open_batch_points(") < e.index("!tables") < e.index("batch_points_step(p,")
    st = unit[unit.index("static int batch_points_step("):unit.index("}  // namespace hbatch")]       # the step's host path
    assert st.index("launch(std::true_type{})") < st.index("kernel_end_mark((hipStream_t)stream);") < st.index("launch_batch_reduce(")


# ------------------------------------------------------------------------------------------------------------------ the Python surface
def _geo(size=(40, 36), levels=4, features=2, log2_table=10):
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, level_resolutions
    return HashGeometry(size, tuple(level_resolutions(levels, 16, max(size))), features, log2_table)


def _params(geo, b=3):
    lf = geo.width
    return [torch.zeros(b, 64, lf), torch.zeros(b, 64), torch.zeros(b, 64, 64), torch.zeros(b, 64), torch.zeros(b, 3, 64), torch.zeros(b, 3)]


BAD_POINTS = (torch.zeros(7), torch.zeros(7, 3), torch.zeros(2, 7, 2), torch.zeros(3, 7, 3), torch.zeros(7, 2, dtype=torch.float64), [[0.0, 0.0]], None)
BAD_COUNTS = ((1, 2), (1, 2, 3, 4), (1, 2, 8), (-1, 0, 0), (1.0, 2, 3), (True, 1, 1), "123", torch.tensor([1.0, 2.0, 3.0]), torch.tensor([1, 2]),
              torch.tensor([[1, 2, 3]]), torch.tensor([1, 2, 8]), torch.tensor([0, -1, 0], dtype=torch.int32))
GOOD_COUNTS = (None, (7, 0, 3), [0, 0, 0], torch.tensor([7, 7, 7]), torch.tensor([1, 2, 3], dtype=torch.int32), np.array([1, 2, 3]))


def _bad_orders(n=7):
    return (torch.zeros(3, n, dtype=torch.int64), torch.zeros(3, n), torch.zeros(3, n - 1, dtype=torch.int32), torch.zeros(n, dtype=torch.int32),
            torch.zeros(2, n, dtype=torch.int32), [[0] * n] * 3)


def test_the_wrappers_refuse_before_a_device():
    from neural_image_compression_v2_amd import hashgrid
    geo = _geo()
    tables, params = torch.zeros(3, *geo.table_shape()), _params(geo)
    pts, target, gm = torch.zeros(3, 7, 2), torch.zeros(3, 7, 3), [torch.zeros_like(p) for p in params]

    def fb(tables=tables, points=pts, params=params, target=target, gm=gm, **kw):
        return hashgrid.hash_batch_forward_backward_points(geo, tables, points, params, target, gm, **kw)
    for bad in (tables[0], torch.zeros(3, 4, 1024), torch.zeros(3, 4, 512, 2), torch.zeros(0, 4, 1024, 2)):
        with pytest.raises(ValueError, match="tables"):
            fb(tables=bad)
        with pytest.raises(ValueError, match="table_grads"):
            fb(table_grads=bad)
    with pytest.raises(ValueError, match="table_grads"):
        fb(table_grads=torch.zeros(2, *geo.table_shape()))
    with pytest.raises(TypeError):
        fb(tables=None)
    for k, shape in enumerate([(3, 64, 9), (3, 32), (3, 64, 32), (2, 64), (3, 64, 3), (3,)]):
        bad = list(params)
        bad[k] = torch.zeros(*shape)
        with pytest.raises(ValueError, match="params"):
            fb(params=bad)
        with pytest.raises(ValueError, match="mlp_grads"):
            fb(gm=bad)
    for bad in BAD_POINTS:
        with pytest.raises(ValueError, match="points"):
            fb(points=bad)
    with pytest.raises(ValueError, match="no points"):
        fb(points=torch.zeros(3, 0, 2), target=torch.zeros(3, 0, 3))
    for bad in (torch.zeros(7, 3), torch.zeros(2, 7, 3), torch.zeros(3, 8, 3), torch.zeros(3, 7, 4), None):
        with pytest.raises(ValueError, match="target"):
            fb(target=bad)
    for bad in BAD_COUNTS:
        with pytest.raises(ValueError, match="counts"):
            fb(counts=bad)
    for bad in _bad_orders():
        with pytest.raises(ValueError, match="order"):
            fb(order=bad)
    for bad in (torch.zeros(3, 7, 4), torch.zeros(2, 7, 3), torch.zeros(3, 7, 3, dtype=torch.float64), torch.zeros(3, 3, 7).transpose(1, 2)):
        with pytest.raises(ValueError, match="want_y"):
            fb(want_y=bad)
    for bad in (torch.zeros(2), torch.zeros(3, 1), torch.zeros(3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="loss"):
            fb(loss=bad)
    with pytest.raises(ValueError, match="too large"):
        hashgrid.hash_batch_forward_backward_points(hashgrid.HashGeometry((1 << 22, 8), (1, 1), 2, 10), torch.zeros(3, 2, 1024, 2), pts, _params(_geo(levels=2)),
                                                    target, [torch.zeros_like(p) for p in _params(_geo(levels=2))])
    # with everything shaped right the refusal is the device's: nothing was launched
    for counts in GOOD_COUNTS:
        with pytest.raises(RuntimeError, match="HIP device"):
            fb(counts=counts, order=torch.zeros(3, 7, dtype=torch.int32), want_y=torch.zeros(3, 7, 3), loss=torch.zeros(3))
    with pytest.raises(RuntimeError, match="HIP device"):
        fb(points=torch.zeros(7, 2), want_y=True)                        # shared points
    # the order of a batch
    po = hashgrid.hash_batch_point_order
    for bad in (torch.zeros(7, 2), torch.zeros(3, 7, 3), torch.zeros(3, 7, 2, dtype=torch.float64), torch.zeros(0, 7, 2), None):
        with pytest.raises(ValueError, match="points"):
            po(geo, bad)
    for bad in BAD_COUNTS:
        with pytest.raises(ValueError, match="counts"):
            po(geo, pts, bad)
    for counts in GOOD_COUNTS:
        with pytest.raises(RuntimeError, match="HIP device"):
            po(geo, pts, counts)


def _bare(decode_only=False, num_bits=None, frozen=False):
    """a batch put together by hand on the CPU"""
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch, hash_stored_bytes
    geo = _geo()
    f = HashGridFieldBatch.__new__(HashGridFieldBatch)
    f.n_fields, f.field_size, f.device, f.num_bits, f.frozen, f.geo = 3, (40, 36), torch.device("cpu"), num_bits, frozen, geo
    f.groups_per_field, f.steps, f.noise_seed, f._pass_samples, f._grad_clean = 0, 0, 7, 5, True
    f.params, f.optimizer, f.scheduler = _params(geo), None, None
    f._gm = [torch.zeros_like(p) for p in f.params]
    if decode_only:
        f.tables, f.packed, f.stored = None, None, torch.zeros(3, hash_stored_bytes(geo), dtype=torch.uint8)
    else:
        f.tables, f.packed, f.stored = torch.zeros(3, *geo.table_shape()), None, None
    return f


def test_the_class_refuses_on_the_host():
    f = _bare()
    before = dict(f.__dict__)
    pts, target = torch.zeros(3, 7, 2), torch.zeros(3, 7, 3)
    calls = (lambda p, t, **kw: f.train_points(p, t, **kw), lambda p, t, **kw: f.fit_points(p, t, 3, **kw))
    for call in calls:
        for bad in BAD_POINTS:
            with pytest.raises(ValueError, match="points"):
                call(bad, target)
        with pytest.raises(ValueError, match="no points"):
            call(torch.zeros(3, 0, 2), torch.zeros(3, 0, 3))
        for bad in (torch.zeros(7, 3), torch.zeros(2, 7, 3), torch.zeros(3, 8, 3), torch.zeros(3, 7, 4), None):
            with pytest.raises(ValueError, match="target"):
                call(pts, bad)
        for bad in BAD_COUNTS:
            with pytest.raises(ValueError, match="counts"):
                call(pts, target, counts=bad)
        for bad in _bad_orders() + ("morton", "Cell", ""):
            with pytest.raises(ValueError, match="order"):
                call(pts, target, order=bad)
        # everything right: shared or per-field points, every kind of count and order - the refusal is the device's
        for counts in GOOD_COUNTS:
            for order in (None, "cell", torch.zeros(3, 7, dtype=torch.int32)):
                with pytest.raises(RuntimeError, match="HIP device"):
                    call(pts, target, counts=counts, order=order)
        with pytest.raises(RuntimeError, match="HIP device"):
            call(torch.zeros(7, 2), target)
    with pytest.raises(ValueError, match="noise"):
        f.train_points(pts, target, noise=True)                          # no codec: no noise
    assert f.__dict__.keys() == before.keys() and all(f.__dict__[k] is before[k] for k in before)       # nothing was set on the way to a refusal
    # a decode-only batch refuses both, before it looks at an argument
    g = _bare(decode_only=True, num_bits=8, frozen=True)
    with pytest.raises(RuntimeError, match="decode-only"):
        g.train_points(None, None)
    with pytest.raises(RuntimeError, match="decode-only"):
        g.fit_points(None, None, 3)


# ------------------------------------------------------------------------------------------------------------------ teeth
def _moved(bad, ref):
    q, ratio = C.worst(C.measure(bad, ref))
    return q, ratio


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_teeth_a_field_at_its_neighbours_points(shape):
    """field b evaluated at field b + 1's points (its own table, decoder and targets)"""
    for b in range(C.N_FIELDS):
        f, nxt = field_inputs(shape, b), field_inputs(shape, (b + 1) % C.N_FIELDS)
        assert not np.array_equal(f.points, nxt.points, equal_nan=True)
        bad = T.step(f.geo, f.table, f.params, f.target, points=nxt.points, loss_scale=C.LOSS_SCALE)
        q, ratio = _moved(bad, point_reference(shape, b, N, False))
        print(f"{C.shape_id(shape)} field {b} at field {(b + 1) % C.N_FIELDS}'s points: {q} moves by {ratio:.1f} x its bound")
        assert ratio > C.TEETH


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_teeth_the_loss_is_normalised_by_the_fields_own_count(shape):
    """the mean taken over the padded 209 rows instead of the field's n_b: every count below 209 that the GPU test uses"""
    for counts in COUNTS[1:]:
        for b, n_b in enumerate(counts):
            if n_b in (0, N):
                continue
            bad = point_reference(shape, b, n_b, False, loss_scale=C.LOSS_SCALE * n_b / N)
            q, ratio = _moved(bad, point_reference(shape, b, n_b, False))
            print(f"{C.shape_id(shape)} field {b}, {n_b} of {N} points: {q} moves by {ratio:.1f} x its bound")
            assert ratio > C.TEETH


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_teeth_the_noise_is_keyed_by_the_row(shape):
    """with an order, the noise of the POSITION in the order instead of the row's: the step of the permuted set with its noise keyed as it
    lies, its outputs put back at their rows"""
    for b in range(C.N_FIELDS):
        f = field_inputs(shape, b)
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(11 + b))
        assert not torch.equal(perm, torch.arange(N))
        wrong = T.step(f.geo, f.table_q, f.params, f.target[perm], points=f.points[perm.numpy()], loss_scale=C.LOSS_SCALE, noise_key=C.noise_key())
        y = torch.empty_like(wrong.y)
        y[perm] = wrong.y
        bad = types.SimpleNamespace(y=y, loss=wrong.loss, table_grad=wrong.table_grad, decoder_grads=wrong.decoder_grads, dpoints=None)
        q, ratio = _moved(bad, point_reference(shape, b, N, True))
        print(f"{C.shape_id(shape)} field {b}, noise by position: {q} moves by {ratio:.1f} x its bound")
        assert ratio > C.TEETH


def test_the_counts_reach_every_path():
    """a full row, a wave and one point, one point, a whole wave, none, one short of a wave; and fields whose points differ"""
    seen = {n for c in COUNTS[1:] for n in c}
    assert seen == {209, 65, 1, 64, 0, 63} and all(len(c) == C.N_FIELDS for c in COUNTS[1:])
    for dim, shape in ((2, (2, 2, 16)), (3, (3, 4, 8))):
        _, moved = T.clamp_points(field_inputs(shape, 0).geo, field_inputs(shape, 0).points[:63])
        assert moved.any() and np.isnan(field_inputs(shape, 0).points[:63]).any()         # even the short rows hold points outside and NaN
