"""CPU-only tests of the batched hash-grid fields (run with -m "not gpu"): the three nic_hash_batch_* entries are exported, declared
and mirrored with matching argument lists, the ABI version stays 9, the new translation unit is in the build, includes hash_common.hpp and
restates none of its helpers, every argument error is decided on the host in the order of nic_hash_fused_forward_backward (fake pointers and a
16-byte workspace: nothing launches), the automatic groups_per_field rule holds as a pure function and against the library, and the wrappers and
``HashGridFieldBatch`` refuse bad shapes and options before they touch a device."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
UNIT = "hashgrid_batch.hip"
SYMBOLS = {"nic_hash_batch_workspace_bytes": 4, "nic_hash_batch_forward": 8, "nic_hash_batch_forward_backward": 17}
OK, NULL, UNSUP, SHAPE, WORKSPACE, ARG = 0, -1, -2, -3, -4, -5
P = ctypes.c_void_p
REC = 64 * 16 + 64 + 64 * 64 + 64 + 3 * 64 + 3 + 1          # one record at L F = 16: the decoder's gradients + the loss


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


def _train(lib, d, n_fields=2, groups=0, quant=None, tables=16, origins=16, m="default", target=16, table_grads=16, grads="default", loss=16, y=16,
           flags=0, ws=16, ws_bytes=16):
    """the return code of the training entry; every pointer is a dummy that is never dereferenced, and the 16-byte workspace stops an accepted
    call at the last check, so nothing launches"""
    from neural_image_compression_v2_amd._lib import NicMlpGrads
    m = _mlp() if m == "default" else m
    grads = NicMlpGrads() if grads == "default" else grads
    return lib.nic_hash_batch_forward_backward(_ref(d), n_fields, groups, _ref(quant), P(tables), P(origins), _ref(m), P(target), 1.0, P(table_grads),
                                               _ref(grads), P(loss), P(y), flags, P(ws), ws_bytes, None)


def _fwd(lib, d, n_fields=2, groups=0, tables=16, origins=16, m="default", y=16):
    """the forward entry: an accepted call would launch, so only refusals are tried"""
    m = _mlp() if m == "default" else m
    return lib.nic_hash_batch_forward(_ref(d), n_fields, groups, P(tables), P(origins), _ref(m), P(y), None)


def _c_args(header, name):
    m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_entries_are_exported_declared_and_mirrored(lib):
    from neural_image_compression_v2_amd import _lib, hashgrid
    import neural_image_compression_v2_amd as pkg
    header = open(HEADER).read()
    for name, n_args in SYMBOLS.items():
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        cargs = _c_args(header, name)
        assert len(cargs) == len(args) == n_args, (name, cargs)
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int)
        for c, a in zip(cargs, args):
            if "*" in c:
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (name, c)
            else:
                assert a is {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}[c.split()[0]], (name, c)
    assert _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version() and re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)      # additive
    for name in ("hash_batch_forward", "hash_batch_forward_backward", "hash_batch_groups", "HashGridFieldBatch"):
        assert getattr(pkg, name) is getattr(hashgrid, name)
    import inspect
    assert list(inspect.signature(hashgrid.HashGridFieldBatch.__init__).parameters)[1:] == [
        "n_fields", "field_size", "levels", "features", "log2_table", "base_resolution", "finest_resolution", "device", "seed", "num_bits", "noise_seed",
        "groups_per_field", "hidden", "n_linear"]


def test_the_unit_is_in_the_build_and_restates_no_shared_helper():
    from neural_image_compression_v2_amd import _build
    import test_hashgrid_common_cpu as common
    assert UNIT in _build.SOURCES and len(set(_build.SOURCES)) == len(_build.SOURCES)
    assert not UNIT.startswith("hash_")                                 # outside the glob tests/test_hashgrid_common_cpu.py pins
    lines = open(os.path.join(_build.CSRC, UNIT)).read().splitlines()
    assert any(re.match(r'\s*#include\s+"hash_common\.hpp"', ln) for ln in lines)
    device = ["lattice_fixed", "load_decoder", "decoder_forward_half", "decoder_train_half", "write_record", "persistent_grid", "strided_grid"]
    for name in common.FUNCTIONS + list(common.OVERLOADS) + device:
        assert not any(common._function_re(name).match(ln) for ln in lines), name
    for name in common.STRUCTS + ["DecoderSmem", "TrainSmem", "TrainAcc"]:
        assert not any(common._struct_re(name).match(ln) for ln in lines), name
    text = "\n".join(lines)
    for call in ("encode_point<D, F, NIC_HASH_SRC_F32,", "lattice_fixed<D>(", "decoder_train_half<KT>(", "scatter_point<D, F, false>(", "write_record<KT>(",
                 "decoder_forward_half(", "load_decoder(", "nic_hash_fused_supported("):
        assert call in text, call
    assert "blockIdx.y" in text and "hash_batch_reduce_kernel" in text and "tail_block" not in text      # no optimiser tail on the reduction


def test_argument_errors_in_the_order_of_the_single_entry(lib):
    from neural_image_compression_v2_amd._lib import NicHashQuant, NIC_NOISE_KERNEL
    d = _desc()
    both = (lambda *a, **kw: _train(lib, *a, **kw), lambda *a, **kw: _fwd(lib, *a, **kw))
    assert _train(lib, d) == WORKSPACE                                   # every check but the last passes
    # 1. null desc / mlp
    for call in both:
        assert call(None) == NULL and call(d, m=None) == NULL
        assert call(None, n_fields=0, groups=3, tables=0) == NULL
    # 2. the fused set (then 256 S_max < 2^30): before n_fields, the groups and every pointer
    bad = _desc()
    bad.flags = 1
    wide = _desc(resolutions=(16,) * 9, features=8)                       # L F = 72
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (_desc(extent=(257, 8, 1)), SHAPE),
                       (_desc(num_crops=0), SHAPE), (wide, UNSUP), (big, ARG)]:
        for call in both:
            assert call(desc) == want
            assert call(desc, n_fields=0, groups=3, tables=0, y=0) == want
    for call in both:
        assert call(d, m=_mlp(5, 5)) == UNSUP and call(d, m=_mlp(5, 5), n_fields=0) == UNSUP
    # 3. n_fields
    for n in (0, -1, 65536, 1 << 30):
        for call in both:
            assert call(d, n_fields=n) == ARG and call(d, n_fields=n, groups=3, tables=0) == ARG
    assert _train(lib, d, n_fields=65535, groups=8) == WORKSPACE
    # 4. groups_per_field: 0, or a multiple of 8 up to the grid of one field alone (1024 patches: the cap; 16 x 16: one group of four, 8)
    cap = lib.nic_hash_fused_workspace_bytes(_ref(d), _ref(_mlp())) // (REC * 4)
    assert cap >= 8 and cap % 8 == 0
    small = _desc(extent=(16, 16, 1))
    for call in both:
        for g in (-8, -1, 1, 4, 12, cap + 8, 1 << 20):
            assert call(d, groups=g) == ARG and call(d, groups=g, tables=0, y=0) == ARG, g
        assert call(small, groups=16) == ARG
    for g in (0, 8, cap):
        assert _train(lib, d, groups=g) == WORKSPACE, g
    assert _train(lib, small, groups=8) == WORKSPACE and _train(lib, small, groups=0) == WORKSPACE
    # 5. null pointers (table_grads and y may be null), before the flags, the quantiser and the workspace
    for kw in (dict(tables=0), dict(origins=0), dict(target=0), dict(grads=None), dict(loss=0), dict(ws=0), dict(m=_mlp(3, 2))):
        assert _train(lib, d, **kw) == NULL and _train(lib, d, flags=4, **kw) == NULL, kw
    assert _train(lib, d, table_grads=0, y=0) == WORKSPACE
    for kw in (dict(tables=0), dict(origins=0), dict(y=0), dict(m=_mlp(3, 2))):
        assert _fwd(lib, d, **kw) == NULL, kw
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
    # 8. the workspace: n_fields x G records
    for n, g in ((1, 8), (2, 8), (5, 16)):
        need = lib.nic_hash_batch_workspace_bytes(_ref(d), n, g, _ref(_mlp()))
        assert need == n * g * REC * 4
        assert _train(lib, d, n_fields=n, groups=g, ws_bytes=need - 1) == WORKSPACE
    # the query answers 0 for what the entries refuse
    for args in ((None, 2, 0, _mlp()), (d, 2, 0, None), (wide, 2, 0, _mlp()), (d, 0, 0, _mlp()), (d, 2, 4, _mlp()), (small, 2, 16, _mlp())):
        assert lib.nic_hash_batch_workspace_bytes(_ref(args[0]), args[1], args[2], _ref(args[3])) == 0


def test_the_automatic_groups_rule(lib):
    from neural_image_compression_v2_amd.hashgrid import hash_batch_groups
    # cap // B rounded up to a multiple of 8, at least 8, at most the grid of one field alone
    assert [hash_batch_groups(b, 1024, 256) for b in (1, 2, 3, 8, 31, 32, 33, 64, 1000)] == [256, 128, 88, 32, 8, 8, 8, 8, 8]
    assert hash_batch_groups(3, 75, 256) == 24 and hash_batch_groups(1, 75, 256) == 24          # 19 groups of four: the grid of one field is 24
    assert hash_batch_groups(40, 4, 256) == 8 and hash_batch_groups(2, 12, 256) == 8
    assert hash_batch_groups(3, 1024, 304) == 104 and hash_batch_groups(1, 100000, 304) == 304
    assert hash_batch_groups(3, 1024, 256, 16) == 16 and hash_batch_groups(3, 75, 256, 24) == 24
    for bad in (dict(groups_per_field=4), dict(groups_per_field=-8), dict(groups_per_field=264), dict(n_fields=0)):
        kw = dict(n_fields=3, patches=1024, cap=256)
        kw.update(bad)
        with pytest.raises(ValueError):
            hash_batch_groups(**kw)
    with pytest.raises(ValueError):
        hash_batch_groups(3, 75, 256, 32)
    # the library's rule is this one: its workspace is n_fields x G records
    d, m = _desc(), _mlp()
    cap = lib.nic_hash_fused_workspace_bytes(_ref(d), _ref(m)) // (REC * 4)
    for extent, patches in (((256, 256, 1), 1024), ((40, 36, 1), 25), ((16, 16, 1), 4), ((100, 60, 1), 13 * 8)):
        for b in (1, 3, 8, 40, 64):
            need = lib.nic_hash_batch_workspace_bytes(_ref(_desc(extent=extent)), b, 0, _ref(m))
            assert need == b * hash_batch_groups(b, patches, cap) * REC * 4, (extent, b)


def _geo(size=(40, 36), levels=4, features=2, log2_table=10):
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, level_resolutions
    return HashGeometry(size, tuple(level_resolutions(levels, 16, max(size))), features, log2_table)


def _stack(geo, b=3):
    lf = geo.width
    return torch.zeros(b, *geo.table_shape()), [torch.zeros(b, 64, lf), torch.zeros(b, 64), torch.zeros(b, 64, 64), torch.zeros(b, 64), torch.zeros(b, 3, 64),
                                                torch.zeros(b, 3)]


def test_the_wrappers_check_the_stacked_shapes_before_a_device():
    from neural_image_compression_v2_amd import hashgrid
    geo = _geo()
    tables, params = _stack(geo)
    extent, n = (20, 12), 2 * 20 * 12
    coord = [[0, 0], [20, 24]]
    target, gm = torch.zeros(3, n, 3), [torch.zeros_like(p) for p in params]

    def fb(tables=tables, coord=coord, params=params, target=target, gm=gm, **kw):
        return hashgrid.hash_batch_forward_backward(geo, tables, coord, extent, params, target, gm, **kw)
    # the tables: [B, L, T, F]
    for bad in (tables[0], torch.zeros(3, 4, 1024), torch.zeros(3, 4, 512, 2), torch.zeros(3, 5, 1024, 2), torch.zeros(0, 4, 1024, 2)):
        with pytest.raises(ValueError, match="tables"):
            hashgrid.hash_batch_forward(geo, bad, coord, extent, params)
        with pytest.raises(ValueError, match="tables"):
            fb(tables=bad)
    with pytest.raises(TypeError):
        hashgrid.hash_batch_forward(geo, None, coord, extent, params)
    # the decoder: six tensors stacked like the tables
    for k, shape in enumerate([(3, 64, 9), (3, 32), (3, 64, 32), (2, 64), (3, 64, 3), (3,)]):
        bad = list(params)
        bad[k] = torch.zeros(*shape)
        with pytest.raises(ValueError, match="params"):
            hashgrid.hash_batch_forward(geo, tables, coord, extent, bad)
        with pytest.raises(ValueError, match="params"):
            fb(params=bad)
        with pytest.raises(ValueError, match="mlp_grads"):
            fb(gm=bad)
    with pytest.raises(ValueError, match="params"):
        hashgrid.hash_batch_forward(geo, tables, coord, extent, params[:4])
    one = [p[:1] for p in params]
    with pytest.raises(ValueError, match="params"):
        hashgrid.hash_batch_forward(geo, tables, coord, extent, one)      # a decoder for one field, three tables
    # with everything shaped right the refusal is the device's: nothing was launched
    with pytest.raises(RuntimeError, match="HIP device"):
        hashgrid.hash_batch_forward(geo, tables, coord, extent, params)
    with pytest.raises(RuntimeError, match="HIP device"):
        fb()


def test_per_field_origins_are_checked_like_check_crops():
    from neural_image_compression_v2_amd import hashgrid
    geo = _geo()
    o = hashgrid._batch_origins(geo, [[0, 0], [20, 24]], (20, 12), 3, "cpu")
    assert o.dtype == torch.int32 and o.shape == (3, 2, 2) and o.is_contiguous() and torch.equal(o[0], o[2])
    per = torch.tensor([[[0, 0], [20, 24]], [[1, 2], [3, 4]], [[20, 24], [0, 0]]])
    assert torch.equal(hashgrid._batch_origins(geo, per, (20, 12), 3, "cpu"), per.to(torch.int32))
    bad = per.clone()
    bad[1, 1, 0] = 21                                                     # 21 + 20 > 40: one crop of one field leaves the field
    with pytest.raises(IndexError):
        hashgrid._batch_origins(geo, bad, (20, 12), 3, "cpu")
    bad[1, 1, 0] = -1
    with pytest.raises(IndexError):
        hashgrid._batch_origins(geo, bad, (20, 12), 3, "cpu")
    with pytest.raises(ValueError):
        hashgrid._batch_origins(geo, per[:2], (20, 12), 3, "cpu")          # two fields' crops for three fields
    with pytest.raises(ValueError):
        hashgrid._batch_origins(geo, per, (20, 12, 1), 3, "cpu")
    with pytest.raises(ValueError):
        hashgrid._batch_origins(geo, per, (20, 0), 3, "cpu")


def test_the_class_refuses_on_the_host():
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, HashGridField, HashGridFieldBatch, level_resolutions
    kw = dict(levels=8, features=2, log2_table=12, device="cpu")
    # the constructor: every refusal before the device (which "cpu" would fail last)
    with pytest.raises(NotImplementedError):
        HashGridFieldBatch(2, (64, 64), num_bits=[8] * 8, **kw)            # a bit depth per level
    with pytest.raises(NotImplementedError):
        HashGridFieldBatch(2, (64, 64), num_bits=(4, 4, 4, 4, 8, 8, 8, 8), **kw)
    for bits in (0, 9, -1):
        with pytest.raises(ValueError, match="num_bits"):
            HashGridFieldBatch(2, (64, 64), num_bits=bits, **kw)
    with pytest.raises(ValueError, match="hidden"):
        HashGridFieldBatch(2, (64, 64), hidden=32, **kw)
    with pytest.raises(ValueError, match="n_linear"):
        HashGridFieldBatch(2, (64, 64), n_linear=5, **kw)
    with pytest.raises(ValueError, match="fused set"):
        HashGridFieldBatch(2, (64, 64), levels=9, features=8, log2_table=12, device="cpu")     # L F = 72
    for n in (0, -3):
        with pytest.raises(ValueError, match="at least one"):
            HashGridFieldBatch(n, (64, 64), **kw)
    for g in (4, -8, 12):
        with pytest.raises(ValueError, match="groups_per_field"):
            HashGridFieldBatch(2, (64, 64), groups_per_field=g, **kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        HashGridFieldBatch(2, (64, 64), num_bits=8, groups_per_field=16, **kw)

    def bare(n_fields=3, size=(40, 36), num_bits=None, frozen=False):
        f = HashGridFieldBatch.__new__(HashGridFieldBatch)
        f.n_fields, f.field_size, f.device, f.num_bits, f.frozen = n_fields, size, torch.device("cpu"), num_bits, frozen
        f.geo = HashGeometry(size, tuple(level_resolutions(4, 16, max(size))), 2, 10)
        f.groups_per_field, f.steps, f.noise_seed, f._pass_samples, f._grad_clean = 0, 0, 7, 0, True
        return f
    f = bare()
    before = dict(f.__dict__)
    n = 20 * 12
    # train_step: crops per field, the target's shape, noise without a codec
    with pytest.raises(IndexError):
        f.train_step([[21, 0]], (20, 12), torch.zeros(3, n, 3))
    with pytest.raises(IndexError):
        f.train_step(torch.tensor([[[0, 0]], [[0, 25]], [[0, 0]]]), (20, 12), torch.zeros(3, n, 3))
    with pytest.raises(ValueError, match="origins"):
        f.train_step(torch.zeros(2, 1, 2, dtype=torch.int64), (20, 12), torch.zeros(3, n, 3))
    for bad in (torch.zeros(n, 3), torch.zeros(2, n, 3), torch.zeros(3, n + 1, 3), torch.zeros(3, n, 4)):
        with pytest.raises(ValueError, match="target"):
            f.train_step([[0, 0]], (20, 12), bad)
    with pytest.raises(ValueError, match="noise"):
        f.train_step([[0, 0]], (20, 12), torch.zeros(3, n, 3), noise=True)
    # fit, freeze, save_compressed, extract / insert
    for bad in (torch.zeros(40, 36, 3), torch.zeros(2, 40, 36, 3), torch.zeros(3, 36, 40, 3)):
        with pytest.raises(ValueError, match="targets"):
            f.fit(bad, 3)
    with pytest.raises(ValueError, match="chunk"):
        f.fit(torch.zeros(3, 40, 36, 3), 3, chunk=0)
    with pytest.raises(RuntimeError, match="num_bits"):
        f.freeze()
    with pytest.raises(RuntimeError, match="num_bits"):
        f.save_compressed(["a", "b", "c"])
    with pytest.raises(ValueError, match="paths"):
        bare(num_bits=8).save_compressed(["a", "b"])
    for b in (-1, 3):
        with pytest.raises(IndexError):
            f.extract(b)
        with pytest.raises(IndexError):
            f.insert(b, None)
    with pytest.raises(TypeError):
        f.insert(0, object())

    def single(size=(40, 36), log2_table=10, num_bits=None, level_bits=None, hidden=64, n_linear=3, frozen=False, table=True):
        s = HashGridField.__new__(HashGridField)
        s.geo = HashGeometry(size, tuple(level_resolutions(4, 16, max(size))), 2, log2_table)
        s.hidden, s.n_linear, s.num_bits, s.level_bits, s.frozen, s.table = hidden, n_linear, num_bits, level_bits, frozen, (torch.zeros(1) if table else None)
        return s
    for other in (single(size=(40, 40)), single(log2_table=11), single(num_bits=8), single(level_bits=(8,) * 4), single(hidden=32), single(n_linear=5),
                  single(frozen=True), single(table=False)):
        with pytest.raises(ValueError, match="insert"):
            f.insert(1, other)
    with pytest.raises(ValueError, match="insert"):
        bare(num_bits=8).insert(1, single(num_bits=4))
    assert f.__dict__ == before                                   # nothing was set on the way to a refusal
