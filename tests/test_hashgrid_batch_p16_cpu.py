"""CPU-only tests of the batched decode on the 16-bit matrix pipe (run with -m "not gpu"): nic_hash_batch_forward_p16 is exported,
declared in the companion header include/nicv2_hip_ext.h (not in nicv2_hip.h, whose 86 entries stay) and mirrored in _lib.EXT_SIGNATURES with the
same argument list, the ABI version stays 9; every argument error of the entry is decided on the host in the documented order (fake pointers and
refusals only: nothing launches; a launch at no points is NIC_OK); the groups rule on the 16-bit kernel's cap; and ``hash_batch_forward_p16`` and
``HashGridFieldBatch.decode / query / resample(precision=)`` refuse on the host, before a device is touched."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
EXT_HEADER = os.path.join(ROOT, "include", "nicv2_hip_ext.h")
NAME = "nic_hash_batch_forward_p16"
UNIT = "hashgrid_fused16.hip"                 # the unit that holds hash_batch16_kernel
NEW_HEADERS = ["hashgrid_batch.hpp"]
OK, NULL, UNSUP, SHAPE, WORKSPACE, ARG = 0, -1, -2, -3, -4, -5
F32, U8, BITS = 0, 1, 2
SPLIT, BF16 = 1, 2
P = ctypes.c_void_p
REC = 64 * 16 + 64 + 64 * 64 + 64 + 3 * 64 + 3 + 1          # one training record at L F = 16: the workspace query counts the cap in these


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


def _src(kind=U8, bits=8, data=16):
    from neural_image_compression_v2_amd._lib import NicHashSource
    return NicHashSource(kind, bits, data)


def _ref(x):
    return None if x is None else ctypes.byref(x)


def _call(lib, d, n_fields=2, groups=0, src="default", origins=0, points=16, n_points=0, m="default", precision=SPLIT, y=16):
    """the return code of the entry; every pointer is a dummy that is never dereferenced.  An accepted call with origins, or with points and
    n_points > 0, would launch: only refusals and n_points == 0 are tried"""
    m = _mlp() if m == "default" else m
    src = _src() if src == "default" else src
    return lib.nic_hash_batch_forward_p16(_ref(d), n_fields, groups, _ref(src), P(origins), P(points), n_points, _ref(m), precision, P(y), None)


def test_the_entry_is_exported_declared_in_the_companion_header_and_mirrored(lib):
    from neural_image_compression_v2_amd import _lib, hashgrid
    import neural_image_compression_v2_amd as pkg
    header, ext = open(HEADER).read(), open(EXT_HEADER).read()
    assert hasattr(lib, NAME)
    assert NAME not in header and NAME not in _lib.SIGNATURES and NAME in _lib.EXT_SIGNATURES
    assert re.search(r'#include\s+"nicv2_hip\.h"', ext)
    res, args = _lib.EXT_SIGNATURES[NAME]
    m = re.search(rf"\b{NAME}\s*\(([^;]*?)\)\s*;", ext, re.S)
    assert m
    cargs = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(cargs) == len(args) == 11 and res is ctypes.c_int, cargs
    for c, a in zip(cargs, args):
        if "*" in c:
            assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), c
        else:
            assert a is {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[c.split()[0]], c
    assert [c.split()[-1].lstrip("*") for c in cargs] == ["desc", "n_fields", "groups_per_field", "src", "origins", "points", "n_points", "mlp", "precision",
                                                         "y", "stream"]
    # every function the companion header declares is mirrored and bound by load(), and nothing else is
    declared = set(re.findall(r"\b(nic_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", ext, flags=re.S)))
    assert declared == set(_lib.EXT_SIGNATURES) and not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    fn = getattr(lib, NAME)
    assert fn.restype is res and list(fn.argtypes) == args                 # load() set them: a stale build fails there
    assert len(_lib.SIGNATURES) == 86                                      # the main header's set is closed
    assert _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version() and re.search(r"#define\s+NIC_ABI_VERSION\s+9\b", header)      # additive
    for name in ("hash_batch_forward_p16", "hash_batch_groups_p16"):
        assert getattr(pkg, name) is getattr(hashgrid, name)
    assert list(inspect.signature(hashgrid.hash_batch_forward_p16).parameters) == [
        "geo", "data", "params", "precision", "kind", "num_bits", "coord", "extent", "points", "groups_per_field", "out"]
    sig = inspect.signature(hashgrid.hash_batch_forward_p16).parameters
    assert sig["precision"].default is inspect.Parameter.empty and sig["kind"].default == "f32" and sig["groups_per_field"].default == 0


def test_precision_defaults_to_none_on_the_three_methods():
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch
    for name, want in (("decode", ["self", "tile", "precision"]), ("query", ["self", "points", "precision"]),
                       ("resample", ["self", "size", "tile", "precision"])):
        sig = inspect.signature(getattr(HashGridFieldBatch, name)).parameters
        assert list(sig) == want and sig["precision"].default is None, name
    assert inspect.signature(HashGridFieldBatch.decode).parameters["tile"].default == 1024
    assert "precision=" in HashGridFieldBatch.__doc__ and "4.7.15" in HashGridFieldBatch.__doc__


def test_the_unit_is_in_the_build_and_restates_no_shared_helper():
    """the unit that holds the new kernel is compiled, builds on the shared headers, and neither it nor the new header defines a helper that
    tests/test_hashgrid_common_cpu.py holds to one definition; what the two batched units share is defined once, in the new header"""
    from neural_image_compression_v2_amd import _build
    import test_hashgrid_common_cpu as common
    assert UNIT in _build.SOURCES and "hashgrid_batch.hip" in _build.SOURCES and len(set(_build.SOURCES)) == len(_build.SOURCES)
    for h in NEW_HEADERS:
        assert h in _build.HEADERS, h                                      # a change of the header rebuilds the units
    texts = {f: open(os.path.join(_build.CSRC, f)).read() for f in [UNIT, "hashgrid_batch.hip"] + NEW_HEADERS}
    for f in [UNIT] + NEW_HEADERS:
        lines = texts[f].splitlines()
        for name in common.FUNCTIONS + list(common.OVERLOADS) + ["split8", "split_acc", "mfma_bf", "mfma_split", "frag_row", "load_decoder", "decoder_forward_half",
                                                                 "lattice_fixed", "persistent_grid", "strided_grid"]:
            assert not any(common._function_re(name).match(ln) for ln in lines), (f, name)
        for name in common.STRUCTS + ["Frag2", "DecoderSmem", "TrainSmem"]:
            assert not any(common._struct_re(name).match(ln) for ln in lines), (f, name)
    unit = texts[UNIT]
    for h in ("hash_common.hpp", "fused_kernel.hpp", "hashgrid_batch.hpp"):
        assert re.search(rf'^\s*#include\s+"{re.escape(h)}"', unit, re.M), h
    assert re.search(r'^\s*#include\s+"hashgrid_batch\.hpp"', texts["hashgrid_batch.hip"], re.M)
    # one definition each of what the batched units share, and of the 16-bit decoder's helpers
    for name, where in (("field_range", "hashgrid_batch.hpp"), ("batch_groups_in", "hashgrid_batch.hpp"), ("batch_groups_of", "hashgrid_batch.hpp"),
                        ("mlp3_ok", "hashgrid_batch.hpp"), ("decoder16_half", UNIT), ("load_decoder16", UNIT), ("position16", UNIT), ("put8", UNIT),
                        ("weight_frag", UNIT), ("product16", UNIT), ("bias_gelu", UNIT), ("p16_grid", UNIT)):
        found = [f for f, t in texts.items() if any(common._function_re(name).match(ln) for ln in t.splitlines())]
        assert found == [where], (name, found)
    for name, where in (("SParams", "hashgrid_batch.hpp"), ("StoredSrc", "hashgrid_batch.hpp"), ("Smem16", UNIT), ("P16Params", UNIT)):
        found = [f for f, t in texts.items() if any(common._struct_re(name).match(ln) for ln in t.splitlines())]
        assert found == [where], (name, found)
    assert sum(len(re.findall(r"\bkMaxFields\s*=", t)) for t in texts.values()) == 1
    # the new kernel: the batched shape around the 16-bit body
    k = unit[unit.index("hash_batch16_kernel(const"):]
    k = k[:k.index("// ---- host side")]
    for call in ("load_decoder16<WIDE>(", "field_range(", "position16<D>(", "encode_point<D, F, SRC, false, false, false>(", "decoder16_half<MODE, WIDE>(",
                 "Smem16<WIDE>", "blockIdx.x / (unsigned)p.groups"):
        assert call in k, call
    assert "atomic" not in k and k.count("__syncthreads()") == 1          # forward only; the one barrier follows the prologue
    assert "POINTS" not in k                                             # the position source is a launch value: 96 instantiations, as the single kernel


def test_argument_errors_in_the_documented_order(lib):
    d = _desc()
    for prec in (SPLIT, BF16):
        assert _call(lib, d, precision=prec) == OK                       # points, n_points == 0: every check passes, nothing launches
    # 1. null desc / mlp, whatever else is wrong
    assert _call(lib, None) == NULL and _call(lib, d, m=None) == NULL
    assert _call(lib, None, n_fields=0, groups=3, src=None, origins=16, precision=7) == NULL
    # 2. the fused set: before the position pair, n_fields, the groups, every pointer and the precision
    bad = _desc()
    bad.flags = 1
    wide = _desc(resolutions=(16,) * 9, features=8)                       # L F = 72
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (_desc(extent=(257, 8, 1)), SHAPE),
                       (_desc(num_crops=0), SHAPE), (wide, UNSUP)]:
        assert _call(lib, desc) == want
        assert _call(lib, desc, origins=16) == want and _call(lib, desc, points=0) == want
        assert _call(lib, desc, n_fields=0, groups=3, src=None, y=0, precision=7) == want
    assert _call(lib, d, m=_mlp(5, 5)) == UNSUP and _call(lib, d, m=_mlp(5, 5), origins=16, n_fields=0) == UNSUP
    # 3. exactly one of origins / points: before the descriptor of the position, n_fields, the groups, the pointers, the source and the precision
    two = _desc(num_crops=2)
    for kw in (dict(origins=16, points=16), dict(origins=0, points=0)):
        assert _call(lib, d, **kw) == ARG
        assert _call(lib, two, **kw) == ARG
        assert _call(lib, d, n_fields=0, groups=3, src=None, y=0, n_points=-1, precision=0, **kw) == ARG
    # 4. the descriptor of that position: points need one crop (SHAPE); both routes need 256 S_max < 2^30 (ARG)
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    assert _call(lib, two) == SHAPE and _call(lib, two, n_fields=0, groups=3, src=None, precision=0) == SHAPE
    assert _call(lib, two, origins=16, points=0, src=None) == NULL       # the lattice takes several crops: on to the pointers
    assert _call(lib, big) == ARG and _call(lib, big, origins=16, points=0) == ARG
    # 5. n_fields
    for n in (0, -1, 65536, 1 << 30):
        assert _call(lib, d, n_fields=n) == ARG and _call(lib, d, n_fields=n, groups=3, src=None, y=0) == ARG
        assert _call(lib, d, n_fields=n, origins=16, points=0) == ARG
    assert _call(lib, d, n_fields=65535) == OK
    # 6. groups_per_field: 0, or a multiple of 8 up to the 16-bit grid of one field's wave items - its patches, or ceil(n_points / 64)
    for g in (-8, -1, 1, 4, 12, 1 << 20):
        assert _call(lib, d, groups=g) == ARG and _call(lib, d, groups=g, src=None, y=0) == ARG, g
        assert _call(lib, d, groups=g, origins=16, points=0, src=None) == ARG, g
    small = _desc(extent=(16, 16, 1))                                     # 4 patches: one group of four, a grid of 8
    assert _call(lib, small, groups=16, origins=16, points=0, src=None) == ARG
    assert _call(lib, small, groups=8, origins=16, points=0, src=None) == NULL
    assert _call(lib, d, groups=16, n_points=130, src=None) == ARG        # 3 wave items: a grid of 8
    assert _call(lib, d, groups=8, n_points=130, src=None) == NULL
    assert _call(lib, d, groups=16, n_points=64 * 4 * 9, src=None) == NULL      # 9 groups of four: a grid of 16
    assert _call(lib, d, groups=8, n_points=0) == OK and _call(lib, d, groups=16, n_points=0) == ARG      # no points count as one item here
    # 7. null pointers: the source, its data, a decoder layer, y - before the source's own rules, the precision and n_points
    for kw in (dict(src=None), dict(src=_src(data=0)), dict(y=0), dict(m=_mlp(3, 2))):
        assert _call(lib, d, **kw) == NULL, kw
        assert _call(lib, d, n_points=-1, precision=0, **kw) == NULL, kw
        assert _call(lib, d, origins=16, points=0, **kw) == NULL, kw
    assert _call(lib, d, src=_src(U8, 0, 0)) == NULL and _call(lib, d, src=_src(BITS, 9, 0)) == NULL
    # 8. the source: nic_hash_encode_points' rules, before the precision and n_points (a bad source at no points is still refused)
    for s in (_src(U8, 0), _src(U8, 9), _src(BITS, 0), _src(BITS, 9), _src(U8, -1), _src(F32, 8), _src(F32, 1), _src(7, 8), _src(-1, 0), _src(BITS, 4, 18),
              _src(BITS, 8, 17)):
        assert _call(lib, d, src=s) == ARG, (s.kind, s.num_bits, s.data)
        assert _call(lib, d, src=s, origins=16, points=0, precision=0) == ARG, (s.kind, s.num_bits, s.data)
    for s in (_src(U8, 1), _src(U8, 8, 17), _src(BITS, 1), _src(BITS, 8, 20), _src(F32, 0), _src(F32, 0, 18)):
        assert _call(lib, d, src=s) == OK, (s.kind, s.num_bits, s.data)
    # 9. the precision: after the null pointers (NIC_E_NULL wins) and the source, before n_points - both neighbours answer NIC_E_ARG too, so what
    # shows is that no bad precision passes: not with a bad source, not at n_points < 0, and not at n_points == 0, where all else is NIC_OK
    for prec in (0, 3, -1):
        assert _call(lib, d, precision=prec) == ARG                      # at n_points == 0 too: no NIC_OK for a precision that does not exist
        assert _call(lib, d, precision=prec, n_points=-1) == ARG
        assert _call(lib, d, precision=prec, origins=16, points=0) == ARG
        assert _call(lib, d, precision=prec, src=None) == NULL           # a null source comes first
        assert _call(lib, d, precision=prec, src=_src(U8, 9)) == ARG
        assert _call(lib, d, precision=prec, n_fields=0) == ARG and _call(lib, two, precision=prec) == SHAPE
    # 10. n_points < 0, then n_points == 0: NIC_OK with no launch (the pointers are fakes: a launch would fault)
    for n in (-1, -64, -(1 << 40)):
        assert _call(lib, d, n_points=n) == ARG
    for desc in (d, _desc(dim=3, resolutions=(4, 6, 9, 12), features=1, s_max=12, extent=(12, 10, 9)), _desc(features=8)):
        for s in (_src(F32, 0), _src(U8, 8), _src(BITS, 3)):
            for prec in (SPLIT, BF16):
                assert _call(lib, desc, src=s, n_points=0, precision=prec) == OK


def test_the_groups_bounds_follow_the_16_bit_cap(lib):
    from neural_image_compression_v2_amd.hashgrid import hash_batch_groups, hash_batch_groups_p16
    cap = lib.nic_hash_fused_workspace_bytes(_ref(_desc()), _ref(_mlp())) // (REC * 4)      # one workgroup per CU, a multiple of 8
    assert cap >= 8 and cap % 8 == 0
    lat = dict(origins=16, points=0, src=None)                            # accepted groups go on to the null source: NIC_E_NULL, no launch
    # L F = 16 <= 32: two workgroups per CU.  4 crops of 256 x 256 = 4096 patches = 1024 groups of four: the single-field grid is 2 cap
    narrow = _desc(num_crops=4)
    assert 1024 >= 2 * cap
    assert _call(lib, narrow, groups=2 * cap, **lat) == NULL and _call(lib, narrow, groups=cap + 8, **lat) == NULL
    assert _call(lib, narrow, groups=2 * cap + 8, **lat) == ARG
    assert _call(lib, narrow, n_fields=1, groups=2 * cap, **lat) == NULL
    n_big = 64 * 4 * 4 * cap                                              # 4 cap groups of four points' waves
    assert _call(lib, _desc(), groups=2 * cap, n_points=n_big, src=None) == NULL
    assert _call(lib, _desc(), groups=2 * cap + 8, n_points=n_big, src=None) == ARG
    one = _desc()                                                         # 1024 patches = 256 groups: the items bound the grid where 2 cap does not
    top = min(256, 2 * cap)
    assert _call(lib, one, groups=top, **lat) == NULL and _call(lib, one, groups=top + 8, **lat) == ARG
    # L F = 64 > 32: one workgroup per CU, as the fp32 kernels
    wide = _desc(num_crops=4, features=8)
    assert _call(lib, wide, groups=cap, **lat) == NULL and _call(lib, wide, groups=cap + 8, **lat) == ARG
    assert _call(lib, _desc(features=8), groups=cap, n_points=n_big, src=None) == NULL
    assert _call(lib, _desc(features=8), groups=cap + 8, n_points=n_big, src=None) == ARG
    # L F = 32 is still narrow, L F = 40 wide (the LDS layout's boundary)
    assert _call(lib, _desc(num_crops=4, resolutions=(16,) * 16), groups=2 * cap, **lat) == NULL
    assert _call(lib, _desc(num_crops=4, resolutions=(16,) * 10, features=4), groups=cap + 8, **lat) == ARG
    # the rule in Python: hash_batch_groups on the doubled cap where L F <= 32
    assert [hash_batch_groups_p16(b, 4096, 256, False) for b in (1, 2, 3, 8, 31, 63, 64, 65, 1000)] == [512, 256, 176, 64, 16, 8, 8, 8, 8]
    assert [hash_batch_groups_p16(b, 4096, 256, True) for b in (1, 2, 3, 8, 31, 32, 33, 64)] == [256, 128, 88, 32, 8, 8, 8, 8]
    assert hash_batch_groups_p16(64, 1024, 256, False) == 8 and hash_batch_groups_p16(8, 1024, 256, False) == 64
    assert hash_batch_groups_p16(1, 1024, 256, False) == 256 and hash_batch_groups_p16(3, 75, 256, False) == 24      # at most one field's own grid
    assert hash_batch_groups_p16(3, 4096, 256, False, 512) == 512 and hash_batch_groups_p16(3, 4096, 256, True, 256) == 256
    for wide_lf, g in ((False, 520), (True, 264), (False, 4), (False, -8)):
        with pytest.raises(ValueError):
            hash_batch_groups_p16(3, 4096, 256, wide_lf, g)
    with pytest.raises(ValueError):
        hash_batch_groups_p16(0, 4096, 256, False)
    for b in (1, 3, 40):
        for items in (4, 75, 1024, 4096):
            assert hash_batch_groups_p16(b, items, 256, True) == hash_batch_groups(b, items, 256)


def _geo(size=(40, 36), levels=4, features=2, log2_table=10):
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, level_resolutions
    return HashGeometry(size, tuple(level_resolutions(levels, 16, max(size))), features, log2_table)


def _params(geo, b=3):
    lf = geo.width
    return [torch.zeros(b, 64, lf), torch.zeros(b, 64), torch.zeros(b, 64, 64), torch.zeros(b, 64), torch.zeros(b, 3, 64), torch.zeros(b, 3)]


def test_the_wrapper_checks_precision_shapes_and_dtypes_before_a_device():
    from neural_image_compression_v2_amd import hashgrid
    geo = _geo()
    params = _params(geo)
    nu8, nb4 = hashgrid.hash_stored_bytes(geo), hashgrid.hash_packed_bytes(geo, 4)
    tables, stored, packed = torch.zeros(3, *geo.table_shape()), torch.zeros(3, nu8, dtype=torch.uint8), torch.zeros(3, nb4, dtype=torch.uint8)
    coord, extent = [[0, 0], [20, 24]], (20, 12)
    fp = hashgrid.hash_batch_forward_p16
    # the precision, whatever else is wrong
    for bad in (None, "fp32", "SPLIT", 1, 2, "", ("split",)):
        with pytest.raises(ValueError, match="precision"):
            fp(geo, stored, params, bad, "u8", 8, coord=coord, extent=extent)
        with pytest.raises(ValueError, match="precision"):
            fp(geo, None, None, bad, "fp16")
    for prec in ("split", "bf16"):
        # the source kind and its num_bits
        with pytest.raises(ValueError, match="source"):
            fp(geo, tables, params, prec, "fp16", coord=coord, extent=extent)
        with pytest.raises(ValueError, match="num_bits"):
            fp(geo, tables, params, prec, "f32", 8, coord=coord, extent=extent)
        for kind, data in (("u8", stored), ("bits", packed)):
            for bits in (None, 0, 9, [4] * 4):
                with pytest.raises(ValueError, match="num_bits"):
                    fp(geo, data, params, prec, kind, bits, coord=coord, extent=extent)
        with pytest.raises(TypeError):
            fp(geo, None, params, prec, "u8", 8, coord=coord, extent=extent)
        # data: fp32 [B, L, T, F], or uint8 [B, bytes of one field at this depth]
        for bad in (tables[0], torch.zeros(3, 4, 512, 2), tables.double(), stored):
            with pytest.raises(ValueError, match="data"):
                fp(geo, bad, params, prec, "f32", coord=coord, extent=extent)
        for bad in (stored[0], stored[:, :-1], stored.to(torch.int8), stored.float(), packed):
            with pytest.raises(ValueError, match="data"):
                fp(geo, bad, params, prec, "u8", 8, coord=coord, extent=extent)
        for bad in (packed[0], stored, torch.zeros(3, hashgrid.hash_packed_bytes(geo, 5), dtype=torch.uint8)):
            with pytest.raises(ValueError, match="data"):
                fp(geo, bad, params, prec, "bits", 4, coord=coord, extent=extent)
        # the decoder: six fp32 tensors stacked like the tables
        for k, shape in enumerate([(3, 64, 9), (3, 32), (3, 64, 32), (2, 64), (3, 64, 3), (3,)]):
            bad = list(params)
            bad[k] = torch.zeros(*shape)
            with pytest.raises(ValueError, match="params"):
                fp(geo, stored, bad, prec, "u8", 8, coord=coord, extent=extent)
        with pytest.raises(ValueError, match="params"):
            fp(geo, stored, [p.double() for p in params], prec, "u8", 8, coord=coord, extent=extent)
        # exactly one position source
        pts = torch.zeros(7, 2)
        with pytest.raises(ValueError, match="exactly one"):
            fp(geo, stored, params, prec, "u8", 8)
        with pytest.raises(ValueError, match="exactly one"):
            fp(geo, stored, params, prec, "u8", 8, coord=coord, extent=extent, points=pts)
        with pytest.raises(ValueError, match="extent"):
            fp(geo, stored, params, prec, "u8", 8, coord=coord)
        with pytest.raises(ValueError, match="extent"):
            fp(geo, stored, params, prec, "u8", 8, points=pts, extent=extent)
        with pytest.raises(IndexError):
            fp(geo, stored, params, prec, "u8", 8, coord=[[21, 0]], extent=extent)
        for bad in (torch.zeros(7), torch.zeros(7, 3), torch.zeros(2, 7, 2), torch.zeros(7, 2, dtype=torch.float64), [[0.0, 0.0]]):
            with pytest.raises(ValueError, match="points"):
                fp(geo, stored, params, prec, "u8", 8, points=bad)
        # out: [B, N, 3] fp32 contiguous
        for bad in (torch.zeros(3, 7, 4), torch.zeros(2, 7, 3), torch.zeros(3, 7, 3, dtype=torch.float64)):
            with pytest.raises(ValueError, match="out"):
                fp(geo, stored, params, prec, "u8", 8, points=pts, out=bad)
        # with everything shaped right the refusal is the device's: nothing was launched
        for kind, data, bits in (("f32", tables, None), ("u8", stored, 8), ("bits", packed, 4)):
            with pytest.raises(RuntimeError, match="HIP device"):
                fp(geo, data, params, prec, kind, bits, coord=coord, extent=extent)
            with pytest.raises(RuntimeError, match="HIP device"):
                fp(geo, data, params, prec, kind, bits, points=torch.zeros(3, 7, 2))


def _batch(decode_only):
    """a batch put together by hand on the CPU: a decode-only one holding uint8 tables, or a trained one holding fp32 tables"""
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch, hash_stored_bytes
    geo = _geo()
    f = HashGridFieldBatch.__new__(HashGridFieldBatch)
    f.n_fields, f.field_size, f.device, f.num_bits, f.frozen, f.geo = 3, (40, 36), torch.device("cpu"), 8, True, geo
    f.groups_per_field, f.steps, f.noise_seed, f._pass_samples, f._grad_clean = 0, 0, 0, 0, True
    f.params, f.optimizer, f.scheduler, f._gm = _params(geo), None, None, None
    if decode_only:
        f.tables, f.packed, f.stored = None, None, torch.zeros(3, hash_stored_bytes(geo), dtype=torch.uint8)
    else:
        f.tables, f.packed, f.stored = torch.zeros(3, *geo.table_shape()), None, None
    return f


@pytest.mark.parametrize("decode_only", [True, False], ids=["decode-only", "trained"])
def test_the_methods_refuse_on_the_host_and_accept_precision_on_both_kinds_of_batch(decode_only):
    f = _batch(decode_only)
    assert f.decode_only == decode_only
    before = dict(f.__dict__)
    pts = torch.zeros(3, 7, 2)
    for bad in ("fp32", "SPLIT", 1, "", ("bf16",)):
        with pytest.raises(ValueError, match="precision"):
            f.decode(precision=bad)
        with pytest.raises(ValueError, match="precision"):
            f.decode(32, bad)
        with pytest.raises(ValueError, match="precision"):
            f.query(pts, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            f.query(None, bad)                                            # before the points are looked at
        with pytest.raises(ValueError, match="precision"):
            f.resample((32, 32), precision=bad)
        with pytest.raises(ValueError, match="precision"):
            f.resample((32, 32, 32), 8, bad)                              # before the size
    for prec in ("split", "bf16"):
        with pytest.raises(ValueError, match="size"):
            f.resample((32, 32, 32), precision=prec)
        for bad in (torch.zeros(7), torch.zeros(7, 3), torch.zeros(2, 7, 2), torch.zeros(7, 2, dtype=torch.float64)):
            with pytest.raises(ValueError, match="points"):
                f.query(bad, precision=prec)
        # everything right: both kinds of batch take the keyword, and the refusal is the device's
        with pytest.raises(RuntimeError, match="HIP device"):
            f.query(pts, precision=prec)
        with pytest.raises(RuntimeError, match="HIP device"):
            f.query(torch.zeros(7, 2), prec)
        with pytest.raises(RuntimeError, match="HIP device"):
            f.decode(precision=prec)
        with pytest.raises(RuntimeError, match="HIP device"):
            f.decode(16, prec)
        with pytest.raises(RuntimeError, match="HIP device"):
            f.resample((8, 8), precision=prec)
    assert f.__dict__.keys() == before.keys() and all(f.__dict__[k] is before[k] for k in before)       # nothing was set on the way to a refusal
