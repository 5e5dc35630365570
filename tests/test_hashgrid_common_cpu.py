"""The hash-grid translation units share ONE copy of their helpers (csrc/hash_common.hpp): every helper the five sources
use in common is defined in the header and nowhere else, and every source includes it.  Read from the sources as text; nothing is compiled."""
import glob
import os
import re

from neural_image_compression_v2_amd import _build

HEADER = "hash_common.hpp"
UNITS = ["hash_grid.hip", "hash_fused.hip", "hash_points.hip", "hash_points_train.hip", "hash_mixed.hip"]

FUNCTIONS = ["hash_level_dense", "hash_index", "hash_level_entries", "hash_level_dwords", "hash_bits_tight", "load_row", "store_row", "load_row_u8",
             "load_row_bits", "corner_weight", "patch_sample", "level_cell", "sample_coords", "point_fixed", "point_cell", "wave_sync", "mfma", "row_of",
             "wgrad_mfma", "put_tile", "half_sum", "device_cus", "wg_cap", "check_hash_desc", "check_point_desc", "count_patches", "set_dequant", "set_noise",
             # the level loop and the scatter of a point, with and without a level of detail, and what the point units share around them
             "encode_point_levels", "encode_point", "scatter_point", "ordered_row", "level_weight", "xcd_range", "set_point_source",
             "check_lod", "set_lod", "dispatch_dim_features", "dispatch_source", "check_fused_tail", "finish_fused_step"]
# defined in the header only, as overloads: from LodParams, and (0 / null) from any other parameter struct; point_lambda also from the values
OVERLOADS = {"point_lambda": 3, "level_fade": 2}
STRUCTS = ["PatchSample", "RecLayout", "LodParams", "WaveRange", "FusedTail"]

# a definition opens its line with the specifiers of one (a call never does): [static] [__host__] [__device__] [inline | __forceinline__ |
# constexpr], then the return type, then the name and its parameter list
_SPEC = r"(?:static|__host__|__device__|inline|__forceinline__|constexpr)"


def _function_re(name):
    return re.compile(rf"^\s*(?:{_SPEC}\s+)+[\w:<>,&\*\s]*?\b{name}\s*\(")


def _struct_re(name):
    return re.compile(rf"^\s*struct\s+{name}\b")


def _sources():
    paths = sorted(glob.glob(os.path.join(_build.CSRC, "hash_*")))
    out = {}
    for p in paths:
        with open(p) as f:
            out[os.path.basename(p)] = f.read().splitlines()
    return out


def _definitions(pattern, sources):
    return [(name, i + 1) for name, lines in sources.items() for i, ln in enumerate(lines) if pattern.match(ln)]


def test_the_sources_are_the_ones_the_build_compiles():
    src = _sources()
    assert sorted(src) == sorted(UNITS + [HEADER])
    assert all(u in _build.SOURCES for u in UNITS) and HEADER in _build.HEADERS


def test_every_unit_includes_the_header():
    src = _sources()
    for u in UNITS:
        assert any(re.match(r'\s*#include\s+"hash_common\.hpp"', ln) for ln in src[u]), u


def test_every_shared_helper_is_defined_once_in_the_header():
    src = _sources()
    for name in FUNCTIONS + STRUCTS:
        pattern = _struct_re(name) if name in STRUCTS else _function_re(name)
        found = _definitions(pattern, src)
        assert len(found) == 1 and found[0][0] == HEADER, (name, found)


def test_overloaded_helpers_are_defined_in_the_header_only():
    src = _sources()
    for name, count in OVERLOADS.items():
        found = _definitions(_function_re(name), src)
        assert len(found) == count and all(f[0] == HEADER for f in found), (name, found)


def test_the_definition_pattern_sees_a_definition_and_not_a_call():
    assert _function_re("mfma").match("__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return 0; }")
    assert not _function_re("mfma").match("__device__ __forceinline__ void wgrad_mfma(const float* P) {")
    assert not _function_re("mfma").match("            a1[0] = mfma(sm.w1[j * XS + 2 * k + half], b, a1[0]);")
    assert _function_re("check_hash_desc").match("static int check_hash_desc(const nic_hash_desc* d) {")
    assert _function_re("check_hash_desc").match("inline int check_hash_desc(const nic_hash_desc* d) {")
    assert not _function_re("check_hash_desc").match("    const int rc = check_hash_desc(desc);")
    assert _function_re("hash_index").match("__host__ __device__ inline uint32_t hash_index(bool dense, uint32_t R) {")
    assert not _function_re("hash_index").match("    return (int)hash_index(hash_level_dense(desc->dim, R, desc->log2_table), (uint32_t)R);")
    assert _function_re("patch_sample").match("__device__ __forceinline__ PatchSample<D> patch_sample(const nic_hash_desc& d, int64_t wv) {")
    assert _struct_re("PatchSample").match("struct PatchSample {") and not _struct_re("PatchSample").match("    PatchSample<D> s;")


# ---- the second level walk and the host path of the fused step at points: one definition over all of csrc/  --------------------
WALK_HEADER = "hashgrid_pointgrad.hpp"
WALK_HELPERS = ["point_walk_levels", "point_walk", "lambda_passes", "kept_axes", "store_point_grad", "decoder_dx_half"]
RETIRED = ["point_grad_levels", "point_grad_lod_levels", "point_grad_lod_noisy_levels", "fused_step", "joint_step"]
POINT_GRAD_UNITS = ["hash_points_train.hip", "hashgrid_points_joint.hip", "hashgrid_lodtrain.hip", "hashgrid_pointgrad.hip", "hashgrid_lodgrad.hip"]


def _all_sources():
    out = {}
    for p in sorted(glob.glob(os.path.join(_build.CSRC, "*"))):
        if os.path.isfile(p):
            with open(p) as f:
                out[os.path.basename(p)] = f.read().splitlines()
    return out


def test_the_point_walk_and_the_step_host_path_are_defined_once_in_all_of_csrc():
    src = _all_sources()
    assert WALK_HEADER in src and HEADER in src and all(u in src for u in POINT_GRAD_UNITS)
    assert WALK_HEADER in _build.HEADERS and all(u in _build.SOURCES for u in POINT_GRAD_UNITS)
    for name in WALK_HELPERS:
        found = _definitions(_function_re(name), src)
        assert len(found) == 1 and found[0][0] == WALK_HEADER, (name, found)
    found = _definitions(_function_re("points_fused_step"), src)
    assert len(found) == 1 and found[0][0] == HEADER, found
    for name in RETIRED:
        assert _definitions(_function_re(name), src) == [], name
    for u in POINT_GRAD_UNITS:
        assert not any("atomicAdd" in ln for ln in src[u]), u
    # the pattern sees the definitions it is asked about, and tells the shared step from the retired one
    assert _function_re("point_walk").match("__device__ __forceinline__ void point_walk(const Src& s, const uint32_t (&t)[3], int64_t n) {")
    assert not _function_re("point_walk").match("__device__ __forceinline__ void point_walk_levels(const Src& s, const uint32_t (&t)[3]) {")
    assert _function_re("fused_step").match("static int fused_step(Params& p, const nic_hash_quant* quant) {")
    assert not _function_re("fused_step").match("inline int points_fused_step(Params& p, const nic_hash_quant* quant) {")


# ---- the batched entries at points: one step host path, one gradient-only kernel, one copy of the repeated host snippets -------
BATCH_UNIT, BATCH_GRAD_UNIT, BATCH_HEADER = "hashgrid_batch.hip", "hashgrid_batch_grad.hip", "hashgrid_batch.hpp"
BATCH_ONCE = {"batch_points_step": BATCH_UNIT, "open_batch_points": BATCH_UNIT, "launch_batch_reduce": BATCH_UNIT, "batch_points_grad": BATCH_GRAD_UNIT,
              "stacked_source_stride": BATCH_HEADER, "fill_decoder": BATCH_HEADER}
# the gradient-only pair is one kernel behind one launch; the four training kernels at points stay written out (their merge moved the text of all
# 160 instantiations), so their names and launch helpers are not retired
BATCH_RETIRED = ["hash_batch_points_grad_lod_kernel", "launch_lod"]


def test_the_batch_step_host_path_and_its_helpers_are_defined_once_in_all_of_csrc():
    src = _all_sources()
    assert all(f in src for f in (BATCH_UNIT, BATCH_GRAD_UNIT, BATCH_HEADER, "hashgrid_fused16.hip")) and BATCH_HEADER in _build.HEADERS
    for name, where in BATCH_ONCE.items():
        found = _definitions(_function_re(name), src)
        assert len(found) == 1 and found[0][0] == where, (name, found)
    text = {f: "\n".join(lines) for f, lines in src.items()}
    for name in BATCH_RETIRED:
        assert not any(re.search(rf"\b{name}\b", t) for t in text.values()), name
    # the stride of a stacked source, the six decoder pointers of a batch and the launch of the batched reduction: written out once each
    assert [f for f, t in text.items() if "nic_hash_packed_bytes(desc, src->num_bits)" in t] == [BATCH_HEADER]
    assert sum(t.count("nic_hash_stored_bytes(desc) : nic_hash_packed_bytes(") for t in text.values()) == 1
    batch = [BATCH_UNIT, BATCH_GRAD_UNIT, BATCH_HEADER]
    assert sum(text[f].count("p.w1 = mlp->w[0]") for f in batch) == 1 and "p.w1 = mlp->w[0]" in text[BATCH_HEADER]
    assert sum(t.count("hipLaunchKernelGGL(hash_batch_reduce_kernel") for t in text.values()) == 1
    # the eight entries sit on the shared paths: the four steps on open_batch_points + batch_points_step, the two gradient entries on one function
    unit = text[BATCH_UNIT]
    assert unit.count("open_batch_points(desc, mlp, n_fields, groups_per_field, n_points, g)") == 4 and unit.count("return batch_points_step(p,") == 4
    assert text[BATCH_GRAD_UNIT].count("return batch_points_grad(") == 2 and text[BATCH_GRAD_UNIT].count("__global__") == 1
    for f in (BATCH_UNIT, BATCH_GRAD_UNIT, "hashgrid_fused16.hip"):
        assert "stacked_source_stride(desc, src)" in text[f], f
    # the pattern sees the definitions it is asked about
    assert _function_re("batch_points_step").match("static int batch_points_step(Params& p, const nic_hash_desc* desc) {")
    assert not _function_re("launch_lod").match("static int launch_source_lod(const SLParams& p, int n_fields, void* stream) {")
