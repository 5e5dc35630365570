// What the units that launch B fields at once share (hashgrid_batch.hip: the fp32 kernels; hashgrid_fused16.hip: the 16-bit forward kernel): the
// walk of a field's wave items by the field's own workgroups, the parameters of a forward launch from stacked sources, and the host rules on the
// number of fields, on G and on the decoder's pointers.  One copy each.
#pragma once
#include "hash_common.hpp"

namespace nic {
namespace hbatch {
using namespace hcommon;

// xcd_range on (lb, G) instead of (blockIdx.x, gridDim.x): each XCD (local blocks x, x + 8, ..) walks one contiguous range of groups of 4 patches
__device__ __forceinline__ WaveRange field_range(int64_t n_waves, int lb, int G) {
    const int xcd = lb & 7;
    const int64_t n_groups = (n_waves + 3) >> 2, chunk = (n_groups + 7) >> 3;
    const int64_t g_begin = xcd * chunk;
    return WaveRange{g_begin + (lb >> 3), g_begin + chunk < n_groups ? g_begin + chunk : n_groups, G >> 3};
}

// what a field's summed squared error is multiplied by for its loss, loss_scale / (3 n), n = the field's OWN samples: the single-field entries'
// expression, in double on either side.  The training kernels' dscale is twice this.  n > 0
__host__ __device__ inline float field_loss_mul(float loss_scale, int64_t n) { return (float)((double)loss_scale / (3.0 * (double)n)); }
// field b's count of points: counts null = every field has n, else counts[b] clamped to [0, n]
__device__ __forceinline__ int64_t field_count(const int32_t* counts, int b, int64_t n) {
    if (counts == nullptr) return n;
    const int64_t c = counts[b];
    return c < 0 ? 0 : (c > n ? n : c);
}

// ---- forward only, from any table source, on the lattice or at points --------------------------------------------------------
struct SParams {
    nic_hash_desc d;          // one field's; at points extent[a] = S_a, num_crops = 1
    int64_t stride;           // bytes from field b's table to field b + 1's
    const int32_t* origins;   // [B, num_crops, dim], or
    const float* points;      // [B, n, dim]
    int64_t n;                // points of one field
    const float* table;       // NIC_HASH_SRC_F32: the base of the stack (set_point_source fills the one of its kind)
    const uint8_t* stored;    // NIC_HASH_SRC_U8
    const uint32_t* packed;   // NIC_HASH_SRC_BITS, 4-byte aligned
    float q_scale, q_bias;    // load4fp: (u - q_bias + 1) / q_scale
    int32_t q_bits, q_tight;
    const float *w1, *b1, *w2, *b2, *w3, *b3;      // bases of the stacked decoder
    float* y;                 // [B, rows, 3]
    int64_t n_items;          // wave items of one field: patches, or groups of 64 points
    int64_t n_rows;           // rows of y per field
    int32_t groups;           // G
};

// what encode_point reads of a stored source, for field b
struct StoredSrc {
    const nic_hash_desc& d;
    const float* table;
    const uint8_t* stored;
    const uint32_t* packed;
    float q_scale, q_bias;
    int32_t q_bits, q_tight;
};

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kMaxFields = 65535;                 // the reduction's blockIdx.y

// G on a launch whose single-field grid is `top` under the workgroup cap `cap`: 0 = cap / B rounded up to a multiple of 8, at least 8, at most
// top; a positive value must be a multiple of 8 within top.  -1: refused
static int batch_groups_in(int top, int cap, int n_fields, int groups_per_field) {
    if (groups_per_field < 0 || (groups_per_field & 7) || groups_per_field > top) return -1;
    if (groups_per_field > 0) return groups_per_field;
    int g = (cap / n_fields + 7) / 8 * 8;
    g = g < 8 ? 8 : g;
    return g < top ? g : top;
}
// the fp32 kernels: one workgroup per CU, the single field's persistent grid
static int batch_groups_of(int64_t n_items, int n_fields, int groups_per_field) {
    return batch_groups_in(persistent_grid(n_items), wg_cap(), n_fields, groups_per_field);
}
static bool mlp3_ok(const nic_mlp* m) {
    for (int i = 0; i < 3; ++i)
        if (!m->w[i] || !m->b[i]) return false;
    return true;
}
// the bases of the stacked decoder, into any parameter struct of a batch
template <class Params>
static void fill_decoder(Params& p, const nic_mlp* mlp) {
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
}
// SParams::stride of a stack of sources of src's kind: fp32 [L, T, F], the compact uint8 table or the bit-packed one.  <= 0: refused
static int64_t stacked_source_stride(const nic_hash_desc* desc, const nic_hash_source* src) {
    return src->kind == NIC_HASH_SRC_F32 ? (((int64_t)desc->levels << desc->log2_table) * desc->features) * (int64_t)sizeof(float)
         : src->kind == NIC_HASH_SRC_U8 ? nic_hash_stored_bytes(desc) : nic_hash_packed_bytes(desc, src->num_bits);
}

}  // namespace hbatch
}  // namespace nic
