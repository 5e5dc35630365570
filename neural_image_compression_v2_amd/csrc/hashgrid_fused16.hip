// The forward-only fused hash-grid routes (decode, query, resample) with the 64-64-3 decoder on the 16-bit matrix pipe
// (include/nicv2_hip.h: nic_hash_fused_forward_p16; hashgrid.py, precision="split" | "bf16").
//
//   the gather is the existing one: a wave takes 64 samples - a patch of a crop lattice or 64 consecutive points - and runs THE level loop
//   (hash_common.hpp, encode_point) into its LDS row tile, so the row x [L F] is nic_hash_encode / _u8 / _bits' on the lattice and
//   nic_hash_encode_points' at points, bit for bit.
//   the decoder then runs per 32-sample half tile on v_mfma_f32_32x32x16_bf16 with the operand split, the fragments and the k order of
//   fused_kernel.hpp (split8 / split_acc / mfma_split / mfma_bf): per layer z = W a with both operands as hi = bf16(v), lo = bf16(v - hi),
//   P16_SPLIT: lo x hi + hi x lo + hi x hi, P16_BF16: hi x hi alone, fp32 accumulation from zero; the bias, GELU and the output sigmoid are the
//   fp32 route's.  An accumulator tile is the next layer's B fragment as it stands (no lane movement).
//   the loop-invariant weights live in LDS as bf16 hi / lo images in natural [unit][k] order (an A fragment is two 8-byte reads of a row): L F
//   is a launch value, so the layer-1 fragments cannot sit in registers under a compile-time index, and images of at most 36 KB beside row tiles
//   of L F <= 32 columns (WIDE = false) leave the workgroup at 61 KB of LDS - two workgroups per CU, a second wave per SIMD for the gathers.
// B fields of one geometry per launch (include/nicv2_hip_ext.h: nic_hash_batch_forward_p16; hashgrid.py, HashGridFieldBatch.decode / query /
// resample(precision=)): hash_batch16_kernel is the kernel above in hash_batch_decode_kernel's shape (hashgrid_batch.hip) - a
// workgroup belongs to field b = blockIdx.x / G, stages field b's decoder once and walks field b's wave items (field_range); the table, the
// origins or points and y at the field's strides.  Per sample the same encode_point and decoder16_half in the same order: the single kernel's bits.
#include "hash_common.hpp"
#include "fused_kernel.hpp"
#include "hashgrid_batch.hpp"
#include "../../include/nicv2_hip_ext.h"

namespace nic {
namespace hf16 {
using namespace hcommon;

enum { P16_SPLIT = NIC_HASH_PREC_SPLIT, P16_BF16 = NIC_HASH_PREC_BF16 };

struct P16Params {
    nic_hash_desc d;          // lattice: extent = the crop's, num_crops crops; points: extent[a] = S_a, num_crops = 1
    const int32_t* origins;   // lattice: [num_crops, dim]; null = the samples are `points`
    const float* points;      // [n, dim]
    int64_t n;                // points
    int64_t n_waves;          // lattice: patches; points: ceil(n / 64)
    const float* table;       // NIC_HASH_SRC_F32
    const uint8_t* stored;    // NIC_HASH_SRC_U8
    const uint32_t* packed;   // NIC_HASH_SRC_BITS, 4-byte aligned
    float q_scale, q_bias;    // load4fp: (u - q_bias + 1) / q_scale
    int32_t q_bits, q_tight;
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    float* y;
};

// WIDE: L F in 33 .. 64 (k padded to 64), else L F <= 32 (k padded to 32).  Row strides: the fp32 row tile odd (lanes that walk rows hit
// different banks), the bf16 images 2 mod 4 dwords (fused_kernel.hpp, Lds)
template <bool WIDE>
struct Smem16 {
    static constexpr int KP = WIDE ? 64 : 32, XS16 = KP + 1, LD1 = KP + 4, LD2 = kH + 4;
    float x[4][64 * XS16];                 // per wave: the encoding rows [sample][column]; columns past L F stay zero
    float b1[kH], b2[kH], b3[4];
    __attribute__((aligned(8))) __bf16 w1[2][kH * LD1];      // hi, lo; columns past L F are zero
    __attribute__((aligned(8))) __bf16 w2[2][kH * LD2];
    __attribute__((aligned(8))) __bf16 w3[2][4 * LD2];       // rows 0 .. 2 and a zero row for the lanes of output rows 3 .. 31
};

// what position16 and load_decoder16 read of P16Params, for field b of a batch: the shared descriptor by reference, the field's own positions and
// decoder
struct Field16 {
    const nic_hash_desc& d;
    const int32_t* origins;   // [num_crops, dim]; null = the samples are `points`
    const float* points;      // [n, dim]
    int64_t n, n_waves;
    const float *w1, *b1, *w2, *b2, *w3, *b3;
};

// the sample lane `lane` of wave item `wv` handles: its row of y and its fixed-point position.  A lane without a sample (the rim of a patch,
// past the last point) gets the position of a real one; it stores nothing.  P: P16Params, or Field16
template <int D, class P>
__device__ __forceinline__ bool position16(const P& p, int64_t wv, int lane, int64_t& row, uint32_t (&t)[3]) {
    if (p.origins != nullptr) {
        const PatchSample<D> s = patch_sample<D>(p.d, wv, p.n_waves, lane);
        lattice_fixed<D>(p.d, p.origins, s, t);
        row = s.n;
        return s.live;
    }
    row = (wv << 6) + lane;
    const bool live = wv < p.n_waves && row < p.n;
    row = live ? row : p.n - 1;
    point_fixed<D>(p.d, p.points, row, t);
    return live;
}

// 8 consecutive k of one weight row as hi / lo bf16 into the natural-order images
__device__ __forceinline__ void put8(__bf16* hi, __bf16* lo, const float (&v)[8]) {
    const Frag2 f = split8(v);
    const s16x8 h = __builtin_bit_cast(s16x8, f.hi), l = __builtin_bit_cast(s16x8, f.lo);
    *reinterpret_cast<s16x4*>(hi) = s16x4{h[0], h[1], h[2], h[3]};
    *reinterpret_cast<s16x4*>(hi + 4) = s16x4{h[4], h[5], h[6], h[7]};
    *reinterpret_cast<s16x4*>(lo) = s16x4{l[0], l[1], l[2], l[3]};
    *reinterpret_cast<s16x4*>(lo + 4) = s16x4{l[4], l[5], l[6], l[7]};
}
// the decoder's weights as bf16 images (columns past L F zero), the biases, and the wave's row tile cleared; the caller synchronises after it
template <bool WIDE, class P>
__device__ __forceinline__ void load_decoder16(Smem16<WIDE>& sm, const P& p, int LF, int tid) {
    using S = Smem16<WIDE>;
    for (int e = tid; e < kH * (S::KP / 8); e += 256) {
        const int h = e / (S::KP / 8), k0 = 8 * (e - h * (S::KP / 8));
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = k0 + i < LF ? p.w1[h * LF + k0 + i] : 0.f;
        put8(sm.w1[0] + h * S::LD1 + k0, sm.w1[1] + h * S::LD1 + k0, v);
    }
    for (int e = tid; e < kH * (kH / 8); e += 256) {
        const int h = e >> 3, k0 = 8 * (e & 7);
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p.w2[h * kH + k0 + i];
        put8(sm.w2[0] + h * S::LD2 + k0, sm.w2[1] + h * S::LD2 + k0, v);
    }
    if (tid < 4 * (kH / 8)) {
        const int h = tid >> 3, k0 = 8 * (tid & 7);
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = h < 3 ? p.w3[h * kH + k0 + i] : 0.f;
        put8(sm.w3[0] + h * S::LD2 + k0, sm.w3[1] + h * S::LD2 + k0, v);
    }
    if (tid < kH) { sm.b1[tid] = p.b1[tid]; sm.b2[tid] = p.b2[tid]; }
    if (tid < 4) sm.b3[tid] = tid < 3 ? p.b3[tid] : 0.f;
    float* xs = sm.x[tid >> 6];
    for (int e = tid & 63; e < 64 * S::XS16; e += 64) xs[e] = 0.f;
}

// the A fragment of k-step s of image row `row` (this lane's output unit): hi, and lo where the mode multiplies it
template <int MODE>
__device__ __forceinline__ Frag2 weight_frag(const __bf16* hi, const __bf16* lo, int at) {
    Frag2 a;
    a.hi = frag_row((lds_cbf*)(hi + at));
    if constexpr (MODE == P16_SPLIT) a.lo = frag_row((lds_cbf*)(lo + at));
    else a.lo = a.hi;                                   // never multiplied
    return a;
}
template <int MODE>
__device__ __forceinline__ f32x16 product16(const Frag2& a, const Frag2& b, f32x16 c) {
    if constexpr (MODE == P16_SPLIT) return mfma_split(a, b, c);
    else return mfma_bf(a.hi, b.hi, c);
}
template <int T>
__device__ __forceinline__ void bias_gelu(f32x16 (&a)[T], const float* bias, int half) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float av, dv;
            gelu_and_grad(a[t][r] + bias[32 * t + row_of(r, half)], av, dv);
            a[t][r] = av;
        }
}

// y of the sample whose row is `xb` (lane j of a 32-sample half tile) in registers 0 .. 2 of half 0.  k-step s of a product contracts the
// columns 16 s .. 16 s + 15 in the order of split_acc: element e of lane half g is column 16 s + 8 (e >> 2) + 4 g + (e & 3)
template <int MODE, bool WIDE>
__device__ __forceinline__ void decoder16_half(const Smem16<WIDE>& sm, const float* xb, int j, int half, int ks1, float (&yv)[3]) {
    using S = Smem16<WIDE>;
    f32x16 a1[2] = {f32x16{}, f32x16{}};
    for (int s = 0; s < ks1; ++s) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = xb[16 * s + 8 * (e >> 2) + 4 * half + (e & 3)];
        const Frag2 b = split8(x);
#pragma unroll
        for (int t = 0; t < 2; ++t)
            a1[t] = product16<MODE>(weight_frag<MODE>(sm.w1[0], sm.w1[1], (32 * t + j) * S::LD1 + 16 * s + 4 * half), b, a1[t]);
    }
    bias_gelu<2>(a1, sm.b1, half);
    f32x16 a2[2] = {f32x16{}, f32x16{}};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const Frag2 b = split_acc(a1[s >> 1], s & 1);
#pragma unroll
        for (int t = 0; t < 2; ++t)
            a2[t] = product16<MODE>(weight_frag<MODE>(sm.w2[0], sm.w2[1], (32 * t + j) * S::LD2 + 16 * s + 4 * half), b, a2[t]);
    }
    bias_gelu<2>(a2, sm.b2, half);
    f32x16 z3 = f32x16{};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const Frag2 b = split_acc(a2[s >> 1], s & 1);
        z3 = product16<MODE>(weight_frag<MODE>(sm.w3[0], sm.w3[1], (j < 3 ? j : 3) * S::LD2 + 16 * s + 4 * half), b, z3);
    }
#pragma unroll
    for (int o = 0; o < 3; ++o) yv[o] = sigmoid_f(z3[o] + sm.b3[o]);
}

// gather + decoder in one launch (hash_mixed_fused_kernel's shape): 4 waves, a wave per 64 samples, each XCD walking one range of them
template <int D, int F, int SRC, int MODE, bool WIDE>
__global__ void __launch_bounds__(256) hash_fused16_kernel(const P16Params p) {
    using S = Smem16<WIDE>;
    __shared__ S sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F, ks1 = (LF + 15) >> 4;
    load_decoder16<WIDE>(sm, p, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * S::XS16;
    const WaveRange wr = xcd_range(p.n_waves);
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= p.n_waves) continue;                          // wave-uniform; nothing below synchronises the workgroup
        int64_t row;
        uint32_t t[3];
        const bool live_lane = position16<D>(p, wv, lane, row, t);
        encode_point<D, F, SRC, false, false, false>(p, t, row, 0.f, xrow);
        wave_sync();
        const unsigned long long live_mask = __ballot(live_lane);
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            if (((live_mask >> (32 * nt)) & 0xFFFFFFFFull) == 0ull) continue;      // a half tile without a sample (wave-uniform)
            const int src = 32 * nt + j;
            const int64_t r = (int64_t)(uint32_t)__shfl((int)(uint32_t)row, src) | ((int64_t)__shfl((int)(row >> 32), src) << 32);
            float yv[3];
            decoder16_half<MODE, WIDE>(sm, xs + src * S::XS16, j, half, ks1, yv);
            if (half == 0 && ((live_mask >> src) & 1ull)) {
#pragma unroll
                for (int o = 0; o < 3; ++o) p.y[r * 3 + o] = yv[o];
            }
        }
        wave_sync();
    }
}

// the same per field (hash_batch_decode_kernel's shape, hashgrid_batch.hip): workgroup (b, lb) of G per field stages field b's decoder and walks
// field b's wave items; a workgroup without one does nothing after its prologue.  Nothing synchronises across workgroups.
template <int D, int F, int SRC, int MODE, bool WIDE>
__global__ void __launch_bounds__(256) hash_batch16_kernel(const hbatch::SParams p) {
    using S = Smem16<WIDE>;
    __shared__ S sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F, ks1 = (LF + 15) >> 4;
    const int b = (int)(blockIdx.x / (unsigned)p.groups), lb = (int)(blockIdx.x - (unsigned)b * (unsigned)p.groups);
    const Field16 fb{p.d,
                     p.origins != nullptr ? p.origins + (int64_t)b * p.d.num_crops * D : nullptr,
                     p.origins != nullptr ? nullptr : p.points + (int64_t)b * p.n * D,
                     p.n, p.n_items,
                     p.w1 + (int64_t)b * kH * LF, p.b1 + b * kH, p.w2 + (int64_t)b * kH * kH, p.b2 + b * kH, p.w3 + b * 3 * kH, p.b3 + b * 3};
    load_decoder16<WIDE>(sm, fb, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * S::XS16;
    const int64_t tab_off = (int64_t)b * p.stride;
    const hbatch::StoredSrc src_b{p.d,
                                  SRC == NIC_HASH_SRC_F32 ? reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(p.table) + tab_off) : nullptr,
                                  SRC == NIC_HASH_SRC_U8 ? p.stored + tab_off : nullptr,
                                  SRC == NIC_HASH_SRC_BITS ? reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(p.packed) + tab_off) : nullptr,
                                  p.q_scale, p.q_bias, p.q_bits, p.q_tight};
    float* y = p.y + (int64_t)b * p.n_rows * 3;
    const WaveRange wr = hbatch::field_range(p.n_items, lb, p.groups);
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= p.n_items) continue;                          // wave-uniform; nothing below synchronises the workgroup
        int64_t row;
        uint32_t t[3];
        const bool live_lane = position16<D>(fb, wv, lane, row, t);
        encode_point<D, F, SRC, false, false, false>(src_b, t, row, 0.f, xrow);
        wave_sync();
        const unsigned long long live_mask = __ballot(live_lane);
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            if (((live_mask >> (32 * nt)) & 0xFFFFFFFFull) == 0ull) continue;      // a half tile without a sample (wave-uniform)
            const int src = 32 * nt + j;
            const int64_t r = (int64_t)(uint32_t)__shfl((int)(uint32_t)row, src) | ((int64_t)__shfl((int)(row >> 32), src) << 32);
            float yv[3];
            decoder16_half<MODE, WIDE>(sm, xs + src * S::XS16, j, half, ks1, yv);
            if (half == 0 && ((live_mask >> src) & 1ull)) {
#pragma unroll
                for (int o = 0; o < 3; ++o) y[r * 3 + o] = yv[o];
            }
        }
        wave_sync();
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// the lattice route goes through the fixed-point cell too: 256 S_max < 2^30, as at points
static int p16_check_desc(const nic_hash_desc* d, bool at_points) {
    if (at_points) return check_point_desc(d);
    const int rc = check_hash_desc(d);
    if (rc) return rc;
    return 256 * (int64_t)d->S_max >= (int64_t(1) << 30) ? NIC_E_ARG : NIC_OK;
}
// two workgroups fit a CU where L F <= 32 (Smem16<false>: 61 KB): the persistent grid may be twice persistent_grid's
static int p16_grid(int64_t n_waves, bool wide) {
    const int64_t groups = (n_waves + 3) / 4, want = (groups + 7) / 8 * 8, cap = (int64_t)wg_cap() * (wide ? 1 : 2);
    return (int)(want < cap ? want : cap);
}
template <int SRC, int MODE>
static int launch16(const P16Params& p, void* stream) {
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        const hipStream_t s = (hipStream_t)stream;
        if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_fused16_kernel<D, F, SRC, MODE, true>), dim3(p16_grid(p.n_waves, true)), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((hash_fused16_kernel<D, F, SRC, MODE, false>), dim3(p16_grid(p.n_waves, false)), dim3(256), 0, s, p);
    });
}

template <int SRC, int MODE>
static int launch_batch16(const hbatch::SParams& p, int n_fields, void* stream) {
    const dim3 grid((unsigned)n_fields * (unsigned)p.groups);
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        const hipStream_t s = (hipStream_t)stream;
        if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_batch16_kernel<D, F, SRC, MODE, true>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((hash_batch16_kernel<D, F, SRC, MODE, false>), grid, dim3(256), 0, s, p);
    });
}

}  // namespace hf16
}  // namespace nic

using namespace nic;
using namespace nic::hf16;

extern "C" {

int nic_hash_fused_forward_p16(const nic_hash_desc* desc, const nic_hash_source* src, const int32_t* origins, const float* points, int64_t n_points,
                               const nic_mlp* mlp, int precision, float* y, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((origins != nullptr) == (points != nullptr)) return NIC_E_ARG;
    if ((rc = p16_check_desc(desc, points != nullptr)) != NIC_OK) return rc;
    if (!src || !src->data || !y) return NIC_E_NULL;
    for (int i = 0; i < 3; ++i)
        if (!mlp->w[i] || !mlp->b[i]) return NIC_E_NULL;
    P16Params p{};
    p.d = *desc; p.origins = origins; p.points = points; p.y = y;
    p.n = origins ? 0 : n_points;
    p.n_waves = origins ? count_patches(desc) : (n_points + 63) >> 6;
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if (precision != NIC_HASH_PREC_SPLIT && precision != NIC_HASH_PREC_BF16) return NIC_E_ARG;
    if (points && n_points < 0) return NIC_E_ARG;
    if (points && n_points == 0) return NIC_OK;
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
    return dispatch_source(src->kind, [&](auto kind) {
        constexpr int SRC = decltype(kind)::value;
        return precision == NIC_HASH_PREC_SPLIT ? launch16<SRC, P16_SPLIT>(p, stream) : launch16<SRC, P16_BF16>(p, stream);
    });
}

int nic_hash_batch_forward_p16(const nic_hash_desc* desc, int n_fields, int groups_per_field, const nic_hash_source* src, const int32_t* origins,
                               const float* points, int64_t n_points, const nic_mlp* mlp, int precision, float* y, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((origins != nullptr) == (points != nullptr)) return NIC_E_ARG;
    if ((rc = p16_check_desc(desc, points != nullptr)) != NIC_OK) return rc;
    if (n_fields < 1 || n_fields > hbatch::kMaxFields) return NIC_E_ARG;
    // G on the wave items of ONE field under this kernel's cap (p16_grid); a count of points that launches nothing stands as one item here
    const int64_t n_items = origins ? count_patches(desc) : (n_points > 0 ? (n_points + 63) >> 6 : 1);
    const bool wide = desc->levels * desc->features > 32;
    const int g = hbatch::batch_groups_in(p16_grid(n_items, wide), wg_cap() * (wide ? 1 : 2), n_fields, groups_per_field);
    if (g < 0) return NIC_E_ARG;
    if (!src || !src->data || !hbatch::mlp3_ok(mlp) || !y) return NIC_E_NULL;
    hbatch::SParams p{};
    p.d = *desc; p.origins = origins; p.points = points; p.y = y; p.groups = g; p.n_items = n_items;
    p.n = origins ? 0 : n_points;
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if (precision != NIC_HASH_PREC_SPLIT && precision != NIC_HASH_PREC_BF16) return NIC_E_ARG;
    if (points && n_points < 0) return NIC_E_ARG;
    if (points && n_points == 0) return NIC_OK;
    p.stride = hbatch::stacked_source_stride(desc, src);
    if (p.stride <= 0) return NIC_E_ARG;
    p.n_rows = origins ? (int64_t)desc->num_crops * desc->extent[0] * desc->extent[1] * (desc->dim == 3 ? desc->extent[2] : 1) : n_points;
    hbatch::fill_decoder(p, mlp);
    return dispatch_source(src->kind, [&](auto kind) {
        constexpr int SRC = decltype(kind)::value;
        return precision == NIC_HASH_PREC_SPLIT ? launch_batch16<SRC, P16_SPLIT>(p, n_fields, stream) : launch_batch16<SRC, P16_BF16>(p, n_fields, stream);
    });
}

}  // extern "C"
