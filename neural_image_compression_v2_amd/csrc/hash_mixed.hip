// The hash-grid codec with a bit depth PER LEVEL (include/nicv2_hip.h: nic_hash_*_levels; hashgrid.py, HashGridField(num_bits=[..]);
// DESIGN 4.7.6).  Everything is the uniform codec applied per level with b = level_bits[l]: the clamp range, the power-of-two scale of the
// training noise, and the stored format nicv2-hashgrid-bits/2 - format /1 with b replaced by b_l inside level l, so level l of a mixed table
// holds the bytes level l of a /1 table of depth b_l holds.
//
//   one level loop (encode_levels) serves every launch of this file: it is fed a fixed-point position t[3] and per level reads b_l once
//   (uniform over the wave: a scalar load and scalar branches), picks the tight or the straddling window of load_row_bits, carries the level's
//   dword offset as a running sum and, with noise, scales the unchanged generator block by 2^-b_l.
//   one position provider (sample_position) serves both sources, chosen per launch: a lattice sample i of a crop is the point t = 256 i + 128
//   (hash_common.hpp, lattice_fixed: the crop route's row bit for bit), a point goes through point_fixed.  Lattice launches keep one wave per
//   8 x 8 / 4 x 4 x 4 patch with x the fastest lane axis and number rows and noise keys in the crop's sample order; point launches give a
//   wave 64 consecutive (ordered) points.
//   fused training is hash_points_fused_train_kernel's body on those two pieces: encode -> decoder_train_half -> scatter_point ->
//   write_record, then hash_fused_reduce_kernel (hash_fused.hip) with the optimiser tail riding on it.
#include "hash_common.hpp"

namespace nic {
namespace hmixed {
using namespace hcommon;

enum MixedSrc { MSRC_F32 = NIC_HASH_SRC_F32, MSRC_BITS = NIC_HASH_SRC_BITS };

struct MParams {
    nic_hash_desc d;          // lattice: extent = the crop's, num_crops crops; points: extent[a] = S_a, num_crops = 1
    nic_hash_level_bits lb;   // b_l
    uint32_t tight;           // bit l: F b_l divides 32, or is 64 (hash_bits_tight) - no entry of level l leaves the dword(s) it starts in
    const int32_t* origins;   // lattice: [num_crops, dim]; null = the samples are `points`
    const float* points;      // [n, dim]
    int64_t n;                // points
    int64_t n_waves;          // lattice: patches; points: ceil(n / 64)
    const int32_t* order;     // points only: null, or [n] row indices (clamped)
    const float* table;       // MSRC_F32
    const uint32_t* packed;   // MSRC_BITS: format /2, 4-byte aligned
    float* out;
    float* grad;              // table gradient (null = frozen table, no scatter)
    NoiseSrc noise;           // scale is set per level
    uint64_t sample_base;
    // fused only
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const float* target;
    float* y;
    float* partials;
    float dscale;             // 2 loss_scale / (3 N)
};

// the sample lane `lane` of wave item `wv` handles: its row (targets, outputs, noise keys) and fixed-point position.  A lane without a sample
// (the rim of a patch, past the last point) gets the position of a real one; it stores and adds nothing.
template <int D>
__device__ __forceinline__ bool sample_position(const MParams& p, int64_t wv, int lane, int64_t& row, uint32_t (&t)[3]) {
    if (p.origins != nullptr) {
        const PatchSample<D> s = patch_sample<D>(p.d, wv, p.n_waves, lane);
        lattice_fixed<D>(p.d, p.origins, s, t);
        row = s.n;
        return s.live;
    }
    const int64_t pos = (wv << 6) + lane;
    const bool live = wv < p.n_waves && pos < p.n;
    row = ordered_row(p.order, p.n, live ? pos : p.n - 1);
    point_fixed<D>(p.d, p.points, row, t);
    return live;
}

template <int D, int F, bool TIGHT>
__device__ __forceinline__ void blend_bits(const uint32_t* lev, bool dense, uint32_t R, uint32_t mask, const uint32_t (&v)[3], const float (&w)[3],
                                           int bits, float (&acc)[F]) {
    const float scale = (float)((1 << bits) - 1), bias = (float)(1 << (bits - 1));      // load4fp: (u - bias + 1) / scale
#pragma unroll
    for (int c = 0; c < (1 << D); ++c) {
        const uint32_t e = hash_index(dense, R, mask, v[0] + (c & 1), v[1] + ((c >> 1) & 1), D == 3 ? v[2] + ((c >> 2) & 1) : 0u);
        float tv[F];
        load_row_bits<F, TIGHT>(lev, e, bits, scale, bias, tv);
        const float cw = corner_weight<D>(w, c);
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = fmaf(cw, tv[f], acc[f]);
    }
}

// THE level loop.  VEC: the row goes out in F-wide stores (global), else value by value (an LDS tile).  The blend is written as fmaf: the uniform
// kernels' `acc += cw * v` compiles to one fused multiply-add per corner, and bit equality with them must not hang on the vectoriser's choice
// (left free, it split the F = 1 straddling blend into packed multiplies and separate adds: one ulp off)
template <int D, int F, int SRC, bool NOISE, bool VEC>
__device__ __forceinline__ void encode_levels(const MParams& p, const uint32_t (&t)[3], uint64_t sample, float* row) {
    const nic_hash_desc& d = p.d;
    const uint32_t S = (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const float fdiv = (float)(256u * S);
    [[maybe_unused]] int64_t lev_dw = 0;               // MSRC_BITS: dword offset of level l = sum_{k<l} ceil(E_k F b_k / 32)
    [[maybe_unused]] U4 nblk{0u, 0u, 0u, 0u};          // NOISE: the generator block of columns (l F) & ~15 ..
#pragma unroll 2
    for (int l = 0; l < d.levels; ++l) {
        const uint32_t R = (uint32_t)d.resolution[l];
        const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
        [[maybe_unused]] const int bits = p.lb.bits[l];
        uint32_t v[3];
        float w[3];
        point_cell<D>(t, R, S, fdiv, v, w);
        float acc[F];
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = 0.f;
        if constexpr (SRC == MSRC_BITS) {
            const uint32_t* lev = p.packed + lev_dw;
            lev_dw += hash_level_dwords(D, (int32_t)R, d.log2_table, F, bits);
            if ((p.tight >> l) & 1u) blend_bits<D, F, true>(lev, dense, R, mask, v, w, bits, acc);
            else blend_bits<D, F, false>(lev, dense, R, mask, v, w, bits, acc);
        } else {
            const float* tab = p.table + ((int64_t)l << d.log2_table) * F;
#pragma unroll
            for (int c = 0; c < (1 << D); ++c) {
                const uint32_t e = hash_index(dense, R, mask, v[0] + (c & 1), v[1] + ((c >> 1) & 1), D == 3 ? v[2] + ((c >> 2) & 1) : 0u);
                float tv[F];
                load_row<F>(tab + (int64_t)e * F, tv);
                const float cw = corner_weight<D>(w, c);
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] = fmaf(cw, tv[f], acc[f]);
            }
        }
        if constexpr (NOISE) {
            // 16 % F == 0: a level's F columns lie in one generator block; it is generated at its first column and reused by the next levels.
            // Only the scale is the level's: 2^-b_l as an exponent field
            const int c0 = l * F;
            if ((c0 & 15) == 0) nblk = noise_block(p.noise, sample, c0 >> 4);
            NoiseSrc nl = p.noise;
            nl.scale = __uint_as_float((uint32_t)(127 - bits) << 23);
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] += noise_from_block(nl, nblk, (c0 + f) & 15);
        }
        if constexpr (VEC) {
            store_row<F>(row + l * F, acc);
        } else {
#pragma unroll
            for (int f = 0; f < F; ++f) row[l * F + f] = acc[f];
        }
    }
}

// ---- the [N, L F] row: 4 wave items per workgroup, grid-strided ---------------------------------------------------------------------------
template <int D, int F, int SRC, bool NOISE>
__global__ void __launch_bounds__(256) hash_mixed_encode_kernel(const MParams p) {
    const int LF = p.d.levels * F, lane = threadIdx.x & 63;
    for (int64_t wb = (int64_t)blockIdx.x * 4; wb < p.n_waves; wb += (int64_t)gridDim.x * 4) {
        int64_t row;
        uint32_t t[3];
        if (!sample_position<D>(p, wb + (threadIdx.x >> 6), lane, row, t)) continue;
        encode_levels<D, F, SRC, NOISE, true>(p, t, p.sample_base + (uint64_t)row, p.out + row * LF);
    }
}

// ---- gather + decoder in one launch (hash_points_fused_kernel's shape) ----------------------------------------------------------------------
template <int D, int F, int SRC>
__global__ void __launch_bounds__(256) hash_mixed_fused_kernel(const MParams p) {
    __shared__ DecoderSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    load_decoder(sm, p.w1, p.b1, p.w2, p.b2, p.w3, p.b3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;
    const int ks1 = (LF + 1) >> 1;
    const WaveRange wr = xcd_range(p.n_waves);
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= p.n_waves) continue;                          // wave-uniform; nothing below synchronises the workgroup
        int64_t row;
        uint32_t t[3];
        const bool live_lane = sample_position<D>(p, wv, lane, row, t);
        encode_levels<D, F, SRC, false, false>(p, t, 0u, xrow);
        wave_sync();
        const unsigned long long live_mask = __ballot(live_lane);
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            const int src = 32 * nt + j;
            const int64_t r = (int64_t)(uint32_t)__shfl((int)(uint32_t)row, src) | ((int64_t)__shfl((int)(row >> 32), src) << 32);
            float yv[3];
            decoder_forward_half(sm, xs, nt, j, half, ks1, yv);
            if (half == 0 && ((live_mask >> src) & 1ull)) {
#pragma unroll
                for (int o = 0; o < 3; ++o) p.y[r * 3 + o] = yv[o];
            }
        }
        wave_sync();
    }
}

// ---- the fused training step (hash_points_fused_train_kernel's body) ------------------------------------------------------------------------
template <int D, int F, int KT, bool NOISE>
__global__ void __launch_bounds__(256) hash_mixed_fused_train_kernel(const MParams p) {
    __shared__ TrainSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    load_decoder(sm, p.w1, p.b1, p.w2, p.b2, p.w3, p.b3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;
    float* P = sm.p[wave];
    float* Q = sm.q[wave];
    TrainAcc<KT> A;
    A.clear();
    const int ks1 = (LF + 1) >> 1;
    const WaveRange wr = xcd_range(p.n_waves);
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= p.n_waves) continue;                          // wave-uniform; nothing below synchronises the workgroup
        int64_t row;
        uint32_t t[3];
        const bool live_lane = sample_position<D>(p, wv, lane, row, t);
        encode_levels<D, F, MSRC_F32, NOISE, false>(p, t, p.sample_base + (uint64_t)row, xrow);
        wave_sync();
        const unsigned long long live_mask = __ballot(live_lane);
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            const int src = 32 * nt + j;
            const bool mine = half == 0 && ((live_mask >> src) & 1ull);
            const int64_t r = (int64_t)(uint32_t)__shfl((int)(uint32_t)row, src) | ((int64_t)__shfl((int)(row >> 32), src) << 32);
            decoder_train_half<KT>(sm, xs, P, Q, nt, j, half, ks1, mine, p.target + r * 3, p.y != nullptr ? p.y + r * 3 : nullptr, p.dscale,
                                   p.grad != nullptr, A);
        }
        wave_sync();
        if (p.grad != nullptr)
            scatter_point<D, F, false>(p.d, t, p.grad, nullptr, 0.f, live_lane, lane, [&](int l, float (&gv)[F]) {
#pragma unroll
                for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
            });
        wave_sync();
    }
    write_record<KT>(sm, A, LF, p.partials + (int64_t)blockIdx.x * RecLayout(LF).rec, tid);
}

// ---- pack and clamp -------------------------------------------------------------------------------------------------------------------
// fp32 [L, T, F] -> format /2: one output dword per thread, assembled in registers from the values whose bits fall into it (hash_pack_bits_kernel's
// shape and arithmetic per value, with the level's b); the level comes from the dword prefix pre[].  Padding and the two tail dwords come out zero.
struct MPackParams {
    const float* src;
    uint32_t* packed;
    int64_t pre[NIC_HASH_MAX_LEVELS + 1];        // dword offset of level l; pre[levels] = the first tail dword
    int64_t vals[NIC_HASH_MAX_LEVELS];           // E_l F
    nic_hash_level_bits lb;
    int levels, log2_table, features;
};
__global__ void __launch_bounds__(256) hash_mixed_pack_kernel(const MPackParams p) {
    const int64_t n = p.pre[p.levels] + 2;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        int l = 0, bits = p.lb.bits[0];
        int64_t base = 0, vals = p.vals[0];
#pragma unroll
        for (int j = 1; j < NIC_HASH_MAX_LEVELS; ++j) {
            const bool past = j < p.levels && k >= p.pre[j];
            l = past ? j : l;
            base = past ? p.pre[j] : base;
            vals = past ? p.vals[j] : vals;
            bits = past ? p.lb.bits[j] : bits;
        }
        uint32_t w = 0u;
        if (k < p.pre[p.levels]) {
            const uint32_t vmask = (1u << bits) - 1u;
            const float scale = (float)((1 << bits) - 1), bias = (float)((1 << (bits - 1)) - 1);
            const int64_t bit0 = (k - base) << 5;                       // first stream bit of this dword
            const float* src = p.src + ((int64_t)l << p.log2_table) * p.features;
            for (int64_t i = bit0 / bits; i < vals && i * bits < bit0 + 32; ++i) {
                const float v = __fadd_rn(floorf(__fadd_rn(__fmul_rn(src[i], scale), 0.5f)), bias);
                const uint32_t u = (uint32_t)(uint8_t)(int)v & vmask;
                const int at = (int)(i * bits - bit0);                  // -7 .. 31: a value may begin in the dword before
                w |= at >= 0 ? u << at : u >> -at;
            }
        }
        p.packed[k] = w;
    }
}

// level l of the fp32 [L, T, F] table into [-(2^b_l - 1) / 2^(b_l + 1), 1/2] in place (both bounds exact in fp32)
struct MClampParams {
    float* table;
    int64_t n;                // L T F
    int shift;                // log2(T F)
    nic_hash_level_bits lb;
};
__global__ void __launch_bounds__(256) hash_mixed_clamp_kernel(const MClampParams p) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int bits = p.lb.bits[(int)(i >> p.shift)];
        const float lo = -(float)((1 << bits) - 1) * __uint_as_float((uint32_t)(127 - (bits + 1)) << 23);
        p.table[i] = clamp_keep_nan(p.table[i], lo, 0.5f);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// the lattice route goes through the fixed-point cell too: 256 S_max < 2^30, as at points
static int check_position_desc(const nic_hash_desc* d, bool at_points) {
    if (at_points) return check_point_desc(d);
    const int rc = check_hash_desc(d);
    if (rc) return rc;
    return 256 * (int64_t)d->S_max >= (int64_t(1) << 30) ? NIC_E_ARG : NIC_OK;
}
static int check_bits(const nic_hash_desc* d, const nic_hash_level_bits* lb) {
    for (int l = 0; l < d->levels; ++l)
        if (lb->bits[l] < 1 || lb->bits[l] > 8) return NIC_E_ARG;
    return NIC_OK;
}
// sum_l ceil(E_l F b_l / 32); pre (optional) gets the dword offset of every level and the first tail dword at [levels]
static int64_t packed_prefix(const nic_hash_desc* d, const nic_hash_level_bits* lb, int64_t* pre) {
    int64_t off = 0;
    for (int l = 0; l < d->levels; ++l) {
        if (pre) pre[l] = off;
        off += hash_level_dwords(d->dim, d->resolution[l], d->log2_table, d->features, lb->bits[l]);
    }
    if (pre) pre[d->levels] = off;
    return off;
}

// descriptor, level bits and position source into the parameters
static void fill_common(MParams& p, const nic_hash_desc* d, const nic_hash_level_bits* lb, const int32_t* origins, const float* points, int64_t n_points) {
    p.d = *d;
    for (int l = 0; l < d->levels; ++l) {
        p.lb.bits[l] = lb->bits[l];
        if (hash_bits_tight(d->features, lb->bits[l])) p.tight |= 1u << l;
    }
    p.origins = origins; p.points = points;
    p.n = origins ? 0 : n_points;
    p.n_waves = origins ? count_patches(d) : (n_points + 63) >> 6;
    p.noise.mode = NIC_NOISE_NONE;
}
// the table source: F32, or BITS (format /2, 4-byte aligned); src->num_bits must be 0 - the depths are the levels'
static int set_source(MParams& p, const nic_hash_source* src) {
    if (src->kind != NIC_HASH_SRC_F32 && src->kind != NIC_HASH_SRC_BITS) return NIC_E_ARG;
    if (src->num_bits != 0) return NIC_E_ARG;
    if (src->kind == NIC_HASH_SRC_F32) {
        p.table = (const float*)src->data;
        return NIC_OK;
    }
    if ((uintptr_t)src->data & 3u) return NIC_E_ARG;                 // the gather reads aligned dwords
    p.packed = (const uint32_t*)src->data;
    return NIC_OK;
}
enum MKernel { MK_ENC, MK_ENC_NOISY, MK_ENC_BITS, MK_FUSED, MK_FUSED_BITS, MK_TRAIN, MK_TRAIN_NOISY };

template <int K, int D, int F>
static void launch_k(const MParams& p, int nb, hipStream_t s) {
    if constexpr (K == MK_ENC) hipLaunchKernelGGL((hash_mixed_encode_kernel<D, F, MSRC_F32, false>), dim3(nb), dim3(256), 0, s, p);
    else if constexpr (K == MK_ENC_NOISY) hipLaunchKernelGGL((hash_mixed_encode_kernel<D, F, MSRC_F32, true>), dim3(nb), dim3(256), 0, s, p);
    else if constexpr (K == MK_ENC_BITS) hipLaunchKernelGGL((hash_mixed_encode_kernel<D, F, MSRC_BITS, false>), dim3(nb), dim3(256), 0, s, p);
    else if constexpr (K == MK_FUSED) hipLaunchKernelGGL((hash_mixed_fused_kernel<D, F, MSRC_F32>), dim3(nb), dim3(256), 0, s, p);
    else if constexpr (K == MK_FUSED_BITS) hipLaunchKernelGGL((hash_mixed_fused_kernel<D, F, MSRC_BITS>), dim3(nb), dim3(256), 0, s, p);
    else {
        constexpr bool NOISE = K == MK_TRAIN_NOISY;
        if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_mixed_fused_train_kernel<D, F, 2, NOISE>), dim3(nb), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((hash_mixed_fused_train_kernel<D, F, 1, NOISE>), dim3(nb), dim3(256), 0, s, p);
    }
}
template <int K>
static int launch(const MParams& p, int nb, void* stream) {
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        launch_k<K, decltype(dim)::value, decltype(features)::value>(p, nb, (hipStream_t)stream);
    });
}

}  // namespace hmixed
}  // namespace nic

using namespace nic;
using namespace nic::hmixed;

extern "C" {

int64_t nic_hash_packed_bytes_levels(const nic_hash_desc* desc, const nic_hash_level_bits* level_bits) {
    int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (!level_bits) return NIC_E_NULL;
    if ((rc = check_bits(desc, level_bits)) != NIC_OK) return rc;
    return 4 * packed_prefix(desc, level_bits, nullptr) + 8;
}

int nic_hash_pack_bits_levels(const nic_hash_desc* desc, const nic_hash_level_bits* level_bits, const float* table, uint8_t* packed, void* stream) {
    int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (!level_bits || !table || !packed) return NIC_E_NULL;
    if ((rc = check_bits(desc, level_bits)) != NIC_OK) return rc;
    if ((uintptr_t)packed & 3u) return NIC_E_ARG;
    MPackParams p{};
    p.src = table; p.packed = (uint32_t*)packed;
    p.levels = desc->levels; p.log2_table = desc->log2_table; p.features = desc->features;
    packed_prefix(desc, level_bits, p.pre);
    for (int l = 0; l < desc->levels; ++l) {
        p.vals[l] = (int64_t)desc->features * hash_level_entries(desc->dim, desc->resolution[l], desc->log2_table);
        p.lb.bits[l] = level_bits->bits[l];
    }
    const int64_t b = (p.pre[p.levels] + 2 + 255) / 256;
    hipLaunchKernelGGL(hash_mixed_pack_kernel, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int nic_hash_clamp_levels(const nic_hash_desc* desc, const nic_hash_level_bits* level_bits, float* table, void* stream) {
    int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (!level_bits || !table) return NIC_E_NULL;
    if ((rc = check_bits(desc, level_bits)) != NIC_OK) return rc;
    MClampParams p{};
    p.table = table;
    p.shift = desc->log2_table + (desc->features == 1 ? 0 : desc->features == 2 ? 1 : desc->features == 4 ? 2 : 3);
    p.n = (int64_t)desc->levels << p.shift;
    for (int l = 0; l < desc->levels; ++l) p.lb.bits[l] = level_bits->bits[l];
    const int64_t b = (p.n + 255) / 256;
    hipLaunchKernelGGL(hash_mixed_clamp_kernel, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int nic_hash_encode_levels(const nic_hash_desc* desc, const nic_hash_level_bits* level_bits, const nic_hash_source* src, const nic_hash_quant* quant,
                           const int32_t* origins, const float* points, int64_t n_points, float* out, void* stream) {
    int rc = check_hash_desc(desc);
    if (rc) return rc;
    if ((origins != nullptr) == (points != nullptr)) return NIC_E_ARG;
    if ((rc = check_position_desc(desc, points != nullptr)) != NIC_OK) return rc;
    if (!level_bits || !src || !src->data || !out) return NIC_E_NULL;
    if ((rc = check_bits(desc, level_bits)) != NIC_OK) return rc;
    MParams p{};
    fill_common(p, desc, level_bits, origins, points, n_points);
    p.out = out;
    if ((rc = set_source(p, src)) != NIC_OK) return rc;
    if (quant && src->kind != NIC_HASH_SRC_F32) return NIC_E_ARG;        // noise belongs to training, which reads the fp32 table
    if ((rc = set_noise(quant, false, p.noise, p.sample_base)) != NIC_OK) return rc;
    if (points && n_points < 0) return NIC_E_ARG;
    if (points && n_points == 0) return NIC_OK;
    const int nb = strided_grid(p.n_waves);
    if (src->kind == NIC_HASH_SRC_BITS) return launch<MK_ENC_BITS>(p, nb, stream);
    return p.noise.mode == NIC_NOISE_KERNEL ? launch<MK_ENC_NOISY>(p, nb, stream) : launch<MK_ENC>(p, nb, stream);
}

int nic_hash_fused_forward_levels(const nic_hash_desc* desc, const nic_hash_level_bits* level_bits, const nic_hash_source* src, const int32_t* origins,
                                  const float* points, int64_t n_points, const nic_mlp* mlp, float* y, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((origins != nullptr) == (points != nullptr)) return NIC_E_ARG;
    if ((rc = check_position_desc(desc, points != nullptr)) != NIC_OK) return rc;
    if (!level_bits || !src || !src->data || !y) return NIC_E_NULL;
    for (int i = 0; i < 3; ++i)
        if (!mlp->w[i] || !mlp->b[i]) return NIC_E_NULL;
    if ((rc = check_bits(desc, level_bits)) != NIC_OK) return rc;
    MParams p{};
    fill_common(p, desc, level_bits, origins, points, n_points);
    p.y = y;
    if ((rc = set_source(p, src)) != NIC_OK) return rc;
    if (points && n_points < 0) return NIC_E_ARG;
    if (points && n_points == 0) return NIC_OK;
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
    const int grid = persistent_grid(p.n_waves);
    return src->kind == NIC_HASH_SRC_BITS ? launch<MK_FUSED_BITS>(p, grid, stream) : launch<MK_FUSED>(p, grid, stream);
}

int nic_hash_fused_forward_backward_levels(const nic_hash_desc* desc, const nic_hash_level_bits* level_bits, const nic_hash_quant* quant,
                                           const float* table, const int32_t* origins, const float* points, int64_t n_points, const int32_t* order,
                                           const nic_mlp* mlp, const float* target, float loss_scale, float* table_grad,
                                           const nic_mlp_grads* mlp_grads, float* loss, float* y, int flags, void* workspace, size_t workspace_bytes,
                                           const nic_step_tail* tail, void* stream) {
    const KernelEndDrop end;
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((origins != nullptr) == (points != nullptr)) return NIC_E_ARG;
    if (order && !points) return NIC_E_ARG;                              // an order names points
    if ((rc = check_position_desc(desc, points != nullptr)) != NIC_OK) return rc;
    bool mlp_ok = true;
    for (int i = 0; i < 3; ++i) mlp_ok = mlp_ok && mlp->w[i] && mlp->b[i];
    if (!level_bits || !table || !mlp_ok || !target || !mlp_grads || !loss || !workspace) return NIC_E_NULL;
    if ((rc = check_bits(desc, level_bits)) != NIC_OK) return rc;
    if (flags & ~(NIC_HASH_FUSED_ADD_GRADS | NIC_HASH_FUSED_ADD_LOSS)) return NIC_E_ARG;
    MParams p{};
    fill_common(p, desc, level_bits, origins, points, n_points);
    p.order = order; p.table = table; p.target = target; p.grad = table_grad; p.y = y;
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
    if ((rc = set_noise(quant, false, p.noise, p.sample_base)) != NIC_OK) return rc;
    if (points && (n_points < 0 || (order && n_points >= (int64_t(1) << 31)))) return NIC_E_ARG;
    const int lf = desc->levels * desc->features;
    if (workspace_bytes < (size_t)wg_cap() * RecLayout(lf).rec * sizeof(float)) return NIC_E_WORKSPACE;
    FusedTail ft;
    if ((rc = check_fused_tail(tail, mlp_grads, lf, ft)) != NIC_OK) return rc;
    if (points && n_points == 0) return NIC_OK;                       // nothing to launch: *loss and every gradient stay as they are
    const double n_samples = points ? (double)n_points : (double)desc->num_crops * desc->extent[0] * desc->extent[1] * (desc->dim == 3 ? desc->extent[2] : 1);
    const int grid = persistent_grid(p.n_waves);
    const float loss_mul = (float)((double)loss_scale / (3.0 * n_samples));
    p.dscale = 2.0f * loss_mul;
    p.partials = (float*)workspace;
    return finish_fused_step(ft, mlp_grads, flags, lf, grid, loss_mul, loss, p.partials, stream, [&] {
        return p.noise.mode == NIC_NOISE_KERNEL ? launch<MK_TRAIN_NOISY>(p, grid, stream) : launch<MK_TRAIN>(p, grid, stream);
    });
}

}  // extern "C"
