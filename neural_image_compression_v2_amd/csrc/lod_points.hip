// The hash-grid field at points with a LEVEL OF DETAIL per point (include/nicv2_hip.h: nic_hash_lod, nic_hash_encode_points_lod / _backward_lod,
// nic_hash_fused_forward_points_lod, nic_hash_fused_forward_backward_points_lod; hashgrid.py, HashGridField.query / train_points(lod=), decode_mip,
// fit_mips).  lambda of a point = (lod ? lod[n] : 0) + lod_uniform, NaN -> 0, clamped to [0, 32]; level l of that point weighs
// a_l = min(max((fade[l] - lambda) + 1, 0), 1) and column l F + f of its row is fl(a_l r), r the value of hash_points.hip (blend, plus noise).
// Positions, cells, entry index, sources, noise keys and the meaning of `order` are those kernels', through the same helpers of hash_common.hpp.
//
//   skip      a level no lane of the wave weighs above 0 is jumped over by the whole wave (a ballot): no cell arithmetic, no gather, no noise,
//             no atomic - its stored offsets still advance.  Inside a live level a lane of weight 0 reads nothing and writes zeros.
//   noise     the generator block of columns (l F) & ~15 .. is made by the first LIVE level of this lane that needs it, not at the block's first
//             column: a skipped level at a block boundary leaves the later levels of the block their noise.
//   backward  the run sums shuffle across the whole wave, so only the ballot skips; a lane of weight 0 takes part in its run with zeros, and a
//             run whose lanes all weigh 0 issues no atomic.
//   fused     hash_points_fused_kernel / hash_points_fused_train_kernel with the weight applied where the row enters the LDS tile and again on
//             d loss / d row before the scatter; the decoder is hash_common.hpp's.
#include <cmath>

#include "hash_common.hpp"

namespace nic {
namespace hlod {
using namespace hcommon;

enum LodSrc { LSRC_F32 = NIC_HASH_SRC_F32, LSRC_U8 = NIC_HASH_SRC_U8, LSRC_BITS = NIC_HASH_SRC_BITS };

struct LodParams {
    nic_hash_desc d;          // extent[a] = S_a, num_crops = 1
    float fade[NIC_HASH_MAX_LEVELS];
    float lod_uniform;
    const float* lod;         // null, or [n]
    const float* points;      // [n, dim]
    int64_t n;
    const int32_t* order;     // null, or [n] row indices (clamped); backward and fused training only
    const float* table;       // LSRC_F32
    const uint8_t* stored;    // LSRC_U8
    const uint32_t* packed;   // LSRC_BITS, 4-byte aligned
    const float* dx;
    float* out;
    float* grad;              // table gradient (fused training: null = frozen table, no scatter)
    NoiseSrc noise;
    uint64_t sample_base;
    float q_scale, q_bias;    // load4fp: (u - q_bias + 1) / q_scale
    int32_t q_bits, q_tight;
    // fused only
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const float* target;
    float* y;
    float* partials;
    float dscale;             // 2 loss_scale / (3 N)
};

// the row lane `pos` of the launch handles: order[pos] clamped into the point set, or pos itself
__device__ __forceinline__ int64_t ordered_row(const LodParams& p, int64_t pos) {
    if (p.order == nullptr) return pos;
    const int64_t i = p.order[pos];
    return i < 0 ? 0 : (i >= p.n ? p.n - 1 : i);
}
__device__ __forceinline__ float point_lambda(const LodParams& p, int64_t n) {
    float v = __fadd_rn(p.lod != nullptr ? p.lod[n] : 0.f, p.lod_uniform);
    v = v == v ? v : 0.f;
    v = v >= 0.f ? v : 0.f;
    return v <= 32.f ? v : 32.f;
}
// one subtract, one add: nothing to contract
__device__ __forceinline__ float level_weight(float fade, float lam) {
    const float a = __fadd_rn(__fsub_rn(fade, lam), 1.0f);
    return a >= 0.f ? (a <= 1.f ? a : 1.f) : 0.f;
}

// encode_levels of hash_points.hip with the weight of `lam` on every level; `sample` keys the noise
template <int D, int F, int SRC, bool NOISE, bool TIGHT, bool VEC>
__device__ __forceinline__ void encode_levels_lod(const LodParams& p, const uint32_t (&t)[3], uint64_t sample, float lam, float* row) {
    const nic_hash_desc& d = p.d;
    const uint32_t S = (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const float fdiv = (float)(256u * S);
    [[maybe_unused]] int64_t lev_off = 0;              // LSRC_U8: byte offset of level l = F * sum_{k<l} E_k
    [[maybe_unused]] int64_t lev_dw = 0;               // LSRC_BITS: dword offset of level l = sum_{k<l} ceil(E_k F b / 32)
    [[maybe_unused]] U4 nblk{0u, 0u, 0u, 0u};          // NOISE: the generator block `nblk_id` of this sample (-1: none yet)
    [[maybe_unused]] int nblk_id = -1;
#pragma unroll 2
    for (int l = 0; l < d.levels; ++l) {
        const uint32_t R = (uint32_t)d.resolution[l];
        [[maybe_unused]] const float* tab = nullptr;
        if constexpr (SRC == LSRC_F32) tab = p.table + ((int64_t)l << d.log2_table) * F;
        [[maybe_unused]] const uint8_t* stab = nullptr;
        if constexpr (SRC == LSRC_U8) {
            stab = p.stored + lev_off;
            lev_off += (int64_t)F * hash_level_entries(D, (int32_t)R, d.log2_table);
        }
        [[maybe_unused]] const uint32_t* btab = nullptr;
        if constexpr (SRC == LSRC_BITS) {
            btab = p.packed + lev_dw;
            lev_dw += hash_level_dwords(D, (int32_t)R, d.log2_table, F, p.q_bits);
        }
        const float a = level_weight(p.fade[l], lam);
        float acc[F];
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = 0.f;
        if (__ballot(a > 0.f) != 0ull && a > 0.f) {    // the ballot is wave-uniform: a level no lane needs costs the wave nothing below
            const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
            uint32_t v[3];
            float w[3];
            point_cell<D>(t, R, S, fdiv, v, w);
#pragma unroll
            for (int c = 0; c < (1 << D); ++c) {
                const uint32_t e = hash_index(dense, R, mask, v[0] + (c & 1), v[1] + ((c >> 1) & 1), D == 3 ? v[2] + ((c >> 2) & 1) : 0u);
                float tv[F];
                if constexpr (SRC == LSRC_U8) load_row_u8<F>(stab + (int64_t)e * F, p.q_scale, p.q_bias, tv);
                else if constexpr (SRC == LSRC_BITS) load_row_bits<F, TIGHT>(btab, e, p.q_bits, p.q_scale, p.q_bias, tv);
                else load_row<F>(tab + (int64_t)e * F, tv);
                const float cw = corner_weight<D>(w, c);
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] += cw * tv[f];
            }
            if constexpr (NOISE) {
                // 16 % F == 0: a level's F columns lie in one block, made by the first live level of the block
                const int c0 = l * F;
                if ((c0 >> 4) != nblk_id) {
                    nblk_id = c0 >> 4;
                    nblk = noise_block(p.noise, sample, nblk_id);
                }
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] += noise_from_block(p.noise, nblk, (c0 + f) & 15);
            }
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] = __fmul_rn(a, acc[f]);
        }
        if constexpr (VEC) {
            store_row<F>(row + l * F, acc);
        } else {
#pragma unroll
            for (int f = 0; f < F; ++f) row[l * F + f] = acc[f];
        }
    }
}
// b is uniform over the launch: the width of the packed window is decided once per row, not per corner
template <int D, int F, int SRC, bool NOISE, bool VEC>
__device__ __forceinline__ void encode_point_lod(const LodParams& p, const uint32_t (&t)[3], uint64_t sample, float lam, float* row) {
    if constexpr (SRC == LSRC_BITS) {
        if (p.q_tight) encode_levels_lod<D, F, SRC, NOISE, true, VEC>(p, t, sample, lam, row);
        else encode_levels_lod<D, F, SRC, NOISE, false, VEC>(p, t, sample, lam, row);
    } else {
        encode_levels_lod<D, F, SRC, NOISE, false, VEC>(p, t, sample, lam, row);
    }
}

// scatter_point of hash_common.hpp with the weight of `lam`: `grow(l, g)` hands over the F gradient values of level l, weighed here.  The whole
// wave must call this together (shuffles), so a level is skipped only when the ballot finds no lane for it.
template <int D, int F, class GRow>
__device__ __forceinline__ void scatter_point_lod(const LodParams& p, const uint32_t (&t)[3], float lam, bool live, int lane, GRow grow) {
    const nic_hash_desc& d = p.d;
    const uint32_t S = (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const float fdiv = (float)(256u * S);
    for (int l = 0; l < d.levels; ++l) {
        const float a = live ? level_weight(p.fade[l], lam) : 0.f;
        if (__ballot(a > 0.f) == 0ull) continue;
        const uint32_t R = (uint32_t)d.resolution[l];
        const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
        float* gtab = p.grad + ((int64_t)l << d.log2_table) * F;
        uint32_t v[3];
        float w[3];
        point_cell<D>(t, R, S, fdiv, v, w);
        float g[F];
#pragma unroll
        for (int f = 0; f < F; ++f) g[f] = 0.f;
        if (a > 0.f) {
            grow(l, g);
#pragma unroll
            for (int f = 0; f < F; ++f) g[f] = __fmul_rn(a, g[f]);
        }
        const int64_t key = (int64_t)v[0] + ((int64_t)R + 1) * ((int64_t)v[1] + ((int64_t)R + 1) * (int64_t)v[2]);
        const RunMasks m = run_masks(live ? key : -1 - (int64_t)lane, lane);
        float weighed = a > 0.f ? 1.f : 0.f;            // lanes of this run with something to add
        if (m.any_shared) weighed = run_sum(weighed, m);
        const bool issue = live && m.head && weighed > 0.f;
#pragma unroll
        for (int c = 0; c < (1 << D); ++c) {
            const uint32_t e = hash_index(dense, R, mask, v[0] + (c & 1), v[1] + ((c >> 1) & 1), D == 3 ? v[2] + ((c >> 2) & 1) : 0u);
            const float cw = corner_weight<D>(w, c);
#pragma unroll
            for (int f = 0; f < F; ++f) {
                float val = cw * g[f];
                if (m.any_shared) val = run_sum(val, m);
                if (issue) atomicAdd(gtab + (int64_t)e * F + f, val);
            }
        }
    }
}

template <int D, int F, int SRC, bool NOISE>
__global__ void __launch_bounds__(256) hash_lod_encode_kernel(const LodParams p) {
    const int LF = p.d.levels * F;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < p.n; n += (int64_t)gridDim.x * 256) {
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, n, t);
        encode_point_lod<D, F, SRC, NOISE, true>(p, t, p.sample_base + (uint64_t)n, point_lambda(p, n), p.out + n * LF);
    }
}

template <int D, int F>
__global__ void __launch_bounds__(256) hash_lod_backward_kernel(const LodParams p) {
    const int lane = threadIdx.x & 63;
    const int LF = p.d.levels * F;
    for (int64_t nb = (int64_t)blockIdx.x * 256; nb < p.n; nb += (int64_t)gridDim.x * 256) {      // block-uniform trip count: the shuffles see whole waves
        const int64_t pos = nb + threadIdx.x;
        const bool live = pos < p.n;
        const int64_t n = ordered_row(p, live ? pos : p.n - 1);                                     // a dead lane reads the last point, adds nothing
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, n, t);
        const float* drow = p.dx + n * LF;
        scatter_point_lod<D, F>(p, t, point_lambda(p, n), live, lane, [&](int l, float (&g)[F]) { load_row<F>(drow + l * F, g); });
    }
}

// hash_points_fused_kernel (hash_points.hip) with the weighed row, one wave per 64 consecutive points
template <int D, int F, int SRC>
__global__ void __launch_bounds__(256) hash_lod_fused_kernel(const LodParams p) {
    __shared__ DecoderSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    load_decoder(sm, p.w1, p.b1, p.w2, p.b2, p.w3, p.b3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;

    // each XCD (blocks b, b + 8, ..) walks one contiguous range of groups of 4 waves of points
    const int64_t n_waves = (p.n + 63) >> 6;
    const int xcd = blockIdx.x & 7, nb8 = gridDim.x >> 3;
    const int64_t n_groups = (n_waves + 3) >> 2, chunk = (n_groups + 7) >> 3;
    const int64_t g_begin = xcd * chunk, g_end = g_begin + chunk < n_groups ? g_begin + chunk : n_groups;
    const int ks1 = (LF + 1) >> 1;
    for (int64_t g = g_begin + (blockIdx.x >> 3); g < g_end; g += nb8) {
        const int64_t wv = 4 * g + wave;
        if (wv >= n_waves) continue;                            // wave-uniform; nothing below synchronises the workgroup
        const int64_t n0 = wv << 6, n_raw = n0 + lane, row = n_raw < p.n ? n_raw : p.n - 1;
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, row, t);                  // a lane past the end decodes the last point; its output is not stored
        encode_point_lod<D, F, SRC, false, false>(p, t, 0u, point_lambda(p, row), xrow);
        wave_sync();
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            const int64_t n = n0 + 32 * nt + j;
            float yv[3];
            decoder_forward_half(sm, xs, nt, j, half, ks1, yv);
            if (half == 0 && n < p.n) {
#pragma unroll
                for (int o = 0; o < 3; ++o) p.y[n * 3 + o] = yv[o];
            }
        }
        wave_sync();
    }
}

// hash_points_fused_train_kernel (hash_points_train.hip) with the weighed row and the weighed row gradient
template <int D, int F, int KT, bool NOISE>
__global__ void __launch_bounds__(256) hash_lod_fused_train_kernel(const LodParams p) {
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

    // each XCD (blocks b, b + 8, ..) walks one contiguous range of groups of 4 waves of (ordered) points
    const int64_t n_waves = (p.n + 63) >> 6;
    const int xcd = blockIdx.x & 7, nb8 = gridDim.x >> 3;
    const int64_t n_groups = (n_waves + 3) >> 2, chunk = (n_groups + 7) >> 3;
    const int64_t g_begin = xcd * chunk, g_end = g_begin + chunk < n_groups ? g_begin + chunk : n_groups;
    const int ks1 = (LF + 1) >> 1;
    for (int64_t g = g_begin + (blockIdx.x >> 3); g < g_end; g += nb8) {
        const int64_t wv = 4 * g + wave;
        if (wv >= n_waves) continue;                            // wave-uniform; nothing below synchronises the workgroup
        const int64_t pos = (wv << 6) + lane;
        const bool live_lane = pos < p.n;
        const int64_t row = ordered_row(p, live_lane ? pos : p.n - 1);       // a lane past the end takes the last point; it stores and adds nothing
        const float lam = point_lambda(p, row);
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, row, t);
        encode_point_lod<D, F, LSRC_F32, NOISE, false>(p, t, p.sample_base + (uint64_t)row, lam, xrow);
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
            scatter_point_lod<D, F>(p, t, lam, live_lane, lane, [&](int l, float (&gv)[F]) {
#pragma unroll
                for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
            });
        wave_sync();
    }
    write_record<KT>(sm, A, LF, p.partials + (int64_t)blockIdx.x * RecLayout(LF).rec, tid);
}

// ---- host side (the descriptor checks and grid rules are hash_common.hpp's) -------------------------------------------------------------
static int check_lod(const nic_hash_desc* d, const nic_hash_lod* lp) {
    for (int l = 0; l < d->levels; ++l)
        if (!std::isfinite(lp->fade[l]) || lp->fade[l] < 0.f) return NIC_E_ARG;
    if (!std::isfinite(lp->lod_uniform) || lp->reserved != 0) return NIC_E_ARG;
    return NIC_OK;
}
static void set_lod(LodParams& p, const nic_hash_lod* lp, const float* lod) {
    for (int l = 0; l < NIC_HASH_MAX_LEVELS; ++l) p.fade[l] = l < p.d.levels ? lp->fade[l] : 0.f;
    p.lod_uniform = lp->lod_uniform;
    p.lod = lod;
}
// the table source into the parameters, as in hash_points.hip: NIC_E_ARG in the order of the _u8 / _bits siblings (bit depth, alignment)
static int set_source(LodParams& p, const nic_hash_source* src) {
    if (src->kind == NIC_HASH_SRC_F32) {
        if (src->num_bits != 0) return NIC_E_ARG;
        p.table = (const float*)src->data;
        return NIC_OK;
    }
    if (src->kind != NIC_HASH_SRC_U8 && src->kind != NIC_HASH_SRC_BITS) return NIC_E_ARG;
    if (src->num_bits < 1 || src->num_bits > 8) return NIC_E_ARG;
    set_dequant(p, src->num_bits);
    if (src->kind == NIC_HASH_SRC_U8) {
        p.stored = (const uint8_t*)src->data;
        return NIC_OK;
    }
    if ((uintptr_t)src->data & 3u) return NIC_E_ARG;                 // the gather reads aligned dwords
    p.packed = (const uint32_t*)src->data;
    p.q_bits = src->num_bits;
    p.q_tight = hash_bits_tight(p.d.features, src->num_bits) ? 1 : 0;
    return NIC_OK;
}

enum LodKernel { LK_FWD, LK_FWD_NOISY, LK_BWD, LK_FUSED, LK_TRAIN, LK_TRAIN_NOISY };

template <int K, int SRC, int D, int F>
static void launch_k(const LodParams& p, int nb, hipStream_t s) {
    if constexpr (K == LK_BWD) {
        hipLaunchKernelGGL((hash_lod_backward_kernel<D, F>), dim3(nb), dim3(256), 0, s, p);
    } else if constexpr (K == LK_FUSED) {
        hipLaunchKernelGGL((hash_lod_fused_kernel<D, F, SRC>), dim3(nb), dim3(256), 0, s, p);
    } else if constexpr (K == LK_FWD_NOISY) {
        hipLaunchKernelGGL((hash_lod_encode_kernel<D, F, LSRC_F32, true>), dim3(nb), dim3(256), 0, s, p);
    } else if constexpr (K == LK_FWD) {
        hipLaunchKernelGGL((hash_lod_encode_kernel<D, F, SRC, false>), dim3(nb), dim3(256), 0, s, p);
    } else {
        constexpr bool NOISE = K == LK_TRAIN_NOISY;
        if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_lod_fused_train_kernel<D, F, 2, NOISE>), dim3(nb), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((hash_lod_fused_train_kernel<D, F, 1, NOISE>), dim3(nb), dim3(256), 0, s, p);
    }
}
template <int K, int SRC, int D>
static void launch_f(const LodParams& p, int nb, hipStream_t s) {
    switch (p.d.features) {
        case 1: launch_k<K, SRC, D, 1>(p, nb, s); break;
        case 2: launch_k<K, SRC, D, 2>(p, nb, s); break;
        case 4: launch_k<K, SRC, D, 4>(p, nb, s); break;
        default: launch_k<K, SRC, D, 8>(p, nb, s); break;
    }
}
template <int K, int SRC>
static int launch_d(const LodParams& p, int nb, void* stream) {
    if (p.d.dim == 2) launch_f<K, SRC, 2>(p, nb, (hipStream_t)stream);
    else launch_f<K, SRC, 3>(p, nb, (hipStream_t)stream);
    return (int)hipGetLastError();
}
template <int K>
static int launch_src(const LodParams& p, int kind, int nb, void* stream) {
    if (kind == NIC_HASH_SRC_U8) return launch_d<K, LSRC_U8>(p, nb, stream);
    if (kind == NIC_HASH_SRC_BITS) return launch_d<K, LSRC_BITS>(p, nb, stream);
    return launch_d<K, LSRC_F32>(p, nb, stream);
}

}  // namespace hlod
}  // namespace nic

using namespace nic;
using namespace nic::hlod;

extern "C" {

int nic_hash_encode_points_lod(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_source* src, const nic_hash_quant* quant,
                               const float* points, const float* lod, int64_t n_points, float* out, void* stream) {
    int rc = check_point_desc(desc);
    if (rc) return rc;
    if (!src || !src->data || !lodp || !points || !out) return NIC_E_NULL;
    if ((rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    LodParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.out = out;
    set_lod(p, lodp, lod);
    if ((rc = set_source(p, src)) != NIC_OK) return rc;
    if (quant && src->kind != NIC_HASH_SRC_F32) return NIC_E_ARG;        // noise belongs to training, which reads the fp32 table
    if ((rc = set_noise(quant, true, p.noise, p.sample_base)) != NIC_OK) return rc;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    if (p.noise.mode == NIC_NOISE_KERNEL) return launch_d<LK_FWD_NOISY, LSRC_F32>(p, strided_grid((n_points + 63) >> 6), stream);
    return launch_src<LK_FWD>(p, src->kind, strided_grid((n_points + 63) >> 6), stream);
}

int nic_hash_encode_points_backward_lod(const nic_hash_desc* desc, const nic_hash_lod* lodp, const float* points, const float* lod, int64_t n_points,
                                        const float* dx, const int32_t* order, float* table_grad, void* stream) {
    int rc = check_point_desc(desc);
    if (rc) return rc;
    if (!lodp || !points || !dx || !table_grad) return NIC_E_NULL;
    if ((rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    if (n_points < 0 || (order && n_points >= (int64_t(1) << 31))) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    LodParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.dx = dx; p.order = order; p.grad = table_grad;
    set_lod(p, lodp, lod);
    return launch_d<LK_BWD, LSRC_F32>(p, strided_grid((n_points + 63) >> 6), stream);
}

int nic_hash_fused_forward_points_lod(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_source* src, const float* points,
                                      const float* lod, int64_t n_points, const nic_mlp* mlp, float* y, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((rc = check_point_desc(desc)) != NIC_OK) return rc;
    if (!src || !src->data || !lodp || !points || !y) return NIC_E_NULL;
    for (int i = 0; i < 3; ++i)
        if (!mlp->w[i] || !mlp->b[i]) return NIC_E_NULL;
    if ((rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    LodParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.y = y;
    set_lod(p, lodp, lod);
    if ((rc = set_source(p, src)) != NIC_OK) return rc;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
    return launch_src<LK_FUSED>(p, src->kind, persistent_grid((n_points + 63) >> 6), stream);
}

int nic_hash_fused_forward_backward_points_lod(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_quant* quant, const float* table,
                                               const float* points, const float* lod, int64_t n_points, const int32_t* order, const nic_mlp* mlp,
                                               const float* target, float loss_scale, float* table_grad, const nic_mlp_grads* mlp_grads, float* loss,
                                               float* y, int flags, void* workspace, size_t workspace_bytes, const nic_step_tail* tail, void* stream) {
    const KernelEndDrop end;
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((rc = check_point_desc(desc)) != NIC_OK) return rc;
    bool mlp_ok = true;
    for (int i = 0; i < 3; ++i) mlp_ok = mlp_ok && mlp->w[i] && mlp->b[i];
    if (!lodp || !table || !points || !mlp_ok || !target || !mlp_grads || !loss || !workspace) return NIC_E_NULL;
    if ((rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    if (flags & ~(NIC_HASH_FUSED_ADD_GRADS | NIC_HASH_FUSED_ADD_LOSS)) return NIC_E_ARG;
    LodParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.order = order; p.table = table; p.target = target; p.grad = table_grad; p.y = y;
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
    set_lod(p, lodp, lod);
    p.noise.mode = NIC_NOISE_NONE;
    if ((rc = set_noise(quant, true, p.noise, p.sample_base)) != NIC_OK) return rc;
    if (n_points < 0 || (order && n_points >= (int64_t(1) << 31))) return NIC_E_ARG;
    const int lf = desc->levels * desc->features;
    const RecLayout rl(lf);
    if (workspace_bytes < (size_t)wg_cap() * rl.rec * sizeof(float)) return NIC_E_WORKSPACE;
    // the optimiser tail (nic_hash_fused_forward_backward): a decoder entry's gradient is one of the buffers this call's reduction writes
    const int reduce_blocks = (rl.rec + 31) / 32;
    StepTail tl;
    tl.t.count = 0; tl.t.sched = nullptr; tl.n_stream = 0; tl.reduce_blocks = 0x7fffffff;
    int64_t tail_blocks = 0;
    if (tail) {
        if (!tail->tensors) return NIC_E_NULL;
        if (tail->count < 1 || tail->count > NIC_ADAM_MAX_TENSORS || tail->n_stream < 0 || tail->n_stream > tail->count) return NIC_E_ARG;
        if (tail->sched != nullptr) return NIC_E_ARG;                 // the device schedule belongs to the captured dense step
        for (int i = tail->n_stream; i < tail->count; ++i) {
            bool found = false;
            for (int k = 0; k < 3; ++k)
                found = found || (tail->tensors[i].grad != nullptr && (tail->tensors[i].grad == mlp_grads->w[k] || tail->tensors[i].grad == mlp_grads->b[k]));
            if (!found) return NIC_E_ARG;
        }
        rc = adam_build_table(tail->tensors, tail->count, tail->n_stream, tail->beta1, tail->beta2, tail->eps, nullptr, 0, nullptr, tl.t, tl.n_stream,
                              tail_blocks);
        if (rc) return rc;
        tl.reduce_blocks = reduce_blocks;
    }
    if (n_points == 0) return NIC_OK;                                 // nothing to launch: *loss and every gradient stay as they are
    const int grid = persistent_grid((n_points + 63) >> 6);
    const float loss_mul = (float)((double)loss_scale / (3.0 * (double)n_points));
    p.dscale = 2.0f * loss_mul;
    p.partials = (float*)workspace;
    rc = p.noise.mode == NIC_NOISE_KERNEL ? launch_d<LK_TRAIN_NOISY, LSRC_F32>(p, grid, stream) : launch_d<LK_TRAIN, LSRC_F32>(p, grid, stream);
    if (rc) return rc;
    kernel_end_mark((hipStream_t)stream);
    hipLaunchKernelGGL(hfused::hash_fused_reduce_kernel, dim3((unsigned)(reduce_blocks + tail_blocks)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)p.partials, grid, lf, *mlp_grads, loss, loss_mul, (flags & NIC_HASH_FUSED_ADD_GRADS) ? 1 : 0,
                       (flags & NIC_HASH_FUSED_ADD_LOSS) ? 1 : 0, tl);
    return (int)hipGetLastError();
}

}  // extern "C"
