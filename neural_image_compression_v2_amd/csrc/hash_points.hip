// The hash-grid field at ARBITRARY points (include/nicv2_hip.h: nic_hash_encode_points / _backward / nic_hash_fused_forward_points; hashgrid.py,
// HashGridField.query / resample / train_points).  A point is `dim` fp32 coordinates in sample units (p = i: the centre of integer
// sample i); it becomes fixed point with 8 fractional bits, t = rint(256 p) + 128 clamped to [0, 256 S - 1], and from there on the cell arithmetic
// is the exact-integer arithmetic of hash_grid.hip with 256 S_max in the place of 2 S_max: q = t R, v = q div 256 S_max, w = fp32(q mod 256 S_max)
// / fp32(256 S_max).  At a sample centre both operands of that quotient are 128 times the lattice route's, so v, w and the row are its, bit for bit.
//
// q < 2^38, but q div / mod 256 S_max needs no 64-bit division: q >> 8 < 2^30 is divided by S_max in 32 bits and the low 8 bits of q re-enter the
// remainder, ((q >> 8) mod S_max) 256 + (q & 255) < 256 S_max < 2^30.
//
// One lane per point, row n = point n, in any order: the run sums of the backward merge whichever NEIGHBOURING lanes share a base vertex (whole
// runs in raster order, none for random points, the whole wave when all points coincide).  The fused decode is hash_fused.hip's forward mode
// with the lane's coordinates taken from the point array.  The helpers are hash_common.hpp's.
//
// With a level of detail per point (nic_hash_lod, nic_hash_encode_points_lod, nic_hash_fused_forward_points_lod): level l of point n
// is weighed by a_l = min(max((fade[l] - lambda_n) + 1, 0), 1), column l F + f of its row is fl(a_l r), r the value without it.  The encode is the
// same kernel on LodParams; the level loop of hash_common.hpp says what a weight of 0 skips.
#include "hash_common.hpp"

namespace nic {
namespace hpoints {
using namespace hcommon;

struct PointParams {
    nic_hash_desc d;          // extent[a] = S_a, num_crops = 1
    const float* points;      // [n, dim]
    int64_t n;
    const float* table;       // NIC_HASH_SRC_F32
    const uint8_t* stored;    // NIC_HASH_SRC_U8
    const uint32_t* packed;   // NIC_HASH_SRC_BITS, 4-byte aligned
    const float* dx;
    float* out;
    float* grad;
    NoiseSrc noise;
    uint64_t sample_base;
    float q_scale, q_bias;    // load4fp: (u - q_bias + 1) / q_scale
    int32_t q_bits, q_tight;
    // fused decode only
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    float* y;
};

// Params: PointParams, or LodParams with a level of detail per point (hash_common.hpp; the level loop and the scatter are the header's)
template <int D, int F, int SRC, bool NOISE, class Params>
__global__ void __launch_bounds__(256) hash_points_encode_kernel(const Params p) {
    const int LF = p.d.levels * F;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < p.n; n += (int64_t)gridDim.x * 256) {
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, n, t);
        encode_point<D, F, SRC, NOISE, true, is_lod<Params>>(p, t, n, point_lambda(p, n), p.out + n * LF);
    }
}

// The loop of hash_common.hpp's scatter_point, written out: calling scatter_point here compiles to other code (the zero fill of a dead lane's
// gradient moves), and that code has not been timed on a GPU
template <int D, int F>
__global__ void __launch_bounds__(256) hash_points_backward_kernel(const PointParams p) {
    const nic_hash_desc& d = p.d;
    const int lane = threadIdx.x & 63;
    const uint32_t S = (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const float fdiv = (float)(256u * S);
    const int LF = d.levels * F;
    for (int64_t nb = (int64_t)blockIdx.x * 256; nb < p.n; nb += (int64_t)gridDim.x * 256) {      // block-uniform trip count: the shuffles see whole waves
        const int64_t n_raw = nb + threadIdx.x;
        const bool live = n_raw < p.n;
        const int64_t n = live ? n_raw : p.n - 1;                                                   // a dead lane reads the last point, adds nothing
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, n, t);
        const float* drow = p.dx + n * LF;
        for (int l = 0; l < d.levels; ++l) {
            const uint32_t R = (uint32_t)d.resolution[l];
            const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
            float* gtab = p.grad + ((int64_t)l << d.log2_table) * F;
            uint32_t v[3];
            float w[3];
            point_cell<D>(t, R, S, fdiv, v, w);
            float g[F];
            if (live) load_row<F>(drow + l * F, g);
            else {
#pragma unroll
                for (int f = 0; f < F; ++f) g[f] = 0.f;
            }
            // runs keyed on the base VERTEX, as in hash_encode_backward_kernel; the lanes of a run may sit anywhere in their cell (each weighs its
            // own gradient before the sum), and only NEIGHBOURING lanes merge, so any point order is right and raster order keeps its long runs
            const int64_t key = (int64_t)v[0] + ((int64_t)R + 1) * ((int64_t)v[1] + ((int64_t)R + 1) * (int64_t)v[2]);
            const RunMasks m = run_masks(live ? key : -1 - (int64_t)lane, lane);
            const bool issue = live && m.head;
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
}

// ---- the fused decode at points: hash_fused_kernel's forward mode (hash_fused.hip), one wave per 64 consecutive points -------------------
// The decoder keeps its own body: hash_common.hpp's load_decoder + decoder_forward_half compile to other code (registers and scratch no worse,
// DESIGN 4.7.7), and that code's results and time against this body have not been measured on a GPU.
template <int D, int F, int SRC>
__global__ void __launch_bounds__(256) hash_points_fused_kernel(const PointParams p) {
    __shared__ DecoderSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    for (int e = tid; e < kH * XS; e += 256) {
        const int h = e / XS, k = e - h * XS;
        sm.w1[e] = k < LF ? p.w1[h * LF + k] : 0.f;
        sm.w2[e] = k < kH ? p.w2[h * kH + k] : 0.f;
    }
    sm.w3[tid] = tid < 3 * kH ? p.w3[tid] : 0.f;
    if (tid < kH) { sm.b1[tid] = p.b1[tid]; sm.b2[tid] = p.b2[tid]; }
    if (tid < 4) sm.b3[tid] = tid < 3 ? p.b3[tid] : 0.f;
    float* xs = sm.x[wave];
    for (int e = lane; e < kH * XS; e += 64) xs[e] = 0.f;       // the columns past L F stay finite (their weights are zero)
    __syncthreads();
    float* xrow = xs + lane * XS;

    const int64_t n_waves = (p.n + 63) >> 6;
    const WaveRange wr = xcd_range(n_waves);
    const int ks1 = (LF + 1) >> 1;
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= n_waves) continue;                            // wave-uniform; nothing below synchronises the workgroup
        const int64_t n0 = wv << 6, n_raw = n0 + lane;
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, n_raw < p.n ? n_raw : p.n - 1, t);    // a lane past the end decodes the last point; its output is not stored
        encode_point<D, F, SRC, false, false, false>(p, t, 0, 0.f, xrow);
        wave_sync();
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            const int src = 32 * nt + j;
            const int64_t n = n0 + src;
            const float* xb = xs + src * XS;
            // ---- layer 1
            f32x16 a1[2] = {f32x16{}, f32x16{}};
            for (int k = 0; k < ks1; ++k) {
                const float b = xb[2 * k + half];
                a1[0] = mfma(sm.w1[j * XS + 2 * k + half], b, a1[0]);
                a1[1] = mfma(sm.w1[(32 + j) * XS + 2 * k + half], b, a1[1]);
            }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float av, dv;
                    gelu_and_grad(a1[tt][r] + sm.b1[32 * tt + row_of(r, half)], av, dv);
                    a1[tt][r] = av;
                }
            // ---- layer 2
            f32x16 a2[2] = {f32x16{}, f32x16{}};
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = 32 * tt + row_of(r, half);
                    a2[0] = mfma(sm.w2[j * XS + k], a1[tt][r], a2[0]);
                    a2[1] = mfma(sm.w2[(32 + j) * XS + k], a1[tt][r], a2[1]);
                }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float av, dv;
                    gelu_and_grad(a2[tt][r] + sm.b2[32 * tt + row_of(r, half)], av, dv);
                    a2[tt][r] = av;
                }
            // ---- output layer: rows 0 .. 2 of one tile (registers 0 .. 2 of half 0)
            f32x16 z3 = f32x16{};
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = 32 * tt + row_of(r, half);
                    z3 = mfma(j < 3 ? sm.w3[j * kH + k] : 0.f, a2[tt][r], z3);
                }
            if (half == 0 && n < p.n) {
#pragma unroll
                for (int o = 0; o < 3; ++o) p.y[n * 3 + o] = sigmoid_f(z3[o] + sm.b3[o]);
            }
        }
        wave_sync();
    }
}

// the same with the weighed row, on the decoder of hash_common.hpp
template <int D, int F, int SRC>
__global__ void __launch_bounds__(256) hash_lod_fused_kernel(const LodParams p) {
    __shared__ DecoderSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    load_decoder(sm, p.w1, p.b1, p.w2, p.b2, p.w3, p.b3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;
    const int64_t n_waves = (p.n + 63) >> 6;
    const WaveRange wr = xcd_range(n_waves);
    const int ks1 = (LF + 1) >> 1;
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= n_waves) continue;                            // wave-uniform; nothing below synchronises the workgroup
        const int64_t n0 = wv << 6, n_raw = n0 + lane, row = n_raw < p.n ? n_raw : p.n - 1;
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, row, t);                  // a lane past the end decodes the last point; its output is not stored
        encode_point<D, F, SRC, false, false, true>(p, t, 0, point_lambda(p, row), xrow);
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

// ---- host side (the descriptor checks and grid rules are hash_common.hpp's) -------------------------------------------------------------
static int check_source(const nic_hash_source* src) {
    if (!src || !src->data) return NIC_E_NULL;
    return NIC_OK;
}

enum PointKernel { PK_FWD, PK_FWD_NOISY, PK_BWD, PK_FUSED };

template <int K, int SRC, class Params>
static int launch(const Params& p, int nb, void* stream) {
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        const hipStream_t s = (hipStream_t)stream;
        if constexpr (K == PK_FUSED && is_lod<Params>) hipLaunchKernelGGL((hash_lod_fused_kernel<D, F, SRC>), dim3(nb), dim3(256), 0, s, p);
        else if constexpr (K == PK_FUSED) hipLaunchKernelGGL((hash_points_fused_kernel<D, F, SRC>), dim3(nb), dim3(256), 0, s, p);
        else if constexpr (K == PK_BWD) hipLaunchKernelGGL((hash_points_backward_kernel<D, F>), dim3(nb), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((hash_points_encode_kernel<D, F, SRC, K == PK_FWD_NOISY, Params>), dim3(nb), dim3(256), 0, s, p);
    });
}
template <int K, class Params>
static int launch_src(const Params& p, int kind, int nb, void* stream) {
    return dispatch_source(kind, [&](auto src) { return launch<K, decltype(src)::value>(p, nb, stream); });
}

}  // namespace hpoints
}  // namespace nic

using namespace nic;
using namespace nic::hpoints;

extern "C" {

int nic_hash_encode_points(const nic_hash_desc* desc, const nic_hash_source* src, const nic_hash_quant* quant, const float* points, int64_t n_points,
                           float* out, void* stream) {
    int rc = check_point_desc(desc);
    if (rc) return rc;
    if ((rc = check_source(src)) != NIC_OK) return rc;
    if (!points || !out) return NIC_E_NULL;
    PointParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.out = out;
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if (quant && src->kind != NIC_HASH_SRC_F32) return NIC_E_ARG;        // noise belongs to training, which reads the fp32 table
    if ((rc = set_noise(quant, true, p.noise, p.sample_base)) != NIC_OK) return rc;
    const bool noisy = p.noise.mode == NIC_NOISE_KERNEL;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    if (noisy) return launch<PK_FWD_NOISY, NIC_HASH_SRC_F32>(p, strided_grid((n_points + 63) >> 6), stream);
    return launch_src<PK_FWD>(p, src->kind, strided_grid((n_points + 63) >> 6), stream);
}

int nic_hash_encode_points_backward(const nic_hash_desc* desc, const float* points, int64_t n_points, const float* dx, float* table_grad, void* stream) {
    const int rc = check_point_desc(desc);
    if (rc) return rc;
    if (!points || !dx || !table_grad) return NIC_E_NULL;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    PointParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.dx = dx; p.grad = table_grad;
    return launch<PK_BWD, NIC_HASH_SRC_F32>(p, strided_grid((n_points + 63) >> 6), stream);
}

int nic_hash_fused_forward_points(const nic_hash_desc* desc, const nic_hash_source* src, const float* points, int64_t n_points, const nic_mlp* mlp,
                                  float* y, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((rc = check_point_desc(desc)) != NIC_OK) return rc;
    if ((rc = check_source(src)) != NIC_OK) return rc;
    if (!points || !y) return NIC_E_NULL;
    for (int i = 0; i < 3; ++i)
        if (!mlp->w[i] || !mlp->b[i]) return NIC_E_NULL;
    PointParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.y = y;
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
    return launch_src<PK_FUSED>(p, src->kind, persistent_grid((n_points + 63) >> 6), stream);
}

// ---- with a level of detail per point: the same checks with those of the nic_hash_lod after the null checks, the same launches ------------
int nic_hash_encode_points_lod(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_source* src, const nic_hash_quant* quant,
                               const float* points, const float* lod, int64_t n_points, float* out, void* stream) {
    int rc = check_point_desc(desc);
    if (rc) return rc;
    if (check_source(src) != NIC_OK || !lodp || !points || !out) return NIC_E_NULL;
    if ((rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    LodParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.out = out;
    set_lod(p, lodp, lod);
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if (quant && src->kind != NIC_HASH_SRC_F32) return NIC_E_ARG;        // noise belongs to training, which reads the fp32 table
    if ((rc = set_noise(quant, true, p.noise, p.sample_base)) != NIC_OK) return rc;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    if (p.noise.mode == NIC_NOISE_KERNEL) return launch<PK_FWD_NOISY, NIC_HASH_SRC_F32>(p, strided_grid((n_points + 63) >> 6), stream);
    return launch_src<PK_FWD>(p, src->kind, strided_grid((n_points + 63) >> 6), stream);
}

int nic_hash_fused_forward_points_lod(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_source* src, const float* points,
                                      const float* lod, int64_t n_points, const nic_mlp* mlp, float* y, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((rc = check_point_desc(desc)) != NIC_OK) return rc;
    if (check_source(src) != NIC_OK || !lodp || !points || !y) return NIC_E_NULL;
    for (int i = 0; i < 3; ++i)
        if (!mlp->w[i] || !mlp->b[i]) return NIC_E_NULL;
    if ((rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    LodParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.y = y;
    set_lod(p, lodp, lod);
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
    return launch_src<PK_FUSED>(p, src->kind, persistent_grid((n_points + 63) >> 6), stream);
}

}  // extern "C"
