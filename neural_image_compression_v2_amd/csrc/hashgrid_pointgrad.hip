// The gradient of the hash-grid field with respect to the POINT COORDINATES (include/nicv2_hip.h: nic_hash_encode_points_grad,
// nic_hash_fused_points_grad; hashgrid.py, HashGridField.point_gradient / jacobian / query_differentiable).
//
//   The row of a point is the multilinear blend of the 2^dim corner entries of its cell per level, with the weights w_a = fp32(q mod 256 S_max) /
//   fp32(256 S_max), q = t_a R_l (hash_common.hpp, point_cell).  One sample is 1/256 of t and one cell of level l is 256 S_max / R_l of those
//   units, so d w_a / d p_a = R_l / S_max and
//       d row[l F + f] / d p_a = a_l (R_l / S_max) sum_c (c_a ? +1 : -1) prod_{b != a} cw_b(c) value[l, idx(v + c), f]
//   - the derivative of the interpolant at the rounded position the forward route uses; an axis whose floating-point clamp moved the point gives 0.
//   The layer-wise kernel takes d loss / d row from memory, one lane per point.  The fused kernel keeps row and row gradient on the chip: a wave
//   gathers the rows of 64 points into its LDS tile (THE level loop of hash_common.hpp), runs the 64-64-3 decoder forward and its backward to the
//   input alone on v_mfma_f32_32x32x2_f32 (decoder_train_half without its weight-gradient passes, the same products in the same order) with d loss /
//   d row written over the row, and walks the levels a second time for the position gradient - the corner lines were fetched microseconds ago.
//   Nothing is added anywhere: row n of every output is written once by the lane of point n, so the result does not change from run to run.
#include "hash_common.hpp"
#include "hashgrid_pointgrad.hpp"

namespace nic {
namespace hpgrad {
using namespace hcommon;

struct GradParams {
    nic_hash_desc d;          // extent[a] = S_a, num_crops = 1
    float fade[NIC_HASH_MAX_LEVELS];
    float lod_uniform;
    const float* lod;         // null, or [n]
    const float* points;      // [n, dim]
    int64_t n;
    const float* table;       // NIC_HASH_SRC_F32
    const uint8_t* stored;    // NIC_HASH_SRC_U8
    const uint32_t* packed;   // NIC_HASH_SRC_BITS, 4-byte aligned
    float q_scale, q_bias;    // load4fp: (u - q_bias + 1) / q_scale
    int32_t q_bits, q_tight;
    const float* dx;          // layer-wise: [n, L F]
    float* dpoints;           // [n, dim]
    // fused only
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const float* dy;          // [n, 3], or null: the gradient comes from `target`
    const float* target;      // [n, 3]
    float* y;                 // null, or [n, 3]
    float dscale;             // 2 loss_scale / (3 N)
};

// kept_axes, point_walk (the level loop: point_cell<D>(t, R, S, fdiv, v, w), the 2^D corner rows, the D signed weights per corner) and
// store_point_grad live in hashgrid_pointgrad.hpp: the joint training kernel (hashgrid_points_joint.hip) walks the levels with the same code

// ---- layer-wise: d loss / d row from memory, one lane per point ----------------------------------------------------------------------------
template <int D, int F, int SRC, bool LOD>
__global__ void __launch_bounds__(256) hash_points_grad_kernel(const GradParams p) {
    const int LF = p.d.levels * F;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < p.n; n += (int64_t)gridDim.x * 256) {
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, n, t);
        const float lam = LOD ? point_lambda(p.lod, p.lod_uniform, n) : 0.f;
        const float* drow = p.dx + n * LF;
        float g[D], unused;
        point_walk<D, F, SRC, LOD, false, false>(p, t, n, lam, [&](int l, float (&gv)[F]) { load_row<F>(drow + l * F, gv); }, g, unused);
        store_point_grad<D>(p.dpoints, n, kept_axes<D>(p.d, p.points, n), g);
    }
}

// decoder_dx_half - the decoder's backward to the input alone, decoder_train_half without its weight-gradient passes - lives in
// hashgrid_pointgrad.hpp: the batched kernel (hashgrid_batch_grad.hip) runs the same products in the same order

// ---- fused: gather, decoder forward, backward to the row, position gradient; one wave per 64 consecutive points ------------------------------
template <int D, int F, int SRC, int KT, bool LOD>
__global__ void __launch_bounds__(256) hash_points_fused_grad_kernel(const GradParams p) {
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
        const int64_t n0 = wv << 6, n_raw = n0 + lane;
        const bool live_lane = n_raw < p.n;
        const int64_t row = live_lane ? n_raw : p.n - 1;        // a lane past the end takes the last point; it stores nothing
        const float lam = LOD ? point_lambda(p.lod, p.lod_uniform, row) : 0.f;
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, row, t);
        encode_point<D, F, SRC, false, false, LOD>(p, t, 0, lam, xrow);
        wave_sync();
        const unsigned long long live_mask = __ballot(live_lane);
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            if (((live_mask >> (32 * nt)) & 0xFFFFFFFFull) == 0ull) continue;      // a half tile without a live sample (wave-uniform)
            const int64_t n = n0 + 32 * nt + j;
            const bool mine = half == 0 && n < p.n;
            const int64_t r = n < p.n ? n : p.n - 1;
            decoder_dx_half<KT>(sm, xs, nt, j, half, ks1, mine, p.dy != nullptr ? p.dy + r * 3 : nullptr, p.target != nullptr ? p.target + r * 3 : nullptr,
                                p.y != nullptr ? p.y + r * 3 : nullptr, p.dscale);
        }
        wave_sync();
        float gp[D], unused;
        point_walk<D, F, SRC, LOD, false, false>(p, t, row, lam, [&](int l, float (&gv)[F]) {
#pragma unroll
            for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
        }, gp, unused);
        if (live_lane) store_point_grad<D>(p.dpoints, n_raw, kept_axes<D>(p.d, p.points, row), gp);
        wave_sync();
    }
}

// ---- host side (the descriptor checks, the source and the grid rules are hash_common.hpp's) --------------------------------------------------
template <bool FUSED, int SRC, bool LOD>
static int launch(const GradParams& p, int nb, void* stream) {
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        const hipStream_t s = (hipStream_t)stream;
        if constexpr (!FUSED) hipLaunchKernelGGL((hash_points_grad_kernel<D, F, SRC, LOD>), dim3(nb), dim3(256), 0, s, p);
        else if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_points_fused_grad_kernel<D, F, SRC, 2, LOD>), dim3(nb), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((hash_points_fused_grad_kernel<D, F, SRC, 1, LOD>), dim3(nb), dim3(256), 0, s, p);
    });
}
template <bool FUSED>
static int launch_src(const GradParams& p, int kind, bool lod, int nb, void* stream) {
    return dispatch_source(kind, [&](auto src) {
        constexpr int SRC = decltype(src)::value;
        return lod ? launch<FUSED, SRC, true>(p, nb, stream) : launch<FUSED, SRC, false>(p, nb, stream);
    });
}
// a null nic_hash_lod is "no level of detail" and then takes no per-point array; else the checks of check_lod, and the struct into the parameters
static int set_grad_lod(GradParams& p, const nic_hash_lod* lodp, const float* lod) {
    if (!lodp) return lod ? NIC_E_ARG : NIC_OK;
    const int rc = check_lod(&p.d, lodp);
    if (rc) return rc;
    for (int l = 0; l < NIC_HASH_MAX_LEVELS; ++l) p.fade[l] = l < p.d.levels ? lodp->fade[l] : 0.f;
    p.lod_uniform = lodp->lod_uniform;
    p.lod = lod;
    return NIC_OK;
}

}  // namespace hpgrad
}  // namespace nic

using namespace nic;
using namespace nic::hpgrad;

extern "C" {

int nic_hash_encode_points_grad(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_source* src, const float* points, const float* lod,
                                int64_t n_points, const float* dx, float* dpoints, void* stream) {
    int rc = check_point_desc(desc);
    if (rc) return rc;
    if (!src || !src->data || !points || !dx || !dpoints) return NIC_E_NULL;
    GradParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.dx = dx; p.dpoints = dpoints;
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if ((rc = set_grad_lod(p, lodp, lod)) != NIC_OK) return rc;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    return launch_src<false>(p, src->kind, lodp != nullptr, strided_grid((n_points + 63) >> 6), stream);
}

int nic_hash_fused_points_grad(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_source* src, const float* points, const float* lod,
                               int64_t n_points, const nic_mlp* mlp, const float* dy, const float* target, float loss_scale, float* y, float* dpoints,
                               void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((rc = check_point_desc(desc)) != NIC_OK) return rc;
    if (!src || !src->data || !points || !dpoints) return NIC_E_NULL;
    for (int i = 0; i < 3; ++i)
        if (!mlp->w[i] || !mlp->b[i]) return NIC_E_NULL;
    GradParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.dy = dy; p.target = target; p.y = y; p.dpoints = dpoints;
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if ((rc = set_grad_lod(p, lodp, lod)) != NIC_OK) return rc;
    if ((dy != nullptr) == (target != nullptr)) return NIC_E_ARG;        // exactly one of the two
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
    p.dscale = 2.0f * (float)((double)loss_scale / (3.0 * (double)n_points));
    return launch_src<true>(p, src->kind, lodp != nullptr, persistent_grid((n_points + 63) >> 6), stream);
}

}  // extern "C"
