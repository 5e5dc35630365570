// The gradient of the hash-grid field with respect to the LEVEL OF DETAIL of a point, next to the one with respect to its coordinates
// (include/nicv2_hip_ext.h: nic_hash_encode_points_grad_lod, nic_hash_fused_points_grad_lod; hashgrid.py, HashGridField.point_gradient_lod /
// jacobian_lod / query_differentiable_lod).
//
//   Column l F + f of the row of a point is a_l r[l, f] with a_l = clamp((fade[l] - lambda) + 1, 0, 1) and r the unweighed multilinear blend, so
//       dlod[n] = - sum_{l: 0 < a_raw <= 1} sum_f g[n, l F + f] r[n, l, f]
//   with g = d loss / d row - the right-hand derivative: a level exactly at its fade start has slope -1, one exactly at its end slope 0 - and
//   exactly 0.0f where the clamp of lambda itself is flat (lambda_raw < 0, >= 32 or NaN).  Both kernels are hashgrid_pointgrad.hip's with the
//   walk of hashgrid_pointgrad.hpp asked for d / d lambda too: the same gathers, the same dpoints bit for bit, one more accumulator and one
//   more store per point.  Nothing is added anywhere: row n of every output is written once by the lane of point n.
#include "hash_common.hpp"
#include "hashgrid_pointgrad.hpp"

namespace nic {
namespace hlgrad {
using namespace hcommon;

struct LodGradParams {
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
    float* dlod;              // [n]
    // fused only
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const float* dy;          // [n, 3], or null: the gradient comes from `target`
    const float* target;      // [n, 3]
    float* y;                 // null, or [n, 3]
    float dscale;             // 2 loss_scale / (3 N)
};

// ---- layer-wise: d loss / d row from memory, one lane per point ----------------------------------------------------------------------------
template <int D, int F, int SRC>
__global__ void __launch_bounds__(256) hash_points_grad_lod_kernel(const LodGradParams p) {
    const int LF = p.d.levels * F;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < p.n; n += (int64_t)gridDim.x * 256) {
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, n, t);
        const float lam = point_lambda(p.lod, p.lod_uniform, n);
        const float* drow = p.dx + n * LF;
        float g[D], gl;
        point_walk<D, F, SRC, true, true, false>(p, t, n, lam, [&](int l, float (&gv)[F]) { load_row<F>(drow + l * F, gv); }, g, gl);
        store_point_grad<D>(p.dpoints, n, kept_axes<D>(p.d, p.points, n), g);
        p.dlod[n] = lambda_passes(p.lod, p.lod_uniform, n) ? gl : 0.0f;
    }
}

// ---- fused: gather, decoder forward, backward to the row, position and lambda gradient; one wave per 64 consecutive points --------------------
template <int D, int F, int SRC, int KT>
__global__ void __launch_bounds__(256) hash_points_fused_grad_lod_kernel(const LodGradParams p) {
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
        const float lam = point_lambda(p.lod, p.lod_uniform, row);
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, row, t);
        encode_point<D, F, SRC, false, false, true>(p, t, 0, lam, xrow);
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
        float gp[D], gl;
        point_walk<D, F, SRC, true, true, false>(p, t, row, lam, [&](int l, float (&gv)[F]) {
#pragma unroll
            for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
        }, gp, gl);
        if (live_lane) {
            store_point_grad<D>(p.dpoints, n_raw, kept_axes<D>(p.d, p.points, row), gp);
            p.dlod[n_raw] = lambda_passes(p.lod, p.lod_uniform, row) ? gl : 0.0f;
        }
        wave_sync();
    }
}

// ---- host side (the descriptor checks, the source and the grid rules are hash_common.hpp's) --------------------------------------------------
template <bool FUSED, int SRC>
static int launch(const LodGradParams& p, int nb, void* stream) {
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        const hipStream_t s = (hipStream_t)stream;
        if constexpr (!FUSED) hipLaunchKernelGGL((hash_points_grad_lod_kernel<D, F, SRC>), dim3(nb), dim3(256), 0, s, p);
        else if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_points_fused_grad_lod_kernel<D, F, SRC, 2>), dim3(nb), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((hash_points_fused_grad_lod_kernel<D, F, SRC, 1>), dim3(nb), dim3(256), 0, s, p);
    });
}
template <bool FUSED>
static int launch_src(const LodGradParams& p, int kind, int nb, void* stream) {
    return dispatch_source(kind, [&](auto src) { return launch<FUSED, decltype(src)::value>(p, nb, stream); });
}

}  // namespace hlgrad
}  // namespace nic

using namespace nic;
using namespace nic::hlgrad;

extern "C" {

int nic_hash_encode_points_grad_lod(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_source* src, const float* points,
                                    const float* lod, int64_t n_points, const float* dx, float* dpoints, float* dlod, void* stream) {
    int rc = check_point_desc(desc);
    if (rc) return rc;
    if (!lodp || !src || !src->data || !points || !dx || !dpoints || !dlod) return NIC_E_NULL;
    LodGradParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.dx = dx; p.dpoints = dpoints; p.dlod = dlod;
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if ((rc = check_lod(&p.d, lodp)) != NIC_OK) return rc;
    set_lod(p, lodp, lod);
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    return launch_src<false>(p, src->kind, strided_grid((n_points + 63) >> 6), stream);
}

int nic_hash_fused_points_grad_lod(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_source* src, const float* points,
                                   const float* lod, int64_t n_points, const nic_mlp* mlp, const float* dy, const float* target, float loss_scale,
                                   float* y, float* dpoints, float* dlod, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((rc = check_point_desc(desc)) != NIC_OK) return rc;
    if (!lodp || !src || !src->data || !points || !dpoints || !dlod) return NIC_E_NULL;
    for (int i = 0; i < 3; ++i)
        if (!mlp->w[i] || !mlp->b[i]) return NIC_E_NULL;
    LodGradParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.dy = dy; p.target = target; p.y = y; p.dpoints = dpoints; p.dlod = dlod;
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if ((rc = check_lod(&p.d, lodp)) != NIC_OK) return rc;
    set_lod(p, lodp, lod);
    if ((dy != nullptr) == (target != nullptr)) return NIC_E_ARG;        // exactly one of the two
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
    p.dscale = 2.0f * (float)((double)loss_scale / (3.0 * (double)n_points));
    return launch_src<true>(p, src->kind, persistent_grid((n_points + 63) >> 6), stream);
}

}  // extern "C"
