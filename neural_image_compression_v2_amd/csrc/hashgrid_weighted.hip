// The fused training step at ARBITRARY points with a WEIGHT PER POINT in its loss (include/nicv2_hip_ext.h:
// nic_hash_fused_forward_backward_points_weighted; hashgrid.py, HashGridField.train_points_weighted).
//
//       loss = loss_scale sum_n w_n sum_o (y[n, o] - t[n, o])^2 / (3 N),     w_n = weight[n] > 0 ? weight[n] : 0   (a NaN fails the comparison)
//   with N the number of points, not the sum of the weights.  Everything downstream is the derivative of that loss: the lane that owns sample r
//   hands the decoder dscale w_r in the place of dscale, so d loss / d row, the table gradient, the decoder gradients, dpoints and dlod carry
//   w_r; the loss partial is (w_r e) e.  A point of weight 0 gets its y, adds +0 to the loss and zeros to every gradient.
//   The kernel is hash_points_lod_train_kernel (hashgrid_lodtrain.hip) from the same pieces - encode_point, decoder_train_half, scatter_point,
//   point_walk, write_record - with the level of detail always compiled in (without a nic_hash_lod it runs at lambda = 0 with every fade 0:
//   every level weighs exactly 1, the rows of the plain step bit for bit) and the second walk only where dpoints is asked for, its lambda
//   accumulator only where dlod is.  At w = 1 the two products with w are exact, so the call reproduces the sibling of the same arguments.
#include "hash_common.hpp"
#include "hashgrid_pointgrad.hpp"

namespace nic {
namespace hweighted {
using namespace hcommon;

// LodParams with the weights and the two outputs on top; the layout of the base is kept, the helpers read it through `const LodParams&`
struct WeightedParams : LodParams {
    const float* weight;      // null (every point weighs 1), or [n]
    float* dpoints;           // WALK >= 1: [n, dim]
    float* dlod;              // WALK == 2: [n]
};

enum Walk { WALK_NONE = 0, WALK_POINTS = 1, WALK_POINTS_LOD = 2 };

// one wave per 64 consecutive (ordered) points
template <int D, int F, int KT, bool NOISE, int WALK>
__global__ void __launch_bounds__(256) hash_points_weighted_train_kernel(const WeightedParams p) {
    const LodParams& s = p;
    __shared__ TrainSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = s.d.levels * F;
    load_decoder(sm, s.w1, s.b1, s.w2, s.b2, s.w3, s.b3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;
    float* P = sm.p[wave];
    float* Q = sm.q[wave];
    TrainAcc<KT> A;
    A.clear();

    const int64_t n_waves = (s.n + 63) >> 6;
    const WaveRange wr = xcd_range(n_waves);
    const int ks1 = (LF + 1) >> 1;
    const bool want_dx = WALK != WALK_NONE || s.grad != nullptr;
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= n_waves) continue;                            // wave-uniform; nothing below synchronises the workgroup
        const int64_t pos = (wv << 6) + lane;
        const bool live_lane = pos < s.n;
        const int64_t row = ordered_row(s.order, s.n, live_lane ? pos : s.n - 1);      // a lane past the end takes the last point; it stores and adds nothing
        const float lam = point_lambda(s, row);
        uint32_t t[3];
        point_fixed<D>(s.d, s.points, row, t);
        encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, true>(s, t, row, lam, xrow);
        wave_sync();
        const unsigned long long live_mask = __ballot(live_lane);
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            const int src = 32 * nt + j;
            const bool mine = half == 0 && ((live_mask >> src) & 1ull);
            const int64_t r = (int64_t)(uint32_t)__shfl((int)(uint32_t)row, src) | ((int64_t)__shfl((int)(row >> 32), src) << 32);
            // r is a row of the launch on every lane (a dead lane's is the last point): the weight is read where the target is
            float w = p.weight != nullptr ? p.weight[r] : 1.0f;
            w = w > 0.f ? w : 0.f;
            decoder_train_half<KT, true>(sm, xs, P, Q, nt, j, half, ks1, mine, s.target + r * 3, s.y != nullptr ? s.y + r * 3 : nullptr,
                                         __fmul_rn(s.dscale, w), want_dx, A, w);
        }
        wave_sync();
        // d loss / d row of this lane's point is its row of the tile from here to the last wave_sync: the scatter and the walk only read it
        auto grow = [&](int l, float (&gv)[F]) {
#pragma unroll
            for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
        };
        if (s.grad != nullptr) scatter_point<D, F, true>(s.d, t, s.grad, level_fade(s), lam, live_lane, lane, grow);
        if constexpr (WALK != WALK_NONE) {
            constexpr bool DLOD = WALK == WALK_POINTS_LOD;
            float gp[D], gl;
            point_walk<D, F, NIC_HASH_SRC_F32, true, DLOD, NOISE && DLOD>(s, t, row, lam, grow, gp, gl);
            if (live_lane) {
                store_point_grad<D>(p.dpoints, row, kept_axes<D>(s.d, s.points, row), gp);
                if constexpr (DLOD) p.dlod[row] = lambda_passes(s.lod, s.lod_uniform, row) ? gl : 0.0f;
            }
        }
        wave_sync();
    }
    write_record<KT>(sm, A, LF, s.partials + (int64_t)blockIdx.x * RecLayout(LF).rec, tid);
}

// ---- host side (the checks, the grid rules and the end of the step are hash_common.hpp's) ---------------------------------------------------
template <bool NOISE, int WALK>
static int launch(const WeightedParams& p, int nb, void* stream) {
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        const hipStream_t s = (hipStream_t)stream;
        if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_points_weighted_train_kernel<D, F, 2, NOISE, WALK>), dim3(nb), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((hash_points_weighted_train_kernel<D, F, 1, NOISE, WALK>), dim3(nb), dim3(256), 0, s, p);
    });
}

}  // namespace hweighted
}  // namespace nic

using namespace nic;
using namespace nic::hweighted;

extern "C" {

int nic_hash_fused_forward_backward_points_weighted(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_quant* quant,
                                                    const float* table, const float* points, const float* lod, const float* weight,
                                                    int64_t n_points, const int32_t* order, const nic_mlp* mlp, const float* target,
                                                    float loss_scale, float* table_grad, const nic_mlp_grads* mlp_grads, float* loss, float* y,
                                                    float* dpoints, float* dlod, int flags, void* workspace, size_t workspace_bytes,
                                                    const nic_step_tail* tail, void* stream) {
    const KernelEndDrop end;
    int rc = open_fused_points(desc, mlp);
    if (rc) return rc;
    if (!table || !points || !target || !mlp_grads || !loss || !workspace) return NIC_E_NULL;
    if (flags & ~(NIC_HASH_FUSED_ADD_GRADS | NIC_HASH_FUSED_ADD_LOSS)) return NIC_E_ARG;
    if ((lod && !lodp) || (dlod && !lodp) || (dlod && !dpoints)) return NIC_E_ARG;
    if (lodp && (rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    WeightedParams p{};                                            // without a nic_hash_lod: every fade 0, lambda 0 - every level weighs 1
    fill_fused_points(p, desc, points, n_points, order, table, target, table_grad, y, mlp);
    p.weight = weight; p.dpoints = dpoints; p.dlod = dlod;
    if (lodp) set_lod(p, lodp, lod);
    return points_fused_step(p, quant, order, loss_scale, mlp_grads, loss, flags, workspace, workspace_bytes, tail, stream, [&](auto noise, int grid) {
        constexpr bool NOISE = decltype(noise)::value;
        if (dlod) return launch<NOISE, WALK_POINTS_LOD>(p, grid, stream);
        if (dpoints) return launch<NOISE, WALK_POINTS>(p, grid, stream);
        return launch<NOISE, WALK_NONE>(p, grid, stream);
    });
}

}  // extern "C"
