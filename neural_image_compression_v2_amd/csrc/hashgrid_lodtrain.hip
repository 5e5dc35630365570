// The gradient with respect to the LEVEL OF DETAIL from the training step (include/nicv2_hip_ext.h: nic_hash_fused_forward_backward_points_grad_lod,
// nic_hash_encode_points_grad_lod_noisy; hashgrid.py, HashGridField.train_points_grad_lod / train_points_differentiable_lod).
//
//   The row the step decodes has column l F + f = a_l (r[l, f] + nz[l F + f]): the codec noise sits INSIDE the weighed column, so
//       dlod[n] = passes(n) ? - sum_{l: 0 < a_raw <= 1} sum_f g[n, l F + f] (r[n, l, f] + nz[n, l F + f]) : 0
//   with g = d loss / d row of the loss the call returns, the conventions of hashgrid_lodgrad.hip (the right-hand derivative; exactly 0.0f where
//   the clamp of lambda is flat) and nz the value the forward added - regenerated from the same key in the walk, not carried.
//   The fused kernel is hash_points_joint_train_kernel (hashgrid_points_joint.hip) with a level of detail always on and the walk of
//   hashgrid_pointgrad.hpp asked for d / d lambda and the noise: the same gathers, the same records, the same scatter, the same dpoints bit for bit, one
//   more accumulator and one more store per point.  The layer-wise kernel is hash_points_grad_lod_kernel (hashgrid_lodgrad.hip) from the fp32
//   table with the same walk.  Rows of dpoints and dlod are written once by their lane; nothing is added to them.
#include "hash_common.hpp"
#include "hashgrid_pointgrad.hpp"

namespace nic {
namespace hltrain {
using namespace hcommon;

// LodParams with the two outputs on top; the layout of the base is kept, the helpers read it through `const LodParams&`
struct LodTrainParams : LodParams {
    float* dpoints;           // [n, dim]
    float* dlod;              // [n]
};

// ---- layer-wise: d loss / d row from memory, one lane per point ----------------------------------------------------------------------------
template <int D, int F, bool NOISE>
__global__ void __launch_bounds__(256) hash_points_grad_lod_noisy_kernel(const LodTrainParams p) {
    const LodParams& s = p;
    const int LF = s.d.levels * F;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < s.n; n += (int64_t)gridDim.x * 256) {
        uint32_t t[3];
        point_fixed<D>(s.d, s.points, n, t);
        const float lam = point_lambda(s, n);
        const float* drow = s.dx + n * LF;
        float g[D], gl;
        point_walk<D, F, NIC_HASH_SRC_F32, true, true, NOISE>(s, t, n, lam, [&](int l, float (&gv)[F]) { load_row<F>(drow + l * F, gv); }, g, gl);
        store_point_grad<D>(p.dpoints, n, kept_axes<D>(s.d, s.points, n), g);
        p.dlod[n] = lambda_passes(s.lod, s.lod_uniform, n) ? gl : 0.0f;
    }
}

// ---- fused: the training step at points with d loss / d points and d loss / d lambda; one wave per 64 consecutive (ordered) points -----------
template <int D, int F, int KT, bool NOISE>
__global__ void __launch_bounds__(256) hash_points_lod_train_kernel(const LodTrainParams p) {
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
            decoder_train_half<KT>(sm, xs, P, Q, nt, j, half, ks1, mine, s.target + r * 3, s.y != nullptr ? s.y + r * 3 : nullptr, s.dscale, true, A);
        }
        wave_sync();
        // d loss / d row of this lane's point is its row of the tile from here to the last wave_sync: the scatter and the walk only read it
        auto grow = [&](int l, float (&gv)[F]) {
#pragma unroll
            for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
        };
        if (s.grad != nullptr) scatter_point<D, F, true>(s.d, t, s.grad, level_fade(s), lam, live_lane, lane, grow);
        float gp[D], gl;
        point_walk<D, F, NIC_HASH_SRC_F32, true, true, NOISE>(s, t, row, lam, grow, gp, gl);
        if (live_lane) {
            store_point_grad<D>(p.dpoints, row, kept_axes<D>(s.d, s.points, row), gp);
            p.dlod[row] = lambda_passes(s.lod, s.lod_uniform, row) ? gl : 0.0f;
        }
        wave_sync();
    }
    write_record<KT>(sm, A, LF, s.partials + (int64_t)blockIdx.x * RecLayout(LF).rec, tid);
}

// ---- host side (the checks, the grid rules and the end of the step are hash_common.hpp's) ---------------------------------------------------
template <bool FUSED, bool NOISE>
static int launch(const LodTrainParams& p, int nb, void* stream) {
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        const hipStream_t s = (hipStream_t)stream;
        if constexpr (!FUSED) hipLaunchKernelGGL((hash_points_grad_lod_noisy_kernel<D, F, NOISE>), dim3(nb), dim3(256), 0, s, p);
        else if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_points_lod_train_kernel<D, F, 2, NOISE>), dim3(nb), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((hash_points_lod_train_kernel<D, F, 1, NOISE>), dim3(nb), dim3(256), 0, s, p);
    });
}

}  // namespace hltrain
}  // namespace nic

using namespace nic;
using namespace nic::hltrain;

extern "C" {

int nic_hash_encode_points_grad_lod_noisy(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_quant* quant, const float* table,
                                          const float* points, const float* lod, int64_t n_points, const float* dx, float* dpoints, float* dlod,
                                          void* stream) {
    int rc = check_point_desc(desc);
    if (rc) return rc;
    if (!lodp || !table || !points || !dx || !dpoints || !dlod) return NIC_E_NULL;
    LodTrainParams p{};
    p.d = *desc; p.table = table; p.points = points; p.n = n_points; p.dx = dx; p.dpoints = dpoints; p.dlod = dlod;
    if ((rc = check_lod(&p.d, lodp)) != NIC_OK) return rc;
    set_lod(p, lodp, lod);
    p.noise.mode = NIC_NOISE_NONE;
    if ((rc = set_noise(quant, true, p.noise, p.sample_base)) != NIC_OK) return rc;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    const int nb = strided_grid((n_points + 63) >> 6);
    return p.noise.mode == NIC_NOISE_KERNEL ? launch<false, true>(p, nb, stream) : launch<false, false>(p, nb, stream);
}

// nic_hash_fused_forward_backward_points_grad (hashgrid_points_joint.hip) with lodp != NULL, check for check
int nic_hash_fused_forward_backward_points_grad_lod(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_quant* quant,
                                                    const float* table, const float* points, const float* lod, int64_t n_points,
                                                    const int32_t* order, const nic_mlp* mlp, const float* target, float loss_scale,
                                                    float* table_grad, const nic_mlp_grads* mlp_grads, float* loss, float* y, float* dpoints,
                                                    float* dlod, int flags, void* workspace, size_t workspace_bytes, const nic_step_tail* tail,
                                                    void* stream) {
    const KernelEndDrop end;
    int rc = open_fused_points(desc, mlp);
    if (rc) return rc;
    if (!lodp || !table || !points || !target || !mlp_grads || !loss || !dpoints || !dlod || !workspace) return NIC_E_NULL;
    if (flags & ~(NIC_HASH_FUSED_ADD_GRADS | NIC_HASH_FUSED_ADD_LOSS)) return NIC_E_ARG;
    if ((rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    LodTrainParams p{};
    fill_fused_points(p, desc, points, n_points, order, table, target, table_grad, y, mlp);
    p.dpoints = dpoints; p.dlod = dlod;
    set_lod(p, lodp, lod);
    return points_fused_step(p, quant, order, loss_scale, mlp_grads, loss, flags, workspace, workspace_bytes, tail, stream,
                             [&](auto noise, int grid) { return launch<true, decltype(noise)::value>(p, grid, stream); });
}

}  // extern "C"
