// The fused training step at ARBITRARY points that also hands back the gradient with respect to the POINT COORDINATES (include/nicv2_hip.h:
// nic_hash_fused_forward_backward_points_grad; hashgrid.py, HashGridField.train_points(dpoints=) / train_points_differentiable).
//
//   hash_points_fused_train_kernel (hash_points_train.hip) from the same pieces of hash_common.hpp - a wave gathers the rows of 64 consecutive
//   (ordered) points into its LDS tile, runs the decoder forward and backward on the fp32 matrix pipe and leaves d loss / d row in the tile,
//   scatters it with the run sums, one record per workgroup for hash_fused_reduce_kernel - with two differences: the backward to the row is
//   always taken (a frozen table still has positions to move), and after the scatter, the row gradient still untouched in the tile, the levels
//   are walked once more for the position gradient: point_grad of hashgrid_pointgrad.hpp, the walk of hash_points_fused_grad_kernel.
//   Row `row` of dpoints - the caller's numbering, order[pos] with an order - is written once by its lane; nothing is added to it.
#include "hash_common.hpp"
#include "hashgrid_pointgrad.hpp"

namespace nic {
namespace hpjoint {
using namespace hcommon;

// TParams of hash_points_train.hip without the fields of the key and ordered-scatter kernels (that unit's kernels must not move, so the
// struct is restated here: a field the fused training kernel gains there is added here too)
struct PlainParams {
    nic_hash_desc d;          // extent[a] = S_a, num_crops = 1
    const float* points;      // [n, dim]
    int64_t n;
    const int32_t* order;     // null, or [n] row indices (clamped)
    const float* table;
    float* grad;              // table gradient (null = frozen table, no scatter)
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const float* target;
    float* y;
    float* partials;
    NoiseSrc noise;
    uint64_t sample_base;
    float dscale;             // 2 loss_scale / (3 N)
};
// the parameters of the sibling kernel - PlainParams, or LodParams with a level of detail per point - with the one output on top; the layout
// of the base is kept, the helpers read it through `const Base&`
template <class Base>
struct JointParams : Base {
    using base = Base;
    float* dpoints;           // [n, dim]
};

// Params: JointParams<PlainParams> or JointParams<LodParams>
template <int D, int F, int KT, bool NOISE, class Params>
__global__ void __launch_bounds__(256) hash_points_joint_train_kernel(const Params p) {
    using Base = typename Params::base;
    constexpr bool LOD = is_lod<Base>;
    const Base& s = p;
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
        encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, LOD>(s, t, row, lam, xrow);
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
        if (s.grad != nullptr) scatter_point<D, F, LOD>(s.d, t, s.grad, level_fade(s), lam, live_lane, lane, grow);
        // through point_grad: with point_walk called from here and its unused `glam` a local of the kernel, every instantiation comes out with its
        // MFMA accumulators in other registers
        float gp[D];
        point_grad<D, F, NIC_HASH_SRC_F32, LOD>(s, t, lam, grow, gp);
        if (live_lane) store_point_grad<D>(p.dpoints, row, kept_axes<D>(s.d, s.points, row), gp);
        wave_sync();
    }
    write_record<KT>(sm, A, LF, s.partials + (int64_t)blockIdx.x * RecLayout(LF).rec, tid);
}

// ---- host side (the checks, the grid rules and the end of the step are hash_common.hpp's) ---------------------------------------------------
template <bool NOISE, class Params>
static int launch(const Params& p, int nb, void* stream) {
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        const hipStream_t s = (hipStream_t)stream;
        if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_points_joint_train_kernel<D, F, 2, NOISE, Params>), dim3(nb), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((hash_points_joint_train_kernel<D, F, 1, NOISE, Params>), dim3(nb), dim3(256), 0, s, p);
    });
}

}  // namespace hpjoint
}  // namespace nic

using namespace nic;
using namespace nic::hpjoint;

extern "C" {

int nic_hash_fused_forward_backward_points_grad(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_quant* quant, const float* table,
                                                const float* points, const float* lod, int64_t n_points, const int32_t* order, const nic_mlp* mlp,
                                                const float* target, float loss_scale, float* table_grad, const nic_mlp_grads* mlp_grads, float* loss,
                                                float* y, float* dpoints, int flags, void* workspace, size_t workspace_bytes, const nic_step_tail* tail,
                                                void* stream) {
    const KernelEndDrop end;
    int rc = open_fused_points(desc, mlp);
    if (rc) return rc;
    if (!table || !points || !target || !mlp_grads || !loss || !dpoints || !workspace) return NIC_E_NULL;
    // flags, then the level of detail: the order include/nicv2_hip.h states for this entry (the _lod sibling asks check_lod first; both are
    // NIC_E_ARG, so no caller can tell)
    if (flags & ~(NIC_HASH_FUSED_ADD_GRADS | NIC_HASH_FUSED_ADD_LOSS)) return NIC_E_ARG;
    if (lodp && (rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    if (!lodp && lod) return NIC_E_ARG;
    auto step = [&](auto& p) {
        return points_fused_step(p, quant, order, loss_scale, mlp_grads, loss, flags, workspace, workspace_bytes, tail, stream,
                                 [&](auto noise, int grid) { return launch<decltype(noise)::value>(p, grid, stream); });
    };
    if (lodp) {
        JointParams<LodParams> p{};
        fill_fused_points(p, desc, points, n_points, order, table, target, table_grad, y, mlp);
        p.dpoints = dpoints;
        set_lod(p, lodp, lod);
        return step(p);
    }
    JointParams<PlainParams> p{};
    fill_fused_points(p, desc, points, n_points, order, table, target, table_grad, y, mlp);
    p.dpoints = dpoints;
    return step(p);
}

}  // extern "C"
