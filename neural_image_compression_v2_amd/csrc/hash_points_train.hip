// Cell-ordered and fused training of the hash-grid field at ARBITRARY points (include/nicv2_hip.h: nic_hash_point_keys,
// nic_hash_encode_points_backward_ordered, nic_hash_fused_points_workspace_bytes, nic_hash_fused_forward_backward_points; hashgrid.py,
// HashGridField.train_points(order=, fused=) / fit_points).
//
//   keys      one Morton key per point from the clamped fixed-point position of nic_hash_encode_points: Z-order is hierarchical, so neighbours in
//             key order share their cell at the coarse levels and mostly at the fine ones.  The sort is the caller's (a stable device sort).
//   ordered   hash_points_backward_kernel with lane n on point order[n]: the run sums merge neighbouring lanes of one cell again, which random
//             batches lost (124 ms against 14 ms for 8.3 M points).
//   fused     hash_fused_kernel's training mode with hash_points_fused_kernel's sample source: a wave gathers the rows of 64 consecutive
//             (ordered) points into its LDS tile, runs the decoder forward and backward on the fp32 matrix pipe, leaves d loss / d row in the
//             tile and scatters it with the run sums keyed on the base vertex; one record per workgroup, reduced in a fixed order by
//             hash_fused_reduce_kernel (hash_fused.hip) with the optimiser tail riding on it.
//
// With a level of detail per point (nic_hash_encode_points_backward_lod, nic_hash_fused_forward_backward_points_lod) the ordered
// scatter and the fused step are the same kernels on LodParams: the weight a_l of hash_points.hip on the row and again on its gradient.
//
// Every index read from `order` is clamped to [0, n_points - 1]: a buffer that is no permutation gives the sum over the rows it names.
#include "hash_common.hpp"

namespace nic {
namespace hptrain {
using namespace hcommon;

struct TParams {
    nic_hash_desc d;          // extent[a] = S_a, num_crops = 1
    const float* points;      // [n, dim]
    int64_t n;
    const int32_t* order;     // null, or [n] row indices (clamped)
    const float* table;
    const float* dx;          // ordered scatter: [n, L F]
    float* grad;              // table gradient (fused: null = frozen table, no scatter)
    int64_t* keys;
    int32_t key_shift;        // s = max(0, b - k)
    // fused only
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const float* target;
    float* y;
    float* partials;
    NoiseSrc noise;
    uint64_t sample_base;
    float dscale;             // 2 loss_scale / (3 N)
};

// bit j of x -> bit 2 j (x < 2^31) / bit 3 j (x < 2^21)
__device__ __forceinline__ uint64_t spread2(uint64_t x) {
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}
__device__ __forceinline__ uint64_t spread3(uint64_t x) {
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

template <int D>
__global__ void __launch_bounds__(256) hash_point_keys_kernel(const TParams p) {
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < p.n; n += (int64_t)gridDim.x * 256) {
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, n, t);
        uint64_t key;
        if (D == 2) key = spread2(t[0] >> p.key_shift) | (spread2(t[1] >> p.key_shift) << 1);
        else key = spread3(t[0] >> p.key_shift) | (spread3(t[1] >> p.key_shift) << 1) | (spread3(t[2] >> p.key_shift) << 2);
        p.keys[n] = (int64_t)key;
    }
}

// Params: TParams, or LodParams with a level of detail per point (hash_common.hpp), in both kernels below
template <int D, int F, class Params>
__global__ void __launch_bounds__(256) hash_points_backward_ordered_kernel(const Params p) {
    const int lane = threadIdx.x & 63;
    const int LF = p.d.levels * F;
    for (int64_t nb = (int64_t)blockIdx.x * 256; nb < p.n; nb += (int64_t)gridDim.x * 256) {      // block-uniform trip count: the shuffles see whole waves
        const int64_t pos = nb + threadIdx.x;
        const bool live = pos < p.n;
        const int64_t last = live ? pos : p.n - 1;                                                  // a dead lane reads the last point, adds nothing
        const int64_t n = ordered_row(p.order, p.n, last);                                          // (`last` first: n is read before order, as it was)
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, n, t);
        const float* drow = p.dx + n * LF;
        scatter_point<D, F, is_lod<Params>>(p.d, t, p.grad, level_fade(p), point_lambda(p, n), live, lane, [&](int l, float (&g)[F]) { load_row<F>(drow + l * F, g); });
    }
}

// LodParams: the weight is applied where the row enters the LDS tile and again on d loss / d row before the scatter
template <int D, int F, int KT, bool NOISE, class Params>
__global__ void __launch_bounds__(256) hash_points_fused_train_kernel(const Params p) {
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

    const int64_t n_waves = (p.n + 63) >> 6;
    const WaveRange wr = xcd_range(n_waves);
    const int ks1 = (LF + 1) >> 1;
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= n_waves) continue;                            // wave-uniform; nothing below synchronises the workgroup
        const int64_t pos = (wv << 6) + lane;
        const bool live_lane = pos < p.n;
        const int64_t row = ordered_row(p.order, p.n, live_lane ? pos : p.n - 1);      // a lane past the end takes the last point; it stores and adds nothing
        const float lam = point_lambda(p, row);
        uint32_t t[3];
        point_fixed<D>(p.d, p.points, row, t);
        encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, is_lod<Params>>(p, t, row, lam, xrow);
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
            scatter_point<D, F, is_lod<Params>>(p.d, t, p.grad, level_fade(p), lam, live_lane, lane, [&](int l, float (&gv)[F]) {
#pragma unroll
                for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
            });
        wave_sync();
    }
    write_record<KT>(sm, A, LF, p.partials + (int64_t)blockIdx.x * RecLayout(LF).rec, tid);
}

// ---- host side (the checks and grid rules are hash_common.hpp's) -----------------------------------------------------------------------------
enum TKernel { TK_BWD, TK_TRAIN, TK_TRAIN_NOISY };

template <int K, class Params>
static int launch(const Params& p, int nb, void* stream) {
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        constexpr bool NOISE = K == TK_TRAIN_NOISY;
        const hipStream_t s = (hipStream_t)stream;
        if constexpr (K == TK_BWD) hipLaunchKernelGGL((hash_points_backward_ordered_kernel<D, F, Params>), dim3(nb), dim3(256), 0, s, p);
        else if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_points_fused_train_kernel<D, F, 2, NOISE, Params>), dim3(nb), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((hash_points_fused_train_kernel<D, F, 1, NOISE, Params>), dim3(nb), dim3(256), 0, s, p);
    });
}

}  // namespace hptrain
}  // namespace nic

using namespace nic;
using namespace nic::hptrain;

extern "C" {

int nic_hash_point_keys(const nic_hash_desc* desc, const float* points, int64_t n_points, int64_t* keys, void* stream) {
    const int rc = check_point_desc(desc);
    if (rc) return rc;
    if (!points || !keys) return NIC_E_NULL;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    TParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.keys = keys;
    int b = 0;                                                          // bit length of 256 S_max - 1 (<= 30)
    for (uint32_t top = 256u * (uint32_t)desc->S_max - 1u; top; top >>= 1) ++b;
    const int k = desc->dim == 2 ? 31 : 21;
    p.key_shift = b > k ? b - k : 0;
    const int nb = strided_grid((n_points + 63) >> 6);
    if (desc->dim == 2) hipLaunchKernelGGL(hash_point_keys_kernel<2>, dim3(nb), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(hash_point_keys_kernel<3>, dim3(nb), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int nic_hash_encode_points_backward_ordered(const nic_hash_desc* desc, const float* points, int64_t n_points, const float* dx, const int32_t* order,
                                            float* table_grad, void* stream) {
    if (!order) return nic_hash_encode_points_backward(desc, points, n_points, dx, table_grad, stream);
    const int rc = check_point_desc(desc);
    if (rc) return rc;
    if (!points || !dx || !table_grad) return NIC_E_NULL;
    if (n_points < 0 || n_points >= (int64_t(1) << 31)) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    TParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.dx = dx; p.order = order; p.grad = table_grad;
    return launch<TK_BWD>(p, strided_grid((n_points + 63) >> 6), stream);
}

size_t nic_hash_fused_points_workspace_bytes(const nic_hash_desc* desc, const nic_mlp* mlp) {
    if (!desc || !mlp || nic_hash_fused_supported(desc, kH, mlp->n_linear) != NIC_OK || check_point_desc(desc) != NIC_OK) return 0;
    return points_workspace_bytes(desc->levels * desc->features);
}

int nic_hash_fused_forward_backward_points(const nic_hash_desc* desc, const nic_hash_quant* quant, const float* table, const float* points,
                                           int64_t n_points, const int32_t* order, const nic_mlp* mlp, const float* target, float loss_scale,
                                           float* table_grad, const nic_mlp_grads* mlp_grads, float* loss, float* y, int flags, void* workspace,
                                           size_t workspace_bytes, const nic_step_tail* tail, void* stream) {
    const KernelEndDrop end;
    int rc = open_fused_points(desc, mlp);
    if (rc) return rc;
    if (!table || !points || !target || !mlp_grads || !loss || !workspace) return NIC_E_NULL;
    if (flags & ~(NIC_HASH_FUSED_ADD_GRADS | NIC_HASH_FUSED_ADD_LOSS)) return NIC_E_ARG;
    TParams p{};
    fill_fused_points(p, desc, points, n_points, order, table, target, table_grad, y, mlp);
    return points_fused_step(p, quant, order, loss_scale, mlp_grads, loss, flags, workspace, workspace_bytes, tail, stream,
                             [&](auto noise, int grid) { return launch<decltype(noise)::value ? TK_TRAIN_NOISY : TK_TRAIN>(p, grid, stream); });
}

// ---- with a level of detail per point: the checks of the nic_hash_lod follow the null checks, the launches are the same ------
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
    return launch<TK_BWD>(p, strided_grid((n_points + 63) >> 6), stream);
}

int nic_hash_fused_forward_backward_points_lod(const nic_hash_desc* desc, const nic_hash_lod* lodp, const nic_hash_quant* quant, const float* table,
                                               const float* points, const float* lod, int64_t n_points, const int32_t* order, const nic_mlp* mlp,
                                               const float* target, float loss_scale, float* table_grad, const nic_mlp_grads* mlp_grads, float* loss,
                                               float* y, int flags, void* workspace, size_t workspace_bytes, const nic_step_tail* tail, void* stream) {
    const KernelEndDrop end;
    int rc = open_fused_points(desc, mlp);
    if (rc) return rc;
    if (!lodp || !table || !points || !target || !mlp_grads || !loss || !workspace) return NIC_E_NULL;
    if ((rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    if (flags & ~(NIC_HASH_FUSED_ADD_GRADS | NIC_HASH_FUSED_ADD_LOSS)) return NIC_E_ARG;
    LodParams p{};
    fill_fused_points(p, desc, points, n_points, order, table, target, table_grad, y, mlp);
    set_lod(p, lodp, lod);
    return points_fused_step(p, quant, order, loss_scale, mlp_grads, loss, flags, workspace, workspace_bytes, tail, stream,
                             [&](auto noise, int grid) { return launch<decltype(noise)::value ? TK_TRAIN_NOISY : TK_TRAIN>(p, grid, stream); });
}

}  // extern "C"
