// The gradient with respect to the POINT COORDINATES of B hash-grid fields per launch (include/nicv2_hip_ext.h: nic_hash_batch_points_grad,
// nic_hash_batch_points_grad_lod; hashgrid.py, hash_batch_points_grad, HashGridFieldBatch.point_gradient / jacobian / query_differentiable).
//
//   hash_points_fused_grad_kernel (hashgrid_pointgrad.hip) with the shape of a batch (hashgrid_batch.hip): a workgroup BELONGS to a field -
//   b = blockIdx.x / G -, loads field b's decoder once and walks field b's wave items only (field_range over ceil(n_b / 64), n_b the field's
//   own count).  A wave gathers the rows of 64 points of the field's order from the field's table - fp32, compact uint8 or bit-packed, b
//   strides after the base - into its LDS tile, runs the decoder forward and its backward to the input alone (decoder_dx_half, the single
//   field's products in the same order) and walks the levels a second time for the position gradient (point_grad).  Row order[b, pos] of y and
//   dpoints is written once by its lane; tables and decoders are constants, so nothing is added anywhere, no workspace, no reduction: the same
//   call gives the same bits, and field b's rows are nic_hash_fused_points_grad's on field b's tensors bit for bit.
//   with the gradient with respect to the LEVEL OF DETAIL on top (nic_hash_batch_points_grad_lod; HashGridFieldBatch.point_gradient_lod /
//   jacobian_lod / query_differentiable_lod): the same kernel with DLOD - a level of detail always on and the walk asked for
//   d / d lambda (point_walk, hashgrid_pointgrad.hpp): one more accumulator on the corners it gathers anyway, one more store per point:
//   dlod[b, row], exactly 0.0f where the clamp of lambda is flat.
// Every device helper is hash_common.hpp's, hashgrid_pointgrad.hpp's or hashgrid_batch.hpp's; this unit holds the one kernel, its
// parameters and the host side.
#include "hash_common.hpp"
#include "hashgrid_pointgrad.hpp"
#include "hashgrid_batch.hpp"
#include "../../include/nicv2_hip_ext.h"

namespace nic {
namespace hbgrad {
using namespace hcommon;
using namespace hbatch;

// SParams at points (origins null; n_items the wave items of the padded row) with the level of detail of a launch, the ragged point sets of
// the batched training kernel at points and the gradient's own input and output
struct GParams : SParams {
    float fade[NIC_HASH_MAX_LEVELS];
    float lod_uniform;
    const float* lod;         // null, or [B, n]
    const int32_t* counts;    // null (every field has n points), or [B], clamped to [0, n]
    const int32_t* order;     // null, or [B, n] field-local row indices: the first n_b of a row are read, clamped to [0, n_b - 1]
    const float* dy;          // [B, n, 3], or null: the gradient comes from `target`
    const float* target;      // [B, n, 3]
    float loss_scale;         // with a target: dscale = 2 field_loss_mul(loss_scale, n_b), per field
    float* dpoints;           // [B, n, dim]; rows at or past n_b are not written (y, which may be null, alike)
};
// with the gradient with respect to the level of detail: the second output on top; the layout of the base is kept
struct GLParams : GParams {
    float* dlod;              // [B, n]; rows at or past n_b are not written
};
// StoredSrc with what the LOD level loop reads on top: the launch's fade
struct GradSrc : StoredSrc {
    const float (&fade)[NIC_HASH_MAX_LEVELS];
};

// P: GParams, or with DLOD GLParams - the parameter struct is a template argument, so that each instantiation keeps the kernel arguments it had
// as a kernel of its own.  DLOD: point_walk<.., DLOD = true> where the other calls point_grad - the same gathers, y and dpoints bit for bit; row
// `row` of field b's slice of dlod is written once by the live lane that handles it, nothing is added anywhere
template <int D, int F, int SRC, int KT, bool LOD, bool DLOD, class P>
__global__ void __launch_bounds__(256) hash_batch_points_grad_kernel(const P p) {
    static_assert(LOD || !DLOD, "d / d lambda needs a level of detail");
    __shared__ DecoderSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    const int b = (int)(blockIdx.x / (unsigned)p.groups), lb = (int)(blockIdx.x - (unsigned)b * (unsigned)p.groups);
    load_decoder(sm, p.w1 + (int64_t)b * kH * LF, p.b1 + b * kH, p.w2 + (int64_t)b * kH * kH, p.b2 + b * kH, p.w3 + b * 3 * kH, p.b3 + b * 3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;
    const int64_t tab_off = (int64_t)b * p.stride, row_off = (int64_t)b * p.n * 3;
    const GradSrc src_b{{p.d,
                         SRC == NIC_HASH_SRC_F32 ? reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(p.table) + tab_off) : nullptr,
                         SRC == NIC_HASH_SRC_U8 ? p.stored + tab_off : nullptr,
                         SRC == NIC_HASH_SRC_BITS ? reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(p.packed) + tab_off) : nullptr,
                         p.q_scale, p.q_bias, p.q_bits, p.q_tight},
                        p.fade};
    const int64_t n_b = field_count(p.counts, b, p.n);          // workgroup-uniform
    const float dscale = n_b > 0 ? 2.0f * field_loss_mul(p.loss_scale, n_b) : 0.f;
    const float* points = p.points + (int64_t)b * p.n * D;
    [[maybe_unused]] const float* lod_b = p.lod != nullptr ? p.lod + (int64_t)b * p.n : nullptr;
    const int32_t* order = p.order != nullptr ? p.order + (int64_t)b * p.n : nullptr;
    const float* dy = p.dy != nullptr ? p.dy + row_off : nullptr;
    const float* target = p.target != nullptr ? p.target + row_off : nullptr;
    float* y = p.y != nullptr ? p.y + row_off : nullptr;
    float* dpoints = p.dpoints + (int64_t)b * p.n * D;
    [[maybe_unused]] float* dlod = nullptr;
    if constexpr (DLOD) dlod = p.dlod + (int64_t)b * p.n;
    const int ks1 = (LF + 1) >> 1;
    const int64_t n_waves = (n_b + 63) >> 6;                    // 0 at n_b = 0: the field walks nothing and writes nothing
    const WaveRange wr = field_range(n_waves, lb, p.groups);
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= n_waves) continue;                            // wave-uniform; nothing below synchronises the workgroup
        const int64_t pos = (wv << 6) + lane;
        const bool live_lane = pos < n_b;
        const int64_t row = ordered_row(order, n_b, live_lane ? pos : n_b - 1);      // a lane past the end takes the field's last point; it stores nothing
        const float lam = LOD ? point_lambda(lod_b, p.lod_uniform, row) : 0.f;       // at the ROW, as the point
        uint32_t t[3];
        point_fixed<D>(p.d, points, row, t);
        encode_point<D, F, SRC, false, false, LOD>(src_b, t, row, lam, xrow);
        wave_sync();
        const unsigned long long live_mask = __ballot(live_lane);
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            if (((live_mask >> (32 * nt)) & 0xFFFFFFFFull) == 0ull) continue;      // a half tile without a live sample (wave-uniform)
            const int src = 32 * nt + j;
            const bool mine = half == 0 && ((live_mask >> src) & 1ull);
            const int64_t r = __shfl((int)row, src);            // row < n_b <= n < 2^31
            decoder_dx_half<KT>(sm, xs, nt, j, half, ks1, mine, dy != nullptr ? dy + r * 3 : nullptr, target != nullptr ? target + r * 3 : nullptr,
                                y != nullptr ? y + r * 3 : nullptr, dscale);
        }
        wave_sync();
        auto grow = [&](int l, float (&gv)[F]) {
#pragma unroll
            for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
        };
        float gp[D];
        if constexpr (DLOD) {
            float gl;
            point_walk<D, F, SRC, true, true, false>(src_b, t, row, lam, grow, gp, gl);
            if (live_lane) {
                store_point_grad<D>(dpoints, row, kept_axes<D>(p.d, points, row), gp);
                dlod[row] = lambda_passes(lod_b, p.lod_uniform, row) ? gl : 0.0f;
            }
        } else {
            point_grad<D, F, SRC, LOD>(src_b, t, lam, grow, gp);
            if (live_lane) store_point_grad<D>(dpoints, row, kept_axes<D>(p.d, points, row), gp);
        }
        wave_sync();
    }
}

// ---- host side (the checks and grid rules are hash_common.hpp's; kMaxFields, batch_groups_of, mlp3_ok and the fills: hashgrid_batch.hpp) ----------
template <int SRC, bool LOD, bool DLOD, class P>
static int launch(const P& p, int n_fields, void* stream) {
    const dim3 grid((unsigned)n_fields * (unsigned)p.groups);
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_batch_points_grad_kernel<D, F, SRC, 2, LOD, DLOD, P>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((hash_batch_points_grad_kernel<D, F, SRC, 1, LOD, DLOD, P>), grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

// the two entries.  `with_dlod`: nic_hash_batch_points_grad_lod - lodp and dlod join the other pointers of the null list, and the DLOD kernel runs
static int batch_points_grad(const nic_hash_desc* desc, int n_fields, int groups_per_field, const nic_hash_lod* lodp, const nic_hash_source* src,
                             const float* points, const float* lod, int64_t n_points, const int32_t* counts, const int32_t* order, const nic_mlp* mlp,
                             const float* dy, const float* target, float loss_scale, float* y, float* dpoints, float* dlod, bool with_dlod, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((rc = check_point_desc(desc)) != NIC_OK) return rc;
    if (n_fields < 1 || n_fields > kMaxFields) return NIC_E_ARG;
    const int64_t n_items = n_points > 0 ? (n_points + 63) >> 6 : 1;     // a count that launches nothing (checked below) stands as one item here
    const int g = batch_groups_of(n_items, n_fields, groups_per_field);
    if (g < 0) return NIC_E_ARG;
    if ((with_dlod && (!lodp || !dlod)) || !src || !src->data || !points || !mlp3_ok(mlp) || !dpoints) return NIC_E_NULL;
    GLParams p{};
    p.d = *desc; p.points = points; p.y = y; p.groups = g; p.n_items = n_items; p.n = n_points; p.n_rows = n_points;
    p.counts = counts; p.order = order; p.dy = dy; p.target = target; p.loss_scale = loss_scale; p.dpoints = dpoints; p.dlod = dlod;
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if (!lodp && lod) return NIC_E_ARG;                                  // a null nic_hash_lod is "no level of detail" and takes no per-point array
    if (lodp) {
        if ((rc = check_lod(desc, lodp)) != NIC_OK) return rc;
        set_lod(p, lodp, lod);
    }
    if ((dy != nullptr) == (target != nullptr)) return NIC_E_ARG;        // exactly one of the two
    if (n_points < 0 || n_points >= (int64_t(1) << 31)) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    p.stride = stacked_source_stride(desc, src);
    if (p.stride <= 0) return NIC_E_ARG;
    fill_decoder(p, mlp);
    return dispatch_source(src->kind, [&](auto kind) {
        constexpr int SRC = decltype(kind)::value;
        if (with_dlod) return launch<SRC, true, true>(p, n_fields, stream);
        const GParams& q = p;                                            // the kernels without dlod take the base, as they did
        return lodp ? launch<SRC, true, false>(q, n_fields, stream) : launch<SRC, false, false>(q, n_fields, stream);
    });
}

}  // namespace hbgrad
}  // namespace nic

using namespace nic;
using namespace nic::hbgrad;

extern "C" {

int nic_hash_batch_points_grad(const nic_hash_desc* desc, int n_fields, int groups_per_field, const nic_hash_lod* lodp, const nic_hash_source* src,
                               const float* points, const float* lod, int64_t n_points, const int32_t* counts, const int32_t* order, const nic_mlp* mlp,
                               const float* dy, const float* target, float loss_scale, float* y, float* dpoints, void* stream) {
    return batch_points_grad(desc, n_fields, groups_per_field, lodp, src, points, lod, n_points, counts, order, mlp, dy, target, loss_scale, y, dpoints,
                             nullptr, false, stream);
}

// nic_hash_batch_points_grad with a level of detail always on and dlod after dpoints: its checks in its order, lodp and dlod with the other pointers
int nic_hash_batch_points_grad_lod(const nic_hash_desc* desc, int n_fields, int groups_per_field, const nic_hash_lod* lodp, const nic_hash_source* src,
                                   const float* points, const float* lod, int64_t n_points, const int32_t* counts, const int32_t* order,
                                   const nic_mlp* mlp, const float* dy, const float* target, float loss_scale, float* y, float* dpoints, float* dlod,
                                   void* stream) {
    return batch_points_grad(desc, n_fields, groups_per_field, lodp, src, points, lod, n_points, counts, order, mlp, dy, target, loss_scale, y, dpoints,
                             dlod, true, stream);
}

}  // extern "C"
