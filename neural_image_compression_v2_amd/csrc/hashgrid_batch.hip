// B hash-grid fields of ONE geometry per launch (include/nicv2_hip.h: nic_hash_batch_*; hashgrid.py, HashGridFieldBatch).
// A small field cannot fill the chip: a 256 x 256 image is 256 groups of four patches, each workgroup of the single-field kernel stages the whole
// decoder to decode one of them, and a folder of such images pays that one after the other.  Here a workgroup BELONGS to a field:
//
//   field b = blockIdx.x / G, local block lb = blockIdx.x % G.  G is a multiple of 8, so lb & 7 is still the workgroup's XCD and the patch walk
//   is xcd_range's arithmetic on (lb, G) over the patches of ONE field (field_range below).  The workgroup loads field b's decoder once and
//   walks only field b's patches; nothing synchronises across workgroups, so B G may exceed the CU count (the grid is then not persistent).
//   storage is stacked and contiguous, the field strides follow from the descriptor: tables / table gradients [B, L, T, F], decoder tensors and
//   their gradients [B, ...], origins [B, num_crops, dim], target / y [B, N, 3], records [B, G, rec], loss [B].
//   training: encode_point on lattice_fixed's position (the crop route's row bit for bit) with the noise keyed by the field-LOCAL sample id - field
//   b sees the noise of a single-field call with the same nic_hash_quant -, decoder_train_half, scatter_point into field b's gradient,
//   write_record to record (b, lb); a workgroup without a patch writes its all-zero record.  hash_batch_reduce_kernel is
//   hash_fused_reduce_kernel's fixed-order sum with blockIdx.y = b, without the optimiser tail: one nic_adam_multi over the stacked tensors
//   steps every field.
//   decoding from a stored table and at points (nic_hash_batch_forward_source): hash_batch_decode_kernel is the forward branch
//   above with two sources added.  The table: field b's starts at base + b stride, fp32 [L, T, F], compact uint8 or bit-packed, the stride
//   from the shared descriptor (a packed table is 4 sum + 8 bytes: every field of a 4-byte-aligned stack is aligned, and its 8 zero bytes keep
//   the widest window of its last level inside the field).  The position: the lattice as above, or points [B, n, dim] through point_fixed,
//   one wave item = 64 consecutive points of one field; a lane past the end decodes the field's last point and stores nothing.
//   training at points (nic_hash_batch_forward_backward_points): hash_batch_points_kernel is the training branch above with the
//   sample source of hash_points_fused_train_kernel (hash_points_train.hip), per field: points / target / y [B, n, ..], order [B, n] of field-LOCAL
//   rows, and a count n_b <= n per field (counts [B], null = n) - real point sets are ragged.  Field b walks ceil(n_b / 64) wave items, divides
//   its loss by ITS n_b, and leaves rows at or past n_b alone; the reduction takes the same counts.
//   with a level of detail per point (nic_hash_batch_forward_points_lod, nic_hash_batch_forward_backward_points_lod):
//   hash_batch_decode_lod_kernel and hash_batch_points_lod_kernel are the two kernels at points with hash_common.hpp's LOD level loop and
//   scatter, lod [B, n] read at the field-local row; kernels of their own, so that the plain ones keep their code.
//   the training step that also hands back d loss / d points (nic_hash_batch_forward_backward_points_grad):
//   hash_batch_points_joint_kernel, at the end of the unit, is the two training kernels at points with the two differences of
//   hash_points_joint_train_kernel (hashgrid_points_joint.hip) - the backward to the row is always taken, and after the scatter the levels are
//   walked once more for the position gradient (hashgrid_pointgrad.hpp), row `row` of field b's slice of dpoints written once by its lane.
//   the same step with d loss / d lambda on top (nic_hash_batch_forward_backward_points_grad_lod): hash_batch_points_joint_lod_kernel,
//   after it, asks that walk for the level-of-detail accumulator and the noise term and stores dlod[b, row] beside dpoints.
//   the host side of the four training entries at points is one path: open_batch_points, the entry's own null list and
//   level-of-detail lines, batch_points_step - the batch counterpart of hash_common.hpp's points_fused_step -, launch_batch_reduce.
// Every device helper is hash_common.hpp's or hashgrid_pointgrad.hpp's; this unit holds the crop-route kernel, the two decode kernels, the four
// training kernels at points - still written out one by one: as one template the text of all 160 instantiations moved -, the
// reduction, their parameters and the host side.  What the 16-bit batched kernel (hashgrid_fused16.hip) and the gradient-only unit
// (hashgrid_batch_grad.hip) share with them - field_range, SParams, StoredSrc, the rules on B and G, the stride of a stacked source, the decoder
// fill - is hashgrid_batch.hpp's.
#include "hash_common.hpp"
#include "hashgrid_batch.hpp"
#include "hashgrid_pointgrad.hpp"
#include "../../include/nicv2_hip_ext.h"

namespace nic {
namespace hbatch {
using namespace hcommon;

struct BParams {
    nic_hash_desc d;          // one field's: every field of the batch shares it
    const float* tables;      // [B, L, T, F]
    const int32_t* origins;   // [B, num_crops, dim]
    const float *w1, *b1, *w2, *b2, *w3, *b3;      // bases of the stacked decoder
    const float* target;      // [B, N, 3]
    float* y;                 // [B, N, 3] (training: may be null)
    float* grads;             // [B, L, T, F] (null: frozen tables, no scatter)
    float* partials;          // [B, G, rec]
    NoiseSrc noise;           // mode NIC_NOISE_NONE / NIC_NOISE_KERNEL
    uint64_t sample_base;
    float dscale;             // 2 loss_scale / (3 N), N = the samples of ONE field
    int64_t n_patches;        // of one field
    int64_t n_samples;        // N
    int32_t groups;           // G
};

// what encode_point reads of a source, for field b: the shared descriptor and noise by reference, the field's own table
struct FieldSrc {
    const nic_hash_desc& d;
    const float* table;
    const NoiseSrc& noise;
    uint64_t sample_base;
};

// the sample of lane `lane` in patch `wv` of a field: its row inside the field (targets, outputs, noise keys) and its fixed-point position.  A
// lane on the rim of a patch gets the position of a real sample; it stores and adds nothing.
template <int D>
__device__ __forceinline__ bool lattice_position(const nic_hash_desc& d, const int32_t* origins, int64_t wv, int64_t n_patches, int lane, int64_t& row,
                                                 uint32_t (&t)[3]) {
    const PatchSample<D> s = patch_sample<D>(d, wv, n_patches, lane);
    lattice_fixed<D>(d, origins, s, t);
    row = s.n;
    return s.live;
}

// MODE: forward only (DecoderSmem, y stored), training, training with the codec's noise on the row
enum { HB_FWD = 0, HB_TRAIN = 1, HB_TRAIN_NOISY = 2 };

template <int D, int F, int KT, int MODE>
__global__ void __launch_bounds__(256) hash_batch_kernel(const BParams p) {
    constexpr bool TRAIN = MODE != HB_FWD;
    __shared__ std::conditional_t<TRAIN, TrainSmem, DecoderSmem> sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    const int b = (int)(blockIdx.x / (unsigned)p.groups), lb = (int)(blockIdx.x - (unsigned)b * (unsigned)p.groups);
    const int64_t tab_off = (((int64_t)b * p.d.levels) << p.d.log2_table) * F, row_off = (int64_t)b * p.n_samples * 3;
    load_decoder(sm, p.w1 + (int64_t)b * kH * LF, p.b1 + b * kH, p.w2 + (int64_t)b * kH * kH, p.b2 + b * kH, p.w3 + b * 3 * kH, p.b3 + b * 3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;
    const int32_t* origins = p.origins + (int64_t)b * p.d.num_crops * D;
    const FieldSrc src_b{p.d, p.tables + tab_off, p.noise, p.sample_base};
    const int ks1 = (LF + 1) >> 1;
    const WaveRange wr = field_range(p.n_patches, lb, p.groups);
    if constexpr (TRAIN) {
        float* P = sm.p[wave];
        float* Q = sm.q[wave];
        float* grad = p.grads != nullptr ? p.grads + tab_off : nullptr;
        const float* target = p.target + row_off;
        float* y = p.y != nullptr ? p.y + row_off : nullptr;
        TrainAcc<KT> A;
        A.clear();
        for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
            const int64_t wv = 4 * g + wave;
            if (wv >= p.n_patches) continue;                    // wave-uniform; nothing below synchronises the workgroup
            int64_t row;
            uint32_t t[3];
            const bool live_lane = lattice_position<D>(p.d, origins, wv, p.n_patches, lane, row, t);
            encode_point<D, F, NIC_HASH_SRC_F32, MODE == HB_TRAIN_NOISY, false, false>(src_b, t, row, 0.f, xrow);
            wave_sync();
            const unsigned long long live_mask = __ballot(live_lane);
#pragma unroll 1
            for (int nt = 0; nt < 2; ++nt) {
                const int src = 32 * nt + j;
                const bool mine = half == 0 && ((live_mask >> src) & 1ull);
                const int64_t r = (int64_t)(uint32_t)__shfl((int)(uint32_t)row, src) | ((int64_t)__shfl((int)(row >> 32), src) << 32);
                decoder_train_half<KT>(sm, xs, P, Q, nt, j, half, ks1, mine, target + r * 3, y != nullptr ? y + r * 3 : nullptr, p.dscale,
                                       grad != nullptr, A);
            }
            wave_sync();
            if (grad != nullptr)
                scatter_point<D, F, false>(p.d, t, grad, nullptr, 0.f, live_lane, lane, [&](int l, float (&gv)[F]) {
#pragma unroll
                    for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
                });
            wave_sync();
        }
        write_record<KT>(sm, A, LF, p.partials + (int64_t)blockIdx.x * RecLayout(LF).rec, tid);      // record (b, lb); all zero without a patch
    } else {
        float* y = p.y + row_off;
        for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
            const int64_t wv = 4 * g + wave;
            if (wv >= p.n_patches) continue;                    // wave-uniform; nothing below synchronises the workgroup
            int64_t row;
            uint32_t t[3];
            const bool live_lane = lattice_position<D>(p.d, origins, wv, p.n_patches, lane, row, t);
            encode_point<D, F, NIC_HASH_SRC_F32, false, false, false>(src_b, t, row, 0.f, xrow);
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
                    for (int o = 0; o < 3; ++o) y[r * 3 + o] = yv[o];
                }
            }
            wave_sync();
        }
    }
}

// ---- training at points, a count per field -------------------------------------------------------------------------------------
struct PParams {
    nic_hash_desc d;          // one field's; extent[a] = S_a, num_crops = 1
    const float* tables;      // [B, L, T, F]
    const float* points;      // [B, n, dim]
    const int32_t* counts;    // null (every field has n points), or [B], clamped to [0, n]
    const int32_t* order;     // null, or [B, n] field-local row indices: the first n_b of a row are read, clamped to [0, n_b - 1]
    const float *w1, *b1, *w2, *b2, *w3, *b3;      // bases of the stacked decoder
    const float* target;      // [B, n, 3]
    float* y;                 // [B, n, 3] (may be null); rows at or past n_b are not written
    float* grads;             // [B, L, T, F] (null: frozen tables, no scatter)
    float* partials;          // [B, G, rec]
    NoiseSrc noise;           // mode NIC_NOISE_NONE / NIC_NOISE_KERNEL
    uint64_t sample_base;
    float loss_scale;         // dscale = 2 field_loss_mul(loss_scale, n_b), per field
    int64_t n;                // the padded width: points of one field's row
    int32_t groups;           // G
};

// hash_batch_kernel's training branch on hash_points_fused_train_kernel's samples: wave item wv of field b = the points at positions 64 wv ..
// of the field's order.  The noise is keyed by the field-local ROW, so field b sees the noise of a single-field call whatever the order.
template <int D, int F, int KT, bool NOISE>
__global__ void __launch_bounds__(256) hash_batch_points_kernel(const PParams p) {
    __shared__ TrainSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    const int b = (int)(blockIdx.x / (unsigned)p.groups), lb = (int)(blockIdx.x - (unsigned)b * (unsigned)p.groups);
    const int64_t tab_off = (((int64_t)b * p.d.levels) << p.d.log2_table) * F, row_off = (int64_t)b * p.n * 3;
    load_decoder(sm, p.w1 + (int64_t)b * kH * LF, p.b1 + b * kH, p.w2 + (int64_t)b * kH * kH, p.b2 + b * kH, p.w3 + b * 3 * kH, p.b3 + b * 3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;
    float* P = sm.p[wave];
    float* Q = sm.q[wave];
    const int64_t n_b = field_count(p.counts, b, p.n);          // workgroup-uniform
    const float dscale = n_b > 0 ? 2.0f * field_loss_mul(p.loss_scale, n_b) : 0.f;
    const float* points = p.points + (int64_t)b * p.n * D;
    const int32_t* order = p.order != nullptr ? p.order + (int64_t)b * p.n : nullptr;
    const FieldSrc src_b{p.d, p.tables + tab_off, p.noise, p.sample_base};
    float* grad = p.grads != nullptr ? p.grads + tab_off : nullptr;
    const float* target = p.target + row_off;
    float* y = p.y != nullptr ? p.y + row_off : nullptr;
    const int ks1 = (LF + 1) >> 1;
    const int64_t n_waves = (n_b + 63) >> 6;
    const WaveRange wr = field_range(n_waves, lb, p.groups);
    TrainAcc<KT> A;
    A.clear();
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= n_waves) continue;                            // wave-uniform; nothing below synchronises the workgroup
        const int64_t pos = (wv << 6) + lane;
        const bool live_lane = pos < n_b;
        const int64_t row = ordered_row(order, n_b, live_lane ? pos : n_b - 1);      // a lane past the end takes the field's last point; it stores and adds nothing
        uint32_t t[3];
        point_fixed<D>(p.d, points, row, t);
        encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, false>(src_b, t, row, 0.f, xrow);
        wave_sync();
        const unsigned long long live_mask = __ballot(live_lane);
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            const int src = 32 * nt + j;
            const bool mine = half == 0 && ((live_mask >> src) & 1ull);
            const int r = __shfl((int)row, src);                // row < n_b <= n < 2^31
            decoder_train_half<KT>(sm, xs, P, Q, nt, j, half, ks1, mine, target + (int64_t)r * 3, y != nullptr ? y + (int64_t)r * 3 : nullptr, dscale,
                                   grad != nullptr, A);
        }
        wave_sync();
        if (grad != nullptr)
            scatter_point<D, F, false>(p.d, t, grad, nullptr, 0.f, live_lane, lane, [&](int l, float (&gv)[F]) {
#pragma unroll
                for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
            });
        wave_sync();
    }
    write_record<KT>(sm, A, LF, p.partials + (int64_t)blockIdx.x * RecLayout(LF).rec, tid);      // record (b, lb); all zero without an item (n_b = 0 too)
}

// ---- forward only, from any table source, on the lattice or at points --------------------------------------------------------
// SParams, StoredSrc: hashgrid_batch.hpp
template <int D, int F, int SRC, bool POINTS>
__global__ void __launch_bounds__(256) hash_batch_decode_kernel(const SParams p) {
    __shared__ DecoderSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    const int b = (int)(blockIdx.x / (unsigned)p.groups), lb = (int)(blockIdx.x - (unsigned)b * (unsigned)p.groups);
    load_decoder(sm, p.w1 + (int64_t)b * kH * LF, p.b1 + b * kH, p.w2 + (int64_t)b * kH * kH, p.b2 + b * kH, p.w3 + b * 3 * kH, p.b3 + b * 3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;
    const int64_t tab_off = (int64_t)b * p.stride;
    const StoredSrc src_b{p.d,
                          SRC == NIC_HASH_SRC_F32 ? reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(p.table) + tab_off) : nullptr,
                          SRC == NIC_HASH_SRC_U8 ? p.stored + tab_off : nullptr,
                          SRC == NIC_HASH_SRC_BITS ? reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(p.packed) + tab_off) : nullptr,
                          p.q_scale, p.q_bias, p.q_bits, p.q_tight};
    [[maybe_unused]] const int32_t* origins = POINTS ? nullptr : p.origins + (int64_t)b * p.d.num_crops * D;
    [[maybe_unused]] const float* points = POINTS ? p.points + (int64_t)b * p.n * D : nullptr;
    float* y = p.y + (int64_t)b * p.n_rows * 3;
    const int ks1 = (LF + 1) >> 1;
    const WaveRange wr = field_range(p.n_items, lb, p.groups);
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= p.n_items) continue;                          // wave-uniform; nothing below synchronises the workgroup
        int64_t row;
        uint32_t t[3];
        bool live_lane;
        if constexpr (POINTS) {
            const int64_t n_raw = (wv << 6) + lane;
            live_lane = n_raw < p.n;
            row = live_lane ? n_raw : p.n - 1;                  // a lane past the end decodes the field's last point; its output is not stored
            point_fixed<D>(p.d, points, row, t);
        } else {
            live_lane = lattice_position<D>(p.d, origins, wv, p.n_items, lane, row, t);
        }
        encode_point<D, F, SRC, false, false, false>(src_b, t, row, 0.f, xrow);
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
                for (int o = 0; o < 3; ++o) y[r * 3 + o] = yv[o];
            }
        }
        wave_sync();
    }
}

// ---- with a level of detail per point (nic_hash_batch_forward_points_lod, nic_hash_batch_forward_backward_points_lod) -----------
// The two kernels at points above with hash_common.hpp's LOD level loop and scatter: lambda of a lane = point_lambda(field b's [n] slice of lod or
// null, lod_uniform, the lane's field-local ROW) - with an order the row order[b, pos] clamped to the field's count, as the point is read -, the
// fade shared by every field of the launch.  Kernels of their own beside the plain ones, whose code they leave as it was.
struct PLParams : PParams {
    float fade[NIC_HASH_MAX_LEVELS];
    float lod_uniform;
    const float* lod;         // null, or [B, n]
};
struct SLParams : SParams {   // points only: origins is null
    float fade[NIC_HASH_MAX_LEVELS];
    float lod_uniform;
    const float* lod;         // null, or [B, n]
};
// FieldSrc / StoredSrc with what the LOD level loop reads on top: the launch's fade
struct LodFieldSrc : FieldSrc {
    const float (&fade)[NIC_HASH_MAX_LEVELS];
};
struct LodStoredSrc : StoredSrc {
    const float (&fade)[NIC_HASH_MAX_LEVELS];
};

template <int D, int F, int KT, bool NOISE>
__global__ void __launch_bounds__(256) hash_batch_points_lod_kernel(const PLParams p) {
    __shared__ TrainSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    const int b = (int)(blockIdx.x / (unsigned)p.groups), lb = (int)(blockIdx.x - (unsigned)b * (unsigned)p.groups);
    const int64_t tab_off = (((int64_t)b * p.d.levels) << p.d.log2_table) * F, row_off = (int64_t)b * p.n * 3;
    load_decoder(sm, p.w1 + (int64_t)b * kH * LF, p.b1 + b * kH, p.w2 + (int64_t)b * kH * kH, p.b2 + b * kH, p.w3 + b * 3 * kH, p.b3 + b * 3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;
    float* P = sm.p[wave];
    float* Q = sm.q[wave];
    const int64_t n_b = field_count(p.counts, b, p.n);          // workgroup-uniform
    const float dscale = n_b > 0 ? 2.0f * field_loss_mul(p.loss_scale, n_b) : 0.f;
    const float* points = p.points + (int64_t)b * p.n * D;
    const float* lod_b = p.lod != nullptr ? p.lod + (int64_t)b * p.n : nullptr;
    const int32_t* order = p.order != nullptr ? p.order + (int64_t)b * p.n : nullptr;
    const LodFieldSrc src_b{{p.d, p.tables + tab_off, p.noise, p.sample_base}, p.fade};
    float* grad = p.grads != nullptr ? p.grads + tab_off : nullptr;
    const float* target = p.target + row_off;
    float* y = p.y != nullptr ? p.y + row_off : nullptr;
    const int ks1 = (LF + 1) >> 1;
    const int64_t n_waves = (n_b + 63) >> 6;
    const WaveRange wr = field_range(n_waves, lb, p.groups);
    TrainAcc<KT> A;
    A.clear();
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= n_waves) continue;                            // wave-uniform; nothing below synchronises the workgroup
        const int64_t pos = (wv << 6) + lane;
        const bool live_lane = pos < n_b;
        const int64_t row = ordered_row(order, n_b, live_lane ? pos : n_b - 1);      // a lane past the end takes the field's last point; it stores and adds nothing
        const float lam = point_lambda(lod_b, p.lod_uniform, row);                   // at the ROW, as the point
        uint32_t t[3];
        point_fixed<D>(p.d, points, row, t);
        encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, true>(src_b, t, row, lam, xrow);
        wave_sync();
        const unsigned long long live_mask = __ballot(live_lane);
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            const int src = 32 * nt + j;
            const bool mine = half == 0 && ((live_mask >> src) & 1ull);
            const int r = __shfl((int)row, src);                // row < n_b <= n < 2^31
            decoder_train_half<KT>(sm, xs, P, Q, nt, j, half, ks1, mine, target + (int64_t)r * 3, y != nullptr ? y + (int64_t)r * 3 : nullptr, dscale,
                                   grad != nullptr, A);
        }
        wave_sync();
        if (grad != nullptr)
            scatter_point<D, F, true>(p.d, t, grad, p.fade, lam, live_lane, lane, [&](int l, float (&gv)[F]) {
#pragma unroll
                for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
            });
        wave_sync();
    }
    write_record<KT>(sm, A, LF, p.partials + (int64_t)blockIdx.x * RecLayout(LF).rec, tid);      // record (b, lb); all zero without an item (n_b = 0 too)
}

template <int D, int F, int SRC>
__global__ void __launch_bounds__(256) hash_batch_decode_lod_kernel(const SLParams p) {
    __shared__ DecoderSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    const int b = (int)(blockIdx.x / (unsigned)p.groups), lb = (int)(blockIdx.x - (unsigned)b * (unsigned)p.groups);
    load_decoder(sm, p.w1 + (int64_t)b * kH * LF, p.b1 + b * kH, p.w2 + (int64_t)b * kH * kH, p.b2 + b * kH, p.w3 + b * 3 * kH, p.b3 + b * 3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;
    const int64_t tab_off = (int64_t)b * p.stride;
    const LodStoredSrc src_b{{p.d,
                              SRC == NIC_HASH_SRC_F32 ? reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(p.table) + tab_off) : nullptr,
                              SRC == NIC_HASH_SRC_U8 ? p.stored + tab_off : nullptr,
                              SRC == NIC_HASH_SRC_BITS ? reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(p.packed) + tab_off) : nullptr,
                              p.q_scale, p.q_bias, p.q_bits, p.q_tight},
                             p.fade};
    const float* points = p.points + (int64_t)b * p.n * D;
    const float* lod_b = p.lod != nullptr ? p.lod + (int64_t)b * p.n : nullptr;
    float* y = p.y + (int64_t)b * p.n_rows * 3;
    const int ks1 = (LF + 1) >> 1;
    const WaveRange wr = field_range(p.n_items, lb, p.groups);
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= p.n_items) continue;                          // wave-uniform; nothing below synchronises the workgroup
        const int64_t n0 = wv << 6, n_raw = n0 + lane, row = n_raw < p.n ? n_raw : p.n - 1;
        uint32_t t[3];
        point_fixed<D>(p.d, points, row, t);                    // a lane past the end decodes the field's last point; its output is not stored
        encode_point<D, F, SRC, false, false, true>(src_b, t, row, point_lambda(lod_b, p.lod_uniform, row), xrow);
        wave_sync();
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            const int64_t r = n0 + 32 * nt + j;
            float yv[3];
            decoder_forward_half(sm, xs, nt, j, half, ks1, yv);
            if (half == 0 && r < p.n) {
#pragma unroll
                for (int o = 0; o < 3; ++o) y[r * 3 + o] = yv[o];
            }
        }
        wave_sync();
    }
}

// hash_fused_reduce_kernel's fixed-order sum, field blockIdx.y: a block = 32 outputs x 8 slices of the field's G records, the slices combined
// through LDS in slice order.  `g` holds the BASES of the stacked gradients, `loss` is [B].  No optimiser tail.  `counts` null: field b's summed
// error times `loss_mul`, the crop route's; else times field_loss_mul(loss_scale, n_b) of its own count (clamped to [0, n_points]; 0 at n_b = 0).
__global__ void __launch_bounds__(256) hash_batch_reduce_kernel(const float* partials, int n_rec, int lf, nic_mlp_grads g, float* loss, float loss_mul,
                                                                int add_grads, int add_loss, const int32_t* counts, int64_t n_points, float loss_scale) {
    __shared__ float red[8][32];
    const RecLayout rl(lf);
    const int64_t b = blockIdx.y;
    const int slice = threadIdx.x >> 5, e = blockIdx.x * 32 + (threadIdx.x & 31);
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    const int per = (n_rec + 7) >> 3, w_lo = slice * per, w_hi = w_lo + per < n_rec ? w_lo + per : n_rec;
    if (e < rl.rec) {
        const float* src = partials + b * n_rec * rl.rec + e;
        int w = w_lo;
        for (; w + 4 <= w_hi; w += 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) part[k] += src[(int64_t)(w + k) * rl.rec];
        }
        for (; w < w_hi; ++w) part[0] += src[(int64_t)w * rl.rec];
    }
    red[slice][threadIdx.x & 31] = (part[0] + part[1]) + (part[2] + part[3]);
    __syncthreads();
    if (slice != 0 || e >= rl.rec) return;
    float acc = red[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < 8; ++k) acc += red[k][threadIdx.x];
    if (e == rl.loss) {
        if (counts != nullptr) {
            const int64_t n_b = field_count(counts, (int)b, n_points);
            loss_mul = n_b > 0 ? field_loss_mul(loss_scale, n_b) : 0.f;
        }
        if (loss) loss[b] = add_loss ? loss[b] + acc * loss_mul : acc * loss_mul;
        return;
    }
    float* dst = e < rl.b1 ? (g.w[0] ? g.w[0] + b * rl.b1 + e : nullptr) : e < rl.w2 ? (g.b[0] ? g.b[0] + b * kH + (e - rl.b1) : nullptr)
               : e < rl.b2 ? (g.w[1] ? g.w[1] + b * kH * kH + (e - rl.w2) : nullptr) : e < rl.w3 ? (g.b[1] ? g.b[1] + b * kH + (e - rl.b2) : nullptr)
               : e < rl.b3 ? (g.w[2] ? g.w[2] + b * 3 * kH + (e - rl.w3) : nullptr) : (g.b[2] ? g.b[2] + b * 3 + (e - rl.b3) : nullptr);
    if (!dst) return;
    *dst = add_grads ? acc + *dst : acc;
}

// ---- host side (the checks and grid rules are hash_common.hpp's; kMaxFields, batch_groups_of, mlp3_ok: hashgrid_batch.hpp) ------------------------
// the lattice goes through the fixed-point cell: 256 S_max < 2^30, as in every unit that reads a crop through lattice_fixed
static int check_batch_desc(const nic_hash_desc* d, int n_linear) {
    const int rc = nic_hash_fused_supported(d, kH, n_linear);            // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    return 256 * (int64_t)d->S_max >= (int64_t(1) << 30) ? NIC_E_ARG : NIC_OK;
}
static int batch_groups(const nic_hash_desc* d, int n_fields, int groups_per_field) { return batch_groups_of(count_patches(d), n_fields, groups_per_field); }
static void fill(BParams& p, const nic_hash_desc* d, const float* tables, const int32_t* origins, const nic_mlp* mlp, float* y, int groups) {
    p.d = *d; p.tables = tables; p.origins = origins; p.y = y; p.groups = groups;
    fill_decoder(p, mlp);
    p.n_patches = count_patches(d);
    p.n_samples = (int64_t)d->num_crops * d->extent[0] * d->extent[1] * (d->dim == 3 ? d->extent[2] : 1);
    p.noise.mode = NIC_NOISE_NONE;
}
template <int MODE>
static int launch(const BParams& p, int n_fields, void* stream) {
    const dim3 grid((unsigned)n_fields * (unsigned)p.groups);
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_batch_kernel<D, F, 2, MODE>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((hash_batch_kernel<D, F, 1, MODE>), grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

template <int SRC>
static int launch_source(const SParams& p, int n_fields, void* stream) {
    const dim3 grid((unsigned)n_fields * (unsigned)p.groups);
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        if (p.points != nullptr) hipLaunchKernelGGL((hash_batch_decode_kernel<D, F, SRC, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((hash_batch_decode_kernel<D, F, SRC, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

template <bool NOISE>
static int launch_points(const PParams& p, int n_fields, void* stream) {
    const dim3 grid((unsigned)n_fields * (unsigned)p.groups);
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_batch_points_kernel<D, F, 2, NOISE>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((hash_batch_points_kernel<D, F, 1, NOISE>), grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}
// G at points: on the wave items of ONE field's padded row; a count that launches nothing stands as one item (nic_hash_batch_forward_source's rule)
static int point_groups(int64_t n_points, int n_fields, int groups_per_field) {
    return batch_groups_of(n_points > 0 ? (n_points + 63) >> 6 : 1, n_fields, groups_per_field);
}

// with a level of detail per point: the same grids, the _lod kernels
template <int SRC>
static int launch_source_lod(const SLParams& p, int n_fields, void* stream) {
    const dim3 grid((unsigned)n_fields * (unsigned)p.groups);
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        hipLaunchKernelGGL((hash_batch_decode_lod_kernel<D, F, SRC>), grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}
template <bool NOISE>
static int launch_points_lod(const PLParams& p, int n_fields, void* stream) {
    const dim3 grid((unsigned)n_fields * (unsigned)p.groups);
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_batch_points_lod_kernel<D, F, 2, NOISE>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((hash_batch_points_lod_kernel<D, F, 1, NOISE>), grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

// ---- training at points that also hands back d loss / d points (nic_hash_batch_forward_backward_points_grad) --------------------
// hash_batch_points_kernel (LOD false) / hash_batch_points_lod_kernel (LOD true) from the same helpers, with the two differences of
// hash_points_joint_train_kernel: the decoder's backward always reaches the row (a frozen table still has positions to move), and after the
// scatter, the row gradient still untouched in the wave's tile, the levels are walked a second time for the position gradient - point_grad, the
// walk of the gradient-only kernels, the same operations in the same order.  Row `row` of field b's slice of dpoints - the caller's numbering,
// order[b, pos] with an order - is written once by the live lane that handles it; rows at or past n_b are not written, nothing is added.
struct PJParams : PLParams {  // without a level of detail fade, lod_uniform and lod are not read
    float* dpoints;           // [B, n, dim]
};

template <int D, int F, int KT, bool NOISE, bool LOD>
__global__ void __launch_bounds__(256) hash_batch_points_joint_kernel(const PJParams p) {
    __shared__ TrainSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    const int b = (int)(blockIdx.x / (unsigned)p.groups), lb = (int)(blockIdx.x - (unsigned)b * (unsigned)p.groups);
    const int64_t tab_off = (((int64_t)b * p.d.levels) << p.d.log2_table) * F, row_off = (int64_t)b * p.n * 3;
    load_decoder(sm, p.w1 + (int64_t)b * kH * LF, p.b1 + b * kH, p.w2 + (int64_t)b * kH * kH, p.b2 + b * kH, p.w3 + b * 3 * kH, p.b3 + b * 3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;
    float* P = sm.p[wave];
    float* Q = sm.q[wave];
    const int64_t n_b = field_count(p.counts, b, p.n);          // workgroup-uniform
    const float dscale = n_b > 0 ? 2.0f * field_loss_mul(p.loss_scale, n_b) : 0.f;
    const float* points = p.points + (int64_t)b * p.n * D;
    [[maybe_unused]] const float* lod_b = p.lod != nullptr ? p.lod + (int64_t)b * p.n : nullptr;
    const int32_t* order = p.order != nullptr ? p.order + (int64_t)b * p.n : nullptr;
    const LodFieldSrc src_b{{p.d, p.tables + tab_off, p.noise, p.sample_base}, p.fade};
    float* grad = p.grads != nullptr ? p.grads + tab_off : nullptr;
    const float* target = p.target + row_off;
    float* y = p.y != nullptr ? p.y + row_off : nullptr;
    float* dpoints = p.dpoints + (int64_t)b * p.n * D;
    const int ks1 = (LF + 1) >> 1;
    const int64_t n_waves = (n_b + 63) >> 6;
    const WaveRange wr = field_range(n_waves, lb, p.groups);
    TrainAcc<KT> A;
    A.clear();
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= n_waves) continue;                            // wave-uniform; nothing below synchronises the workgroup
        const int64_t pos = (wv << 6) + lane;
        const bool live_lane = pos < n_b;
        const int64_t row = ordered_row(order, n_b, live_lane ? pos : n_b - 1);      // a lane past the end takes the field's last point; it stores and adds nothing
        const float lam = LOD ? point_lambda(lod_b, p.lod_uniform, row) : 0.f;       // at the ROW, as the point
        uint32_t t[3];
        point_fixed<D>(p.d, points, row, t);
        encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, LOD>(src_b, t, row, lam, xrow);
        wave_sync();
        const unsigned long long live_mask = __ballot(live_lane);
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            const int src = 32 * nt + j;
            const bool mine = half == 0 && ((live_mask >> src) & 1ull);
            const int r = __shfl((int)row, src);                // row < n_b <= n < 2^31
            decoder_train_half<KT>(sm, xs, P, Q, nt, j, half, ks1, mine, target + (int64_t)r * 3, y != nullptr ? y + (int64_t)r * 3 : nullptr, dscale,
                                   true, A);
        }
        wave_sync();
        // d loss / d row of this lane's point is its row of the tile from here to the last wave_sync: the scatter and the walk only read it
        auto grow = [&](int l, float (&gv)[F]) {
#pragma unroll
            for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
        };
        if (grad != nullptr) scatter_point<D, F, LOD>(p.d, t, grad, LOD ? p.fade : nullptr, lam, live_lane, lane, grow);
        float gp[D];
        point_grad<D, F, NIC_HASH_SRC_F32, LOD>(src_b, t, lam, grow, gp);
        if (live_lane) store_point_grad<D>(dpoints, row, kept_axes<D>(p.d, points, row), gp);
        wave_sync();
    }
    write_record<KT>(sm, A, LF, p.partials + (int64_t)blockIdx.x * RecLayout(LF).rec, tid);      // record (b, lb); all zero without an item (n_b = 0 too)
}
template <bool NOISE, bool LOD>
static int launch_points_joint(const PJParams& p, int n_fields, void* stream) {
    const dim3 grid((unsigned)n_fields * (unsigned)p.groups);
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_batch_points_joint_kernel<D, F, 2, NOISE, LOD>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((hash_batch_points_joint_kernel<D, F, 1, NOISE, LOD>), grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

// ---- the same step that also hands back d loss / d lambda (nic_hash_batch_forward_backward_points_grad_lod) ---------------------
// hash_batch_points_joint_kernel<.., LOD = true> with the walk asked for d / d lambda and the noise (point_walk, hashgrid_pointgrad.hpp) where that
// calls point_grad - hash_points_lod_train_kernel (hashgrid_lodtrain.hip) per field: the same gathers, records, scatter and dpoints bit for bit,
// one more accumulator and one more store per point.  `row` is the field-local row the forward keyed its noise with (sample_base + row), so the
// nz the walk regenerates is the value the forward added.  Row `row` of field b's slice of dlod is written once by its live lane, exactly 0.0f
// where the clamp of lambda is flat; rows at or past n_b are not written, nothing is added.  A kernel of its own: the one above keeps its code.
struct PJLParams : PJParams {
    float* dlod;              // [B, n]
};

template <int D, int F, int KT, bool NOISE>
__global__ void __launch_bounds__(256) hash_batch_points_joint_lod_kernel(const PJLParams p) {
    __shared__ TrainSmem sm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
    const int LF = p.d.levels * F;
    const int b = (int)(blockIdx.x / (unsigned)p.groups), lb = (int)(blockIdx.x - (unsigned)b * (unsigned)p.groups);
    const int64_t tab_off = (((int64_t)b * p.d.levels) << p.d.log2_table) * F, row_off = (int64_t)b * p.n * 3;
    load_decoder(sm, p.w1 + (int64_t)b * kH * LF, p.b1 + b * kH, p.w2 + (int64_t)b * kH * kH, p.b2 + b * kH, p.w3 + b * 3 * kH, p.b3 + b * 3, LF, tid);
    __syncthreads();
    float* xs = sm.x[wave];
    float* xrow = xs + lane * XS;
    float* P = sm.p[wave];
    float* Q = sm.q[wave];
    const int64_t n_b = field_count(p.counts, b, p.n);          // workgroup-uniform
    const float dscale = n_b > 0 ? 2.0f * field_loss_mul(p.loss_scale, n_b) : 0.f;
    const float* points = p.points + (int64_t)b * p.n * D;
    const float* lod_b = p.lod != nullptr ? p.lod + (int64_t)b * p.n : nullptr;
    const int32_t* order = p.order != nullptr ? p.order + (int64_t)b * p.n : nullptr;
    const LodFieldSrc src_b{{p.d, p.tables + tab_off, p.noise, p.sample_base}, p.fade};
    float* grad = p.grads != nullptr ? p.grads + tab_off : nullptr;
    const float* target = p.target + row_off;
    float* y = p.y != nullptr ? p.y + row_off : nullptr;
    float* dpoints = p.dpoints + (int64_t)b * p.n * D;
    float* dlod = p.dlod + (int64_t)b * p.n;
    const int ks1 = (LF + 1) >> 1;
    const int64_t n_waves = (n_b + 63) >> 6;
    const WaveRange wr = field_range(n_waves, lb, p.groups);
    TrainAcc<KT> A;
    A.clear();
    for (int64_t g = wr.begin; g < wr.end; g += wr.step) {
        const int64_t wv = 4 * g + wave;
        if (wv >= n_waves) continue;                            // wave-uniform; nothing below synchronises the workgroup
        const int64_t pos = (wv << 6) + lane;
        const bool live_lane = pos < n_b;
        const int64_t row = ordered_row(order, n_b, live_lane ? pos : n_b - 1);      // a lane past the end takes the field's last point; it stores and adds nothing
        const float lam = point_lambda(lod_b, p.lod_uniform, row);                   // at the ROW, as the point
        uint32_t t[3];
        point_fixed<D>(p.d, points, row, t);
        encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, true>(src_b, t, row, lam, xrow);
        wave_sync();
        const unsigned long long live_mask = __ballot(live_lane);
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            const int src = 32 * nt + j;
            const bool mine = half == 0 && ((live_mask >> src) & 1ull);
            const int r = __shfl((int)row, src);                // row < n_b <= n < 2^31
            decoder_train_half<KT>(sm, xs, P, Q, nt, j, half, ks1, mine, target + (int64_t)r * 3, y != nullptr ? y + (int64_t)r * 3 : nullptr, dscale,
                                   true, A);
        }
        wave_sync();
        // d loss / d row of this lane's point is its row of the tile from here to the last wave_sync: the scatter and the walk only read it
        auto grow = [&](int l, float (&gv)[F]) {
#pragma unroll
            for (int f = 0; f < F; ++f) gv[f] = xrow[l * F + f];
        };
        if (grad != nullptr) scatter_point<D, F, true>(p.d, t, grad, p.fade, lam, live_lane, lane, grow);
        float gp[D], gl;
        point_walk<D, F, NIC_HASH_SRC_F32, true, true, NOISE>(src_b, t, row, lam, grow, gp, gl);
        if (live_lane) {
            store_point_grad<D>(dpoints, row, kept_axes<D>(p.d, points, row), gp);
            dlod[row] = lambda_passes(lod_b, p.lod_uniform, row) ? gl : 0.0f;
        }
        wave_sync();
    }
    write_record<KT>(sm, A, LF, p.partials + (int64_t)blockIdx.x * RecLayout(LF).rec, tid);      // record (b, lb); all zero without an item (n_b = 0 too)
}
template <bool NOISE>
static int launch_points_joint_lod(const PJLParams& p, int n_fields, void* stream) {
    const dim3 grid((unsigned)n_fields * (unsigned)p.groups);
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        constexpr int D = decltype(dim)::value, F = decltype(features)::value;
        if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_batch_points_joint_lod_kernel<D, F, 2, NOISE>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((hash_batch_points_joint_lod_kernel<D, F, 1, NOISE>), grid, dim3(256), 0, (hipStream_t)stream, p);
    });
}

// the fixed-order sum of the G records of every field into the stacked gradients and loss [B]; `counts` / `n_points` / `loss_scale` as the kernel reads them
static int launch_batch_reduce(const float* partials, int g, int lf, int n_fields, const nic_mlp_grads* mlp_grads, float* loss, float loss_mul, int flags,
                               const int32_t* counts, int64_t n_points, float loss_scale, void* stream) {
    hipLaunchKernelGGL(hash_batch_reduce_kernel, dim3((unsigned)((RecLayout(lf).rec + 31) / 32), (unsigned)n_fields), dim3(256), 0, (hipStream_t)stream,
                       partials, g, lf, *mlp_grads, loss, loss_mul, (flags & NIC_HASH_FUSED_ADD_GRADS) ? 1 : 0, (flags & NIC_HASH_FUSED_ADD_LOSS) ? 1 : 0,
                       counts, n_points, loss_scale);
    return (int)hipGetLastError();
}

// ---- the training step at points, the same at its four entry points: the batch counterpart of hash_common.hpp's points_fused_step ----------------
// The opening of an entry: the descriptor, the number of fields and G.  Each entry follows it with its own null list and, where it has a level of
// detail, its lodp / check_lod lines (_points_grad: a lod without lodp is refused, then check_lod where lodp is given), then the step below.
static int open_batch_points(const nic_hash_desc* desc, const nic_mlp* mlp, int n_fields, int groups_per_field, int64_t n_points, int& g) {
    if (!desc || !mlp) return NIC_E_NULL;
    const int rc = check_batch_desc(desc, mlp->n_linear);
    if (rc) return rc;
    if (n_fields < 1 || n_fields > kMaxFields) return NIC_E_ARG;
    g = point_groups(n_points, n_fields, groups_per_field);
    return g < 0 ? NIC_E_ARG : NIC_OK;
}
// From the flags on.  `p` arrives zeroed but for what only its entry has (the level of detail, dpoints, dlod); `launch(noise)` starts the entry's
// training kernel, `noise` a std::bool_constant
template <class Params, class Launch>
static int batch_points_step(Params& p, const nic_hash_desc* desc, int n_fields, int g, const nic_hash_quant* quant, const float* tables,
                             const float* points, int64_t n_points, const int32_t* counts, const int32_t* order, const nic_mlp* mlp, const float* target,
                             float loss_scale, float* table_grads, const nic_mlp_grads* mlp_grads, float* loss, float* y, int flags, void* workspace,
                             size_t workspace_bytes, void* stream, Launch launch) {
    if (flags & ~(NIC_HASH_FUSED_ADD_GRADS | NIC_HASH_FUSED_ADD_LOSS)) return NIC_E_ARG;
    p.d = *desc; p.tables = tables; p.points = points; p.counts = counts; p.order = order; p.target = target; p.y = y; p.grads = table_grads;
    fill_decoder(p, mlp);
    p.n = n_points; p.groups = g; p.loss_scale = loss_scale;
    p.noise.mode = NIC_NOISE_NONE;
    int rc = set_noise(quant, true, p.noise, p.sample_base);
    if (rc) return rc;
    const int lf = desc->levels * desc->features;
    if (workspace_bytes < (size_t)n_fields * g * RecLayout(lf).rec * sizeof(float)) return NIC_E_WORKSPACE;
    if ((rc = check_point_desc(desc)) != NIC_OK) return rc;
    if (n_points < 0 || n_points >= (int64_t(1) << 31)) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;                                   // nothing to launch: loss and every gradient output stay as they are
    p.partials = (float*)workspace;
    rc = p.noise.mode == NIC_NOISE_KERNEL ? launch(std::true_type{}) : launch(std::false_type{});
    if (rc != NIC_OK) return rc;
    kernel_end_mark((hipStream_t)stream);
    return launch_batch_reduce(p.partials, g, lf, n_fields, mlp_grads, loss, counts ? 0.f : field_loss_mul(loss_scale, n_points), flags, counts, n_points,
                               loss_scale, stream);
}

}  // namespace hbatch
}  // namespace nic

using namespace nic;
using namespace nic::hbatch;

extern "C" {

size_t nic_hash_batch_workspace_bytes(const nic_hash_desc* desc, int n_fields, int groups_per_field, const nic_mlp* mlp) {
    if (!desc || !mlp || check_batch_desc(desc, mlp->n_linear) != NIC_OK || n_fields < 1 || n_fields > kMaxFields) return 0;
    const int g = batch_groups(desc, n_fields, groups_per_field);
    if (g < 0) return 0;
    return (size_t)n_fields * g * RecLayout(desc->levels * desc->features).rec * sizeof(float);
}

int nic_hash_batch_forward(const nic_hash_desc* desc, int n_fields, int groups_per_field, const float* tables, const int32_t* origins,
                           const nic_mlp* mlp, float* y, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    const int rc = check_batch_desc(desc, mlp->n_linear);
    if (rc) return rc;
    if (n_fields < 1 || n_fields > kMaxFields) return NIC_E_ARG;
    const int g = batch_groups(desc, n_fields, groups_per_field);
    if (g < 0) return NIC_E_ARG;
    if (!tables || !origins || !mlp3_ok(mlp) || !y) return NIC_E_NULL;
    BParams p{};
    fill(p, desc, tables, origins, mlp, y, g);
    return launch<HB_FWD>(p, n_fields, stream);
}

int nic_hash_batch_forward_source(const nic_hash_desc* desc, int n_fields, int groups_per_field, const nic_hash_source* src, const int32_t* origins,
                                  const float* points, int64_t n_points, const nic_mlp* mlp, float* y, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((origins != nullptr) == (points != nullptr)) return NIC_E_ARG;
    if (points) {
        if ((rc = check_point_desc(desc)) != NIC_OK) return rc;
    } else if (256 * (int64_t)desc->S_max >= (int64_t(1) << 30)) {
        return NIC_E_ARG;
    }
    if (n_fields < 1 || n_fields > kMaxFields) return NIC_E_ARG;
    // G on the wave items of ONE field; a count of points that launches nothing (checked below) stands as one item here
    const int64_t n_items = origins ? count_patches(desc) : (n_points > 0 ? (n_points + 63) >> 6 : 1);
    const int g = batch_groups_of(n_items, n_fields, groups_per_field);
    if (g < 0) return NIC_E_ARG;
    if (!src || !src->data || !mlp3_ok(mlp) || !y) return NIC_E_NULL;
    SParams p{};
    p.d = *desc; p.origins = origins; p.points = points; p.y = y; p.groups = g; p.n_items = n_items;
    p.n = origins ? 0 : n_points;
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if (points && n_points < 0) return NIC_E_ARG;
    if (points && n_points == 0) return NIC_OK;
    p.stride = stacked_source_stride(desc, src);
    if (p.stride <= 0) return NIC_E_ARG;
    p.n_rows = origins ? (int64_t)desc->num_crops * desc->extent[0] * desc->extent[1] * (desc->dim == 3 ? desc->extent[2] : 1) : n_points;
    fill_decoder(p, mlp);
    return dispatch_source(src->kind, [&](auto kind) { return launch_source<decltype(kind)::value>(p, n_fields, stream); });
}

int nic_hash_batch_forward_backward(const nic_hash_desc* desc, int n_fields, int groups_per_field, const nic_hash_quant* quant, const float* tables,
                                    const int32_t* origins, const nic_mlp* mlp, const float* target, float loss_scale, float* table_grads,
                                    const nic_mlp_grads* mlp_grads, float* loss, float* y, int flags, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    const KernelEndDrop end;
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = check_batch_desc(desc, mlp->n_linear);
    if (rc) return rc;
    if (n_fields < 1 || n_fields > kMaxFields) return NIC_E_ARG;
    const int g = batch_groups(desc, n_fields, groups_per_field);
    if (g < 0) return NIC_E_ARG;
    if (!tables || !origins || !mlp3_ok(mlp) || !target || !mlp_grads || !loss || !workspace) return NIC_E_NULL;
    if (flags & ~(NIC_HASH_FUSED_ADD_GRADS | NIC_HASH_FUSED_ADD_LOSS)) return NIC_E_ARG;
    BParams p{};
    fill(p, desc, tables, origins, mlp, y, g);
    p.target = target; p.grads = table_grads;
    if ((rc = set_noise(quant, true, p.noise, p.sample_base)) != NIC_OK) return rc;
    const int lf = desc->levels * desc->features;
    if (workspace_bytes < (size_t)n_fields * g * RecLayout(lf).rec * sizeof(float)) return NIC_E_WORKSPACE;
    const float loss_mul = field_loss_mul(loss_scale, p.n_samples);
    p.dscale = 2.0f * loss_mul;
    p.partials = (float*)workspace;
    if ((rc = p.noise.mode == NIC_NOISE_KERNEL ? launch<HB_TRAIN_NOISY>(p, n_fields, stream) : launch<HB_TRAIN>(p, n_fields, stream)) != NIC_OK) return rc;
    kernel_end_mark((hipStream_t)stream);
    return launch_batch_reduce(p.partials, g, lf, n_fields, mlp_grads, loss, loss_mul, flags, nullptr, 0, loss_scale, stream);
}

// ---- with a level of detail per point: the siblings' checks in their order, lodp with the other pointers, check_lod right after them
int nic_hash_batch_forward_points_lod(const nic_hash_desc* desc, int n_fields, int groups_per_field, const nic_hash_lod* lodp, const nic_hash_source* src,
                                      const float* points, const float* lod, int64_t n_points, const nic_mlp* mlp, float* y, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((rc = check_point_desc(desc)) != NIC_OK) return rc;
    if (n_fields < 1 || n_fields > kMaxFields) return NIC_E_ARG;
    const int64_t n_items = n_points > 0 ? (n_points + 63) >> 6 : 1;     // a count that launches nothing (checked below) stands as one item here
    const int g = batch_groups_of(n_items, n_fields, groups_per_field);
    if (g < 0) return NIC_E_ARG;
    if (!lodp || !src || !src->data || !points || !mlp3_ok(mlp) || !y) return NIC_E_NULL;
    if ((rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    SLParams p{};
    p.d = *desc; p.points = points; p.y = y; p.groups = g; p.n_items = n_items; p.n = n_points; p.n_rows = n_points;
    set_lod(p, lodp, lod);
    if ((rc = set_point_source(p, src)) != NIC_OK) return rc;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    p.stride = stacked_source_stride(desc, src);
    if (p.stride <= 0) return NIC_E_ARG;
    fill_decoder(p, mlp);
    return dispatch_source(src->kind, [&](auto kind) { return launch_source_lod<decltype(kind)::value>(p, n_fields, stream); });
}

size_t nic_hash_batch_points_workspace_bytes(const nic_hash_desc* desc, int n_fields, int groups_per_field, int64_t n_points, const nic_mlp* mlp) {
    if (!desc || !mlp || check_batch_desc(desc, mlp->n_linear) != NIC_OK || n_fields < 1 || n_fields > kMaxFields) return 0;
    const int g = point_groups(n_points, n_fields, groups_per_field);
    if (g < 0 || check_point_desc(desc) != NIC_OK || n_points < 0 || n_points >= (int64_t(1) << 31)) return 0;
    return (size_t)n_fields * g * RecLayout(desc->levels * desc->features).rec * sizeof(float);
}

// ---- the training step at points: open_batch_points, the entry's own null list and level-of-detail lines, batch_points_step ----------------------
int nic_hash_batch_forward_backward_points(const nic_hash_desc* desc, int n_fields, int groups_per_field, const nic_hash_quant* quant, const float* tables,
                                           const float* points, int64_t n_points, const int32_t* counts, const int32_t* order, const nic_mlp* mlp,
                                           const float* target, float loss_scale, float* table_grads, const nic_mlp_grads* mlp_grads, float* loss,
                                           float* y, int flags, void* workspace, size_t workspace_bytes, void* stream) {
    const KernelEndDrop end;
    int g;
    const int rc = open_batch_points(desc, mlp, n_fields, groups_per_field, n_points, g);
    if (rc) return rc;
    if (!tables || !points || !mlp3_ok(mlp) || !target || !mlp_grads || !loss || !workspace) return NIC_E_NULL;
    PParams p{};
    return batch_points_step(p, desc, n_fields, g, quant, tables, points, n_points, counts, order, mlp, target, loss_scale, table_grads, mlp_grads, loss, y,
                             flags, workspace, workspace_bytes, stream,
                             [&](auto noise) { return launch_points<decltype(noise)::value>(p, n_fields, stream); });
}

// with a level of detail per point: lodp with the other pointers, check_lod right after them
int nic_hash_batch_forward_backward_points_lod(const nic_hash_desc* desc, int n_fields, int groups_per_field, const nic_hash_lod* lodp,
                                               const nic_hash_quant* quant, const float* tables, const float* points, const float* lod, int64_t n_points,
                                               const int32_t* counts, const int32_t* order, const nic_mlp* mlp, const float* target, float loss_scale,
                                               float* table_grads, const nic_mlp_grads* mlp_grads, float* loss, float* y, int flags, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    const KernelEndDrop end;
    int g;
    int rc = open_batch_points(desc, mlp, n_fields, groups_per_field, n_points, g);
    if (rc) return rc;
    if (!lodp || !tables || !points || !mlp3_ok(mlp) || !target || !mlp_grads || !loss || !workspace) return NIC_E_NULL;
    if ((rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    PLParams p{};
    p.d = *desc;                                                         // set_lod reads the levels
    set_lod(p, lodp, lod);
    return batch_points_step(p, desc, n_fields, g, quant, tables, points, n_points, counts, order, mlp, target, loss_scale, table_grads, mlp_grads, loss, y,
                             flags, workspace, workspace_bytes, stream,
                             [&](auto noise) { return launch_points_lod<decltype(noise)::value>(p, n_fields, stream); });
}

// the step that also writes d loss / d points: nic_hash_batch_forward_backward_points with lodp == NULL, else ..._points_lod,
// argument for argument, dpoints with the other pointers
int nic_hash_batch_forward_backward_points_grad(const nic_hash_desc* desc, int n_fields, int groups_per_field, const nic_hash_lod* lodp,
                                                const nic_hash_quant* quant, const float* tables, const float* points, const float* lod, int64_t n_points,
                                                const int32_t* counts, const int32_t* order, const nic_mlp* mlp, const float* target, float loss_scale,
                                                float* table_grads, const nic_mlp_grads* mlp_grads, float* loss, float* y, float* dpoints, int flags,
                                                void* workspace, size_t workspace_bytes, void* stream) {
    const KernelEndDrop end;
    int g;
    int rc = open_batch_points(desc, mlp, n_fields, groups_per_field, n_points, g);
    if (rc) return rc;
    if (!tables || !points || !mlp3_ok(mlp) || !target || !mlp_grads || !loss || !dpoints || !workspace) return NIC_E_NULL;
    if (!lodp && lod) return NIC_E_ARG;                                  // a null nic_hash_lod is "no level of detail" and takes no per-point array
    if (lodp && (rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    PJParams p{};
    p.d = *desc;                                                         // set_lod reads the levels
    p.dpoints = dpoints;
    if (lodp) set_lod(p, lodp, lod);
    return batch_points_step(p, desc, n_fields, g, quant, tables, points, n_points, counts, order, mlp, target, loss_scale, table_grads, mlp_grads, loss, y,
                             flags, workspace, workspace_bytes, stream, [&](auto noise) {
                                 constexpr bool NOISE = decltype(noise)::value;
                                 return lodp ? launch_points_joint<NOISE, true>(p, n_fields, stream) : launch_points_joint<NOISE, false>(p, n_fields, stream);
                             });
}

// the same step that also writes d loss / d lambda: the entry above with a level of detail always on and dlod after dpoints, lodp
// and dlod with the other pointers
int nic_hash_batch_forward_backward_points_grad_lod(const nic_hash_desc* desc, int n_fields, int groups_per_field, const nic_hash_lod* lodp,
                                                    const nic_hash_quant* quant, const float* tables, const float* points, const float* lod,
                                                    int64_t n_points, const int32_t* counts, const int32_t* order, const nic_mlp* mlp,
                                                    const float* target, float loss_scale, float* table_grads, const nic_mlp_grads* mlp_grads,
                                                    float* loss, float* y, float* dpoints, float* dlod, int flags, void* workspace,
                                                    size_t workspace_bytes, void* stream) {
    const KernelEndDrop end;
    int g;
    int rc = open_batch_points(desc, mlp, n_fields, groups_per_field, n_points, g);
    if (rc) return rc;
    if (!lodp || !tables || !points || !mlp3_ok(mlp) || !target || !mlp_grads || !loss || !dpoints || !dlod || !workspace) return NIC_E_NULL;
    if ((rc = check_lod(desc, lodp)) != NIC_OK) return rc;
    PJLParams p{};
    p.d = *desc;                                                         // set_lod reads the levels
    p.dpoints = dpoints; p.dlod = dlod;
    set_lod(p, lodp, lod);
    return batch_points_step(p, desc, n_fields, g, quant, tables, points, n_points, counts, order, mlp, target, loss_scale, table_grads, mlp_grads, loss, y,
                             flags, workspace, workspace_bytes, stream,
                             [&](auto noise) { return launch_points_joint_lod<decltype(noise)::value>(p, n_fields, stream); });
}

}  // extern "C"
