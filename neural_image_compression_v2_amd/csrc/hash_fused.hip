// Hash-grid encoding + ColorDecoder(L F, 64, 3) in ONE kernel (include/nicv2_hip.h: nic_hash_fused_*; hashgrid.py, HashGridField(fused=True);
// DESIGN 4.7.2).  The [N, L F] encoding row and its gradient never reach global memory: a wave gathers the rows of its patch into an LDS tile,
// runs the decoder forward and backward on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32: an exact fmaf chain, the arithmetic of the general
// decoder the layer-wise route uses), leaves d loss / d row in the same tile and scatters it into the table gradient with the run sums of
// hash_encode_backward_kernel.  Semantics are those of hash_grid.hip; the helpers, LDS layout and record layout are hash_common.hpp's.
//
//   one wave per patch of 8 x 8 (2D) / 4 x 4 x 4 (3D) samples, x the fastest lane axis (the row numbering of nic_hash_encode: the noise keys
//   and the run sums carry over); 4 waves per workgroup, one workgroup per CU, persistent, each XCD walks one contiguous range of patches.
//   MLP: a wave's 64 samples in two halves of 32 (nt).  Z^T[h][n] = sum_k W[h][k] A[n][k]: the hidden unit is the MFMA row, the sample the
//   column, so register r of lane (j, half) holds unit rho = 32 t + (r & 3) + 8 (r >> 2) + 4 half of sample 32 nt + j - and that register IS
//   the B operand of k-step (t, r) of the next product (the reduction index may be walked in any order); only the weights come from LDS.
//   Weight gradients reduce over the samples, which sit in the lanes: dZ and A go through two 16-sample LDS tiles per wave ([n][unit]) and
//   come back as operands; their accumulators stay in registers for the whole launch and leave as one record per workgroup (summed over the
//   four waves in wave order through LDS), which hash_fused_reduce_kernel adds up in a fixed order - with the optimiser tail riding on it.
#include "hash_common.hpp"

namespace nic {
namespace hfused {
using namespace hcommon;

enum { HF_FWD = 0, HF_FWD_U8 = 1, HF_TRAIN = 2, HF_FWD_BITS = 3 };

struct FParams {
    nic_hash_desc d;
    const float* table;
    const uint8_t* stored;
    const int32_t* origins;
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const float* target;
    float* y;
    float* grad;              // table gradient (null: frozen table, no scatter)
    float* partials;          // one record per workgroup
    NoiseSrc noise;           // mode NIC_NOISE_NONE / NIC_NOISE_KERNEL
    uint64_t sample_base;
    float q_scale, q_bias;
    float dscale;             // 2 loss_scale / (3 N)
    int64_t n_patches;
    // HF_FWD_BITS only (appended: the other modes read the fields above at the offsets they always had)
    const uint32_t* packed;   // bit-packed table, 4-byte aligned
    int32_t q_bits, q_tight;  // b; F b divides 32 or is 64 (hash_grid.hip, load_row_bits)
};

// the level loop of hash_encode_kernel with the row going to LDS
template <int D, int F, int MODE, bool TIGHT = false>
__device__ __forceinline__ void encode_row(const FParams& p, const PatchSample<D>& s, const uint32_t (&i)[3], float* xrow) {
    const nic_hash_desc& d = p.d;
    const uint32_t S2 = 2u * (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    [[maybe_unused]] int64_t lev_off = 0;
    [[maybe_unused]] int64_t lev_dw = 0;
    [[maybe_unused]] U4 nblk{0u, 0u, 0u, 0u};
    [[maybe_unused]] const bool noisy = MODE == HF_TRAIN && p.noise.mode == NIC_NOISE_KERNEL;
#pragma unroll 2
    for (int l = 0; l < d.levels; ++l) {
        const uint32_t R = (uint32_t)d.resolution[l];
        const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
        const float* tab = p.table + ((int64_t)l << d.log2_table) * F;
        [[maybe_unused]] const uint8_t* stab = nullptr;
        if constexpr (MODE == HF_FWD_U8) {
            stab = p.stored + lev_off;
            lev_off += (int64_t)F * hash_level_entries(D, (int32_t)R, d.log2_table);
        }
        [[maybe_unused]] const uint32_t* btab = nullptr;
        if constexpr (MODE == HF_FWD_BITS) {
            btab = p.packed + lev_dw;
            lev_dw += hash_level_dwords(D, (int32_t)R, d.log2_table, F, p.q_bits);
        }
        uint32_t v[3];
        float w[3];
        level_cell<D>(i, R, S2, v, w);
        float acc[F];
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = 0.f;
#pragma unroll
        for (int c = 0; c < (1 << D); ++c) {
            const uint32_t e = hash_index(dense, R, mask, v[0] + (c & 1), v[1] + ((c >> 1) & 1), D == 3 ? v[2] + ((c >> 2) & 1) : 0u);
            float t[F];
            if constexpr (MODE == HF_FWD_U8) load_row_u8<F>(stab + (int64_t)e * F, p.q_scale, p.q_bias, t);
            else if constexpr (MODE == HF_FWD_BITS) load_row_bits<F, TIGHT>(btab, e, p.q_bits, p.q_scale, p.q_bias, t);
            else load_row<F>(tab + (int64_t)e * F, t);
            const float cw = corner_weight<D>(w, c);
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] += cw * t[f];
        }
        if constexpr (MODE == HF_TRAIN) {
            if (noisy) {
                const int c0 = l * F;
                if ((c0 & 15) == 0) nblk = noise_block(p.noise, p.sample_base + (uint64_t)s.n, c0 >> 4);
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] += noise_from_block(p.noise, nblk, (c0 + f) & 15);
            }
        }
#pragma unroll
        for (int f = 0; f < F; ++f) xrow[l * F + f] = acc[f];
    }
}

// the level loop of hash_encode_backward_kernel with d loss / d row coming from LDS
template <int D, int F>
__device__ __forceinline__ void scatter_row(const FParams& p, const PatchSample<D>& s, const uint32_t (&i)[3], const float* xrow, int lane) {
    const nic_hash_desc& d = p.d;
    const uint32_t S2 = 2u * (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    for (int l = 0; l < d.levels; ++l) {
        const uint32_t R = (uint32_t)d.resolution[l];
        const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
        float* gtab = p.grad + ((int64_t)l << d.log2_table) * F;
        uint32_t v[3];
        float w[3];
        level_cell<D>(i, R, S2, v, w);
        float g[F];
#pragma unroll
        for (int f = 0; f < F; ++f) g[f] = s.live ? xrow[l * F + f] : 0.f;
        const int64_t key = (int64_t)v[0] + ((int64_t)R + 1) * ((int64_t)v[1] + ((int64_t)R + 1) * (int64_t)v[2]);
        const RunMasks m = run_masks(s.live ? key : -1 - (int64_t)lane, lane);
        const bool issue = s.live && m.head;
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

// The decoder keeps its own body in every mode: hash_common.hpp's decoder_forward_half / decoder_train_half / write_record are the same products
// in the same order but compile to other code, which has not been measured against this body on a GPU.
template <int D, int F, int KT, int MODE>
__global__ void __launch_bounds__(256) hash_fused_kernel(const FParams p) {
    __shared__ TrainSmem sm;
    constexpr bool TRAIN = MODE == HF_TRAIN;
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
    [[maybe_unused]] float* P = sm.p[wave];
    [[maybe_unused]] float* Q = sm.q[wave];

    [[maybe_unused]] f32x16 gW1[2][KT], gW2[2][2], gW3[1][2];
    [[maybe_unused]] float gb1[2] = {0.f, 0.f}, gb2[2] = {0.f, 0.f}, gb3[1] = {0.f}, sse = 0.f;
    if constexpr (TRAIN) {
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int b = 0; b < KT; ++b) gW1[a][b] = f32x16{};
            gW2[a][0] = f32x16{}; gW2[a][1] = f32x16{};
            gW3[0][a] = f32x16{};
        }
    }

    // each XCD (blocks b, b + 8, ..) walks one contiguous range of groups of 4 patches
    const int xcd = blockIdx.x & 7, nb8 = gridDim.x >> 3;
    const int64_t n_groups = (p.n_patches + 3) >> 2, chunk = (n_groups + 7) >> 3;
    const int64_t g_begin = xcd * chunk, g_end = g_begin + chunk < n_groups ? g_begin + chunk : n_groups;
    const int ks1 = (LF + 1) >> 1;
    for (int64_t g = g_begin + (blockIdx.x >> 3); g < g_end; g += nb8) {
        const int64_t wv = 4 * g + wave;
        if (wv >= p.n_patches) continue;                        // wave-uniform; nothing below synchronises the workgroup
        const PatchSample<D> s = patch_sample<D>(p.d, wv, p.n_patches, lane);
        uint32_t ci[3];
        sample_coords<D>(p.d, p.origins, s, ci);
        if constexpr (MODE == HF_FWD_BITS) {                     // b is uniform over the launch: the window's width is decided once per row
            if (p.q_tight) encode_row<D, F, MODE, true>(p, s, ci, xrow);
            else encode_row<D, F, MODE, false>(p, s, ci, xrow);
        } else {
            encode_row<D, F, MODE>(p, s, ci, xrow);
        }
        wave_sync();
        const unsigned long long live_mask = __ballot(s.live);
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            const int src = 32 * nt + j;
            const bool live = (live_mask >> src) & 1ull;
            const int64_t n = (int64_t)(uint32_t)__shfl((int)(uint32_t)s.n, src) | ((int64_t)__shfl((int)(s.n >> 32), src) << 32);
            const float* xb = xs + src * XS;
            // ---- layer 1
            f32x16 a1[2] = {f32x16{}, f32x16{}};
            [[maybe_unused]] f32x16 d1[2];
            for (int k = 0; k < ks1; ++k) {
                const float b = xb[2 * k + half];
                a1[0] = mfma(sm.w1[j * XS + 2 * k + half], b, a1[0]);
                a1[1] = mfma(sm.w1[(32 + j) * XS + 2 * k + half], b, a1[1]);
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float av, dv;
                    gelu_and_grad(a1[t][r] + sm.b1[32 * t + row_of(r, half)], av, dv);
                    a1[t][r] = av;
                    if constexpr (TRAIN) d1[t][r] = dv;
                }
            // ---- layer 2
            f32x16 a2[2] = {f32x16{}, f32x16{}};
            [[maybe_unused]] f32x16 d2[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = 32 * t + row_of(r, half);
                    a2[0] = mfma(sm.w2[j * XS + k], a1[t][r], a2[0]);
                    a2[1] = mfma(sm.w2[(32 + j) * XS + k], a1[t][r], a2[1]);
                }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float av, dv;
                    gelu_and_grad(a2[t][r] + sm.b2[32 * t + row_of(r, half)], av, dv);
                    a2[t][r] = av;
                    if constexpr (TRAIN) d2[t][r] = dv;
                }
            // ---- output layer: rows 0 .. 2 of one tile (registers 0 .. 2 of half 0)
            f32x16 z3 = f32x16{};
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = 32 * t + row_of(r, half);
                    z3 = mfma(j < 3 ? sm.w3[j * kH + k] : 0.f, a2[t][r], z3);
                }
            float yv[3];
#pragma unroll
            for (int o = 0; o < 3; ++o) yv[o] = sigmoid_f(z3[o] + sm.b3[o]);
            const bool mine = half == 0 && live;
            if (mine && p.y != nullptr) {
#pragma unroll
                for (int o = 0; o < 3; ++o) p.y[n * 3 + o] = yv[o];
            }
            if constexpr (TRAIN) {
                // ---- dZ3 = dy y (1 - y), dy = 2 (y - t) loss_scale / (3 N)
                float dz3[4] = {0.f, 0.f, 0.f, 0.f};
                if (mine) {
#pragma unroll
                    for (int o = 0; o < 3; ++o) {
                        const float e = yv[o] - p.target[n * 3 + o];
                        sse += e * e;
                        dz3[o] = p.dscale * e * yv[o] * (1.0f - yv[o]);
                    }
                }
                // dW3 [o][h] += dZ3^T A2
#pragma unroll 1
                for (int q = 0; q < 2; ++q) {
                    if ((j >> 4) == q) {
                        put_tile<2>(Q, j, half, a2);
                        if (half == 0) {
#pragma unroll
                            for (int o = 0; o < 4; ++o) P[(j & 15) * XS + o] = dz3[o];
                        }
                    }
                    wave_sync();
                    wgrad_mfma<1, 2, true>(P, Q, j, half, gW3, gb3);
                    wave_sync();
                }
                // dA2 = W3^T dZ3 (k-steps: o = s of half 0; half 1 carries zeros), dZ2 = dA2 gelu'
                f32x16 dz2[2] = {f32x16{}, f32x16{}};
#pragma unroll
                for (int o = 0; o < 3; ++o) {
                    const float b = half == 0 ? dz3[o] : 0.f;
                    dz2[0] = mfma(half == 0 ? sm.w3[o * kH + j] : 0.f, b, dz2[0]);
                    dz2[1] = mfma(half == 0 ? sm.w3[o * kH + 32 + j] : 0.f, b, dz2[1]);
                }
#pragma unroll
                for (int t = 0; t < 2; ++t) dz2[t] *= d2[t];
                // dW2 [h2][h] += dZ2^T A1
#pragma unroll 1
                for (int q = 0; q < 2; ++q) {
                    if ((j >> 4) == q) {
                        put_tile<2>(P, j, half, dz2);
                        put_tile<2>(Q, j, half, a1);
                    }
                    wave_sync();
                    wgrad_mfma<2, 2, false>(P, Q, j, half, gW2, gb2);
                    wave_sync();
                }
                // dA1 = W2^T dZ2, dZ1 = dA1 gelu'
                f32x16 dz1[2] = {f32x16{}, f32x16{}};
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int k = 32 * t + row_of(r, half);
                        dz1[0] = mfma(sm.w2[k * XS + j], dz2[t][r], dz1[0]);
                        dz1[1] = mfma(sm.w2[k * XS + 32 + j], dz2[t][r], dz1[1]);
                    }
#pragma unroll
                for (int t = 0; t < 2; ++t) dz1[t] *= d1[t];
                // dW1 [h][k] += dZ1^T X (X: the rows of this half, in place)
#pragma unroll 1
                for (int q = 0; q < 2; ++q) {
                    if ((j >> 4) == q) put_tile<2>(P, j, half, dz1);
                    wave_sync();
                    wgrad_mfma<2, KT, false>(P, xs + (32 * nt + 16 * q) * XS, j, half, gW1, gb1);
                    wave_sync();
                }
                // dX = W1^T dZ1 over the rows of this half (their X is spent)
                if (p.grad != nullptr) {
                    f32x16 dx[KT];
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt) dx[kt] = f32x16{};
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int h = 32 * t + row_of(r, half);
#pragma unroll
                            for (int kt = 0; kt < KT; ++kt) dx[kt] = mfma(sm.w1[h * XS + 32 * kt + j], dz1[t][r], dx[kt]);
                        }
                    float* xw = xs + src * XS;
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) xw[32 * kt + row_of(r, half)] = dx[kt][r];
                }
            }
        }
        if constexpr (TRAIN) {
            wave_sync();
            if (p.grad != nullptr) scatter_row<D, F>(p, s, ci, xrow, lane);
            wave_sync();
        } else {
            wave_sync();
        }
    }

    if constexpr (TRAIN) {
        // ---- the workgroup's record: the four waves add their accumulators in wave order into the (now free) row tiles
        const RecLayout rl(LF);
        float* R = &sm.x[0][0];
        __syncthreads();
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
                const bool first = w == 0;
                auto put = [&](int at, float v) { R[at] = first ? v : R[at] + v; };
#pragma unroll
                for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int h = 32 * ta + row_of(r, half);
#pragma unroll
                        for (int tb = 0; tb < KT; ++tb)
                            if (32 * tb + j < LF) put(rl.w1 + h * LF + 32 * tb + j, gW1[ta][tb][r]);
#pragma unroll
                        for (int tb = 0; tb < 2; ++tb) put(rl.w2 + h * kH + 32 * tb + j, gW2[ta][tb][r]);
                    }
#pragma unroll
                for (int ta = 0; ta < 2; ++ta) {                 // lane (i, half) summed the samples of parity `half`
                    const float s1 = gb1[ta] + __shfl_xor(gb1[ta], 32), s2 = gb2[ta] + __shfl_xor(gb2[ta], 32);
                    if (half == 0) { put(rl.b1 + 32 * ta + j, s1); put(rl.b2 + 32 * ta + j, s2); }
                }
                const float s3 = gb3[0] + __shfl_xor(gb3[0], 32);
                if (lane < 3) put(rl.b3 + lane, s3);
#pragma unroll
                for (int o = 0; o < 3; ++o) {
                    if (half == 0) { put(rl.w3 + o * kH + j, gW3[0][0][o]); put(rl.w3 + o * kH + 32 + j, gW3[0][1][o]); }
                }
                const float sl = half_sum(sse);
                if (lane == 0) put(rl.loss, sl);
            }
            __syncthreads();
        }
        float* rec = p.partials + (int64_t)blockIdx.x * rl.rec;
        for (int e = tid; e < rl.rec; e += 256) rec[e] = R[e];
    }
}

// Fixed-order sum of the records: a block = 32 outputs x 8 slices of the record list, the slices combined through LDS in slice order
// (reduce_partials_kernel's shape).  add_grads / add_loss: the result is added to what the buffers hold (a chunked pass).
__global__ void __launch_bounds__(256) hash_fused_reduce_kernel(const float* partials, int n_rec, int lf, nic_mlp_grads g, float* loss, float loss_mul,
                                                                int add_grads, int add_loss, const StepTail tl) {
    if (tail_block(tl)) return;
    __shared__ float red[8][32];
    const RecLayout rl(lf);
    const int slice = threadIdx.x >> 5, e = blockIdx.x * 32 + (threadIdx.x & 31);
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    const int per = (n_rec + 7) >> 3, w_lo = slice * per, w_hi = w_lo + per < n_rec ? w_lo + per : n_rec;
    if (e < rl.rec) {
        const float* src = partials + e;
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
        if (loss) *loss = add_loss ? *loss + acc * loss_mul : acc * loss_mul;
        return;
    }
    float* dst = e < rl.b1 ? (g.w[0] ? g.w[0] + e : nullptr) : e < rl.w2 ? (g.b[0] ? g.b[0] + (e - rl.b1) : nullptr)
               : e < rl.b2 ? (g.w[1] ? g.w[1] + (e - rl.w2) : nullptr) : e < rl.w3 ? (g.b[1] ? g.b[1] + (e - rl.b2) : nullptr)
               : e < rl.b3 ? (g.w[2] ? g.w[2] + (e - rl.w3) : nullptr) : (g.b[2] ? g.b[2] + (e - rl.b3) : nullptr);
    if (!dst) return;
    if (add_grads) acc += *dst;
    if (tl.t.count > 0) tail_store(tl, dst, acc);
    else *dst = acc;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// the supported set, the only copy: dim 2 / 3, F in {1, 2, 4, 8}, L F <= 64, hidden 64, 3 Linear layers
static int supported(const nic_hash_desc* d, int hidden, int n_linear) {
    const int rc = check_hash_desc(d);
    if (rc) return rc;
    if (d->levels * d->features > kH) return NIC_E_UNSUPPORTED;
    if (hidden != kH || (n_linear != 3 && n_linear != 0)) return NIC_E_UNSUPPORTED;
    return NIC_OK;
}
static bool mlp3_ok(const nic_mlp* m) {
    for (int i = 0; i < 3; ++i)
        if (!m->w[i] || !m->b[i]) return false;
    return true;
}

template <int MODE, int D, int F>
static void launch_kt(const FParams& p, int grid, hipStream_t s) {
    if (p.d.levels * F > 32) hipLaunchKernelGGL((hash_fused_kernel<D, F, 2, MODE>), dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((hash_fused_kernel<D, F, 1, MODE>), dim3(grid), dim3(256), 0, s, p);
}
template <int MODE>
static int launch(const FParams& p, int grid, void* stream) {
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        launch_kt<MODE, decltype(dim)::value, decltype(features)::value>(p, grid, (hipStream_t)stream);
    });
}

static void fill_common(FParams& p, const nic_hash_desc* d, const int32_t* origins, const nic_mlp* mlp, float* y) {
    p.d = *d; p.origins = origins; p.y = y;
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
    p.n_patches = count_patches(d);
    p.noise.mode = NIC_NOISE_NONE;
}

}  // namespace hfused
}  // namespace nic

using namespace nic;
using namespace nic::hfused;

extern "C" {

int nic_hash_fused_supported(const nic_hash_desc* desc, int hidden, int n_linear) { return supported(desc, hidden, n_linear); }

size_t nic_hash_fused_workspace_bytes(const nic_hash_desc* desc, const nic_mlp* mlp) {
    if (!desc || !mlp || supported(desc, kH, mlp->n_linear) != NIC_OK) return 0;
    return (size_t)wg_cap() * RecLayout(desc->levels * desc->features).rec * sizeof(float);
}

int nic_hash_fused_forward(const nic_hash_desc* desc, const float* table, const int32_t* origins, const nic_mlp* mlp, float* y, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    const int rc = supported(desc, kH, mlp->n_linear);
    if (rc) return rc;
    if (!table || !origins || !mlp3_ok(mlp) || !y) return NIC_E_NULL;
    FParams p{};
    fill_common(p, desc, origins, mlp, y);
    p.table = table;
    return launch<HF_FWD>(p, persistent_grid(p.n_patches), stream);
}

int nic_hash_fused_forward_u8(const nic_hash_desc* desc, int num_bits, const uint8_t* stored, const int32_t* origins, const nic_mlp* mlp, float* y,
                              void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    const int rc = supported(desc, kH, mlp->n_linear);
    if (rc) return rc;
    if (!stored || !origins || !mlp3_ok(mlp) || !y) return NIC_E_NULL;
    if (num_bits < 1 || num_bits > 8) return NIC_E_ARG;
    FParams p{};
    fill_common(p, desc, origins, mlp, y);
    p.stored = stored;
    set_dequant(p, num_bits);
    return launch<HF_FWD_U8>(p, persistent_grid(p.n_patches), stream);
}

int nic_hash_fused_forward_bits(const nic_hash_desc* desc, int num_bits, const uint8_t* packed, const int32_t* origins, const nic_mlp* mlp, float* y,
                                void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    const int rc = supported(desc, kH, mlp->n_linear);
    if (rc) return rc;
    if (!packed || !origins || !mlp3_ok(mlp) || !y) return NIC_E_NULL;
    if (num_bits < 1 || num_bits > 8) return NIC_E_ARG;
    if ((uintptr_t)packed & 3u) return NIC_E_ARG;                    // the gather reads aligned dwords
    FParams p{};
    fill_common(p, desc, origins, mlp, y);
    p.packed = (const uint32_t*)packed;
    p.q_bits = num_bits; p.q_tight = hash_bits_tight(desc->features, num_bits) ? 1 : 0;
    set_dequant(p, num_bits);
    return launch<HF_FWD_BITS>(p, persistent_grid(p.n_patches), stream);
}

int nic_hash_fused_forward_backward(const nic_hash_desc* desc, const nic_hash_quant* quant, const float* table, const int32_t* origins,
                                    const nic_mlp* mlp, const float* target, float loss_scale, float* table_grad, const nic_mlp_grads* mlp_grads,
                                    float* loss, float* y, int flags, void* workspace, size_t workspace_bytes, const nic_step_tail* tail,
                                    void* stream) {
    const KernelEndDrop end;
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = supported(desc, kH, mlp->n_linear);
    if (rc) return rc;
    if (!table || !origins || !mlp3_ok(mlp) || !target || !mlp_grads || !loss || !workspace) return NIC_E_NULL;
    if (flags & ~(NIC_HASH_FUSED_ADD_GRADS | NIC_HASH_FUSED_ADD_LOSS)) return NIC_E_ARG;
    FParams p{};
    fill_common(p, desc, origins, mlp, y);
    p.table = table; p.target = target; p.grad = table_grad;
    if ((rc = set_noise(quant, true, p.noise, p.sample_base)) != NIC_OK) return rc;
    const int lf = desc->levels * desc->features, grid = persistent_grid(p.n_patches);
    if (workspace_bytes < (size_t)grid * RecLayout(lf).rec * sizeof(float)) return NIC_E_WORKSPACE;
    FusedTail ft;
    if ((rc = check_fused_tail(tail, mlp_grads, lf, ft)) != NIC_OK) return rc;
    const double n_samples = (double)desc->num_crops * desc->extent[0] * desc->extent[1] * (desc->dim == 3 ? desc->extent[2] : 1);
    const float loss_mul = (float)((double)loss_scale / (3.0 * n_samples));
    p.dscale = 2.0f * loss_mul;
    p.partials = (float*)workspace;
    return finish_fused_step(ft, mlp_grads, flags, lf, grid, loss_mul, loss, p.partials, stream, [&] { return launch<HF_TRAIN>(p, grid, stream); });
}

}  // extern "C"
