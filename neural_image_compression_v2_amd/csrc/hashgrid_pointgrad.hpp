// The second level walk of the hash-grid point kernels, the one copy of it: the gradient with respect
// to the point coordinates and, on request, to the level of detail.  hashgrid_pointgrad.hip and hashgrid_lodgrad.hip (the field's parameters
// constant), hashgrid_points_joint.hip and hashgrid_lodtrain.hip (the training step that also hands the gradients back) and the batched forms
// (hashgrid_batch_grad.hip, hashgrid_batch.hip's joint kernel) include this header; so is the decoder's backward to the input alone.  `s` is
// whatever holds the source - a kernel's parameter struct: d, the table of SRC, with LOD fade, with NOISE noise and sample_base - and each field
// is read where the loop uses it, as in encode_point_levels (hash_common.hpp).  Everything is force-inlined.
#pragma once
#include "hash_common.hpp"

namespace nic {
namespace hcommon {

// bit a: the floating-point clamp of point_fixed kept p_a as it was (a NaN fails both comparisons)
template <int D>
__device__ __forceinline__ uint32_t kept_axes(const nic_hash_desc& d, const float* points, int64_t n) {
    uint32_t m = 0u;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const float x = points[n * D + a];
        if (x >= -0.5f && x <= (float)d.extent[a] - 0.5f) m |= 1u << a;
    }
    return m;
}
// lambda_raw = (lod ? lod[n] : 0) + lod_uniform of point_lambda before its clamps: the clamp passes the gradient on [0, 32) (the right-hand
// derivative of the clamp; a NaN fails both comparisons)
__device__ __forceinline__ bool lambda_passes(const float* lod, float lod_uniform, int64_t n) {
    const float v = __fadd_rn(lod != nullptr ? lod[n] : 0.f, lod_uniform);
    return v >= 0.f && v < 32.f;
}

// The level loop of encode_point_levels (same offsets, same index, same loaders, same point_cell) with the D signed weights per corner in the
// place of the one weight.  `grow(l, gv)` hands over the F values of d loss / d row of level l; with cw_a(c) = c_a ? w_a : 1 - w_a,
//     dot(l, c) = sum_f grow(l)[f] value[l, idx(v + c), f],
//     g[a] = sum_l a_l (R_l / S_max) sum_c (c_a ? +1 : -1) prod_{b != a} cw_b(c) dot(l, c).
// LOD: a_l = clamp(a_raw, 0, 1), a_raw = (fade[l] - lambda) + 1; a level of weight 0 is not gathered, a level no lane of the wave weighs is
// jumped over by the wave.
// DLOD: column l F + f of the row is a_l r[l, f], so d column / d lambda = -r[l, f] on the ramp 0 < a_raw <= 1 (the right-hand derivative: a
// level exactly at its fade start has slope -1, one exactly at its end slope 0) and 0 elsewhere,
//     glam = - sum_{l on the ramp} sum_c prod_a cw_a(c) dot(l, c)
// - one more accumulator on the corners the walk gathers anyway.  Without DLOD `glam` is not touched.
// NOISE (training: the fp32 table only): the column is a_l (r[l, f] + nz[l F + f]), nz the codec noise the forward added, so
//     glam = - sum_{l on the ramp} (sum_c prod_a cw_a(c) dot(l, c) + sum_f grow(l)[f] nz[l F + f]).
// nz is regenerated, not carried: the same key sample_base + n (n the caller's row), the same generator block, the same noise_from_block.  The
// block of columns (l F) & ~15 .. is made by the first level ON THE RAMP of this lane that needs it (encode_point_levels' caching rule on the
// levels that read it here) and lives in registers.
// One body, so `g` is the same bits whatever is asked for on top of it, and with a level of detail at weight 1 it is the plain walk's.
template <int D, int F, int SRC, bool TIGHT, bool LOD, bool DLOD, bool NOISE, class Src, class GRow>
__device__ __forceinline__ void point_walk_levels(const Src& s, const uint32_t (&t)[3], [[maybe_unused]] int64_t n, float lam, GRow grow, float (&g)[D],
                                                  [[maybe_unused]] float& glam) {
    static_assert(!DLOD || LOD, "d / d lambda needs a level of detail");
    static_assert(!NOISE || (DLOD && SRC == NIC_HASH_SRC_F32), "the noise is a term of d / d lambda, and training reads the fp32 table");
    const nic_hash_desc& d = s.d;
    const uint32_t S = (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const float fdiv = (float)(256u * S);
    [[maybe_unused]] int64_t lev_off = 0;              // _U8: byte offset of level l
    [[maybe_unused]] int64_t lev_dw = 0;               // _BITS: dword offset of level l
    [[maybe_unused]] U4 nblk{0u, 0u, 0u, 0u};          // NOISE: the generator block `nblk_id` of this lane's sample (-1: none yet)
    [[maybe_unused]] int nblk_id = -1;
#pragma unroll
    for (int a = 0; a < D; ++a) g[a] = 0.f;
    if constexpr (DLOD) glam = 0.f;
    for (int l = 0; l < d.levels; ++l) {
        const uint32_t R = (uint32_t)d.resolution[l];
        [[maybe_unused]] const float* tab = nullptr;
        if constexpr (SRC == NIC_HASH_SRC_F32) tab = s.table + ((int64_t)l << d.log2_table) * F;
        [[maybe_unused]] const uint8_t* stab = nullptr;
        if constexpr (SRC == NIC_HASH_SRC_U8) {
            stab = s.stored + lev_off;
            lev_off += (int64_t)F * hash_level_entries(D, (int32_t)R, d.log2_table);
        }
        [[maybe_unused]] const uint32_t* btab = nullptr;
        if constexpr (SRC == NIC_HASH_SRC_BITS) {
            btab = s.packed + lev_dw;
            lev_dw += hash_level_dwords(D, (int32_t)R, d.log2_table, F, s.q_bits);
        }
        // level_weight's expression before its clamp, in its order: the ramp is decided on it
        [[maybe_unused]] float a_raw = 0.f;
        if constexpr (DLOD) a_raw = __fadd_rn(__fsub_rn(s.fade[l], lam), 1.0f);
        [[maybe_unused]] float wl = 1.0f;
        if constexpr (LOD) wl = level_weight(s.fade[l], lam);
        if (!LOD || (__ballot(wl > 0.f) != 0ull && wl > 0.f)) {
            const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
            uint32_t v[3];
            float w[3];
            point_cell<D>(t, R, S, fdiv, v, w);
            float gv[F];
            grow(l, gv);
            float acc[D];
#pragma unroll
            for (int a = 0; a < D; ++a) acc[a] = 0.f;
            [[maybe_unused]] float accl = 0.f;
#pragma unroll
            for (int c = 0; c < (1 << D); ++c) {
                const uint32_t e = hash_index(dense, R, mask, v[0] + (c & 1), v[1] + ((c >> 1) & 1), D == 3 ? v[2] + ((c >> 2) & 1) : 0u);
                float tv[F];
                if constexpr (SRC == NIC_HASH_SRC_U8) load_row_u8<F>(stab + (int64_t)e * F, s.q_scale, s.q_bias, tv);
                else if constexpr (SRC == NIC_HASH_SRC_BITS) load_row_bits<F, TIGHT>(btab, e, s.q_bits, s.q_scale, s.q_bias, tv);
                else load_row<F>(tab + (int64_t)e * F, tv);
                // every operation spelled out: nothing for the compiler to contract one way in one instantiation and another way in the next
                float dot = 0.f;
#pragma unroll
                for (int f = 0; f < F; ++f) dot = fmaf(gv[f], tv[f], dot);
                float cw[3];
#pragma unroll
                for (int a = 0; a < D; ++a) cw[a] = ((c >> a) & 1) ? w[a] : __fsub_rn(1.0f, w[a]);
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    float sw = ((c >> a) & 1) ? 1.0f : -1.0f;
#pragma unroll
                    for (int b = 0; b < D; ++b)
                        if (b != a) sw = __fmul_rn(sw, cw[b]);
                    acc[a] = fmaf(sw, dot, acc[a]);
                }
                if constexpr (DLOD) {
                    float pw = cw[0];
#pragma unroll
                    for (int a = 1; a < D; ++a) pw = __fmul_rn(pw, cw[a]);
                    accl = fmaf(pw, dot, accl);
                }
            }
            float scale = __fdiv_rn((float)R, (float)S);
            if constexpr (LOD) scale = __fmul_rn(scale, wl);
#pragma unroll
            for (int a = 0; a < D; ++a) g[a] = fmaf(scale, acc[a], g[a]);
            if constexpr (DLOD) {
                if (a_raw <= 1.0f) {                                  // wl > 0 is a_raw > 0: on the ramp
                    if constexpr (NOISE) {
                        // 16 % F == 0: the level's F columns lie in one generator block
                        const int c0 = l * F;
                        if ((c0 >> 4) != nblk_id) {
                            nblk_id = c0 >> 4;
                            nblk = noise_block(s.noise, s.sample_base + (uint64_t)n, nblk_id);
                        }
                        float nd = 0.f;
#pragma unroll
                        for (int f = 0; f < F; ++f) nd = fmaf(gv[f], noise_from_block(s.noise, nblk, (c0 + f) & 15), nd);
                        glam = __fsub_rn(glam, __fadd_rn(accl, nd));
                    } else {
                        glam = __fsub_rn(glam, accl);
                    }
                }
            }
        }
    }
}
// q_tight is uniform over the launch: the width of the packed window is decided once per point (encode_point's rule)
template <int D, int F, int SRC, bool LOD, bool DLOD, bool NOISE, class Src, class GRow>
__device__ __forceinline__ void point_walk(const Src& s, const uint32_t (&t)[3], int64_t n, float lam, GRow grow, float (&g)[D], float& glam) {
    if constexpr (SRC == NIC_HASH_SRC_BITS) {
        if (s.q_tight) point_walk_levels<D, F, SRC, true, LOD, DLOD, NOISE>(s, t, n, lam, grow, g, glam);
        else point_walk_levels<D, F, SRC, false, LOD, DLOD, NOISE>(s, t, n, lam, grow, g, glam);
    } else {
        point_walk_levels<D, F, SRC, false, LOD, DLOD, NOISE>(s, t, n, lam, grow, g, glam);
    }
}
// the position gradient alone: the batch units (hashgrid_batch.hip, hashgrid_batch_grad.hip) and the joint training kernel
template <int D, int F, int SRC, bool LOD, class Src, class GRow>
__device__ __forceinline__ void point_grad(const Src& s, const uint32_t (&t)[3], float lam, GRow grow, float (&g)[D]) {
    float unused;
    point_walk<D, F, SRC, LOD, false, false>(s, t, 0, lam, grow, g, unused);
}
// row n of dpoints: 0 on an axis whose clamp moved the point
template <int D>
__device__ __forceinline__ void store_point_grad(float* dpoints, int64_t n, uint32_t kept, const float (&g)[D]) {
#pragma unroll
    for (int a = 0; a < D; ++a) dpoints[n * D + a] = ((kept >> a) & 1u) ? g[a] : 0.0f;
}


// ---- the decoder's backward to the input alone -----------------------------------------------------------------------------------------------
// decoder_train_half (hash_common.hpp) without its three weight-gradient passes and without TrainAcc, the same products in the same order:
// forward of the 32 samples `32 nt + j` of the row tile `xs` keeping the two GELU derivative tiles, dZ3 = dy y (1 - y), dA2 = W3^T dZ3,
// dZ2 = dA2 gelu', dA1 = W2^T dZ2, dZ1 = dA1 gelu', dX = W1^T dZ1 written over the rows of this half.  `mine`: this lane (half 0) owns a live
// sample; its dy is read at `dyrow`, or formed from `trow` as dscale (y - target); y goes to `yrow` when that is not null.
template <int KT>
__device__ __forceinline__ void decoder_dx_half(const DecoderSmem& sm, float* xs, int nt, int j, int half, int ks1, bool mine, const float* dyrow,
                                                const float* trow, float* yrow, float dscale) {
    const int src = 32 * nt + j;
    const float* xb = xs + src * XS;
    // ---- layer 1
    f32x16 a1[2] = {f32x16{}, f32x16{}};
    f32x16 d1[2];
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
            d1[t][r] = dv;
        }
    // ---- layer 2
    f32x16 a2[2] = {f32x16{}, f32x16{}};
    f32x16 d2[2];
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
            d2[t][r] = dv;
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
    if (mine && yrow != nullptr) {
#pragma unroll
        for (int o = 0; o < 3; ++o) yrow[o] = yv[o];
    }
    // ---- dZ3 = dy y (1 - y); with a target dy = 2 (y - t) loss_scale / (3 N)
    float dz3[3] = {0.f, 0.f, 0.f};
    if (mine) {
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            if (dyrow != nullptr) dz3[o] = dyrow[o] * yv[o] * (1.0f - yv[o]);
            else dz3[o] = dscale * (yv[o] - trow[o]) * yv[o] * (1.0f - yv[o]);
        }
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
    // dX = W1^T dZ1 over the rows of this half (their X is spent: every lane of the wave has issued its layer-1 reads)
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

}  // namespace hcommon
}  // namespace nic
