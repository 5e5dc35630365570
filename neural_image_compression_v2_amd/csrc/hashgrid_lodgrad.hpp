// The position-gradient walk of hashgrid_pointgrad.hpp with one more output: the gradient with respect to the LEVEL OF DETAIL lambda
// (hashgrid_lodgrad.hip includes this header).  The weight of level l is a_l = clamp((fade[l] - lambda) + 1, 0, 1), column
// l F + f of the row is a_l r[l, f], so d column / d lambda = -r[l, f] on the ramp 0 < a_raw <= 1 (the right-hand derivative) and 0 elsewhere:
//     glam = - sum_{l on the ramp} sum_c prod_a cw_a(c) sum_f grow(l)[f] value[l, idx(v + c), f].
// The walk already gathers every corner of every live level and already forms the per-corner dot: one more accumulator, no extra gather.
// Same offsets, index, loaders and point_cell as point_grad_levels<.., LOD = true>, the same acc[a] / g[a] operations in the same order:
// `g` is that walk's bit for bit.  Everything is force-inlined.
#pragma once
#include "hashgrid_pointgrad.hpp"

namespace nic {
namespace hcommon {

// lambda_raw = (lod ? lod[n] : 0) + lod_uniform of point_lambda before its clamps: the clamp passes the gradient on [0, 32) (the right-hand
// derivative of the clamp; a NaN fails both comparisons)
__device__ __forceinline__ bool lambda_passes(const float* lod, float lod_uniform, int64_t n) {
    const float v = __fadd_rn(lod != nullptr ? lod[n] : 0.f, lod_uniform);
    return v >= 0.f && v < 32.f;
}

template <int D, int F, int SRC, bool TIGHT, class Src, class GRow>
__device__ __forceinline__ void point_grad_lod_levels(const Src& s, const uint32_t (&t)[3], float lam, GRow grow, float (&g)[D], float& glam) {
    const nic_hash_desc& d = s.d;
    const uint32_t S = (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const float fdiv = (float)(256u * S);
    [[maybe_unused]] int64_t lev_off = 0;              // _U8: byte offset of level l
    [[maybe_unused]] int64_t lev_dw = 0;               // _BITS: dword offset of level l
#pragma unroll
    for (int a = 0; a < D; ++a) g[a] = 0.f;
    glam = 0.f;
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
        const float a_raw = __fadd_rn(__fsub_rn(s.fade[l], lam), 1.0f);
        const float wl = level_weight(s.fade[l], lam);
        if (__ballot(wl > 0.f) != 0ull && wl > 0.f) {
            const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
            uint32_t v[3];
            float w[3];
            point_cell<D>(t, R, S, fdiv, v, w);
            float gv[F];
            grow(l, gv);
            float acc[D];
#pragma unroll
            for (int a = 0; a < D; ++a) acc[a] = 0.f;
            float accl = 0.f;
#pragma unroll
            for (int c = 0; c < (1 << D); ++c) {
                const uint32_t e = hash_index(dense, R, mask, v[0] + (c & 1), v[1] + ((c >> 1) & 1), D == 3 ? v[2] + ((c >> 2) & 1) : 0u);
                float tv[F];
                if constexpr (SRC == NIC_HASH_SRC_U8) load_row_u8<F>(stab + (int64_t)e * F, s.q_scale, s.q_bias, tv);
                else if constexpr (SRC == NIC_HASH_SRC_BITS) load_row_bits<F, TIGHT>(btab, e, s.q_bits, s.q_scale, s.q_bias, tv);
                else load_row<F>(tab + (int64_t)e * F, tv);
                // every operation spelled out, as in point_grad_levels: `g` is that walk's bit for bit
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
                float pw = cw[0];
#pragma unroll
                for (int a = 1; a < D; ++a) pw = __fmul_rn(pw, cw[a]);
                accl = fmaf(pw, dot, accl);
            }
            const float scale = __fmul_rn(__fdiv_rn((float)R, (float)S), wl);
#pragma unroll
            for (int a = 0; a < D; ++a) g[a] = fmaf(scale, acc[a], g[a]);
            if (a_raw <= 1.0f) glam = __fsub_rn(glam, accl);      // wl > 0 is a_raw > 0: on the ramp
        }
    }
}
// b is uniform over the launch: the width of the packed window is decided once per point (encode_point's rule)
template <int D, int F, int SRC, class Src, class GRow>
__device__ __forceinline__ void point_grad_lod(const Src& s, const uint32_t (&t)[3], float lam, GRow grow, float (&g)[D], float& glam) {
    if constexpr (SRC == NIC_HASH_SRC_BITS) {
        if (s.q_tight) point_grad_lod_levels<D, F, SRC, true>(s, t, lam, grow, g, glam);
        else point_grad_lod_levels<D, F, SRC, false>(s, t, lam, grow, g, glam);
    } else {
        point_grad_lod_levels<D, F, SRC, false>(s, t, lam, grow, g, glam);
    }
}

}  // namespace hcommon
}  // namespace nic
