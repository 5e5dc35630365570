// The combined walk of hashgrid_lodgrad.hpp for a row that carries the codec NOISE of training (hashgrid_lodtrain.hip includes
// this header).  In encode_point_levels column l F + f of the row is a_l (r[l, f] + nz[l F + f]), so on the ramp 0 < a_raw <= 1
//     d column / d lambda = -(r[l, f] + nz[l F + f]),
//     glam = - sum_{l on the ramp} (sum_c prod_a cw_a(c) sum_f grow(l)[f] value[l, idx(v + c), f] + sum_f grow(l)[f] nz[l F + f]).
// nz is the value the forward added: the same key sample_base + n (n the caller's row), the same generator block, the same noise_from_block;
// the block of columns (l F) & ~15 .. is made by the first level ON THE RAMP of this lane that needs it (encode_point_levels' caching rule on
// the levels that read it here) and lives in registers: no memory is added anywhere.  Training reads the fp32 table only, so there is no SRC.
// The same offsets, index, loader and point_cell as point_grad_lod_levels, the same acc[a] / g[a] / accl operations in the same order: `g` is
// that walk's bit for bit, and without noise the walk IS that one (point_grad_lod_noisy calls it).  Everything is force-inlined.
#pragma once
#include "hashgrid_lodgrad.hpp"

namespace nic {
namespace hcommon {

template <int D, int F, class Src, class GRow>
__device__ __forceinline__ void point_grad_lod_noisy_levels(const Src& s, const uint32_t (&t)[3], int64_t n, float lam, GRow grow, float (&g)[D],
                                                            float& glam) {
    const nic_hash_desc& d = s.d;
    const uint32_t S = (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const float fdiv = (float)(256u * S);
    U4 nblk{0u, 0u, 0u, 0u};                           // the generator block `nblk_id` of this lane's sample (-1: none yet)
    int nblk_id = -1;
#pragma unroll
    for (int a = 0; a < D; ++a) g[a] = 0.f;
    glam = 0.f;
    for (int l = 0; l < d.levels; ++l) {
        const uint32_t R = (uint32_t)d.resolution[l];
        const float* tab = s.table + ((int64_t)l << d.log2_table) * F;
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
                load_row<F>(tab + (int64_t)e * F, tv);
                // every operation spelled out, as in point_grad_lod_levels: `g` and accl are that walk's bit for bit
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
            if (a_raw <= 1.0f) {                                  // wl > 0 is a_raw > 0: on the ramp
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
            }
        }
    }
}
// NOISE is uniform over the launch; without it the walk is point_grad_lod's from the fp32 table, operation for operation
template <int D, int F, bool NOISE, class Src, class GRow>
__device__ __forceinline__ void point_grad_lod_noisy(const Src& s, const uint32_t (&t)[3], int64_t n, float lam, GRow grow, float (&g)[D], float& glam) {
    if constexpr (NOISE) point_grad_lod_noisy_levels<D, F>(s, t, n, lam, grow, g, glam);
    else point_grad_lod<D, F, NIC_HASH_SRC_F32>(s, t, lam, grow, g, glam);
}

}  // namespace hcommon
}  // namespace nic
