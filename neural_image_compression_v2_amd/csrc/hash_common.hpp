// What the hash-grid kernels share, the one copy of it: all five translation units (hash_grid.hip, hash_fused.hip, hash_points.hip,
// hash_points_train.hip, hash_mixed.hip) include this header and keep only their kernels, parameter structs and launch tables.
// The index helpers, the fp32, uint8 and packed row loaders, the cell of a lattice sample (2 S_max arithmetic) and the fixed-point position and
// cell of a point or of a lattice sample (include/nicv2_hip.h, nic_hash_encode_points), the level loops of the encode (row into an LDS tile) and
// of the scatter (run sums keyed on the base vertex), the ColorDecoder(L F, 64, 3) forward + backward on v_mfma_f32_32x32x2_f32 with its
// register-resident weight-gradient accumulators and per-workgroup record, and the host side of the entry points: descriptor checks, grid
// rules, dequantisation constants, the noise source of a nic_hash_quant.  Everything on the device side is force-inlined, so a kernel's code
// does not depend on where a helper is declared (profiles/hashgrid_common_disasm.txt).  run_masks / run_sum, the noise generator and the
// activations come from nic_device.hpp, the optimiser tail from nic_adam.hpp.
#pragma once
#include <cmath>
#include <type_traits>

#include "nic_device.hpp"
#include "nic_adam.hpp"

namespace nic {
namespace hcommon {

// ---- index helpers and loaders ---------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool hash_level_dense(int dim, int32_t R, int log2_table) {
    uint64_t p = 1;
    for (int a = 0; a < dim; ++a) {
        p *= (uint64_t)R + 1;
        if (p > (1ull << log2_table)) return false;
    }
    return true;
}
// the entry of vertex (vx, vy, vz) in a level of resolution R (vz = 0 in 2D); masked with T - 1: no input can leave a level
__host__ __device__ inline uint32_t hash_index(bool dense, uint32_t R, uint32_t mask, uint32_t vx, uint32_t vy, uint32_t vz) {
    const uint32_t h = dense ? vx + (R + 1u) * (vy + (R + 1u) * vz) : (vx ^ (vy * 2654435761u) ^ (vz * 805459861u));
    return h & mask;
}
template <int F>
__device__ __forceinline__ void load_row(const float* p, float (&v)[F]) {
    if constexpr (F == 1) {
        v[0] = *p;
    } else if constexpr (F == 2) {
        const float2 a = *reinterpret_cast<const float2*>(p);
        v[0] = a.x; v[1] = a.y;
    } else {
#pragma unroll
        for (int k = 0; k < F; k += 4) {
            const float4 a = *reinterpret_cast<const float4*>(p + k);
            v[k] = a.x; v[k + 1] = a.y; v[k + 2] = a.z; v[k + 3] = a.w;
        }
    }
}
template <int F>
__device__ __forceinline__ void store_row(float* p, const float (&v)[F]) {
    if constexpr (F == 1) {
        *p = v[0];
    } else if constexpr (F == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int k = 0; k < F; k += 4) *reinterpret_cast<float4*>(p + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    }
}
// one compact uint8 entry of F bytes as ONE load (ubyte / ushort / dword / dwordx2), dequantised like load4fp_kernel (simple_kernels.hip)
template <int F>
__device__ __forceinline__ void load_row_u8(const uint8_t* p, float scale, float bias, float (&v)[F]) {
    uint32_t w[(F + 3) / 4];
    if constexpr (F == 1) {
        w[0] = *p;
    } else if constexpr (F == 2) {
        w[0] = *reinterpret_cast<const uint16_t*>(p);
    } else if constexpr (F == 4) {
        w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else {
        const uint2 a = *reinterpret_cast<const uint2*>(p);
        w[0] = a.x; w[1] = a.y;
    }
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const float u = (float)((w[f >> 2] >> (8 * (f & 3))) & 0xFFu);
        v[f] = __fdiv_rn(__fadd_rn(__fsub_rn(u, bias), 1.0f), scale);
    }
}
// entries a level stores: the (R + 1)^dim vertices of a dense level, all T of a hashed one; dwords of its bit stream at `bits` bits per value
__host__ __device__ inline int64_t hash_level_entries(int dim, int32_t R, int log2_table) {
    if (!hash_level_dense(dim, R, log2_table)) return int64_t(1) << log2_table;
    int64_t e = 1;
    for (int a = 0; a < dim; ++a) e *= (int64_t)R + 1;
    return e;
}
__host__ __device__ inline int64_t hash_level_dwords(int dim, int32_t R, int log2_table, int F, int bits) {
    return (hash_level_entries(dim, R, log2_table) * (F * bits) + 31) >> 5;
}
__host__ __device__ inline bool hash_bits_tight(int F, int bits) { return 32 % (F * bits) == 0 || F * bits == 64; }
// one bit-packed entry of F b bits at bit e F b of its level's stream `lev`: aligned dword loads only - the dword the entry starts in and the
// next one (F <= 4: F b <= 32) or two (F = 8: F b <= 64; the 8 zero bytes after the last level keep that window inside the buffer), funnel-
// shifted so that the entry starts at bit 0.  TIGHT (uniform over the launch or the level): no entry straddles, the extra dword is not read.
// The value then takes load_row_u8's dequantisation, expression for expression.
template <int F, bool TIGHT>
__device__ __forceinline__ void load_row_bits(const uint32_t* lev, uint32_t e, int bits, float scale, float bias, float (&v)[F]) {
    const uint32_t bit = e * (uint32_t)(F * bits), sh = bit & 31u;
    const uint32_t* q = lev + (bit >> 5);
    uint32_t x0, x1 = 0u;
    const uint32_t w0 = q[0];
    if constexpr (F <= 4) {
        if constexpr (TIGHT) x0 = w0 >> sh;
        else x0 = __builtin_amdgcn_alignbit(q[1], w0, sh);
    } else {
        if constexpr (TIGHT) {
            x0 = w0 >> sh;
            if (bits == 8) x1 = q[1];                                // F b = 64 starts on a dword
        } else {
            const uint32_t w1 = q[1], w2 = q[2];
            x0 = __builtin_amdgcn_alignbit(w1, w0, sh);
            x1 = __builtin_amdgcn_alignbit(w2, w1, sh);
        }
    }
#pragma unroll
    for (int f = 0; f < F; ++f) {
        uint32_t uv;
        if constexpr (F <= 4) uv = __builtin_amdgcn_ubfe(x0, (uint32_t)(f * bits), (uint32_t)bits);      // f b + b <= 32
        else uv = __builtin_amdgcn_ubfe((uint32_t)((((uint64_t)x1 << 32) | x0) >> (f * bits)), 0u, (uint32_t)bits);
        const float u = (float)uv;
        v[f] = __fdiv_rn(__fadd_rn(__fsub_rn(u, bias), 1.0f), scale);
    }
}
template <int D>
__device__ __forceinline__ float corner_weight(const float (&w)[3], int c) {
    float r = ((c & 1) ? w[0] : 1.0f - w[0]) * ((c & 2) ? w[1] : 1.0f - w[1]);
    if (D == 3) r *= (c & 4) ? w[2] : 1.0f - w[2];
    return r;
}

// ---- the fixed-point split of a point ------------------------------------------------------------------------------------------------------
// the position of point n per axis: clamped in floating point first (NaN fails both comparisons' "keep" side and lands on the low edge,
// -inf / +inf on the nearer one), so the conversion sees |256 p| < 2^30; then t = rint(256 p) + 128 (v_rndne: half to even; 256 p is exact)
// clamped to [0, 256 S - 1] - the upper edge p = S - 1/2 gives 256 S and comes back into the last cell, so v <= R - 1 on every level
template <int D>
__device__ __forceinline__ void point_fixed(const nic_hash_desc& d, const float* points, int64_t n, uint32_t (&t)[3]) {
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const float x = points[n * D + a], lo = -0.5f, hi = (float)d.extent[a] - 0.5f;
        float c = x >= lo ? x : lo;
        c = c <= hi ? c : hi;
        const int ti = (int)rintf(256.0f * c) + 128, tmax = 256 * d.extent[a] - 1;
        t[a] = (uint32_t)(ti < 0 ? 0 : (ti > tmax ? tmax : ti));
    }
    if (D == 2) t[2] = 0;
}
// q = t R (< 2^38), v = q div 256 S_max, w = fp32(q mod 256 S_max) / fp32(256 S_max), through q >> 8 (< 2^30) div / mod S_max in 32 bits
template <int D>
__device__ __forceinline__ void point_cell(const uint32_t (&t)[3], uint32_t R, uint32_t S, float fdiv, uint32_t (&v)[3], float (&w)[3]) {
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const uint64_t q = (uint64_t)t[a] * R;
        const uint32_t qh = (uint32_t)(q >> 8), ql = (uint32_t)q & 255u;
        v[a] = qh / S;
        w[a] = (float)(((qh - v[a] * S) << 8) | ql) / fdiv;
    }
    if (D == 2) { v[2] = 0; w[2] = 0.f; }
}

// ---- the lattice as a position source -------------------------------------------------------------------------------------------------------
// the sample of this lane in patch `wv` of 8 x 8 / 4 x 4 x 4 samples, x the fastest lane axis (clamped to the last patch; `live` = a real
// sample of a real patch); n = its row in nic_encode sample order
template <int D>
struct PatchSample {
    int crop;
    int idx[3];
    bool live;
    int64_t n;
};
template <int D>
__device__ __forceinline__ PatchSample<D> patch_sample(const nic_hash_desc& d, int64_t wv, int64_t n_patches, int lane) {
    constexpr int PS = D == 2 ? 8 : 4;
    const int np1 = (d.extent[1] + PS - 1) / PS, np2 = D == 3 ? (d.extent[2] + PS - 1) / PS : 1;
    const int64_t per_crop = (int64_t)((d.extent[0] + PS - 1) / PS) * np1 * np2;
    const int64_t wc = wv < n_patches ? wv : n_patches - 1;
    PatchSample<D> s;
    s.crop = (int)(wc / per_crop);
    int64_t pr = wc - (int64_t)s.crop * per_crop;
    int pt[3] = {0, 0, 0};
    if (D == 3) { pt[2] = (int)(pr % np2); pr /= np2; }
    pt[1] = (int)(pr % np1);
    pt[0] = (int)(pr / np1);
    if (D == 2) {
        s.idx[0] = PS * pt[0] + (lane & 7);
        s.idx[1] = PS * pt[1] + (lane >> 3);
        s.idx[2] = 0;
    } else {
        s.idx[0] = PS * pt[0] + (lane & 3);
        s.idx[1] = PS * pt[1] + ((lane >> 2) & 3);
        s.idx[2] = PS * pt[2] + (lane >> 4);
    }
    s.live = wv < n_patches;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        s.live = s.live && s.idx[a] < d.extent[a];
        s.idx[a] = s.idx[a] < d.extent[a] ? s.idx[a] : d.extent[a] - 1;
    }
    const int64_t n_per_crop = (int64_t)d.extent[0] * d.extent[1] * (D == 3 ? d.extent[2] : 1);
    s.n = (int64_t)s.crop * n_per_crop + ((int64_t)s.idx[0] * d.extent[1] + s.idx[1]) * (D == 3 ? d.extent[2] : 1) + (D == 3 ? s.idx[2] : 0);
    return s;
}
// integer sample coordinate per axis, clamped into the field (an origin outside it is refused on the host; this keeps q < 2^31 regardless)
template <int D>
__device__ __forceinline__ void sample_coords(const nic_hash_desc& d, const int32_t* origins, const PatchSample<D>& s, uint32_t (&i)[3]) {
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const int c = origins[s.crop * D + a] + s.idx[a];
        i[a] = (uint32_t)(c < 0 ? 0 : (c >= d.S_max ? d.S_max - 1 : c));
    }
    if (D == 2) i[2] = 0;
}
// base vertex and fp32 weight per axis of one level on the crop route: q = (2 i + 1) R, v = q / 2 S_max, w = (q mod 2 S_max) / 2 S_max
template <int D>
__device__ __forceinline__ void level_cell(const uint32_t (&i)[3], uint32_t R, uint32_t S2, uint32_t (&v)[3], float (&w)[3]) {
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const uint32_t q = (2u * i[a] + 1u) * R;
        v[a] = q / S2;
        w[a] = (float)(q - v[a] * S2) / (float)S2;
    }
    if (D == 2) { v[2] = 0; w[2] = 0.f; }
}
// lattice sample i (origin + index, clamped into the field like sample_coords) as the point t = 256 i + 128: both operands of the cell
// quotient are 128 times the crop route's, so v, w and the row are nic_hash_encode's bit for bit (include/nicv2_hip.h)
template <int D>
__device__ __forceinline__ void lattice_fixed(const nic_hash_desc& d, const int32_t* origins, const PatchSample<D>& s, uint32_t (&t)[3]) {
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const int c = origins[s.crop * D + a] + s.idx[a];
        t[a] = 256u * (uint32_t)(c < 0 ? 0 : (c >= d.S_max ? d.S_max - 1 : c)) + 128u;
    }
    if (D == 2) t[2] = 0;
}

// ---- the field at points, with and without a level of detail per point ---------------------------------------------------------------------
// the parameters of the four kernels with a level of detail per point (hash_points.hip, hash_points_train.hip)
struct LodParams {
    nic_hash_desc d;          // extent[a] = S_a, num_crops = 1
    float fade[NIC_HASH_MAX_LEVELS];
    float lod_uniform;
    const float* lod;         // null, or [n]
    const float* points;      // [n, dim]
    int64_t n;
    const int32_t* order;     // null, or [n] row indices (clamped); backward and fused training only
    const float* table;       // NIC_HASH_SRC_F32
    const uint8_t* stored;    // NIC_HASH_SRC_U8
    const uint32_t* packed;   // NIC_HASH_SRC_BITS, 4-byte aligned
    const float* dx;
    float* out;
    float* grad;              // table gradient (fused training: null = frozen table, no scatter)
    NoiseSrc noise;
    uint64_t sample_base;
    float q_scale, q_bias;    // load4fp: (u - q_bias + 1) / q_scale
    int32_t q_bits, q_tight;
    // fused only
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    const float* target;
    float* y;
    float* partials;
    float dscale;             // 2 loss_scale / (3 N)
};
template <class Params>
constexpr bool is_lod = std::is_same<Params, LodParams>::value;

// the row lane `pos` of a launch handles: order[pos] clamped into the n points, or pos itself
__device__ __forceinline__ int64_t ordered_row(const int32_t* order, int64_t n, int64_t pos) {
    if (order == nullptr) return pos;
    const int64_t i = order[pos];
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}
// lambda of point n = (lod ? lod[n] : 0) + lod_uniform, NaN -> 0, clamped to [0, 32]
__device__ __forceinline__ float point_lambda(const float* lod, float lod_uniform, int64_t n) {
    float v = __fadd_rn(lod != nullptr ? lod[n] : 0.f, lod_uniform);
    v = v == v ? v : 0.f;
    v = v >= 0.f ? v : 0.f;
    return v <= 32.f ? v : 32.f;
}
// a_l = min(max((fade[l] - lambda) + 1, 0), 1): one subtract, one add, nothing to contract
__device__ __forceinline__ float level_weight(float fade, float lam) {
    const float a = __fadd_rn(__fsub_rn(fade, lam), 1.0f);
    return a >= 0.f ? (a <= 1.f ? a : 1.f) : 0.f;
}
// lambda of row n of a launch: LodParams', and 0 for every other parameter struct (which has no level of detail)
__device__ __forceinline__ float point_lambda(const LodParams& p, int64_t n) { return point_lambda(p.lod, p.lod_uniform, n); }
template <class Params>
__device__ __forceinline__ float point_lambda(const Params&, int64_t) {
    return 0.f;
}
__device__ __forceinline__ const float* level_fade(const LodParams& p) { return p.fade; }
template <class Params>
__device__ __forceinline__ const float* level_fade(const Params&) {
    return nullptr;
}

// each XCD (blocks b, b + 8, ..) walks one contiguous range of groups of 4 wave items
struct WaveRange {
    int64_t begin, end;
    int step;
};
__device__ __forceinline__ WaveRange xcd_range(int64_t n_waves) {
    const int xcd = blockIdx.x & 7;
    const int64_t n_groups = (n_waves + 3) >> 2, chunk = (n_groups + 7) >> 3;
    const int64_t g_begin = xcd * chunk;
    return WaveRange{g_begin + (blockIdx.x >> 3), g_begin + chunk < n_groups ? g_begin + chunk : n_groups, (int)(gridDim.x >> 3)};
}

// THE level loop of a table of one bit depth at one point (hash_encode_kernel's, on the fixed-point position t).  `s` is whatever holds the
// source - a kernel's parameter struct: d, the table of SRC (table / stored + q_scale, q_bias / packed + q_bits too), with NOISE noise and
// sample_base, with LOD fade - and each field is read where the loop uses it: filled into a struct of its own at the call site, the kernarg
// loads move and every kernel compiles to other code.  SRC picks the loader; NOISE: the noise of nic_hash_encode_noisy keyed
// by sample_base + n and the column; VEC: the row goes out in F-wide stores (global), else value by value (an LDS tile).
// LOD: level l is weighed by a_l = level_weight(fade[l], lam), column l F + f is fl(a_l r).  A level no lane of the wave weighs
// above 0 is jumped over by the whole wave (the ballot is wave-uniform: no cell arithmetic, no gather, no noise - its stored offsets still
// advance); inside a live level a lane of weight 0 reads nothing and writes zeros; the generator block of columns (l F) & ~15 .. is made by
// the first LIVE level of this lane that needs it, so a skipped level at a block boundary leaves the later levels of the block their noise.
// `dense` and the zero fill stand where the loop without and the loop with a level of detail each had them: the order is the schedule's.
template <int D, int F, int SRC, bool NOISE, bool TIGHT, bool VEC, bool LOD, class Src>
__device__ __forceinline__ void encode_point_levels(const Src& s, const uint32_t (&t)[3], int64_t n, float lam, float* row) {
    const nic_hash_desc& d = s.d;
    const uint32_t S = (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const float fdiv = (float)(256u * S);
    [[maybe_unused]] int64_t lev_off = 0;              // _U8: byte offset of level l = F * sum_{k<l} E_k
    [[maybe_unused]] int64_t lev_dw = 0;               // _BITS: dword offset of level l = sum_{k<l} ceil(E_k F b / 32)
    [[maybe_unused]] U4 nblk{0u, 0u, 0u, 0u};          // NOISE: the generator block of columns (l F) & ~15 ..; LOD: block `nblk_id` (-1: none yet)
    [[maybe_unused]] int nblk_id = -1;
#pragma unroll 2
    for (int l = 0; l < d.levels; ++l) {
        const uint32_t R = (uint32_t)d.resolution[l];
        [[maybe_unused]] bool dense = false;
        if constexpr (!LOD) dense = hash_level_dense(D, (int32_t)R, d.log2_table);
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
        [[maybe_unused]] float a = 1.0f;
        if constexpr (LOD) a = level_weight(s.fade[l], lam);
        float acc[F];
        if constexpr (LOD) {
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] = 0.f;
        }
        if (!LOD || (__ballot(a > 0.f) != 0ull && a > 0.f)) {
            if constexpr (LOD) dense = hash_level_dense(D, (int32_t)R, d.log2_table);      // only a live level asks
            uint32_t v[3];
            float w[3];
            point_cell<D>(t, R, S, fdiv, v, w);
            if constexpr (!LOD) {
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] = 0.f;
            }
#pragma unroll
            for (int c = 0; c < (1 << D); ++c) {
                const uint32_t e = hash_index(dense, R, mask, v[0] + (c & 1), v[1] + ((c >> 1) & 1), D == 3 ? v[2] + ((c >> 2) & 1) : 0u);
                float tv[F];
                if constexpr (SRC == NIC_HASH_SRC_U8) load_row_u8<F>(stab + (int64_t)e * F, s.q_scale, s.q_bias, tv);
                else if constexpr (SRC == NIC_HASH_SRC_BITS) load_row_bits<F, TIGHT>(btab, e, s.q_bits, s.q_scale, s.q_bias, tv);
                else load_row<F>(tab + (int64_t)e * F, tv);
                const float cw = corner_weight<D>(w, c);
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] += cw * tv[f];
            }
            if constexpr (NOISE) {
                // 16 % F == 0: a level's F columns lie in one generator block, made once (at its first column; LOD: by the block's first live level)
                const int c0 = l * F;
                if constexpr (LOD) {
                    if ((c0 >> 4) != nblk_id) {
                        nblk_id = c0 >> 4;
                        nblk = noise_block(s.noise, s.sample_base + (uint64_t)n, nblk_id);
                    }
                } else {
                    if ((c0 & 15) == 0) nblk = noise_block(s.noise, s.sample_base + (uint64_t)n, c0 >> 4);
                }
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] += noise_from_block(s.noise, nblk, (c0 + f) & 15);
            }
            if constexpr (LOD) {
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] = __fmul_rn(a, acc[f]);
            }
        }
        if constexpr (VEC) {
            store_row<F>(row + l * F, acc);
        } else {
#pragma unroll
            for (int f = 0; f < F; ++f) row[l * F + f] = acc[f];
        }
    }
}
// b is uniform over the launch: the width of the packed window is decided once per row, not per corner
template <int D, int F, int SRC, bool NOISE, bool VEC, bool LOD, class Src>
__device__ __forceinline__ void encode_point(const Src& s, const uint32_t (&t)[3], int64_t n, float lam, float* row) {
    if constexpr (SRC == NIC_HASH_SRC_BITS) {
        if (s.q_tight) encode_point_levels<D, F, SRC, NOISE, true, VEC, LOD>(s, t, n, lam, row);
        else encode_point_levels<D, F, SRC, NOISE, false, VEC, LOD>(s, t, n, lam, row);
    } else {
        encode_point_levels<D, F, SRC, NOISE, false, VEC, LOD>(s, t, n, lam, row);
    }
}

// the level loop of the backward for one lane's point: `grow(l, g)` hands over the F gradient values of level l (a dead lane gets zeros without
// the call).  Runs are keyed on the base VERTEX; each lane weighs its own gradient before the sum and only NEIGHBOURING lanes merge, so any point
// order is right - and cell order makes the runs long.  The whole wave must call this together (shuffles).  LOD: the gradient of level l is
// weighed by a_l here; the run sums shuffle across the whole wave, so a level is skipped only when the ballot finds no lane for it, a lane of
// weight 0 takes part in its run with zeros, and a run whose lanes all weigh 0 issues no atomic.
template <int D, int F, bool LOD, class GRow>
__device__ __forceinline__ void scatter_point(const nic_hash_desc& d, const uint32_t (&t)[3], float* grad, const float* fade, float lam, bool live,
                                              int lane, GRow grow) {
    const uint32_t S = (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const float fdiv = (float)(256u * S);
    for (int l = 0; l < d.levels; ++l) {
        [[maybe_unused]] float a = 1.0f;
        if constexpr (LOD) {
            a = live ? level_weight(fade[l], lam) : 0.f;
            if (__ballot(a > 0.f) == 0ull) continue;
        }
        const uint32_t R = (uint32_t)d.resolution[l];
        const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
        float* gtab = grad + ((int64_t)l << d.log2_table) * F;
        uint32_t v[3];
        float w[3];
        point_cell<D>(t, R, S, fdiv, v, w);
        float g[F];
#pragma unroll
        for (int f = 0; f < F; ++f) g[f] = 0.f;
        if constexpr (LOD) {
            if (a > 0.f) {
                grow(l, g);
#pragma unroll
                for (int f = 0; f < F; ++f) g[f] = __fmul_rn(a, g[f]);
            }
        } else {
            if (live) grow(l, g);
        }
        const int64_t key = (int64_t)v[0] + ((int64_t)R + 1) * ((int64_t)v[1] + ((int64_t)R + 1) * (int64_t)v[2]);
        const RunMasks m = run_masks(live ? key : -1 - (int64_t)lane, lane);
        [[maybe_unused]] float weighed = 1.f;           // LOD: lanes of this run with something to add
        if constexpr (LOD) {
            weighed = a > 0.f ? 1.f : 0.f;
            if (m.any_shared) weighed = run_sum(weighed, m);
        }
        const bool issue = live && m.head && (!LOD || weighed > 0.f);
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

// ---- the decoder on the fp32 matrix pipe ---------------------------------------------------------------------------------------------------
constexpr int XS = kH + 1;      // row stride of every LDS tile: lanes that walk rows hit 64 different banks
constexpr int NQ = 16;          // samples per weight-gradient pass (the two transposed tiles of a wave)

// the record of a workgroup, nn.Linear layouts back to back: dW1 [64, L F] | db1 | dW2 [64, 64] | db2 | dW3 [3, 64] | db3 | sum of squared errors
// (hash_fused_reduce_kernel reads records of this layout)
struct RecLayout {
    int w1, b1, w2, b2, w3, b3, loss, rec;
    __host__ __device__ explicit RecLayout(int lf) {
        w1 = 0; b1 = kH * lf; w2 = b1 + kH; b2 = w2 + kH * kH; w3 = b2 + kH; b3 = w3 + 3 * kH; loss = b3 + 3; rec = loss + 1;
    }
};

struct DecoderSmem {             // what a forward-only launch needs: the leading part of TrainSmem, member for member
    float w1[kH * XS], w2[kH * XS], w3[4 * kH], b1[kH], b2[kH], b3[4];
    float x[4][kH * XS];        // per wave: the encoding rows [sample][column], later d loss / d row; at the end of the launch the workgroup's record
};
struct TrainSmem : DecoderSmem {
    float p[4][NQ * XS], q[4][NQ * XS];
};

// LDS traffic between the lanes of ONE wave: its LDS instructions execute in order, the compiler must not move them across
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ int row_of(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// acc[ta][tb] += sum over the NQ samples of a pass of P[n][32 ta + i] Q[n][32 tb + j]   (MASK4: P has 4 columns, one row tile)
// side[ta] += every P operand of this lane: the bias gradient (column sums of dZ) of unit 32 ta + i over the samples of this half's parity
template <int TA, int TB, bool MASK4>
__device__ __forceinline__ void wgrad_mfma(const float* P, const float* Q, int j, int half, f32x16 (&acc)[TA][TB], float (&side)[TA]) {
#pragma unroll
    for (int s = 0; s < NQ / 2; ++s) {
        float a[TA], b[TB];
#pragma unroll
        for (int ta = 0; ta < TA; ++ta) a[ta] = MASK4 ? (j < 4 ? P[(2 * s + half) * XS + j] : 0.f) : P[(2 * s + half) * XS + 32 * ta + j];
#pragma unroll
        for (int tb = 0; tb < TB; ++tb) b[tb] = Q[(2 * s + half) * XS + 32 * tb + j];
#pragma unroll
        for (int ta = 0; ta < TA; ++ta) {
            side[ta] += a[ta];
#pragma unroll
            for (int tb = 0; tb < TB; ++tb) acc[ta][tb] = mfma(a[ta], b[tb], acc[ta][tb]);
        }
    }
}
// the [unit] values of this lane's sample -> row (j & 15) of a transposed tile
template <int T>
__device__ __forceinline__ void put_tile(float* P, int j, int half, const f32x16 (&u)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) P[(j & 15) * XS + 32 * t + row_of(r, half)] = u[t][r];
}
__device__ __forceinline__ float half_sum(float v) {      // over the 32 lanes of this lane's half, fixed order
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// the weight-gradient accumulators of one wave: in registers for the whole launch
template <int KT>
struct TrainAcc {
    f32x16 gW1[2][KT], gW2[2][2], gW3[1][2];
    float gb1[2], gb2[2], gb3[1], sse;
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int b = 0; b < KT; ++b) gW1[a][b] = f32x16{};
            gW2[a][0] = f32x16{}; gW2[a][1] = f32x16{};
            gW3[0][a] = f32x16{};
            gb1[a] = 0.f; gb2[a] = 0.f;
        }
        gb3[0] = 0.f; sse = 0.f;
    }
};

// the decoder's weights into LDS (columns past L F are zero) and the wave's row tile cleared; the caller synchronises the workgroup after it
__device__ __forceinline__ void load_decoder(DecoderSmem& sm, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                                             const float* b3, int LF, int tid) {
    for (int e = tid; e < kH * XS; e += 256) {
        const int h = e / XS, k = e - h * XS;
        sm.w1[e] = k < LF ? w1[h * LF + k] : 0.f;
        sm.w2[e] = k < kH ? w2[h * kH + k] : 0.f;
    }
    sm.w3[tid] = tid < 3 * kH ? w3[tid] : 0.f;
    if (tid < kH) { sm.b1[tid] = b1[tid]; sm.b2[tid] = b2[tid]; }
    if (tid < 4) sm.b3[tid] = tid < 3 ? b3[tid] : 0.f;
    float* xs = sm.x[tid >> 6];
    for (int e = tid & 63; e < kH * XS; e += 64) xs[e] = 0.f;       // the columns past L F stay finite (their weights are zero)
}

// the forward half of decoder_train_half alone (hash_fused_kernel's forward mode, the same products in the same order): y of sample
// 32 nt + j of the row tile `xs` in registers 0 .. 2 of half 0
__device__ __forceinline__ void decoder_forward_half(const DecoderSmem& sm, const float* xs, int nt, int j, int half, int ks1, float (&yv)[3]) {
    const float* xb = xs + (32 * nt + j) * XS;
    f32x16 a1[2] = {f32x16{}, f32x16{}};
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
        }
    f32x16 a2[2] = {f32x16{}, f32x16{}};
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
        }
    f32x16 z3 = f32x16{};
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = 32 * t + row_of(r, half);
            z3 = mfma(j < 3 ? sm.w3[j * kH + k] : 0.f, a2[t][r], z3);
        }
#pragma unroll
    for (int o = 0; o < 3; ++o) yv[o] = sigmoid_f(z3[o] + sm.b3[o]);
}

// forward, loss and backward of the 32 samples `32 nt + j` of a wave's row tile `xs` (hash_fused_kernel's training mode, the same products in
// the same order).  `mine`: this lane (half 0) owns a live sample; it reads its target at `trow`, writes y to `yrow` when that is not null.
// The weight gradients go into `A`; with `want_dx`, d loss / d row replaces the rows of this half in `xs`.
// WEIGHT (hashgrid_weighted.hip): the owner's sample counts `w` times in the loss - `dscale` arrives as dscale w, the loss partial
// is (w e) e, the expression of the plain partial with one exact factor at w = 1.  Without WEIGHT `w` is not read.
template <int KT, bool WEIGHT = false>
__device__ __forceinline__ void decoder_train_half(TrainSmem& sm, float* xs, float* P, float* Q, int nt, int j, int half, int ks1, bool mine,
                                                   const float* trow, float* yrow, float dscale, bool want_dx, TrainAcc<KT>& A,
                                                   [[maybe_unused]] float w = 1.0f) {
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
    // ---- dZ3 = dy y (1 - y), dy = 2 (y - t) loss_scale / (3 N)
    float dz3[4] = {0.f, 0.f, 0.f, 0.f};
    if (mine) {
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            const float e = yv[o] - trow[o];
            if constexpr (WEIGHT) {
                const float we = __fmul_rn(w, e);
                A.sse += we * e;
            } else {
                A.sse += e * e;
            }
            dz3[o] = dscale * e * yv[o] * (1.0f - yv[o]);
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
        wgrad_mfma<1, 2, true>(P, Q, j, half, A.gW3, A.gb3);
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
        wgrad_mfma<2, 2, false>(P, Q, j, half, A.gW2, A.gb2);
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
        wgrad_mfma<2, KT, false>(P, xs + (32 * nt + 16 * q) * XS, j, half, A.gW1, A.gb1);
        wave_sync();
    }
    // dX = W1^T dZ1 over the rows of this half (their X is spent)
    if (want_dx) {
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

// the workgroup's record: the four waves add their accumulators in wave order into the (now free) row tiles, then the record goes to `rec`
template <int KT>
__device__ __forceinline__ void write_record(TrainSmem& sm, const TrainAcc<KT>& A, int LF, float* rec, int tid) {
    const int wave = tid >> 6, lane = tid & 63, j = lane & 31, half = lane >> 5;
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
                        if (32 * tb + j < LF) put(rl.w1 + h * LF + 32 * tb + j, A.gW1[ta][tb][r]);
#pragma unroll
                    for (int tb = 0; tb < 2; ++tb) put(rl.w2 + h * kH + 32 * tb + j, A.gW2[ta][tb][r]);
                }
#pragma unroll
            for (int ta = 0; ta < 2; ++ta) {                 // lane (i, half) summed the samples of parity `half`
                const float s1 = A.gb1[ta] + __shfl_xor(A.gb1[ta], 32), s2 = A.gb2[ta] + __shfl_xor(A.gb2[ta], 32);
                if (half == 0) { put(rl.b1 + 32 * ta + j, s1); put(rl.b2 + 32 * ta + j, s2); }
            }
            const float s3 = A.gb3[0] + __shfl_xor(A.gb3[0], 32);
            if (lane < 3) put(rl.b3 + lane, s3);
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                if (half == 0) { put(rl.w3 + o * kH + j, A.gW3[0][0][o]); put(rl.w3 + o * kH + 32 + j, A.gW3[0][1][o]); }
            }
            const float sl = half_sum(A.sse);
            if (lane == 0) put(rl.loss, sl);
        }
        __syncthreads();
    }
    for (int e = tid; e < rl.rec; e += 256) rec[e] = R[e];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// what every entry point asks of a descriptor, in this order (tests/test_host_cpu.py and the *_cpu hash-grid tests pin it)
inline int check_hash_desc(const nic_hash_desc* d) {
    if (!d) return NIC_E_NULL;
    if (d->dim != 2 && d->dim != 3) return NIC_E_UNSUPPORTED;
    if (d->features != 1 && d->features != 2 && d->features != 4 && d->features != 8) return NIC_E_UNSUPPORTED;
    if (d->levels < 1 || d->levels > NIC_HASH_MAX_LEVELS) return NIC_E_ARG;
    if (d->log2_table < 10 || d->log2_table > 24) return NIC_E_ARG;
    if (d->S_max < 1 || d->flags != 0) return NIC_E_ARG;
    for (int l = 0; l < d->levels; ++l)      // q = (2 i + 1) R_l < 2 S_max R_l must stay below 2^31
        if (d->resolution[l] < 1 || 2 * (int64_t)d->S_max * d->resolution[l] >= (int64_t(1) << 31)) return NIC_E_ARG;
    if (d->num_crops < 1) return NIC_E_SHAPE;
    for (int a = 0; a < d->dim; ++a)
        if (d->extent[a] < 1 || d->extent[a] > d->S_max) return NIC_E_SHAPE;
    return NIC_OK;
}
// then what the point entry points add: one field, 256 S_max < 2^30 (point_cell divides q >> 8 in 32 bits)
inline int check_point_desc(const nic_hash_desc* d) {
    const int rc = check_hash_desc(d);
    if (rc) return rc;
    if (d->num_crops != 1) return NIC_E_SHAPE;
    if (256 * (int64_t)d->S_max >= (int64_t(1) << 30)) return NIC_E_ARG;
    return NIC_OK;
}

inline int device_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
        else n = 256;
    }
    return n;
}
// workgroups a persistent launch may use: one per CU, a multiple of 8 (one slice of the range per XCD)
inline int wg_cap() {
    const int c = device_cus() / 8 * 8;
    return c < 8 ? 8 : c;
}
// patches of 8 x 8 / 4 x 4 x 4 samples in the crops of a lattice launch: one wave each
inline int64_t count_patches(const nic_hash_desc* d) {
    const int PS = d->dim == 2 ? 8 : 4;
    int64_t patches = d->num_crops;
    for (int a = 0; a < d->dim; ++a) patches *= (d->extent[a] + PS - 1) / PS;
    return patches;
}
// workgroups of a persistent launch over `n_waves` wave items (patches, or groups of 64 points), four to a workgroup: a multiple of 8, capped
inline int persistent_grid(int64_t n_waves) {
    const int64_t groups = (n_waves + 3) / 4, want = (groups + 7) / 8 * 8;
    return (int)(want < wg_cap() ? want : wg_cap());
}
// workgroups of a grid-strided launch over the same wave items, four to a workgroup: at least one, capped
inline int strided_grid(int64_t n_waves) {
    const int64_t b = (n_waves + 3) / 4;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// load4fp's constants into a parameter struct: (u - q_bias + 1) / q_scale, q_scale = 2^b - 1, q_bias = 2^(b-1)
template <class Params>
inline void set_dequant(Params& p, int num_bits) {
    p.q_scale = (float)((1 << num_bits) - 1);
    p.q_bias = (float)(1 << (num_bits - 1));
}
// the noise source of a launch from a nic_hash_quant, with its argument checks; null, or noise_mode NIC_NOISE_NONE, leaves `noise` as it is.
// uniform_depth: the scale is 2^-num_bits; without it num_bits is ignored and the scale is the kernel's to set (a depth per level)
inline int set_noise(const nic_hash_quant* quant, bool uniform_depth, NoiseSrc& noise, uint64_t& sample_base) {
    if (!quant) return NIC_OK;
    if ((uniform_depth && (quant->num_bits < 1 || quant->num_bits > 8)) || quant->sample_base < 0) return NIC_E_ARG;
    if (quant->noise_mode == NIC_NOISE_TENSOR) return NIC_E_UNSUPPORTED;
    if (quant->noise_mode != NIC_NOISE_NONE && quant->noise_mode != NIC_NOISE_KERNEL) return NIC_E_ARG;
    if (quant->noise_mode == NIC_NOISE_KERNEL) {
        noise.mode = NIC_NOISE_KERNEL;
        noise.k0 = (uint32_t)quant->noise_seed; noise.k1 = (uint32_t)(quant->noise_seed >> 32);
        noise.off_lo = (uint32_t)quant->noise_offset; noise.off_hi = (uint32_t)(quant->noise_offset >> 32);
        if (uniform_depth) noise.scale = ldexpf(1.0f, -quant->num_bits);
        sample_base = (uint64_t)quant->sample_base;
    }
    return NIC_OK;
}

// the table source of a point launch into its parameters (PointParams, LodParams); the caller has refused a null source.  NIC_E_ARG in the
// order of the _u8 / _bits siblings (bit depth, alignment)
template <class Params>
inline int set_point_source(Params& p, const nic_hash_source* src) {
    if (src->kind == NIC_HASH_SRC_F32) {
        if (src->num_bits != 0) return NIC_E_ARG;
        p.table = (const float*)src->data;
        return NIC_OK;
    }
    if (src->kind != NIC_HASH_SRC_U8 && src->kind != NIC_HASH_SRC_BITS) return NIC_E_ARG;
    if (src->num_bits < 1 || src->num_bits > 8) return NIC_E_ARG;
    set_dequant(p, src->num_bits);
    if (src->kind == NIC_HASH_SRC_U8) {
        p.stored = (const uint8_t*)src->data;
        return NIC_OK;
    }
    if ((uintptr_t)src->data & 3u) return NIC_E_ARG;                 // the gather reads aligned dwords
    p.packed = (const uint32_t*)src->data;
    p.q_bits = src->num_bits;
    p.q_tight = hash_bits_tight(p.d.features, src->num_bits) ? 1 : 0;
    return NIC_OK;
}
// a nic_hash_lod: its checks, and the struct with the per-point array into the parameters
inline int check_lod(const nic_hash_desc* d, const nic_hash_lod* lp) {
    for (int l = 0; l < d->levels; ++l)
        if (!std::isfinite(lp->fade[l]) || lp->fade[l] < 0.f) return NIC_E_ARG;
    if (!std::isfinite(lp->lod_uniform) || lp->reserved != 0) return NIC_E_ARG;
    return NIC_OK;
}
template <class Params>      // LodParams, and the batch unit's parameter structs with the same three fields
inline void set_lod(Params& p, const nic_hash_lod* lp, const float* lod) {
    for (int l = 0; l < NIC_HASH_MAX_LEVELS; ++l) p.fade[l] = l < p.d.levels ? lp->fade[l] : 0.f;
    p.lod_uniform = lp->lod_uniform;
    p.lod = lod;
}

// dim x features of a checked descriptor as compile-time constants: fn(std::integral_constant<int, D>, std::integral_constant<int, F>), then the
// error of the launch fn made; `kind` of a checked nic_hash_source likewise
template <class Fn>
inline int dispatch_dim_features(const nic_hash_desc& d, Fn fn) {
    auto features = [&](auto dim) {
        switch (d.features) {
            case 1: fn(dim, std::integral_constant<int, 1>{}); break;
            case 2: fn(dim, std::integral_constant<int, 2>{}); break;
            case 4: fn(dim, std::integral_constant<int, 4>{}); break;
            default: fn(dim, std::integral_constant<int, 8>{}); break;
        }
    };
    if (d.dim == 2) features(std::integral_constant<int, 2>{});
    else features(std::integral_constant<int, 3>{});
    return (int)hipGetLastError();
}
template <class Fn>
inline int dispatch_source(int kind, Fn fn) {
    if (kind == NIC_HASH_SRC_U8) return fn(std::integral_constant<int, NIC_HASH_SRC_U8>{});
    if (kind == NIC_HASH_SRC_BITS) return fn(std::integral_constant<int, NIC_HASH_SRC_BITS>{});
    return fn(std::integral_constant<int, NIC_HASH_SRC_F32>{});
}

struct KernelEndDrop {        // a training entry point consumes the parked nic_mark_kernel_end event on every return
    ~KernelEndDrop() { kernel_end_drop(); }
};

}  // namespace hcommon

namespace hfused {
// defined in hash_fused.hip; reads records of hcommon::RecLayout.  The fused training entry points of every translation unit launch it.
__global__ void __launch_bounds__(256) hash_fused_reduce_kernel(const float* partials, int n_rec, int lf, nic_mlp_grads g, float* loss, float loss_mul,
                                                                int add_grads, int add_loss, const StepTail tl);
}  // namespace hfused

namespace hcommon {
// ---- the end of a fused training step, the same at every entry point ------------------------------------------------------------------------
// The optimiser tail that rides on the record reduction (fused_capi.hip, TailScope::open): a decoder entry's gradient must be one of the buffers
// this call's reduction writes.  Split in two because the entry points return NIC_E_WORKSPACE before the tail's codes and NIC_OK for no points
// after them.
struct FusedTail {
    StepTail tl;
    int64_t tail_blocks;
    int reduce_blocks;
};
inline int check_fused_tail(const nic_step_tail* tail, const nic_mlp_grads* mlp_grads, int lf, FusedTail& ft) {
    ft.reduce_blocks = (RecLayout(lf).rec + 31) / 32;
    ft.tl.t.count = 0; ft.tl.t.sched = nullptr; ft.tl.n_stream = 0; ft.tl.reduce_blocks = 0x7fffffff;
    ft.tail_blocks = 0;
    if (!tail) return NIC_OK;
    if (!tail->tensors) return NIC_E_NULL;
    if (tail->count < 1 || tail->count > NIC_ADAM_MAX_TENSORS || tail->n_stream < 0 || tail->n_stream > tail->count) return NIC_E_ARG;
    if (tail->sched != nullptr) return NIC_E_ARG;                     // the device schedule belongs to the captured dense step
    for (int i = tail->n_stream; i < tail->count; ++i) {
        bool found = false;
        for (int k = 0; k < 3; ++k)
            found = found || (tail->tensors[i].grad != nullptr && (tail->tensors[i].grad == mlp_grads->w[k] || tail->tensors[i].grad == mlp_grads->b[k]));
        if (!found) return NIC_E_ARG;
    }
    const int rc = adam_build_table(tail->tensors, tail->count, tail->n_stream, tail->beta1, tail->beta2, tail->eps, nullptr, 0, nullptr, ft.tl.t,
                                    ft.tl.n_stream, ft.tail_blocks);
    if (rc) return rc;
    ft.tl.reduce_blocks = ft.reduce_blocks;
    return NIC_OK;
}
// `launch()` starts the training kernel, which leaves `grid` records in `partials`; then the end mark and the reduction with the tail
template <class Launch>
inline int finish_fused_step(const FusedTail& ft, const nic_mlp_grads* mlp_grads, int flags, int lf, int grid, float loss_mul, float* loss,
                             const float* partials, void* stream, Launch launch) {
    const int rc = launch();
    if (rc) return rc;
    kernel_end_mark((hipStream_t)stream);
    hipLaunchKernelGGL(hfused::hash_fused_reduce_kernel, dim3((unsigned)(ft.reduce_blocks + ft.tail_blocks)), dim3(256), 0, (hipStream_t)stream, partials,
                       grid, lf, *mlp_grads, loss, loss_mul, (flags & NIC_HASH_FUSED_ADD_GRADS) ? 1 : 0, (flags & NIC_HASH_FUSED_ADD_LOSS) ? 1 : 0,
                       ft.tl);
    return (int)hipGetLastError();
}

// ---- the fused training step at points, the same at its four entry points (hash_points_train.hip, hashgrid_points_joint.hip,
// hashgrid_lodtrain.hip) -----------------------------------------------------------------------------------------------------------------------
// the workspace of the step: one record per workgroup of the widest persistent launch
inline size_t points_workspace_bytes(int lf) { return (size_t)wg_cap() * RecLayout(lf).rec * sizeof(float); }
// The opening of an entry: the descriptor and the decoder.  Each entry follows it with its own null list, then `flags` and check_lod in the
// order include/nicv2_hip.h states for it: _points has no level of detail; _points_lod asks check_lod, then flags; _points_grad flags, then
// check_lod where lodp is given; _points_grad_lod flags, then check_lod.
inline int open_fused_points(const nic_hash_desc* desc, const nic_mlp* mlp) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((rc = check_point_desc(desc)) != NIC_OK) return rc;
    for (int i = 0; i < 3; ++i)
        if (!mlp->w[i] || !mlp->b[i]) return NIC_E_NULL;
    return NIC_OK;
}
// what every parameter struct of the step holds, from the arguments every entry has
template <class Params>
inline void fill_fused_points(Params& p, const nic_hash_desc* desc, const float* points, int64_t n_points, const int32_t* order, const float* table,
                              const float* target, float* table_grad, float* y, const nic_mlp* mlp) {
    p.d = *desc; p.points = points; p.n = n_points; p.order = order; p.table = table; p.target = target; p.grad = table_grad; p.y = y;
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
}
// From the first check that needs the parameters on: the quantiser, the point count, the workspace, the tail, then the step.  `p` arrives with
// everything but noise, dscale and partials set; `launch(noise, grid)` starts the entry's training kernel, `noise` a std::bool_constant
template <class Params, class Launch>
inline int points_fused_step(Params& p, const nic_hash_quant* quant, const int32_t* order, float loss_scale, const nic_mlp_grads* mlp_grads, float* loss,
                             int flags, void* workspace, size_t workspace_bytes, const nic_step_tail* tail, void* stream, Launch launch) {
    p.noise.mode = NIC_NOISE_NONE;
    int rc = set_noise(quant, true, p.noise, p.sample_base);
    if (rc) return rc;
    if (p.n < 0 || (order && p.n >= (int64_t(1) << 31))) return NIC_E_ARG;
    const int lf = p.d.levels * p.d.features;
    if (workspace_bytes < points_workspace_bytes(lf)) return NIC_E_WORKSPACE;
    FusedTail ft;
    if ((rc = check_fused_tail(tail, mlp_grads, lf, ft)) != NIC_OK) return rc;
    if (p.n == 0) return NIC_OK;                                      // nothing to launch: *loss and every gradient output stay as they are
    const int grid = persistent_grid((p.n + 63) >> 6);
    const float loss_mul = (float)((double)loss_scale / (3.0 * (double)p.n));
    p.dscale = 2.0f * loss_mul;
    p.partials = (float*)workspace;
    return finish_fused_step(ft, mlp_grads, flags, lf, grid, loss_mul, loss, p.partials, stream, [&] {
        return p.noise.mode == NIC_NOISE_KERNEL ? launch(std::true_type{}, grid) : launch(std::false_type{}, grid);
    });
}
}  // namespace hcommon
}  // namespace nic
