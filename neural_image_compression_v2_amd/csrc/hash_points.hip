// The hash-grid field at ARBITRARY points (include/nicv2_hip.h: nic_hash_encode_points / _backward / nic_hash_fused_forward_points; hashgrid.py,
// HashGridField.query / resample / train_points).  A point is `dim` fp32 coordinates in sample units (p = i: the centre of integer
// sample i); it becomes fixed point with 8 fractional bits, t = rint(256 p) + 128 clamped to [0, 256 S - 1], and from there on the cell arithmetic
// is the exact-integer arithmetic of hash_grid.hip with 256 S_max in the place of 2 S_max: q = t R, v = q div 256 S_max, w = fp32(q mod 256 S_max)
// / fp32(256 S_max).  At a sample centre both operands of that quotient are 128 times the lattice route's, so v, w and the row are its, bit for bit.
//
// q < 2^38, but q div / mod 256 S_max needs no 64-bit division: q >> 8 < 2^30 is divided by S_max in 32 bits and the low 8 bits of q re-enter the
// remainder, ((q >> 8) mod S_max) 256 + (q & 255) < 256 S_max < 2^30.
//
// One lane per point, row n = point n, in any order: the run sums of the backward merge whichever NEIGHBOURING lanes share a base vertex (whole
// runs in raster order, none for random points, the whole wave when all points coincide).  The fused decode is hash_fused.hip's forward mode
// with the lane's coordinates taken from the point array; that file and hash_grid.hip are pinned, so their helpers are restated here unchanged.
#include "nic_device.hpp"

namespace nic {
namespace hpoints {

// ---- restated from hash_grid.hip / hash_fused.hip -------------------------------------------------------------------------------------
__host__ __device__ inline bool hash_level_dense(int dim, int32_t R, int log2_table) {
    uint64_t p = 1;
    for (int a = 0; a < dim; ++a) {
        p *= (uint64_t)R + 1;
        if (p > (1ull << log2_table)) return false;
    }
    return true;
}
__host__ __device__ inline uint32_t hash_index(bool dense, uint32_t R, uint32_t mask, uint32_t vx, uint32_t vy, uint32_t vz) {
    const uint32_t h = dense ? vx + (R + 1u) * (vy + (R + 1u) * vz) : (vx ^ (vy * 2654435761u) ^ (vz * 805459861u));
    return h & mask;
}
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
// ---- end of the restated helpers ------------------------------------------------------------------------------------------------------

enum PointSrc { PSRC_F32 = NIC_HASH_SRC_F32, PSRC_U8 = NIC_HASH_SRC_U8, PSRC_BITS = NIC_HASH_SRC_BITS };

struct PointParams {
    nic_hash_desc d;          // extent[a] = S_a, num_crops = 1
    const float* points;      // [n, dim]
    int64_t n;
    const float* table;       // PSRC_F32
    const uint8_t* stored;    // PSRC_U8
    const uint32_t* packed;   // PSRC_BITS, 4-byte aligned
    const float* dx;
    float* out;
    float* grad;
    NoiseSrc noise;
    uint64_t sample_base;
    float q_scale, q_bias;    // load4fp: (u - q_bias + 1) / q_scale
    int32_t q_bits, q_tight;
    // fused decode only
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    float* y;
};

// the fixed-point position of point n per axis: clamped in floating point first (NaN fails both comparisons' "keep" side and lands on the low
// edge, -inf / +inf on the nearer one), so the conversion sees |256 p| < 2^30; then t = rint(256 p) + 128 (v_rndne: half to even; 256 p is exact)
// clamped to [0, 256 S - 1] - the upper edge p = S - 1/2 gives 256 S and comes back into the last cell, so v <= R - 1 on every level
template <int D>
__device__ __forceinline__ void point_fixed(const PointParams& p, int64_t n, uint32_t (&t)[3]) {
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const float x = p.points[n * D + a], lo = -0.5f, hi = (float)p.d.extent[a] - 0.5f;
        float c = x >= lo ? x : lo;
        c = c <= hi ? c : hi;
        const int ti = (int)rintf(256.0f * c) + 128, tmax = 256 * p.d.extent[a] - 1;
        t[a] = (uint32_t)(ti < 0 ? 0 : (ti > tmax ? tmax : ti));
    }
    if (D == 2) t[2] = 0;
}

// base vertex and fp32 weight per axis of one level: q = t R (< 2^38), v = q div 256 S_max, w = fp32(q mod 256 S_max) / fp32(256 S_max),
// through q >> 8 (< 2^30) div / mod S_max in 32 bits (file comment)
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

// the level loop of hash_encode_kernel for one point; VEC: the row goes out in F-wide stores (global), else value by value (an LDS tile)
template <int D, int F, int SRC, bool NOISE, bool TIGHT, bool VEC>
__device__ __forceinline__ void encode_levels(const PointParams& p, const uint32_t (&t)[3], int64_t n, float* row) {
    const nic_hash_desc& d = p.d;
    const uint32_t S = (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const float fdiv = (float)(256u * S);
    [[maybe_unused]] int64_t lev_off = 0;              // PSRC_U8: byte offset of level l = F * sum_{k<l} E_k
    [[maybe_unused]] int64_t lev_dw = 0;               // PSRC_BITS: dword offset of level l = sum_{k<l} ceil(E_k F b / 32)
    [[maybe_unused]] U4 nblk{0u, 0u, 0u, 0u};          // NOISE: the generator block of columns (l F) & ~15 ..
#pragma unroll 2
    for (int l = 0; l < d.levels; ++l) {
        const uint32_t R = (uint32_t)d.resolution[l];
        const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
        [[maybe_unused]] const float* tab = nullptr;
        if constexpr (SRC == PSRC_F32) tab = p.table + ((int64_t)l << d.log2_table) * F;
        [[maybe_unused]] const uint8_t* stab = nullptr;
        if constexpr (SRC == PSRC_U8) {
            stab = p.stored + lev_off;
            lev_off += (int64_t)F * hash_level_entries(D, (int32_t)R, d.log2_table);
        }
        [[maybe_unused]] const uint32_t* btab = nullptr;
        if constexpr (SRC == PSRC_BITS) {
            btab = p.packed + lev_dw;
            lev_dw += hash_level_dwords(D, (int32_t)R, d.log2_table, F, p.q_bits);
        }
        uint32_t v[3];
        float w[3];
        point_cell<D>(t, R, S, fdiv, v, w);
        float acc[F];
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = 0.f;
#pragma unroll
        for (int c = 0; c < (1 << D); ++c) {
            const uint32_t e = hash_index(dense, R, mask, v[0] + (c & 1), v[1] + ((c >> 1) & 1), D == 3 ? v[2] + ((c >> 2) & 1) : 0u);
            float tv[F];
            if constexpr (SRC == PSRC_U8) load_row_u8<F>(stab + (int64_t)e * F, p.q_scale, p.q_bias, tv);
            else if constexpr (SRC == PSRC_BITS) load_row_bits<F, TIGHT>(btab, e, p.q_bits, p.q_scale, p.q_bias, tv);
            else load_row<F>(tab + (int64_t)e * F, tv);
            const float cw = corner_weight<D>(w, c);
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] += cw * tv[f];
        }
        if constexpr (NOISE) {
            // 16 % F == 0: a level's F columns lie in one block; it is generated once, at its first column, and reused by the next levels
            const int c0 = l * F;
            if ((c0 & 15) == 0) nblk = noise_block(p.noise, p.sample_base + (uint64_t)n, c0 >> 4);
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] += noise_from_block(p.noise, nblk, (c0 + f) & 15);
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
template <int D, int F, int SRC, bool NOISE, bool VEC>
__device__ __forceinline__ void encode_point(const PointParams& p, const uint32_t (&t)[3], int64_t n, float* row) {
    if constexpr (SRC == PSRC_BITS) {
        if (p.q_tight) encode_levels<D, F, SRC, NOISE, true, VEC>(p, t, n, row);
        else encode_levels<D, F, SRC, NOISE, false, VEC>(p, t, n, row);
    } else {
        encode_levels<D, F, SRC, NOISE, false, VEC>(p, t, n, row);
    }
}

template <int D, int F, int SRC, bool NOISE>
__global__ void __launch_bounds__(256) hash_points_encode_kernel(const PointParams p) {
    const int LF = p.d.levels * F;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < p.n; n += (int64_t)gridDim.x * 256) {
        uint32_t t[3];
        point_fixed<D>(p, n, t);
        encode_point<D, F, SRC, NOISE, true>(p, t, n, p.out + n * LF);
    }
}

template <int D, int F>
__global__ void __launch_bounds__(256) hash_points_backward_kernel(const PointParams p) {
    const nic_hash_desc& d = p.d;
    const int lane = threadIdx.x & 63;
    const uint32_t S = (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const float fdiv = (float)(256u * S);
    const int LF = d.levels * F;
    for (int64_t nb = (int64_t)blockIdx.x * 256; nb < p.n; nb += (int64_t)gridDim.x * 256) {      // block-uniform trip count: the shuffles see whole waves
        const int64_t n_raw = nb + threadIdx.x;
        const bool live = n_raw < p.n;
        const int64_t n = live ? n_raw : p.n - 1;                                                   // a dead lane reads the last point, adds nothing
        uint32_t t[3];
        point_fixed<D>(p, n, t);
        const float* drow = p.dx + n * LF;
        for (int l = 0; l < d.levels; ++l) {
            const uint32_t R = (uint32_t)d.resolution[l];
            const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
            float* gtab = p.grad + ((int64_t)l << d.log2_table) * F;
            uint32_t v[3];
            float w[3];
            point_cell<D>(t, R, S, fdiv, v, w);
            float g[F];
            if (live) load_row<F>(drow + l * F, g);
            else {
#pragma unroll
                for (int f = 0; f < F; ++f) g[f] = 0.f;
            }
            // runs keyed on the base VERTEX, as in hash_encode_backward_kernel; the lanes of a run may sit anywhere in their cell (each weighs its
            // own gradient before the sum), and only NEIGHBOURING lanes merge, so any point order is right and raster order keeps its long runs
            const int64_t key = (int64_t)v[0] + ((int64_t)R + 1) * ((int64_t)v[1] + ((int64_t)R + 1) * (int64_t)v[2]);
            const RunMasks m = run_masks(live ? key : -1 - (int64_t)lane, lane);
            const bool issue = live && m.head;
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
}

// ---- the fused decode at points: hash_fused_kernel's forward mode (hash_fused.hip), one wave per 64 consecutive points -------------------
constexpr int XS = kH + 1;      // row stride of every LDS tile: lanes that walk rows hit 64 different banks

struct Smem {
    float w1[kH * XS], w2[kH * XS], w3[4 * kH], b1[kH], b2[kH], b3[4];
    float x[4][kH * XS];        // per wave: the encoding rows [point][column]
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ int row_of(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

template <int D, int F, int SRC>
__global__ void __launch_bounds__(256) hash_points_fused_kernel(const PointParams p) {
    __shared__ Smem sm;
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

    // each XCD (blocks b, b + 8, ..) walks one contiguous range of groups of 4 waves of points
    const int64_t n_waves = (p.n + 63) >> 6;
    const int xcd = blockIdx.x & 7, nb8 = gridDim.x >> 3;
    const int64_t n_groups = (n_waves + 3) >> 2, chunk = (n_groups + 7) >> 3;
    const int64_t g_begin = xcd * chunk, g_end = g_begin + chunk < n_groups ? g_begin + chunk : n_groups;
    const int ks1 = (LF + 1) >> 1;
    for (int64_t g = g_begin + (blockIdx.x >> 3); g < g_end; g += nb8) {
        const int64_t wv = 4 * g + wave;
        if (wv >= n_waves) continue;                            // wave-uniform; nothing below synchronises the workgroup
        const int64_t n0 = wv << 6, n_raw = n0 + lane;
        uint32_t t[3];
        point_fixed<D>(p, n_raw < p.n ? n_raw : p.n - 1, t);    // a lane past the end decodes the last point; its output is not stored
        encode_point<D, F, SRC, false, false>(p, t, n_raw, xrow);
        wave_sync();
#pragma unroll 1
        for (int nt = 0; nt < 2; ++nt) {
            const int src = 32 * nt + j;
            const int64_t n = n0 + src;
            const float* xb = xs + src * XS;
            // ---- layer 1
            f32x16 a1[2] = {f32x16{}, f32x16{}};
            for (int k = 0; k < ks1; ++k) {
                const float b = xb[2 * k + half];
                a1[0] = mfma(sm.w1[j * XS + 2 * k + half], b, a1[0]);
                a1[1] = mfma(sm.w1[(32 + j) * XS + 2 * k + half], b, a1[1]);
            }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float av, dv;
                    gelu_and_grad(a1[tt][r] + sm.b1[32 * tt + row_of(r, half)], av, dv);
                    a1[tt][r] = av;
                }
            // ---- layer 2
            f32x16 a2[2] = {f32x16{}, f32x16{}};
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = 32 * tt + row_of(r, half);
                    a2[0] = mfma(sm.w2[j * XS + k], a1[tt][r], a2[0]);
                    a2[1] = mfma(sm.w2[(32 + j) * XS + k], a1[tt][r], a2[1]);
                }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float av, dv;
                    gelu_and_grad(a2[tt][r] + sm.b2[32 * tt + row_of(r, half)], av, dv);
                    a2[tt][r] = av;
                }
            // ---- output layer: rows 0 .. 2 of one tile (registers 0 .. 2 of half 0)
            f32x16 z3 = f32x16{};
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = 32 * tt + row_of(r, half);
                    z3 = mfma(j < 3 ? sm.w3[j * kH + k] : 0.f, a2[tt][r], z3);
                }
            if (half == 0 && n < p.n) {
#pragma unroll
                for (int o = 0; o < 3; ++o) p.y[n * 3 + o] = sigmoid_f(z3[o] + sm.b3[o]);
            }
        }
        wave_sync();
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
static int device_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
        else n = 256;
    }
    return n;
}
// workgroups of a fused launch: one per CU, a multiple of 8 (one slice of the point range per XCD)
static int fused_grid(int64_t n_points) {
    const int cap = device_cus() / 8 * 8 < 8 ? 8 : device_cus() / 8 * 8;
    const int64_t groups = (n_points + 255) / 256, want = (groups + 7) / 8 * 8;
    return (int)(want < cap ? want : cap);
}
static int point_blocks(int64_t n_points) {
    const int64_t b = (n_points + 255) / 256;
    return (int)(b > 2048 ? 2048 : b);                     // the cap of the crop route (hash_blocks)
}

// check_hash_desc of hash_grid.hip, then what the point entry points add: one field, 256 S_max < 2^30
static int check_point_desc(const nic_hash_desc* d) {
    if (!d) return NIC_E_NULL;
    if (d->dim != 2 && d->dim != 3) return NIC_E_UNSUPPORTED;
    if (d->features != 1 && d->features != 2 && d->features != 4 && d->features != 8) return NIC_E_UNSUPPORTED;
    if (d->levels < 1 || d->levels > NIC_HASH_MAX_LEVELS) return NIC_E_ARG;
    if (d->log2_table < 10 || d->log2_table > 24) return NIC_E_ARG;
    if (d->S_max < 1 || d->flags != 0) return NIC_E_ARG;
    for (int l = 0; l < d->levels; ++l)
        if (d->resolution[l] < 1 || 2 * (int64_t)d->S_max * d->resolution[l] >= (int64_t(1) << 31)) return NIC_E_ARG;
    if (d->num_crops < 1) return NIC_E_SHAPE;
    for (int a = 0; a < d->dim; ++a)
        if (d->extent[a] < 1 || d->extent[a] > d->S_max) return NIC_E_SHAPE;
    if (d->num_crops != 1) return NIC_E_SHAPE;
    if (256 * (int64_t)d->S_max >= (int64_t(1) << 30)) return NIC_E_ARG;
    return NIC_OK;
}

// the table source into the parameters; NIC_E_NULL / NIC_E_ARG in the order of the _u8 / _bits siblings (null, bit depth, alignment)
static int check_source(const nic_hash_source* src) {
    if (!src || !src->data) return NIC_E_NULL;
    return NIC_OK;
}
static int set_source(PointParams& p, const nic_hash_source* src) {
    if (src->kind == NIC_HASH_SRC_F32) {
        if (src->num_bits != 0) return NIC_E_ARG;
        p.table = (const float*)src->data;
        return NIC_OK;
    }
    if (src->kind != NIC_HASH_SRC_U8 && src->kind != NIC_HASH_SRC_BITS) return NIC_E_ARG;
    if (src->num_bits < 1 || src->num_bits > 8) return NIC_E_ARG;
    p.q_scale = (float)((1 << src->num_bits) - 1);
    p.q_bias = (float)(1 << (src->num_bits - 1));
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

enum PointKernel { PK_FWD, PK_FWD_NOISY, PK_BWD, PK_FUSED };

template <int K, int SRC, int D, int F>
static void launch_k(const PointParams& p, int nb, hipStream_t s) {
    if constexpr (K == PK_BWD) hipLaunchKernelGGL((hash_points_backward_kernel<D, F>), dim3(nb), dim3(256), 0, s, p);
    else if constexpr (K == PK_FUSED) hipLaunchKernelGGL((hash_points_fused_kernel<D, F, SRC>), dim3(nb), dim3(256), 0, s, p);
    else if constexpr (K == PK_FWD_NOISY) hipLaunchKernelGGL((hash_points_encode_kernel<D, F, PSRC_F32, true>), dim3(nb), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((hash_points_encode_kernel<D, F, SRC, false>), dim3(nb), dim3(256), 0, s, p);
}
template <int K, int SRC, int D>
static void launch_f(const PointParams& p, int nb, hipStream_t s) {
    switch (p.d.features) {
        case 1: launch_k<K, SRC, D, 1>(p, nb, s); break;
        case 2: launch_k<K, SRC, D, 2>(p, nb, s); break;
        case 4: launch_k<K, SRC, D, 4>(p, nb, s); break;
        default: launch_k<K, SRC, D, 8>(p, nb, s); break;
    }
}
template <int K, int SRC>
static int launch_d(const PointParams& p, int nb, void* stream) {
    if (p.d.dim == 2) launch_f<K, SRC, 2>(p, nb, (hipStream_t)stream);
    else launch_f<K, SRC, 3>(p, nb, (hipStream_t)stream);
    return (int)hipGetLastError();
}
template <int K>
static int launch_src(const PointParams& p, int kind, int nb, void* stream) {
    if (kind == NIC_HASH_SRC_U8) return launch_d<K, PSRC_U8>(p, nb, stream);
    if (kind == NIC_HASH_SRC_BITS) return launch_d<K, PSRC_BITS>(p, nb, stream);
    return launch_d<K, PSRC_F32>(p, nb, stream);
}

}  // namespace hpoints
}  // namespace nic

using namespace nic;
using namespace nic::hpoints;

extern "C" {

int nic_hash_encode_points(const nic_hash_desc* desc, const nic_hash_source* src, const nic_hash_quant* quant, const float* points, int64_t n_points,
                           float* out, void* stream) {
    int rc = check_point_desc(desc);
    if (rc) return rc;
    if ((rc = check_source(src)) != NIC_OK) return rc;
    if (!points || !out) return NIC_E_NULL;
    PointParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.out = out;
    if ((rc = set_source(p, src)) != NIC_OK) return rc;
    bool noisy = false;
    if (quant) {
        if (src->kind != NIC_HASH_SRC_F32) return NIC_E_ARG;            // noise belongs to training, which reads the fp32 table
        if (quant->num_bits < 1 || quant->num_bits > 8 || quant->sample_base < 0) return NIC_E_ARG;
        if (quant->noise_mode == NIC_NOISE_TENSOR) return NIC_E_UNSUPPORTED;
        if (quant->noise_mode != NIC_NOISE_NONE && quant->noise_mode != NIC_NOISE_KERNEL) return NIC_E_ARG;
        if (quant->noise_mode == NIC_NOISE_KERNEL) {
            noisy = true;
            p.noise.mode = NIC_NOISE_KERNEL;
            p.noise.k0 = (uint32_t)quant->noise_seed; p.noise.k1 = (uint32_t)(quant->noise_seed >> 32);
            p.noise.off_lo = (uint32_t)quant->noise_offset; p.noise.off_hi = (uint32_t)(quant->noise_offset >> 32);
            p.noise.scale = ldexpf(1.0f, -quant->num_bits);
            p.sample_base = (uint64_t)quant->sample_base;
        }
    }
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    if (noisy) return launch_d<PK_FWD_NOISY, PSRC_F32>(p, point_blocks(n_points), stream);
    return launch_src<PK_FWD>(p, src->kind, point_blocks(n_points), stream);
}

int nic_hash_encode_points_backward(const nic_hash_desc* desc, const float* points, int64_t n_points, const float* dx, float* table_grad, void* stream) {
    const int rc = check_point_desc(desc);
    if (rc) return rc;
    if (!points || !dx || !table_grad) return NIC_E_NULL;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    PointParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.dx = dx; p.grad = table_grad;
    return launch_d<PK_BWD, PSRC_F32>(p, point_blocks(n_points), stream);
}

int nic_hash_fused_forward_points(const nic_hash_desc* desc, const nic_hash_source* src, const float* points, int64_t n_points, const nic_mlp* mlp,
                                  float* y, void* stream) {
    if (!desc || !mlp) return NIC_E_NULL;
    int rc = nic_hash_fused_supported(desc, kH, mlp->n_linear);          // the only copy of the fused set (hash_fused.hip)
    if (rc) return rc;
    if ((rc = check_point_desc(desc)) != NIC_OK) return rc;
    if ((rc = check_source(src)) != NIC_OK) return rc;
    if (!points || !y) return NIC_E_NULL;
    for (int i = 0; i < 3; ++i)
        if (!mlp->w[i] || !mlp->b[i]) return NIC_E_NULL;
    PointParams p{};
    p.d = *desc; p.points = points; p.n = n_points; p.y = y;
    if ((rc = set_source(p, src)) != NIC_OK) return rc;
    if (n_points < 0) return NIC_E_ARG;
    if (n_points == 0) return NIC_OK;
    p.w1 = mlp->w[0]; p.b1 = mlp->b[0]; p.w2 = mlp->w[1]; p.b2 = mlp->b[1]; p.w3 = mlp->w[2]; p.b3 = mlp->b[2];
    return launch_src<PK_FUSED>(p, src->kind, fused_grid(n_points), stream);
}

}  // extern "C"
