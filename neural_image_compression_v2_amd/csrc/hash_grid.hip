// Multi-resolution hash-grid encoding (include/nicv2_hip.h: nic_hash_encode / nic_hash_encode_backward; hashgrid.py).  No reference
// counterpart: the semantics are this project's own and are spelled out in the header.  One wave per patch of 8 x 8 (2D) / 4 x 4 x 4 (3D)
// samples - the patches of encode_backward_kernel - with x the fastest lane axis: at the finest levels the lanes of a row then read and add into
// neighbouring entries (hashed: v_x enters the hash with factor 1, so 8 consecutive vertices are a permutation of 8 consecutive entries), at the
// coarse levels whole rows or the whole wave share a vertex.  Every table address is masked with T - 1: no input can leave a level.
//
// -DNIC_HASH_NO_RUNSUM: every live lane issues its own atomics (the A/B of the run sums, ab/bench_hashgrid.py).
//
// The codec (nic_hash_encode_noisy / _u8 / nic_hash_pack_u8): the same forward kernel with a table source (fp32 [L, T, F] or the compact uint8
// table, dequantised per corner with load4fp's arithmetic) and optional in-kernel noise on every column, one generator block per 16 columns.
//
// The bit-packed table (nic_hash_encode_bits / nic_hash_pack_bits / nic_hash_unpack_bits; the format is spelled out in the header): a third
// table source, b bits per value in one little-endian bit stream per level.  An entry is read as a window of aligned dwords from the dword it
// starts in, funnel-shifted to bit 0 and masked into the uint8 value, which then takes load_row_u8's dequantisation and the same blend.
#include "hash_common.hpp"

namespace nic {
using namespace hcommon;

struct HashParams {
    nic_hash_desc d;
    const float* table;
    const int32_t* origins;
    const float* dx;
    float* out;
    float* grad;
    // codec launches only (appended: the plain kernels read the fields above at the offsets they always had)
    const uint8_t* stored;   // compact uint8 table (HSRC_U8)
    NoiseSrc noise;          // in-kernel noise (NOISE)
    uint64_t sample_base;
    float q_scale, q_bias;   // load4fp: (u - q_bias + 1) / q_scale, q_scale = 2^b - 1, q_bias = 2^(b-1)
    // bit-packed launches only (appended likewise)
    const uint32_t* packed;  // bit-packed table (HSRC_BITS), 4-byte aligned
    int32_t q_bits;          // b
    int32_t q_tight;         // F b divides 32, or is 64: no entry leaves the dword(s) it starts in, so the window shrinks to them
};

enum HashSrc { HSRC_F32 = 0, HSRC_U8 = 1, HSRC_BITS = 2 };

template <int D, int F, int SRC = HSRC_F32, bool NOISE = false>
__global__ void __launch_bounds__(256) hash_encode_kernel(HashParams p) {
    const nic_hash_desc& d = p.d;
    const int lane = threadIdx.x & 63;
    constexpr int PS = D == 2 ? 8 : 4;
    int64_t n_patches = d.num_crops;
#pragma unroll
    for (int a = 0; a < D; ++a) n_patches *= (d.extent[a] + PS - 1) / PS;
    const uint32_t S2 = 2u * (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const int LF = d.levels * F;
    for (int64_t wb = (int64_t)blockIdx.x * 4; wb < n_patches; wb += (int64_t)gridDim.x * 4) {
        const PatchSample<D> s = patch_sample<D>(d, wb + (threadIdx.x >> 6), n_patches, lane);
        if (!s.live) continue;
        uint32_t i[3];
        sample_coords<D>(d, p.origins, s, i);
        float* orow = p.out + s.n * LF;
        [[maybe_unused]] int64_t lev_off = 0;              // HSRC_U8: byte offset of level l = F * sum_{k<l} E_k
        [[maybe_unused]] int64_t lev_dw = 0;               // HSRC_BITS: dword offset of level l = sum_{k<l} ceil(E_k F b / 32)
        [[maybe_unused]] U4 nblk{0u, 0u, 0u, 0u};          // NOISE: the generator block of columns (l F) & ~15 ..
        for (int l = 0; l < d.levels; ++l) {
            const uint32_t R = (uint32_t)d.resolution[l];
            const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
            const float* tab = p.table + ((int64_t)l << d.log2_table) * F;
            [[maybe_unused]] const uint8_t* stab = nullptr;
            if constexpr (SRC == HSRC_U8) {
                stab = p.stored + lev_off;
                lev_off += (int64_t)F * hash_level_entries(D, (int32_t)R, d.log2_table);
            }
            [[maybe_unused]] const uint32_t* btab = nullptr;
            if constexpr (SRC == HSRC_BITS) {
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
                if constexpr (SRC == HSRC_U8) load_row_u8<F>(stab + (int64_t)e * F, p.q_scale, p.q_bias, t);
                else if constexpr (SRC == HSRC_BITS) {
                    if (p.q_tight) load_row_bits<F, true>(btab, e, p.q_bits, p.q_scale, p.q_bias, t);
                    else load_row_bits<F, false>(btab, e, p.q_bits, p.q_scale, p.q_bias, t);
                }
                else load_row<F>(tab + (int64_t)e * F, t);
                const float cw = corner_weight<D>(w, c);
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] += cw * t[f];
            }
            if constexpr (NOISE) {
                // 16 % F == 0: a level's F columns lie in one block; it is generated once, at its first column, and reused by the next levels
                const int c0 = l * F;
                if ((c0 & 15) == 0) nblk = noise_block(p.noise, p.sample_base + (uint64_t)s.n, c0 >> 4);
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] += noise_from_block(p.noise, nblk, (c0 + f) & 15);
            }
            store_row<F>(orow + l * F, acc);
        }
    }
}

template <int D, int F>
__global__ void __launch_bounds__(256) hash_encode_backward_kernel(HashParams p) {
    const nic_hash_desc& d = p.d;
    const int lane = threadIdx.x & 63;
    constexpr int PS = D == 2 ? 8 : 4;
    int64_t n_patches = d.num_crops;
#pragma unroll
    for (int a = 0; a < D; ++a) n_patches *= (d.extent[a] + PS - 1) / PS;
    const uint32_t S2 = 2u * (uint32_t)d.S_max, mask = (1u << d.log2_table) - 1u;
    const int LF = d.levels * F;
    for (int64_t wb = (int64_t)blockIdx.x * 4; wb < n_patches; wb += (int64_t)gridDim.x * 4) {      // block-uniform trip count: the shuffles see whole waves
        const PatchSample<D> s = patch_sample<D>(d, wb + (threadIdx.x >> 6), n_patches, lane);
        uint32_t i[3];
        sample_coords<D>(d, p.origins, s, i);
        const float* drow = p.dx + s.n * LF;
        for (int l = 0; l < d.levels; ++l) {
            const uint32_t R = (uint32_t)d.resolution[l];
            const bool dense = hash_level_dense(D, (int32_t)R, d.log2_table);
            float* gtab = p.grad + ((int64_t)l << d.log2_table) * F;
            uint32_t v[3];
            float w[3];
            level_cell<D>(i, R, S2, v, w);
            float g[F];
            if (s.live) load_row<F>(drow + l * F, g);
            else {
#pragma unroll
                for (int f = 0; f < F; ++f) g[f] = 0.f;
            }
#ifndef NIC_HASH_NO_RUNSUM
            // runs keyed on the base VERTEX (unique per cell, unlike its hashed entry: two cells whose base entries collide still differ in
            // their other corners); dead lanes get negative keys of their own
            const int64_t key = (int64_t)v[0] + ((int64_t)R + 1) * ((int64_t)v[1] + ((int64_t)R + 1) * (int64_t)v[2]);
            const RunMasks m = run_masks(s.live ? key : -1 - (int64_t)lane, lane);
            const bool issue = s.live && m.head;
#else
            const bool issue = s.live;
#endif
#pragma unroll
            for (int c = 0; c < (1 << D); ++c) {
                const uint32_t e = hash_index(dense, R, mask, v[0] + (c & 1), v[1] + ((c >> 1) & 1), D == 3 ? v[2] + ((c >> 2) & 1) : 0u);
                const float cw = corner_weight<D>(w, c);
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    float val = cw * g[f];
#ifndef NIC_HASH_NO_RUNSUM
                    if (m.any_shared) val = run_sum(val, m);
#endif
                    if (issue) atomicAdd(gtab + (int64_t)e * F + f, val);
                }
            }
        }
    }
}

// fp32 [L, T, F] -> compact uint8 (save4fp_kernel's arithmetic); one byte per thread, level found from the byte prefix pre[] (static
// indices: the prefix stays in scalar registers)
struct HashPackParams {
    const float* src;
    uint8_t* dst;
    int64_t pre[NIC_HASH_MAX_LEVELS + 1];   // byte offset of level l in dst; pre[levels] = total
    int levels, log2_table, features;
    float scale, bias;
};
__global__ void __launch_bounds__(256) hash_pack_u8_kernel(HashPackParams p) {
    const int64_t n = p.pre[p.levels];
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        int l = 0;
        int64_t base = 0;
#pragma unroll
        for (int j = 1; j < NIC_HASH_MAX_LEVELS; ++j) {
            const bool past = j < p.levels && k >= p.pre[j];
            l = past ? j : l;
            base = past ? p.pre[j] : base;
        }
        const int64_t src = ((int64_t)l << p.log2_table) * p.features + (k - base);
        const float v = __fadd_rn(floorf(__fadd_rn(__fmul_rn(p.src[src], p.scale), 0.5f)), p.bias);
        p.dst[k] = (uint8_t)(int)v;                               // torch float -> uint8 cast truncates
    }
}

// fp32 [L, T, F] -> bit-packed: one output dword per thread, assembled in registers from the values whose bits fall into it (hash_pack_u8_kernel's
// arithmetic per value, & (2^b - 1)); the level comes from the dword prefix pre[].  The padding bits and the two tail dwords come out zero.
struct HashBitsParams {
    const float* src;
    uint32_t* packed;                            // pack: destination
    const uint32_t* packed_in;                   // unpack: source
    uint8_t* dst_u8;                             // unpack: the compact uint8 table
    int64_t pre[NIC_HASH_MAX_LEVELS + 1];        // dword offset of level l in the packed table; pre[levels] = the first tail dword
    int64_t pre_u8[NIC_HASH_MAX_LEVELS + 1];     // byte offset of level l in the compact uint8 table (= F * sum E_k: values before level l)
    int levels, log2_table, features, bits;
    float scale, bias;
};
__global__ void __launch_bounds__(256) hash_pack_bits_kernel(HashBitsParams p) {
    const int64_t n = p.pre[p.levels] + 2;
    const uint32_t vmask = (1u << p.bits) - 1u;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        int l = 0;
        int64_t base = 0, vals = p.pre_u8[1];
#pragma unroll
        for (int j = 1; j < NIC_HASH_MAX_LEVELS; ++j) {
            const bool past = j < p.levels && k >= p.pre[j];
            l = past ? j : l;
            base = past ? p.pre[j] : base;
            vals = past ? p.pre_u8[j + 1] - p.pre_u8[j] : vals;
        }
        uint32_t w = 0u;
        if (k < p.pre[p.levels]) {
            const int64_t bit0 = (k - base) << 5;                       // first stream bit of this dword
            const float* src = p.src + ((int64_t)l << p.log2_table) * p.features;
            for (int64_t i = bit0 / p.bits; i < vals && i * p.bits < bit0 + 32; ++i) {
                const float v = __fadd_rn(floorf(__fadd_rn(__fmul_rn(src[i], p.scale), 0.5f)), p.bias);
                const uint32_t u = (uint32_t)(uint8_t)(int)v & vmask;
                const int at = (int)(i * p.bits - bit0);                // -7 .. 31: a value may begin in the dword before
                w |= at >= 0 ? u << at : u >> -at;
            }
        }
        p.packed[k] = w;
    }
}
// bit-packed -> compact uint8: one byte per thread (hash_pack_u8_kernel's shape), the value's two-dword window funnel-shifted and masked
__global__ void __launch_bounds__(256) hash_unpack_bits_kernel(HashBitsParams p) {
    const int64_t n = p.pre_u8[p.levels];
    const uint32_t vmask = (1u << p.bits) - 1u;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        int64_t base = 0, dw = 0;
#pragma unroll
        for (int j = 1; j < NIC_HASH_MAX_LEVELS; ++j) {
            const bool past = j < p.levels && k >= p.pre_u8[j];
            base = past ? p.pre_u8[j] : base;
            dw = past ? p.pre[j] : dw;
        }
        const int64_t bit = (k - base) * p.bits;
        const uint32_t* q = p.packed_in + dw + (bit >> 5);
        p.dst_u8[k] = (uint8_t)(__builtin_amdgcn_alignbit(q[1], q[0], (uint32_t)bit & 31u) & vmask);
    }
}

}  // namespace nic

using namespace nic;

enum HashKernel { HK_FWD, HK_BWD, HK_FWD_NOISY, HK_FWD_U8, HK_FWD_BITS };

template <int K, int D, int F>
static void launch_k(const HashParams& p, int nb, hipStream_t s) {
    if constexpr (K == HK_BWD) hipLaunchKernelGGL((hash_encode_backward_kernel<D, F>), dim3(nb), dim3(256), 0, s, p);
    else if constexpr (K == HK_FWD_NOISY) hipLaunchKernelGGL((hash_encode_kernel<D, F, HSRC_F32, true>), dim3(nb), dim3(256), 0, s, p);
    else if constexpr (K == HK_FWD_U8) hipLaunchKernelGGL((hash_encode_kernel<D, F, HSRC_U8, false>), dim3(nb), dim3(256), 0, s, p);
    else if constexpr (K == HK_FWD_BITS) hipLaunchKernelGGL((hash_encode_kernel<D, F, HSRC_BITS, false>), dim3(nb), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((hash_encode_kernel<D, F>), dim3(nb), dim3(256), 0, s, p);
}

template <int K>
static int hash_launch(const HashParams& p, void* stream) {
    const int nb = strided_grid(count_patches(&p.d));         // one wave per patch, four waves per block
    return dispatch_dim_features(p.d, [&](auto dim, auto features) {
        launch_k<K, decltype(dim)::value, decltype(features)::value>(p, nb, (hipStream_t)stream);
    });
}

// F * sum_l E_l; pre (optional) gets the byte offset of every level and the total at [levels]
static int64_t hash_stored_prefix(const nic_hash_desc* d, int64_t* pre) {
    int64_t off = 0;
    for (int l = 0; l < d->levels; ++l) {
        if (pre) pre[l] = off;
        off += (int64_t)d->features * hash_level_entries(d->dim, d->resolution[l], d->log2_table);
    }
    if (pre) pre[d->levels] = off;
    return off;
}

// sum_l ceil(E_l F b / 32); pre (optional) gets the dword offset of every level and the first tail dword at [levels]
static int64_t hash_packed_prefix(const nic_hash_desc* d, int num_bits, int64_t* pre) {
    int64_t off = 0;
    for (int l = 0; l < d->levels; ++l) {
        if (pre) pre[l] = off;
        off += hash_level_dwords(d->dim, d->resolution[l], d->log2_table, d->features, num_bits);
    }
    if (pre) pre[d->levels] = off;
    return off;
}

extern "C" {

int nic_hash_encode(const nic_hash_desc* desc, const float* table, const int32_t* origins, float* out, void* stream) {
    const int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (!table || !origins || !out) return NIC_E_NULL;
    HashParams p{};
    p.d = *desc; p.table = table; p.origins = origins; p.out = out;
    return hash_launch<HK_FWD>(p, stream);
}

int nic_hash_encode_backward(const nic_hash_desc* desc, const int32_t* origins, const float* dx, float* table_grad, void* stream) {
    const int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (!origins || !dx || !table_grad) return NIC_E_NULL;
    HashParams p{};
    p.d = *desc; p.origins = origins; p.dx = dx; p.grad = table_grad;
    return hash_launch<HK_BWD>(p, stream);
}

int nic_hash_index_host(const nic_hash_desc* desc, int level, int32_t vx, int32_t vy, int32_t vz) {
    const int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (level < 0 || level >= desc->levels) return NIC_E_ARG;
    const int32_t R = desc->resolution[level];
    return (int)hash_index(hash_level_dense(desc->dim, R, desc->log2_table), (uint32_t)R, (1u << desc->log2_table) - 1u, (uint32_t)vx,
                           (uint32_t)vy, desc->dim == 3 ? (uint32_t)vz : 0u);
}

int nic_hash_encode_noisy(const nic_hash_desc* desc, const nic_hash_quant* quant, const float* table, const int32_t* origins, float* out,
                          void* stream) {
    int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (!quant || !table || !origins || !out) return NIC_E_NULL;
    HashParams p{};
    p.d = *desc; p.table = table; p.origins = origins; p.out = out;
    if ((rc = set_noise(quant, true, p.noise, p.sample_base)) != NIC_OK) return rc;
    return p.noise.mode == NIC_NOISE_KERNEL ? hash_launch<HK_FWD_NOISY>(p, stream) : hash_launch<HK_FWD>(p, stream);
}

int nic_hash_encode_u8(const nic_hash_desc* desc, int num_bits, const uint8_t* stored, const int32_t* origins, float* out, void* stream) {
    const int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (!stored || !origins || !out) return NIC_E_NULL;
    if (num_bits < 1 || num_bits > 8) return NIC_E_ARG;
    HashParams p{};
    p.d = *desc; p.stored = stored; p.origins = origins; p.out = out;
    set_dequant(p, num_bits);
    return hash_launch<HK_FWD_U8>(p, stream);
}

int nic_hash_pack_u8(const nic_hash_desc* desc, int num_bits, const float* table, uint8_t* stored, void* stream) {
    const int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (!table || !stored) return NIC_E_NULL;
    if (num_bits < 1 || num_bits > 8) return NIC_E_ARG;
    HashPackParams p{};
    p.src = table; p.dst = stored;
    p.levels = desc->levels; p.log2_table = desc->log2_table; p.features = desc->features;
    p.scale = (float)((1 << num_bits) - 1);
    p.bias = (float)((1 << (num_bits - 1)) - 1);
    const int64_t n = hash_stored_prefix(desc, p.pre);
    const int64_t b = (n + 255) / 256;
    hipLaunchKernelGGL(hash_pack_u8_kernel, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int64_t nic_hash_stored_bytes(const nic_hash_desc* desc) {
    const int rc = check_hash_desc(desc);
    if (rc) return rc;
    return hash_stored_prefix(desc, nullptr);
}

int64_t nic_hash_packed_bytes(const nic_hash_desc* desc, int num_bits) {
    const int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (num_bits < 1 || num_bits > 8) return NIC_E_ARG;
    return 4 * hash_packed_prefix(desc, num_bits, nullptr) + 8;
}

int nic_hash_encode_bits(const nic_hash_desc* desc, int num_bits, const uint8_t* packed, const int32_t* origins, float* out, void* stream) {
    const int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (!packed || !origins || !out) return NIC_E_NULL;
    if (num_bits < 1 || num_bits > 8) return NIC_E_ARG;
    if ((uintptr_t)packed & 3u) return NIC_E_ARG;                    // the gather reads aligned dwords
    HashParams p{};
    p.d = *desc; p.packed = (const uint32_t*)packed; p.origins = origins; p.out = out;
    p.q_bits = num_bits; p.q_tight = hash_bits_tight(desc->features, num_bits) ? 1 : 0;
    set_dequant(p, num_bits);
    return hash_launch<HK_FWD_BITS>(p, stream);
}

static int hash_bits_params(HashBitsParams& p, const nic_hash_desc* desc, int num_bits) {
    p.levels = desc->levels; p.log2_table = desc->log2_table; p.features = desc->features; p.bits = num_bits;
    p.scale = (float)((1 << num_bits) - 1);
    p.bias = (float)((1 << (num_bits - 1)) - 1);
    hash_stored_prefix(desc, p.pre_u8);
    hash_packed_prefix(desc, num_bits, p.pre);
    return 0;
}

int nic_hash_pack_bits(const nic_hash_desc* desc, int num_bits, const float* table, uint8_t* packed, void* stream) {
    const int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (!table || !packed) return NIC_E_NULL;
    if (num_bits < 1 || num_bits > 8) return NIC_E_ARG;
    if ((uintptr_t)packed & 3u) return NIC_E_ARG;
    HashBitsParams p{};
    hash_bits_params(p, desc, num_bits);
    p.src = table; p.packed = (uint32_t*)packed;
    const int64_t b = (p.pre[p.levels] + 2 + 255) / 256;
    hipLaunchKernelGGL(hash_pack_bits_kernel, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

int nic_hash_unpack_bits(const nic_hash_desc* desc, int num_bits, const uint8_t* packed, uint8_t* stored, void* stream) {
    const int rc = check_hash_desc(desc);
    if (rc) return rc;
    if (!packed || !stored) return NIC_E_NULL;
    if (num_bits < 1 || num_bits > 8) return NIC_E_ARG;
    if ((uintptr_t)packed & 3u) return NIC_E_ARG;
    HashBitsParams p{};
    hash_bits_params(p, desc, num_bits);
    p.packed_in = (const uint32_t*)packed; p.dst_u8 = stored;
    const int64_t b = (p.pre_u8[p.levels] + 255) / 256;
    hipLaunchKernelGGL(hash_unpack_bits_kernel, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

}  // extern "C"
