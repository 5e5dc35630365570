// Host-side launchers of fused_kernel; one translation unit per layout (fused_m1.hip .. fused_m4.hip) so the big template instantiation sets
// compile in parallel.
#pragma once
#include "fused_dispatch.hpp"

namespace nic {

template <int METHOD, int SRC>
static int launch_fused(int mode, const FusedParams& p, int grid, hipStream_t s) {
    using L = Layout<METHOD>;
    const dim3 g(grid), b(256);
    if constexpr (SRC == SRC_MEMORY) {
        if (mode == MODE_INFER) hipLaunchKernelGGL((fused_kernel<L, SRC_MEMORY, MODE_INFER>), g, b, 0, s, p);
        else if (mode == MODE_TRAIN_DY) hipLaunchKernelGGL((fused_kernel<L, SRC_MEMORY, MODE_TRAIN_DY>), g, b, 0, s, p);
        else return NIC_E_UNSUPPORTED;
    } else if (mode == MODE_INFER && (p.d.flags & NIC_FLAG_SPLIT_BF16) && L::NSLOT % 8 == 0) {   // 2D and 3D method 3
        if constexpr (L::NSLOT % 8 == 0) {
            if (p.grid_u8) hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_INFER, uint8_t, PREC_SPLIT>), g, b, 0, s, p);
            else hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_INFER, float, PREC_SPLIT>), g, b, 0, s, p);
        }
    }
    else if (mode == MODE_INFER && p.grid_u8) hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_INFER, uint8_t>), g, b, 0, s, p);
    else if (p.grid_u8) return NIC_E_UNSUPPORTED;
    else if (mode == MODE_INFER) hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_INFER>), g, b, 0, s, p);
    else if (p.d.flags & NIC_FLAG_SPLIT_BF16) {                          // training kernels, 2D layouts
        if constexpr (L::NSLOT % 8 == 0 && L::DIM == 2) {
            if (mode == MODE_TRAIN_MSE) hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_TRAIN_MSE, float, PREC_SPLIT>), g, b, 0, s, p);
            else if (mode == MODE_TRAIN_IMG) hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_TRAIN_IMG, float, PREC_SPLIT>), g, b, 0, s, p);
            else hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_TRAIN_DY, float, PREC_SPLIT>), g, b, 0, s, p);
        } else if constexpr (L::NSLOT % 8 == 0) {     // 3D: chained products only (PREC_CHAIN)
            if (mode == MODE_TRAIN_MSE) hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_TRAIN_MSE, float, PREC_CHAIN>), g, b, 0, s, p);
            else if (mode == MODE_TRAIN_IMG) hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_TRAIN_IMG, float, PREC_CHAIN>), g, b, 0, s, p);
            else hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_TRAIN_DY, float, PREC_CHAIN>), g, b, 0, s, p);
        } else return NIC_E_UNSUPPORTED;
    }
    else if (mode == MODE_TRAIN_MSE) hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_TRAIN_MSE>), g, b, 0, s, p);
    else if (mode == MODE_TRAIN_IMG) hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_TRAIN_IMG>), g, b, 0, s, p);
    else hipLaunchKernelGGL((fused_kernel<L, SRC_ENCODE, MODE_TRAIN_DY>), g, b, 0, s, p);
    return (int)hipGetLastError();
}

template <int METHOD>
static int reduce_fused(const FusedParams& p, int n_rec, const nic_mlp_grads& g, float* loss, hipStream_t s) {
    using L = Layout<METHOD>;
    const int n = Lds<L>::NACC * 1024 + Lds<L>::TAIL;
    const TailLaunch t = tail_for((n + 31) / 32);
    hipLaunchKernelGGL((reduce_partials_kernel<L>), dim3(t.blocks), dim3(256), 0, s, p.partials, n_rec, g, loss, p.d.loss_scale, t.tl);
    return (int)hipGetLastError();
}

template <int METHOD, int SRC>
FusedKernel fused_kernels() {
    using L = Layout<METHOD>;
    return {SRC == SRC_ENCODE ? FAM_FUSED : FAM_DECODER, METHOD, kC, kP, 3, {Lds<L>::REC, L::TX, L::TY, L::TZ, L::CIN, 4},
            &launch_fused<METHOD, SRC>, &reduce_fused<METHOD>};
}

}  // namespace nic
