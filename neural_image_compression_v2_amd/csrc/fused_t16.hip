// the 8-wave / 16-sample 2D training kernels (fused_train16.hpp): Layout<1> (triangular PE) and Layout<2> (sinusoidal PE)
#include "fused_train16.hpp"
#include "fused_dispatch.hpp"

namespace nic {

template <class L>
static int launch_t16(int mode, const FusedParams& p, int grid, hipStream_t s) {
    const dim3 g(grid), b(512);
    if (mode == MODE_TRAIN_MSE) hipLaunchKernelGGL((fused_train16_kernel<L, MODE_TRAIN_MSE>), g, b, 0, s, p);
    else if (mode == MODE_TRAIN_IMG && p.timg_u8 == 2) hipLaunchKernelGGL((fused_train16_kernel<L, MODE_TRAIN_RGBX>), g, b, 0, s, p);
    else if (mode == MODE_TRAIN_IMG) hipLaunchKernelGGL((fused_train16_kernel<L, MODE_TRAIN_IMG>), g, b, 0, s, p);
    else if (mode == MODE_TRAIN_DY) hipLaunchKernelGGL((fused_train16_kernel<L, MODE_TRAIN_DY>), g, b, 0, s, p);
    else return NIC_E_UNSUPPORTED;
    return (int)hipGetLastError();
}

template <class L>
static int reduce_t16(const FusedParams& p, int n_rec, const nic_mlp_grads& g, float* loss, hipStream_t s) {
    constexpr int outs = 256 / NIC_R16_SLICES;
    const TailLaunch t = tail_for((kR16_SRC + outs - 1) / outs);
    hipLaunchKernelGGL((reduce16_kernel<L>), dim3(t.blocks), dim3(256), 0, s, p.partials, n_rec, g, loss, p.d.loss_scale, t.tl);
    return (int)hipGetLastError();
}

template <int LAYOUT>
FusedKernel train16_kernels() {
    return {FAM_T16, LAYOUT, kC, kP, 3, {Lds16::REC, 16, 1, 1, 73, 8}, &launch_t16<Layout<LAYOUT>>, &reduce_t16<Layout<LAYOUT>>};
}
template FusedKernel train16_kernels<1>();
template FusedKernel train16_kernels<2>();

}  // namespace nic
