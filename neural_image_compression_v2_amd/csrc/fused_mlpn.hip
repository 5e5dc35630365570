// depth-generic 2D fused kernels (fused_mlpn.hpp): NL = 5 (the "4 x 64" decoder) for training and decode; NL = 3 is instantiated too,
// as the cross-check of the layer loop against the dedicated 3-layer kernels (NIC_FLAG_MLPN).
#include "fused_mlpn.hpp"
#include "fused_dispatch.hpp"

namespace nic {

template <class L, int NL>
static int launch_n(int mode, const FusedParams& p, int grid, hipStream_t s) {
    const dim3 g(grid), b(256);
    if (mode == MODE_INFER) hipLaunchKernelGGL((fused_mlpn_kernel<L, MODE_INFER, NL>), g, b, 0, s, p);
    else if (mode == MODE_TRAIN_MSE) hipLaunchKernelGGL((fused_mlpn_kernel<L, MODE_TRAIN_MSE, NL>), g, b, 0, s, p);
    else if (mode == MODE_TRAIN_IMG) hipLaunchKernelGGL((fused_mlpn_kernel<L, MODE_TRAIN_IMG, NL>), g, b, 0, s, p);
    else if (mode == MODE_TRAIN_DY) hipLaunchKernelGGL((fused_mlpn_kernel<L, MODE_TRAIN_DY, NL>), g, b, 0, s, p);
    else return NIC_E_UNSUPPORTED;
    return (int)hipGetLastError();
}

template <class L, int NL>
static int reduce_n(const FusedParams& p, int n_rec, const nic_mlp_grads& g, float* loss, hipStream_t s) {
    constexpr int n_out = kH * 73 + kH + (NL - 2) * (kH * kH + kH) + 3 * kH + 3 + 1;
    const TailLaunch t = tail_for((n_out + 31) / 32);
    hipLaunchKernelGGL((reducen_kernel<L, NL>), dim3(t.blocks), dim3(256), 0, s, p.partials, n_rec, g, loss, p.d.loss_scale, t.tl);
    return (int)hipGetLastError();
}

template <int LAYOUT, int NL>
FusedKernel mlpn_kernels() {
    return {FAM_MLPN, LAYOUT, kC, kP, NL, {LdsN<NL>::REC, 16, 1, 1, 73, 4}, &launch_n<Layout<LAYOUT>, NL>, &reduce_n<Layout<LAYOUT>, NL>};
}
template FusedKernel mlpn_kernels<1, 3>();
template FusedKernel mlpn_kernels<1, 5>();
template FusedKernel mlpn_kernels<2, 3>();
template FusedKernel mlpn_kernels<2, 5>();

}  // namespace nic
