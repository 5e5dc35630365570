// Host-side launchers of fused_q16_kernel: the quarter layouts QL<METHOD> (fused_q1.hip .. fused_q4.hip), their other channel counts
// (fused_qc.hip) and the multi-level layouts (fused_ml.hip), one translation unit per instantiation set so they compile in parallel.
#pragma once
#include "fused_q16.hpp"
#include "fused_dispatch.hpp"

namespace nic {

template <class Q, int NL, bool F16 = false>
static int launch_q16_nl(int mode, const FusedParams& p, int grid, hipStream_t s) {
    const dim3 g(grid), b(512);
    if (mode == MODE_TRAIN_MSE) hipLaunchKernelGGL((fused_q16_kernel<Q, MODE_TRAIN_MSE, NL, F16>), g, b, 0, s, p);
    else if (mode == MODE_TRAIN_IMG) hipLaunchKernelGGL((fused_q16_kernel<Q, MODE_TRAIN_IMG, NL, F16>), g, b, 0, s, p);
    else if (mode == MODE_TRAIN_DY) hipLaunchKernelGGL((fused_q16_kernel<Q, MODE_TRAIN_DY, NL, F16>), g, b, 0, s, p);
    else if (mode == MODE_INFER) hipLaunchKernelGGL((fused_q16_kernel<Q, MODE_INFER, NL, F16>), g, b, 0, s, p);
    else return NIC_E_UNSUPPORTED;
    return (int)hipGetLastError();
}
// the default channel counts also run on IEEE half operands (NIC_FLAG_FP16)
template <class Q, int NL>
static int launch_q16_f16(int mode, const FusedParams& p, int grid, hipStream_t s) {
    return p.f16 ? launch_q16_nl<Q, NL, true>(mode, p, grid, s) : launch_q16_nl<Q, NL>(mode, p, grid, s);
}
// the multi-level layouts: the training step on a target tensor and the forward pass
template <class Q, int NL>
static int launch_ml(int mode, const FusedParams& p, int grid, hipStream_t s) {
    const dim3 g(grid), b(512);
    if (mode == MODE_TRAIN_MSE) hipLaunchKernelGGL((fused_q16_kernel<Q, MODE_TRAIN_MSE, NL>), g, b, 0, s, p);
    else if (mode == MODE_INFER) hipLaunchKernelGGL((fused_q16_kernel<Q, MODE_INFER, NL>), g, b, 0, s, p);
    else return NIC_E_UNSUPPORTED;
    return (int)hipGetLastError();
}
template <int LV, int C, int NL>
static int launch_ml_pe(int mode, const FusedParams& p, int grid, hipStream_t s) {
    return p.d.pe_mode == NIC_PE_TRIANGULAR ? launch_ml<QML<LV, C, 6, NIC_PE_TRIANGULAR>, NL>(mode, p, grid, s)
                                            : launch_ml<QML<LV, C, 6, NIC_PE_SINUSOIDAL>, NL>(mode, p, grid, s);
}

template <class Q, int NL>
static int reduce_q16(const FusedParams& p, int n_rec, const nic_mlp_grads& g, float* loss, hipStream_t s) {
    constexpr int n_out = reduce_q16_outputs<Q, NL>();
    static_assert(256 % NIC_RQ_SLICES == 0, "256 threads per block (the tail's streaming blocks too: nic_adam.hpp)");
    constexpr int outs = 256 / NIC_RQ_SLICES;
    const TailLaunch t = tail_for((n_out + outs - 1) / outs);
    hipLaunchKernelGGL((reduce_q16_kernel<Q, NL>), dim3(t.blocks), dim3(256), 0, s, p.partials, n_rec, g, loss, p.d.loss_scale, t.tl);
    return (int)hipGetLastError();
}
template <int LV, int C, int NL>
static int reduce_ml_pe(const FusedParams& p, int n_rec, const nic_mlp_grads& g, float* loss, hipStream_t s) {
    return p.d.pe_mode == NIC_PE_TRIANGULAR ? reduce_q16<QML<LV, C, 6, NIC_PE_TRIANGULAR>, NL>(p, n_rec, g, loss, s)
                                            : reduce_q16<QML<LV, C, 6, NIC_PE_SINUSOIDAL>, NL>(p, n_rec, g, loss, s);
}

template <int METHOD, int NL>
FusedKernel q16_kernels() {
    using Q = QL<METHOD>;
    return {FAM_Q16, METHOD, kC, kP, NL, {LdsQ<Q, NL>::REC, 16, 1, 1, Q::CIN, 8}, &launch_q16_f16<Q, NL>, &reduce_q16<Q, NL>};
}
// other channel counts: 3-layer decoder, bf16 operands
template <int METHOD, int C, int P>
FusedKernel q16_cp_kernels() {
    using Q = QL<METHOD, C, P>;
    return {FAM_Q16, METHOD, C, P, 3, {LdsQ<Q, 3>::REC, 16, 1, 1, Q::CIN, 8}, &launch_q16_nl<Q, 3>, &reduce_q16<Q, 3>};
}
template <int LV, int C, int NL>
FusedKernel ml_kernels() {
    using Q = QML<LV, C, 6, NIC_PE_TRIANGULAR>;                 // (the record and the inputs do not depend on the encoding)
    return {FAM_ML, LV, C, 6, NL, {LdsQ<Q, NL>::REC, 16, 1, 1, Q::CIN, 8}, &launch_ml_pe<LV, C, NL>, &reduce_ml_pe<LV, C, NL>};
}

}  // namespace nic
