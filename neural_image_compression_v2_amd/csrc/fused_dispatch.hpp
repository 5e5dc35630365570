// The record of every instantiated fused-kernel set: what the host needs to size, launch and reduce it.  Each family's translation unit
// defines its records; fused_capi.hip collects them into one table and picks from it.
#pragma once
#include "fused_kernel.hpp"

namespace nic {

struct FusedInfo {
    int rec;              // floats of the partial record of one workgroup
    int tx, ty, tz;       // macro-tile, in cell blocks
    int cin;              // decoder inputs
    int waves;            // waves per workgroup (= work units per workgroup round)
};
enum Family {
    FAM_FUSED,            // fused_kernel (fused_launch.hpp): 32 samples x 4 waves, every layout, 3 Linear layers
    FAM_DECODER,          // .. its SRC_MEMORY form: decoder inputs read from memory (nic_decoder_*)
    FAM_T16,              // fused_train16_kernel (fused_t16.hip): 16 samples x 8 waves, 2D split-bf16 training
    FAM_MLPN,             // fused_mlpn_kernel (fused_mlpn.hip): depth-generic, 2D split-bf16
    FAM_Q16,              // fused_q16_kernel on QL<layout, C, P> (fused_q16_launch.hpp): plain bf16 / fp16 products
    FAM_ML,               // .. on QML<levels, C, 6, pe>: several level pairs per sample
};
struct FusedKernel {
    Family family;
    int layout, c, p, n_linear;       // the key of the set (FAM_ML: layout = level pairs)
    FusedInfo info;
    int (*launch)(int mode, const FusedParams& p, int grid, hipStream_t s);                                  // MODE_*
    int (*reduce)(const FusedParams& p, int n_rec, const nic_mlp_grads& g, float* loss, hipStream_t s);    // sums p.partials
};

template <int METHOD, int SRC>
FusedKernel fused_kernels();          // fused_m<METHOD>.hip
template <int LAYOUT>
FusedKernel train16_kernels();        // fused_t16.hip
template <int LAYOUT, int NL>
FusedKernel mlpn_kernels();           // fused_mlpn.hip
template <int METHOD, int NL>
FusedKernel q16_kernels();            // fused_q<METHOD>.hip
template <int METHOD, int C, int P>
FusedKernel q16_cp_kernels();         // fused_qc.hip: NIC_CP_LIST
template <int LV, int C, int NL>
FusedKernel ml_kernels();             // fused_ml.hip: NIC_ML_LIST

}  // namespace nic
