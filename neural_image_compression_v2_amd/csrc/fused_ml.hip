// multi-level plain-bf16 fused kernels (fused_q16.hpp::QML) for one NIC_ML_LIST entry (fused_capi.hip): _build.py compiles this file once per
// entry, with NIC_ENTRY = levels, C, n_linear
#include "fused_q16_launch.hpp"
namespace nic {
template FusedKernel ml_kernels<NIC_ENTRY>();
}
