// plain-bf16 fused kernels (fused_q16.hpp) for one NIC_CP_LIST entry (fused_capi.hip): _build.py compiles this file once per entry, with
// NIC_ENTRY = layout, C, P
#include "fused_q16_launch.hpp"
namespace nic {
template FusedKernel q16_cp_kernels<NIC_ENTRY>();
}
