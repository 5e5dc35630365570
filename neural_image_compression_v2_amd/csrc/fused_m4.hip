// fused kernels for Layout<4> (see nic_device.hpp)
#include "fused_launch.hpp"
namespace nic {
template FusedKernel fused_kernels<4, SRC_ENCODE>();
template FusedKernel fused_kernels<4, SRC_MEMORY>();
}
