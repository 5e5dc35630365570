// fused kernels for Layout<3> (see nic_device.hpp)
#include "fused_launch.hpp"
namespace nic {
template FusedKernel fused_kernels<3, SRC_ENCODE>();
template FusedKernel fused_kernels<3, SRC_MEMORY>();
}
