// fused kernels for Layout<1> (2D, triangular PE; see nic_device.hpp)
#include "fused_launch.hpp"
namespace nic {
template FusedKernel fused_kernels<1, SRC_ENCODE>();
template FusedKernel fused_kernels<1, SRC_MEMORY>();
}
