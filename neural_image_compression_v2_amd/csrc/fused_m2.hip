// fused kernels for Layout<2> (2D, sinusoidal PE; see nic_device.hpp)
#include "fused_launch.hpp"
namespace nic {
template FusedKernel fused_kernels<2, SRC_ENCODE>();
template FusedKernel fused_kernels<2, SRC_MEMORY>();
}
