// plain 16-bit fused kernels (fused_q16.hpp) for quarter layout QL<2>, 3 and 5 Linear layers
#include "fused_q16_launch.hpp"
namespace nic {
template FusedKernel q16_kernels<2, 3>();
template FusedKernel q16_kernels<2, 5>();
}
