// Tap-sparse instantiations of the halo kernel (conv_kernel_halo.h, SP): BN = 128 column tile, waves 1 x 4 - the shape of conv_halo_128.hip.
#include "conv_kernel_halo.h"
namespace fusg {
hipError_t launch_halo_ts_128(const HaloK& k, dim3 grid, hipStream_t s, int pk, int mode, int sp) { return launch_halo_ts<4,1,1,4>(k, grid, s, pk, mode, sp); }
}  // namespace fusg
