// Tap-sparse instantiations of the halo kernel (conv_kernel_halo.h, SP): BN = 64 column tile, waves 2 x 2 - the shape of conv_halo_64.hip.
#include "conv_kernel_halo.h"
namespace fusg {
hipError_t launch_halo_ts_64(const HaloK& k, dim3 grid, hipStream_t s, int pk, int mode, int sp) { return launch_halo_ts<2,1,2,2>(k, grid, s, pk, mode, sp); }
}  // namespace fusg
