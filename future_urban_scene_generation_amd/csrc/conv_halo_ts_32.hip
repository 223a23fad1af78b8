// Tap-sparse instantiations of the halo kernel (conv_kernel_halo.h, SP): BN = 32 column tile, waves 4 x 1 - the shape of conv_halo_32.hip.
#include "conv_kernel_halo.h"
namespace fusg {
hipError_t launch_halo_ts_32(const HaloK& k, dim3 grid, hipStream_t s, int pk, int mode, int sp) { return launch_halo_ts<1,1,4,1>(k, grid, s, pk, mode, sp); }
}  // namespace fusg
