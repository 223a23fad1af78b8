// Tap-sparse instantiations of the halo kernel (conv_kernel_halo.h, SP): BN = 64 column tile, K split over two waves per 32-column tile - the shape of conv_halo_64k.hip.
#include "conv_kernel_halo.h"
namespace fusg {
hipError_t launch_halo_ts_64k(const HaloK& k, dim3 grid, hipStream_t s, int pk, int mode, int sp) { return launch_halo_ts<4,1,1,2,2>(k, grid, s, pk, mode, sp); }
}  // namespace fusg
