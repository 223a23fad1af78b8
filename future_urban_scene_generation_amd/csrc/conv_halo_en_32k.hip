// Entry-NiN instantiation of the halo kernel (conv_kernel_halo.h, EN): BN = 32 column tile with K split over the four waves - the
// shape of conv_halo_32k.hip, which small grids give the 128-column layer too.
#include "conv_kernel_halo.h"
namespace fusg {
hipError_t launch_halo_en_32k(const HaloK& k, const EntryK& en, dim3 grid, hipStream_t s) { return launch_halo_en<4,1,1,1,4>(k, en, grid, s); }
}  // namespace fusg
