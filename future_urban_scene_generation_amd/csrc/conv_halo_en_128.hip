// Entry-NiN instantiation of the halo kernel (conv_kernel_halo.h, EN): BN = 128 column tile, waves 1 x 4 - the shape of conv_halo_128.hip.
#include "conv_kernel_halo.h"
namespace fusg {
hipError_t launch_halo_en_128(const HaloK& k, const EntryK& en, dim3 grid, hipStream_t s, bool colmajor) {
    return launch_halo_en<4,1,1,4>(k, en, grid, s, colmajor);
}
}  // namespace fusg
