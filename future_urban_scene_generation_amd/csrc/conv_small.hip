// Small-spatial split-fp16 convolution (conv_kernel_small.h): launcher.
#include "conv_kernel_small.h"
namespace fusg {
hipError_t launch_small(const SmallK& k, dim3 grid, hipStream_t s, int pk) {
    const size_t lds = small_lds_bytes(k.nchw, k.NPIX);
    const void* fn = pick_pk(pk, [](auto pkc) { return (const void*)conv_small_h3<decltype(pkc)::value>; });
    SmallK kk = k;
    kk.part_off = (int)((size_t)2 * k.nchw * k.NPIX * 32 * sizeof(_Float16));
    return launch_kernel(fn, grid, lds, 144 * 1024, kk, s);
}
}  // namespace fusg
