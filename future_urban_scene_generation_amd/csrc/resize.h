// cv::resize INTER_LINEAR for uint8, written once for host and device (cvops.hip, inpaint_inputs.h): source index / 11-bit
// weights of one destination coordinate (float arithmetic as in resize.cpp), horizontal pass in int, vertical pass
// ((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2.  Restated independently in oracle/cv_host.py (resize_linear_u8).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define FUSG_HD __host__ __device__ __forceinline__
#else
#define FUSG_HD inline
#endif

namespace fusg {

FUSG_HD void resize_coef(int d, int ssize, int dsize, int& s, int& a0, int& a1) {
    const double scale = (double)ssize / dsize;
    float f = (float)((d + 0.5) * scale - 0.5);
    int si = (int)floorf(f);
    f -= (float)si;
    if (si < 0) { f = 0.f; si = 0; }
    if (si >= ssize - 1) { f = 0.f; si = ssize - 1; }
    s = si;
    a0 = (int)rintf((1.f - f) * 2048.f);
    a1 = (int)rintf(f * 2048.f);
}

// the vertical pass on two horizontally interpolated rows S0, S1 (<< 11), clamped to uint8
FUSG_HD int resize_mix(int S0, int S1, int ay0, int ay1) {
    const int o = (((ay0 * (S0 >> 4)) >> 16) + ((ay1 * (S1 >> 4)) >> 16) + 2) >> 2;
    return o < 0 ? 0 : (o > 255 ? 255 : o);
}

}  // namespace fusg
