// The per-row sums behind the GAN objectives (EdgeConnect's AdversarialLoss, Warp&Learn's GANLoss) and the count-excluding
// 3 x 3 stride-2 average pool, for host and device: the rules fusg_gan_terms_rows_f32 and fusg_avgpool3s2_f32 (gan_terms.hip)
// share with their host twins.
//
// Terms.  A row is one image of pred [B, C, H, W]; its n = C H W elements x are taken in the order (y, x, c), c fastest, each
// widened to float64 first.  Columns of out[r]:
//   0  n
//   1  sum x
//   2  sum (m x - m label)^2      m = the mask sampled at the element's pixel (nearest, below), 1 without a mask
//   3  sum relu(1 + x)
//   4  sum relu(1 - x)
//   5  sum -[label max(log x, -100) + (1 - label) max(log(1 - x), -100)]      nn.BCELoss's clamp; NaN for x outside [0, 1]
// log is glog below on both sides - plain float64 +, *, / and fma in one order, so host and device agree to the bit, which
// neither's library log promises.  The mask multiplies in column 2 only (GANLoss's use).
//   chunks   G = groups(n) workgroups of WG per row, a function of n only; chunk g is the elements [g K, min(n, (g + 1) K)),
//            K = chunk(n) = ceil(n / G) rounded up to a multiple of WG
//   sums     thread t of chunk g adds elements g K + t, + WG, ... in order; the 64 lanes of a wave by the halving tree, the
//            four waves in order; then lane l of one wave per row adds chunks l, l + 64, ... and the same tree
// Mask.  [B, 1, Hm, Wm] is read as F.interpolate(mask, size=(H, W)) reads it in its default nearest mode: source index
// min((int)floorf(dst * scale), Hm - 1), scale = (float)Hm / (float)H (Wm / W for columns).
//
// Pool.  nn.AvgPool2d(3, stride=2, padding=1, count_include_pad=False): output floor((H - 1) / 2) + 1; the taps inside the
// image are added to +0 in fp32 in raster order, then divided once by their number (4, 6 or 9; fewer for
// images narrower than the window).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "resize.h"                                               // FUSG_HD

namespace fusg {
namespace gt {

constexpr int LANES = 64, WG = 256, PER_GROUP = 4096, MAX_GROUPS = 256, COLUMNS = 6, SUMS = 5, MAX_B = 1 << 16;

FUSG_HD int groups(long n) {
    const long want = (n + PER_GROUP - 1) / PER_GROUP;
    return (int)(want < 1 ? 1 : (want > MAX_GROUPS ? MAX_GROUPS : want));
}
FUSG_HD long chunk(long n) {
    const long g = groups(n), k = (n + g - 1) / g;
    return (k + WG - 1) / WG * WG;
}

// natural logarithm of a float64: x = m 2^e with m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1),
// log x = e ln2 + 2 s (1 + s^2 / 3 + s^4 / 5 + ...) - |s| < 0.1716, the series cut after s^24 / 25 (< 2e-20 relative).
// A few ulp; log 0 = -inf, negative or NaN -> NaN, +inf -> +inf.  Subnormals are scaled up first.
FUSG_HD double glog(double x) {
    if (!(x >= 0.0)) return NAN;
    if (x == 0.0) return -INFINITY;
    if (x > 1.7976931348623157e308) return x;
    int e = 0;
    if (x < 2.2250738585072014e-308) { x *= 4503599627370496.0; e = -52; }      // 2^52
    uint64_t u;
    memcpy(&u, &x, 8);
    e += (int)((u >> 52) & 0x7ff) - 1023;
    u = (u & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL;
    double m;
    memcpy(&m, &u, 8);                                             // [1, 2)
    if (m >= 1.4142135623730951) { m *= 0.5; e += 1; }
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double p = 1.0 / 25.0;
    p = fma(p, z, 1.0 / 23.0);
    p = fma(p, z, 1.0 / 21.0);
    p = fma(p, z, 1.0 / 19.0);
    p = fma(p, z, 1.0 / 17.0);
    p = fma(p, z, 1.0 / 15.0);
    p = fma(p, z, 1.0 / 13.0);
    p = fma(p, z, 1.0 / 11.0);
    p = fma(p, z, 1.0 / 9.0);
    p = fma(p, z, 1.0 / 7.0);
    p = fma(p, z, 1.0 / 5.0);
    p = fma(p, z, 1.0 / 3.0);
    const double lm = fma(2.0 * s * z, p, 2.0 * s);               // log m
    const double ed = (double)e;
    // ln2 = hi + lo, hi with 21 trailing zero bits: ed * hi is exact
    return fma(ed, 6.93147180369123816490e-01, fma(ed, 1.90821492927058770002e-10, lm));
}

FUSG_HD double clamp_log(double x) { const double l = glog(x); return l < -100.0 ? -100.0 : l; }   // a NaN stays

// the five summands of one element; acc[i] += them, in this order of operations on both sides
FUSG_HD void add_terms(double* acc, float xf, float mf, double label) {
    const double x = (double)xf, m = (double)mf;
    const double d = m * x - m * label;
    const double p1 = 1.0 + x, m1 = 1.0 - x;
    acc[0] += x;
    acc[1] += d * d;
    acc[2] += p1 > 0.0 ? p1 : (p1 != p1 ? p1 : 0.0);
    acc[3] += m1 > 0.0 ? m1 : (m1 != m1 ? m1 : 0.0);
    acc[4] += -(label * clamp_log(x) + (1.0 - label) * clamp_log(m1));
}

FUSG_HD int nearest_src(int d, float scale, int n) {
    const int i = (int)floorf((float)d * scale);
    return i < n - 1 ? i : n - 1;
}

// lane 0's value of the halving tree over 64 lanes (host form; v is overwritten)
inline double tree64(double* v) {
    for (int off = LANES / 2; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] += v[l + off];
    return v[0];
}

// ---- pool
FUSG_HD int pool_out(long n) { return (int)((n - 1) / 2 + 1); }

}  // namespace gt
}  // namespace fusg
