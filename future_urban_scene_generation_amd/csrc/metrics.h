// Per-image quality metrics of two uint8 images, for host and device: the arithmetic fusg_image_metrics_u8 (metrics.hip)
// and its host twin share.  The definition is the test oracle's SSIM (Wang et al. 2004):
//   window   11 x 11 Gaussian, sigma 1.5, the outer product of the normalised 1-D taps; "valid" positions only, so an
//            H x W image has (H - 10) x (W - 10) of them per channel
//   sums     the five window sums of a, b, a^2, b^2 and ab, as two separable 11-tap passes (rows, then columns)
//   formula  ((2 mu_a mu_b + C1)(2 s_ab + C2)) / ((mu_a^2 + mu_b^2 + C1)(s_aa + s_bb + C2)), C1 = (0.01 * 255)^2,
//            C2 = (0.03 * 255)^2, s_xy = E[xy] - mu_x mu_y
// Everything from the window sums on is float64: s_aa = E[a^2] - mu_a^2 cancels up to 65025 against a C2 of 58.5, and
// float32 sums miss the oracle by 1.4e-5 on a nearly flat bright image.  No contraction (-ffp-contract=off), so the host
// twin and the kernel round alike.
//
// Work is cut into tiles of TILE x TILE valid positions.  A tile reads its positions' pixels plus the 10-pixel apron of the
// windows (LT x LT pixels); the integer statistics (sum of squared differences, differing values, largest difference) of a
// pixel belong to the tile whose TILE x TILE square holds it, and the last tile of a row / column also owns the apron
// behind it, so every pixel of the image is counted exactly once although aprons overlap.
// The SSIM values of a tile are summed in a fixed order - NT "threads" t = oy * TILE + ox, each adding its position's
// channels in order; a 64-lane halving tree inside each group of 64; the groups in order - and the tiles of an image in a
// fixed order again (lane l takes tiles l, l + 64, ...; the same tree).  `tree64` states that tree for the host; the kernel
// runs it with wave shuffles.
#pragma once
#include <math.h>
#include <stdint.h>
#include "resize.h"                                               // FUSG_HD

namespace fusg {
namespace im {

constexpr int WIN = 11, APRON = WIN - 1, TILE = 16, LT = TILE + APRON, MAXC = 4, NT = TILE * TILE, LANES = 64;
constexpr int COLS = 6;                                           // ssim, mse, psnr, max_abs, n_diff, sse
constexpr double K1 = 0.01, K2 = 0.03, RANGE = 255.0, SIGMA = 1.5;

struct Taps { double w[WIN]; };
struct Sums { double a, b, aa, bb, ab; };

// the normalised 1-D Gaussian (host: the kernel takes the table by value)
inline Taps gauss_taps() {
    Taps t;
    double s = 0.0;
    for (int i = 0; i < WIN; ++i) {
        const double d = (double)(i - WIN / 2);
        t.w[i] = exp(-(d * d) / (2.0 * SIGMA * SIGMA));
        s += t.w[i];
    }
    for (int i = 0; i < WIN; ++i) t.w[i] /= s;
    return t;
}

// the row pass at one pixel: a(k), b(k) = the pixel values at columns x + k, k < WIN
template <class FA, class FB>
FUSG_HD Sums row_sums(FA a, FB b, const Taps& t) {
    Sums s{0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < WIN; ++k) {
        const double w = t.w[k], x = (double)a(k), y = (double)b(k);
        s.a += w * x;
        s.b += w * y;
        s.aa += w * (x * x);
        s.bb += w * (y * y);
        s.ab += w * (x * y);
    }
    return s;
}

// the column pass: row(k) = the row sums at rows y + k, k < WIN
template <class F>
FUSG_HD Sums col_sums(F row, const Taps& t) {
    Sums s{0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < WIN; ++k) {
        const double w = t.w[k];
        const Sums r = row(k);
        s.a += w * r.a;
        s.b += w * r.b;
        s.aa += w * r.aa;
        s.bb += w * r.bb;
        s.ab += w * r.ab;
    }
    return s;
}

FUSG_HD double ssim_px(const Sums& s) {
    const double c1 = (K1 * RANGE) * (K1 * RANGE), c2 = (K2 * RANGE) * (K2 * RANGE);
    const double s_aa = s.aa - s.a * s.a, s_bb = s.bb - s.b * s.b, s_ab = s.ab - s.a * s.b;
    return ((2.0 * s.a * s.b + c1) * (2.0 * s_ab + c2)) / ((s.a * s.a + s.b * s.b + c1) * (s_aa + s_bb + c2));
}

// the tiling of one image
struct Tiling { int tiles_x, tiles_y; };
FUSG_HD Tiling tiling(int H, int W) { return Tiling{(W - APRON + TILE - 1) / TILE, (H - APRON + TILE - 1) / TILE}; }
// the first pixel past tile index i's own pixels along an axis of n pixels and nt tiles
FUSG_HD int own_end(int i, int nt, int n) { return i == nt - 1 ? n : (i + 1) * TILE; }

// lane 0's value of the halving tree over 64 lanes (host form; v is overwritten)
template <class T>
inline T tree64(T* v) {
    for (int off = LANES / 2; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] += v[l + off];
    return v[0];
}

// the six columns of one row of the table from the image's totals
FUSG_HD void finish_row(double ssim_sum, uint64_t sse, uint64_t n_diff, uint32_t max_abs, int H, int W, int C, double* out) {
    const double mse = (double)sse / ((double)H * (double)W * (double)C);
    out[0] = ssim_sum / ((double)C * (double)(H - APRON) * (double)(W - APRON));
    out[1] = mse;
    out[2] = sse == 0 ? (double)INFINITY : 10.0 * log10((RANGE * RANGE) / mse);
    out[3] = (double)max_abs;
    out[4] = (double)n_diff;
    out[5] = (double)sse;
}

// per-tile partials in the caller's scratch: B * T of each, in this order (8-byte items first)
struct Scratch { size_t off_sse, off_nd, off_mx, total; };
inline Scratch scratch_layout(long B, long T) {
    const size_t n = (size_t)B * (size_t)T;
    Scratch s;
    s.off_sse = n * sizeof(double);
    s.off_nd = s.off_sse + n * sizeof(uint64_t);
    s.off_mx = s.off_nd + n * sizeof(uint32_t);
    s.total = (s.off_mx + n * sizeof(uint32_t) + 15) / 16 * 16;
    return s;
}

}  // namespace im
}  // namespace fusg
