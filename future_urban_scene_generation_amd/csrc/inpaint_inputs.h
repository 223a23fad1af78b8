// EdgeConnect's four input tensors from a detector mask - create_inpaint_inputs_shape (utils/inpaint_utils.py:35-58,
// called at trajectory_inference.py:121 and :326) - written once for host and device.  The definition the kernels are
// pinned to (parity with OpenCV / scikit-image themselves is unpinned):
//
// Inputs per vehicle v: the frame (u8 HWC, channel order as stored: the reference applies the BGR formulas, so channel 0
// takes the "B" weight), box = (x0, y0, x1, y1) = bbox_new_img (half-open, as the reference slices it) and a detector mask
// u8 [V, 1, H, W] in frame coordinates that is read ONLY inside the box (non-zero = vehicle): pixels outside the box do
// not exist for the dilation.  R = 256; sigma is a float (default 2.0, edgeconnect/config.py:48).
//  1 dilate (:42-43)   OpenCV's 8 x 8 ellipse as getStructuringElement builds it: r = c = 4; row i: dy = i - 4,
//                      dx = round_half_even(c * sqrt((r^2 - dy^2) / r^2)), columns max(c - dx, 0) .. min(c + dx + 1, 8) - 1
//                      (rows {4}, 1-7, 1-7, 0-7, 0-7, 0-7, 1-7, 1-7: 53 taps); anchor (4, 4);
//                      dst(y, x) = max over taps (i, j) of src(y + i - 4, x + j - 4), taps outside the box ignored.
//  2 whiten (:44-45)   box pixels whose dilated mask is 255 become (255, 255, 255).
//  3 resize (:46, :48) cv2.resize(.., (256, 256)) INTER_LINEAR of the whitened box and of the dilated mask (resize.h).
//  4 gray (:47)        of the RESIZED image, OpenCV 4's 8-bit formula (3735 c0 + 19235 c1 + 9798 c2 + 16384) >> 15.
//  5 binarise (:49-50) mask = 255 where the resized mask > 0; valid = (mask == 0) is Canny's mask.
//  6 Canny (:51)       scikit-image's algorithm in float64, no contraction, only + - * / sqrt; the Gaussian weights are a
//                      host-computed table w[0 .. radius], radius = int(4 sigma + 0.5), w[k] = exp(-k^2 / (2 sigma^2)) / sum:
//    a  m = gray where valid else 0 (0 .. 255 scale), f = valid as 0 / 1
//    b  Gaussian of m and f, zero outside the image, axis 0 then axis 1, summed as SciPy's symmetric branch does:
//       t = x[l] w[0]; for d = radius .. 1: t += (x[l - d] + x[l + d]) w[d]
//    c  s = G(m) / (G(f) + 2.220446049250313e-16)
//    d  gi = sobel(s, axis 0), gj = sobel(s, axis 1): derivative [-1, 0, 1] along the axis first, then [1, 2, 1] across
//       it, the edge sample repeated (mode 'reflect'); mag = sqrt(gi gi + gj gj)
//    e  er = valid eroded by the full 3 x 3, outside = false (image-border pixels are never edges)
//    f  non-maximum suppression on er & mag > 0, four sectors evaluated in order, a later one overwrites (nms_px)
//    g  low = lm & mag >= 25.5, high = lm & mag >= 51.0 (0.1 and 0.2 of 255)
//    h  hysteresis: every low pixel whose 8-connected low component holds a high pixel
//  7 outputs (:53-56)  img [V, 3, R, R] and gray [V, 1, R, R] = v / 255, mask and edge [V, 1, R, R] exactly 0.0 / 1.0, float32.
// A zero-extent box gives img = gray = mask = edge = 0.
//
// Everything below is per-pixel (or per 64-pixel word) arithmetic over caller-provided fetch functions: the device kernels
// (inpaint_inputs.hip) feed it from LDS tiles, the host twin from plain arrays.  All float operations are correctly
// rounded on both sides and the translation unit is compiled with -ffp-contract=off, so the two agree bit for bit.
#pragma once
#include <stdint.h>
#include "resize.h"

namespace fusg {
namespace ii {

constexpr int R = 256;                               // EdgeConnect's input size (hard-coded in the reference)
constexpr int KS = 8, ANCHOR = 4;                    // the structuring element
constexpr int MAX_RADIUS = 32;                       // Gaussian table: sigma up to 8
constexpr int WPR = R / 64;                          // 64-pixel words per row of the hysteresis bitmaps
constexpr double EPS = 2.220446049250313e-16;        // np.finfo(float).eps
constexpr double LOW_T = 25.5, HIGH_T = 51.0;

struct Gauss { double w[MAX_RADIUS + 1]; int radius; };
struct Ellipse { int8_t j0[KS], j1[KS]; };           // inclusive column span of every row

FUSG_HD void ellipse_row(int i, int& j0, int& j1) {
    const int r = KS / 2, c = KS / 2, dy = i - r;
    const int dx = (int)__builtin_rint((double)c * __builtin_sqrt((double)(r * r - dy * dy) / (double)(r * r)));
    j0 = c - dx > 0 ? c - dx : 0;
    j1 = (c + dx + 1 < KS ? c + dx + 1 : KS) - 1;
}
FUSG_HD Ellipse ellipse() {
    Ellipse e;
    for (int i = 0; i < KS; ++i) {
        int a, b;
        ellipse_row(i, a, b);
        e.j0[i] = (int8_t)a;
        e.j1[i] = (int8_t)b;
    }
    return e;
}

// A box row (x0, y0, x1, y1) as origin and extent; a box that leaves the frame or exceeds the extents the scratch was sized
// for has no pixels (the host entry points refuse it where they can see it; the device never reads outside the frame).
struct Box { int x0, y0, bw, bh; };
FUSG_HD bool box_ok(const int32_t* b, int H, int W, int max_h, int max_w) {
    return b[0] >= 0 && b[1] >= 0 && b[2] >= b[0] && b[3] >= b[1] && b[2] <= W && b[3] <= H && b[2] - b[0] <= max_w && b[3] - b[1] <= max_h;
}
FUSG_HD Box box_of(const int32_t* b, int H, int W, int max_h, int max_w) {
    Box o = {0, 0, 0, 0};
    if (box_ok(b, H, W, max_h, max_w)) { o.x0 = b[0]; o.y0 = b[1]; o.bw = b[2] - b[0]; o.bh = b[3] - b[1]; }
    return o;
}

// step 1 at box pixel (y, x); src(yy, xx): the mask at an in-box position
template <class F>
FUSG_HD int dilate_px(F src, int y, int x, int bh, int bw, const Ellipse& e) {
    int m = 0;
    for (int i = 0; i < KS; ++i) {
        const int yy = y + i - ANCHOR;
        if ((unsigned)yy >= (unsigned)bh) continue;
        for (int j = e.j0[i]; j <= e.j1[i]; ++j) {
            const int xx = x + j - ANCHOR;
            if ((unsigned)xx >= (unsigned)bw) continue;
            const int v = src(yy, xx);
            m = v > m ? v : m;
        }
    }
    return m;
}

// steps 2-5 at output pixel (y, x) of the R x R images; img(yy, xx, c): the frame at an in-box position, dil(yy, xx): the
// dilated mask there.  c[3], gray: uint8 values; hole: the binarised mask.
struct BoxPx { int c[3]; int gray; bool hole; };
template <class FI, class FM>
FUSG_HD BoxPx box_px(FI img, FM dil, int y, int x, int bh, int bw) {
    BoxPx o = {{0, 0, 0}, 0, false};
    if (bw <= 0 || bh <= 0) return o;
    int m;
    if (bw == R && bh == R) {                        // cv::resize to the same size: a copy
        m = dil(y, x);
        for (int c = 0; c < 3; ++c) o.c[c] = m == 255 ? 255 : img(y, x, c);
    } else {
        int sx, ax0, ax1, sy, ay0, ay1;
        resize_coef(x, bw, R, sx, ax0, ax1);
        resize_coef(y, bh, R, sy, ay0, ay1);
        const int sx1 = sx + 1 < bw ? sx + 1 : bw - 1, sy1 = sy + 1 < bh ? sy + 1 : bh - 1;
        const int d00 = dil(sy, sx), d01 = dil(sy, sx1), d10 = dil(sy1, sx), d11 = dil(sy1, sx1);
        m = resize_mix(d00 * ax0 + d01 * ax1, d10 * ax0 + d11 * ax1, ay0, ay1);
        for (int c = 0; c < 3; ++c) {
            const int p00 = d00 == 255 ? 255 : img(sy, sx, c), p01 = d01 == 255 ? 255 : img(sy, sx1, c);
            const int p10 = d10 == 255 ? 255 : img(sy1, sx, c), p11 = d11 == 255 ? 255 : img(sy1, sx1, c);
            o.c[c] = resize_mix(p00 * ax0 + p01 * ax1, p10 * ax0 + p11 * ax1, ay0, ay1);
        }
    }
    o.gray = (3735 * o.c[0] + 19235 * o.c[1] + 9798 * o.c[2] + 16384) >> 15;
    o.hole = m > 0;
    return o;
}
// what Canny reads of a pixel, in one int16: its gray value, or -1 in the hole
FUSG_HD int16_t gray_valid(const BoxPx& p) { return (int16_t)(p.hole ? -1 : p.gray); }

// step 6b along one axis at index l; at(k): the sample, 0 outside the image
template <class F>
FUSG_HD double gauss_px(F at, int l, const Gauss& g) {
    double t = at(l) * g.w[0];
    for (int d = g.radius; d >= 1; --d) t += (at(l - d) + at(l + d)) * g.w[d];
    return t;
}

// step 6d at (i, j); s(ii, jj): the smoothed image with the edge sample repeated (the caller clamps)
template <class F>
FUSG_HD void sobel_px(F s, int i, int j, double& gi, double& gj) {
    const double a0 = s(i + 1, j - 1) - s(i - 1, j - 1), a1 = s(i + 1, j) - s(i - 1, j), a2 = s(i + 1, j + 1) - s(i - 1, j + 1);
    gi = a1 * 2.0 + (a0 + a2);
    const double b0 = s(i - 1, j + 1) - s(i - 1, j - 1), b1 = s(i, j + 1) - s(i, j - 1), b2 = s(i + 1, j + 1) - s(i + 1, j - 1);
    gj = b1 * 2.0 + (b0 + b2);
}
FUSG_HD double magnitude(double gi, double gj) { return __builtin_sqrt(gi * gi + gj * gj); }

// step 6f for a pixel with er & m > 0; mag(di, dj): the magnitude at (i + di, j + dj).  Sector: which of the four decided
// (the last one that applies), for the tests' bookkeeping.
FUSG_HD bool nms_side(double c1, double c2, double w, double m) { return c2 * w + c1 * (1.0 - w) <= m; }
template <class F>
FUSG_HD bool nms_px(double gi, double gj, double m, F mag, int* sector = nullptr) {
    const double ai = gi < 0.0 ? -gi : gi, aj = gj < 0.0 ? -gj : gj;
    const bool same = (gi >= 0.0 && gj >= 0.0) || (gi <= 0.0 && gj <= 0.0);
    const bool opp = (gi <= 0.0 && gj >= 0.0) || (gi >= 0.0 && gj <= 0.0);
    bool lm = false;
    int sec = 0;
    if (same && ai >= aj) {
        const double w = aj / ai;
        lm = nms_side(mag(1, 0), mag(1, 1), w, m) && nms_side(mag(-1, 0), mag(-1, -1), w, m);
        sec = 1;
    }
    if (same && ai <= aj) {
        const double w = ai / aj;
        lm = nms_side(mag(0, 1), mag(1, 1), w, m) && nms_side(mag(0, -1), mag(-1, -1), w, m);
        sec = 2;
    }
    if (opp && ai <= aj) {
        const double w = ai / aj;
        lm = nms_side(mag(0, 1), mag(-1, 1), w, m) && nms_side(mag(0, -1), mag(1, -1), w, m);
        sec = 3;
    }
    if (opp && ai >= aj) {
        const double w = aj / ai;
        lm = nms_side(mag(-1, 0), mag(-1, 1), w, m) && nms_side(mag(1, 0), mag(1, -1), w, m);
        sec = 4;
    }
    if (sector) *sector = sec;
    return lm;
}
// step 6g: 0 = nothing, 1 = low only, 2 = low and high
FUSG_HD int threshold_code(bool lm, double m) { return lm && m >= LOW_T ? (m >= HIGH_T ? 2 : 1) : 0; }

// step 6h on bitmaps: bit b of word (y, w) is pixel (y, 64 w + b).  One round replaces a word of the kept set by its low
// run(s) that touch a kept pixel of the 3 x 3 neighbourhood; the kept set only grows and is bounded by low, so rounds
// repeated until no word changes end at the unique reachability set, whatever the order the words are visited in.
FUSG_HD uint64_t hdilate(uint64_t k, uint64_t left, uint64_t right) { return k | (k << 1) | (k >> 1) | (left >> 63) | (right << 63); }
FUSG_HD uint64_t fill_word(uint64_t s, uint64_t l) {                       // the bits of l connected to s (a subset of l) within the word
    uint64_t g = s, p = l;
    for (int sh = 1; sh < 64; sh <<= 1) { g |= p & (g << sh); p &= p << sh; }
    p = l;
    for (int sh = 1; sh < 64; sh <<= 1) { g |= p & (g >> sh); p &= p >> sh; }
    return g;
}
// kept(yy, ww): the kept word, 0 outside the image
template <class F>
FUSG_HD uint64_t hysteresis_word(F kept, uint64_t low, int y, int w) {
    uint64_t d = 0;
    for (int dy = -1; dy <= 1; ++dy) d |= hdilate(kept(y + dy, w), kept(y + dy, w - 1), kept(y + dy, w + 1));
    return fill_word(d & low, low);
}

// scratch: per vehicle the dilated box (uint8, row pitch max_box_w), gray / valid (int16 R x R), the smoothed image
// (double R x R) and the low / high bitmaps (2 x R x WPR words)
struct Scratch { long dil_v, off_gv, off_s, off_bits, total; };
FUSG_HD Scratch scratch_layout(long V, long max_h, long max_w) {
    Scratch s;
    s.dil_v = (max_h * max_w + 15) / 16 * 16;
    s.off_gv = V * s.dil_v;
    s.off_s = s.off_gv + V * (long)R * R * 2;
    s.off_bits = s.off_s + V * (long)R * R * 8;
    s.total = s.off_bits + V * 2L * R * WPR * 8;
    return s;
}

}  // namespace ii
}  // namespace fusg
