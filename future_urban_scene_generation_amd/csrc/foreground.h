// A vehicle's removal mask from the estimated background, for host and device: the arithmetic fusg_foreground_masks_u8
// (foreground.hip) and its host twin share.  Integer and bitwise from end to end.  The definition, per box b with the half-open
// frame rectangle (x0, y0, x1, y1), w = x1 - x0, h = y1 - y0, and a core rectangle (cx0, cy0, cx1, cy1) in frame coordinates -
// the part of the box taken to be the vehicle for certain.  Pixels are local to the box:
//   F0      max over the three channels of |frame - background| > thr (the maximum, not the sum; strictly greater)
//   F1      opening of F0 by the (2 open_r + 1)^2 square: erosion, then dilation, outside the box = 0 for both (SciPy's
//           binary_opening default); open_r = 0: F1 = F0
//   F2      closing of F1 by the (2 close_r + 1)^2 square: dilation with outside = 0, then erosion with outside = 1 - a vehicle
//           cut by the box or frame edge is not eaten back from that edge (NOT SciPy's binary_closing default)
//   seed    F2 and the core, the core clipped to the box; an empty intersection is an empty seed
//   R       the pixels of F2 that are 4-connected to the seed inside F2 (binary_propagation(seed, mask=F2))
//   M       R plus every pixel outside R that is not 4-connected to the box border through pixels outside R
//           (binary_fill_holes(R)); a hole that opens to the border stays open
//   empty seed: M is empty, or with `fallback` the clipped core rectangle (the vehicle is still removed, as a block)
//   grow    M dilated by the (2 grow + 1)^2 square, cut at the box
//   mask[offs[b] + i w + j] = 255 where M, else 0;  stats[b] = { n_F0, n_seed, n_mask (of the grown M),
//           flags: 1 fallback taken, 2 the grown M touches the box border, 4 the box was refused }
// A box is refused - flagged, its mask bytes not written, never read - when it leaves the frame (x0 < 0, y0 < 0, x1 > W, y1 > H,
// x1 < x0, y1 < y0), exceeds the max_box bound of the call, or its h w bytes at offs[b] would leave the mask buffer.
//
// Layout: an image of the box is a bit plane, one bit per pixel, 32 per word, row stride words(w) words, bit j of word k = pixel
// 32 k + j; the bits past w in a row's last word are kept 0, and a pass that wants the outside to be 1 sets them as it loads.
// TWO planes, A and B, carry everything:
//   threshold -> A;  every square pass goes A -> B along the rows (shifts with carries from the two neighbouring words; radii
//   stay below 32) and B -> A across them (AND / OR of the rows i - r .. i + r);  seed -> B;  flood 1 grows B inside A;  the
//   border pixels outside R -> A (F2 is no longer needed: R is a part of it);  flood 2 grows A inside NOT B;  M = NOT A.
// A flood sweep is, per row: pull from the rows above and below, then fill along the row - an occluded (Kogge-Stone) fill inside
// a word and a carry across words, once in each direction.  Even rows first, then odd rows, so that no row is read while it is
// written; sweeps repeat until one changes nothing (a workgroup-wide vote).
// Why device and host agree bit for bit: a sweep only ever adds pixels of the mask that are connected to the seed, and a sweep
// that changes nothing has every connected neighbour in already; so the loop ends at the set of mask pixels 4-connected to the
// seed, and that set is unique.  The order in which rows are visited, and the number of sweeps, change the way there, never a bit
// of the result - which is also why no sweep count is reported.  Everything else is a pure function of the pixel's neighbourhood.
//
// Where the planes live: with cap = max_box_h * words(max_box_w), PLANES * cap * 4 bytes.  Up to LDS_BUDGET they are in LDS
// (gfx950 has 160 KiB per CU; 32 KiB per workgroup of 256 leaves room for five workgroups, and a 200 x 150 box needs 8.4 KiB);
// above it the same code runs on a scratch buffer of the caller's, PLANES * cap words per box.
#pragma once
#include <stdint.h>
#include "workgroup.h"

namespace fusg {
namespace fg {

using wg::MAX_DIM;
constexpr int MAX_THR = 254, MAX_OPEN = 3, MAX_CLOSE = 7, MAX_GROW = 15;
constexpr int PLANES = 2, THREADS = 256;
constexpr long LDS_BUDGET = 32 * 1024;
enum { FLAG_FALLBACK = 1, FLAG_BORDER = 2, FLAG_REFUSED = 4 };

struct Params { int thr, open_r, close_r, grow, fallback; };

// one accepted box: where it reads and writes, its extent, its core (local, clipped; empty when c1 <= c0)
struct Box {
    const unsigned char* frame;
    const unsigned char* bgd;
    unsigned char* mask;
    int32_t* stats;
    int W, x0, y0, w, h, cx0, cy0, cx1, cy1;
};

FUSG_HD int words(int w) { return (w + 31) >> 5; }
FUSG_HD long plane_words(int max_h, int max_w) { return (long)max_h * words(max_w); }
FUSG_HD long planes_bytes(int max_h, int max_w) { return PLANES * plane_words(max_h, max_w) * 4; }
FUSG_HD bool in_lds(int max_h, int max_w) { return planes_bytes(max_h, max_w) <= LDS_BUDGET; }

FUSG_HD bool accept(const int32_t* b, int H, int W, int max_h, int max_w, long off, long mask_len) {
    if (b[0] < 0 || b[1] < 0 || b[2] < b[0] || b[3] < b[1] || b[2] > W || b[3] > H) return false;
    const int w = b[2] - b[0], h = b[3] - b[1];
    if (w > max_w || h > max_h) return false;
    return off >= 0 && off <= mask_len && (long)h * w <= mask_len - off;
}

FUSG_HD int clampi(long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

FUSG_HD void set_core(Box& bx, const int32_t* c) {
    bx.cx0 = clampi((long)c[0] - bx.x0, 0, bx.w);
    bx.cx1 = clampi((long)c[2] - bx.x0, 0, bx.w);
    bx.cy0 = clampi((long)c[1] - bx.y0, 0, bx.h);
    bx.cy1 = clampi((long)c[3] - bx.y0, 0, bx.h);
}

// the bits j of word k with a <= 32 k + j < b
FUSG_HD uint32_t span(int k, int a, int b) {
    int lo = a - 32 * k, hi = b - 32 * k;
    lo = lo < 0 ? 0 : lo;
    hi = hi > 32 ? 32 : hi;
    if (hi <= lo) return 0u;
    const uint32_t m = hi == 32 ? ~0u : ((1u << hi) - 1u);
    return m & ~((1u << lo) - 1u);
}

// word k of row i: the pixels of the box border in it
FUSG_HD uint32_t border(int i, int k, int h, int w) {
    return (i == 0 || i == h - 1) ? span(k, 0, w) : (span(k, 0, 1) | span(k, w - 1, w));
}

FUSG_HD bool over(const unsigned char* f, const unsigned char* g, long px, int thr) {
    const unsigned char* a = f + 3 * px;
    const unsigned char* b = g + 3 * px;
    int d0 = (int)a[0] - (int)b[0], d1 = (int)a[1] - (int)b[1], d2 = (int)a[2] - (int)b[2];
    d0 = d0 < 0 ? -d0 : d0;
    d1 = d1 < 0 ? -d1 : d1;
    d2 = d2 < 0 ? -d2 : d2;
    const int m = d0 > d1 ? (d0 > d2 ? d0 : d2) : (d1 > d2 ? d1 : d2);
    return m > thr;
}

FUSG_HD int popc(uint32_t x) { return __builtin_popcount(x); }

// word k of row i of a plane; outside the box, and in the bits past w, `one` decides
FUSG_HD uint32_t ld(const uint32_t* p, int i, int k, int h, int nw, int w, bool one) {
    if (i < 0 || i >= h || k < 0 || k >= nw) return one ? ~0u : 0u;
    uint32_t v = p[i * nw + k];
    if (one && k == nw - 1) v |= ~span(k, 0, w);
    return v;
}

// erosion (AND) or dilation (OR) of word (i, k) by the 2 r + 1 pixels along the row, r < 32
FUSG_HD uint32_t morph_h(const uint32_t* src, int i, int k, int h, int nw, int w, int r, bool erode, bool one) {
    const uint32_t L = ld(src, i, k - 1, h, nw, w, one), Cc = ld(src, i, k, h, nw, w, one), R = ld(src, i, k + 1, h, nw, w, one);
    uint32_t acc = Cc;
    for (int s = 1; s <= r; ++s) {
        const uint32_t up = (Cc << s) | (L >> (32 - s)), dn = (Cc >> s) | (R << (32 - s));
        acc = erode ? (acc & up & dn) : (acc | up | dn);
    }
    return acc & span(k, 0, w);
}

// the same across the rows i - r .. i + r (the bits past w are 0 in src and stay 0)
FUSG_HD uint32_t morph_v(const uint32_t* src, int i, int k, int h, int nw, int r, bool erode, bool one) {
    uint32_t acc = src[i * nw + k];
    for (int d = 1; d <= r; ++d) {
        for (int q = 0; q < 2; ++q) {
            const int y = q ? i + d : i - d;
            if (y >= 0 && y < h) {
                const uint32_t v = src[y * nw + k];
                acc = erode ? (acc & v) : (acc | v);
            } else if (erode && !one) {
                acc = 0u;
            }
        }
    }
    return acc;
}

// g (a part of m) grown along the word inside m, both ways: the occluded fill
FUSG_HD uint32_t fill(uint32_t g, uint32_t m) {
    uint32_t a = g, p = m;
    a |= p & (a << 1);  p &= p << 1;
    a |= p & (a << 2);  p &= p << 2;
    a |= p & (a << 4);  p &= p << 4;
    a |= p & (a << 8);  p &= p << 8;
    a |= p & (a << 16);
    uint32_t b = g;
    p = m;
    b |= p & (b >> 1);  p &= p >> 1;
    b |= p & (b >> 2);  p &= p >> 2;
    b |= p & (b >> 4);  p &= p >> 4;
    b |= p & (b >> 8);  p &= p >> 8;
    b |= p & (b >> 16);
    return a | b;
}

// one row of a flood sweep: pull from the rows above and below, fill along the row; true if the row changed.
// mask(i, k): word k of row i of what the flood may enter; it must not change during the flood.
// CLOSED is the caller's word that every state word is closed under fill inside its mask word when the flood starts (a sweep
// keeps it so: it only ever stores fill(g, m)).  Then a word whose neighbours bring nothing new (g & m == old) would be filled
// to itself, and the fill is made only behind the test, at the rim of what has been reached: the same bits, sweep for sweep.
// With a seed that is NOT closed, CLOSED = true ends the flood at the seed - wrong, and silently fast.
template <bool CLOSED, class Mask>
FUSG_HD bool flood_row(uint32_t* st, int i, int h, int nw, Mask mask) {
    uint32_t* row = st + i * nw;
    bool changed = false;
    uint32_t carry = 0u;
    for (int k = 0; k < nw; ++k) {
        const uint32_t m = mask(i, k), old = row[k];
        uint32_t g = old | carry;
        if (i > 0) g |= st[(i - 1) * nw + k];
        if (i + 1 < h) g |= st[(i + 1) * nw + k];
        g &= m;
        if (!CLOSED) g = fill(g, m);
        if (g != old) { if (CLOSED) g = fill(g, m); row[k] = g; changed = true; }
        carry = g >> 31;
    }
    carry = 0u;
    for (int k = nw - 1; k >= 0; --k) {
        const uint32_t m = mask(i, k), old = row[k];
        uint32_t g = (old | carry) & m;
        if (!CLOSED) g = fill(g, m);
        if (g != old) { if (CLOSED) g = fill(g, m); row[k] = g; changed = true; }
        carry = (g & 1u) << 31;
    }
    return changed;
}

// Ex: who runs it (workgroup.h).
template <class Ex>
FUSG_HD void square(Ex& ex, uint32_t* A, uint32_t* B, int h, int nw, int w, int r, bool erode, bool one) {
    if (r <= 0) return;
    const int n = h * nw;
    for (int e = ex.tid(); e < n; e += ex.nth()) {
        const int i = e / nw;
        B[e] = morph_h(A, i, e - i * nw, h, nw, w, r, erode, one);
    }
    ex.sync();
    for (int e = ex.tid(); e < n; e += ex.nth()) {
        const int i = e / nw;
        A[e] = morph_v(B, i, e - i * nw, h, nw, r, erode, one);
    }
    ex.sync();
}

template <bool CLOSED, class Ex, class Mask>
FUSG_HD void flood(Ex& ex, uint32_t* st, int h, int nw, Mask mask) {
    bool changed;
    do {
        changed = false;
        for (int i = 2 * ex.tid(); i < h; i += 2 * ex.nth()) changed |= flood_row<CLOSED>(st, i, h, nw, mask);
        ex.sync();
        for (int i = 2 * ex.tid() + 1; i < h; i += 2 * ex.nth()) changed |= flood_row<CLOSED>(st, i, h, nw, mask);
    } while (ex.any(changed));
}

// plane A = F0: the only pass that touches the images
template <class Ex>
FUSG_HD void threshold(Ex& ex, const Box& bx, int thr, uint32_t* A) {
    ex.plane(A, bx.h, bx.w, words(bx.w), false,
             [&](int i, int j) { return over(bx.frame, bx.bgd, (long)(bx.y0 + i) * bx.W + bx.x0 + j, thr); },
             [](bool p) { return p; }, [](bool) {});
}

template <class Ex>
FUSG_HD void run_box(Ex& ex, const Box& bx, const Params& P, uint32_t* A, uint32_t* B) {
    const int h = bx.h, w = bx.w, nw = words(w), n = h * nw, t = ex.tid(), T = ex.nth();
    int flags = 0;
    threshold(ex, bx, P.thr, A);
    int cnt = 0;
    for (int e = t; e < n; e += T) cnt += popc(A[e]);
    const int n_f0 = ex.sum(cnt);
    square(ex, A, B, h, nw, w, P.open_r, true, false);
    square(ex, A, B, h, nw, w, P.open_r, false, false);
    square(ex, A, B, h, nw, w, P.close_r, false, false);
    square(ex, A, B, h, nw, w, P.close_r, true, true);
    cnt = 0;
    for (int e = t; e < n; e += T) {
        const int i = e / nw;
        const uint32_t s = (i >= bx.cy0 && i < bx.cy1) ? (A[e] & span(e - i * nw, bx.cx0, bx.cx1)) : 0u;
        B[e] = s;
        cnt += popc(s);
    }
    const int n_seed = ex.sum(cnt);
    if (n_seed > 0) {
        // neither seed is closed under fill: F2 and the core here, the border pixels outside R below
        flood<false>(ex, B, h, nw, [A, nw](int i, int k) { return A[i * nw + k]; });
        for (int e = t; e < n; e += T) {
            const int i = e / nw, k = e - i * nw;
            A[e] = ~B[e] & border(i, k, h, w);
        }
        ex.sync();
        flood<false>(ex, A, h, nw, [B, nw, w](int i, int k) { return ~B[i * nw + k] & span(k, 0, w); });
        for (int e = t; e < n; e += T) {
            const int i = e / nw;
            A[e] = ~A[e] & span(e - i * nw, 0, w);
        }
    } else {
        const bool fb = P.fallback != 0;
        flags |= fb ? FLAG_FALLBACK : 0;
        for (int e = t; e < n; e += T) {
            const int i = e / nw;
            A[e] = (fb && i >= bx.cy0 && i < bx.cy1) ? span(e - i * nw, bx.cx0, bx.cx1) : 0u;
        }
    }
    ex.sync();
    square(ex, A, B, h, nw, w, P.grow, false, false);
    cnt = 0;
    int edge = 0;
    for (int e = t; e < n; e += T) {
        const int i = e / nw;
        cnt += popc(A[e]);
        edge += (A[e] & border(i, e - i * nw, h, w)) != 0u;
    }
    const int n_mask = ex.sum(cnt);
    flags |= ex.sum(edge) > 0 ? FLAG_BORDER : 0;
    const long np = (long)h * w;
    for (long p = t; p < np; p += T) {
        const int i = (int)(p / w), j = (int)(p - (long)i * w);
        bx.mask[p] = ((A[i * nw + (j >> 5)] >> (j & 31)) & 1u) ? 255 : 0;
    }
    if (t == 0) {
        bx.stats[0] = n_f0;
        bx.stats[1] = n_seed;
        bx.stats[2] = n_mask;
        bx.stats[3] = flags;
    }
}

// the ranges the masks and the boxes share, on the host, in the words of both
inline int check_ranges(int H, int W, int thr, int open_r, int close_r, const char* what) {
    if (const int rc = wg::check_frame_size(H, W, what)) return rc;
    FUSG_CHECK(thr >= 0 && thr <= MAX_THR, "%s: thr = %d (0..%d)", what, thr, MAX_THR);
    FUSG_CHECK(open_r >= 0 && open_r <= MAX_OPEN, "%s: open_r = %d (0..%d)", what, open_r, MAX_OPEN);
    FUSG_CHECK(close_r >= 0 && close_r <= MAX_CLOSE, "%s: close_r = %d (0..%d)", what, close_r, MAX_CLOSE);
    return FUSG_OK;
}

}  // namespace fg
}  // namespace fusg
