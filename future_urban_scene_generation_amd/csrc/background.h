// A video's background frame from its own frames, for host and device: the arithmetic fusg_background_median_u8
// (background.hip) and its host twin share.  The definition:
//   inputs     T frames, dense uint8 [H, W, 3]; per frame t a list of int32 boxes (x0, y0, x1, y1); margin >= 0; min_valid in 1..T
//   coverage   pixel (x, y) is covered in frame t if a box of t has x0 - margin <= x <= x1 + margin and y0 - margin <= y <= y1 + margin
//              (both ends inclusive).  Boxes may reach outside the frame; a box with x1 < x0 or y1 < y0 covers nothing.
//   samples    n(x, y) = the frames that do not cover the pixel.  n >= min_valid: those n frames; otherwise all T (the fallback)
//   bg         per channel the LOWER median of the m samples: the element of rank (m - 1) / 2 (0-based, integer division) in
//              ascending order.  Always a value that occurred; nothing is averaged or rounded.
//   count      n as uint8: a fallback pixel is one with count < min_valid
//
// The unit of work is one dword of the frame's 3 H W bytes: bytes 4 i .. 4 i + 3, which belong to pixel A = 4 i / 3 and to
// pixel A + 1 (`sel_a`: which of the four).  All four bytes are selected at once, on bit planes:
//   Planes<TB>   p[b][g], b < 8, g < TB / 8: bit s of byte j = 1 where sample 8 g + s has bit b of byte j CLEAR.  Inserting
//                a sample is 8 shift-and-or steps whatever the byte; the sample itself is not kept.
//   alive[g]     the same layout: the samples still in the race per byte, started from the pixels' validity masks - which is
//                all a covered frame costs
//   round b      (7 down to 0) z = alive & p[b]: the candidates with a 0 there; c0 = their number per byte (`pop_bytes`,
//                at most 64); the rank k < c0 keeps them and the bit is 0, else the bit is 1, k -= c0 and the others stay
// Eight rounds end at the byte of rank k among the valid samples: exact, no comparison of two samples anywhere.
// Every index into p, alive and z is a constant once the loops are unrolled (TB is a template parameter: 8, 16, 32 or 64, the
// frames past T never valid), so a lane holds them in registers.
#pragma once
#include <stdint.h>
#include "workgroup.h"

namespace fusg {
namespace bg {

using wg::MAX_DIM;
constexpr int MAX_T = 64, MAX_BOXES = 64, MAX_MARGIN = 32767;
constexpr uint32_t ONES = 0x01010101u;

FUSG_HD int bucket(int T) { return T <= 8 ? 8 : (T <= 16 ? 16 : (T <= 32 ? 32 : 64)); }

// a box grown by the margin and cut to the frame; false: it covers no pixel of the frame
struct Rect { int16_t x0, y0, x1, y1; };
FUSG_HD bool grow(const int32_t* b, int margin, int H, int W, Rect& r) {
    if (b[2] < b[0] || b[3] < b[1]) return false;
    const long x0 = (long)b[0] - margin, y0 = (long)b[1] - margin, x1 = (long)b[2] + margin, y1 = (long)b[3] + margin;
    if (x1 < 0 || y1 < 0 || x0 > W - 1 || y0 > H - 1) return false;
    r.x0 = (int16_t)(x0 < 0 ? 0 : x0);
    r.y0 = (int16_t)(y0 < 0 ? 0 : y0);
    r.x1 = (int16_t)(x1 > W - 1 ? W - 1 : x1);
    r.y1 = (int16_t)(y1 > H - 1 ? H - 1 : y1);
    return true;
}
FUSG_HD bool inside(const Rect& r, int x, int y) { return x >= r.x0 && x <= r.x1 && y >= r.y0 && y <= r.y1; }
FUSG_HD bool meets(const Rect& r, const Rect& q) { return r.x0 <= q.x1 && r.x1 >= q.x0 && r.y0 <= q.y1 && r.y1 >= q.y0; }

// the pixels of the bytes [b0, b1) of a frame (0 <= b0 < b1 <= 3 H W) lie in this rectangle
FUSG_HD Rect bytes_rect(long b0, long b1, int W) {
    const int p0 = (int)(b0 / 3), p1 = (int)((b1 - 1) / 3), ya = p0 / W, yb = p1 / W;
    Rect r;
    r.y0 = (int16_t)ya;
    r.y1 = (int16_t)yb;
    r.x0 = (int16_t)(ya == yb ? p0 % W : 0);
    r.x1 = (int16_t)(ya == yb ? p1 % W : W - 1);
    return r;
}

// the dword at byte b: 0x01 in the bytes (byte 0 = the lowest address) of pixel b / 3, the others are pixel b / 3 + 1's
FUSG_HD uint32_t sel_a(long b) {
    const int r = (int)(b % 3);
    return r == 0 ? 0x00010101u : (r == 1 ? 0x00000101u : 0x00000001u);
}

// which frames a pixel samples, and what it reports
struct Pick { uint64_t mask; int n; };
FUSG_HD Pick pick(uint64_t covered, int T, int min_valid) {
    const uint64_t all = T >= 64 ? ~0ull : ((1ull << T) - 1ull);
    const uint64_t free_ = ~covered & all;
    Pick p;
    p.n = __builtin_popcountll(free_);
    p.mask = p.n >= min_valid ? free_ : all;
    return p;
}

template <int TB>
struct Planes { uint32_t p[8][TB / 8]; };

FUSG_HD uint32_t pop_bytes(uint32_t x) {                           // the number of set bits of every byte
    x = x - ((x >> 1) & 0x55555555u);
    x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
    return (x + (x >> 4)) & 0x0f0f0f0fu;
}

// The dword of lower medians.  load(t): the dword of frame t, t < 8 ceil(T / 8) (a frame past T is read, never counted);
// ma, mb: the sample masks of pixel A and of pixel A + 1 (mb = 0 where that pixel does not exist: its bytes come out as 0).
template <int TB, class Load>
FUSG_HD uint32_t median4(int T, uint64_t ma, uint64_t mb, uint32_t sa, Load load) {
    constexpr int G = TB / 8;
    const uint32_t sb = ONES ^ sa;
    Planes<TB> P;
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int b = 0; b < 8; ++b) P.p[b][g] = 0u;
        if (g * 8 < T) {
            uint32_t v[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) v[s] = ~load(g * 8 + s);
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int b = 0; b < 8; ++b) P.p[b][g] |= ((v[s] >> b) & ONES) << s;
        }
    }
    uint32_t alive[G];
#pragma unroll
    for (int g = 0; g < G; ++g) alive[g] = (uint32_t)((ma >> (8 * g)) & 0xffull) * sa + (uint32_t)((mb >> (8 * g)) & 0xffull) * sb;
    const int na = __builtin_popcountll(ma), nb = __builtin_popcountll(mb);
    uint32_t k = (uint32_t)(na > 0 ? (na - 1) >> 1 : 0) * sa + (uint32_t)(nb > 0 ? (nb - 1) >> 1 : 0) * sb;
    uint32_t res = 0u;
#pragma unroll
    for (int b = 7; b >= 0; --b) {
        uint32_t z[G], c0 = 0u;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            z[g] = alive[g] & P.p[b][g];
            c0 += pop_bytes(z[g]);
        }
        const uint32_t ge = (((k | 0x80808080u) - c0) >> 7) & ONES;   // per byte: k >= c0 (both at most 64: no borrow between bytes)
        const uint32_t m = (ge << 8) - ge;                            // 0xff there
        res |= ge << b;
        k -= c0 & m;
#pragma unroll
        for (int g = 0; g < G; ++g) alive[g] = (z[g] & ~m) | ((alive[g] ^ z[g]) & m);
    }
    return res;
}

}  // namespace bg
}  // namespace fusg
