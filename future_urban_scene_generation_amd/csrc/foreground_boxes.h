// Vehicle boxes from the estimated background, for host and device: the arithmetic fusg_foreground_boxes_u8
// (foreground_boxes.hip) and its host twin share.  Integer and bitwise from end to end.  The definition, per frame f of T, with
// the call's thr, cell, min_count, open_r, close_r, min_area, min_w, min_h, K and the half-open pixel rectangle roi = (rx0, ry0,
// rx1, ry1):
//   P(y, x)   fg::over(frame, background, y W + x, thr) - max over the three channels of |frame - background| > thr, strictly, the
//             masks' predicate (foreground.h) - and (x, y) inside roi
//   grid      gh = ceil(H / cell), gw = ceil(W / cell); cell (i, j) covers the rows [i cell, min(H, (i + 1) cell)) and the
//             columns likewise: edge cells are partial and count only their own pixels.  cnt[i, j] = its P pixels; ext[i, j] =
//             (min x, max x, min y, max y) of them as offsets inside the cell, meaningless when cnt = 0
//   G0        cnt >= min_count
//   G1        opening of G0 by the (2 open_r + 1)^2 square, outside the grid = 0 for both halves
//   G2        closing of G1 by the (2 close_r + 1)^2 square: dilation with outside = 0, then erosion with outside = 1 - the
//             masks' rule: a vehicle cut by the frame edge is not eaten back from it.  A radius of 0 is the identity
//   components of G2 are 4-connected, ordered by their first cell in raster order (smallest i, then smallest j).  Only the
//             first MAX_COMPONENTS are examined; if G2 has more, the frame's flag TRUNCATED is set and the rest are ignored
//   per examined component: n_cells; area = the sum of cnt over its cells (a cell the closing added brings what cnt it has);
//             its box (x0, y0, x1, y1), half-open and pixel-tight, over its cells with cnt > 0: x0 = min(j cell + min x),
//             x1 = max(j cell + max x) + 1, likewise y.  KEPT if area >= min_area, x1 - x0 >= min_w and y1 - y0 >= min_h
//             (min_area >= 1, so a component without a P pixel is never kept and its box is never formed)
//   boxes[f][k], box_stats[f][k] = (area, n_cells) for the first K kept components in order; the rows from min(n_kept, K) on
//             are zeros: both tables are written whole.  stats[f] = (n_kept, n_examined, n_P = the sum of cnt over the frame,
//             flags: 1 OVERFLOW n_kept > K, 2 TRUNCATED)
//
// Two passes.  The CELL pass reads the images once and leaves one 32-bit record per cell (pack below: cnt in 9 bits, the four
// extents in 4 bits each; cell <= 16) in a scratch table [T][gh][gw] that it writes whole.  The LABEL pass works on that table
// alone: G0 as a bit plane (foreground.h's layout: one bit per cell, 32 per word, row stride words(gw), the bits past gw kept 0),
// the four fg::square passes A -> B -> A, and then, while plane A - what is left of G2 - has a bit: its first bit in raster
// order seeds plane B, a flood (fg::flood<true>: the seed word is stored filled) grows B inside A, the records of B's cells are
// reduced to (n_cells, area, extents), B is taken out of A and cleared, and the component is emitted or skipped.  TWO planes
// carry everything: the morphology's second plane is free again when the labelling starts.
// Why device and host agree bit for bit: the records and the morphology are pure functions of a cell's pixels and of a cell's
// neighbourhood; a flood ends at the cells of A that are 4-connected to the seed, whatever the order of the sweeps (foreground.h);
// the first remaining bit in raster order belongs to the component whose first cell it is, so the order of the components is
// that of the definition; and every total, minimum and maximum is an integer one, the same in any order.  No sweep count is
// reported.
//
// Where the planes live: in the LDS of the one workgroup that labels a frame, PLANES gh words(gw) words.  With what the
// reductions and votes take (LDS_STATIC) they must fit LDS_BUDGET = 64 KiB, else the call is refused with the advice to raise
// cell; 720 x 1280 at cell 4 needs 14.4 KB.
#pragma once
#include <stdint.h>
#include "foreground.h"

namespace fusg {
namespace fgb {

constexpr int MAX_COMPONENTS = 256, MAX_K = 64, MAX_CELL = 16;
constexpr int PLANES = 2, THREADS = 256;
constexpr long LDS_BUDGET = 64 * 1024, LDS_STATIC = 512;
constexpr int NONE = 0x7fffffff;                                  // "no bit": above every cell index (gh gw < 2^26)
enum { FLAG_OVERFLOW = 1, FLAG_TRUNCATED = 2 };

struct Params { int thr, cell, min_count, open_r, close_r, min_area, min_w, min_h, K, rx0, ry0, rx1, ry1; };

FUSG_HD int cells(int n, int cell) { return (n + cell - 1) / cell; }
FUSG_HD long plane_words(int gh, int gw) { return (long)gh * fg::words(gw); }
FUSG_HD long planes_bytes(int gh, int gw) { return PLANES * plane_words(gh, gw) * 4; }
FUSG_HD bool fits(int gh, int gw) { return planes_bytes(gh, gw) + LDS_STATIC <= LDS_BUDGET; }
FUSG_HD long scratch_words(int T, int gh, int gw) { return (long)T * gh * gw; }

FUSG_HD bool pix(const unsigned char* f, const unsigned char* g, int W, int x, int y, const Params& P) {
    return x >= P.rx0 && x < P.rx1 && y >= P.ry0 && y < P.ry1 && fg::over(f, g, (long)y * W + x, P.thr);
}

// a cell's record: cnt | min x << 9 | max x << 13 | min y << 17 | max y << 21; 0 for a cell without a P pixel
FUSG_HD int rec_cnt(uint32_t r) { return (int)(r & 511u); }
FUSG_HD int rec_minx(uint32_t r) { return (int)((r >> 9) & 15u); }
FUSG_HD int rec_maxx(uint32_t r) { return (int)((r >> 13) & 15u); }
FUSG_HD int rec_miny(uint32_t r) { return (int)((r >> 17) & 15u); }
FUSG_HD int rec_maxy(uint32_t r) { return (int)((r >> 21) & 15u); }

// one cell while its rows go by: row(field, r) takes the P bits of the cell's row r (bit x = column x of the cell), r rising
struct CellAcc {
    int cnt = 0, miny = 0, maxy = 0;
    uint32_t any = 0u;
    FUSG_HD void row(uint32_t field, int r) {
        if (field == 0u) return;
        if (any == 0u) miny = r;
        maxy = r;
        any |= field;
        cnt += fg::popc(field);
    }
    FUSG_HD uint32_t pack() const {
        if (any == 0u) return 0u;
        const uint32_t minx = (uint32_t)__builtin_ctz(any), maxx = 31u - (uint32_t)__builtin_clz(any);
        return (uint32_t)cnt | (minx << 9) | (maxx << 13) | ((uint32_t)miny << 17) | ((uint32_t)maxy << 21);
    }
};

// what a component's cells add up to; x1, y1 are the largest pixel + 1
struct Acc {
    int n_cells = 0, area = 0, x0 = NONE, y0 = NONE, x1 = 0, y1 = 0;
    FUSG_HD void cell(uint32_t r, int i, int j, int cell) {
        ++n_cells;
        if (r == 0u) return;
        area += rec_cnt(r);
        const int ax = j * cell + rec_minx(r), bx = j * cell + rec_maxx(r) + 1, ay = i * cell + rec_miny(r), by = i * cell + rec_maxy(r) + 1;
        x0 = ax < x0 ? ax : x0;
        y0 = ay < y0 ? ay : y0;
        x1 = bx > x1 ? bx : x1;
        y1 = by > y1 ? by : y1;
    }
};

// plane A = G0 from the frame's records; returns this member's share of the sum of cnt
template <class Ex>
FUSG_HD int grid0(Ex& ex, const uint32_t* rec, int gh, int gw, int min_count, uint32_t* A) {
    int np = 0;
    ex.plane(A, gh, gw, fg::words(gw), 0, [&](int i, int j) { return rec_cnt(rec[(long)i * gw + j]); },
             [&](int cnt) { return cnt >= min_count; }, [&](int cnt) { np += cnt; });
    return np;
}

// Ex: who runs it (workgroup.h), with total(acc): the members' Acc combined, in every member (barriers).
// Every branch around a barrier below is on a value that came out of one of these: the same in every member.
template <class Ex>
FUSG_HD void label_frame(Ex& ex, const uint32_t* rec, int gh, int gw, const Params& P, uint32_t* A, uint32_t* B, int32_t* boxes,
                         int32_t* box_stats, int32_t* stats) {
    const int nw = fg::words(gw), n = gh * nw, t = ex.tid(), T = ex.nth();
    const int n_p = ex.sum(grid0(ex, rec, gh, gw, P.min_count, A));
    fg::square(ex, A, B, gh, nw, gw, P.open_r, true, false);
    fg::square(ex, A, B, gh, nw, gw, P.open_r, false, false);
    fg::square(ex, A, B, gh, nw, gw, P.close_r, false, false);
    fg::square(ex, A, B, gh, nw, gw, P.close_r, true, true);
    for (int e = t; e < n; e += T) B[e] = 0u;
    ex.sync();
    int n_kept = 0, n_exam = 0, flags = 0;
    for (;;) {
        int first = NONE;
        for (int e = t; e < n; e += T)
            if (A[e] != 0u) { first = 32 * e + __builtin_ctz(A[e]); break; }
        first = ex.min(first);
        if (first == NONE) break;
        if (n_exam == MAX_COMPONENTS) { flags |= FLAG_TRUNCATED; break; }
        ++n_exam;
        if (t == 0) B[first >> 5] = fg::fill(1u << (first & 31), A[first >> 5]);
        ex.sync();
        fg::flood<true>(ex, B, gh, nw, [A, nw](int i, int k) { return A[i * nw + k]; });   // closed: the seed is stored filled
        Acc acc;
        for (int e = t; e < n; e += T) {
            uint32_t b = B[e];
            if (b == 0u) continue;
            A[e] &= ~b;
            B[e] = 0u;
            const int i = e / nw, j0 = 32 * (e - i * nw);
            while (b != 0u) {                                       // four cells a turn: their records are loaded before any is used
                int j[4];
                uint32_t r[4];
                for (int u = 0; u < 4; ++u) {
                    j[u] = b != 0u ? j0 + __builtin_ctz(b) : -1;
                    b &= b - 1u;
                    r[u] = j[u] >= 0 ? rec[(long)i * gw + j[u]] : 0u;
                }
                for (int u = 0; u < 4; ++u)
                    if (j[u] >= 0) acc.cell(r[u], i, j[u], P.cell);
            }
        }
        ex.total(acc);
        if (acc.area >= P.min_area && acc.x1 - acc.x0 >= P.min_w && acc.y1 - acc.y0 >= P.min_h) {
            if (n_kept < P.K && t == 0) {
                int32_t* b = boxes + 4 * n_kept;
                b[0] = acc.x0; b[1] = acc.y0; b[2] = acc.x1; b[3] = acc.y1;
                box_stats[2 * n_kept] = acc.area;
                box_stats[2 * n_kept + 1] = acc.n_cells;
            }
            ++n_kept;
        }
    }
    const int used = n_kept < P.K ? n_kept : P.K;
    for (int e = 4 * used + t; e < 4 * P.K; e += T) boxes[e] = 0;
    for (int e = 2 * used + t; e < 2 * P.K; e += T) box_stats[e] = 0;
    if (t == 0) {
        stats[0] = n_kept;
        stats[1] = n_exam;
        stats[2] = n_p;
        stats[3] = flags | (n_kept > P.K ? FLAG_OVERFLOW : 0);
    }
}

}  // namespace fgb
}  // namespace fusg
