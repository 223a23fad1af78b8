// The Gram matrix of an activation and the per-row L1 distance of two, for host and device: the rules fusg_gram_f32 and
// fusg_abs_diff_rows_f32 (perceptual.hip) share with their host twins.
//
// Gram.  out[b][i][j] = (sum over the H W pixels p of x[b, i, p] x[b, j, p]) / (H W C) - EdgeConnect's StyleLoss.compute_gram.
// The contraction runs over PIXELS (every other kernel of the library contracts over channels and taps):
//   tiles    channels are cut into super tiles of ST = 64; one workgroup owns one pair (I, J), I <= J, of them and four
//            32 x 32 sub-tiles of the pair's 64 x 64 block, one per wave (on a diagonal pair the sub-tile below the diagonal
//            is not computed: its mirror is)
//   chunks   the pixels are cut into chunks of gram_chunk(C, HW) pixels - a function of C and HW only, so that a row's sums
//            do not depend on the batch it is in: about WG_TARGET workgroups per image, never fewer than MIN_CHUNK pixels
//            (below that the second launch's reads outweigh the first's), a multiple of the staged block of PB pixels
//   sums     inside a chunk an entry is ONE fp32 fmaf chain in pixel order, starting from +0 (v_mfma_f32_32x32x2_f32 is bit
//            for bit that chain, two pixels per instruction); pixels past the image and channels past C are staged as zeros,
//            and fmaf(0, 0, acc) = acc.  The chunk partials are added in ascending chunk order in float64, divided by
//            H W C and rounded once to fp32; entry (i, j), i <= j, is written to both triangles.
// Error of an entry against exact arithmetic: (gamma_n + u) S / (H W C) plus the float64 sums' 2^-53 terms, u = 2^-24,
// n = gram_chunk, gamma_n = n u / (1 - n u), S = sum_p |x_i x_j|.
//
// L1.  out[r] = sum over row r of |(double)a - (double)b|, elements in the order (y, x, c), c fastest.  G = abs_groups(n)
// workgroups of 256 per row (a function of the row's element count n only); thread t of group g adds elements
// g * 256 + t, + G * 256, ... in order; the 64 lanes of a wave by the halving tree, the four waves in order; then lane l of
// one wave per row adds groups l, l + 64, ... and the same tree.
#pragma once
#include <math.h>
#include <stdint.h>
#include "resize.h"                                               // FUSG_HD

namespace fusg {
namespace pc {

constexpr int ST = 64, SUB = 32, PB = 32, MIN_CHUNK = 128, WG_TARGET = 64, LANES = 64, WG = 256;
constexpr int MAX_C = 1024, MAX_HW = 1 << 24, MAX_B = 1 << 16;
constexpr int ABS_PER_GROUP = 4096, ABS_MAX_GROUPS = 256;

FUSG_HD int tiles(int C) { return (C + ST - 1) / ST; }
FUSG_HD int pairs(int T) { return T * (T + 1) / 2; }
// index of the pair (I, J), I <= J < T, in the order (0, 0), (0, 1), ..., (0, T - 1), (1, 1), ...
FUSG_HD int pair_index(int I, int J, int T) { return I * T - I * (I - 1) / 2 + (J - I); }

FUSG_HD int gram_chunk(int C, long HW) {
    const int np = pairs(tiles(C));
    const long want = (WG_TARGET + np - 1) / np;                  // chunks per image that would give WG_TARGET workgroups
    long k = (HW + want - 1) / want;
    if (k < MIN_CHUNK) k = MIN_CHUNK;
    return (int)((k + PB - 1) / PB * PB);
}
FUSG_HD int gram_chunks(int C, long HW) { const long k = gram_chunk(C, HW); return (int)((HW + k - 1) / k); }
// floats of chunk partials per image: [chunk][pair][ST][ST]
FUSG_HD long gram_partials(int C, long HW) { return (long)gram_chunks(C, HW) * pairs(tiles(C)) * ST * ST; }

// an entry from the float64 sum of its chunk partials: the one rounding to fp32
FUSG_HD float gram_entry(double s, int C, long HW) { return (float)(s / ((double)HW * (double)C)); }

FUSG_HD int abs_groups(long n) {
    const long want = (n + ABS_PER_GROUP - 1) / ABS_PER_GROUP;
    return (int)(want < 1 ? 1 : (want > ABS_MAX_GROUPS ? ABS_MAX_GROUPS : want));
}

// lane 0's value of the halving tree over 64 lanes (host form; v is overwritten)
inline double tree64(double* v) {
    for (int off = LANES / 2; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] += v[l + off];
    return v[0];
}

}  // namespace pc
}  // namespace fusg
