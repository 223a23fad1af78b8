// Border correction of nn.Upsample(2) -> ReflectionPad2d(2) -> 5x5 conv after the phase-form launch.
//
// u = up2(f(x)), R = u reflect-padded by 2, C = u replicate-padded by 2.  Nearest upsampling duplicates rows and columns, so
// R and C agree everywhere but on the outermost frame of the padded image, where D = R - C is a difference of two low-res
// pixels: f(x[1, j]) - f(x[0, j]) on the top frame row, f(x[h-2, j]) - f(x[h-1, j]) on the bottom one, the same along x on the
// sides, f(x[1, 1]) - f(x[0, 0]) and its mirrors in the frame corners.  The phase-form launch equals conv5x5(C) on every pixel,
// hence  conv5x5(R) = phase_form + conv5x5(D),  and conv5x5(D) is non-zero only on the outermost ring of output pixels and
// uses only the taps that land on the frame (5 of the 25 on an edge pixel, 9 on a corner pixel).
//
// One-dimensional form, per side: a line of L output pixels (L = 2w on the top / bottom side, 2h on the left / right one),
//   delta[p][co] = sum_{t = 0..4} sum_ci W_side[t][ci][co] * E[p + t - 2][ci],        p = 0 .. L-1,
//   E[P] = f(x[a1, j]) - f(x[a0, j]),  j = clamp(P, 0, L-1) >> 1                      P = -1 .. L,
//   E[-2] = f(x[a1, 1]) - f(x[a0, 0]),  E[L+1] = f(x[a1, l-2]) - f(x[a0, l-1])        the frame corners, rows pass only
// with (a1, a0) = (1, 0) on the top / left side and (l'-2, l'-1) on the bottom / right one, W_top[t] = w[ky = 0][kx = t],
// W_bottom[t] = w[4][t], W_left[t] = w[t][0], W_right[t] = w[t][4].  The columns pass takes E[-2] = E[L+1] = 0: a corner
// pixel gets its five row taps (the frame corner among them) from the rows pass and its four remaining column taps from the
// columns pass, which is issued after it on the same stream.
//
// Edge weights (pack.pack_conv_up2_edge): fp32, [side 4][tap 5][Cin/16][Cout/16][lane 64][4]; the lane (n = l & 15, g = l >> 4)
// holds w[co = 16 ct + n][ci = 16 c16 + 4 g + e], e = 0..3: the B operand of the four v_mfma_f32_16x16x4_f32 of a 16-channel
// group, one 16-byte load (instruction e contracts channels {16 c16 + 4 g + e}, the halo kernel's MODE 2 order).
#pragma once
#include "common.h"

namespace fusg {

constexpr int UP2E_CH = 32;                 // channels staged per chunk
constexpr int UP2E_PITCH = UP2E_CH + 4;     // floats per staged frame element (16-byte rows, bank-spread)

struct Up2EdgeK {
    const float* src;           // low-res source, NHWC-physical
    long ssn, ssh, ssw;
    int h, w, Cin, Cout;
    int pre_relu_affine;        // 0: f = identity; 1: f(v) = max(fma(v, scale, shift), 0)
    const float* pre_scale;
    const float* pre_shift;
    long pre_bstride;
    const float* wedge;
    float* dst;                 // [B, Cout, 2h, 2w] NHWC-physical, updated in place
    long dsn, dsh, dsw;
    double* delta;              // optional [B][n_entries][2] = (sum of delta, sum of delta * (2 old + delta)) per workgroup
    int n_entries, entry0;      // entries per image; first entry of this pass
    int axis;                   // 0: rows pass (top, bottom), 1: columns pass (left, right)
    int nseg;                   // segments per side
};

}  // namespace fusg
