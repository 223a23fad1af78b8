// Two VUnet Residuals and their two skip NiNs per launch (fusg_vunet_respair, include/fusg.h): the 32-channel shape-encoder
// levels at full and half resolution (vunet/models.py: shape_encoder_1 + shape_skip_1_b/c, shape_encoder_1_a + shape_skip_1_a_b/c),
// split-fp16 arithmetic of conv_kernel_h3.h:
//   x0 = entry ? NiN_in(elu(u)) + b_in : x
//   s0 = conv3x3_A(elu(x0)) + bA + x0        (zero padding 1)
//   s1 = conv3x3_B(elu(s0)) + bB + s0
//   kb = conv1x1_b(elu(s0)) + b_b,   kc = conv1x1_c(elu(s1)) + b_c
// written: s1, kb, kc.  x0 and s0 never reach memory: as five launches each is written once and read 2 - 3 times (3x3 halo,
// residual add, skip NiN), and every launch pays its own set-up and its own LDS detour on the way out.
//
// A workgroup owns an 8 x 16 patch of one image (conv_bneck.hip's scheme on the halo kernel's patch):
//   0. x0 on the patch + 2 ring (12 x 20 pixels), ELU'd and split to (hi, lo') -> LDS image X.  Entry form: the fp32 fmaf chain
//      of conv_pointwise_small, from u's <= 8 channels.  Pixels outside the image are ZERO (conv A's padding), not NiN(0) + bias.
//   1. conv A on the patch + 1 ring (10 x 18 = 180 pixels) as 12 GEMM column groups of 16 pixels: the 8 patch rows (the groups
//      conv B uses too, so a lane keeps the raw fp32 s0 of its patch pixels in registers for conv B's residual) and the 52
//      ring pixels in 4 groups.  Result + bias + x0, zero outside the image, ELU + split from the accumulators -> LDS image S.
//   2. conv B and NiN b from S (NiN b's operand is conv B's centre tap); s1 and kb leave as 16-byte stores; elu(s1) goes
//      through a wave-private corner of X (dead by now) into operand order for NiN c.
// The MFMA runs transposed as in conv_bneck.hip - weights (the `wfrag` copy, one 1 KiB wave load per fragment) as the A
// operand, pixels as B - so a lane ends up with 4 consecutive channels of one pixel: 8-byte LDS stores per fp16 half and
// 16-byte global stores, no transposition step.  Every wave computes all 32 channels of its pixels (3 of the 12 groups of
// conv A, 2 of the 8 of conv B), as a wave of the 32-column halo launch does.
//
// Bits: every accumulator sees the products of the unfused launches in their order - per tap ah wh, ah wl, al' (wh 2^-11),
// taps in order (TAPSPLIT false: the halo kernel with the M split over the waves, grids of more than 1024 workgroups), or, on the
// small grids where the router gives the 3x3 launches the K split over the waves (conv_kernel_halo.h, KS = 4), four partial
// sums over the taps w, w + 4, w + 8 added in wave order (TAPSPLIT true) - and the same epilogue arithmetic: fmaf(acc, wscale,
// bias) + residual.  s1, kb and kc are bit for bit what the five launches write (tests/test_gpu_vunet_respair.py).
// LDS: X 30 KiB + S 22.5 KiB (entry form: + 1 KiB of NiN weights) -> 2 workgroups per CU, 3 in the plain form (52.5 KiB, <= 168 VGPRs).
#include "conv_kernel_h3.h"

namespace fusg {

struct RespairK {
    const float* x; long xsn, xsh, xsw;                 // entry form: u
    float* s1; float* kb; float* kc;
    long s1n, s1h, s1w, kbn, kbh, kbw, kcn, kch, kcw;
    const float* w_in; const float* b_in; int cin, kpad_in;
    const _Float16* wA; const _Float16* wB; const _Float16* wb; const _Float16* wc;
    const float* bA; const float* bB; const float* bb; const float* bc;
    const float* sA; const float* sB; const float* sb; const float* sc;
    const float* zeros;
    int* status;
    int B, H, W, tiles_x, tiles_y;
};

constexpr int RP_XW = 20, RP_XPIX = 12 * 20;          // x0 image: patch + 2 ring
constexpr int RP_SW = 18, RP_SPIX = 10 * 18;          // s0 image: patch + 1 ring
constexpr size_t respair_lds(bool entry) { return (size_t)(RP_XPIX + RP_SPIX) * 2 * 32 * sizeof(_Float16) + (entry ? 8 * 32 * sizeof(float) : 0); }

struct RpFrag { h8 f[2][2]; };                         // [16-channel half][hi | lo] of one tap's 32 x 32 weights

__device__ __forceinline__ f32x4 rp_mfma(const h8 a, const h8 b, const f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// the halo kernel's slot swizzle: 16-byte slot g of image column hx lives at g ^ 2 ((hx >> 2) & 1)
__device__ __forceinline__ int rp_swz(int hx) { return ((hx >> 2) & 1) << 1; }

// conv_pointwise_small's chain for 4 output channels: ELU of the pixel's 8 (4) inputs, k order 0, 4, 1, 5, 2, 6, 3, 7, then
// fmaf(acc, 1, bias).  `two` false (at most 4 input channels): that kernel's k = 4 .. 7 steps are fmaf(0, 0, acc) with an acc
// that is never -0 (it starts at +0, and x + (+0) is never -0) - identities, left out here.
__device__ __forceinline__ f32x4 rp_nin(f32x4 xa, const float* pb, bool two, const f32x4 (&w)[8], const f32x4 bias) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) xa[c] = elu1(xa[c]);
    if (two) {                                           // (wave-uniform; the VUnet's stem has 3 channels)
        f32x4 xb = *(const f32x4*)pb;
#pragma unroll
        for (int c = 0; c < 4; ++c) xb[c] = elu1(xb[c]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(xb[e], w[4 + e][j], fmaf(xa[e], w[e][j], acc[j]));
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(xa[e], w[e][j], acc[j]);
    }
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaf(acc[j], 1.f, bias[j]);
    return v;
}

template <int C, bool ENTRY, bool TAPSPLIT>
__global__ __launch_bounds__(256, TAPSPLIT ? 1 : 2) void vunet_respair_h3(const RespairK k) {
    static_assert(C == 32, "one 32-channel chunk per pixel");
    constexpr int NP = TAPSPLIT ? 4 : 1;                // partial sums per accumulator
    extern __shared__ __attribute__((aligned(16))) _Float16 smem_h[];
    _Float16* Xh = smem_h;
    _Float16* Xl = Xh + RP_XPIX * 32;
    _Float16* Sh = Xl + RP_XPIX * 32;
    _Float16* Sl = Sh + RP_SPIX * 32;
    float* wl = (float*)(Sl + RP_SPIX * 32);           // entry form: NiN weights [8 input channels][32]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lp = lane & 15, lg = lane >> 4;
    const int tile = xcd_tile();
    const int tpi = k.tiles_x * k.tiles_y;
    const int b = tile / tpi, t2 = tile - b * tpi;
    const int ty = t2 / k.tiles_x, tx = t2 - ty * k.tiles_x;
    const int oy0 = ty * 8, ox0 = tx * 16;
    const float* ximg = k.x + (long)b * k.xsn;
    float amax = 0.f;
    const float ninf = -__builtin_inff();
    const bool two = ENTRY && k.cin > 4;                // u has a second 16-byte piece per pixel

    // The 18 taps' weights of conv A and conv B are one stream of 4 KiB fragments sets, fetched PF taps ahead of their use through a
    // ring of PF + 1 sets: a tap is 18 (12) MFMAs = 290 (190) cycles, an L2 round trip is two to three of those.  The first PF
    // are requested before x0 is staged.  (The tap-split form accumulates 4x the registers and keeps one set ahead: small grids.)
    constexpr int PF = TAPSPLIT ? 1 : 3, NR = PF + 1;
    RpFrag wf[NR];
    auto load_s = [&](int st) __attribute__((always_inline)) {
        const _Float16* w = (st < 9 ? k.wA : k.wB) + (((st < 9 ? st : st - 9) * 4) * 512 + lane * 8);
        RpFrag& F = wf[st % NR];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int hl = 0; hl < 2; ++hl) F.f[ct][hl] = *(const h8*)(w + (ct * 2 + hl) * 512);
    };

    // ------------------------------------------------------------------ 0. x0 on the patch + 2 ring -> X
    {
        const int kc = t & 7;
        f32x4 ra[8];
        const float* pb[8];                              // entry form with 5 - 8 input channels: the pixel's second piece
        unsigned inimg = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int pix = (t + 256 * j) >> 3;
            const int hy = pix / RP_XW, hx = pix - hy * RP_XW;
            const int iy = oy0 - 2 + hy, ix = ox0 - 2 + hx;
            const bool ok = pix < RP_XPIX && (unsigned)iy < (unsigned)k.H && (unsigned)ix < (unsigned)k.W;
            inimg |= (ok ? 1u : 0u) << j;
            const float* p = ximg + (long)iy * k.xsh + (long)ix * k.xsw;
            if constexpr (ENTRY) {
                ra[j] = *(const f32x4*)(ok ? p : k.zeros);
                pb[j] = (ok && two) ? p + 4 : k.zeros;
            } else {
                ra[j] = *(const f32x4*)(ok ? p + kc * 4 : k.zeros);
            }
        }
        if constexpr (!TAPSPLIT) {
#pragma unroll
            for (int st = 0; st < PF; ++st) load_s(st);
        }
        f32x4 w[8], bias = {0.f, 0.f, 0.f, 0.f};
        if constexpr (ENTRY) {
            const int c = t >> 5, n = t & 31;
            wl[t] = c < k.cin ? k.w_in[(long)n * k.kpad_in + c] : 0.f;
            __syncthreads();
#pragma unroll
            for (int c2 = 0; c2 < 8; ++c2) w[c2] = *(const f32x4*)(wl + c2 * 32 + kc * 4);
            bias = *(const f32x4*)(k.b_in + kc * 4);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int pix = (t + 256 * j) >> 3;
            const int hy = pix / RP_XW, hx = pix - hy * RP_XW;
            f32x4 v = ra[j];
            if constexpr (ENTRY) {
                v = rp_nin(ra[j], pb[j], two, w, bias);
                const bool ok = (inimg >> j) & 1u;
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = ok ? v[c] : 0.f;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = elu1(v[c]);
            h4 hi, lo;
            split4<false>(v, ninf, hi, lo, amax);
            if (pix < RP_XPIX) {
                const int o = pix * 32 + ((((kc >> 1) ^ rp_swz(hx)) << 3) | ((kc & 1) << 2));
                *(h4*)(Xh + o) = hi;
                *(h4*)(Xl + o) = lo;
            }
        }
    }

    // this lane's pixel in each of the wave's column groups, in S coordinates (S(sy, sx) = image (oy0 - 1 + sy, ox0 - 1 + sx)):
    // groups 0, 1 = patch rows 2 wave, 2 wave + 1; group 2 = ring pixels 16 wave + lp of 52 (top row, bottom row, left, right)
    int sy[3], sx[3];
    bool inS[3];                                         // a pixel of S at all (the last ring group has 12 idle lanes)
#pragma unroll
    for (int i = 0; i < 2; ++i) { sy[i] = 2 * wave + i + 1; sx[i] = lp + 1; inS[i] = true; }
    {
        const int q = wave * 16 + lp;
        inS[2] = q < 52;
        if (q < 18) { sy[2] = 0; sx[2] = q; }
        else if (q < 36) { sy[2] = 9; sx[2] = q - 18; }
        else if (q < 44) { sy[2] = q - 35; sx[2] = 0; }
        else if (q < 52) { sy[2] = q - 43; sx[2] = 17; }
        else { sy[2] = 0; sx[2] = 0; }
    }
    bool inimg3[3];
    long goff[3];                                        // element offset of the pixel inside an image of x (xs*) - valid when inimg3
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int iy = oy0 - 1 + sy[i], ix = ox0 - 1 + sx[i];
        inimg3[i] = inS[i] && (unsigned)iy < (unsigned)k.H && (unsigned)ix < (unsigned)k.W;
        goff[i] = (long)iy * k.xsh + (long)ix * k.xsw;
    }
    // conv A's residual x0 of those pixels: fetched now, used after the taps (entry form: the pixel's u, the chain is redone)
    f32x4 resA[3][2], ua[3];
    const float* pub[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float* p = ximg + goff[i];
        if constexpr (ENTRY) {
            ua[i] = *(const f32x4*)(inimg3[i] ? p : k.zeros);
            pub[i] = (inimg3[i] && two) ? p + 4 : k.zeros;
        } else {
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) resA[i][ct] = *(const f32x4*)(inimg3[i] ? p + ct * 16 + lg * 4 : k.zeros);
        }
    }

    auto load_w = [&](RpFrag& F, const _Float16* w, int tap) __attribute__((always_inline)) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int hl = 0; hl < 2; ++hl) F.f[ct][hl] = *(const h8*)(w + ((tap * 2 + ct) * 2 + hl) * 512 + lane * 8);
    };
    // the unfused launches' sum of the partial tiles, in wave order
    auto total = [&](const f32x4 (&a)[NP]) __attribute__((always_inline)) {
        f32x4 s = a[0];
#pragma unroll
        for (int q = 1; q < NP; ++q) s += a[q];
        return s;
    };

    // ------------------------------------------------------------------ 1. conv A: 3 column groups x 9 taps from X
    f32x4 accA[3][2][NP];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int q = 0; q < NP; ++q) accA[i][ct][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    int xbase[3][3];                                     // [group][kx]: the lane's fragment of X(sy, sx + kx) (tap row 0)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) xbase[i][kx] = (sy[i] * RP_XW + sx[i] + kx) * 32 + ((lg ^ rp_swz(sx[i] + kx)) << 3);
    if constexpr (TAPSPLIT) load_s(0);
    __syncthreads();                                     // X is complete
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        load_s(tap + PF);                                // (the last PF taps fetch conv B's first)
        const RpFrag& F = wf[tap % NR];
        const int ky = tap / 3, kx = tap - ky * 3;
        h8 xh[3], xl[3], bs[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            xh[i] = *(const h8*)(Xh + xbase[i][kx] + ky * RP_XW * 32);
            xl[i] = *(const h8*)(Xl + xbase[i][kx] + ky * RP_XW * 32);
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) bs[ct] = scale_m11(F.f[ct][0]);
#pragma unroll
        for (int term = 0; term < 3; ++term)
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
                    accA[i][ct][TAPSPLIT ? (tap & 3) : 0] = rp_mfma(term == 0 ? F.f[ct][0] : term == 1 ? F.f[ct][1] : bs[ct],
                                                                    term == 2 ? xl[i] : xh[i], accA[i][ct][TAPSPLIT ? (tap & 3) : 0]);
    }

    // s0 = fmaf(acc, wscale, bias) + x0, zero outside the image; raw for conv B's residual, ELU'd and split -> S
    f32x4 s0raw[2][2];
    {
        f32x4 w[8];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int n0 = ct * 16 + lg * 4;
            const f32x4 bias = *(const f32x4*)(k.bA + n0), wsc = *(const f32x4*)(k.sA + n0);
            f32x4 bin = {0.f, 0.f, 0.f, 0.f};
            if constexpr (ENTRY) {
#pragma unroll
                for (int c2 = 0; c2 < 8; ++c2) w[c2] = *(const f32x4*)(wl + c2 * 32 + n0);
                bin = *(const f32x4*)(k.b_in + n0);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                f32x4 r;
                if constexpr (ENTRY) {
                    r = rp_nin(ua[i], pub[i], two, w, bin);
                } else {
                    r = resA[i][ct];
                }
                const f32x4 a = total(accA[i][ct]);
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float y = fmaf(a[e], wsc[e], bias[e]) + r[e]; v[e] = inimg3[i] ? y : 0.f; }
                if (i < 2) s0raw[i][ct] = v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = elu1(v[e]);
                h4 hi, lo;
                split4<false>(v, ninf, hi, lo, amax);
                if (inS[i]) {
                    const int o = (sy[i] * RP_SW + sx[i]) * 32 + ((((ct << 1) | (lg >> 1)) ^ rp_swz(sx[i])) << 3) + ((lg & 1) << 2);
                    *(h4*)(Sh + o) = hi;
                    *(h4*)(Sl + o) = lo;
                }
            }
        }
    }
    __syncthreads();                                     // S is complete; X is dead
    RpFrag wfb, wfc;                                     // NiN b (used at the centre tap) and NiN c (after the taps)
    load_w(wfb, k.wb, 0);
    load_w(wfc, k.wc, 0);

    // ------------------------------------------------------------------ 2. conv B (9 taps) and NiN b (the centre tap's operand) from S
    f32x4 accB[2][2][NP], accb[2][2], accc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
            for (int q = 0; q < NP; ++q) accB[i][ct][q] = f32x4{0.f, 0.f, 0.f, 0.f};
            accb[i][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
            accc[i][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    int sbase[3];                                        // [kx]: the lane's fragment of S(2 wave, lp + kx); patch row i: + i rows
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) sbase[kx] = (2 * wave * RP_SW + lp + kx) * 32 + ((lg ^ rp_swz(lp + kx)) << 3);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        if (tap + PF < 9) load_s(9 + tap + PF);
        const RpFrag& F = wf[(9 + tap) % NR];
        const int ky = tap / 3, kx = tap - ky * 3;
        h8 xh[2], xl[2], bs[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            xh[i] = *(const h8*)(Sh + sbase[kx] + (ky + i) * RP_SW * 32);
            xl[i] = *(const h8*)(Sl + sbase[kx] + (ky + i) * RP_SW * 32);
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) bs[ct] = scale_m11(F.f[ct][0]);
#pragma unroll
        for (int term = 0; term < 3; ++term)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
                    accB[i][ct][TAPSPLIT ? (tap & 3) : 0] = rp_mfma(term == 0 ? F.f[ct][0] : term == 1 ? F.f[ct][1] : bs[ct],
                                                                    term == 2 ? xl[i] : xh[i], accB[i][ct][TAPSPLIT ? (tap & 3) : 0]);
        if (tap == 4) {                                   // elu(s0) of the patch pixel itself: NiN b
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) bs[ct] = scale_m11(wfb.f[ct][0]);
#pragma unroll
            for (int term = 0; term < 3; ++term)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
                        accb[i][ct] = rp_mfma(term == 0 ? wfb.f[ct][0] : term == 1 ? wfb.f[ct][1] : bs[ct], term == 2 ? xl[i] : xh[i], accb[i][ct]);
        }
    }

    // kb and s1 leave; elu(s1), split, goes through this wave's 32 pixels of X into operand order
    _Float16* Th = Xh + wave * 32 * 32;
    _Float16* Tl = Xl + wave * 32 * 32;
    const int oxl = ox0 + lp;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int n0 = ct * 16 + lg * 4;
        const f32x4 biasB = *(const f32x4*)(k.bB + n0), wscB = *(const f32x4*)(k.sB + n0);
        const f32x4 biasb = *(const f32x4*)(k.bb + n0), wscb = *(const f32x4*)(k.sb + n0);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int oy = oy0 + 2 * wave + i;
            f32x4 vb, v;
#pragma unroll
            for (int e = 0; e < 4; ++e) vb[e] = fmaf(accb[i][ct][e], wscb[e], biasb[e]);
            *(f32x4*)(k.kb + (long)b * k.kbn + (long)oy * k.kbh + (long)oxl * k.kbw + n0) = vb;
            const f32x4 a = total(accB[i][ct]);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaf(a[e], wscB[e], biasB[e]) + s0raw[i][ct][e];
            *(f32x4*)(k.s1 + (long)b * k.s1n + (long)oy * k.s1h + (long)oxl * k.s1w + n0) = v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = elu1(v[e]);
            h4 hi, lo;
            split4<false>(v, ninf, hi, lo, amax);
            const int o = (i * 16 + lp) * 32 + ((((ct << 1) | (lg >> 1)) ^ rp_swz(lp)) << 3) + ((lg & 1) << 2);
            *(h4*)(Th + o) = hi;
            *(h4*)(Tl + o) = lo;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    {
        h8 xh[2], xl[2], bs[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int o = (i * 16 + lp) * 32 + ((lg ^ rp_swz(lp)) << 3);
            xh[i] = *(const h8*)(Th + o);
            xl[i] = *(const h8*)(Tl + o);
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) bs[ct] = scale_m11(wfc.f[ct][0]);
#pragma unroll
        for (int term = 0; term < 3; ++term)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
                    accc[i][ct] = rp_mfma(term == 0 ? wfc.f[ct][0] : term == 1 ? wfc.f[ct][1] : bs[ct], term == 2 ? xl[i] : xh[i], accc[i][ct]);
    }
    if (amax >= F16X3_LIMIT && k.status) *k.status = 1;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int n0 = ct * 16 + lg * 4;
        const f32x4 bias = *(const f32x4*)(k.bc + n0), wsc = *(const f32x4*)(k.sc + n0);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int oy = oy0 + 2 * wave + i;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaf(accc[i][ct][e], wsc[e], bias[e]);
            *(f32x4*)(k.kc + (long)b * k.kcn + (long)oy * k.kch + (long)oxl * k.kcw + n0) = v;
        }
    }
}

}  // namespace fusg

using namespace fusg;

static bool rp_aligned16(const void* p) { return p != nullptr && (((uintptr_t)p) & 15) == 0; }

static int respair_impl(const fusg_respair_desc* d, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    FUSG_CHECK(d != nullptr, "vunet_respair: null descriptor");
    const fusg_tensor& x = d->x;
    FUSG_CHECK(d->channels == 32, "vunet_respair: channels %d (32 is built)", d->channels);
    FUSG_CHECK(d->entry == 0 || d->entry == 1, "vunet_respair: entry %d", d->entry);
    FUSG_CHECK(d->tap_order >= 0 && d->tap_order <= 2, "vunet_respair: tap_order %d", d->tap_order);
    FUSG_CHECK(is_nhwc(x) && x.n >= 1 && x.h >= 8 && x.w >= 16 && x.h % 8 == 0 && x.w % 16 == 0,
               "vunet_respair: x must be NHWC-physical f32 with h %% 8 == 0 and w %% 16 == 0 (8 x 16 patches, as the halo kernel)");
    if (d->entry) {
        FUSG_CHECK(x.c >= 1 && x.c <= 8 && d->cin >= 4 && d->cin <= 8 && d->cin % 4 == 0 && d->cin <= x.sw && x.c <= d->cin,
                   "vunet_respair: entry form takes u with at most 8 channels, cin (K-channels of the NiN) 4 or 8 <= its pixel pitch");
        FUSG_CHECK(rp_aligned16(d->w_in) && rp_aligned16(d->bias_in) && d->kpad_in >= d->cin,
                   "vunet_respair: the entry NiN's wpack / bias are missing or not 16-byte aligned");
    } else {
        FUSG_CHECK(x.c == 32, "vunet_respair: x has %ld channels, not 32", (long)x.c);
    }
    const fusg_tensor* outs[3] = {&d->s1, &d->kb, &d->kc};
    for (const fusg_tensor* o : outs) {
        FUSG_CHECK(is_nhwc(*o) && same_nhw(x, *o) && o->c == 32, "vunet_respair: s1 / kb / kc must be NHWC-physical f32 [n, 32, h, w] like x");
        FUSG_CHECK(o->data != x.data, "vunet_respair: an output aliases x (neighbouring patches read x's ring)");
    }
    FUSG_CHECK(d->s1.data != d->kb.data && d->s1.data != d->kc.data && d->kb.data != d->kc.data, "vunet_respair: outputs alias each other");
    const void* ptrs[] = {d->wfragA, d->biasA, d->wscaleA, d->wfragB, d->biasB, d->wscaleB,
                          d->wfrag_b, d->bias_b, d->wscale_b, d->wfrag_c, d->bias_c, d->wscale_c};
    for (const void* p : ptrs) FUSG_CHECK(rp_aligned16(p), "vunet_respair: a parameter array is missing or not 16-byte aligned");
    FUSG_CHECK(d->status != nullptr, "vunet_respair: status word missing");
    FUSG_CHECK(x.n * x.h * x.w * x.sw < (1L << 40), "vunet_respair: extent");
    RespairK k;
    memset(&k, 0, sizeof(k));
    k.x = (const float*)x.data; k.xsn = x.sn; k.xsh = x.sh; k.xsw = x.sw;
    k.s1 = (float*)d->s1.data; k.s1n = d->s1.sn; k.s1h = d->s1.sh; k.s1w = d->s1.sw;
    k.kb = (float*)d->kb.data; k.kbn = d->kb.sn; k.kbh = d->kb.sh; k.kbw = d->kb.sw;
    k.kc = (float*)d->kc.data; k.kcn = d->kc.sn; k.kch = d->kc.sh; k.kcw = d->kc.sw;
    k.w_in = d->w_in; k.b_in = d->bias_in; k.cin = d->cin; k.kpad_in = d->kpad_in;
    k.wA = (const _Float16*)d->wfragA; k.wB = (const _Float16*)d->wfragB; k.wb = (const _Float16*)d->wfrag_b; k.wc = (const _Float16*)d->wfrag_c;
    k.bA = d->biasA; k.bB = d->biasB; k.bb = d->bias_b; k.bc = d->bias_c;
    k.sA = d->wscaleA; k.sB = d->wscaleB; k.sb = d->wscale_b; k.sc = d->wscale_c;
    k.status = d->status;
    k.zeros = zero_line();
    if (!k.zeros) { set_error("vunet_respair: cannot allocate the zero line"); return FUSG_ERR_LAUNCH; }
    k.B = (int)x.n; k.H = (int)x.h; k.W = (int)x.w;
    k.tiles_x = k.W / 16; k.tiles_y = k.H / 8;
    const long wgs = (long)k.B * k.tiles_x * k.tiles_y;
    FUSG_CHECK(wgs < (1L << 31), "vunet_respair: grid");
    // the order of the 3x3 launches this replaces: route_conv gives a 32-column 3x3 halo launch of at most 1024 workgroups the K
    // split over the waves (conv_igemm.hip, ConvRoute::ksw)
    // (tap_order 0 counts the patches of the routing batch when one is set, as route_conv does: common.h, route_n)
    const bool split = d->tap_order == 0 ? (!env_switches().no_ksplit && route_n((long)k.B) * k.tiles_x * k.tiles_y <= 1024) : d->tap_order == 2;
    const void* fn = d->entry ? (split ? (const void*)vunet_respair_h3<32, true, true> : (const void*)vunet_respair_h3<32, true, false>)
                              : (split ? (const void*)vunet_respair_h3<32, false, true> : (const void*)vunet_respair_h3<32, false, false>);
    const size_t lds = respair_lds(d->entry != 0);
    const double M = (double)x.n * x.h * x.w;
    // the five convolutions' own FLOPs (no ring recompute), K as the unfused launches count it (k_pad)
    prof_begin(0, s, 2.0 * M * 32.0 * ((d->entry ? (double)d->kpad_in : 0.0) + 2.0 * 9.0 * 32.0 + 2.0 * 32.0));
    const hipError_t e = launch_kernel(fn, dim3((unsigned)wgs), lds, (int)lds, k, s);
    prof_end(0, s);
    if (e != hipSuccess) { set_error("vunet_respair launch: %s", hipGetErrorString(e)); return FUSG_ERR_LAUNCH; }
    note_conv_kernel(FUSG_CONV_RESPAIR);
    return FUSG_OK;
}
extern "C" int fusg_vunet_respair(const fusg_respair_desc* d, void* stream) { return fusg::plan_dispatch(respair_impl, stream, d); }
extern "C" int fusg_sizeof_respair_desc(void) { return (int)sizeof(fusg_respair_desc); }
