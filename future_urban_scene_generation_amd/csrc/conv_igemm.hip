// Host side of the fused implicit-GEMM convolution: descriptor validation, tile / split-K
// heuristics, routing to a kernel family, launch, and the deterministic split-K slab reduction.  Kernel: conv_kernel.h.
#include <stdlib.h>
#include <mutex>
#include "conv_kernel_tapunit.h"
#include "conv_kernel_small.h"
#include "conv_kernel_tapunit_f32.h"

namespace fusg {

// Deterministic split-K slab reduction + the same epilogue.  One thread per (phase, m, 4 channels).
__global__ __launch_bounds__(256) void conv_splitk_reduce(const ConvK p, int nphase) {
    const int n4 = p.Cout_pad >> 2;
    const long total = (long)nphase * p.M * n4;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % n4);
    const long pm = idx / n4;
    const int m = (int)(pm % p.M);
    const int phase = (int)(pm / p.M);
    // slabs are summed in slab order (the result does not depend on the unrolling); eight independent 16-byte loads are
    // in flight per thread instead of one load per dependent add (the loop used to pay one L2 round trip per slab)
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    const float* base = p.ws + ((long)phase * p.ksplit * p.M + m) * p.Cout_pad + c4 * 4;
    const long slab = (long)p.M * p.Cout_pad;
    int k = 0;
    for (; k + 8 <= p.ksplit; k += 8) {
        f32x4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = *(const f32x4*)(base + (long)(k + j) * slab);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    if (k + 4 <= p.ksplit) {
        f32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = *(const f32x4*)(base + (long)(k + j) * slab);
#pragma unroll
        for (int j = 0; j < 4; ++j) s += v[j];
        k += 4;
    }
    for (; k < p.ksplit; ++k) s += *(const f32x4*)(base + (long)k * slab);
    PixOff po;
    if (!pix_offsets(p, phase, m, po)) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int n = c4 * 4 + c;
        if (n < p.Cout) {
            PixOff co;
            chan_offsets(p, n, co);
            epi_store(p, po, co, p.bias[n], p.wscale ? p.wscale[n] : 1.f, s[c]);
        }
    }
}

// Pointwise convolution from at most 8 input channels (the VUnet's NiN stems, 6 -> 128 and 3 -> 32 at full resolution):
// such a layer is a stream of output stores (1.07 GB for 6 -> 128 at B = 32) with 3 - 8 multiply-adds per output
// element - nothing for the matrix cores.  A workgroup takes PW_ITEMS * 256 / n4 consecutive pixels (n4 = cout_pad / 4):
//   1. its pixels' input channels are loaded ONCE (one 16-byte load per thread), pre-processed (ELU / ReLU) and parked in
//      LDS - with one thread per (pixel, 4 output channels) every thread of a pixel would otherwise redo the 8 ELUs;
//   2. a thread's 4 output columns are the same for all of its items (256 % n4 == 0): their 8 weight vectors and the bias
//      are read once into registers;
//   3. per item: the pixel's 8 values from LDS (two broadcast reads), an fp32 fmaf chain per output channel in the exact-
//      fp32 MFMA kernel's k order (bit for bit what that kernel computes: no fp16 split, no range status to raise), bias /
//      activation / residuals, ONE fully coalesced 16-byte store per lane.
// (Measured on the way: 4 columns per thread with per-thread ELUs and 64-bit index divisions 0.47 ms for 6 -> 128 at B = 32,
// 16 columns per thread - four 16-byte stores 64 bytes apart between lanes - 0.62 ms; the tap-unit MFMA kernel 0.31 ms.)
constexpr int PW_ITEMS = 16;
__global__ __launch_bounds__(256) void conv_pointwise_small(const ConvK p, int npix) {
    extern __shared__ __attribute__((aligned(16))) float smem_pw[];
    const int n4 = p.Cout_pad >> 2;                    // threads per pixel; divides 256 (host-checked)
    const int ppb = PW_ITEMS * 256 / n4;               // pixels per workgroup
    float* wl = smem_pw;                               // [8 channels][Cout_pad]
    float* xs = smem_pw + p.Cout_pad * 8;              // [ppb][8]: pre-processed inputs
    const int t = threadIdx.x;
    for (int i = t; i < p.Cout_pad * 8; i += 256) {
        const int c = i / p.Cout_pad, n = i - c * p.Cout_pad;
        wl[i] = c < p.C0 ? p.wpack[(long)n * p.K_pad + c] : 0.f;
    }
    const int hw = p.Ho * p.Wo;
    const int pix0 = blockIdx.x * ppb;
    const int halves = p.C0 > 4 ? 2 : 1;               // 16-byte pieces per pixel
    for (int i = t; i < ppb * 2; i += 256) {
        const int pl = i >> 1, hf = i & 1, m = pix0 + pl;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (m < npix && hf < halves) {
            const int b = m / hw, rem = m - b * hw, oy = rem / p.Wo, ox = rem - oy * p.Wo;
            v = *(const f32x4*)(p.src0 + ((long)(b * p.H + oy) * p.W + ox) * p.Cs0 + hf * 4);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (p.pre_op == FUSG_PRE_ELU) v[c] = elu1(v[c]);
                else if (p.pre_op == FUSG_PRE_RELU) v[c] = fmaxf(v[c], 0.f);
            }
        }
        *(f32x4*)(xs + pl * 8 + hf * 4) = v;
    }
    __syncthreads();
    const int c4 = t % n4, n = c4 * 4, pl0 = t / n4, ppi = 256 / n4;     // this thread's columns; pixels advance by ppi per item
    if (n >= p.Cout) return;
    f32x4 w[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c] = *(const f32x4*)(wl + c * p.Cout_pad + n);
    const f32x4 bias = *(const f32x4*)(p.bias + n);
#pragma unroll 4
    for (int it = 0; it < PW_ITEMS; ++it) {
        const int pl = it * ppi + pl0, m = pix0 + pl;
        if (m >= npix) return;
        const f32x4 xa = *(const f32x4*)(xs + pl * 8), xb = *(const f32x4*)(xs + pl * 8 + 4);
        // k order 0, 4, 1, 5, 2, 6, 3, 7: v_mfma_f32_32x32x2_f32 takes k = e from lane half 0 and k = 4 + e from half 1 in the
        // exact-fp32 kernel; channels past C0 meet zero weights
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(xb[e], w[4 + e][j], fmaf(xa[e], w[e][j], acc[j]));
        const int b = m / hw, rem = m - b * hw, oy = rem / p.Wo, ox = rem - oy * p.Wo;
        const long Y = (long)oy * p.osy + p.ooy[0], X = (long)ox * p.osx + p.oox[0];
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = act_apply(fmaf(acc[j], 1.f, bias[j]), p.act);
        if (p.res0) v += *(const f32x4*)(p.res0 + b * p.r0n + Y * p.r0h + X * p.r0w + n);
        if (p.res1) v += *(const f32x4*)(p.res1 + b * p.r1n + Y * p.r1h + X * p.r1w + n);
        *(f32x4*)(p.dst + b * p.dsn + Y * p.dsh + X * p.dsw + p.dst_c_off + n) = v;
    }
}

struct TileCfg { int bm, bn; };
static const TileCfg kTiles[] = {{0, 0}, {128, 128}, {128, 64}, {128, 32}, {64, 64}, {64, 128}};

// 256 zero bytes per device, allocated on first use (see ConvK::zeros)
const float* zero_line() {
    static std::mutex mu;
    static float* z[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> g(mu);
    if (!z[dev]) {
        float* q = nullptr;
        if (hipMalloc((void**)&q, 256) != hipSuccess) return nullptr;
        // one-time: the memset runs on the null stream, which non-blocking streams do not wait for
        if (hipMemset(q, 0, 256) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipFree(q); return nullptr; }
        z[dev] = q;
    }
    return z[dev];
}

// a device pointer that is present and 16-byte aligned
static bool aligned16(const void* p) { return p != nullptr && (((uintptr_t)p) & 15) == 0; }

// Does this launch take the small-spatial kernel (conv_kernel_small.h), and with which K ranges?  (plan_impl)
struct SmallCfg { int nimg, rpi, rpi_shift, tpi, wide, RIN, WIN, NPIX, nchw, ksplit, nch32, ntaps; long mt; };
static bool small_cfg(const fusg_conv_desc* d, int precision, SmallCfg* out) {
    // (FUSG_NO_SMALL is read per call: tests and the A/B tools flip it at run time)
    if (getenv("FUSG_NO_SMALL") != nullptr || env_switches().no_halo) return false;
    const int nphase = d->nphase > 0 ? d->nphase : 1;
    if (precision != FUSG_PREC_F16X3 || nphase != 1 || d->kh < 1 || d->kw < 1 || d->kh > 3 || d->kw > 3 || d->dil != 1 ||
        (d->pad_mode != FUSG_PAD_ZERO && d->pad_mode != FUSG_PAD_REPLICATE) || d->upsample != 0 || (d->stride != 1 && d->stride != 2) ||
        d->tile_list || d->stats_out || !aligned16(d->wfrag) || (d->wfrag_order != 0 && d->wfrag_order != 1))
        return false;
    const int ntaps = d->kh * d->kw;
    if (d->c0k <= 0 || d->c0k % 32 || d->k_pad % ntaps) return false;
    const int ctot = d->k_pad / ntaps, c1k = ctot - d->c0k;
    if (c1k < 0 || c1k % 32 || (c1k > 0 && !d->src1.data)) return false;
    if (d->wfrag_order == 1 && !(d->stride == 2 && d->kh == 3 && d->kw == 3 && d->pad_h == 1 && d->pad_w == 1)) return false;
    const int Ho = d->qh, Wo = d->qw, hw = Ho * Wo;
    // a WINDOW of a larger output (the ring launches of the ICN's up-convolutions: one edge row / column / corner) can use no
    // other fast kernel, whatever its size; whole images only up to small_maxhw pixels (beyond, the halo kernel is faster)
    const long full_h = (d->src0.h + 2L * d->pad_h - d->kh) / d->stride + 1, full_w = (d->src0.w + 2L * d->pad_w - d->kw) / d->stride + 1;
    const bool part = (d->q_oy | d->q_ox) != 0 || Ho != full_h || Wo != full_w;
    const bool window = part && d->pad_mode == FUSG_PAD_REPLICATE;     // (zero padding: whole images only - q_size launches keep their kernels)
    if (part && !window) return false;
    if (!window && hw > env_switches().small_maxhw) return false;
    SmallCfg c;
    c.tpi = 1; c.wide = 0; c.rpi = SMALL_ROWS; c.rpi_shift = 5;
    const long B = d->src0.n;
    if (hw < SMALL_ROWS && SMALL_ROWS % hw == 0 && !window) {          // several whole images per workgroup
        c.nimg = SMALL_ROWS / hw; c.rpi = hw;
        c.rpi_shift = 0;
        while ((1 << c.rpi_shift) < c.rpi) ++c.rpi_shift;
        c.RIN = (Ho - 1) * d->stride + d->kh;
        c.WIN = (Wo - 1) * d->stride + d->kw;
        c.mt = (B + c.nimg - 1) / c.nimg;
    } else {                                                            // runs of 32 pixels of one image (the last run of an image may be short)
        c.nimg = 1;
        c.tpi = (hw + SMALL_ROWS - 1) / SMALL_ROWS;
        if (Wo >= SMALL_ROWS) {
            if (!(Ho == 1 || Wo % SMALL_ROWS == 0)) return false;       // a run must stay inside one output row
            c.wide = 1;
            c.RIN = d->kh;
            c.WIN = (SMALL_ROWS - 1) * d->stride + d->kw;
        } else {
            if (SMALL_ROWS % Wo) return false;
            c.RIN = (SMALL_ROWS / Wo - 1) * d->stride + d->kh;
            c.WIN = (Wo - 1) * d->stride + d->kw;
        }
        c.mt = B * c.tpi;
    }
    c.NPIX = c.nimg * c.RIN * c.WIN;
    if (c.NPIX > SMALL_MAXPIX || c.mt * c.tpi >= (1L << 31) || c.mt * (d->cout_pad / 32) >= (1L << 31) || (long)hw * c.tpi >= (1L << 16)) return false;
    c.nch32 = ctot / 32; c.ntaps = ntaps;
    // chunks per K range: the staged image must fit (<= 112 KiB) and a wave should not need more than two rounds of weights
    int nchw = (112 * 1024) / (c.NPIX * 128);
    const int by_rounds = (2 * 4 * SMALL_NS) / ntaps;
    if (by_rounds < nchw) nchw = by_rounds;
    if (nchw < 1) return false;
    if (d->ksplit == 1 && nchw < c.nch32) return false;            // the caller wants K whole
    if (nchw > c.nch32) nchw = c.nch32;
    c.ksplit = (c.nch32 + nchw - 1) / nchw;
    c.nchw = (c.nch32 + c.ksplit - 1) / c.ksplit;
    c.ksplit = (c.nch32 + c.nchw - 1) / c.nchw;                    // every range non-empty
    // K ranges over workgroups (+ the slab reduce) are implemented and tested, but measured SLOWER than the generic gather
    // they would replace (profiles/r04_ab_experiments.txt: 1024 -> 512 k3 at 4 x 4, B = 32: 75.6 vs 41.6 us - sixteen row
    // tiles each stream the 18.9 MB of weights; 512 -> 128: 20.6 vs 16.5 us): FUSG_SMALL_KSPLIT=1 lets them through
    if (c.ksplit > 1 && getenv("FUSG_SMALL_KSPLIT") == nullptr) return false;
    *out = c;
    return true;
}

// Tile, K split and workspace bytes.  Reads only shapes, so it also serves fusg_conv2d_plan on a bare descriptor.
// `small` (may be NULL) receives the small kernel's configuration; small->ksplit == 0: the launch does not take it.
// The tile and the K split are CHOSEN for route_n(n) images (the routing batch when one is set: common.h) and the workspace is
// SIZED for the n images of the launch.
static int64_t plan_impl(fusg_conv_desc* d, SmallCfg* small) {
    const long M = (long)d->src0.n * d->qh * d->qw;
    const long Mr = route_n((long)d->src0.n) * d->qh * d->qw;      // what the choices below see
    const int nphase = d->nphase > 0 ? d->nphase : 1;
    SmallCfg sc;
    if (small_cfg(d, d->precision == FUSG_PREC_BF16 || d->precision == FUSG_PREC_F16 ? FUSG_PREC_F16X3 : d->precision, &sc)) {
        d->tile = FUSG_TILE_128x32;
        d->ksplit = sc.ksplit;
        if (small) *small = sc;
        return sc.ksplit > 1 ? (int64_t)sc.ksplit * M * d->cout_pad * (int64_t)sizeof(float) : 0;
    }
    if (small) small->ksplit = 0;
    if (d->tile == FUSG_TILE_AUTO) {
        int bn = d->cout_pad >= 128 && d->cout_pad % 128 == 0 ? 128 : (d->cout_pad % 64 == 0 ? 64 : 32);
        int bm = 128;
        // small problems: prefer more, smaller tiles
        long tiles = ((Mr + 127) / 128) * (d->cout_pad / bn) * nphase;
        if (tiles < 256 && bn == 128) { bn = 64; tiles = ((Mr + 127) / 128) * (d->cout_pad / bn) * nphase; }
        if (tiles < 256 && bn == 64) { bm = 64; }
        d->tile = bm == 128 ? (bn == 128 ? FUSG_TILE_128x128 : bn == 64 ? FUSG_TILE_128x64 : FUSG_TILE_128x32)
                            : FUSG_TILE_64x64;
        // Split-fp16 generic kernel: staging-bound rather than matrix-bound, so the 64-row tiles (32
        // accumulator VGPRs per 64x128, 48 KiB LDS -> 3 workgroups/CU) beat the 128-row ones by 10-20 %
        // on every large layer measured (tools/bench_layer.py); the 32-wide tile only exists as 128x32.
        if (d->precision == FUSG_PREC_F16X3 && bm == 128 && bn >= 64)
            d->tile = bn == 128 ? FUSG_TILE_64x128 : FUSG_TILE_64x64;
    }
    const TileCfg tc = kTiles[d->tile];
    const long tiles = ((Mr + tc.bm - 1) / tc.bm) * (d->cout_pad / tc.bn) * nphase;
    const int nk = d->k_pad / BK;
    if (d->ksplit <= 0) {
        int ks = 1;
        if (tiles < 192 && nk >= 8) {
            ks = (int)((512 + tiles - 1) / tiles);
            if (ks > nk / 4) ks = nk / 4;
            if (ks > 32) ks = 32;
            if (ks < 1) ks = 1;
        }
        d->ksplit = ks;
    }
    if (d->ksplit <= 1) { d->ksplit = 1; return 0; }
    return (int64_t)nphase * d->ksplit * M * d->cout_pad * (int64_t)sizeof(float);
}

// Column-tile width of the halo and tap-unit kernels: the widest of 128 / 64 / 32 that divides cout_pad and is at most
// `cap`, halved while a grid of `mt` row tiles would have fewer than `min_wg` workgroups; FUSG_HALO_BN overrides.
static int column_tile(int cout_pad, int cap, long mt = 0, long min_wg = 0) {
    int bn = cout_pad % 128 == 0 ? 128 : (cout_pad % 64 == 0 ? 64 : 32);
    if (bn > cap) bn = cap;
    while (bn > 32 && mt * (cout_pad / bn) < min_wg) bn /= 2;
    if (const int v = env_switches().halo_bn; (v == 32 || v == 64 || v == 128) && cout_pad % v == 0) bn = v;
    return bn;
}

// LDS offsets of the tap-unit kernels' K units (`unit` channels of one tap, taps row-major; halo rows RP apart, pixels
// c0k apart).  Returns the number of units.
static int tapunit_offsets(int* uoff, const fusg_conv_desc& d, int unit, int RP) {
    const int upp = d.c0k / unit, nunits = d.kh * d.kw * upp;
    for (int j = 0; j < nunits; ++j) {
        const int tap = j / upp, u = j - tap * upp, ky = tap / d.kw, kx = tap - ky * d.kw;
        uoff[j] = ky * RP + kx * d.c0k + u * unit;
    }
    return nunits;
}

// The taps of a stride-2 layer in parity-quadrant slab order (include/fusg.h wfrag_order 1, pack.s2d_tap_order): input row
// 2Y - 1 + ky has parity (ky - 1) & 1, so quadrant q = 2 ((ky - 1) & 1) + ((kx - 1) & 1); fn(q, ky, kx) quadrant by quadrant.
template <class Fn> static void for_each_quadrant_tap(int kh, int kw, Fn fn) {
    for (int q = 0; q < 4; ++q)
        for (int ky = 0; ky < kh; ++ky)
            if (((ky - 1) & 1) == (q >> 1))
                for (int kx = 0; kx < kw; ++kx)
                    if (((kx - 1) & 1) == (q & 1)) fn(q, ky, kx);
}

// What route_conv decided: the kernel family and what its launch needs beyond the descriptor.
struct ConvRoute {
    int family;                 // FUSG_CONV_*
    int vec_epi;                // 16-byte epilogue accesses (ConvK::vec_epi)
    SmallCfg sc;                // FUSG_CONV_SMALL: its configuration (plan_impl)
    int mode;                   // halo / tap-unit arithmetic: 0 split-fp16, 1 bf16, 2 exact fp32, 3 single-pass fp16
    int bn;                     // halo / tap-unit: column-tile width
    bool ksw;                   // halo: K split over the waves (the 64k / 32k instantiations)
    bool s2d;                   // halo: parity-quadrant form
    int sp;                     // halo: tap-sparse pattern the launch skips by (fusg_conv_desc.tap_sparse), 0 = dense
    bool cm;                    // halo: a chunk's taps column-major (conv_kernel_halo.h, CM) - another summation order
    int HH, HW;                 // halo / tap-unit: halo extent in (virtual) input pixels
    int RP, unit;               // tap-unit: LDS pitch of a halo row, channels per K unit
};

// Validation and the family choice of fusg_conv2d - no HIP call, no allocation.  `d` is the caller's descriptor, copied: it
// leaves planned (tile, ksplit) and with the arithmetic that runs (FUSG_PREC_BF16, FUSG_PREC_F16 -> F16X3).  Returns FUSG_OK or the error
// fusg_conv2d reports (the workspace and split-K counters, the caller's allocations, are checked by the launch).
static int route_conv(fusg_conv_desc* d, ConvRoute* r) {
    // FUSG_PREC_BF16: single-pass bf16 on the halo / tap-unit kernels where the layer qualifies, F16X3 everywhere else
    const bool want_bf16 = d->precision == FUSG_PREC_BF16;
    if (want_bf16) d->precision = FUSG_PREC_F16X3;
    // FUSG_PREC_F16: the same rule with one fp16 product on the `hi` fragments of `wfrag` (mode 3) where bf16 takes mode 1
    const bool want_f16 = d->precision == FUSG_PREC_F16;
    if (want_f16) d->precision = FUSG_PREC_F16X3;
    const fusg_tensor& x0 = d->src0;
    FUSG_CHECK(is_nhwc(x0), "conv2d: src0 must be NHWC-physical f32 (sc=1, Cs%%4=0, 16B aligned)");
    const bool has1 = d->src1.data != nullptr;
    if (has1) {
        FUSG_CHECK(is_nhwc(d->src1) && same_nhw(x0, d->src1), "conv2d: src1 must be NHWC-physical with src0's n,h,w");
    }
    FUSG_CHECK(d->bias && d->ktab, "conv2d: bias/ktab missing");
    FUSG_CHECK(d->precision >= FUSG_PREC_F32 && d->precision <= FUSG_PREC_EMU_BF16X2, "conv2d: precision %d", d->precision);
    if (d->precision != FUSG_PREC_F16X3) FUSG_CHECK(d->wpack, "conv2d: wpack missing");
    else FUSG_CHECK(aligned16(d->wpack_h) && aligned16(d->wscale) && d->status,
                    "conv2d: F16X3 needs 16B-aligned wpack_h and wscale, and a status word");
    FUSG_CHECK((((uintptr_t)d->wpack) & 15) == 0 && (((uintptr_t)d->ktab) & 7) == 0, "conv2d: wpack/ktab misaligned");
    FUSG_CHECK(d->k_pad > 0 && d->k_pad % BK == 0, "conv2d: k_pad %d not a positive multiple of %d", d->k_pad, BK);
    FUSG_CHECK(d->cout > 0 && d->cout_pad % 32 == 0 && d->cout <= d->cout_pad, "conv2d: bad cout %d / cout_pad %d", d->cout, d->cout_pad);
    FUSG_CHECK(d->c0k >= 0 && d->c0k % 4 == 0 && d->c0k <= x0.sw, "conv2d: bad c0k %d (src0 Cs %ld)", d->c0k, (long)x0.sw);
    FUSG_CHECK(d->stride == 1 || d->stride == 2, "conv2d: stride %d", d->stride);
    FUSG_CHECK(d->upsample == 0 || d->upsample == 1, "conv2d: upsample %d", d->upsample);
    FUSG_CHECK(d->pad_mode == FUSG_PAD_ZERO || d->pad_mode == FUSG_PAD_REFLECT || d->pad_mode == FUSG_PAD_REPLICATE, "conv2d: pad_mode");
    FUSG_CHECK(!d->tile_list || (d->tile_count > 0 && !d->stats_out), "conv2d: tile_list needs tile_count > 0 and no stats_out");
    FUSG_CHECK(d->pre_op >= 0 && d->pre_op <= FUSG_PRE_AFFINE, "conv2d: pre_op");
    FUSG_CHECK(d->act >= 0 && d->act <= FUSG_ACT_LEAKY02, "conv2d: act");
    if (d->pre_op >= FUSG_PRE_AFFINE_RELU) {
        FUSG_CHECK(d->pre_scale && d->pre_shift && ((((uintptr_t)d->pre_scale) | ((uintptr_t)d->pre_shift)) & 15) == 0 &&
                   d->pre_bstride % 4 == 0, "conv2d: affine pre-op needs 16B-aligned scale/shift");
    }
    const int nphase = d->nphase > 0 ? d->nphase : 1;
    FUSG_CHECK(nphase == 1 || nphase == 4, "conv2d: nphase %d", nphase);
    r->sp = 0;
    r->cm = false;
    if (d->tap_sparse != 0) {
        // the patterns describe ONE weight form (include/fusg.h): anything else would run dense weights that are not the layer
        if (!((d->tap_sparse == 1 || d->tap_sparse == 2) && d->kh == 3 && d->kw == 3 && d->pad_h == 1 && d->pad_w == 1 &&
              d->stride == 1 && d->dil == 1 && d->upsample == 0 && d->pad_mode == FUSG_PAD_ZERO && d->store_mode == FUSG_STORE_D2S && nphase == 1 &&
              d->cout > 0 && d->cout % 128 == 0 && d->cout_pad == d->cout)) {
            set_error("conv2d: tap_sparse %d needs a 3x3 zero-pad 1 stride 1 dil 1 D2S launch with nphase 1 and cout %% 128 == 0 "
                      "(kh %d kw %d pad %d,%d stride %d dil %d store %d nphase %d cout %d)", d->tap_sparse, d->kh, d->kw,
                      d->pad_h, d->pad_w, d->stride, d->dil, d->store_mode, nphase, d->cout);
            return FUSG_ERR_UNSUPPORTED;
        }
    }
    FUSG_CHECK(d->qh > 0 && d->qw > 0, "conv2d: empty output grid");
    FUSG_CHECK(d->q_oy >= 0 && d->q_ox >= 0 && (d->store_mode == FUSG_STORE_NORMAL || (d->q_oy | d->q_ox) == 0) &&
               !(d->stats_out && (d->q_oy | d->q_ox)), "conv2d: q-space origin (%d, %d)", d->q_oy, d->q_ox);
    if (nphase == 1 && d->kh > 0 && d->kw > 0) {
        // the q window must stay inside the convolution's own output range: every tap then lands within one
        // padding width of the (virtual) input, which is all the gathers' single reflection / clamp handles
        const long Hv = x0.h << d->upsample, Wv = x0.w << d->upsample;
        // (zero padding bounds-checks every tap, so any window is safe there)
        FUSG_CHECK(d->dil >= 1 && d->pad_h >= 0 && d->pad_w >= 0 &&
                   (d->pad_mode == FUSG_PAD_ZERO ||
                    ((long)(d->q_oy + d->qh - 1) * d->stride + (long)(d->kh - 1) * d->dil - d->pad_h <= Hv - 1 + d->pad_h &&
                     (long)(d->q_ox + d->qw - 1) * d->stride + (long)(d->kw - 1) * d->dil - d->pad_w <= Wv - 1 + d->pad_w &&
                     d->pad_h <= Hv - 1 && d->pad_w <= Wv - 1)),
                   "conv2d: q window [%d+%d, %d+%d] reaches outside the padded input", d->q_oy, d->qh, d->q_ox, d->qw);
    }
    const long Ml = (long)x0.n * d->qh * d->qw;
    FUSG_CHECK(Ml > 0 && Ml < (1L << 31), "conv2d: M out of range");
    FUSG_CHECK(x0.n * x0.h * x0.w * x0.sw < (1L << 40), "conv2d: src too large");
    const fusg_tensor& o = d->dst;
    FUSG_CHECK(o.data && o.dtype == FUSG_F32 && o.n == x0.n, "conv2d: dst missing / batch mismatch");
    // logical output extents implied by the store mode
    long oh, ow, oc;
    if (d->store_mode == FUSG_STORE_D2S) {
        FUSG_CHECK(d->cout % 4 == 0 && nphase == 1, "conv2d: D2S needs cout%%4==0");
        oh = 2L * d->qh; ow = 2L * d->qw; oc = d->cout / 4;
    } else if (d->store_mode == FUSG_STORE_S2D) {
        FUSG_CHECK(d->qh % 2 == 0 && d->qw % 2 == 0 && nphase == 1, "conv2d: S2D needs even output grid");
        oh = d->qh / 2; ow = d->qw / 2; oc = 4L * d->cout;
    } else {
        FUSG_CHECK(d->store_mode == FUSG_STORE_NORMAL && d->out_sy >= 1 && d->out_sx >= 1, "conv2d: store mode / out stride");
        oh = 0; ow = 0;
        for (int ph = 0; ph < nphase; ++ph) {
            FUSG_CHECK(d->out_oy[ph] >= 0 && d->out_ox[ph] >= 0, "conv2d: negative phase offset");
            const long eh = (long)(d->q_oy + d->qh - 1) * d->out_sy + d->out_oy[ph] + 1, ew = (long)(d->q_ox + d->qw - 1) * d->out_sx + d->out_ox[ph] + 1;
            oh = oh > eh ? oh : eh;
            ow = ow > ew ? ow : ew;
        }
        oc = d->cout;
    }
    FUSG_CHECK(oh <= o.h && ow <= o.w && d->dst_c_off >= 0 && d->dst_c_off + oc <= o.c,
               "conv2d: dst [%ld,%ld,%ld,%ld] too small for output %ldx%ldx%ld at channel offset %d",
               (long)o.n, (long)o.c, (long)o.h, (long)o.w, oc, oh, ow, d->dst_c_off);
    const fusg_tensor* rs[2] = {&d->res0, &d->res1};
    for (int i = 0; i < 2; ++i) {
        if (!rs[i]->data) continue;
        FUSG_CHECK(d->store_mode == FUSG_STORE_NORMAL && rs[i]->dtype == FUSG_F32 && rs[i]->n == o.n &&
                   rs[i]->c >= oc && rs[i]->h >= oh && rs[i]->w >= ow, "conv2d: residual %d shape mismatch", i);
    }

    // Plan after the bf16 rewrite above: a caller that did not plan (tile AUTO) gets the tile of the F16X3 kernels its layer
    // falls back to, while ops.conv, which plans first, has planned with its own precision code (bf16: the 128-row tiles).
    // Both are kept as they are - the tile and the K split fix the summation order of the generic kernels, hence their bits.
    plan_impl(d, &r->sc);
    FUSG_CHECK(d->tile >= 1 && d->tile <= 5, "conv2d: tile %d", d->tile);
    FUSG_CHECK(d->cout_pad % kTiles[d->tile].bn == 0, "conv2d: cout_pad %d not a multiple of tile N %d", d->cout_pad, kTiles[d->tile].bn);
    {   // 16-byte epilogue accesses need channel-contiguous, 16-byte aligned destinations and residuals
        auto vec_ok = [](const fusg_tensor& t) {
            return t.sc == 1 && (((uintptr_t)t.data) & 15) == 0 && t.sw % 4 == 0 && t.sh % 4 == 0 && t.sn % 4 == 0;
        };
        bool v = d->cout % 4 == 0 && d->dst_c_off % 4 == 0 && vec_ok(o) && !env_switches().no_vec_epi;
        if (d->store_mode == FUSG_STORE_D2S) v = v && (d->cout / 4) % 4 == 0;
        if (d->res0.data) v = v && vec_ok(d->res0);
        if (d->res1.data) v = v && vec_ok(d->res1);
        r->vec_epi = v ? 1 : 0;
    }
    if (d->stats_out) {
        // a DepthToSpace store only changes the store address (chan_offsets / pix_offsets): the slots are then per stacked column
        if (!(r->vec_epi && d->act == FUSG_ACT_NONE && !d->res0.data && !d->res1.data &&
              (d->store_mode == FUSG_STORE_NORMAL || d->store_mode == FUSG_STORE_D2S) &&
              nphase == 1 && d->ksplit <= 1 && ((long)d->qh * d->qw) % 32 == 0)) {
            set_error("conv2d: fused statistics need act NONE, no residual, NORMAL or D2S store, nphase 1, ksplit 1, qh*qw%%32==0 "
                      "and a channel-contiguous aligned dst with cout%%4==0");
            return FUSG_ERR_UNSUPPORTED;
        }
        const int slots = (int)(((long)d->qh * d->qw) / 32);
        if (d->stats_slots > 0 && d->stats_slots < slots) { set_error("conv2d: stats_slots %d < %d slots of this launch", d->stats_slots, slots); return FUSG_ERR_INVALID; }
    }

    // ---- the family, in this order; a family whose LDS does not fit goes on to the next
    const int ntaps = d->kh * d->kw;
    // small images (<= 16 x 16): the latency-built kernel of conv_kernel_small.h
    if (r->sc.ksplit > 0) { r->family = FUSG_CONV_SMALL; return FUSG_OK; }
    // pointwise from <= 8 channels: the streaming VALU kernel above - an exact fp32 fmaf chain in the generic fp32 kernel's k
    // order, so it serves both the split-fp16 and (round 4) the exact-fp32 precision with that kernel's bits
    // (FUSG_NO_POINTWISE, read per call, keeps the MFMA kernels: tests compare the two)
    if ((d->precision == FUSG_PREC_F16X3 || d->precision == FUSG_PREC_F32) && getenv("FUSG_NO_POINTWISE") == nullptr && nphase == 1 && d->kh == 1 && d->kw == 1 && d->stride == 1 && d->upsample == 0 && !has1 &&
        d->c0k >= 4 && d->c0k <= 8 && d->ksplit <= 1 && d->store_mode == FUSG_STORE_NORMAL && r->vec_epi && !d->stats_out &&
        d->cout % 4 == 0 && d->pre_op <= FUSG_PRE_ELU && (d->q_oy | d->q_ox) == 0 && !d->tile_list && d->wpack && d->pad_h == 0 &&
        d->pad_w == 0 && 256 % (d->cout_pad >> 2) == 0 && !env_switches().no_halo && !env_switches().no_pointwise) {
        r->family = FUSG_CONV_POINTWISE;
        return FUSG_OK;
    }
    // exact fp32 on the halo-family kernels (FUSG_NO_F32_HALO, read per call, keeps the generic fp32 gather)
    const bool f32_frag = d->precision == FUSG_PREC_F32 && aligned16(d->wfrag_f32) && getenv("FUSG_NO_F32_HALO") == nullptr;
    // few-channel k x k layers (the 7x7 stems): the tap-unit kernels, exact fp32 (round 4, conv_kernel_tapunit_f32.h) or
    // split-fp16 / bf16 (conv_kernel_tapunit.h)
    const bool tap_geom = d->wfrag_order == 2 && nphase == 1 && d->upsample == 0 && d->ksplit <= 1 && !has1 && d->c0k >= 4 &&
                          d->c0k <= 24 && d->kh >= 1 && d->kw >= 1 && d->dil == 1 && d->qh % 8 == 0 && d->qw % 16 == 0 &&
                          d->k_pad >= ntaps * d->c0k && (d->q_oy | d->q_ox) == 0 && !d->tile_list && !env_switches().no_halo;
    if (tap_geom && (f32_frag || (d->precision == FUSG_PREC_F16X3 && aligned16(d->wfrag)))) {
        const bool f32 = f32_frag;
        r->HH = 7 * d->stride + d->kh; r->HW = 15 * d->stride + d->kw;
        r->unit = f32 || d->c0k % 8 ? 4 : 8;
        r->RP = f32 ? r->HW * d->c0k : (r->HW * d->c0k + 127) / 128 * 128;     // split-fp16 rows 256 B apart: conflict-free 16-lane read groups
        const int nunits = ntaps * (d->c0k / r->unit), nsteps = (nunits + 16 / r->unit - 1) / (16 / r->unit);
        const size_t lds = f32 ? (size_t)r->HH * r->RP * sizeof(float) : tapunit_lds_bytes(r->HH, r->RP);
        if (nunits <= (f32 ? 320 : 160) && lds <= 80 * 1024 && r->HH * r->HW * (d->c0k / 4) <= 256 * 8) {
            // FUSG_PREC_BF16: the stem in single-pass bf16 too (wfrag_bf16 in the tap-unit form, pack.py: frag_tapunit_bf16)
            r->mode = f32 ? 2 : (want_bf16 && aligned16(d->wfrag_bf16) && getenv("FUSG_NO_BF16_TAPUNIT") == nullptr ? 1 : 0);
            // FUSG_PREC_F16: the stem in single-pass fp16 (FUSG_NO_F16_TAPUNIT, read per call, keeps the split-fp16 kernel)
            if (!f32 && want_f16 && getenv("FUSG_NO_F16_TAPUNIT") == nullptr) r->mode = 3;
            // thin split-fp16 / bf16 layers (a handful of k-steps: the launch is a stream of output stores) run 24-45 % faster on
            // the 64-column tile: its 16 KiB epilogue detour leaves room for more resident workgroups than the 128-column one
            r->bn = column_tile(d->cout_pad, !f32 && nsteps <= 4 ? 64 : 128);
            r->family = f32 ? FUSG_CONV_TAPUNIT_F32 : r->mode == 3 ? FUSG_CONV_TAPUNIT_F16 : r->mode ? FUSG_CONV_TAPUNIT_BF16 : FUSG_CONV_TAPUNIT;
            return FUSG_OK;
        }
    }
    // halo kernel: stride 1 (any dilation / padding mode / fused upsample), or stride 2 in parity-quadrant form
    // (wfrag_order 1: k3/k4, pad 1, one source, even H and W, zero or reflect padding - the quadrant staging has no clamp);
    // everything else takes the generic gather
    const bool s2d = d->wfrag_order == 1 && d->stride == 2 && x0.h % 2 == 0 && x0.w % 2 == 0 && d->pad_mode != FUSG_PAD_REPLICATE;
    if ((d->precision == FUSG_PREC_F16X3 || f32_frag) && nphase == 1 && d->ksplit <= 1 &&
        ((d->stride == 1 && d->wfrag_order == 0) || (s2d && d->upsample == 0)) &&
        d->kh >= 1 && d->kw >= 1 && d->dil >= 1 && d->c0k % 32 == 0 && d->c0k > 0 &&
        (!has1 || (d->k_pad / ntaps - d->c0k) % 32 == 0) && d->qh % 8 == 0 && d->qw % 16 == 0 &&
        d->k_pad % ntaps == 0 && aligned16(d->wfrag) && !env_switches().no_halo && (d->q_oy | d->q_ox) == 0) {
        if (s2d && !(d->kh == d->kw && (d->kh == 3 || d->kh == 4) && d->pad_h == 1 && d->pad_w == 1 && d->dil == 1 && !has1)) {
            set_error("conv2d: wfrag_order 1 needs stride 2, k3/k4, pad 1, dil 1, one source");
            return FUSG_ERR_INVALID;
        }
        const int tiles_per_img = (d->qh / 8) * (d->qw / 16);
        if (d->tile_list && d->tile_count > tiles_per_img) {
            set_error("conv2d: tile_count %d > %d patches per image", d->tile_count, tiles_per_img);
            return FUSG_ERR_INVALID;
        }
        r->s2d = s2d;
        r->HH = s2d ? 10 : 8 + (d->kh - 1) * d->dil;
        r->HW = s2d ? 18 : 16 + (d->kw - 1) * d->dil;
        // (Round 3 tried 16 x 16 pixel patches for the 32 / 64-column tiles - half the workgroups, twice the work each,
        // halo 1.27x instead of 1.41x of the patch: every such launch got 13 - 51 % SLOWER (32 -> 32 1x1 at 256 x 256
        // 130 -> 186 us, 64 -> 32 3x3 311 -> 351 us), conv time of the pass 23.9 -> 24.5 ms; round 4's bf16 128-column tile on a
        // 16 x 16 patch: 1.4x - 3x slower, profiles/r04_ab_experiments.txt.  Dropped.)
        if (halo_fits(r->HH, r->HW)) {
            // (row tiles as the two choices below count them: of the routing batch when one is set)
            const long mt = route_n((long)x0.n) * (d->tile_list ? d->tile_count : tiles_per_img);
            // pointwise layers are bound by their output stores, not by operand staging: the 64-column tile (a quarter of
            // the epilogue LDS, more resident workgroups) is 6-24 % faster there (hourglass 1x1s); k x k layers keep 128.
            // Small grids: narrower column tiles until the launch has enough workgroups to fill the chip.
            r->bn = column_tile(d->cout_pad, ntaps == 1 ? 64 : 128, mt, env_switches().halo_minwg);
            // narrow column tiles of k x k layers on SMALL grids: K split over the waves (conv_kernel_halo.h, KS) when every wave
            // gets a tap.  Measured per dispatch inside the pass (round 3, same card): grids of 256 - 1024 workgroups 2 - 14 %
            // shorter (their time is one workgroup's latency); grids of 4096 - 16384 workgroups 19 - 42 % LONGER (the four
            // partial tiles need 64 KiB of LDS: two workgroups per CU instead of three, and those launches move 3 - 4.4 TB/s -
            // they live on bytes in flight).  Hence the limit.
            r->ksw = !s2d && !d->tile_list && !env_switches().no_ksplit && mt * (d->cout_pad / r->bn) <= 1024 &&
                     ((r->bn == 32 && ntaps >= 4) || (r->bn == 64 && ntaps >= 2));
            const bool bf = want_bf16 && aligned16(d->wfrag_bf16);
            const bool f16 = want_f16 && !f32_frag;                  // (aligned16(d->wfrag) holds on this route)
            r->mode = f32_frag ? 2 : (bf ? 1 : f16 ? 3 : 0);
            // tap-sparse weights: the sibling instantiations skip the dead taps (bf16 and single-pass fp16 have none: they run the
            // dense kernel on the same weights, whose dead blocks are zeros)
            r->sp = r->mode != 1 && r->mode != 3 ? d->tap_sparse : 0;
            // dense 3x3 dil 1 split-fp16 launches of the 128-column tile: the taps of a chunk column-major (each staged row read
            // once per tap column).  (FUSG_NO_HALO_COLMAJOR, read per call, keeps the tap-major order: tests and the A/B compare the two)
            r->cm = r->bn == 128 && !r->ksw && r->mode == 0 && r->sp == 0 && !s2d && d->kh == 3 && d->kw == 3 && d->dil == 1 &&
                    getenv("FUSG_NO_HALO_COLMAJOR") == nullptr;
            r->family = f32_frag ? FUSG_CONV_HALO_F32 : bf ? FUSG_CONV_HALO_BF16 : f16 ? FUSG_CONV_HALO_F16
                                                                               : (s2d ? FUSG_CONV_HALO_S2D : FUSG_CONV_HALO);
            return FUSG_OK;
        }
    }
    if (d->tile_list) {
        set_error("conv2d: tile_list needs a launch that qualifies for the halo kernel");
        return FUSG_ERR_UNSUPPORTED;
    }
    r->family = d->precision == FUSG_PREC_F16X3 ? FUSG_CONV_GENERIC_F16X3 : FUSG_CONV_GENERIC_F32;
    return FUSG_OK;
}

// ---- one launch per family: the family's parameter block around the common ConvK
static hipError_t run_small(ConvK& k, const fusg_conv_desc& d, const SmallCfg& sc, hipStream_t s, int pk) {
    k.MT = (int)sc.mt; k.NT = d.cout_pad / 32;                  // (k is also what the split-K reduce behind it reads)
    k.ksplit = sc.ksplit;
    SmallK h;
    memset(&h, 0, sizeof(h));
    h.c = k;
    h.kh = d.kh; h.kw = d.kw; h.pad_h = d.pad_h; h.pad_w = d.pad_w; h.stride = d.stride;
    h.nch0 = d.c0k / 32; h.nch32 = sc.nch32; h.ntaps = sc.ntaps;
    h.wfrag = (const _Float16*)d.wfrag; h.nt32 = d.cout_pad / 32;
    if (d.wfrag_order == 1) {                   // parity-quadrant slab order of the stride-2 3x3 layers
        int slab = 0;
        for_each_quadrant_tap(d.kh, d.kw, [&](int, int ky, int kx) { h.tapslab |= (unsigned long long)(slab++) << (4 * (ky * d.kw + kx)); });
    } else {
        for (int tp = 0; tp < sc.ntaps; ++tp) h.tapslab |= (unsigned long long)tp << (4 * tp);
    }
    h.nchw = sc.nchw; h.nimg = sc.nimg; h.rpi = sc.rpi; h.rpi_shift = sc.rpi_shift; h.tpi = sc.tpi; h.wide = sc.wide;
    h.pad_mode = d.pad_mode;
    h.RIN = sc.RIN; h.WIN = sc.WIN; h.NPIX = sc.NPIX;
    // (the reciprocals are exact while dividend * divisor < 2^32: the dividends are tile indices (< 2^31 / tpi, checked in
    // small_cfg), pixel indices inside a 32-row tile and step numbers)
    auto magic = [](int dv) -> unsigned { return dv < 2 ? 0u : (unsigned)(((1UL << 32) + (unsigned long)dv - 1) / (unsigned long)dv); };
    h.m_wo = magic(d.qw); h.m_hw = magic(d.qh * d.qw); h.m_win = magic(sc.WIN); h.m_rw = magic(sc.RIN * sc.WIN);
    h.m_npix = magic(sc.NPIX); h.m_taps = magic(sc.ntaps); h.m_tpi = magic(sc.tpi);
    return launch_small(h, dim3(k.MT * k.NT, 1, sc.ksplit), s, pk);
}

static hipError_t run_pointwise(const ConvK& k, const fusg_conv_desc& d, hipStream_t s) {
    const int n4 = d.cout_pad >> 2, ppb = PW_ITEMS * 256 / n4;
    hipLaunchKernelGGL(conv_pointwise_small, dim3((unsigned)(((long)k.M + ppb - 1) / ppb)), dim3(256),
                       (size_t)(d.cout_pad * 8 + ppb * 8) * sizeof(float), s, k, k.M);
    return hipGetLastError();
}

// the two tap-unit parameter blocks (TapUnitF: exact fp32, TapUnitK: split-fp16 / bf16) up to their weights
template <class H> static dim3 tapunit_block(H& h, const ConvK& k, const fusg_conv_desc& d, const ConvRoute& r) {
    memset(&h, 0, sizeof(h));
    h.c = k;
    h.stride = d.stride; h.pad_h = d.pad_h; h.pad_w = d.pad_w;
    h.HH = r.HH; h.HW = r.HW; h.CP = d.c0k; h.PP = d.c0k; h.RP = r.RP;
    h.nunits = tapunit_offsets(h.uoff, d, r.unit, h.RP);
    h.nt32 = d.cout_pad / 32;
    h.tiles_x = d.qw / 16; h.tiles_per_img = (d.qh / 8) * h.tiles_x;
    h.c.MT = (int)d.src0.n * h.tiles_per_img; h.c.NT = d.cout_pad / r.bn;
    h.c.ksplit = 1;
    if (r.mode != 0 && r.mode != 3) { h.c.wscale = nullptr; h.c.status = nullptr; }       // (single-pass fp16 keeps the scales and the guard)
    return dim3(h.c.MT * h.c.NT, 1, 1);
}

static hipError_t run_tapunit(const ConvK& k, const fusg_conv_desc& d, const ConvRoute& r, hipStream_t s, int pk) {
    if (r.mode == 2) {
        TapUnitF h;
        const dim3 grid = tapunit_block(h, k, d, r);
        h.wfrag = (const float*)d.wfrag_f32;
        return r.bn == 128 ? launch_tapunit_f32_128(h, grid, s, pk) : r.bn == 64 ? launch_tapunit_f32_64(h, grid, s, pk)
                                                                                 : launch_tapunit_f32_32(h, grid, s, pk);
    }
    TapUnitK h;
    const dim3 grid = tapunit_block(h, k, d, r);
    h.nsteps = (h.nunits + 16 / r.unit - 1) / (16 / r.unit);
    h.wfrag = (const _Float16*)(r.mode == 1 ? d.wfrag_bf16 : d.wfrag);
    return r.bn == 128 ? launch_tapunit_128(h, grid, s, pk, r.unit, r.mode) : r.bn == 64 ? launch_tapunit_64(h, grid, s, pk, r.unit, r.mode)
                                                                                         : launch_tapunit_32(h, grid, s, pk, r.unit, r.mode);
}

static hipError_t run_halo(const ConvK& k, const fusg_conv_desc& d, const ConvRoute& r, hipStream_t s, int pk, const EntryK* en = nullptr) {
    HaloK h;
    memset(&h, 0, sizeof(h));
    h.c = k;
    h.kh = d.kh; h.kw = d.kw; h.dil = d.dil; h.pad_h = d.pad_h; h.pad_w = d.pad_w;
    h.c1k = d.k_pad / (d.kh * d.kw) - d.c0k;
    h.wfrag = (const _Float16*)(r.mode == 1 ? d.wfrag_bf16 : r.mode == 2 ? d.wfrag_f32 : d.wfrag);
    if (r.mode != 0 && r.mode != 3) { h.c.wscale = nullptr; h.c.status = nullptr; }       // (single-pass fp16 keeps the scales and the guard)
    h.nt32 = d.cout_pad / 32;
    h.c.NT = d.cout_pad / r.bn;
    h.c.ksplit = 1;
    h.HH = r.HH; h.HW = r.HW;
    if (r.s2d) {                                // (quadrant slabs are consecutive: qwoff is the running sum of qtaps)
        h.s2d = 1;
        for_each_quadrant_tap(d.kh, d.kw, [&](int q, int ky, int kx) {
            const int n = h.qtaps[q]++;
            h.qtdy[q][n] = ((ky - 1) >> 1) + 1;                   // arithmetic shift: floor
            h.qtdx[q][n] = ((kx - 1) >> 1) + 1;
        });
        for (int q = 1; q < 4; ++q) h.qwoff[q] = h.qwoff[q - 1] + h.qtaps[q - 1];
    }
    h.tiles_x = d.qw / 16; h.tiles_per_img = (d.qh / 8) * h.tiles_x;
    h.c.MT = (int)d.src0.n * h.tiles_per_img;
    if (d.tile_list) {
        h.tile_list = d.tile_list; h.tile_count = d.tile_count;
        h.c.MT = (int)d.src0.n * d.tile_count;
    }
    const dim3 grid(h.c.MT * h.c.NT, 1, 1);
    if (en)                                     // entry-NiN launches: the two forms entry_route admits
        return r.bn == 128 && !r.ksw ? launch_halo_en_128(h, *en, grid, s, r.cm)
                                     : r.bn == 32 && r.ksw ? launch_halo_en_32k(h, *en, grid, s) : hipErrorInvalidValue;
    if (r.sp)
        return r.bn == 128 ? launch_halo_ts_128(h, grid, s, pk, r.mode, r.sp)
                           : r.bn == 64 ? (r.ksw ? launch_halo_ts_64k(h, grid, s, pk, r.mode, r.sp) : launch_halo_ts_64(h, grid, s, pk, r.mode, r.sp))
                                        : (r.ksw ? launch_halo_ts_32k(h, grid, s, pk, r.mode, r.sp) : launch_halo_ts_32(h, grid, s, pk, r.mode, r.sp));
    return r.bn == 128 ? launch_halo_128(h, grid, s, pk, r.mode, r.cm)
                       : r.bn == 64 ? (r.ksw ? launch_halo_64k(h, grid, s, pk, r.mode) : launch_halo_64(h, grid, s, pk, r.mode))
                                    : (r.ksw ? launch_halo_32k(h, grid, s, pk, r.mode) : launch_halo_32(h, grid, s, pk, r.mode));
}

// the generic gathers by [split-fp16][tile]
typedef hipError_t (*GenericLaunch)(const ConvK&, dim3, hipStream_t, int, bool);
static const GenericLaunch kGeneric[2][6] = {
    {nullptr, launch_tile_128x128, launch_tile_128x64, launch_tile_128x32, launch_tile_64x64, launch_tile_64x128},
    {nullptr, launch_h3_128x128, launch_h3_128x64, launch_h3_128x32, launch_h3_64x64, launch_h3_64x128}};

}  // namespace fusg

using namespace fusg;

extern "C" int64_t fusg_conv2d_plan(fusg_conv_desc* d) { return plan_impl(d, nullptr); }

extern "C" int fusg_conv2d_route(const fusg_conv_desc* din) {
    fusg_conv_desc d = *din;
    ConvRoute r;
    const int rc = route_conv(&d, &r);
    return rc != FUSG_OK ? rc : r.family;
}

extern "C" int fusg_conv2d_route_order(const fusg_conv_desc* din, int32_t out[4]) {
    FUSG_CHECK(din != nullptr && out != nullptr, "conv2d_route_order: null argument");
    fusg_conv_desc d = *din;
    ConvRoute r;
    if (const int rc = route_conv(&d, &r); rc != FUSG_OK) return rc;
    const bool generic = r.family == FUSG_CONV_GENERIC_F32 || r.family == FUSG_CONV_GENERIC_F16X3;
    const bool halo = r.family == FUSG_CONV_HALO || r.family == FUSG_CONV_HALO_S2D || r.family == FUSG_CONV_HALO_BF16 ||
                      r.family == FUSG_CONV_HALO_F32 || r.family == FUSG_CONV_HALO_F16;
    const bool tapunit = r.family == FUSG_CONV_TAPUNIT || r.family == FUSG_CONV_TAPUNIT_F32 || r.family == FUSG_CONV_TAPUNIT_BF16 ||
                         r.family == FUSG_CONV_TAPUNIT_F16;
    out[0] = r.family;
    out[1] = generic ? d.tile : (halo || tapunit ? r.bn : 0);
    out[2] = r.family == FUSG_CONV_SMALL ? r.sc.ksplit : (generic ? d.ksplit : 1);
    out[3] = halo && r.ksw ? 1 : (halo && r.cm ? 2 : 0);       // K split over the waves / column-major taps / neither
    return FUSG_OK;
}

// `en`: source 0 is not read but computed by the entry NiN (fusg_conv2d_entry_nin below; the launch is a halo launch)
static int conv2d_run(const fusg_conv_desc* din, const EntryK* en, void* stream) {
    fusg_conv_desc dd = *din;
    fusg_conv_desc* d = &dd;
    ConvRoute r;
    if (const int rc = route_conv(d, &r); rc != FUSG_OK) return rc;
    FUSG_CHECK(!en || (r.family == FUSG_CONV_HALO && r.mode == 0 && r.sp == 0), "conv2d_entry_nin: not a split-fp16 halo launch");
    hipStream_t s = (hipStream_t)stream;
    const fusg_tensor& x0 = d->src0;
    const fusg_tensor& o = d->dst;
    const bool has1 = d->src1.data != nullptr;
    const int nphase = d->nphase > 0 ? d->nphase : 1;
    const long Ml = (long)x0.n * d->qh * d->qw;
    const TileCfg tc = kTiles[d->tile];
    if (d->ksplit > 1) FUSG_CHECK(d->workspace && (((uintptr_t)d->workspace) & 15) == 0, "conv2d: split-K needs a 16B-aligned workspace");
    if (d->ksplit > 1 && d->splitk_counters)
        FUSG_CHECK((long)((Ml + tc.bm - 1) / tc.bm) * (d->cout_pad / tc.bn) * nphase <= d->splitk_counters_len,
                   "conv2d: %d split-K counters for %ld tiles", d->splitk_counters_len, (long)((Ml + tc.bm - 1) / tc.bm) * (d->cout_pad / tc.bn) * nphase);

    ConvK k;
    memset(&k, 0, sizeof(k));
    k.src0 = (const float*)x0.data; k.src1 = has1 ? (const float*)d->src1.data : (const float*)x0.data;
    k.wpack = d->wpack; k.bias = d->bias; k.ktab = (const int2*)d->ktab;
    k.pre_scale = d->pre_scale; k.pre_shift = d->pre_shift; k.pre_bstride = d->pre_bstride;
    k.dst = (float*)o.data; k.dsn = o.sn; k.dsc = o.sc; k.dsh = o.sh; k.dsw = o.sw;
    if (d->res0.data) { k.res0 = (const float*)d->res0.data; k.r0n = d->res0.sn; k.r0c = d->res0.sc; k.r0h = d->res0.sh; k.r0w = d->res0.sw; }
    if (d->res1.data) { k.res1 = (const float*)d->res1.data; k.r1n = d->res1.sn; k.r1c = d->res1.sc; k.r1h = d->res1.sh; k.r1w = d->res1.sw; }
    k.ws = d->workspace;
    k.counters = d->ksplit > 1 ? d->splitk_counters : nullptr;
    k.qy0 = d->q_oy; k.qx0 = d->q_ox;
    k.zeros = zero_line();
    if (!k.zeros) { set_error("conv2d: cannot allocate the zero line"); return FUSG_ERR_LAUNCH; }
    k.touch_w = env_switches().no_touch ? 0 : 1;
    k.wpack_h = (const _Float16*)d->wpack_h;
    if (d->precision == FUSG_PREC_F16X3) { k.wscale = d->wscale; k.status = d->status; }
    k.round_bits = d->precision == FUSG_PREC_EMU_BF16 ? 8 : (d->precision == FUSG_PREC_EMU_BF16X2 ? 16 : 0);
    k.H = (int)x0.h; k.W = (int)x0.w; k.ups = d->upsample; k.Hv = k.H << k.ups; k.Wv = k.W << k.ups;
    k.Cs0 = (int)x0.sw; k.Cs1 = has1 ? (int)d->src1.sw : (int)x0.sw; k.C0 = d->c0k;
    k.K_pad = d->k_pad; k.nk = d->k_pad / BK; k.Cout = d->cout; k.Cout_pad = d->cout_pad;
    k.stride = d->stride; k.pad_mode = d->pad_mode; k.pre_op = d->pre_op; k.act = d->act; k.store_mode = d->store_mode;
    k.B = (int)x0.n; k.Ho = d->qh; k.Wo = d->qw; k.M = (int)Ml;
    k.MT = (k.M + tc.bm - 1) / tc.bm; k.NT = d->cout_pad / tc.bn;
    k.osy = d->out_sy; k.osx = d->out_sx;
    for (int i = 0; i < 4; ++i) { k.ooy[i] = d->out_oy[i]; k.oox[i] = d->out_ox[i]; }
    k.dst_c_off = d->dst_c_off; k.Cd = d->store_mode == FUSG_STORE_D2S ? d->cout / 4 : d->cout;
    k.ksplit = d->ksplit; k.steps_per_split = (k.nk + d->ksplit - 1) / d->ksplit;
    k.vec_epi = r.vec_epi;
    k.stats = d->stats_out;
    if (d->stats_out) k.stats_slots = d->stats_slots > 0 ? d->stats_slots : (int)(((long)d->qh * d->qw) / 32);
    int pk = PK_NONE;
    k.pre_relu = 0;
    switch (d->pre_op) {
        case FUSG_PRE_RELU: k.pre_relu = 1; break;
        case FUSG_PRE_ELU: pk = PK_ELU; break;
        case FUSG_PRE_AFFINE_RELU: pk = PK_AFFINE; k.pre_relu = 1; break;
        case FUSG_PRE_AFFINE: pk = PK_AFFINE; break;
        default: break;
    }

    const double flops = 2.0 * (double)Ml * d->cout * d->k_pad * nphase;   // padded-K flops; bench uses algorithmic ones
    prof_begin(0, s, flops);
    hipError_t e;
    const char* what = "conv2d launch";
    switch (r.family) {
        case FUSG_CONV_SMALL:     what = "conv2d small-image launch"; e = run_small(k, *d, r.sc, s, pk); break;
        case FUSG_CONV_POINTWISE: what = "conv2d pointwise launch"; e = run_pointwise(k, *d, s); break;
        case FUSG_CONV_TAPUNIT_F32: case FUSG_CONV_TAPUNIT: case FUSG_CONV_TAPUNIT_BF16: case FUSG_CONV_TAPUNIT_F16:
            what = r.mode == 2 ? "conv2d fp32 tap-unit launch" : "conv2d tap-unit launch";
            e = run_tapunit(k, *d, r, s, pk);
            break;
        case FUSG_CONV_GENERIC_F32: case FUSG_CONV_GENERIC_F16X3:
            e = kGeneric[d->precision == FUSG_PREC_F16X3][d->tile](k, dim3(k.MT * k.NT, nphase, d->ksplit), s, pk,
                                                                   d->pad_mode != FUSG_PAD_ZERO || d->upsample != 0);
            break;
        default:                  what = "conv2d halo launch"; e = run_halo(k, *d, r, s, pk, en); break;
    }
    // K ranges over workgroups: the slab reduce (the generic kernels combine in-launch when given split-K counters)
    if (e == hipSuccess && k.ksplit > 1 && (r.family == FUSG_CONV_SMALL || k.counters == nullptr)) {
        what = "conv2d split-K reduce launch";
        const long total = (long)nphase * k.M * (k.Cout_pad >> 2);
        hipLaunchKernelGGL(conv_splitk_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, k, nphase);
        e = hipGetLastError();
    }
    prof_end(0, s);
    if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return FUSG_ERR_LAUNCH; }
    note_conv_kernel(en ? FUSG_CONV_HALO_ENTRY : r.family);
    return FUSG_OK;
}
static int conv2d_impl(const fusg_conv_desc* din, void* stream) { return conv2d_run(din, nullptr, stream); }
extern "C" int fusg_conv2d(const fusg_conv_desc* din, void* stream) { return fusg::plan_dispatch(conv2d_impl, stream, din); }

// ---- fusg_conv2d_entry_nin: a few-channel pointwise NiN and the 3x3 Residual that is its only reader, as one halo launch
// Which form would run: 0 none (the pair stays two launches), 1 the 128-column tile (M split over the waves), 2 the 32-column
// tile with K split over the waves - the form fusg_conv2d gives the Residual at this grid size, so that the sums keep their
// order - or a negative FUSG_ERR_*.  Fills the halo launch's descriptor and the NiN's parameter block.
static int entry_route(const fusg_conv_desc* res, const fusg_conv_desc* nin, fusg_conv_desc* dd, EntryK* en) {
    FUSG_CHECK(res != nullptr && nin != nullptr, "conv2d_entry_nin: null descriptor");
    const fusg_tensor& u = nin->src0;
    const fusg_tensor& o = res->dst;
    FUSG_CHECK(is_nhwc(u) && is_nhwc(o) && same_nhw(u, o) && o.data != u.data, "conv2d_entry_nin: u and dst must be distinct NHWC-physical f32 tensors with the same n, h, w");
    // the NiN as the launch of its own that it would be (its output has dst's shape)
    fusg_conv_desc nd = *nin;
    nd.dst = o;
    ConvRoute nr;
    if (const int rc = route_conv(&nd, &nr); rc != FUSG_OK) return rc;
    if (!(nr.family == FUSG_CONV_POINTWISE && nin->precision == FUSG_PREC_F16X3 && nin->pre_op == FUSG_PRE_ELU && nin->act == FUSG_ACT_NONE &&
          !nin->res0.data && !nin->res1.data && nin->dst_c_off == 0 && nin->out_sy == 1 && nin->out_sx == 1 && nin->out_oy[0] == 0 &&
          nin->out_ox[0] == 0 && nin->qh == u.h && nin->qw == u.w && nin->cout == nin->cout_pad && aligned16(nin->bias) && nin->k_pad >= nin->c0k))
        return 0;
    // the Residual: single-source k3 s1 p1 zero-padded ELU launch from the NiN's channels, its residual the NiN's output
    if (!(res->precision == FUSG_PREC_F16X3 && res->pre_op == FUSG_PRE_ELU && res->act == FUSG_ACT_NONE && res->store_mode == FUSG_STORE_NORMAL &&
          res->kh == 3 && res->kw == 3 && res->dil == 1 && res->pad_h == 1 && res->pad_w == 1 && res->stride == 1 && res->upsample == 0 &&
          res->pad_mode == FUSG_PAD_ZERO && (res->nphase == 0 || res->nphase == 1) && !res->src1.data && !res->res1.data && !res->tile_list &&
          !res->stats_out && res->tap_sparse == 0 && res->wfrag_order == 0 && res->dst_c_off == 0 && res->out_sy == 1 && res->out_sx == 1 &&
          res->out_oy[0] == 0 && res->out_ox[0] == 0 && (res->q_oy | res->q_ox) == 0 && res->qh == o.h && res->qw == o.w &&
          res->c0k == nin->cout && res->cout == res->c0k && res->cout_pad == res->cout && res->k_pad == 9 * res->c0k && o.c == res->cout &&
          res->c0k == 128))                                    // (128 channels is what is built and tested)
        return 0;
    *dd = *res;
    dd->src0 = o;                                              // x0's geometry; never read
    dd->src1 = fusg_tensor{};
    dd->res0 = fusg_tensor{};
    ConvRoute r;
    if (const int rc = route_conv(dd, &r); rc != FUSG_OK) return rc;
    if (!(r.family == FUSG_CONV_HALO && r.mode == 0 && r.sp == 0 && !r.s2d && r.vec_epi)) return 0;
    en->u = (const float*)u.data; en->usn = u.sn; en->ush = u.sh; en->usw = u.sw;
    en->w_in = nin->wpack; en->b_in = nin->bias; en->cin = nin->c0k; en->kpad = nin->k_pad;
    return r.bn == 128 && !r.ksw ? 1 : (r.bn == 32 && r.ksw ? 2 : 0);
}
static int entry_nin_impl(const fusg_conv_desc* res, const fusg_conv_desc* nin, void* stream) {
    fusg_conv_desc dd;
    EntryK en;
    const int form = entry_route(res, nin, &dd, &en);
    if (form < 0) return form;
    if (form == 0) { set_error("conv2d_entry_nin: this pair does not fuse (fusg_conv2d_entry_nin_route == 0): run the two launches"); return FUSG_ERR_UNSUPPORTED; }
    return conv2d_run(&dd, &en, stream);
}
extern "C" int fusg_conv2d_entry_nin(const fusg_conv_desc* res, const fusg_conv_desc* nin, void* stream) {
    return fusg::plan_dispatch(entry_nin_impl, stream, res, nin);
}
extern "C" int fusg_conv2d_entry_nin_route(const fusg_conv_desc* res, const fusg_conv_desc* nin) {
    fusg_conv_desc dd;
    EntryK en;
    return entry_route(res, nin, &dd, &en);
}
