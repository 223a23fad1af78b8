// Halo-tiled split-fp16 convolution for k x k layers whose sources have a multiple of 32 channels (the layers that
// carry most of the FLOPs: 3x3 / dilated 3x3 / 5x5(+2x upsample) / 7x1 / 1x1, stride 1; stride-2 k3/k4 in
// parity-quadrant form).
//
// The generic kernel (conv_kernel_h3.h) re-gathers and re-converts the A operand for every tap: for a 3x3 layer every
// activation is fetched from L2, pre-processed (ELU / affine+ReLU) and split into fp16 (hi, lo') nine times, and on
// gfx950 that VALU + L2 work - not the matrix pipe - is what bounds it (measured: MFMA pipe 26 % busy).  Here a
// workgroup owns an 8 x 16 patch of output pixels of ONE image and BN output channels.  For each 32-channel chunk of
// the input it stages the patch's halo ((8+(kh-1)d) x (16+(kw-1)d) pixels) ONCE: gather -> pre-op -> fp16 split ->
// LDS.  All kh*kw taps then read their A fragments from that LDS image; only the (static, pre-split) weight tile of
// each (chunk, tap) streams in.  Per output tile this cuts the A-side L2 traffic and the staging VALU work by ~kh*kw.
//
// Contraction: v_mfma_f32_16x16x32_f16 (16 x 16 tiles, one instruction per 32 k = one staged chunk).  Same FLOPs per
// cycle as 32x32x16, but under the board's power limit the chip holds a higher clock on this shape
// (MI355X_MICROARCH.md, DVFS give-back item 7): measured on the layers of the crop pass, sustained, same card, same
// run: 256->256 3x3 372 -> 412 TFLOP/s, 128->128 3x3 @256 322 -> 348, 5x5+upsample 256->128 402 -> 464, dilated 3x3
// 363 -> 395, joules per launch -8..-13 % (profiles/r02_halo_m16_ab.txt).
// A fragments: one patch row (16 pixels) x 32 channels per instruction: lane l = pixel l & 15, channels
// 8 (l >> 4) .. +8.  The halo image has a 64-byte pixel pitch (no padding) and the 16-byte channel slot g of halo
// column hx is stored at slot g ^ 2 ((hx >> 2) & 1): with that swizzle the four 16-lane service groups of a
// ds_read_b128 each touch 16 distinct 16-byte bank groups for EVERY tap shift (exhaustive search over pitches 64-144 B
// and 4-class swizzles; the unswizzled 64- and 80-byte pitches are 2-way conflicted on this operand shape).
//
// Weights never touch LDS: pack.py stores them a second time in MFMA-fragment order (lane l: column l & 15, k
// 8 (l >> 4) .. +8), so the B operand of every (tap, chunk, 16-column tile) is ONE contiguous 1 KiB wave load (16 B
// per lane) that goes straight into registers, one step ahead of its use.  Waves therefore only meet at chunk
// boundaries (two barriers per kh*kw taps) instead of once per tap.
//
// Loop nest: source -> 32-channel chunk -> tap;  K index of a (chunk, tap) weight tile in the packed
// panel = tap * Ctot + channel (same panels as the generic kernel, no re-packing).
// Summation order of an accumulator: (chunk, ky, kx, term) with term = (ah wh, ah wl, al wh 2^-11) - except in the column-major
// instantiations (CM below: the 128-column tile's dense 3x3 dil 1 split-fp16 launches), where it is (chunk, kx, ky, term).  Which of
// the two a launch takes depends on its descriptor and tile alone (fusg_conv2d_route_order reports it), never on the batch.
#pragma once
#include "conv_kernel_h3.h"
#ifndef FUSG_HALO_WAVES
#define FUSG_HALO_WAVES 2
#endif

namespace fusg {

// MODE 1 (FUSG_PREC_BF16, BASELINE configs[4]'s "bf16 MFMA conv path"): the same kernel with ONE bf16 product per
// (a, w) pair instead of three fp16 products: operands rounded to bf16 (v_cvt_pk_bf16_f32, ties to even) while the
// halo is staged, one LDS image instead of two, weights pre-rounded to bf16 in fragment order, v_mfma_f32_16x16x32_bf16
// with fp32 accumulation.  bf16 has fp32's exponent range: no scaling, no range guard.  A third of the matrix work and
// half the operand traffic; ~2^-9 relative error per operand - measured on the networks' fixtures: SSIM >= 0.9997 on
// every image output, NOT bit-exact on the hourglass's keypoint argmax, which therefore stays on f16x3
// (tests::test_reduced_precision_evidence, profiles/r02_parity.json).
// MODE 2 (FUSG_PREC_F32, the reference's own arithmetic and the range guard's fallback): the same kernel on the fp32 matrix
// instruction v_mfma_f32_16x16x4_f32 (an exact fp32 fmaf chain, 64 FLOP / clk / SIMD = the fp32 vector peak): the halo image
// holds the pre-processed activations as fp32 (128 bytes per pixel and chunk: the bytes of the (hi, lo) pair), a lane's A
// operand of the 8 instructions of a 32-channel chunk is two 16-byte reads (channels 4g .. 4g+3 and 16 + 4g .. of its pixel,
// g = lane >> 4; instruction (h, e) contracts channels {16h + 4g + e}), and the weights come from a third fragment-order
// copy [tap][chunk32][cout_pad/32][16-column half][h][64 lanes][4 floats] (pack.py: frag_f32) - again one contiguous 1 KiB
// wave load per fragment, the same 4 KiB per 32-column tile and step as the split-fp16 mode.  The matrix pipe is 16x slower
// per FLOP than in fp16, so neither LDS nor the weight stream matters here (16 KiB of reads per 4096 MFMA cycles and wave).
// K runs chunk-major here and tap-major in the generic fp32 kernel: the two agree to fp32 rounding, not bit for bit.
// MODE 3 (FUSG_PREC_F16): MODE 1's loop in fp16 - ONE fp16 product per (a, w) pair, the first of the split-fp16 mode's three: operands
// rounded to fp16 (ties to even) while the halo is staged, one LDS image, v_mfma_f32_16x16x32_f16 with fp32 accumulation.  The weights
// are the `hi` fragments of the split-fp16 copy (hi = RTN_fp16(w s_n), the `lo` fragments are skipped), so the epilogue multiplies by
// 1 / s_n and the launch keeps the split's range guard: every staged |a| feeds amax, report_range raises the status at 2^15.  11
// significant bits per operand instead of bf16's 8, at the same matrix rate and the same operand bytes.
typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));

// Diagnostic build only (-DFUSG_HALO_STAMPS on conv_halo_128.hip, tools/halo_stamps.py): s_memtime of every wave of the first 64 workgroups at
// the boundaries of each chunk (first tap issued / last tap issued / next chunk committed), into a buffer nothing else reads.
#ifdef FUSG_HALO_STAMPS
__device__ unsigned long long g_halo_stamps[64 * 4 * 40];
#define FUSG_HSTAMP(slot) do { if (blockIdx.x < 64 && (slot) < 40 && lane == 0) g_halo_stamps[(blockIdx.x * 4 + wave) * 40 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define FUSG_HSTAMP(slot) do {} while (0)
#endif

constexpr int HALO_CH = 32;          // channels per staged chunk = k per MFMA
constexpr int HALO_PP = 32;          // halo pixel pitch in halves (64 B, slots swizzled - see above)

struct HaloK {
    ConvK c;
    int kh, kw, dil, pad_h, pad_w;
    int HH, HW;                 // halo extent in (virtual) input pixels
    int RP;                     // LDS pitch of a halo row in halves (halo_row_pitch)
    int tiles_x, tiles_per_img;
    int c1k;                    // K-channels of src1 (0 if absent)
    const _Float16* wfrag;      // f16x3: [tap][chunk][cout_pad/32][16-column half][hi|lo][64 lanes][8] halves
                                // bf16:  [tap][chunk][cout_pad/32][16-column half][64 lanes][8] bf16
                                // f16 (MODE 3): the f16x3 copy, of which only the `hi` fragments are read
    const int* tile_list;       // optional: patch indices (within an image) to compute; MT = B * tile_count
    int tile_count;
    // Stride-2 k3/k4 pad-1 layers as four stride-1 convolutions of the parity sub-images x[2Y+i, 2X+j] (q = 2i+j):
    // a chunk is then (quadrant, 32 channels) with its own short tap list; LDS reads stay unit-stride.
    int s2d;                    // 1: quadrant form of a stride-2 layer (HH x HW = 10 x 18 sub-image pixels)
    int qtaps[4];               // taps of each quadrant
    int qwoff[4];               // first weight slab of each quadrant (slabs of a quadrant are consecutive)
    int qtdy[4][4], qtdx[4][4]; // halo pixel offset (rows, columns) of each (quadrant, local tap)
    int nt32;                   // cout_pad / 32
    int touch_off;              // byte offset of the L2-touch dummy region in dynamic LDS (conv_kernel.h, l2_touch)
    // Reciprocals of the prologue's divisors (launch_halo fills them): n / d == umulhi(n, ceil(2^32 / d)) for every n the
    // kernel divides (n * d < 2^32, checked on the host, which refuses the launch otherwise; 0 = the divisor is 1).  An integer division costs ~25 VALU
    // instructions on gfx950 and the prologue had 3 + NI of them per thread - a sixth of all VALU work of a 32-column
    // launch, which is VALU-issue-bound (profiles/r03_pmc_narrow_layers.txt).
    unsigned m_hw, m_nt, m_tpi, m_tx;
};

// Entry-NiN launches (conv_halo_en below, fusg_conv2d_entry_nin): the few-channel pointwise convolution that would have written
// source 0.  u: its input, NHWC-physical fp32 with at most 8 channels (strides in elements); w_in / b_in: its fusg_conv_desc.wpack
// (row pitch kpad) and bias; cin: its c0k (4 or 8).
struct EntryK {
    const float* u; long usn, ush, usw;
    const float* w_in; const float* b_in;
    int cin, kpad;
};
// first float of the entry-NiN region in dynamic LDS: behind the two halo images, 256-byte aligned
__host__ __device__ inline int en_lds_floats(int HH, int RP) { return ((2 * HH * RP * (int)sizeof(_Float16) + 255) & ~255) / 4; }
// conv_pointwise_small's chain for 4 output channels from the pixel's 8 (4) ELU'd inputs at `up`: k order 0, 4, 1, 5, 2, 6, 3, 7,
// then fmaf(acc, 1, bias).  `two` false (at most 4 input channels): that kernel's k = 4 .. 7 steps are fmaf(0, 0, acc) with an acc that
// is never -0 - identities, left out (as rp_nin of conv_respair.hip does).
__device__ __forceinline__ f32x4 en_nin(const float* up, bool two, const f32x4 (&w)[8], const f32x4 bias) {
    const f32x4 xa = *(const f32x4*)up;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (two) {
        const f32x4 xb = *(const f32x4*)(up + 4);
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

__device__ __forceinline__ void pix_offsets_yx(const ConvK& p, int b, int oy, int ox, PixOff& o) {
    long Y, X, cq = 0;
    if (p.store_mode == FUSG_STORE_D2S) { Y = 2 * oy; X = 2 * ox; }
    else if (p.store_mode == FUSG_STORE_S2D) { Y = oy >> 1; X = ox >> 1; cq = (long)(((oy & 1) << 1) | (ox & 1)) * p.Cout; }
    else { Y = (long)oy * p.osy + p.ooy[0]; X = (long)ox * p.osx + p.oox[0]; }
    o.d = b * p.dsn + Y * p.dsh + X * p.dsw + (cq + p.dst_c_off) * p.dsc;
    o.r0 = b * p.r0n + Y * p.r0h + X * p.r0w;
    o.r1 = b * p.r1n + Y * p.r1h + X * p.r1w;
}

// waves per SIMD the register allocator is asked to allow: the 128-column tile needs ~230 VGPRs (2), the narrower
// tiles far fewer - and their launches (few output channels: VUnet 32 / 64-channel layers, hourglass 1x1) are bound by
// memory latency, so more resident workgroups per CU is what they need
#ifdef FUSG_HALO_OCC
constexpr int halo_waves(int tm, int tn) { return tm * tn == 1 ? 4 : (tm * tn == 2 ? 3 : FUSG_HALO_WAVES); }
#else
constexpr int halo_waves(int, int) { return FUSG_HALO_WAVES; }
#endif

// KS > 1 ("K split over the waves", the narrow column tiles of k x k layers): the workgroup's columns are 32 * WN wide and
// its 4 / WN waves per column each compute ALL 128 pixels of the patch for every KS-th tap of every chunk; the partial
// tiles meet in LDS at the end (summed in wave order: deterministic).  Why: with the M split (round 1-2: 32 pixels x 32
// columns per wave) a (chunk, tap) step is 12 MFMAs = 192 cycles - less than the L2 round trip of the next step's weight
// fragments, and ~60 bookkeeping instructions per step - so those launches ran at an MFMA-pipe busy of 0.22-0.30
// (profiles/r03_pmc_narrow_layers.txt); here a step is 48 MFMAs like on the 128-column tile, every wave fetches different
// weight fragments, and the per-step overhead is paid a quarter as often.  It pays on small grids only (conv_igemm.hip).
// bf16 mode (and the single-pass fp16 mode, MODE 3, which has its loop): THREE (FUSG_BF16_OCC=4: four) waves per SIMD.  A bf16 step is 16 MFMAs = 256 cycles of matrix pipe per wave and ~1000 cycles of
// wave time (tools/halo_stamps.py: the gaps are the step's own instruction stream and, once per chunk, the wait behind the next chunk's halo
// gather - loads return in order); two waves per SIMD leave the pipe half idle inside the taps, a third fills it.  Needs <= 168 VGPRs (the
// instantiations that would spill keep two waves) and the epilogue's LDS detour in two halves (32 KiB per workgroup instead of 64).
#ifndef FUSG_BF16_OCC
#define FUSG_BF16_OCC 3
#endif
constexpr bool halo_bf16_dense(int tm, int wm, int pk, int ni, int mode, int ks) {
    return FUSG_BF16_OCC > 2 && (mode == 1 || mode == 3) && ks == 1 && 32 * tm * wm == 128 &&
           !(tm == 4 && ((pk == PK_AFFINE && ni >= 8) || (pk == PK_NONE && ni >= 10))) &&    // (these spill at 168 registers)
           // (MODE 3 carries the range guard's running maximum, one register more than MODE 1: these two then spill as well)
           !(mode == 3 && ni >= 10 && ((tm == 4 && pk == PK_ELU) || (tm == 2 && pk == PK_AFFINE)));
}
// (K split, MODE 3, affine, 8 items: two registers over 168 when left at two waves - asked to stay where its MODE 1 sibling is)
constexpr int halo_waves_mode(int tm, int tn, int wm, int pk, int ni, int mode, int ks) {
    return halo_bf16_dense(tm, wm, pk, ni, mode, ks) ? FUSG_BF16_OCC
         : (mode == 3 && ks == 4 && pk == PK_AFFINE && ni == 8 && FUSG_HALO_WAVES < 3) ? 3 : halo_waves(tm, tn);
}
// Tap-sparse launches (fusg_conv_desc.tap_sparse, SP below): the dense-equivalent 3x3 / 4 C_out DepthToSpace form of a 2x
// upsampling layer.  Output channel block [ph * C_out, +C_out) is phase ph = 2 py + px of the 2x2 output cell, and a phase
// reads only some low-resolution rows / columns - every other (tap, phase) block of the packed weight is zero:
//   SP 1, nn.Upsample(2, nearest) -> 3x3 pad 1:             parity 0 reads offsets {-1, 0}, parity 1 {0, +1}   (4 of 9 taps)
//   SP 2, nn.ConvTranspose2d(k3, s2, p1, output_padding 1): parity 0 reads {0},         parity 1 {0, +1}   (1, 2, 2, 4 of 9)
// C_out % 32 == 0, and every instantiation gives a wave ONE 32-column tile (TN == 1): a wave's columns lie in one phase, so
// its live taps are a wave-uniform 9-bit mask (bit 3 ky + kx) picked from this table.  Dead taps skip the weight-fragment
// loads and the MFMAs; their products are exact zeros, so the result has the bytes of the dense launch.
constexpr unsigned tap_sparse_axis(int sp, int parity) { return sp == 1 ? (parity ? 0x6u : 0x3u) : (parity ? 0x6u : 0x2u); }
constexpr unsigned tap_sparse_mask(int sp, int phase) {
    unsigned m = 0;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx)
            if (((tap_sparse_axis(sp, phase >> 1) >> ky) & 1u) && ((tap_sparse_axis(sp, phase & 1) >> kx) & 1u)) m |= 1u << (3 * ky + kx);
    return m;
}

// CM = 1 ("column-major taps", the 3x3 dil 1 launches of the 128-column tile in split-fp16 mode): within a chunk the taps are
// walked kx-outer.  The A fragment of output row i at tap (ky, kx) is the fragment of staged halo row i + ky at column shift kx,
// so for a fixed kx the three ky taps touch only 10 distinct halo rows: their (hi, lo) fragments are read from LDS ONCE into
// registers (20 ds_read_b128) and the three taps issue from them - 60 reads per chunk instead of 144.  Weights keep their
// pipeline (one tap ahead, two fragment sets) and their packed layout; only the order in which a chunk's nine slabs are
// visited changes.  Per accumulator the summation order is (chunk, kx, ky, term) instead of (chunk, ky, kx, term): a CM launch
// is deterministic and batch-invariant, but not bit-identical to the tap-major (CM = 0) launch of the same layer.
// launch_halo / launch_halo_en pick the variant on the host (halo_colmajor_ok); the kernel carries no run-time flag.
constexpr bool halo_colmajor_tile(int tm, int ks) { return tm == 4 && ks == 1; }

template <int TM, int TN, int WM, int WN, int PK, int NI, int MODE, int KS = 1, int CM = 0>
__global__ __launch_bounds__(256, halo_waves_mode(TM, TN, WM, PK, NI, MODE, KS)) void conv_halo_h3(const HaloK hk) {
    constexpr int SP = 0, EN = 0;
    const EntryK en = {};
#include "conv_kernel_halo_body.inc"
}
// the tap-sparse sibling (SP = 1, 2): its own symbols, so the dense kernels above keep theirs
template <int TM, int TN, int WM, int WN, int PK, int NI, int MODE, int KS, int SP>
__global__ __launch_bounds__(256, halo_waves_mode(TM, TN, WM, PK, NI, MODE, KS)) void conv_halo_ts(const HaloK hk) {
    static_assert(SP != 0, "conv_halo_h3 is the dense kernel");
    constexpr int EN = 0, CM = 0;
    const EntryK en = {};
#include "conv_kernel_halo_body.inc"
}
// the entry-NiN sibling (EN = 1): source 0 computed from `en.u`; the 3x3 ELU launch of the VUnet's InitBlock(6, 128) in its two forms
template <int TM, int TN, int WM, int WN, int KS, int CM = 0>
__global__ __launch_bounds__(256, FUSG_HALO_WAVES) void conv_halo_en(const HaloK hk, const EntryK en) {
    constexpr int PK = PK_ELU, NI = 6, MODE = 0, SP = 0, EN = 1;
#include "conv_kernel_halo_body.inc"
}

// LDS pitch of one halo row in halves (rows need no padding: one ds_read_b128 instruction reads one patch row)
inline int halo_row_pitch(int HW) { return HW * HALO_PP; }
inline size_t halo_lds_bytes(int HH, int HW) { return (size_t)2 * HH * halo_row_pitch(HW) * sizeof(_Float16); }
// a thread stages at most 10 16-byte items of a 32-channel chunk: halos of up to 320 pixels
inline bool halo_fits(int HH, int HW) { return HH * HW * 8 <= 2560 && halo_lds_bytes(HH, HW) <= 96 * 1024; }

// pick(ni): the instantiation for `ni` staged items per thread, or nullptr when there is none
template <int TM, int TN, int WM, int WN, int KS, class Pick>
hipError_t launch_halo_fn(const HaloK& k, dim3 grid, hipStream_t s, int pk, int mode, Pick pick,       // mode: 0 split-fp16, 1 bf16, 2 exact fp32, 3 single-pass fp16
                          HaloK* prepared = nullptr, size_t* prepared_lds = nullptr) {                  // given: fill these instead of launching
    const int HP = k.HH * k.HW;
    size_t lds = halo_lds_bytes(k.HH, k.HW);
    size_t epi = (size_t)4 * TM * 32 * TN * 32 * sizeof(float);                                                     // epilogue detour (K split: the four partial tiles)
    {   // bf16 at three waves per SIMD: the tile leaves in two halves (exactly the instantiations halo_bf16_dense() names)
        const int nit = (HP * 8 + 255) / 256 <= 6 ? 6 : ((HP * 8 + 255) / 256 <= 8 ? 8 : 10);
        if (TM >= 4 && halo_bf16_dense(TM, WM, pk, nit, mode, KS)) epi /= 2;
    }
    if (lds < epi) lds = epi;
    const int touch_off = (int)lds;
    lds += TOUCH_LDS_BYTES;
    const int ni = (HP * 8 + 255) / 256;
    if (!halo_fits(k.HH, k.HW)) return hipErrorInvalidValue;
    const void* fn = pick(ni);
    if (!fn) return hipErrorInvalidValue;
    HaloK kk = k;
    kk.RP = halo_row_pitch(k.HW);
    kk.touch_off = touch_off;
    bool fits = true;
    auto magic = [&fits](long nmax, int d) -> unsigned {       // exact for n <= nmax when nmax * d < 2^32; 0 for d == 1
        if (d < 1 || nmax * d >= (1L << 32)) fits = false;
        return d < 2 ? 0u : (unsigned)(((1UL << 32) + (unsigned long)d - 1) / (unsigned long)d);
    };
    const long ntiles = (long)grid.x;
    kk.m_hw = magic(256L * 10 + 255, k.HW);                    // pix <= (255 + 256 * (NI - 1)) >> 3, bounded loosely
    kk.m_nt = magic(ntiles, k.c.NT);
    kk.m_tpi = magic(ntiles, k.tiles_per_img);
    kk.m_tx = magic((long)k.tiles_per_img, k.tiles_x);
    if (!fits) return hipErrorInvalidValue;                    // > 2^32 / d tiles: not a shape this kernel is dispatched for
    if (prepared) { *prepared = kk; *prepared_lds = lds; return hipSuccess; }
    return launch_kernel(fn, grid, lds, 96 * 1024 + TOUCH_LDS_BYTES, kk, s);
}

// Does this launch qualify for the column-major tap order (CM above)?  Dense 3x3, dil 1, split-fp16, not the quadrant form.
inline bool halo_colmajor_ok(const HaloK& k, int mode) { return mode == 0 && k.kh == 3 && k.kw == 3 && k.dil == 1 && !k.s2d; }

// colmajor: the caller allows the column-major variant (conv_igemm.hip: on unless FUSG_NO_HALO_COLMAJOR is set)
template <int TM, int TN, int WM, int WN, int KS = 1>
hipError_t launch_halo(const HaloK& k, dim3 grid, hipStream_t s, int pk, int mode, bool colmajor = false) {
    const bool cm = colmajor && halo_colmajor_tile(TM, KS) && halo_colmajor_ok(k, mode);
    return launch_halo_fn<TM, TN, WM, WN, KS>(k, grid, s, pk, mode, [pk, mode, cm](int ni) {
        return pick_pk(pk, [ni, mode, cm](auto pkc) {
            constexpr int PK = decltype(pkc)::value;
            (void)cm;
            if constexpr (halo_colmajor_tile(TM, KS)) {            // (a 10 x 18 halo: 6 items per thread)
                if (cm) return ni <= 6 ? (const void*)conv_halo_h3<TM, TN, WM, WN, PK, 6, 0, KS, 1> : (const void*)nullptr;
            }
            auto by_ni = [ni](auto mdc) {
                constexpr int MD = decltype(mdc)::value;
                return ni <= 6 ? (const void*)conv_halo_h3<TM, TN, WM, WN, PK, 6, MD, KS>
                     : ni <= 8 ? (const void*)conv_halo_h3<TM, TN, WM, WN, PK, 8, MD, KS>
                               : (const void*)conv_halo_h3<TM, TN, WM, WN, PK, 10, MD, KS>;
            };
            return mode == 3 ? by_ni(std::integral_constant<int, 3>{})
                 : mode == 2 ? by_ni(std::integral_constant<int, 2>{}) : mode == 1 ? by_ni(std::integral_constant<int, 1>{})
                                                                                   : by_ni(std::integral_constant<int, 0>{});
        });
    });
}
// tap-sparse launches: 3x3 dil 1 only (a 10 x 18 halo: 6 items per thread), split-fp16 (mode 0) or exact fp32 (mode 2), sp 1 / 2
template <int TM, int TN, int WM, int WN, int KS = 1>
hipError_t launch_halo_ts(const HaloK& k, dim3 grid, hipStream_t s, int pk, int mode, int sp) {
    if ((mode != 0 && mode != 2) || (sp != 1 && sp != 2) || k.kh != 3 || k.kw != 3 || k.dil != 1 || k.s2d) return hipErrorInvalidValue;
    return launch_halo_fn<TM, TN, WM, WN, KS>(k, grid, s, pk, mode, [pk, mode, sp](int ni) {
        if (ni > 6) return (const void*)nullptr;
        return pick_pk(pk, [mode, sp](auto pkc) {
            constexpr int PK = decltype(pkc)::value;
            auto by_sp = [sp](auto mdc) {
                constexpr int MD = decltype(mdc)::value;
                return sp == 1 ? (const void*)conv_halo_ts<TM, TN, WM, WN, PK, 6, MD, KS, 1>
                               : (const void*)conv_halo_ts<TM, TN, WM, WN, PK, 6, MD, KS, 2>;
            };
            return mode == 2 ? by_sp(std::integral_constant<int, 2>{}) : by_sp(std::integral_constant<int, 0>{});
        });
    });
}

// entry-NiN launches: 3x3 dil 1 zero padding 1 (a 10 x 18 halo: 6 items per thread), split-fp16, ELU; the NiN's LDS region must fit
// under the epilogue's detour.  Same LDS bytes, grid and reciprocals as the dense launch it stands for.
template <int TM, int TN, int WM, int WN, int KS = 1>
hipError_t launch_halo_en(const HaloK& k, const EntryK& en, dim3 grid, hipStream_t s, bool colmajor = false) {
    if (k.kh != 3 || k.kw != 3 || k.dil != 1 || k.pad_h != 1 || k.pad_w != 1 || k.s2d || k.c1k || k.tile_list || k.c.pad_mode != FUSG_PAD_ZERO ||
        k.c.ups || !k.c.vec_epi)
        return hipErrorInvalidValue;
    const size_t need = ((size_t)en_lds_floats(k.HH, halo_row_pitch(k.HW)) + 6 * 32 * 8 + 9 * (size_t)k.c.C0) * sizeof(float);
    if (need > (size_t)4 * TM * 32 * TN * 32 * sizeof(float)) return hipErrorInvalidValue;
    HaloK kk;
    size_t lds = 0;
    const void* fn = (const void*)conv_halo_en<TM, TN, WM, WN, KS>;
    if constexpr (halo_colmajor_tile(TM, KS)) {                    // (the checks above are halo_colmajor_ok's)
        if (colmajor) fn = (const void*)conv_halo_en<TM, TN, WM, WN, KS, 1>;
    }
    const hipError_t e = launch_halo_fn<TM, TN, WM, WN, KS>(k, grid, s, PK_ELU, 0, [&](int ni) {
        return ni == 6 ? fn : (const void*)nullptr; }, &kk, &lds);
    if (e != hipSuccess) return e;
    if (hipError_t e2 = ensure_dyn_lds(fn, 96 * 1024 + TOUCH_LDS_BYTES); e2 != hipSuccess) return e2;
    void* args[] = {(void*)&kk, (void*)&en};
    return hipLaunchKernel(fn, grid, dim3(256), args, lds, s);
}

hipError_t launch_halo_128(const HaloK&, dim3, hipStream_t, int, int, bool colmajor);   // colmajor: launch_halo's
hipError_t launch_halo_64(const HaloK&, dim3, hipStream_t, int, int);
hipError_t launch_halo_32(const HaloK&, dim3, hipStream_t, int, int);
hipError_t launch_halo_32k(const HaloK&, dim3, hipStream_t, int, int);      // K split over the four waves
hipError_t launch_halo_64k(const HaloK&, dim3, hipStream_t, int, int);      // K split over two waves per 32-column tile
// the tap-sparse siblings (conv_halo_ts_*.hip); last argument: fusg_conv_desc.tap_sparse (1 / 2)
hipError_t launch_halo_ts_128(const HaloK&, dim3, hipStream_t, int, int, int);
hipError_t launch_halo_ts_64(const HaloK&, dim3, hipStream_t, int, int, int);
hipError_t launch_halo_ts_32(const HaloK&, dim3, hipStream_t, int, int, int);
hipError_t launch_halo_ts_32k(const HaloK&, dim3, hipStream_t, int, int, int);
hipError_t launch_halo_ts_64k(const HaloK&, dim3, hipStream_t, int, int, int);
// the entry-NiN siblings (conv_halo_en_*.hip): the two forms the VUnet's InitBlock(6, 128) launches
hipError_t launch_halo_en_128(const HaloK&, const EntryK&, dim3, hipStream_t, bool colmajor);
hipError_t launch_halo_en_32k(const HaloK&, const EntryK&, dim3, hipStream_t);

}  // namespace fusg
