/*
 * fusg.h - C ABI of libfusg.so: the MI355X (gfx950) kernels behind the per-vehicle novel-view
 * synthesis hot path (stacked-hourglass -> Warp&Learn ICN -> VUnet -> EdgeConnect).
 *
 * The reference (alexj94/future_urban_scene_generation) has no FFI of its own: its hot path is
 * Python nn.Module code that delegates every op to PyTorch.  The drop-in boundary
 * is therefore the Python module surface (future_urban_scene_generation_amd/{stacked_hourglass,
 * warp_learn,vunet,edgeconnect}); this header is the thin C layer those modules bind with ctypes.
 * Each entry point names the reference op(s) it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes.  No torch types.  All pointers are DEVICE pointers
 *    borrowed from the caller (e.g. tensor.data_ptr()); the library never allocates or frees
 *    caller-visible memory and keeps no mutable state besides one-time per-device caches (kernel attributes, a 256-byte zero line) and the opt-in profiler.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Every call only enqueues
 *    work on that stream; nothing synchronises, so calls are graph-capturable.
 *  - Return 0 on success, negative fusg_status otherwise; fusg_last_error() gives a thread-local
 *    message.  Shapes are validated on the host before any launch.
 *  - Tensors are described by logical NCHW extents + element strides.  "NHWC-physical" means
 *    sc == 1 (channels contiguous), sw = Cs, sh = W*Cs, sn = H*W*Cs with Cs >= c, Cs % 4 == 0 and a
 *    16-byte aligned base: the layout every conv source must have.
 */
#ifndef FUSG_H
#define FUSG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FUSG_VERSION 118

typedef enum fusg_status {
    FUSG_OK = 0,
    FUSG_ERR_INVALID = -1,   /* bad shape / stride / enum            */
    FUSG_ERR_LAUNCH = -2,    /* HIP launch or runtime error          */
    FUSG_ERR_UNSUPPORTED = -3
} fusg_status;

typedef enum fusg_dtype { FUSG_F32 = 0, FUSG_U8 = 1, FUSG_I32 = 2 } fusg_dtype;

typedef struct fusg_tensor {
    void*   data;            /* device pointer, NULL = absent */
    int64_t n, c, h, w;      /* logical NCHW extents          */
    int64_t sn, sc, sh, sw;  /* strides in elements           */
    int32_t dtype;           /* fusg_dtype                    */
    int32_t _pad;
} fusg_tensor;

/* ---- convolution ------------------------------------------------------------------------- */

typedef enum fusg_pad_mode {
    FUSG_PAD_ZERO = 0, FUSG_PAD_REFLECT = 1,
    FUSG_PAD_REPLICATE = 2     /* clamp to the edge (the phase form of nn.Upsample(2) -> ReflectionPad2d(2) ->
                                  5x5 conv, pack.py: up2_phase_weights) */
} fusg_pad_mode;

/* op applied to every in-bounds source element while the im2col tile is staged (padding stays 0) */
typedef enum fusg_pre_op {
    FUSG_PRE_NONE = 0,
    FUSG_PRE_RELU = 1,
    FUSG_PRE_ELU = 2,          /* vunet/layers.py:12-15 (Activation) applied before the conv    */
    FUSG_PRE_AFFINE_RELU = 3,  /* relu(x*scale[b,c]+shift[b,c]): eval BatchNorm / InstanceNorm /
                                  custom LayerNorm followed by ReLU, normalise-on-load          */
    FUSG_PRE_AFFINE = 4
} fusg_pre_op;

typedef enum fusg_act {
    FUSG_ACT_NONE = 0, FUSG_ACT_RELU = 1, FUSG_ACT_TANH = 2, FUSG_ACT_SIGMOID = 3,
    FUSG_ACT_TANH01 = 4,       /* (tanh(x)+1)/2, edgeconnect/networks.py:83 */
    FUSG_ACT_LEAKY02 = 5       /* v > 0 ? v : 0.2f v - nn.LeakyReLU(0.2), the discriminators'; a NaN stays a NaN */
} fusg_act;

typedef enum fusg_store_mode {
    FUSG_STORE_NORMAL = 0,
    FUSG_STORE_D2S = 1,        /* DepthToSpace(2), DCR order, vunet/layers.py:173-196 */
    FUSG_STORE_S2D = 2         /* SpaceToDepth(2), vunet/layers.py:199-221            */
} fusg_store_mode;

/* Arithmetic of the conv contraction.
 * F32:   v_mfma_f32_32x32x2_f32, exact fp32 products and accumulation (157 TFLOP/s dense peak).
 * F16X3: operands split into fp16 pairs, a*w ~= ah*wh + ah*wl + al'*(wh*2^-11) on v_mfma_f32_16x16x32_f16 (halo kernel; 32x32x16 in
 *        the generic kernels) with fp32 accumulation; al' = (a - ah)*2^11 and the weights carry a per-output-channel power-of-two scale
 *        (wscale), so every operand in fp16's normal range [2^-14, 2^15) keeps >= 22 significant bits: the
 *        error against fp64 is at or below that of an fp32 fmaf chain for operand scales 1e-4 .. 1e4
 *        (tools/emu_split.py, tests/test_gpu_ops.py::test_f16x3_scale_sweep).  3 MFMA passes at the fp16 rate.
 *        Nothing is clamped: a launch that stages an operand with |x| >= 2^15 (or an infinity) sets
 *        *status = 1 and its output is unspecified; the caller must then redo the work with F32.
 * EMU_BF16 / EMU_BF16X2: evidence paths, not production: the F32 kernel with every staged activation rounded to 8 / 16
 *        significant bits (the caller passes weights rounded the same way in `wpack`): products of such operands are
 *        exact in fp32, so this is the arithmetic of a single-pass bf16 (resp. two-piece bf16) MFMA contraction with
 *        fp32 accumulation, at fp32-MFMA speed.  Used to decide BASELINE configs[4] with data.
 * BF16:  BASELINE configs[4]'s "bf16 MFMA conv path": launches that qualify for the halo kernel (the layers that carry the
 *        FLOPs) contract in ONE bf16 product per operand pair on v_mfma_f32_16x16x32_bf16 (operands rounded to bf16 as
 *        they are staged, weights from `wfrag_bf16`, fp32 accumulation); every other launch runs as F16X3, whose
 *        fields must be given too.  Measured: SSIM >= 0.9997 on every image output of the path, keypoint argmax NOT
 *        bit-exact - the hourglass module keeps F16X3 under this setting.
 * F16:   single-pass fp16, between F16X3 and BF16: launches that qualify for the halo or the tap-unit kernel contract in ONE fp16
 *        product per operand pair - the first of F16X3's three: a' = RTN_fp16(pre_op(a)) rounded as it is staged (ties to even),
 *        w' = RTN_fp16(w * s[n]) = the `hi` half of the split weights, acc += a' * w' on v_mfma_f32_16x16x32_f16 in fp32,
 *        out = act(fmaf(acc, wscale[n], bias[n])).  11 significant bits per operand where BF16 keeps 8, at BF16's matrix rate and
 *        operand bytes, from the F16X3 fields alone: no weight copy of its own.  Activations are staged unscaled, so the 11 bits
 *        hold for staged |a| >= 2^-14; below that a' is an fp16 subnormal (gradual underflow, never flushed): an absolute 2^-25.
 *        F16X3's range guard holds unchanged (every staged operand after the pre-op and a fused ReLU's floor; |a| >= 2^15 or an
 *        infinity sets *status; nothing is clamped), and so does its NaN rule: a NaN reaches the output, or is zeroed by a fused
 *        ReLU without raising *status (csrc/conv_kernel_h3.h).  Every other launch runs as F16X3, bit for bit.  Added without a version step: two enum values, no layout change, and
 *        FUSG_VERSION 118 is what the suite pins. */
typedef enum fusg_precision { FUSG_PREC_F32 = 0, FUSG_PREC_F16X3 = 1, FUSG_PREC_EMU_BF16 = 2, FUSG_PREC_EMU_BF16X2 = 3,
                              FUSG_PREC_BF16 = 4, FUSG_PREC_F16 = 5 } fusg_precision;

typedef enum fusg_tile {       /* workgroup tile (output pixels x output channels); 0 = auto */
    FUSG_TILE_AUTO = 0, FUSG_TILE_128x128 = 1, FUSG_TILE_128x64 = 2, FUSG_TILE_128x32 = 3,
    FUSG_TILE_64x64 = 4, FUSG_TILE_64x128 = 5
} fusg_tile;

/*
 * One fused convolution launch.  Replaces, per call site, the reference's chains of
 *   [torch.cat] -> [BatchNorm2d(eval)/InstanceNorm2d/LayerNorm -> ReLU | ELU] -> [ReflectionPad2d |
 *   ZeroPad2d | nn.Upsample(2)] -> nn.Conv2d / nn.ConvTranspose2d(k4,s2,p1) -> [+bias] ->
 *   [ReLU|tanh|sigmoid] -> [+residual] -> [DepthToSpace | SpaceToDepth]
 * (stacked_hourglass/models.py:22-42; warp_learn/models.py:84-90,106-110,157-159;
 *  vunet/layers.py:33-36,98-102,140-146; edgeconnect/networks.py:41-74,184-203).
 *
 * The GEMM view is  out[m, n] = sum_k A[m, k] * W[n, k],  m = (b, qy, qx) over the "q-space"
 * output grid, k = (tap, concat-channel).  `ktab` (built at weight-pack time, see
 * future_urban_scene_generation_amd/pack.py) has one int2 per 4 consecutive k:
 *     .x = (dy & 0xffff) | (dx << 16)       input offset of the tap (includes -pad and dilation)
 *     .y = channel offset in its source | src_select << 30 | invalid << 31
 * so  A[m, k] = pre_op(src[b, qy*stride + dy, qx*stride + dx, ch])  with padding handled by
 * `pad_mode` on the virtual (optionally 2x nearest-upsampled) input.  A transposed convolution
 * is `nphase` = 4 phase-convolutions with their own tables/weights and output offsets.
 */
typedef struct fusg_conv_desc {
    fusg_tensor src0;            /* NHWC-physical f32                                          */
    fusg_tensor src1;            /* optional second source (channel concat), same n,h,w        */
    fusg_tensor dst;             /* f32, any strides; logical extents of the FINAL output      */
    fusg_tensor res0, res1;      /* optional residuals, same logical extents as dst            */
    const float*   wpack;        /* [nphase][cout_pad][k_pad]                                  */
    const float*   bias;         /* [cout_pad]                                                 */
    const int32_t* ktab;         /* [nphase][k_pad/4][2]                                       */
    const float*   pre_scale;    /* [B or 1][c0k + c1k] for the AFFINE pre-ops                 */
    const float*   pre_shift;
    int64_t        pre_bstride;  /* elements between batches in pre_scale/shift (0 = shared)   */
    float*         workspace;    /* split-K partials: nphase*ksplit*M*cout_pad floats          */
    int32_t k_pad;               /* multiple of 32                                             */
    int32_t c0k;                 /* concat channels taken from src0 (multiple of 4)            */
    int32_t cout, cout_pad;      /* cout_pad multiple of 32                                    */
    int32_t stride;              /* q-space stride (1 or 2)                                    */
    int32_t upsample;            /* 0/1: sources are read through a 2x nearest upsample        */
    int32_t pad_mode;            /* fusg_pad_mode                                              */
    int32_t pre_op;              /* fusg_pre_op                                                */
    int32_t act;                 /* fusg_act                                                   */
    int32_t store_mode;          /* fusg_store_mode                                            */
    int32_t qh, qw;              /* q-space output grid                                        */
    int32_t nphase;              /* 1, or 4 for ConvTranspose2d(k4,s2,p1)                      */
    int32_t out_sy, out_sx;      /* dst y = qy*out_sy + out_oy[phase] (NORMAL store)           */
    int32_t out_oy[4], out_ox[4];
    int32_t dst_c_off;           /* write channels [dst_c_off, dst_c_off + cout') of dst       */
    int32_t tile;                /* fusg_tile                                                  */
    int32_t ksplit;              /* <=1: no split-K                                            */
    int32_t precision;           /* fusg_precision                                             */
    const void*    wpack_h;      /* F16X3 only: [nphase][2][cout_pad][k_pad] fp16 = (hi, lo) of w * s[n]   */
    /* Optional filter geometry (0 = unknown).  When given and the layer qualifies (F16X3, stride 1 - or stride 2
     * with wfrag_order 1 -, nphase 1, source channels % 32 == 0, qh % 8 == 0, qw % 16 == 0) the halo-tiled kernel
     * is used: taps must then be the dense kh x kw grid in (ky, kx) order with
     * dy = ky*dil - pad_h, dx = kx*dil - pad_w, which is what pack.py emits. */
    int32_t kh, kw, dil, pad_h, pad_w;
    int32_t wfrag_order;         /* 0: wfrag slabs in tap order.  1 (stride 2, k3/k4, pad 1, dil 1, one source with
                                    channels % 32 == 0, even H and W): slabs grouped by the parity quadrant of the input
                                    they read (pack.py: s2d_tap_order) - the launch then runs as four stride-1
                                    convolutions of the quarter-size parity sub-images on the halo kernel (odd
                                    H or W: generic gather).
                                    2 (one source with 4..24 channels, dil 1, k x k taps): wfrag holds the weights per
                                    16-k step of the tap-unit kernel (pack.py: frag_tapunit) - the whole few-channel
                                    halo is staged once and K runs over (tap, 8- or 4-channel unit)              */
    /* Halo kernel only: the (hi, lo) fp16 weights again, in MFMA-fragment order
     * [tap][chunk32][cout_pad/32][16-column half][hi|lo][64 lanes][8 halves], lane = (k >> 3) * 16 + column
     * (pack.py: frag_f16x3) = the B operand of v_mfma_f32_16x16x32_f16, so that a fragment is one contiguous
     * 1 KiB wave load.  NULL disables the halo kernel.
     * FUSG_PREC_F16 (the halo kernel's MODE 3, the tap-unit kernel's too) reads only the `hi` fragments of this copy, in either
     * order's layout, and skips the `lo` ones; a tap-sparse copy then runs dense (its dead blocks are zeros: the same bytes). */
    const void*    wfrag;
    /* Optional fused normalisation statistics of the conv OUTPUT (bias included): per image and per
     * 32-pixel slot (slot order is kernel-defined; finalisation is order-independent) the mean and the
     * centred sum of squares of every output channel: float [B][qh*qw/32][cout][2].  Requires
     * act == NONE, no residual, NORMAL or D2S store (D2S: slots per stacked column, cout of them), nphase 1,
     * ksplit <= 1, qh*qw % 32 == 0 and a
     * channel-contiguous 16-byte aligned dst with cout % 4 == 0 (else FUSG_ERR_UNSUPPORTED).
     * Feed to fusg_in_finalize_slots / fusg_ln_finalize_slots. */
    float*         stats_out;
    /* Optional (halo-kernel launches only, else FUSG_ERR_UNSUPPORTED): compute only these 8 x 16-pixel
     * patches of every image - indices into the row-major (qh/8) x (qw/16) patch grid, device memory. */
    const int32_t* tile_list;
    int32_t        tile_count;
    /* Origin of the computed qh x qw window in q-space (default 0, 0): output pixel (qy, qx) of the launch is
     * pixel (q_oy + qy, q_ox + qx) of the full convolution - lets a launch compute one edge row or column. */
    int32_t        q_oy, q_ox;
    /* Slots per image in stats_out (0 = qh*qw/32): lets several launches that each cover part of an image (the four
     * phase launches of a transposed convolution) write disjoint slot ranges of one buffer - offset the stats_out
     * pointer by first_slot*cout*2 floats. */
    int32_t        stats_slots;
    /* F16X3 only.  wscale[cout_pad] = 1 / s[n], s[n] the power of two the channel's weights were multiplied by
     * before the (hi, lo) split (pack.py: split_f16x3); the epilogue computes acc * wscale[n] + bias[n].
     * status: one device int32 (caller-owned, zeroed by the caller), set to 1 by the launch when an operand is
     * outside the split's range - see fusg_precision.  Sticky: the library never clears it. */
    const float*   wscale;
    int32_t*       status;
    /* FUSG_PREC_BF16 only: the weights rounded to bf16 (ties to even) in the halo kernel's fragment order
     * [tap][chunk32][cout_pad/32][16-column half][64 lanes][8 bf16], same tap order as `wfrag` (pack.py: frag_bf16).
     * NULL: the launch runs as F16X3.
     * With wfrag_order 2 (few-channel stems) it holds the tap-unit form instead: [k-step][cout_pad/32][64 lanes][8 bf16], the
     * `wfrag` layout of that order without the (hi | lo) axis (pack.py: frag_tapunit_bf16). */
    const void*    wfrag_bf16;
    /* FUSG_PREC_F32, optional: the fp32 weights in the halo kernel's fragment order for v_mfma_f32_16x16x4_f32,
     * [tap][chunk32][cout_pad/32][16-column half][h][64 lanes][4 floats] with lane = g * 16 + column holding
     * w[column][32 chunk + 16 h + 4 g + e], e = 0..3, same tap order as `wfrag` (pack.py: frag_f32).  Given (with the
     * filter geometry above), a qualifying FUSG_PREC_F32 launch runs on the halo kernel in exact fp32 instead of the
     * generic gather; NULL keeps the generic gather.
     * With wfrag_order 2 (few-channel stems) it holds the tap-unit form instead: [unit of 4 channels][cout_pad/32][64 lanes][2]
     * floats, lane = g * 32 + column holding w[column][4 unit + g], w[column][4 unit + 2 + g] (pack.py: frag_tapunit_f32). */
    const void*    wfrag_f32;
    /* Optional, split-K launches: `splitk_counters_len` device int32 words that are ZERO when the launch starts (the
     * launch leaves them zero).  Given, the workgroup that finishes a tile's last K-slice sums the slices (in slice
     * order: bit-reproducible) and applies the epilogue inside the same launch; NULL, a second kernel does. */
    int32_t*       splitk_counters;
    int32_t        splitk_counters_len;
    /* Tap sparsity of the packed weights (0 = none; this word was padding, so 0 is every older caller): the descriptor is
     * the dense-equivalent 3x3 / pad 1 / stride 1 DepthToSpace form of a 2x upsampling layer with C_out = cout / 4 output
     * channels, phase 2 py + px of the 2 x 2 output cell in channel block [phase * C_out, +C_out), and whole (tap, phase)
     * blocks of the weights are zero:
     *   1  nn.Upsample(2, nearest) -> Conv2d(k3, p1) (pack.py: pack_conv_up2_nearest_d2s): 4 live taps of 9 per phase;
     *   2  nn.ConvTranspose2d(k3, s2, p1, output_padding 1) (pack_conv_transpose_k3s2p1op1_d2s): 1, 2, 2, 4 live taps.
     * Requires kh = kw = 3, zero padding 1, stride 1, dil 1, no upsample, D2S store, nphase 1, cout % 128 == 0 (C_out % 32 == 0) and
     * cout_pad == cout, else FUSG_ERR_UNSUPPORTED.  A launch that takes the halo kernel in F16X3 or exact F32 then skips the
     * weight loads and MFMAs of the dead taps (same bytes as the dense launch: the skipped products are exact zeros); every
     * other route - the generic gather, the small-image kernel, FUSG_PREC_BF16 with wfrag_bf16 given - runs the dense weights,
     * which are correct by construction.  FUSG_PREC_BF16 without wfrag_bf16 runs as F16X3, tap-sparse. */
    int32_t        tap_sparse;
} fusg_conv_desc;

int  fusg_conv2d(const fusg_conv_desc* d, void* stream);
/* Heuristic used when tile == AUTO / to size the workspace: fills tile, ksplit and returns the
 * workspace size in bytes (0 when ksplit <= 1). */
int64_t fusg_conv2d_plan(fusg_conv_desc* d);
/* Dry run of fusg_conv2d: the FUSG_CONV_* family it would launch for this descriptor, or the negative FUSG_ERR_* it would
 * return.  Launches nothing and touches no device; the split-K workspace (the caller's allocation) is not checked. */
int  fusg_conv2d_route(const fusg_conv_desc* d);

/*
 * Routing batch (batch-invariant routing; added without a version step: the entry points are new, nothing existing changed
 * and 0, the default, is the behaviour before them launch for launch).
 * Which kernel family a convolution runs on, its tile and its K split - hence the order of its sums, hence its bits - depend
 * on how many images share the launch.  With a routing batch R > 0 every such CHOICE is made as if the launch held R images,
 * whatever it holds: the tile and ksplit of fusg_conv2d_plan, the column tile and the K split over the waves of the halo
 * kernel (fusg_conv2d, fusg_conv2d_route, fusg_conv2d_entry_nin[_route]), and tap_order 0 of fusg_vunet_respair.  Grids,
 * workspace bytes (the chosen ksplit times the REAL M) and every bounds check keep describing the real launch.  The arithmetic
 * applied to one image then does not depend on its neighbours; R equal to the real batch is the default behaviour at that batch.
 * fusg_hg_bottleneck and the small-image kernel sum per image whatever the grid and read no routing batch.
 * The value is process-wide and read whenever a launch is planned or routed; a launch recorded into a fusg_plan is re-issued
 * under the value it was recorded with.  Do not change it while another thread issues or plans launches.
 * fusg_set_route_batch: n = 0 turns the mode off, 1 .. 2^20 sets it and the PREVIOUS value (>= 0) is returned; a negative or
 * larger n changes nothing and returns FUSG_ERR_INVALID with a message.  fusg_route_batch: the current value.
 */
int     fusg_set_route_batch(int32_t n);
int32_t fusg_route_batch(void);
/* Dry run like fusg_conv2d_route (no launch, no device): what fixes the summation order of the launch fusg_conv2d would make
 * of this descriptor - out = {family (FUSG_CONV_*), tile, ksplit, ksw}.  tile: the FUSG_TILE_* of the generic gathers, the
 * column-tile width (128 / 64 / 32) of the halo and tap-unit kernels, 0 for the others; ksplit: K ranges over workgroups
 * (generic gathers and the small-image kernel; 1 elsewhere); ksw: 1 when the halo kernel splits K over its waves, 2 when
 * its 128-column tile walks a chunk's 3x3 taps column-major (the FUSG_NO_HALO_COLMAJOR environment switch, read per call,
 * keeps them tap-major: 0).
 * Returns FUSG_OK or the negative FUSG_ERR_* fusg_conv2d would return. */
int  fusg_conv2d_route_order(const fusg_conv_desc* d, int32_t out[4]);

/*
 * One pre-activation Bottleneck of the stacked hourglass in ONE launch (split-fp16 arithmetic, FUSG_PREC_F16X3):
 *   out = res + conv3_1x1( relu(bn3( conv2_3x3( relu(bn2( conv1_1x1( relu(bn1(x)) ))) ))) )
 * (stacked_hourglass/models.py:22-42; bn2 / bn3 are folded into conv1 / conv2 at pack time, bn1 is the per-channel
 * affine `pre_scale`, `pre_shift`; `res` is x itself or the block's 1x1 `downsample` conv of x, models.py:37-38).
 * planes P is 128 (every Bottleneck of the hourglass levels, `layer2`, `layer3` and `res`) or 64 (`layer1`): conv1
 * Cin -> P, conv2 P -> P, conv3 P -> 2 P; x has Cin % 32 == 0 channels, res and dst 2 P.
 * A workgroup owns an 8 x 8 pixel patch: conv1 is evaluated on the patch's 10 x 10 halo (zero outside the image, as
 * conv2's zero padding requires), its output and conv2's never leave LDS (already split into fp16 pairs), so the
 * block reads x and res once and writes out once - the three launches it replaces move 2.2x the bytes and, on the
 * hourglass's 4 x 4 .. 16 x 16 levels, are bound by launch-to-launch latency.
 * Weights: the `wfrag` copy (fusg_conv_desc.wfrag, wfrag_order 0) of each of the three convolutions, their `bias`
 * [cout_pad] and `wscale` [cout_pad] arrays.  Same range contract as F16X3 launches: *status = 1 when an operand
 * (bn1 output, or either intermediate) is outside the split's range; the caller then redoes the work in F32 with
 * three fusg_conv2d calls.  x, res, dst: NHWC-physical f32, same n, h, w.
 */
typedef struct fusg_bneck_desc {
    fusg_tensor x, res, dst;
    const float* pre_scale;      /* [Cin] bn1 as y = x * scale + shift, then ReLU               */
    const float* pre_shift;
    const void*  w1frag; const float* bias1; const float* wscale1;     /* conv1 (+bn2): Cin -> P, 1x1    */
    const void*  w2frag; const float* bias2; const float* wscale2;     /* conv2 (+bn3): P -> P, 3x3      */
    const void*  w3frag; const float* bias3; const float* wscale3;     /* conv3: P -> 2 P, 1x1           */
    int32_t*     status;
    int32_t      planes;         /* P: 64 or 128 */
    int32_t      exact_f32;      /* 0: split-fp16 (w*frag = the fusg_conv_desc.wfrag copies; wscale* and status required).
                                    1 (round 4): exact fp32 on v_mfma_f32_16x16x4_f32 - w*frag = the fusg_conv_desc.wfrag_f32
                                    copies (pack.py: frag_f32), wscale* and status unused */
} fusg_bneck_desc;
int fusg_hg_bottleneck(const fusg_bneck_desc* d, void* stream);

/*
 * Two Residuals of the VUnet's 32-channel shape-encoder levels and the two skip NiNs that read them, in ONE launch
 * (split-fp16 arithmetic, FUSG_PREC_F16X3; csrc/conv_respair.hip):
 *   x0 = entry ? NiN_in(elu(u)) + bias_in : x
 *   s0 = convA_3x3(elu(x0)) + biasA + x0,   s1 = convB_3x3(elu(s0)) + biasB + s0        (zero padding 1)
 *   kb = conv_b_1x1(elu(s0)) + bias_b,      kc = conv_c_1x1(elu(s1)) + bias_c
 * s1, kb and kc are written; x0 and s0 stay in the workgroup (vunet/models.py: InitBlock + shape_skip_1_b/c with entry = 1,
 * the two Residuals of DownBlock 1_a + shape_skip_1_a_b/c with entry = 0).  The results are bit for bit those of the five
 * (four) fusg_conv2d launches of the block.
 * x: entry = 0: [n, 32, h, w]; entry = 1: u, [n, <= 8, h, w] as the few-channel pointwise launch takes it (w_in = that NiN's
 * fusg_conv_desc.wpack with row pitch kpad_in, cin = its c0k, bias_in = its bias).  h % 8 == 0, w % 16 == 0.  All tensors
 * NHWC-physical f32; no output may alias x or another output.
 * Weights: the `wfrag` copy (wfrag_order 0), `bias` and `wscale` of the four 32 -> 32 convolutions.
 * tap_order: which of the halo kernel's two summation orders the 3x3 convolutions follow - 0: the one fusg_conv2d gives the
 * unfused launches at this grid size (K split over the waves on grids of at most 1024 patches), 1: taps in order, 2: split.
 * Same range contract as F16X3 launches: *status = 1 when a staged operand (elu of x0, s0 or s1) is outside the split's range.
 */
typedef struct fusg_respair_desc {
    fusg_tensor x, s1, kb, kc;
    const float* w_in; const float* bias_in;                                /* entry NiN (entry = 1)      */
    const void*  wfragA;  const float* biasA;  const float* wscaleA;        /* first Residual's 3x3       */
    const void*  wfragB;  const float* biasB;  const float* wscaleB;        /* second Residual's 3x3      */
    const void*  wfrag_b; const float* bias_b; const float* wscale_b;       /* skip NiN of s0             */
    const void*  wfrag_c; const float* bias_c; const float* wscale_c;       /* skip NiN of s1             */
    int32_t*     status;
    int32_t      channels;       /* 32 */
    int32_t      entry;
    int32_t      cin, kpad_in;
    int32_t      tap_order;
    int32_t      _pad;
} fusg_respair_desc;
int fusg_vunet_respair(const fusg_respair_desc* d, void* stream);

/*
 * The entry of the VUnet's InitBlock(6, 128) (vunet/models.py: app_encoder_1) as ONE halo launch (csrc/conv_kernel_halo.h,
 * conv_halo_en; added without a version step: the entry points are new, nothing existing changed):
 *   x0 = NiN(elu(u)) + bias_in          1x1 from at most 8 channels - never written
 *   dst = conv3x3(elu(x0)) + bias + x0  zero padding 1
 * `nin`: the descriptor of the NiN as fusg_conv2d would take it (src0 = u, FUSG_PRE_ELU, F16X3; its dst is ignored) - a launch
 * the router puts on the pointwise kernel.  `res`: the descriptor of the 3x3 Residual as fusg_conv2d would take it (FUSG_PRE_ELU,
 * F16X3, k3 stride 1 pad 1 dil 1, zero padding, one source of nin.cout = cout = 128 channels); its src0 and res0 are ignored -
 * both are x0, whose shape is dst's.  The halo staging computes x0 with the pointwise kernel's fp32 chain, pixels outside the
 * image are staged as zero, and the epilogue adds the same chain on the patch's own pixels: dst has the bytes of the two
 * launches, and *res.status is raised as the Residual's own launch raises it.
 * fusg_conv2d_entry_nin_route: 0 - this pair does not fuse (fusg_conv2d_entry_nin then returns FUSG_ERR_UNSUPPORTED); 1 - the
 * 128-column tile, M split over the waves; 2 - the 32-column tile, K split over the waves: the form fusg_conv2d gives the
 * Residual at this grid size (grids for which it picks another form stay two launches); negative: FUSG_ERR_*.  No device work.
 */
int fusg_conv2d_entry_nin(const fusg_conv_desc* res, const fusg_conv_desc* nin, void* stream);
int fusg_conv2d_entry_nin_route(const fusg_conv_desc* res, const fusg_conv_desc* nin);

/*
 * The 1x1 head that ends a stack of the hourglass in ONE launch (split-fp16 arithmetic, FUSG_PREC_F16X3; csrc/conv_hghead.hip;
 * added without a version step: the entry points are new, nothing existing changed, and FUSG_VERSION 118 is what the suite pins):
 *   y     = relu(fc_1x1(y_in) + bias_fc)            256 -> 256 (the fc BatchNorm folded at pack time) - never written
 *   score = score_1x1(y) + bias_score               256 -> cout_pad 32; channels [0, score.c) are written
 *   dst   = x + join_1x1(cat[y, score]) + bias_join 288 -> 256                                    (join = 1 only)
 * (stacked_hourglass/models.py: fc, score, and x + fc_(y) + score_(score) as one two-source convolution.)  join = 1 wants
 * score.c == 32 - the score filter zero-padded to 32 output channels, so that the launch writes the padding as exact zeros on
 * every call and `score` is the join's 32-channel second source; join = 0 (the last stack) stops after score.
 * Weights: the `wfrag` copy (fusg_conv_desc.wfrag, wfrag_order 0) of each convolution, their `bias` [cout_pad] and `wscale`
 * [cout_pad] arrays.  y_in, x, dst: NHWC-physical f32 [n, 256, h, w]; score [n, <= 32, h, w].  score and dst have the bytes of
 * the three fusg_conv2d launches on the halo kernel (a 1x1 launch has one summation order there at every batch size).  Same range
 * contract as F16X3 launches: *status = 1 when a staged operand (y_in, y, or score in the join form) is outside the split's range.
 */
typedef struct fusg_hg_head_desc {
    fusg_tensor y_in, x, score, dst;
    const void*  wfrag_fc;    const float* bias_fc;    const float* wscale_fc;
    const void*  wfrag_score; const float* bias_score; const float* wscale_score;
    const void*  wfrag_join;  const float* bias_join;  const float* wscale_join;    /* join = 1 */
    int32_t*     status;
    int32_t      join;
    int32_t      _pad;
} fusg_hg_head_desc;
int fusg_hg_head(const fusg_hg_head_desc* d, void* stream);

/* Load-time weight pre-packing on the HOST (no device work): everything fusg_conv_desc needs for one nn.Conv2d-style
 * filter weight[cout][cin][kh][kw] (torch layout, correlation form) whose input channels come from one source (c0 = cin)
 * or from two concatenated sources (the first c0 channels from src0: torch.cat([x, skip], 1) fused into the gather).
 * The Python modules do the same in future_urban_scene_generation_amd/pack.py (plus the reference-specific folds of
 * weight_norm / spectral_norm / eval BatchNorm, which are a few lines of arithmetic on the weights before this call:
 * vunet/layers.py:29-31, edgeconnect/networks.py:206-210, stacked_hourglass/models.py:11-16); the two are tested
 * against each other bit for bit.  Call fusg_pack_conv_sizes, allocate, call fusg_pack_conv_weights, upload. */
typedef struct fusg_pack_spec {
    int32_t cout, cin, kh, kw;
    int32_t c0;                  /* input channels taken from src0 (cin if there is one source)            */
    int32_t stride, pad, dil;    /* as nn.Conv2d; the taps are dy = ky*dil - pad, dx = kx*dil - pad        */
    int32_t upsample;            /* 1: the conv reads its sources through a 2x nearest upsample            */
    int32_t cin_pad;             /* K-channels of each source are padded to a multiple of this (4; 32 to make a
                                    few-channel layer eligible for the halo kernel)                        */
} fusg_pack_spec;
typedef struct fusg_pack_sizes {
    int32_t cout_pad, k_pad, c0k, c1k;   /* the fusg_conv_desc fields of the same names (c1k: K-channels of src1)   */
    int32_t wfrag_order;                 /* -1: no fragment-order copy (generic gather only), else fusg_conv_desc.wfrag_order */
    int32_t _pad;
    int64_t wpack_floats;                /* cout_pad * k_pad                                                        */
    int64_t ktab_ints;                   /* (k_pad / 4) * 2                                                         */
    int64_t wpack_h_halves;              /* 2 * cout_pad * k_pad                                                    */
    int64_t wfrag_halves;                /* 0 when wfrag_order < 0                                                  */
} fusg_pack_sizes;
int fusg_pack_conv_sizes(const fusg_pack_spec* spec, fusg_pack_sizes* sizes);
/* All pointers are HOST buffers of the sizes above (bias may be NULL = no bias; wfrag NULL = skip the copy);
 * bias_pad and wscale hold cout_pad floats; fp16 data is written as raw uint16 bit patterns. */
int fusg_pack_conv_weights(const fusg_pack_spec* spec, const float* weight, const float* bias, float* wpack, int32_t* ktab,
                           float* bias_pad, uint16_t* wpack_h, float* wscale, uint16_t* wfrag);

/* ---- normalisation statistics -------------------------------------------------------------- */

/* Per-(b, c) shifted sums over H*W in `nchunk` deterministic partials:
 * partial[b][chunk][c] = { sum(x - p), sum((x - p)^2) },  p = x[b, 0, 0, c].   x NHWC-physical. */
int fusg_chan_stats(const fusg_tensor* x, float* partial, int32_t nchunk, void* stream);
/* nn.InstanceNorm2d(affine=False, eps) statistics (warp_learn/models.py:56; edgeconnect/
 * networks.py:44): scale[b,c] = rstd, shift[b,c] = -mean*rstd (biased variance). */
int fusg_in_finalize(const fusg_tensor* x, const float* partial, int32_t nchunk, float eps,
                     float* scale, float* shift, void* stream);
/* Custom LayerNorm (warp_learn/models.py:26-35): per-sample mean and UNBIASED std over C*H*W,
 * eps added to std: scale[b,c] = gamma[c]/(std+eps), shift[b,c] = beta[c] - mean*scale[b,c]. */
int fusg_ln_finalize(const fusg_tensor* x, const float* partial, int32_t nchunk, float eps,
                     const float* gamma, const float* beta, float* scale, float* shift, void* stream);

/* The same two finalisations from the slot statistics a conv launch produced (fusg_conv_desc.stats_out):
 * slots [B][nslots][C][2] = (mean, centred M2) over 32 pixels each, combined in fp64 (Chan et al.). */
int fusg_in_finalize_slots(const float* slots, int32_t batch, int32_t nslots, int32_t channels, float eps,
                           float* scale, float* shift, void* stream);
int fusg_ln_finalize_slots(const float* slots, int32_t batch, int32_t nslots, int32_t channels, float eps,
                           const float* gamma, const float* beta, float* scale, float* shift, void* stream);

/* ---- border ring of nn.Upsample(2) -> ReflectionPad2d(2) -> 5x5 after the phase-form launch (new entry points, FUSG_VERSION
 * stays 118: nothing existing changed its layout, and 118 is what the suite pins) ---------------------------------------------
 * The phase-form launch (3x3 on the low-res input, edge-replicate padding, DepthToSpace store) equals the 5x5 convolution of the
 * REPLICATE-padded upsampled image.  fusg_up2_edge_fix adds, in place, the 5x5 convolution of (reflect-padded - replicate-padded),
 * which is non-zero on the outermost ring of output pixels only and uses only the taps on the padding frame (csrc/up2_edge.h).
 *   src     low-res source [B, Cin, h, w], NHWC-physical, Cin % 32 == 0, h, w >= 2
 *   pre_op  FUSG_PRE_NONE or FUSG_PRE_AFFINE_RELU with scale / shift [b * pre_bstride + c], as fusg_conv_desc takes them
 *   wedge   the frame taps in fp32, [4 sides][5 taps][Cin/16][Cout/16][64][4] (pack.pack_conv_up2_edge)
 *   dst     the phase-form output [B, Cout, 2h, 2w], NHWC-physical, Cout % 16 == 0, Cout <= 256; ring pixels become old + delta
 *   delta   NULL, or [B][n_entries][2] doubles: per workgroup (sum of delta, sum of delta * (2 old + delta)) over its pixels, the
 *           change of the image's sum and sum of squares; n_entries = fusg_up2_edge_entries(h, w)
 * Exact fp32 arithmetic (v_mfma_f32_16x16x4_f32) whatever the precision of the phase launch; no range guard.  Two launches on the
 * stream (rows, then columns); work split and summation orders depend on (h, w, Cin, Cout) only. */
int fusg_up2_edge_entries(int32_t h, int32_t w);
int fusg_up2_edge_fix(const fusg_tensor* src, int32_t pre_op, const float* pre_scale, const float* pre_shift, int64_t pre_bstride,
                      const float* wedge, const fusg_tensor* dst, double* delta, int32_t n_entries, void* stream);
/* fusg_ln_finalize_slots of slots over `columns` stacked columns (a DepthToSpace launch: 4 * channels of them, the same multiset of
 * values) whose image then changed by fusg_up2_edge_fix: the sum of `delta`'s first entries is added to the sum and of its second
 * entries to the sum of squares before mean and unbiased std.  gamma / beta / scale / shift have `channels` entries. */
int fusg_ln_finalize_slots_delta(const float* slots, int32_t batch, int32_t nslots, int32_t columns, int32_t channels, float eps,
                                 const float* gamma, const float* beta, const double* delta, int32_t n_entries,
                                 float* scale, float* shift, void* stream);

/* ---- elementwise / data movement ------------------------------------------------------------ */

/* dst = act(x*scale[b,c] + shift[b,c]) + res  (scale may be NULL: identity).  NHWC-physical.
 * InstanceNorm apply + residual of ResBlock / ResnetBlock (warp_learn/models.py:106-110;
 * edgeconnect/networks.py:198-199). */
int fusg_affine_act(const fusg_tensor* x, const float* scale, const float* shift, int64_t bstride,
                    int32_t act, const fusg_tensor* res, const fusg_tensor* dst, void* stream);
/* F.max_pool2d(x, 2, stride=2) (stacked_hourglass/models.py:72,149), a NaN in the window included: the
 * result is then NaN.  NHWC-physical. */
int fusg_maxpool2(const fusg_tensor* x, const fusg_tensor* dst, void* stream);
/* dst = up1 + nearest_upsample2(low) (stacked_hourglass/models.py:81-82).  NHWC-physical. */
int fusg_upsample2_add(const fusg_tensor* low, const fusg_tensor* up1, const fusg_tensor* dst, void* stream);
/* Generic strided copy dst[b,c,y,x] = src[b,c,y,x]; channels [src.c, dst_c_fill) of dst are
 * zero-filled (NCHW <-> NHWC conversion with channel padding at the module boundary). */
int fusg_copy4d(const fusg_tensor* src, const fusg_tensor* dst, int32_t dst_c_fill, void* stream);
/* dst = a + b with arbitrary strides (Sampler: mu + CPU-drawn noise, vunet/layers.py:166). */
int fusg_add4d(const fusg_tensor* a, const fusg_tensor* b, const fusg_tensor* dst, void* stream);
/* SpaceToDepth(2) / DepthToSpace(2), DCR order (vunet/layers.py:173-221). NHWC-physical; dst may
 * be a channel slice of a wider buffer. */
int fusg_space_to_depth2(const fusg_tensor* x, const fusg_tensor* dst, void* stream);
int fusg_depth_to_space2(const fusg_tensor* x, const fusg_tensor* dst, void* stream);
/* EdgeModel / InpaintingModel input assembly (edgeconnect/models.py:130-133, 236-238):
 * mode 0: dst = cat(images*(1-m)+m, edges*(1-m), m)      images [B,1,H,W] -> dst [B,3(+pad),H,W]
 * mode 1: dst = cat(images*(1-m)+m, edges)               images [B,3,H,W] -> dst [B,4,H,W]    */
int fusg_ec_inputs(const fusg_tensor* images, const fusg_tensor* edges, const fusg_tensor* masks,
                   const fusg_tensor* dst, int32_t mode, void* stream);
/* Second half of the "row-split" small-Cout convolution: a kh x kw conv with cout*kw <= 32 is run
 * as a kh x 1 implicit GEMM producing t[b, co*kw + kx, y, x] = sum_{ky,c} in[y+ky-pad, x, c]*w[co,c,ky,kx]
 * (kw x fewer MFMA flops than padding cout to 32), then
 *   dst[b, co, y, x] = act(bias[co] + sum_kx t[b, co*kw + kx, y, pad_x(x + kx - pad)])
 * with zero / reflect handling of the horizontal border.  t NHWC-physical, dst any strides.
 * The taps are added in fp32 in ascending kx, starting from the bias.  Accepted: 1 <= kw <= 15, 0 <= pad < W,
 * cout*kw <= t.c, and a window that holds its own pixel and fits the row: kw - 1 - pad >= 0, and with reflect
 * padding kw - 1 - pad < W (the right overshoot reflects inside the row like the left one); anything else is
 * FUSG_ERR_INVALID.  A window reaching further right than left (kw - 1 > 2*pad) is served by the direct kernel.
 * Used for the 7x7 heads (warp_learn/models.py:182-183; edgeconnect/networks.py:72-73,123-124). */
int fusg_hshift_sum(const fusg_tensor* t, const float* bias, int32_t kw, int32_t pad, int32_t pad_mode,
                    int32_t act, const fusg_tensor* dst, void* stream);
/* Row-major first-occurrence argmax over H*W per (b, c) -> idx[b*C + c] = y*W + x (int32).
 * Integer contract of get_maxima (utils/keypoint_utils.py:85-88).  A map of equal values (all -inf included)
 * gives 0.  Unspecified for a map that holds a NaN. */
int fusg_argmax_hw(const fusg_tensor* x, int32_t* idx, void* stream);
/* to_image(from_LAB=False) quantiser (warp_learn/planes_utils.py:111-114):
 * u8[b,y,x,c] = trunc(clip((x+1)/2*255, 0, 255)).  dst is a U8 tensor described as NCHW extents
 * with HWC strides. */
int fusg_to_image_u8(const fusg_tensor* x, const fusg_tensor* dst, void* stream);
/* merged = out*m + img*(1-m); u8 = trunc(merged*255) (trajectory_inference.py:126-129). */
int fusg_merge_u8(const fusg_tensor* out, const fusg_tensor* img, const fusg_tensor* mask,
                  const fusg_tensor* dst, void* stream);

/* ---- OpenCV-defined uint8 steps around the ICN (device versions; parity unpinned, see oracle/cv_host.py) ------- */
/* U8 images are fusg_tensors with dtype FUSG_U8, logical [n, 3, h, w] and HWC strides (sc = 1, sw >= 3).           */

/* cv2.warpPerspective(src, H, dsize=(w, h)) with INTER_LINEAR / BORDER_CONSTANT 0 (warp_learn/planes_utils.py:76-77)
 * for n images at once: minv = n row-major 3x3 DOUBLE matrices in DEVICE memory, each the INVERSE of that image's H
 * (OpenCV inverts H on the host too).  Coordinates in double, rounded to 1/32 pixel, 15-bit bilinear weights,
 * (sum + 2^14) >> 15.  src and dst may differ in h, w. */
int fusg_warp_perspective_u8(const fusg_tensor* src, const double* minv, const fusg_tensor* dst, void* stream);
/* The same for a list of jobs inside two image stacks (every plane of every vehicle of a frame in one launch,
 * pipeline.VehiclePipeline.run_frame): job k warps image index[2k] of src with minv[k] into image index[2k + 1] of dst;
 * index = DEVICE int32 [jobs][2]; images of dst no job names are left untouched (the caller zero-fills them:
 * planes_utils.py:57 starts from zeros). */
int fusg_warp_perspective_indexed_u8(const fusg_tensor* src, const double* minv, const int32_t* index, int32_t jobs,
                                     const fusg_tensor* dst, void* stream);
/* The same for the F future frames of a clip that share ONE set of source planes (VehiclePipeline.run_later_frames_batched):
 * src holds the S = src->n planes of the first frame, dst frames * S images; job k reads image index[2k] % S of src and
 * writes image index[2k + 1] of dst, so a table fitted for frames * V vehicles (fusg_plane_homographies: row = (f * V + v) * P
 * + j, source row * P + i) addresses the shared planes as it stands and no copy of them per frame is made.  frames >= 1,
 * jobs <= frames * S, index and minv not NULL (checked on the host before the launch). */
int fusg_warp_perspective_frames_u8(const fusg_tensor* src, const double* minv, const int32_t* index, int32_t jobs,
                                    int32_t frames, const fusg_tensor* dst, void* stream);
/* get_planes (warp_learn/planes_utils.py:11-37): dst[p] = frame * fillPoly(polygon p) for up to 8 polygons of up
 * to 8 int32 vertices.  pts_xy [nplanes][8][2] (x, y) and nverts [nplanes] are HOST arrays (read before return). */
int fusg_fill_poly_planes_u8(const fusg_tensor* frame, const int32_t* pts_xy, const int32_t* nverts, int32_t nplanes,
                             const fusg_tensor* dst, void* stream);
/* get_planes for n_jobs vehicles in one launch: dst[j * n_planes + p] = frame * fillPoly(polygon (j, p)), the bytes of
 * fusg_fill_poly_planes_u8 called once per job.  pts_xy = DEVICE int32 [n_jobs, n_planes, 8, 2] (x, y), nverts = DEVICE
 * int32 [n_jobs, n_planes] (<= 8), n_planes 1..8, n_jobs * n_planes <= 65535; frame uint8 [h, w, 3]; dst uint8
 * [n_jobs * n_planes, h, w, 3] with contiguous rows (sw = 3, sh = 3w).  n_jobs = 0 is a no-op. */
int fusg_fill_poly_planes_batch_u8(const fusg_tensor* frame, const int32_t* pts_xy, const int32_t* nverts, int32_t n_jobs,
                                   int32_t n_planes, const fusg_tensor* dst, void* stream);
/* get_icn_inputs (warp_learn/models.py:323-366) for a batch of B vehicles: sketch [B] (RGB), central [B] (RGB, already
 * dst.h x dst.w), planes [B * P] (BGR, P <= 6, same frame size as sketch); geom = DEVICE int32 [B][8] =
 * (x0, y0, x1, y1, pad_x_before, pad_y_before, pad_x_after, pad_y_after) of square_crop_from_bbox
 * (utils/crop_utils.py:27-50).  Crop of the zero-padded frame -> cv2.resize INTER_LINEAR -> RGB/BGR2LAB (8-bit integer
 * path) -> (v/255 - 0.5)/0.5, written to dst f32 NHWC-physical [B, 3 * (P + 2), h, w] in the reference's channel
 * order (sketch, central, planes). */
int fusg_icn_inputs(const fusg_tensor* sketch, const fusg_tensor* central, const fusg_tensor* planes, const int32_t* geom,
                    const fusg_tensor* dst, void* stream);
/* cv2.cvtColor(x, COLOR_LAB2BGR) on uint8 (to_image(from_LAB=True), warp_learn/planes_utils.py:117). */
int fusg_lab2bgr_u8(const fusg_tensor* src, const fusg_tensor* dst, void* stream);
/* Resize-back + order-dependent masked paste (trajectory_inference.py:184-198) of V network images net [V] (u8,
 * e.g. 256 x 256) into ONE frame: a frame pixel covered by paste masks takes, from the LAST covering vehicle, that
 * vehicle's image resized (cv2.resize INTER_LINEAR) to its crop, padding removed, placed at crop_xy_min - or 0 where
 * the pixel lies outside that rectangle; masks u8 [V, 1, H, W] (non-zero = paste), geom as in fusg_icn_inputs. */
int fusg_paste_back_u8(const fusg_tensor* net, const fusg_tensor* masks, const int32_t* geom, const fusg_tensor* frame, void* stream);
/* The same with --inpaint (trajectory_inference.py:107-145): vehicle v first writes its inpainted box image rect[v] (u8,
 * EdgeConnect's merged output * 255, :126-129), resized (cv2.resize INTER_LINEAR, :130-131) to the rectangle rect_geom[v] =
 * (x0, y0, x1, y1, -, -, -, -) = bbox_new_img, unmasked into the running composite (:140-143), then pastes its masked
 * network image as above (:184-198); vehicles in index order, the last layer covering a pixel wins.  rect / rect_geom
 * (DEVICE int32 [V][8]) both NULL = fusg_paste_back_u8. */
int fusg_paste_layers_u8(const fusg_tensor* net, const fusg_tensor* masks, const int32_t* geom, const fusg_tensor* rect,
                         const int32_t* rect_geom, const fusg_tensor* frame, void* stream);
/* fusg_paste_layers_u8 for F frames of V vehicles each in ONE launch: net, masks, geom (and rect, rect_geom, both NULL for
 * the plain paste) hold frames * V rows, frame-major (row f * V + v = frame f, vehicle v); within a frame the rule is
 * unchanged - vehicle by vehicle, the box first, then the masked crop, the last layer covering a pixel wins.  bases = DEVICE
 * table of `frames` pointers, bases[f] = the dense u8 [H, W, 3] image frame f's composite starts from (read only); dst u8
 * [frames, H, W, 3] is written whole: the covering layer, or the base's pixel.  Checked on the host before the launch:
 * frames >= 1, row counts that are frames * V, geom / bases not NULL, rect with rect_geom. */
int fusg_paste_layers_frames_u8(const fusg_tensor* net, const fusg_tensor* masks, const int32_t* geom, const fusg_tensor* rect,
                                const int32_t* rect_geom, const void* const* bases, int32_t frames, const fusg_tensor* dst,
                                void* stream);

/* ---- frame-chain glue (pipeline.VehiclePipeline.run_frame): the uint8 -> float steps between the frame and the networks */
/* square_crop_from_bbox (utils/crop_utils.py:4-52) + cv2.resize INTER_LINEAR for V windows: src u8 HWC [1] (every
 * window cut from the same image: the frame, trajectory_inference.py:58-60) or [V] (one image per window: the central
 * crop of each vehicle's resized box, warp_learn/vehicle_utils.py:49-52); geom = DEVICE int32 [V][8] as in fusg_icn_inputs;
 * dst [V, 3, h, w].  mode 0: u8 HWC.  mode 1: f32 NHWC-physical, transforms.ToTensor + normalize: (v / 255 - mean[c]) /
 * std[c] (trajectory_inference.py:61-64; mean3 / std3 = HOST arrays of 3 floats, read before return).  mode 2: f32
 * NHWC-physical, to_tensor: v / 255 * 2 - 1 (utils/misc_utils.py:35-49).  A window of zero extent writes zeros. */
int fusg_crop_resize_u8(const fusg_tensor* src, const int32_t* geom, const fusg_tensor* dst, int32_t mode,
                        const float* mean3, const float* std3, void* stream);
/* The VUnet's first-frame inputs (trajectory_inference.py:203-228) for V vehicles: frame u8 HWC [1, 3, H, W]; masks u8
 * [V, 1, H, W] (non-zero = vehicle: the reference's ~src_sketch_mask); src_sketch / dst_sketch u8 HWC [V, 3, H, W];
 * geom = DEVICE int32 [V][8], the square window of each mask's bounding box (fusg_mask_bbox_geom).  Writes
 * x [V, 6, h, w] = cat[to_tensor(resize(crop(frame * mask))), to_tensor(resize(crop(src_sketch))[..., ::-1])] with
 * masked-frame pixels set to 255 where the resized src sketch is all zero, and y [V, 3, h, w] =
 * to_tensor(resize(crop(dst_sketch))[..., ::-1]); both f32 NHWC-physical. */
int fusg_vunet_inputs(const fusg_tensor* frame, const fusg_tensor* masks, const fusg_tensor* src_sketch,
                      const fusg_tensor* dst_sketch, const int32_t* geom, const fusg_tensor* x, const fusg_tensor* y, void* stream);
/* np.nonzero(mask) -> (x_min, y_min, x_max, y_max) (warp_learn/models.py:333-336; trajectory_inference.py:204-206) and
 * the square_crop_from_bbox geometry of that box (utils/crop_utils.py:13-50, Python's float arithmetic in double) for V
 * masks u8 [V, 1, H, W], entirely on the device: bbox = DEVICE int32 [V][4], geom = DEVICE int32 [V][8].  An empty mask
 * gives an all-zero geom row (the reference raises there and skips the vehicle). */
int fusg_mask_bbox_geom(const fusg_tensor* masks, int32_t* bbox, int32_t* geom, void* stream);
/* Heat-map argmax indices -> keypoints in frame pixels (utils/keypoint_utils.py:66-92 after F.interpolate to 256 =
 * (x0 / hm_w, y0 / hm_h); trajectory_inference.py:95-97: * crop side + crop_min - pad, in float64), stored float32
 * [V][nkp][2] - the pose fit's input.  idx = DEVICE int32 [V][nkp] (fusg_argmax_hw), geom as above (the detector
 * box's crop). */
int fusg_keypoints_to_frame(const int32_t* idx, const int32_t* geom, float* out, int32_t vehicles, int32_t nkp,
                            int32_t hm_w, int32_t hm_h, void* stream);

/* ---- frame-indexed glue (pipeline.VehiclePipeline.run_frames_batched: the first frames of several scenes as ONE pass; added
 * without a version step: the entry points are new, nothing existing changed, and FUSG_VERSION 118 is what the suite pins).
 * The three entry points above that read the frame, with the frame a property of the ROW.  Two HOST tables, read before the call
 * returns and handed to the kernel by value: frames = n_frames pointers to dense u8 [H, W, 3] DEVICE images; frame_rows =
 * n_frames + 1 non-decreasing offsets from 0 to `rows`, rows [frame_rows[f], frame_rows[f + 1]) read frame f.  Checked on the
 * host before anything is launched: 1 <= n_frames <= FUSG_MAX_FRAMES, no null pointer, offsets monotone from 0 to rows, every
 * row count equal, rect with rect_geom (a table in device memory could not be checked, and a wrong one is an out-of-bounds
 * read).  The per-pixel arithmetic is that of the one-frame entry points: same bytes. */
#define FUSG_MAX_FRAMES 64
/* fusg_crop_resize_u8 for rows = dst->n windows cut from n_frames images of H x W; modes, mean3 / std3, geom (DEVICE int32
 * [rows][8]) and dst as there.  rows == 0: no launch, returns 0. */
int fusg_crop_resize_frames_u8(const void* const* frames, const int32_t* frame_rows, int32_t n_frames, int32_t H, int32_t W,
                               const int32_t* geom, const fusg_tensor* dst, int32_t mode, const float* mean3, const float* std3,
                               void* stream);
/* fusg_vunet_inputs with the same tables: masks [rows, 1, H, W], src_sketch / dst_sketch [rows], geom [rows][8], x [rows, 6, h,
 * w], y [rows, 3, h, w].  rows == 0: no launch, returns 0. */
int fusg_vunet_inputs_frames(const void* const* frames, const int32_t* frame_rows, int32_t n_frames, const fusg_tensor* masks,
                             const fusg_tensor* src_sketch, const fusg_tensor* dst_sketch, const int32_t* geom,
                             const fusg_tensor* x, const fusg_tensor* y, void* stream);
/* fusg_paste_layers_frames_u8 with another number of layers per frame: frame f's layers are rows [frame_rows[f], frame_rows[f +
 * 1]) of net, masks, geom (and rect, rect_geom: both NULL for the plain paste), in row order, the last covering layer wins.
 * bases = HOST table of n_frames DEVICE pointers, bases[f] = the dense u8 [H, W, 3] image frame f starts from (read only, must
 * not overlap dst); dst u8 [n_frames, H, W, 3] is written whole; a frame without layers is a copy of its base. */
int fusg_paste_layers_ragged_u8(const fusg_tensor* net, const fusg_tensor* masks, const int32_t* geom, const fusg_tensor* rect,
                                const int32_t* rect_geom, const void* const* bases, const int32_t* frame_rows, int32_t n_frames,
                                const fusg_tensor* dst, void* stream);

/* fusg_fill_poly_planes_batch_u8 with the same tables, the rows being JOBS (VehiclePipeline.run_frames_batched_geometry; a new
 * entry point, FUSG_VERSION stays 118): jobs [frame_rows[f], frame_rows[f + 1]) read frame f, dst[j * n_planes + p] =
 * frames[frame of j] * fillPoly(polygon (j, p)).  pts_xy DEVICE int32 [n_jobs][n_planes][8][2], nverts DEVICE int32
 * [n_jobs][n_planes], n_planes in 1..8, n_jobs * n_planes <= 65535, dst u8 [n_jobs * n_planes, H, W, 3] with contiguous rows,
 * not overlapping a frame.  A frame without jobs is not read.  n_jobs == 0: no launch, returns 0. */
int fusg_fill_poly_planes_frames_u8(const void* const* frames, const int32_t* frame_rows, int32_t n_frames, int32_t H, int32_t W,
                                    const int32_t* pts_xy, const int32_t* nverts, int32_t n_jobs, int32_t n_planes,
                                    const fusg_tensor* dst, void* stream);

/* fusg_warp_perspective_frames_u8 with the source stack a property of the DESTINATION image (VehiclePipeline.
 * run_later_clips_batched: the future frames of several clips as ONE pass; a new entry point, FUSG_VERSION stays 118).  Three HOST
 * tables, read before the call returns and handed to the kernel by value: srcs[c] = DEVICE pointer to clip c's dense u8
 * [src_images[c], H, W, 3] source planes; dst_first = n_clips + 1 non-decreasing offsets from 0 to dst->n, clip c owns destination
 * images [dst_first[c], dst_first[c + 1]) - a multiple of src_images[c] (frames * planes), 0 where src_images[c] is 0.  minv
 * (double [jobs][9]) and index (int32 [jobs][2]) are DEVICE tables as above: job k writes image d = index[2k + 1] of dst from image
 * (index[2k] - dst_first[c]) mod src_images[c] (non-negative) of srcs[c], c the clip that owns d - so a table fitted for all rows
 * of the call (source row * P + i) and a compact one (dst_first[c] + v * P + i) both address each clip's own planes.  A job with
 * index[2k] < 0 or d outside [0, dst->n) writes nothing; images no job names are left untouched.  Checked on the host before
 * anything is launched: 1 <= n_clips <= FUSG_MAX_FRAMES, no null source where src_images[c] > 0, src_images[c] >= 0, the offsets,
 * dst dense u8 [n, H, W, 3] overlapping no source, jobs <= dst->n (and <= 65535), index and minv not NULL when jobs > 0.  jobs == 0
 * or dst->n == 0: no launch, returns 0.  The per-pixel arithmetic is fusg_warp_perspective_u8's: same bytes. */
int fusg_warp_perspective_clips_u8(const void* const* srcs, const int32_t* src_images, const int32_t* dst_first, int32_t n_clips,
                                   int32_t H, int32_t W, const double* minv, const int32_t* index, int32_t jobs,
                                   const fusg_tensor* dst, void* stream);

/* ---- pose fit ------------------------------------------------------------------------------- */
/*
 * The reference's pose fit ("CamPoseCalib": Levenberg-Marquardt on a Rodrigues vector + translation, utils/cpc.py:45-139
 * with the iteration / lambda policies of utils/pnp_utils.py:8-41), batched: one GPU thread per (vehicle, start).
 * utils/pnp_utils.py:43-115 (cpc_rodr_4_angles) runs it from four fixed start rotations per vehicle, each run ~52
 * iterations of 12 autograd backward passes on the host (5 s per vehicle measured); here all vehicles and starts of a
 * frame are one launch.  Reference behaviour kept: float32; only the first min(6, npoints) points enter the Jacobian
 * (cpc.py:30) while all points enter the cost and the returned error; every step is accepted; the loop ends when
 * iteration > max_iter (reference: 50).  Device arrays, row-major:
 *   points3d [B][npoints][3], points2d [B][npoints][2], focals [B][2], centers [B][2]   (npoints <= 16)
 *   rvec0 [nstarts][3], tvec0 [3]                                                       start parameters
 *   rvec, tvec [B][nstarts][3], err [B][nstarts]   (err = mean squared residual of the last evaluated iteration)
 * The choice of the best start and the sign flip of pnp_utils.py:117-130 are a few host operations on these outputs
 * (future_urban_scene_generation_amd/utils/pnp_utils.py).
 */
int fusg_pnp_cpc(const float* points3d, const float* points2d, const float* focals, const float* centers,
                 const float* rvec0, const float* tvec0, int32_t B, int32_t npoints, int32_t nstarts, int32_t max_iter,
                 float* rvec, float* tvec, float* err, void* stream);

/* ---- per-vehicle geometry (device versions of the reference's Open3D render and compute_visibility; parity with
 * Open3D / OpenCV unpinned) ------------------------------------------------------------------------------ */
/* One render job: a bank mesh (vertices [v_off, v_off + nv), triangles [t_off, t_off + nt) of the bank arrays, triangle
 * indices local to the mesh) moved as p = v @ R + tr (row vector, R = z_rot(theta): trajectory_inference.py:363), put in
 * the camera as Xc = E[0:3, 0:3] p + E[0:3, 3] and projected with fx, fy, cx, cy (the caller passes Open3D's principal
 * point, render_open3d.py:20).  240 bytes; fusg_sizeof_render_job() gives the compiled size. */
typedef struct fusg_render_job {
    double R[9], tr[3], E[12];
    double fx, fy, cx, cy;
    int32_t v_off, nv, t_off, nt;
} fusg_render_job;
/* get_rendered (warp_learn/render_open3d.py:29-49) for n_jobs posed meshes at once: a triangle rasteriser writing
 * sketch uint8 [n_jobs, h, w, 3] = round(255 * (n + 1) / 2) of the perspective-correct interpolated vertex normal of the
 * nearest triangle (0 where no triangle covers the pixel) and mask uint8 [n_jobs, h, w] = 1 where one does (the
 * complement of the reference's object_mask).  Pixel centres at integer (x, y), coordinates snapped to 1/256 px, int64
 * edge functions with the top-left rule, no back-face culling, depth ties to the lower triangle index; a triangle with
 * a vertex at Zc <= 1e-3 is dropped (no near-plane clipping).  verts / normals = DEVICE float64 [n_verts, 3] (normals:
 * unit vertex normals of the unmoved mesh, rotated by R per job); tris = DEVICE int32 [n_tris, 3]; jobs = DEVICE
 * fusg_render_job [n_jobs] with nv <= max_nv; workspace = DEVICE, 16-byte aligned, n_jobs * (16 + 40 * max_nv) bytes.
 * Optional (NULL = not written): tri_id int32 [n_jobs, h, w] = the winning triangle's index within its mesh (-1: none),
 * covered int32 [n_jobs] = covered pixels per job.  Deterministic: the bytes do not depend on scheduling. */
int fusg_render_normals_u8(const double* verts, const double* normals, int64_t n_verts, const int32_t* tris, int64_t n_tris,
                           const fusg_render_job* jobs, int32_t n_jobs, int32_t max_nv, int32_t h, int32_t w,
                           void* workspace, int64_t workspace_bytes, uint8_t* sketch, uint8_t* mask, int32_t* tri_id,
                           int32_t* covered, void* stream);
/* The areas of compute_visibility (warp_learn/online_visibility.py:105-150) for 7 planes per job (left, right, roof,
 * front, back, front_bt, back_bt): counts int32 [n_jobs, 7, 2] = (absolute, occluded), absolute = pixels of the h x w
 * frame inside or on polygon p, occluded = those of them in no polygon q whose bit is set in nearer[p] (the planes
 * nearer the camera).  Membership is the rule of fusg_fill_poly_planes_u8.  pts_xy = DEVICE int32 [n_jobs, 7, 8, 2],
 * nverts = DEVICE int32 [n_jobs, 7] (<= 8), nearer = DEVICE int32 [n_jobs, 7]; counts are zeroed by the call. */
int fusg_plane_visibility(const int32_t* pts_xy, const int32_t* nverts, const int32_t* nearer, int32_t n_jobs, int32_t h,
                          int32_t w, int32_t* counts, void* stream);
int fusg_sizeof_render_job(void);

/* ---- plane homographies (the stage between the plane corner points and fusg_warp_perspective_indexed_u8) ---------- */
/* warp_jobs + find_homography (warp_learn/planes_utils.py) + the slot rule and the inversion of warp_planes_batch for V
 * vehicles of P <= 8 planes in one launch.  DEVICE inputs: src_pts / dst_pts int32 [V][P][8][2] (corner points, padded),
 * nverts int32 [P] (corner points of plane p; a fit needs 4..8 and equal counts on both sides), src_vis / dst_vis uint8
 * [V][P] (0 / 1).  sym_a, sym_b: the two symmetric planes (left, right), or -1, -1.  Per vehicle and source plane i:
 * i is warped when it is visible in the source and its destination is visible - its own slot i, or, for a symmetric
 * plane whose own destination is hidden, its partner's slot; H12 (src -> dst) and H21 (dst -> src) are fitted in double
 * (normalised DLT through a cyclic Jacobi eigen-decomposition, Levenberg-Marquardt for more than 4 points) and the job
 * exists when both fits and the inverse of H12 are valid; of two jobs on one slot the higher plane index wins.
 * DEVICE outputs, one row per (vehicle, destination slot), row = v * P + j:
 *   minv double [V * P][9]   inverse of the winning H12 (zeros: no job)
 *   index int32 [V * P][2]   (source image v * P + i, or -1: no job; destination image = row) - with minv the arguments of
 *                            fusg_warp_perspective_indexed_u8(jobs = V * P), which skips the rows of source -1
 *   H double [V][P][2][9]    optional (NULL): the winning job's H12, H21 (zeros: no job)
 *   status int32 [V][P]      optional (NULL): 0 no plane gated onto the slot, 1 job, 2 gated but no valid fit
 * V = 0 launches nothing.  Results are bit-identical to fusg_plane_homographies_host (the same code, no contraction). */
int fusg_plane_homographies(const int32_t* src_pts, const int32_t* dst_pts, const int32_t* nverts, const uint8_t* src_vis,
                            const uint8_t* dst_vis, int32_t V, int32_t P, int32_t sym_a, int32_t sym_b, double* minv,
                            int32_t* index, double* H, int32_t* status, void* stream);
/* The same tables computed on the CPU from HOST arrays (no GPU needed). */
int fusg_plane_homographies_host(const int32_t* src_pts, const int32_t* dst_pts, const int32_t* nverts, const uint8_t* src_vis,
                                 const uint8_t* dst_vis, int32_t V, int32_t P, int32_t sym_a, int32_t sym_b, double* minv,
                                 int32_t* index, double* H, int32_t* status);
/* One fit on the CPU: src_xy / dst_xy HOST double [n][2] -> H_out [9] (H[8] = 1) and, when minv_out is not NULL, its
 * inverse.  Returns 1, or 0 where planes_utils.find_homography returns None (n < 4, a zero deviation, rank loss) or H
 * is singular; the outputs are zeros then. */
int fusg_find_homography_host(const double* src_xy, const double* dst_xy, int32_t n, double* H_out, double* minv_out);

/* ---- pose geometry (geometry mode's glue between fusg_pnp_cpc and the render; added without a version step: FUSG_VERSION
 * stays 118, the entry points are new and nothing existing changed) ------------------------------------------------- */
/* Per vehicle, what the frame driver computed in numpy between the pose fit and the render, in the same operation order
 * (csrc/pose_geometry.h): select_and_flip of the four starts (np.argmin: first index on ties, the first NaN wins; sign
 * flip through Rodrigues in float64, the result rounded to float32), the extrinsic [R(rvec) | tvec] (carried in the
 * pose's float32), on a later frame the keypoints moved by kp3d @ z_rot(theta) + tr and projected with K, the texture-plane
 * corner points (x / W * W, y / H * H, truncated), the seven visibility polygons (projected with K @ E[:3], clipped to
 * +-2^20 px, truncated, INT32_MIN for NaN) with their "nearer" masks, and the render job record, Open3D's principal point
 * (W / 2 - 0.5, H / 2 - 0.5) and v_off, nv, t_off, nt from the bank's offset tables.
 * A first frame passes the raw fit rvec / tvec float32 [V][4][3], err float32 [V][4] and kp_xy float32 [V][12][2] (frame
 * pixels) with pose_in = steps = NULL; a later frame passes pose_in float32 [V][7] (a first frame's `pose`) and steps
 * double [V][4] = (theta, tr) with rvec = tvec = err = kp_xy = NULL.  cad_idx int64 [V]; the bank: bank_kp3d float32
 * [n_cad][12][3], bank_v_off / bank_t_off int32 [n_cad + 1] (cumulative vertex / triangle counts).  All of these are
 * DEVICE pointers; K = HOST double [9] (row-major intrinsics), h, w = the frame.
 * DEVICE outputs: pose float32 [V][7] (error, rvec, tvec), extrinsic double [V][12] (rows of [R | t]), kp3d double
 * [V][12][3] (moved on a later frame), jobs [V], vis_pts int32 [V][7][8][2], vis_nv / nearer int32 [V][7] (the arguments
 * of fusg_plane_visibility), tex_pts int32 [V][5][8][2], tex_nv int32 [V][5] (those of fusg_fill_poly_planes_batch_u8 and
 * fusg_plane_homographies), status int32 [V]: 0, or 1 = cad_idx outside [0, n_cad) - that vehicle gets zero keypoints and
 * an empty job (nv = nt = 0) and the bank is not read for it.
 * V = 0 launches nothing.  NULL or inconsistent arguments: FUSG_ERR_INVALID before any launch.  One thread per vehicle. */
int fusg_pose_geometry(const float* rvec, const float* tvec, const float* err, const float* pose_in, const float* kp_xy,
                       const double* steps, const int64_t* cad_idx, const float* bank_kp3d, const int32_t* bank_v_off,
                       const int32_t* bank_t_off, int32_t n_cad, const double* K, int32_t h, int32_t w, int32_t V, float* pose,
                       double* extrinsic, double* kp3d, fusg_render_job* jobs, int32_t* vis_pts, int32_t* vis_nv, int32_t* nearer,
                       int32_t* tex_pts, int32_t* tex_nv, int32_t* status, void* stream);
/* The same code on the CPU for HOST arrays (no GPU needed). */
int fusg_pose_geometry_host(const float* rvec, const float* tvec, const float* err, const float* pose_in, const float* kp_xy,
                            const double* steps, const int64_t* cad_idx, const float* bank_kp3d, const int32_t* bank_v_off,
                            const int32_t* bank_t_off, int32_t n_cad, const double* K, int32_t h, int32_t w, int32_t V, float* pose,
                            double* extrinsic, double* kp3d, fusg_render_job* jobs, int32_t* vis_pts, int32_t* vis_nv,
                            int32_t* nearer, int32_t* tex_pts, int32_t* tex_nv, int32_t* status);

/* The later-frame branch of fusg_pose_geometry for J rows of SEVERAL clips in ONE launch (VehiclePipeline.
 * run_later_clips_batched_geometry; new entry points, FUSG_VERSION stays 118).  Rows are clip-major, frame-major inside a clip: row
 * row_first[c] + f * vehicles[c] + v is clip c, frame f, vehicle v.  Five HOST tables, read and checked before the call returns and
 * handed to the kernel by value: poses[c] = DEVICE float32 [V_c][7] (a first frame's `pose`), cad_idxs[c] = DEVICE int64 [V_c],
 * src_pts[c] = DEVICE int32 [V_c][5][8][2] (the first frame's texture-plane corner points), vehicles[c] = V_c, row_first = n_clips + 1
 * non-decreasing offsets from 0 to J - clip c owns a multiple of V_c rows, 0 where V_c is 0.  DEVICE inputs: steps double [J][4] =
 * (theta, tr) per row, cams double [n_clips][9] = the row-major intrinsics of each clip's camera (in device memory: the tables
 * already take 2.3 KB of the 4 KB kernel-argument space), the bank as above.
 * DEVICE outputs: those of fusg_pose_geometry at J rows, and src_pts_rows int32 [J][5][8][2] = each row's source corner points
 * copied from its clip's table - the src_pts of fusg_plane_homographies for all rows.  A row is bit for bit what fusg_pose_geometry
 * gives for that vehicle with its clip's K (the same code: csrc/pose_geometry.h).
 * FUSG_ERR_INVALID before any launch: n_clips outside 1..FUSG_MAX_FRAMES, J outside 0 .. 2^20 - 1, a null host table, offsets that
 * do not start at 0, decrease or do not end at J, a row count that is no multiple of V_c, a clip that owns rows with a null table
 * entry; with J > 0 also a null device pointer or h, w, n_cad < 1.  J = 0 launches nothing.  One thread per row, ordinary stores. */
int fusg_pose_geometry_clips(const float* const* poses, const int64_t* const* cad_idxs, const int32_t* const* src_pts,
                             const int32_t* vehicles, const int32_t* row_first, int32_t n_clips, const double* steps,
                             const double* cams, const float* bank_kp3d, const int32_t* bank_v_off, const int32_t* bank_t_off,
                             int32_t n_cad, int32_t h, int32_t w, int32_t J, float* pose, double* extrinsic, double* kp3d,
                             fusg_render_job* jobs, int32_t* vis_pts, int32_t* vis_nv, int32_t* nearer, int32_t* tex_pts,
                             int32_t* tex_nv, int32_t* status, int32_t* src_pts_rows, void* stream);
/* The same code on the CPU: every pointer, the tables' entries included, is a HOST pointer (no GPU needed). */
int fusg_pose_geometry_clips_host(const float* const* poses, const int64_t* const* cad_idxs, const int32_t* const* src_pts,
                                  const int32_t* vehicles, const int32_t* row_first, int32_t n_clips, const double* steps,
                                  const double* cams, const float* bank_kp3d, const int32_t* bank_v_off, const int32_t* bank_t_off,
                                  int32_t n_cad, int32_t h, int32_t w, int32_t J, float* pose, double* extrinsic, double* kp3d,
                                  fusg_render_job* jobs, int32_t* vis_pts, int32_t* vis_nv, int32_t* nearer, int32_t* tex_pts,
                                  int32_t* tex_nv, int32_t* status, int32_t* src_pts_rows);

/* ---- the later-frame gate (the tail of a geometry-mode later frame's device stage; like the pose geometry added without a
 * version step: the entry points are new, nothing existing changed, and FUSG_VERSION 118 is what the suite pins) ------- */
/* The tail of a later frame's geometry stage, without a read-back: for J (frame, vehicle) rows
 *   valid[j]      = covered[j] > 0
 *   dst_vis[j][p] = valid[j] && (double)counts[j][p][1] > 0.9 * (double)counts[j][p][0]      p < P <= 7
 *   box_rows[j][0..7] = 0 where !valid[j]   (optional, in place; NULL: none)
 * counts = DEVICE int32 [J][7][2] (fusg_plane_visibility: absolute, occluded), covered = DEVICE int32 [J]
 * (fusg_render_normals_u8); DEVICE outputs dst_vis uint8 [J][P] (0 / 1: the dst_vis of fusg_plane_homographies), valid int32
 * [J], box_rows int32 [J][8] (the box rows of fusg_paste_layers_frames_u8).  The comparison is render.visible's float64
 * expression - one multiply, one compare, no contraction -, so an empty plane (0 > 0) is not visible.
 * J = 0 launches nothing; NULL / P outside 1..7 / J < 0 (or >= 2^20): FUSG_ERR_INVALID before any launch.  One thread per
 * (row, slot of 8), ordinary stores; bit-identical to the host twin (the same code). */
int fusg_later_gate(const int32_t* counts, const int32_t* covered, int32_t J, int32_t P, uint8_t* dst_vis, int32_t* valid,
                    int32_t* box_rows, void* stream);
/* The same code on the CPU for HOST arrays (no GPU needed). */
int fusg_later_gate_host(const int32_t* counts, const int32_t* covered, int32_t J, int32_t P, uint8_t* dst_vis, int32_t* valid,
                         int32_t* box_rows);

/* ---- EdgeConnect's inputs from a detector mask (create_inpaint_inputs_shape, utils/inpaint_utils.py:35-58; like the pose
 * geometry added without a version step: the entry points are new, nothing existing changed, and FUSG_VERSION 118 is what
 * the suite pins) ------------------------------------------------------------------------------------------------------ */
/* Per vehicle v: the detector mask inside the box is dilated by OpenCV's 8 x 8 ellipse (pixels outside the box do not
 * exist), box pixels under a dilated 255 turn white, the box and the dilated mask are resized to 256 x 256 (cv::resize
 * INTER_LINEAR), gray is taken from the resized image, the mask is binarised and scikit-image's Canny runs on gray with
 * the hole masked out - the definition, step by step, heads csrc/inpaint_inputs.h.
 * frame: u8 HWC (n = 1, c = 3); det_masks: u8 [V, 1, H, W] in frame coordinates (non-zero = vehicle; read only inside
 * the box); boxes: DEVICE int32 [V][4] = (x0, y0, x1, y1), half-open; gauss_w: HOST double [radius + 1], the one-sided
 * normalised Gaussian table (copied at the call), radius = int(4 sigma + 0.5) in 0..32; max_box_h / max_box_w: the
 * largest box extents, what the scratch was sized for (the boxes live on the device, so the host cannot look) - a box
 * that exceeds them or leaves the frame is treated as a zero-extent box.  Outputs, f32 with any strides: img
 * [V, 3, 256, 256] and gray [V, 1, 256, 256] = v / 255, mask and edge [V, 1, 256, 256] exactly 0 or 1; a zero-extent
 * box writes zeros to all four.  scratch: DEVICE, 16-byte aligned, the bytes the size query returns; it holds nothing between calls.
 * Shapes and arguments are checked on the host before any launch (FUSG_ERR_INVALID); V = 0 launches nothing.  Five
 * launches, grid.y = V, no atomics; bit-identical to the host twin (the same code, no contraction). */
int fusg_inpaint_inputs(const fusg_tensor* frame, const fusg_tensor* det_masks, const int32_t* boxes, const double* gauss_w,
                        int32_t radius, int32_t max_box_h, int32_t max_box_w, const fusg_tensor* img, const fusg_tensor* gray,
                        const fusg_tensor* edge, const fusg_tensor* mask, void* scratch, void* stream);
/* Bytes of scratch for V vehicles whose boxes are at most max_box_h x max_box_w; -1 for a negative argument. */
int64_t fusg_inpaint_inputs_scratch_bytes(int32_t V, int32_t max_box_h, int32_t max_box_w);
/* The same code on the CPU in plain loops: every pointer (boxes and scratch too) is a HOST pointer, no GPU needed.  It can
 * see the boxes, so one that leaves the frame or exceeds max_box_h x max_box_w is refused (FUSG_ERR_INVALID). */
int fusg_inpaint_inputs_host(const fusg_tensor* frame, const fusg_tensor* det_masks, const int32_t* boxes, const double* gauss_w,
                             int32_t radius, int32_t max_box_h, int32_t max_box_w, const fusg_tensor* img, const fusg_tensor* gray,
                             const fusg_tensor* edge, const fusg_tensor* mask, void* scratch);

/* The same with the detector's masks in BOX coordinates, as Mask R-CNN run on the box crop returns them
 * (trajectory_inference.py:113-119, :316-324) - also added without a version step.  The arguments are those of
 * fusg_inpaint_inputs with det_masks replaced by box_masks: ONE packed DEVICE buffer of n_elems elements of mask_dtype
 * (FUSG_U8: the byte as it is, non-zero = vehicle and only a dilated 255 whitens, as above; FUSG_F32: the reference's
 * binarisation m * 255 > 0 ? 255 : 0, so a NaN gives 0), and offsets: DEVICE int64 [V] - vehicle v's mask is row-major
 * [bh][bw] from element offsets[v], bh x bw its box as clipped above.  V is img's n.  The boxes and offsets live on the
 * device: a vehicle whose offset is negative or whose offsets[v] + bh * bw exceeds n_elems is treated as a zero-extent box
 * (zeros to all four outputs) and is never read.  Only the dilation's tile fill reads the masks; everything behind that
 * pixel, the scratch and its size query are those of fusg_inpaint_inputs.  Bit-identical to the host twin. */
int fusg_inpaint_inputs_boxed(const fusg_tensor* frame, const void* box_masks, int32_t mask_dtype, int64_t n_elems,
                              const int64_t* offsets, const int32_t* boxes, const double* gauss_w, int32_t radius,
                              int32_t max_box_h, int32_t max_box_w, const fusg_tensor* img, const fusg_tensor* gray,
                              const fusg_tensor* edge, const fusg_tensor* mask, void* scratch, void* stream);
/* The same code on the CPU: every pointer is a HOST pointer.  It can see the boxes and offsets, so a mask that would leave
 * the buffer is refused (FUSG_ERR_INVALID) like a box that leaves the frame. */
int fusg_inpaint_inputs_boxed_host(const fusg_tensor* frame, const void* box_masks, int32_t mask_dtype, int64_t n_elems,
                                   const int64_t* offsets, const int32_t* boxes, const double* gauss_w, int32_t radius,
                                   int32_t max_box_h, int32_t max_box_w, const fusg_tensor* img, const fusg_tensor* gray,
                                   const fusg_tensor* edge, const fusg_tensor* mask, void* scratch);

/* ---- per-image quality metrics (the quantity the project's quality bars are stated in, for the product's user; added
 * without a version step: the entry points are new, nothing existing changed, and FUSG_VERSION 118 is what the suite pins) */
/* a, b: u8 [B, C, H, W] descriptors of any strides (the NHWC layout of the pipeline's uint8 crops included), the same
 * shape, C in 1..4, H and W in 11..32767, B < 65536.  out: DEVICE float64 [B][6]; row r =
 *   0 ssim     mean SSIM of image r over its channels and its (H - 10) x (W - 10) valid positions: 11 x 11 Gaussian window
 *              of sigma 1.5 (outer product of the normalised 1-D taps), K1 = 0.01, K2 = 0.03, data range 255
 *   1 mse      sse / (H W C)
 *   2 psnr     10 log10(255^2 / mse) dB, +inf when sse = 0
 *   3 max_abs  largest |a - b|               4 n_diff  number of differing values        5 sse  sum of (a - b)^2
 * Columns 3..5 are exact integers.  The window sums and everything behind them are float64 (csrc/metrics.h says why).
 * scratch: DEVICE, 16-byte aligned, the bytes the size query returns; it holds nothing between calls.  Two launches (a tile
 * kernel, then one wave per image), no atomics: a row is bit-identical from run to run and does not depend on B or on the
 * row's position.  A wrong dtype, C, H < 11, W < 11 or two different shapes: FUSG_ERR_INVALID before any launch; B = 0
 * launches nothing. */
int fusg_image_metrics_u8(const fusg_tensor* a, const fusg_tensor* b, double* out, void* scratch, void* stream);
/* Bytes of scratch for B images of H x W x C; -1 for arguments fusg_image_metrics_u8 would refuse. */
int64_t fusg_image_metrics_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t C);
/* The same code on the CPU, sums in the kernel's order: a, b and out are HOST pointers, no GPU and no scratch needed. */
int fusg_image_metrics_host(const fusg_tensor* a, const fusg_tensor* b, double* out);
/* The counts behind EdgeConnect's EdgeAccuracy: x (labels), y (outputs) f32 [B, 1, H, W] descriptors of any strides, the
 * same shape, H and W in 1..32767; out: DEVICE int64 [B][3] = #(x > threshold), #(y > threshold), #(both), exact.  One
 * workgroup per row, no atomics.  B = 0 launches nothing; anything else wrong: FUSG_ERR_INVALID before any launch. */
int fusg_edge_counts(const fusg_tensor* x, const fusg_tensor* y, float threshold, int64_t* out, void* stream);
/* The same on HOST pointers. */
int fusg_edge_counts_host(const fusg_tensor* x, const fusg_tensor* y, float threshold, int64_t* out);
/* out[0] = the sum over i < n of ((double)a[i] - (double)b[i])^2 for two dense DEVICE float arrays (PSNR of float tensors);
 * out: DEVICE float64 [257] - out[1..256] hold the per-workgroup partials, added in a fixed order by a second launch. */
int fusg_sq_diff_sum_f32(const float* a, const float* b, int64_t n, double* out, void* stream);

/* ---- feature-space distances (EdgeConnect's PerceptualLoss / StyleLoss, forward only; new entry points, FUSG_VERSION stays
 * 118 as for the metrics above) */
/* The Gram matrix of an activation over its pixels: x is an f32 [B, C, H, W] descriptor with channel stride 1 (the NHWC-
 * physical layout, any channel pitch >= C, a channel-slice view of a wider buffer included; padding channels are never
 * read), C in 1..1024, H W in 1..2^24, B < 65536.  out: DEVICE float32 [B][C][C],
 *   out[b][i][j] = (sum over the pixels p of x[b, i, p] x[b, j, p]) / (H W C)        (StyleLoss.compute_gram)
 * exactly symmetric.  The products run on the exact-fp32 matrix instruction: inside a chunk of fusg_gram_chunk_pixels(C, H W)
 * pixels an entry is one fp32 fmaf chain in pixel order; the chunk partials (fp32, in scratch) are added in ascending order
 * in float64, scaled and rounded once by a second launch.  An entry is within (gamma_n + 2u) sum_p |x_i x_j| / (H W C) of
 * exact arithmetic, u = 2^-24, n the chunk size.  scratch: DEVICE, 16-byte aligned, the bytes the size query returns; it
 * holds nothing between calls.  Two launches, no atomics: a row's bits do not depend on B, on the row's position or on the
 * run.  A wrong dtype, a channel stride other than 1 or a size out of range: FUSG_ERR_INVALID before any launch; B = 0
 * launches nothing.  Bit-identical to the host twin. */
int fusg_gram_f32(const fusg_tensor* x, float* out, void* scratch, void* stream);
/* Bytes of scratch for a [B, C, H, W] activation; -1 for sizes fusg_gram_f32 would refuse. */
int64_t fusg_gram_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
/* Pixels per chunk: a function of C and H W only (csrc/perceptual.h states the rule); -1 for sizes out of range. */
int32_t fusg_gram_chunk_pixels(int32_t C, int64_t HW);
/* The same sums in the same order on the CPU: x and out are HOST pointers, no GPU and no scratch needed. */
int fusg_gram_f32_host(const fusg_tensor* x, float* out);
/* out[r] = the sum over row r of |(double)a - (double)b|: a, b f32 [B, C, H, W] descriptors of one shape and any strides
 * (only the C H W logical elements of a row are read), C H W < 2^31, B < 65536; out: DEVICE float64 [B].  Two launches -
 * float64 partials per workgroup into scratch (DEVICE, 16-byte aligned, the size query's bytes), then one fixed-order add
 * per row - no atomics, a row's bits independent of B.  B = 0 launches nothing; anything else wrong: FUSG_ERR_INVALID
 * before any launch.  Bit-identical to the host twin. */
int fusg_abs_diff_rows_f32(const fusg_tensor* a, const fusg_tensor* b, double* out, void* scratch, void* stream);
int64_t fusg_abs_diff_rows_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
/* The same on HOST pointers. */
int fusg_abs_diff_rows_f32_host(const fusg_tensor* a, const fusg_tensor* b, double* out);

/* ---- discriminator glue and GAN terms (EdgeConnect's Discriminator / AdversarialLoss, Warp&Learn's D_NLayersMulti / GANLoss,
 * forward only; new entry points, FUSG_VERSION stays 118 as above) */
/* nn.AvgPool2d(3, stride=2, padding=1, count_include_pad=False): src, dst NHWC-physical f32 (channel stride 1, any channel
 * pitch that is a multiple of 4, a channel-slice view included; padding channels are neither read into a result nor written),
 * any H, W >= 1, dst [B, C, (H - 1) / 2 + 1, (W - 1) / 2 + 1].  The taps inside the image are added to +0 in fp32 in raster
 * order and divided once by their number.  Bit-identical to the host twin (HOST pointers, the same layout). */
int fusg_avgpool3s2_f32(const fusg_tensor* src, const fusg_tensor* dst, void* stream);
int fusg_avgpool3s2_f32_host(const fusg_tensor* src, const fusg_tensor* dst);
/* dst[b, c, y, x] = x[b, c, y, x] * m[b, 0, y, x]: f32 descriptors of any strides, x and dst of one shape, m [B, 1, H, W]. */
int fusg_mask_mul_f32(const fusg_tensor* x, const fusg_tensor* m, const fusg_tensor* dst, void* stream);
/* Per-row sums behind the GAN objectives.  pred: f32 [B, C, H, W] through any strides (only logical elements are read),
 * C H W < 2^31, B < 65536; out: DEVICE float64 [B][fusg_gan_terms_columns() = 6], per row over its elements x (each widened
 * to float64, order (y, x, c)):
 *   0 n   1 sum x   2 sum (m x - m label)^2   3 sum relu(1 + x)   4 sum relu(1 - x)
 *   5 sum -[label max(log x, -100) + (1 - label) max(log(1 - x), -100)]     (nn.BCELoss's clamp)
 * Column 5 is NaN for a row holding an x outside [0, 1] (logits, not probabilities): the caller picks the columns that mean
 * something for its pred.  mask: NULL (or data NULL: m = 1) or f32 [B, 1, Hm, Wm], sampled as F.interpolate(mask,
 * size=(H, W)) samples in its default nearest mode - source index min((int)floorf(dst * ((float)Hm / (float)H)), Hm - 1) -
 * and used in column 2 only.  Two launches: float64 partials per (row, chunk) workgroup into scratch (DEVICE, 16-byte
 * aligned, the size query's bytes; chunk boundaries - fusg_gan_terms_chunk(n) elements each - depend on the row's element
 * count only), then one fixed-order add per row.  No atomics; a row's bits do not depend on B.  B = 0 launches nothing;
 * anything else wrong: FUSG_ERR_INVALID before any launch.  Bit-identical to the host twin: the logarithm is the library's
 * own float64 routine on both sides (csrc/gan_terms.h), a few ulp from the exact value. */
int fusg_gan_terms_rows_f32(const fusg_tensor* pred, const fusg_tensor* mask, float label, double* out, void* scratch, void* stream);
int64_t fusg_gan_terms_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int32_t fusg_gan_terms_columns(void);
int64_t fusg_gan_terms_chunk(int64_t n);
/* The same on HOST pointers. */
int fusg_gan_terms_rows_f32_host(const fusg_tensor* pred, const fusg_tensor* mask, float label, double* out);

/* ---- background frame (what the default mode's composites start from - scene['background'] - estimated from the video's own
 * frames; new entry points, FUSG_VERSION stays 118 as above) */
/* bg[y, x, c] = the LOWER median - rank (m - 1) / 2 of the m samples in ascending order, always a value that occurred - of
 * channel c of pixel (x, y) over the frames in which no box covers the pixel; count[y, x] = n, the number of those frames.
 * Frame t covers (x, y) if one of its boxes has x0 - margin <= x <= x1 + margin and y0 - margin <= y <= y1 + margin (both ends
 * inclusive; a box may reach outside the frame; one with x1 < x0 or y1 < y0 covers nothing).  A pixel with n < min_valid takes
 * all T frames instead (the fallback: the caller sees it as count < min_valid).  csrc/background.h states the arithmetic.
 * frame_ptrs: HOST table of T DEVICE pointers to dense u8 [H, W, 3] frames (separate allocations; 4-byte aligned ones are
 * read as dwords); box_offs: HOST int32 [T + 1], frame t's boxes are rows [box_offs[t], box_offs[t + 1]) of boxes, a DEVICE
 * int32 [box_offs[T]][4] table of (x0, y0, x1, y1) with any values (box_offs NULL: no boxes; boxes may then be NULL).  bg: DEVICE
 * u8 [H, W, 3], count: DEVICE u8 [H, W], both dense and written whole, nothing outside them.  Both HOST tables are read before
 * the call returns.  Checked on the host before anything is launched (FUSG_ERR_INVALID): T in 1..64, H and W in 1..32767,
 * margin in 0..32767, min_valid in 1..T, at most 64 boxes per frame, offsets from 0, no null frame.  One launch (two when 3 H W
 * is not a multiple of 4: the last bytes), no atomics, no scratch memory: a pixel's bytes depend on its own samples and boxes
 * only, not on H, W, T's bucket or the launch.  Bit-identical to the host twin. */
int fusg_background_median_u8(const void* const* frame_ptrs, int32_t T, int32_t H, int32_t W, const int32_t* boxes,
                              const int32_t* box_offs, int32_t margin, int32_t min_valid, uint8_t* bg, uint8_t* count, void* stream);
/* The same code on the CPU: every pointer (the frames, boxes, bg and count included) is a HOST pointer, no GPU needed. */
int fusg_background_median_host(const void* const* frame_ptrs, int32_t T, int32_t H, int32_t W, const int32_t* boxes,
                                const int32_t* box_offs, int32_t margin, int32_t min_valid, uint8_t* bg, uint8_t* count);

/* ---- vehicle masks from the estimated background (what scene['inpaint']['box_masks'] takes without a detector, and a third
 * compositing base: the frame with the selected vehicles replaced by background; new entry points, FUSG_VERSION stays 118) */
/* Per box b = (x0, y0, x1, y1), half-open, of n: inside the box, threshold max_c |frame - background| > thr, open by the
 * (2 open_r + 1)^2 square (outside = 0), close by the (2 close_r + 1)^2 square (dilation outside = 0, erosion outside = 1),
 * keep what is 4-connected to the part inside the core rectangle cores[b] (frame coordinates, clipped to the box), fill the
 * holes that do not open to the box border, dilate by the (2 grow + 1)^2 square cut at the box.  An empty seed gives an empty
 * mask, or with fallback != 0 the clipped core rectangle.  csrc/foreground.h states the definition step by step.
 * In frame-indexed form: frames / backgrounds = HOST tables of n_frames <= FUSG_MAX_FRAMES DEVICE pointers to dense u8 [H, W, 3]
 * images (the same pointer may repeat), frame_rows = HOST int32 [n_frames + 1], non-decreasing from 0 to n: boxes
 * [frame_rows[f], frame_rows[f + 1]) read frame f and background f.  boxes, cores: DEVICE int32 [n][4]; offsets: DEVICE int64 [n].
 * mask: DEVICE u8 [mask_len]; box b's mask is row-major [h][w] from mask[offsets[b]], 255 or 0 - the packed form
 * fusg_inpaint_inputs_boxed takes.  stats: DEVICE int32 [n][4] = n_F0, n_seed, n_mask, flags (1 fallback taken, 2 the mask
 * touches the box border, 4 the box was refused).  max_box_h / max_box_w bound the box extents of the call: up to
 * fusg_foreground_masks_scratch_bytes() == 0 the bit planes of a box live in LDS and scratch may be NULL, above it in scratch
 * (DEVICE, 4-byte aligned, that many bytes; it holds nothing between calls).  The boxes live on the device, so a box that leaves
 * the frame, exceeds the bound or whose h w bytes would leave the mask buffer is REFUSED there: flags = 4, the other stats 0, its
 * mask bytes not written, nothing of it read.  Checked on the host before any launch (FUSG_ERR_INVALID): the tables, H and W in
 * 1..32767, thr 0..254, open_r 0..3, close_r 0..7, grow 0..15, max_box 0..32767, mask_len >= 0.  n == 0: no launch, returns 0.
 * One launch, one workgroup per box, no atomics; bit-identical to the host twin. */
int fusg_foreground_masks_u8(const void* const* frames, const void* const* backgrounds, const int32_t* frame_rows, int32_t n_frames,
                             int32_t H, int32_t W, const int32_t* boxes, const int32_t* cores, const int64_t* offsets, int32_t n,
                             int32_t thr, int32_t open_r, int32_t close_r, int32_t grow, int32_t fallback, int32_t max_box_h,
                             int32_t max_box_w, uint8_t* mask, int64_t mask_len, int32_t* stats, void* scratch, void* stream);
/* Bytes of scratch for n_boxes boxes of at most max_box_h x max_box_w: 0 while the planes fit LDS; -1 for a bad argument. */
int64_t fusg_foreground_masks_scratch_bytes(int32_t n_boxes, int32_t max_box_h, int32_t max_box_w);
/* The same code on the CPU: every pointer is a HOST pointer, no GPU and no scratch needed.  A refused box is flagged as above. */
int fusg_foreground_masks_host(const void* const* frames, const void* const* backgrounds, const int32_t* frame_rows, int32_t n_frames,
                               int32_t H, int32_t W, const int32_t* boxes, const int32_t* cores, const int64_t* offsets, int32_t n,
                               int32_t thr, int32_t open_r, int32_t close_r, int32_t grow, int32_t fallback, int32_t max_box_h,
                               int32_t max_box_w, uint8_t* mask, int64_t mask_len, int32_t* stats);
/* dst = frame, then dst = background at every pixel of a box whose mask byte (mask, offsets, boxes: the packed form above) is
 * non-zero.  frame, background, dst: DEVICE dense u8 [H, W, 3]; dst is written whole and must not overlap the inputs.  Boxes
 * may overlap (every write stores the same background byte); a box that leaves the frame or whose mask would leave the buffer is
 * skipped.  Two launches, no atomics; n == 0 copies the frame. */
int fusg_erase_boxes_u8(const uint8_t* frame, const uint8_t* background, int32_t H, int32_t W, const uint8_t* mask, int64_t mask_len,
                        const int64_t* offsets, const int32_t* boxes, int32_t n, uint8_t* dst, void* stream);
int fusg_erase_boxes_host(const uint8_t* frame, const uint8_t* background, int32_t H, int32_t W, const uint8_t* mask,
                          int64_t mask_len, const int64_t* offsets, const int32_t* boxes, int32_t n, uint8_t* dst);

/* ---- vehicle boxes from the estimated background (what scene['bboxes'] takes without a tracker's detector; new entry points,
 * FUSG_VERSION stays 118) */
/* Per frame f of T: P = max_c |frame - background| > thr inside the half-open pixel rectangle roi4 = (x0, y0, x1, y1); the frame
 * is cut into cell x cell cells (partial at the right and lower edge), a cell is on when it holds >= min_count P pixels; the
 * cell grid is opened by the (2 open_r + 1)^2 square (outside = 0) and closed by the (2 close_r + 1)^2 square (dilation
 * outside = 0, erosion outside = 1); its 4-connected components, ordered by their first cell in raster order, are examined, the
 * first 256 of them; a component's area is the number of P pixels in its cells and its box the pixel-tight, half-open rectangle
 * around them; it is kept if area >= min_area, box width >= min_w and box height >= min_h.  csrc/foreground_boxes.h states the
 * definition step by step.
 * frames / backgrounds = HOST tables of T <= FUSG_MAX_FRAMES DEVICE pointers to dense u8 [H, W, 3] images, read before the call
 * returns (the same pointer may repeat).  Outputs, DEVICE int32, each written whole: boxes [T][K][4] and box_stats [T][K][2] =
 * (area, n_cells) hold the first K kept components in order and zeros from row min(n_kept, K) on; stats [T][4] = n_kept,
 * n_examined, n_P (the frame's P pixels), flags (1 OVERFLOW: n_kept > K; 2 TRUNCATED: more than 256 components, the rest
 * ignored).  scratch: DEVICE, 4-byte aligned, fusg_foreground_boxes_scratch_bytes() bytes (one 32-bit record per cell and
 * frame); every call writes all of it before reading it, it holds nothing between calls.
 * Checked on the host before any launch (FUSG_ERR_INVALID): T in 1..FUSG_MAX_FRAMES, no null pointer, H and W in 1..32767, thr
 * 0..254, cell 4, 8 or 16, min_count 1..cell^2, open_r 0..3, close_r 0..7, min_area, min_w, min_h >= 1, K 1..64, roi inside the
 * frame and not inverted, and the grid's two bit planes of ceil(H / cell) * ceil(ceil(W / cell) / 32) words within 64 KiB of
 * LDS less 512 bytes - else the message says to raise cell.  Two launches (a cell pass over the images, one workgroup per frame
 * for the rest), no atomics, no floating point; bit-identical to the host twin; recorded and replayed by a fusg_plan. */
int fusg_foreground_boxes_u8(const void* const* frames, const void* const* backgrounds, int32_t T, int32_t H, int32_t W, int32_t thr,
                             int32_t cell, int32_t min_count, int32_t open_r, int32_t close_r, int32_t min_area, int32_t min_w,
                             int32_t min_h, const int32_t* roi4, int32_t K, int32_t* boxes, int32_t* box_stats, int32_t* stats,
                             void* scratch, void* stream);
/* Bytes of scratch for T frames of H x W at this cell size: 4 T ceil(H / cell) ceil(W / cell); -1 for a bad argument. */
int64_t fusg_foreground_boxes_scratch_bytes(int32_t T, int32_t H, int32_t W, int32_t cell);
/* The same code on the CPU: every pointer is a HOST pointer, no GPU and no scratch needed. */
int fusg_foreground_boxes_host(const void* const* frames, const void* const* backgrounds, int32_t T, int32_t H, int32_t W, int32_t thr,
                               int32_t cell, int32_t min_count, int32_t open_r, int32_t close_r, int32_t min_area, int32_t min_w,
                               int32_t min_h, const int32_t* roi4, int32_t K, int32_t* boxes, int32_t* box_stats, int32_t* stats);

/* ---- linking the boxes of successive frames into trajectories (a vehicle's identity across frames without a tracker's file;
 * new entry points, FUSG_VERSION stays 118) */
/* Per video s of S, on its own: the frames first[s] .. first[s + 1] - 1 of the tables, which have the absolute frame indices
 * t0[s], t0[s] + 1, ...  Frame t holds clamp(stats[t][0], 0, K) detections boxes[t][k] = half-open (x0, y0, x1, y1):
 * fusg_foreground_boxes_u8's boxes and stats as they are.  A track is live while t - last_t <= max_gap + 1; its expected box is
 * its last box, with predict = 1 and two observations shifted by its centre's velocity (truncating division).  Within a frame the
 * eligible pairs (intersection > 0 and intersection * iou_den >= iou_num * union) are matched best first, a tie going to the
 * smaller track id and then the smaller detection index; a matched detection takes its track's id, the others found tracks with
 * the next ids in detection order.  csrc/track_boxes.h states the definition step by step.
 * boxes [frames][K][4], stats [frames][4], state [S][fusg_link_boxes_state_words()], ids [frames][K], tracks [S][max_tracks][4],
 * out_stats [S][4]: DEVICE int32; first [S + 1] and t0 [S]: HOST int32, read before the call returns.
 * ids: the track of each detection, -1 for the rows past the frame's detections, for a detection that is empty or leaves
 * [0, 16384] (flag 1 BAD_BOX) and for one whose track could not be founded (2 TRACKS_FULL: max_tracks ids are used up;
 * 4 LIVE_FULL: 128 tracks are live); written whole.  tracks: (first_t, last_t, hits, 0) per id, zeros from n_tracks on; rows
 * of tracks that died in an earlier call on the same state are left as that call wrote them.  out_stats: n_tracks, n_live,
 * n_linked (matched detections), flags - all since the state was zeroed.  state is read and written: zeros start a video, and
 * successive calls that carry it (and tracks) give the bits of one call over all their frames.  A call with t0[s] at or below
 * the last frame index the state has seen is refused on the device (flag 8 ORDER in out_stats, ids -1, nothing else touched),
 * a state whose header is out of range likewise (16 BAD_STATE).
 * Checked on the host before the launch (FUSG_ERR_INVALID): S 1..64, K 1..64, 0 < iou_num <= iou_den <= 1024, max_gap 0..255,
 * predict 0 or 1, max_tracks 1..2^20, first[0] = 0 and not falling, t0 >= 0 with t0 + frames <= 2^30, no null pointer (boxes, stats
 * and ids may be null when there is no frame at all).
 * One launch, one workgroup per video, no atomics, integer arithmetic only; bit-identical to the host twin; recorded and
 * replayed by a fusg_plan. */
int fusg_link_boxes(const int32_t* boxes, const int32_t* stats, const int32_t* first, const int32_t* t0, int32_t S, int32_t K,
                    int32_t iou_num, int32_t iou_den, int32_t max_gap, int32_t predict, int32_t max_tracks, int32_t* state,
                    int32_t* ids, int32_t* tracks, int32_t* out_stats, void* stream);
/* The same code on the CPU: every pointer is a HOST pointer, no GPU needed. */
int fusg_link_boxes_host(const int32_t* boxes, const int32_t* stats, const int32_t* first, const int32_t* t0, int32_t S, int32_t K,
                         int32_t iou_num, int32_t iou_den, int32_t max_gap, int32_t predict, int32_t max_tracks, int32_t* state,
                         int32_t* ids, int32_t* tracks, int32_t* out_stats);
/* int32 words of one video's state. */
int32_t fusg_link_boxes_state_words(void);

/* ---- recorded passes ------------------------------------------------------------------------ */
/* A fusg_plan records the launch sequence of one pass (every fusg_* launch made by the recording thread between
 * fusg_plan_begin and fusg_plan_end, with its descriptors copied and its stream remembered; the calls also execute)
 * and replays it with ONE call - the batch-1 call pattern of the reference (trajectory_inference.py:55,65) is bound by
 * the interpreter's ~12 us per launch, not by the GPU.  Not a hipGraph: replay issues the same launches on the same
 * streams (overlap between the branches of a pass is kept; a captured graph serialises them on ROCm 7.2).
 * Every device pointer used while recording must stay valid, with the same meaning, until fusg_plan_destroy. */
typedef struct fusg_plan fusg_plan;
fusg_plan* fusg_plan_create(void);
void       fusg_plan_destroy(fusg_plan* p);
int        fusg_plan_begin(fusg_plan* p);         /* start recording on the calling thread */
int        fusg_plan_end(fusg_plan* p);
/* `waiter` (hipStream_t) may not pass this point before the work issued so far on `signaller` is done. */
int        fusg_plan_add_dependency(fusg_plan* p, void* waiter, void* signaller);
/* asynchronous copy of `bytes` from pinned host memory to the device on `stream`, repeated by every run.  `src` is a
 * ring of `nslots` buffers `slot_stride` bytes apart; run r reads slot r % nslots (the recording is run 0).  Before a
 * run, fusg_plan_next_slot() returns the slot that run will read and waits until the copies that last read it have
 * executed: fill that slot, then call fusg_plan_run. */
int        fusg_plan_add_h2d(fusg_plan* p, void* dst, const void* src, int64_t bytes, int32_t nslots, int64_t slot_stride, void* stream);
int        fusg_plan_next_slot(fusg_plan* p);
int64_t    fusg_plan_size(const fusg_plan* p);    /* recorded operations */
int        fusg_plan_run(fusg_plan* p);           /* re-issue the recording; asynchronous like the launches themselves */
/* The same replay issued by ONE HOST THREAD PER RECORDED STREAM (the caller's thread takes the stream of the first operation,
 * persistent worker threads of the library the others; a wait is held back until its event's record of this run has been issued).
 * For passes that one issuing thread bounds (small batches: ~300 operations of ~6.6 us of host time each).  Same launches, streams and
 * results as fusg_plan_run; returns when every stream's operations have been issued.  fusg_plan_streams: recorded streams (-1: none). */
int32_t    fusg_plan_streams(fusg_plan* p);
int        fusg_plan_run_mt(fusg_plan* p);
/* The same recording as ONE hipGraph (measurement path; the product replays plans).  fusg_plan_graph_capture
 * re-issues the recording under a thread-local stream capture begun on `capture_stream` (the stream the pass was recorded
 * from; the recorded dependencies fork and join the side streams) and instantiates the graph; its h2d copies read pinned
 * ring slot `slot` only.  The capture is always ended, also on failure; the error text names the recorded operation that
 * failed.  fusg_plan_graph_slot waits until the previous launch has consumed that slot and returns it; fill it, then
 * fusg_plan_graph_launch(p, stream).  fusg_plan_graph_nodes: nodes of the captured graph (-1: none). */
int        fusg_plan_graph_capture(fusg_plan* p, void* capture_stream, int32_t slot);
int64_t    fusg_plan_graph_nodes(const fusg_plan* p);
int        fusg_plan_graph_slot(fusg_plan* p);
int        fusg_plan_graph_launch(fusg_plan* p, void* stream);

/* ---- misc ----------------------------------------------------------------------------------- */

int         fusg_version(void);
const char* fusg_last_error(void);
/* Kernel family of this thread's last fusg_conv2d launch (tests assert that the intended path ran):
 * 0 generic fp32, 1 generic split-fp16, 2 halo, 3 halo in parity-quadrant form (stride 2), 4 tap-unit kernel
 * (few-channel stems), 5 halo kernel in single-pass bf16, 15 / 16 halo / tap-unit kernel in single-pass fp16; -1 none yet. */
enum { FUSG_CONV_GENERIC_F32 = 0, FUSG_CONV_GENERIC_F16X3 = 1, FUSG_CONV_HALO = 2, FUSG_CONV_HALO_S2D = 3,
       FUSG_CONV_TAPUNIT = 4, FUSG_CONV_HALO_BF16 = 5, FUSG_CONV_BNECK = 6 /* fusg_hg_bottleneck */,
       FUSG_CONV_POINTWISE = 7 /* 1x1 from <= 8 channels: streaming fp32 FMA kernel, no matrix cores */,
       FUSG_CONV_SMALL = 8 /* small output images (<= 64 pixels): latency-built split-fp16 kernel (csrc/conv_kernel_small.h) */,
       FUSG_CONV_HALO_F32 = 9 /* halo kernel in exact fp32 (v_mfma_f32_16x16x4_f32, fusg_conv_desc.wfrag_f32) */,
       FUSG_CONV_TAPUNIT_F32 = 10 /* few-channel stems in exact fp32 (csrc/conv_kernel_tapunit_f32.h; wfrag_order 2 + wfrag_f32) */,
       FUSG_CONV_TAPUNIT_BF16 = 11 /* few-channel stems in single-pass bf16 (FUSG_PREC_BF16; wfrag_order 2 + wfrag_bf16) */,
       FUSG_CONV_RESPAIR = 12 /* fusg_vunet_respair */,
       FUSG_CONV_HALO_ENTRY = 13 /* fusg_conv2d_entry_nin: halo kernel with the entry NiN computed in its staging */,
       FUSG_CONV_HG_HEAD = 14 /* fusg_hg_head */,
       FUSG_CONV_HALO_F16 = 15 /* halo kernel in single-pass fp16 (FUSG_PREC_F16: one product on the `hi` fragments of wfrag) */,
       FUSG_CONV_TAPUNIT_F16 = 16 /* few-channel stems in single-pass fp16 (FUSG_PREC_F16; wfrag_order 2, `hi` fragments of wfrag) */ };
int         fusg_last_conv_kernel(void);
const char* fusg_arch(void);                      /* "gfx950" */
/* sizeof(fusg_tensor) / sizeof(fusg_conv_desc) as compiled, so that FFI bindings can verify their
 * struct mirrors. */
int         fusg_sizeof_tensor(void);
int         fusg_sizeof_conv_desc(void);
int         fusg_sizeof_bneck_desc(void);
int         fusg_sizeof_respair_desc(void);
int         fusg_sizeof_hg_head_desc(void);
/* Opt-in per-kernel timing with HIP events on the launch stream (bench.py's roofline leg).
 * kind 0 = conv implicit-GEMM kernel.  Disabled by default; enabling makes launches record two
 * events each.  fusg_prof_read synchronises the recorded events and returns totals since reset. */
void fusg_prof_enable(int on);
void fusg_prof_reset(void);
int  fusg_prof_read(int kind, double* total_ms, int64_t* launches, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* FUSG_H */
