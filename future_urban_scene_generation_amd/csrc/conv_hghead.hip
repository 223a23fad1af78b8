// The 1x1 head that ends a stack of the hourglass, per launch (fusg_hg_head, include/fusg.h): split-fp16 arithmetic of
// conv_kernel_h3.h,
//   y     = relu(fc(y_in) + b_fc)                 256 -> 256 (the fc BatchNorm folded by the caller)
//   score = score(y) + b_s                        256 -> 32 (num_classes real columns, the others zero weights and bias)
//   x'    = x + join(cat[y, score]) + b_j         288 -> 256                     (join form; the last stack stops after score)
// written: score, x'.  (stacked_hourglass/models.py: fc, score, fc_ + score_ as the two-source `join`.)
//
// Why: as three halo launches y is written once and read twice and score is read back right after it is written - 0.97 GB
// through HBM/L2 per stack at batch 32 on 64 x 64 where the chain needs 0.42 - and a 1x1 gets nothing from the halo kernel's
// stage-a-chunk / barrier / one-tap-of-MFMAs / barrier rhythm: 112 TFLOP/s and 1.75 TB/s, near neither limit.  The chain is per
// pixel (no halo, no ring to recompute), so a workgroup owns 64 consecutive pixels of one image on conv_bneck.hip's scheme:
//   0. all 256 channels of y_in, split to (hi, lo') -> LDS image Y, [8 chunks][64 pixels][32 halves] per half (64 KiB).
//   1. fc: the four waves split the 256 output channels (no weight fragment is fetched twice per workgroup), all read every
//      pixel fragment.  Result + bias, ReLU, split from the accumulators, overlays Y.
//   2. score: wave w takes pixels 16 w .. of both 16-column tiles; result + bias leaves as 16-byte stores and, split, becomes the
//      ninth chunk of Y (+ 8 KiB -> 72 KiB: two workgroups per CU).
//   3. join over the nine chunks, waves split the channels again; + bias, + x, 16-byte stores.
// The MFMA runs transposed as in conv_bneck.hip (weights = A operand, the `wfrag` copy; pixels = B), so a lane ends up with 4
// consecutive channels of one pixel: 8-byte LDS stores per fp16 half, 16-byte global stores, no transposition step.  Weight
// fragments are fetched one chunk ahead (fc, join) or four (score: a chunk is 6 MFMAs per wave).
//
// Bits: every accumulator sees the products of the unfused launches in their order - chunks 0 .. 7 of y (then the score chunk),
// per chunk ah wh, ah wl, al' (wh 2^-11); a 1x1 halo launch never gets the K split over the waves (route_conv: two taps at
// least), so this is the order at every batch size - and the shared epilogue arithmetic: act(fmaf(acc, wscale, bias)) + residual.
// y and score are split by the halo kernel's no-pre-op staging (split4 under the floor relu_floor gives it, -inf) and feed the
// same running |a| maximum.  score and x' are bit for bit what the three launches write (tests/test_gpu_hg_head.py).
#include "conv_kernel_h3.h"

namespace fusg {

struct HgHeadK {
    const float* yin; const float* x; float* score; float* dst;
    long ysn, ysh, ysw, xsn, xsh, xsw, ssn, ssh, ssw, dsn, dsh, dsw;
    const _Float16* wf; const _Float16* ws; const _Float16* wj;
    const float* bf; const float* bs; const float* bj;
    const float* sf; const float* ss; const float* sj;
    const float* zeros;
    int* status;
    float vfloor;                          // the floor of the no-pre-op staging (-inf), a run-time value as in the halo kernel
    int HW, W, tiles_per_img;
    int score_c;                           // channels of the score tensor (32 in the join form)
};

constexpr int HH_C = 256, HH_NCH = HH_C / 32, HH_PIX = 64;
constexpr int HH_CHUNK = HH_PIX * 32;                                    // halves per chunk of one image half
constexpr size_t hghead_lds() { return (size_t)2 * (HH_NCH + 1) * HH_CHUNK * sizeof(_Float16); }   // 72 KiB

template <int CT> struct HhFrag { h8 f[CT][2]; };      // [16-column tile][hi | lo]

__device__ __forceinline__ f32x4 hh_mfma(const h8 a, const h8 b, const f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// the launches' epilogue value of 4 channels (epilogue_rows / epi_store): act(fmaf(acc, wscale, bias))
__device__ __forceinline__ f32x4 hh_epi(const f32x4 a, const f32x4 wsc, const f32x4 bias, int act) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = act_apply(fmaf(a[e], wsc[e], bias[e]), act);
    return v;
}

template <bool JOIN>
__global__ __launch_bounds__(256, 2) void hg_head_h3(const HgHeadK k) {
    extern __shared__ __attribute__((aligned(16))) _Float16 smem_h[];
    _Float16* Yh = smem_h;                              // [9 chunks][64 pixels][32]: y_in, then y; chunk 8 = score
    _Float16* Yl = Yh + (HH_NCH + 1) * HH_CHUNK;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lp = lane & 15, lg = lane >> 4;           // pixel of the fragment, 8-k slot
    const int tile = xcd_tile();
    const int b = tile / k.tiles_per_img, q0 = (tile - b * k.tiles_per_img) * HH_PIX;
    float amax = 0.f;

    // weight fragments of 16-column tiles gct0 .. gct0 + CT - 1 of chunk `slab` in a panel of nt32 32-column tiles per chunk
    // ([chunk][nt32][16-column half][hi | lo][64 lanes][8 halves], pack.frag_f16x3)
    auto load_w = [&](auto& F, const _Float16* w, int slab, int nt32, int gct0) __attribute__((always_inline)) {
        constexpr int CT = sizeof(F.f) / sizeof(F.f[0]);
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const int gct = gct0 + j;
            const _Float16* p = w + ((long)((slab * nt32 + (gct >> 1)) * 2 + (gct & 1)) * 2) * 512 + lane * 8;
            F.f[j][0] = *(const h8*)(p);
            F.f[j][1] = *(const h8*)(p + 512);
        }
    };
    // element offset of pixel q of the image in a tensor with row / pixel strides (sh, sw); q < HW
    auto pix_off = [&](int q, long sh, long sw) __attribute__((always_inline)) {
        const int y = q / k.W;
        return (long)y * sh + (long)(q - y * k.W) * sw;
    };

    // ------------------------------------------------------------------ 0. y_in -> Y
    HhFrag<4> v0, v1;
    {
        const int kc = t & 7;
        const float* yp[2];
        int soff[2];
        bool ok[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = (t >> 3) + 32 * j;
            ok[j] = q0 + p < k.HW;
            yp[j] = ok[j] ? k.yin + (long)b * k.ysn + pix_off(q0 + p, k.ysh, k.ysw) + kc * 4 : k.zeros;
            soff[j] = p * 32 + ((((kc >> 1) ^ (((p >> 2) & 1) << 1)) << 3) | ((kc & 1) << 2));
        }
        f32x4 r[HH_NCH][2];
#pragma unroll
        for (int c = 0; c < HH_NCH; ++c)
#pragma unroll
            for (int j = 0; j < 2; ++j) r[c][j] = *(const f32x4*)(ok[j] ? yp[j] + c * 32 : k.zeros);
        load_w(v0, k.wf, 0, HH_NCH, wave * 4);
#pragma unroll
        for (int c = 0; c < HH_NCH; ++c)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                h4 hi, lo;
                split4(r[c][j], k.vfloor, hi, lo, amax);
                *(h4*)(Yh + c * HH_CHUNK + soff[j]) = hi;
                *(h4*)(Yl + c * HH_CHUNK + soff[j]) = lo;
            }
    }
    __syncthreads();

    const int sfrag = lp * 32 + ((lg ^ (((lp >> 2) & 1) << 1)) << 3);      // + rg * 512: this lane's fragment of a chunk
    // one chunk of a 256-column convolution: this wave's 4 tiles x the 4 row groups of 16 pixels
    auto compute = [&](f32x4 (&acc)[4][4], const HhFrag<4>& F, int c) __attribute__((always_inline)) {
        h8 xh[4], xl[4], bs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { xh[i] = *(const h8*)(Yh + c * HH_CHUNK + i * 512 + sfrag); xl[i] = *(const h8*)(Yl + c * HH_CHUNK + i * 512 + sfrag); }
#pragma unroll
        for (int j = 0; j < 4; ++j) bs[j] = scale_m11(F.f[j][0]);
#pragma unroll
        for (int term = 0; term < 3; ++term)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = hh_mfma(term == 0 ? F.f[j][0] : term == 1 ? F.f[j][1] : bs[j], term == 2 ? xl[i] : xh[i], acc[i][j]);
    };
    // this lane's 4 channels of 16-channel tile gct at pixel p: chunk gct >> 1, slot 2 (gct & 1) + (lg >> 1), halves (lg & 1) * 4
    auto y_off = [&](int gct, int p) __attribute__((always_inline)) {
        const int g = (gct & 1) * 2 + (lg >> 1);
        return ((gct >> 1) * HH_PIX + p) * 32 + ((g ^ (((p >> 2) & 1) << 1)) << 3) + ((lg & 1) << 2);
    };

    // ------------------------------------------------------------------ 1. fc: this wave's 64 channels
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < HH_NCH; c += 2) {
        load_w(v1, k.wf, c + 1, HH_NCH, wave * 4);
        compute(acc, v0, c);
        if (c + 2 < HH_NCH) load_w(v0, k.wf, c + 2, HH_NCH, wave * 4);
        compute(acc, v1, c + 1);
    }
    __syncthreads();                                            // y_in is dead: y may overwrite it

    // score's first weights on their way while fc's result is written to Y
    HhFrag<2> s[HH_NCH];
#pragma unroll
    for (int c = 0; c < 4; ++c) load_w(s[c], k.ws, c, 1, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gct = wave * 4 + j;
        const int n0 = gct * 16 + lg * 4;
        const f32x4 bias = *(const f32x4*)(k.bf + n0), wsc = *(const f32x4*)(k.sf + n0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            h4 hi, lo;
            split4(hh_epi(acc[i][j], wsc, bias, FUSG_ACT_RELU), k.vfloor, hi, lo, amax);
            const int o = y_off(gct, i * 16 + lp);
            *(h4*)(Yh + o) = hi;
            *(h4*)(Yl + o) = lo;
        }
    }
    __syncthreads();

    // ------------------------------------------------------------------ 2. score: this wave's 16 pixels, both tiles
#pragma unroll
    for (int c = 4; c < HH_NCH; ++c) load_w(s[c], k.ws, c, 1, 0);
    f32x4 accs[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int c = 0; c < HH_NCH; ++c) {
        const h8 xh = *(const h8*)(Yh + c * HH_CHUNK + wave * 512 + sfrag), xl = *(const h8*)(Yl + c * HH_CHUNK + wave * 512 + sfrag);
        h8 bs[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) bs[j] = scale_m11(s[c].f[j][0]);
#pragma unroll
        for (int term = 0; term < 3; ++term)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                accs[j] = hh_mfma(term == 0 ? s[c].f[j][0] : term == 1 ? s[c].f[j][1] : bs[j], term == 2 ? xl : xh, accs[j]);
    }
    if constexpr (JOIN) load_w(v0, k.wj, 0, HH_NCH, wave * 4);
    {
        const int p = wave * 16 + lp;
        const bool ok = q0 + p < k.HW;
        float* sp = k.score + (long)b * k.ssn + (ok ? pix_off(q0 + p, k.ssh, k.ssw) : 0);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n0 = j * 16 + lg * 4;
            const f32x4 v = hh_epi(accs[j], *(const f32x4*)(k.ss + n0), *(const f32x4*)(k.bs + n0), FUSG_ACT_NONE);
            if (ok) {
                if (n0 + 4 <= k.score_c) *(f32x4*)(sp + n0) = v;
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (n0 + e < k.score_c) sp[n0 + e] = v[e];
                }
            }
            if constexpr (JOIN) {                               // the join's second source: the tensor just written
                h4 hi, lo;
                split4(v, k.vfloor, hi, lo, amax);
                const int o = y_off(2 * HH_NCH + j, p);
                *(h4*)(Yh + o) = hi;
                *(h4*)(Yl + o) = lo;
            }
        }
    }
    if (amax >= F16X3_LIMIT && k.status) *k.status = 1;
    if constexpr (!JOIN) return;
    __syncthreads();

    // ------------------------------------------------------------------ 3. join over y's 8 chunks and score's, + x
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    long xoff[4], doff[4];
    bool okp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = q0 + i * 16 + lp;
        okp[i] = q < k.HW;
        xoff[i] = (long)b * k.xsn + (okp[i] ? pix_off(q, k.xsh, k.xsw) : 0);
        doff[i] = (long)b * k.dsn + (okp[i] ? pix_off(q, k.dsh, k.dsw) : 0);
    }
    f32x4 res[4][4];
#pragma unroll
    for (int c = 0; c < HH_NCH; c += 2) {
        load_w(v1, k.wj, c + 1, HH_NCH, wave * 4);
        compute(acc, v0, c);
        load_w(v0, k.wj, c + 2, HH_NCH, wave * 4);
        compute(acc, v1, c + 1);
    }
    // the residual behind the last chunk's MFMAs (the second fragment set is dead: its registers are there)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) res[i][j] = *(const f32x4*)(okp[i] ? k.x + xoff[i] + (wave * 4 + j) * 16 + lg * 4 : k.zeros);
    compute(acc, v0, HH_NCH);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n0 = (wave * 4 + j) * 16 + lg * 4;
        const f32x4 bias = *(const f32x4*)(k.bj + n0), wsc = *(const f32x4*)(k.sj + n0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (okp[i]) *(f32x4*)(k.dst + doff[i] + n0) = hh_epi(acc[i][j], wsc, bias, FUSG_ACT_NONE) + res[i][j];
    }
}

}  // namespace fusg

using namespace fusg;

static bool hh_aligned16(const void* p) { return p != nullptr && (((uintptr_t)p) & 15) == 0; }

static int hg_head_impl(const fusg_hg_head_desc* d, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    FUSG_CHECK(d != nullptr, "hg_head: null descriptor");
    const fusg_tensor& y = d->y_in;
    FUSG_CHECK(d->join == 0 || d->join == 1, "hg_head: join %d", d->join);
    FUSG_CHECK(is_nhwc(y) && y.c == HH_C && y.n >= 1 && y.h >= 1 && y.w >= 1, "hg_head: y_in must be NHWC-physical f32 with 256 channels");
    FUSG_CHECK(is_nhwc(d->score) && same_nhw(y, d->score) && d->score.c >= 1 && d->score.c <= 32,
               "hg_head: score must be NHWC-physical f32 [n, <= 32, h, w] like y_in");
    FUSG_CHECK(d->score.data != y.data, "hg_head: score aliases y_in");
    const void* ptrs[] = {d->wfrag_fc, d->bias_fc, d->wscale_fc, d->wfrag_score, d->bias_score, d->wscale_score};
    for (const void* p : ptrs) FUSG_CHECK(hh_aligned16(p), "hg_head: a parameter array is missing or not 16-byte aligned");
    if (d->join) {
        FUSG_CHECK(d->score.c == 32, "hg_head: the join form reads score as a 32-channel source (%ld channels)", (long)d->score.c);
        FUSG_CHECK(is_nhwc(d->x) && is_nhwc(d->dst) && same_nhw(y, d->x) && same_nhw(y, d->dst) && d->x.c == HH_C && d->dst.c == HH_C,
                   "hg_head: x / dst must be NHWC-physical f32 [n, 256, h, w] like y_in");
        FUSG_CHECK(d->dst.data != y.data && d->dst.data != d->score.data, "hg_head: dst aliases y_in or score");
        const void* pj[] = {d->wfrag_join, d->bias_join, d->wscale_join};
        for (const void* p : pj) FUSG_CHECK(hh_aligned16(p), "hg_head: a join parameter array is missing or not 16-byte aligned");
    }
    FUSG_CHECK(d->status != nullptr, "hg_head: status word missing");
    FUSG_CHECK(y.n * y.h * y.w * y.sw < (1L << 40) && y.h * y.w < (1L << 30), "hg_head: extent");
    HgHeadK k;
    memset(&k, 0, sizeof(k));
    k.yin = (const float*)y.data; k.ysn = y.sn; k.ysh = y.sh; k.ysw = y.sw;
    k.score = (float*)d->score.data; k.ssn = d->score.sn; k.ssh = d->score.sh; k.ssw = d->score.sw;
    k.x = (const float*)d->x.data; k.xsn = d->x.sn; k.xsh = d->x.sh; k.xsw = d->x.sw;
    k.dst = (float*)d->dst.data; k.dsn = d->dst.sn; k.dsh = d->dst.sh; k.dsw = d->dst.sw;
    k.wf = (const _Float16*)d->wfrag_fc; k.ws = (const _Float16*)d->wfrag_score; k.wj = (const _Float16*)d->wfrag_join;
    k.bf = d->bias_fc; k.bs = d->bias_score; k.bj = d->bias_join;
    k.sf = d->wscale_fc; k.ss = d->wscale_score; k.sj = d->wscale_join;
    k.status = d->status;
    k.vfloor = -__builtin_inff();
    k.zeros = zero_line();
    if (!k.zeros) { set_error("hg_head: cannot allocate the zero line"); return FUSG_ERR_LAUNCH; }
    k.HW = (int)(y.h * y.w); k.W = (int)y.w;
    k.tiles_per_img = (k.HW + HH_PIX - 1) / HH_PIX;
    k.score_c = (int)d->score.c;
    const long wgs = (long)y.n * k.tiles_per_img;
    FUSG_CHECK(wgs < (1L << 31), "hg_head: grid");
    const void* fn = d->join ? (const void*)hg_head_h3<true> : (const void*)hg_head_h3<false>;
    const size_t lds = hghead_lds();
    const double M = (double)y.n * y.h * y.w;
    // the convolutions' own FLOPs, K as the unfused launches count it (k_pad: 256, 256, 288)
    prof_begin(0, s, 2.0 * M * ((double)HH_C * HH_C + (double)d->score.c * HH_C + (d->join ? (double)HH_C * (HH_C + 32) : 0.0)));
    const hipError_t e = launch_kernel(fn, dim3((unsigned)wgs), lds, (int)lds, k, s);
    prof_end(0, s);
    if (e != hipSuccess) { set_error("hg_head launch: %s", hipGetErrorString(e)); return FUSG_ERR_LAUNCH; }
    note_conv_kernel(FUSG_CONV_HG_HEAD);
    return FUSG_OK;
}
extern "C" int fusg_hg_head(const fusg_hg_head_desc* d, void* stream) { return fusg::plan_dispatch(hg_head_impl, stream, d); }
extern "C" int fusg_sizeof_hg_head_desc(void) { return (int)sizeof(fusg_hg_head_desc); }
