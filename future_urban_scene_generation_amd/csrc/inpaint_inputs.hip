// EdgeConnect's inputs on the device: fusg_inpaint_inputs (include/fusg.h) runs the steps of inpaint_inputs.h - the same
// per-pixel code as the host twin below - as five launches over all V vehicles (grid.y = V), no atomics:
//   dilate      32 x 8 box pixels per workgroup; the mask tile with its 4 / 3 pixel halo is staged in LDS (53 LDS reads per
//               pixel instead of 53 global ones) and the dilated box is written to scratch once.  The tile is filled
//               through `MaskSrc::px` from either mask source: frame-sized u8 planes (fusg_inpaint_inputs) or one packed
//               buffer of box-sized u8 / f32 masks (fusg_inpaint_inputs_boxed: row pitch = the box width, so rows start
//               unaligned; a tile row is 39 consecutive elements read by 39 consecutive lanes, coalesced either way)
//   box pass    one thread per output pixel: resize of the whitened box (whitened on load) and of the dilated mask, gray,
//               binarise -> img, gray, mask and the int16 gray / valid plane Canny reads
//   smooth      one workgroup per image row: the axis-0 Gaussian of m and f per column (17 coalesced int16 reads), the
//               row through LDS, the axis-1 Gaussian and the division -> s (float64, scratch)
//   nms         64 x 4 pixels per workgroup, one wavefront per 64-pixel row segment: s with a 2-pixel halo in LDS, the
//               magnitude recomputed on a 1-pixel halo, erosion, suppression, thresholds; the low / high bits of a
//               segment leave as two 64-bit ballots (2 bits per pixel)
//   hysteresis  one workgroup per image, the low map and the (double-buffered) kept map as bitmaps in LDS (24 KiB), one
//               thread per word; rounds until no word changed, the flag passed through wave ballots.  No iteration cap:
//               the kept set grows monotonically inside low, so the loop ends at the unique reachability set.
// All kernels are memory- / latency-bound glue in front of the EdgeConnect pass; float64 only in smooth and nms.
#include "common.h"
#include "inpaint_inputs.h"

namespace fusg {

struct F32Out { float* p; long sn, sc, sh, sw; };
struct InpaintK {
    const unsigned char* frame; long fsh, fsw; int H, W;
    const unsigned char* det; long dsn, dsh, dsw;               // the masks as frame-sized planes, or (det == nullptr) ...
    const void* bm; const int64_t* bm_off; long bm_n; int bm_f32;  // ... packed per box: [bh][bw] from element bm_off[v] of bm_n
    const int32_t* boxes;
    F32Out img, gray, edge, mask;
    unsigned char* dil; int16_t* gv; double* s; uint64_t* bits;
    long dil_v; int V, max_h, max_w;
    ii::Ellipse el;
};

static inline F32Out f32out(const fusg_tensor& t) { return F32Out{(float*)t.data, t.sn, t.sc, t.sh, t.sw}; }

// Does vehicle v's packed mask of bh x bw elements lie inside the buffer?  (bh * bw < 2^30: the frame's sides are < 32768)
FUSG_HD bool packed_ok(long off, int bh, int bw, long n) { return off >= 0 && off <= n - (long)bh * bw; }
// Vehicle v's box: ii::box_of, and with packed masks a box whose mask would leave the buffer has no pixels either - every
// step (not only the one that reads the mask) sees the same zero-extent box, so all four outputs are zeros.
FUSG_HD ii::Box vehicle_box(const InpaintK& k, int v) {
    ii::Box b = ii::box_of(k.boxes + v * 4, k.H, k.W, k.max_h, k.max_w);
    if (!k.det && !packed_ok(k.bm_off[v], b.bh, b.bw, k.bm_n)) b = ii::Box{0, 0, 0, 0};
    return b;
}
// The detector mask of one vehicle, addressed in box coordinates; px(yy, xx): the u8 pixel the dilation reads (a float
// mask binarised as the reference does, m * 255 > 0 ? 255 : 0 - a NaN gives 0)
struct MaskSrc {
    const unsigned char* u8; const float* f32; long sh, sw;
    FUSG_HD int px(int yy, int xx) const {
        const long i = (long)yy * sh + (long)xx * sw;
        return f32 ? (f32[i] * 255.f > 0.f ? 255 : 0) : (int)u8[i];
    }
};
FUSG_HD MaskSrc mask_src(const InpaintK& k, int v, const ii::Box& b) {
    if (k.det) return MaskSrc{k.det + (long)v * k.dsn + (long)b.y0 * k.dsh + (long)b.x0 * k.dsw, nullptr, k.dsh, k.dsw};
    const long off = b.bw > 0 && b.bh > 0 ? k.bm_off[v] : 0;
    return k.bm_f32 ? MaskSrc{nullptr, (const float*)k.bm + off, b.bw, 1} : MaskSrc{(const unsigned char*)k.bm + off, nullptr, b.bw, 1};
}

// ------------------------------------------------------------------------------------------------ device kernels
constexpr int DT_W = 32, DT_H = 8, DT_LW = DT_W + ii::KS - 1, DT_LH = DT_H + ii::KS - 1;

__global__ __launch_bounds__(256) void inpaint_dilate_kernel(const InpaintK k, int tiles_x) {
    __shared__ unsigned char tile[DT_LH * DT_LW];
    const int v = blockIdx.y;
    const ii::Box b = vehicle_box(k, v);
    const int tx0 = (blockIdx.x % tiles_x) * DT_W, ty0 = (blockIdx.x / tiles_x) * DT_H;
    if (tx0 >= b.bw || ty0 >= b.bh) return;                       // workgroup-uniform
    const MaskSrc src = mask_src(k, v, b);
    for (int t = threadIdx.x; t < DT_LH * DT_LW; t += 256) {
        const int yy = ty0 - ii::ANCHOR + t / DT_LW, xx = tx0 - ii::ANCHOR + t % DT_LW;
        tile[t] = ((unsigned)yy < (unsigned)b.bh && (unsigned)xx < (unsigned)b.bw) ? (unsigned char)src.px(yy, xx) : 0;
    }
    __syncthreads();
    const int x = tx0 + (threadIdx.x % DT_W), y = ty0 + (threadIdx.x / DT_W);
    if (x >= b.bw || y >= b.bh) return;
    const int m = ii::dilate_px([&](int yy, int xx) { return (int)tile[(yy - ty0 + ii::ANCHOR) * DT_LW + (xx - tx0 + ii::ANCHOR)]; },
                                y, x, b.bh, b.bw, k.el);
    k.dil[(long)v * k.dil_v + (long)y * k.max_w + x] = (unsigned char)m;
}

// the box pass of one output pixel, for host and device
FUSG_HD void box_pass_px(const InpaintK& k, int v, int y, int x) {
    const ii::Box b = vehicle_box(k, v);
    const unsigned char* fr = k.frame + (long)b.y0 * k.fsh + (long)b.x0 * k.fsw;
    const unsigned char* dl = k.dil + (long)v * k.dil_v;
    const ii::BoxPx p = ii::box_px([&](int yy, int xx, int c) { return (int)fr[(long)yy * k.fsh + (long)xx * k.fsw + c]; },
                                   [&](int yy, int xx) { return (int)dl[(long)yy * k.max_w + xx]; }, y, x, b.bh, b.bw);
    for (int c = 0; c < 3; ++c) k.img.p[(long)v * k.img.sn + c * k.img.sc + (long)y * k.img.sh + (long)x * k.img.sw] = (float)p.c[c] / 255.f;
    k.gray.p[(long)v * k.gray.sn + (long)y * k.gray.sh + (long)x * k.gray.sw] = (float)p.gray / 255.f;
    k.mask.p[(long)v * k.mask.sn + (long)y * k.mask.sh + (long)x * k.mask.sw] = p.hole ? 1.f : 0.f;
    k.gv[((long)v * ii::R + y) * ii::R + x] = ii::gray_valid(p);
}

__global__ __launch_bounds__(256) void inpaint_box_kernel(const InpaintK k) {
    box_pass_px(k, blockIdx.y, blockIdx.x, threadIdx.x);
}

// the axis-0 Gaussian of m (which = 0) or f (1) at (y, x), from the gray / valid plane of one image
FUSG_HD double smooth_axis0(const int16_t* gv, int y, int x, int which, const ii::Gauss& g) {
    return ii::gauss_px([&](int l) {
        if ((unsigned)l >= (unsigned)ii::R) return 0.0;
        const int q = gv[l * ii::R + x];
        return q < 0 ? 0.0 : (which ? 1.0 : (double)q);
    }, y, g);
}
// the axis-1 Gaussian of both rows and their quotient
FUSG_HD double smooth_axis1(const double* row_m, const double* row_f, int x, const ii::Gauss& g) {
    const double gm = ii::gauss_px([&](int l) { return (unsigned)l < (unsigned)ii::R ? row_m[l] : 0.0; }, x, g);
    const double gf = ii::gauss_px([&](int l) { return (unsigned)l < (unsigned)ii::R ? row_f[l] : 0.0; }, x, g);
    return gm / (gf + ii::EPS);
}

__global__ __launch_bounds__(256) void inpaint_smooth_kernel(const InpaintK k, const ii::Gauss g) {
    __shared__ double row_m[ii::R], row_f[ii::R];
    const int v = blockIdx.y, y = blockIdx.x, x = threadIdx.x;
    const int16_t* gv = k.gv + (long)v * ii::R * ii::R;
    row_m[x] = smooth_axis0(gv, y, x, 0, g);
    row_f[x] = smooth_axis0(gv, y, x, 1, g);
    __syncthreads();
    k.s[((long)v * ii::R + y) * ii::R + x] = smooth_axis1(row_m, row_f, x, g);
}

// steps d-g at (i, j): s / valid fetch the smoothed image (edge repeated) and the validity (false outside), mag(ii, jj)
// the magnitude of an in-image pixel
template <class FS, class FV, class FM>
FUSG_HD int nms_code(FS s, FV valid, FM mag, int i, int j) {
    bool er = true;
    for (int di = -1; di <= 1; ++di)
        for (int dj = -1; dj <= 1; ++dj) er = er && valid(i + di, j + dj);
    if (!er) return 0;
    double gi, gj;
    ii::sobel_px(s, i, j, gi, gj);
    const double m = ii::magnitude(gi, gj);
    if (!(m > 0.0)) return 0;
    const bool lm = ii::nms_px(gi, gj, m, [&](int di, int dj) { return mag(i + di, j + dj); });
    return ii::threshold_code(lm, m);
}

constexpr int NT_W = 64, NT_H = 4, NS_W = NT_W + 4, NS_H = NT_H + 4, NM_W = NT_W + 2, NM_H = NT_H + 2;

__global__ __launch_bounds__(256) void inpaint_nms_kernel(const InpaintK k) {
    __shared__ double st[NS_H * NS_W], mt[NM_H * NM_W];
    __shared__ unsigned char vt[NM_H * NM_W];
    const int v = blockIdx.y, tx0 = (blockIdx.x % ii::WPR) * NT_W, ty0 = (blockIdx.x / ii::WPR) * NT_H;
    const double* S = k.s + (long)v * ii::R * ii::R;
    const int16_t* gv = k.gv + (long)v * ii::R * ii::R;
    const auto clampi = [](int a) { return a < 0 ? 0 : (a > ii::R - 1 ? ii::R - 1 : a); };
    for (int t = threadIdx.x; t < NS_H * NS_W; t += 256)
        st[t] = S[clampi(ty0 - 2 + t / NS_W) * ii::R + clampi(tx0 - 2 + t % NS_W)];
    for (int t = threadIdx.x; t < NM_H * NM_W; t += 256) {
        const int i = ty0 - 1 + t / NM_W, j = tx0 - 1 + t % NM_W;
        vt[t] = ((unsigned)i < (unsigned)ii::R && (unsigned)j < (unsigned)ii::R) ? gv[i * ii::R + j] >= 0 : 0;
    }
    __syncthreads();
    const auto s = [&](int i, int j) { return st[(i - ty0 + 2) * NS_W + (j - tx0 + 2)]; };
    for (int t = threadIdx.x; t < NM_H * NM_W; t += 256) {
        const int i = ty0 - 1 + t / NM_W, j = tx0 - 1 + t % NM_W;
        double m = 0.0;
        if ((unsigned)i < (unsigned)ii::R && (unsigned)j < (unsigned)ii::R) {
            double gi, gj;
            ii::sobel_px(s, i, j, gi, gj);
            m = ii::magnitude(gi, gj);
        }
        mt[t] = m;
    }
    __syncthreads();
    const int i = ty0 + (threadIdx.x >> 6), j = tx0 + (threadIdx.x & 63);
    const int code = nms_code(s, [&](int a, int b) { return vt[(a - ty0 + 1) * NM_W + (b - tx0 + 1)] != 0; },
                              [&](int a, int b) { return mt[(a - ty0 + 1) * NM_W + (b - tx0 + 1)]; }, i, j);
    // every lane of the wavefront is here: lane l holds pixel (i, tx0 + l)
    const uint64_t low = __ballot(code >= 1), high = __ballot(code == 2);
    if ((threadIdx.x & 63) == 0) {
        uint64_t* bits = k.bits + (long)v * 2 * ii::R * ii::WPR;
        bits[i * ii::WPR + (tx0 >> 6)] = low;
        bits[ii::R * ii::WPR + i * ii::WPR + (tx0 >> 6)] = high;
    }
}

constexpr int HY_WORDS = ii::R * ii::WPR;                         // 1024: one thread per word

__global__ __launch_bounds__(HY_WORDS) void inpaint_hysteresis_kernel(const InpaintK k) {
    __shared__ uint64_t kept[2][HY_WORDS];
    __shared__ int flag[2][HY_WORDS / 64];
    const int v = blockIdx.x, t = threadIdx.x, y = t / ii::WPR, w = t % ii::WPR;
    const uint64_t* bits = k.bits + (long)v * 2 * HY_WORDS;
    const uint64_t low = bits[t];
    kept[0][t] = bits[HY_WORDS + t];
    __syncthreads();
    int cur = 0;
    for (;;) {
        const uint64_t* kc = kept[cur];
        const uint64_t old = kc[t];
        const uint64_t now = ii::hysteresis_word([&](int yy, int ww) {
            return ((unsigned)yy < (unsigned)ii::R && (unsigned)ww < (unsigned)ii::WPR) ? kc[yy * ii::WPR + ww] : (uint64_t)0;
        }, low, y, w);
        kept[cur ^ 1][t] = now;
        const bool any = __ballot(now != old) != 0;
        if ((t & 63) == 0) flag[cur][t >> 6] = any;
        __syncthreads();
        int go = 0;
        for (int q = 0; q < HY_WORDS / 64; ++q) go |= flag[cur][q];
        cur ^= 1;
        if (!go) break;                                           // workgroup-uniform: every thread read the same flags
    }
    // (flag[cur ^ 1] is rewritten two rounds later, behind the next barrier; kept[cur] holds the fixed point)
    const F32Out& e = k.edge;
    for (int p = t; p < ii::R * ii::R; p += HY_WORDS) {
        const int py = p / ii::R, px = p % ii::R;
        e.p[(long)v * e.sn + (long)py * e.sh + (long)px * e.sw] = (float)((kept[cur][py * ii::WPR + (px >> 6)] >> (px & 63)) & 1);
    }
}

}  // namespace fusg

using namespace fusg;

// ------------------------------------------------------------------------------------------------ host side
static bool f32_nchw(const fusg_tensor* t, long V, int c) {
    return t && t->data && t->dtype == FUSG_F32 && t->n == V && t->c == c && t->h == ii::R && t->w == ii::R;
}

// the packed form's mask arguments (fusg_inpaint_inputs_boxed); V comes from img
struct PackedMasks { const void* data; int32_t dtype; int64_t n; const int64_t* off; };

static int inpaint_check(const fusg_tensor* frame, const fusg_tensor* det, const PackedMasks* pm, const int32_t* boxes, const double* gauss_w, int32_t radius,
                         int32_t max_h, int32_t max_w, const fusg_tensor* img, const fusg_tensor* gray, const fusg_tensor* edge,
                         const fusg_tensor* mask, void* scratch, const char* what, InpaintK& k, ii::Gauss& g) {
    FUSG_CHECK(frame && frame->data && frame->dtype == FUSG_U8 && frame->n == 1 && frame->c == 3 && frame->sc == 1 && frame->sw >= 3 &&
               frame->h >= 1 && frame->w >= 1 && frame->h < 32768 && frame->w < 32768 && frame->sh >= frame->w * frame->sw,
               "%s: frame must be one u8 HWC image of 3 channels", what);
    long V;
    if (!pm) {
        FUSG_CHECK(det && det->dtype == FUSG_U8 && det->c == 1 && det->n >= 0 && det->n < (1 << 16) && (det->n == 0 || det->data) &&
                   det->h == frame->h && det->w == frame->w && det->sw >= 1 && det->sh >= det->w * det->sw && (det->n <= 1 || det->sn >= det->h * det->sh),
                   "%s: det_masks must be u8 [V, 1, H, W] of the frame's H x W", what);
        V = det->n;
    } else {
        FUSG_CHECK((pm->dtype == FUSG_U8 || pm->dtype == FUSG_F32) && pm->n >= 0 && (pm->n == 0 || pm->data) &&
                   (pm->dtype != FUSG_F32 || (((uintptr_t)pm->data) & 3) == 0),
                   "%s: box_masks must be one packed u8 or f32 buffer of n_elems >= 0 elements", what);
        FUSG_CHECK(img && img->n >= 0 && img->n < (1 << 16), "%s: img must be f32 [V, 3, %d, %d]", what, ii::R, ii::R);
        V = img->n;
        FUSG_CHECK(V == 0 || pm->off, "%s: offsets is null", what);
    }
    FUSG_CHECK(gauss_w && radius >= 0 && radius <= ii::MAX_RADIUS, "%s: gauss_w (host, radius + 1 doubles) with radius in 0..%d, got %d", what,
               ii::MAX_RADIUS, radius);
    FUSG_CHECK(max_h >= 0 && max_w >= 0 && max_h <= frame->h && max_w <= frame->w, "%s: max_box_h / max_box_w (%d, %d) must lie within the frame", what,
               max_h, max_w);
    FUSG_CHECK(f32_nchw(img, V, 3) || (V == 0 && img && img->n == 0), "%s: img must be f32 [V, 3, %d, %d]", what, ii::R, ii::R);
    const fusg_tensor* one[3] = {gray, edge, mask};
    const char* names[3] = {"gray", "edge", "mask"};
    for (int i = 0; i < 3; ++i)
        FUSG_CHECK(f32_nchw(one[i], V, 1) || (V == 0 && one[i] && one[i]->n == 0), "%s: %s must be f32 [V, 1, %d, %d]", what, names[i], ii::R, ii::R);
    if (V == 0) { k.V = 0; return FUSG_OK; }
    FUSG_CHECK(boxes, "%s: boxes is null", what);
    FUSG_CHECK(scratch && (((uintptr_t)scratch) & 15) == 0, "%s: scratch must be 16-byte aligned (fusg_inpaint_inputs_scratch_bytes)", what);
    const ii::Scratch sl = ii::scratch_layout(V, max_h, max_w);
    char* sc = (char*)scratch;
    k.frame = (const unsigned char*)frame->data; k.fsh = frame->sh; k.fsw = frame->sw; k.H = (int)frame->h; k.W = (int)frame->w;
    if (!pm) { k.det = (const unsigned char*)det->data; k.dsn = det->sn; k.dsh = det->sh; k.dsw = det->sw; }
    else { k.det = nullptr; k.bm = pm->data; k.bm_off = pm->off; k.bm_n = (long)pm->n; k.bm_f32 = pm->dtype == FUSG_F32; }
    k.boxes = boxes;
    k.img = f32out(*img); k.gray = f32out(*gray); k.edge = f32out(*edge); k.mask = f32out(*mask);
    k.dil = (unsigned char*)sc; k.gv = (int16_t*)(sc + sl.off_gv); k.s = (double*)(sc + sl.off_s); k.bits = (uint64_t*)(sc + sl.off_bits);
    k.dil_v = sl.dil_v; k.V = (int)V; k.max_h = max_h; k.max_w = max_w;
    k.el = ii::ellipse();
    g.radius = radius;
    for (int i = 0; i <= ii::MAX_RADIUS; ++i) g.w[i] = i <= radius ? gauss_w[i] : 0.0;
    return FUSG_OK;
}

static int inpaint_launch(InpaintK k, ii::Gauss g, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int tiles_x = (k.max_w + DT_W - 1) / DT_W, tiles_y = (k.max_h + DT_H - 1) / DT_H;
    if (tiles_x > 0 && tiles_y > 0)
        hipLaunchKernelGGL(inpaint_dilate_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)k.V), dim3(256), 0, st, k, tiles_x);
    hipLaunchKernelGGL(inpaint_box_kernel, dim3(ii::R, (unsigned)k.V), dim3(ii::R), 0, st, k);
    hipLaunchKernelGGL(inpaint_smooth_kernel, dim3(ii::R, (unsigned)k.V), dim3(ii::R), 0, st, k, g);
    hipLaunchKernelGGL(inpaint_nms_kernel, dim3(ii::WPR * (ii::R / NT_H), (unsigned)k.V), dim3(256), 0, st, k);
    hipLaunchKernelGGL(inpaint_hysteresis_kernel, dim3((unsigned)k.V), dim3(HY_WORDS), 0, st, k);
    FUSG_LAUNCH_CHECK("inpaint_inputs");
    return FUSG_OK;
}

extern "C" int64_t fusg_inpaint_inputs_scratch_bytes(int32_t V, int32_t max_box_h, int32_t max_box_w) {
    if (V < 0 || max_box_h < 0 || max_box_w < 0) return -1;
    return (int64_t)ii::scratch_layout(V, max_box_h, max_box_w).total;
}

extern "C" int fusg_inpaint_inputs(const fusg_tensor* frame, const fusg_tensor* det_masks, const int32_t* boxes, const double* gauss_w,
                                   int32_t radius, int32_t max_box_h, int32_t max_box_w, const fusg_tensor* img, const fusg_tensor* gray,
                                   const fusg_tensor* edge, const fusg_tensor* mask, void* scratch, void* stream) {
    InpaintK k{};
    ii::Gauss g{};
    const int rc = inpaint_check(frame, det_masks, nullptr, boxes, gauss_w, radius, max_box_h, max_box_w, img, gray, edge, mask, scratch, "inpaint_inputs", k, g);
    if (rc != FUSG_OK || k.V == 0) return rc;
    return fusg::plan_dispatch(inpaint_launch, stream, k, g);     // the table is copied: a recorded call does not keep gauss_w
}

extern "C" int fusg_inpaint_inputs_boxed(const fusg_tensor* frame, const void* box_masks, int32_t mask_dtype, int64_t n_elems,
                                         const int64_t* offsets, const int32_t* boxes, const double* gauss_w, int32_t radius,
                                         int32_t max_box_h, int32_t max_box_w, const fusg_tensor* img, const fusg_tensor* gray,
                                         const fusg_tensor* edge, const fusg_tensor* mask, void* scratch, void* stream) {
    InpaintK k{};
    ii::Gauss g{};
    const PackedMasks pm{box_masks, mask_dtype, n_elems, offsets};
    const int rc = inpaint_check(frame, nullptr, &pm, boxes, gauss_w, radius, max_box_h, max_box_w, img, gray, edge, mask, scratch, "inpaint_inputs_boxed", k, g);
    if (rc != FUSG_OK || k.V == 0) return rc;
    return fusg::plan_dispatch(inpaint_launch, stream, k, g);
}

// ---- host twin: the same header's code on the CPU in plain loops (no GPU needed); every pointer is a host pointer
static int inpaint_host(const InpaintK& k, const ii::Gauss& g, const char* what) {
    const int32_t* boxes = k.boxes;
    for (int v = 0; v < k.V; ++v) {
        const int32_t* b = boxes + v * 4;
        FUSG_CHECK(ii::box_ok(b, k.H, k.W, k.max_h, k.max_w),
                   "%s: box %d = (%d, %d, %d, %d) must lie in the %d x %d frame and within max_box %d x %d", what, v, b[0], b[1], b[2],
                   b[3], k.W, k.H, k.max_w, k.max_h);
        FUSG_CHECK(k.det || packed_ok(k.bm_off[v], b[3] - b[1], b[2] - b[0], k.bm_n),
                   "%s: the %d x %d mask of box %d at offset %lld leaves the buffer of %ld elements", what, b[3] - b[1], b[2] - b[0], v,
                   (long long)k.bm_off[v], k.bm_n);
    }
    constexpr int R = ii::R, WPR = ii::WPR;
    double* row_m = new double[2 * R * R];                        // the axis-0 Gaussians of one image
    double* row_f = row_m + R * R;
    uint64_t* kept = new uint64_t[2 * HY_WORDS];
    for (int v = 0; v < k.V; ++v) {
        const ii::Box bx = vehicle_box(k, v);
        const MaskSrc src = mask_src(k, v, bx);
        for (int y = 0; y < bx.bh; ++y)
            for (int x = 0; x < bx.bw; ++x)
                k.dil[(long)v * k.dil_v + (long)y * k.max_w + x] = (unsigned char)ii::dilate_px(
                    [&](int yy, int xx) { return src.px(yy, xx); }, y, x, bx.bh, bx.bw, k.el);
        for (int y = 0; y < R; ++y)
            for (int x = 0; x < R; ++x) box_pass_px(k, v, y, x);
        const int16_t* gv = k.gv + (long)v * R * R;
        double* S = k.s + (long)v * R * R;
        for (int y = 0; y < R; ++y)
            for (int x = 0; x < R; ++x) {
                row_m[y * R + x] = smooth_axis0(gv, y, x, 0, g);
                row_f[y * R + x] = smooth_axis0(gv, y, x, 1, g);
            }
        for (int y = 0; y < R; ++y)
            for (int x = 0; x < R; ++x) S[y * R + x] = smooth_axis1(row_m + y * R, row_f + y * R, x, g);
        const auto clampi = [](int a) { return a < 0 ? 0 : (a > R - 1 ? R - 1 : a); };
        const auto s = [&](int i, int j) { return S[clampi(i) * R + clampi(j)]; };
        const auto valid = [&](int i, int j) { return (unsigned)i < (unsigned)R && (unsigned)j < (unsigned)R && gv[i * R + j] >= 0; };
        const auto mag = [&](int i, int j) {
            double gi, gj;
            ii::sobel_px(s, i, j, gi, gj);
            return ii::magnitude(gi, gj);
        };
        uint64_t* bits = k.bits + (long)v * 2 * HY_WORDS;
        for (int t = 0; t < 2 * HY_WORDS; ++t) bits[t] = 0;
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < R; ++j) {
                const int code = nms_code(s, valid, mag, i, j);
                if (code >= 1) bits[i * WPR + (j >> 6)] |= (uint64_t)1 << (j & 63);
                if (code == 2) bits[HY_WORDS + i * WPR + (j >> 6)] |= (uint64_t)1 << (j & 63);
            }
        int cur = 0;
        for (int t = 0; t < HY_WORDS; ++t) kept[t] = bits[HY_WORDS + t];
        for (bool go = true; go;) {
            go = false;
            const uint64_t* kc = kept + cur * HY_WORDS;
            for (int t = 0; t < HY_WORDS; ++t) {
                const uint64_t now = ii::hysteresis_word([&](int yy, int ww) {
                    return ((unsigned)yy < (unsigned)R && (unsigned)ww < (unsigned)WPR) ? kc[yy * WPR + ww] : (uint64_t)0;
                }, bits[t], t / WPR, t % WPR);
                kept[(cur ^ 1) * HY_WORDS + t] = now;
                go = go || now != kc[t];
            }
            cur ^= 1;
        }
        for (int p = 0; p < R * R; ++p) {
            const int py = p / R, px = p % R;
            k.edge.p[(long)v * k.edge.sn + (long)py * k.edge.sh + (long)px * k.edge.sw] =
                (float)((kept[cur * HY_WORDS + py * WPR + (px >> 6)] >> (px & 63)) & 1);
        }
    }
    delete[] row_m;
    delete[] kept;
    return FUSG_OK;
}

extern "C" int fusg_inpaint_inputs_host(const fusg_tensor* frame, const fusg_tensor* det_masks, const int32_t* boxes, const double* gauss_w,
                                        int32_t radius, int32_t max_box_h, int32_t max_box_w, const fusg_tensor* img, const fusg_tensor* gray,
                                        const fusg_tensor* edge, const fusg_tensor* mask, void* scratch) {
    InpaintK k{};
    ii::Gauss g{};
    const int rc = inpaint_check(frame, det_masks, nullptr, boxes, gauss_w, radius, max_box_h, max_box_w, img, gray, edge, mask, scratch, "inpaint_inputs_host", k, g);
    if (rc != FUSG_OK || k.V == 0) return rc;
    return inpaint_host(k, g, "inpaint_inputs_host");
}

extern "C" int fusg_inpaint_inputs_boxed_host(const fusg_tensor* frame, const void* box_masks, int32_t mask_dtype, int64_t n_elems,
                                              const int64_t* offsets, const int32_t* boxes, const double* gauss_w, int32_t radius,
                                              int32_t max_box_h, int32_t max_box_w, const fusg_tensor* img, const fusg_tensor* gray,
                                              const fusg_tensor* edge, const fusg_tensor* mask, void* scratch) {
    InpaintK k{};
    ii::Gauss g{};
    const PackedMasks pm{box_masks, mask_dtype, n_elems, offsets};
    const int rc = inpaint_check(frame, nullptr, &pm, boxes, gauss_w, radius, max_box_h, max_box_w, img, gray, edge, mask, scratch, "inpaint_inputs_boxed_host", k, g);
    if (rc != FUSG_OK || k.V == 0) return rc;
    return inpaint_host(k, g, "inpaint_inputs_boxed_host");
}
