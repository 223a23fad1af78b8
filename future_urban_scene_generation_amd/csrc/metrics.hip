// Per-image SSIM / PSNR / difference counts of two uint8 batches, and the counts behind EdgeConnect's EdgeAccuracy, on the
// device (include/fusg.h: fusg_image_metrics_u8, fusg_edge_counts, fusg_sq_diff_sum_f32) with host twins by the same code
// (metrics.h).  Off every product pass: nothing calls these unless asked.
//   tile kernel    one workgroup of 256 per (image, 16 x 16 tile of valid positions): both images' 26 x 26 x C pixels staged
//                  once in LDS as bytes (the integer statistics of the tile's own pixels are taken on the way), then per
//                  channel the row pass (26 x 16 five-sum records, float64, LDS) and the column pass + SSIM formula, one
//                  position per thread; the tile's SSIM sum by wave shuffles, then the four waves through LDS in order.
//                  Partials go to the caller's scratch with ordinary stores.
//   finish kernel  one wave per image: lane l adds tiles l, l + 64, ... in order, the same tree, the six columns.
// No atomics anywhere: an image's row of the table depends on nothing but its own pixels, in a fixed order of sums.
#include "common.h"
#include "metrics.h"

namespace fusg {

struct U8In { const unsigned char* p; long sn, sc, sh, sw; };
struct MetricsK {
    U8In a, b;
    int B, H, W, C, tiles_x, tiles_y;
    double* out;
    double* p_ssim; unsigned long long* p_sse; unsigned* p_nd; unsigned* p_mx;
    im::Taps taps;
};
struct F32In { const float* p; long sn, sh, sw; };
struct EdgeK { F32In x, y; int B, H, W; float thr; long long* out; };

static inline U8In u8in(const fusg_tensor& t) { return U8In{(const unsigned char*)t.data, t.sn, t.sc, t.sh, t.sw}; }
static inline F32In f32in(const fusg_tensor& t) { return F32In{(const float*)t.data, t.sn, t.sh, t.sw}; }
FUSG_HD int px(const U8In& t, int r, int y, int x, int c) { return (int)t.p[(long)r * t.sn + (long)y * t.sh + (long)x * t.sw + (long)c * t.sc]; }

// ------------------------------------------------------------------------------------------------ device kernels
template <class T>
__device__ __forceinline__ T wave_tree(T v) {                     // lane 0: im::tree64 of the wave's values
    for (int off = im::LANES / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
    for (int off = im::LANES / 2; off > 0; off >>= 1) { const unsigned o = __shfl_down(v, off); v = o > v ? o : v; }
    return v;
}

__global__ __launch_bounds__(im::NT) void image_metrics_tile_kernel(const MetricsK k) {
    constexpr int LT = im::LT, TILE = im::TILE, NW = im::NT / im::LANES;
    __shared__ unsigned char ta[im::MAXC * LT * LT], tb[im::MAXC * LT * LT];
    __shared__ im::Sums hs[LT * TILE];
    __shared__ double w_ssim[NW];
    __shared__ unsigned w_int[3][NW];
    const int r = blockIdx.y, t = threadIdx.x;
    const int tix = blockIdx.x % k.tiles_x, tiy = blockIdx.x / k.tiles_x, tx0 = tix * TILE, ty0 = tiy * TILE;
    const int own_x1 = im::own_end(tix, k.tiles_x, k.W), own_y1 = im::own_end(tiy, k.tiles_y, k.H);
    unsigned sse = 0, nd = 0, mx = 0;                             // a tile's sse <= 26 * 26 * 4 * 65025 < 2^32
    for (int i = t; i < LT * LT * k.C; i += im::NT) {
        const int c = i % k.C, p = i / k.C, lx = p % LT, ly = p / LT, y = ty0 + ly, x = tx0 + lx;
        int va = 0, vb = 0;
        if (y < k.H && x < k.W) {
            va = px(k.a, r, y, x, c);
            vb = px(k.b, r, y, x, c);
            if (y < own_y1 && x < own_x1) {
                const unsigned d = (unsigned)(va > vb ? va - vb : vb - va);
                sse += d * d;
                nd += d != 0;
                mx = d > mx ? d : mx;
            }
        }
        ta[(c * LT + ly) * LT + lx] = (unsigned char)va;
        tb[(c * LT + ly) * LT + lx] = (unsigned char)vb;
    }
    __syncthreads();
    const int ox = t % TILE, oy = t / TILE;
    const bool valid = ty0 + oy < k.H - im::APRON && tx0 + ox < k.W - im::APRON;
    double acc = 0.0;
    for (int c = 0; c < k.C; ++c) {
        for (int i = t; i < LT * TILE; i += im::NT) {
            const unsigned char* ra = ta + (c * LT + i / TILE) * LT + i % TILE;
            const unsigned char* rb = tb + (c * LT + i / TILE) * LT + i % TILE;
            hs[i] = im::row_sums([&](int q) { return (int)ra[q]; }, [&](int q) { return (int)rb[q]; }, k.taps);
        }
        __syncthreads();
        if (valid) acc += im::ssim_px(im::col_sums([&](int q) { return hs[(oy + q) * TILE + ox]; }, k.taps));
        __syncthreads();
    }
    acc = wave_tree(acc);
    sse = wave_tree(sse);
    nd = wave_tree(nd);
    mx = wave_max(mx);
    if ((t & (im::LANES - 1)) == 0) {
        const int w = t / im::LANES;
        w_ssim[w] = acc; w_int[0][w] = sse; w_int[1][w] = nd; w_int[2][w] = mx;
    }
    __syncthreads();
    if (t == 0) {
        double s = w_ssim[0];
        unsigned e = w_int[0][0], n = w_int[1][0], m = w_int[2][0];
        for (int w = 1; w < NW; ++w) {
            s += w_ssim[w]; e += w_int[0][w]; n += w_int[1][w];
            m = w_int[2][w] > m ? w_int[2][w] : m;
        }
        const long slot = (long)r * gridDim.x + blockIdx.x;
        k.p_ssim[slot] = s; k.p_sse[slot] = e; k.p_nd[slot] = n; k.p_mx[slot] = m;
    }
}

__global__ __launch_bounds__(im::LANES) void image_metrics_finish_kernel(const MetricsK k) {
    __shared__ unsigned long long l_sse[im::LANES], l_nd[im::LANES];
    __shared__ unsigned l_mx[im::LANES];
    const int r = blockIdx.x, l = threadIdx.x, T = k.tiles_x * k.tiles_y;
    double s = 0.0;
    unsigned long long e = 0, n = 0;
    unsigned m = 0;
    for (int i = l; i < T; i += im::LANES) {
        const long slot = (long)r * T + i;
        s += k.p_ssim[slot]; e += k.p_sse[slot]; n += k.p_nd[slot];
        m = k.p_mx[slot] > m ? k.p_mx[slot] : m;
    }
    s = wave_tree(s);
    l_sse[l] = e; l_nd[l] = n; l_mx[l] = m;
    __syncthreads();
    if (l == 0) {
        for (int q = 1; q < im::LANES; ++q) { e += l_sse[q]; n += l_nd[q]; m = l_mx[q] > m ? l_mx[q] : m; }
        im::finish_row(s, e, n, m, k.H, k.W, k.C, k.out + (long)r * im::COLS);
    }
}

// one workgroup per row: #(x > t), #(y > t), #(x > t and y > t)
__global__ __launch_bounds__(256) void edge_counts_kernel(const EdgeK k) {
    __shared__ unsigned w_cnt[3][4];
    const int r = blockIdx.x, t = threadIdx.x;
    const long n = (long)k.H * k.W;
    unsigned rel = 0, sel = 0, tp = 0;
    for (long i = t; i < n; i += 256) {
        const long yy = i / k.W, xx = i % k.W;
        const bool bx = k.x.p[(long)r * k.x.sn + yy * k.x.sh + xx * k.x.sw] > k.thr;
        const bool by = k.y.p[(long)r * k.y.sn + yy * k.y.sh + xx * k.y.sw] > k.thr;
        rel += bx; sel += by; tp += bx && by;
    }
    rel = wave_tree(rel); sel = wave_tree(sel); tp = wave_tree(tp);
    if ((t & 63) == 0) { w_cnt[0][t >> 6] = rel; w_cnt[1][t >> 6] = sel; w_cnt[2][t >> 6] = tp; }
    __syncthreads();
    if (t < 3) k.out[(long)r * 3 + t] = (long long)w_cnt[t][0] + w_cnt[t][1] + w_cnt[t][2] + w_cnt[t][3];
}

// sum of (a - b)^2 of two float32 arrays in float64: block g's partial to out[1 + g] ...
constexpr int SQ_MAX_BLOCKS = 256, SQ_PER_BLOCK = 4096;
__global__ __launch_bounds__(256) void sq_diff_partial_kernel(const float* a, const float* b, long n, double* out) {
    __shared__ double w_sum[4];
    const int t = threadIdx.x;
    double s = 0.0;
    for (long i = (long)blockIdx.x * 256 + t; i < n; i += (long)gridDim.x * 256) {
        const double d = (double)a[i] - (double)b[i];
        s += d * d;
    }
    s = wave_tree(s);
    if ((t & 63) == 0) w_sum[t >> 6] = s;
    __syncthreads();
    if (t == 0) out[1 + blockIdx.x] = ((w_sum[0] + w_sum[1]) + w_sum[2]) + w_sum[3];
}
// ... and the partials, lane l taking l, l + 64, ..., to out[0]
__global__ __launch_bounds__(im::LANES) void sq_diff_finish_kernel(int G, double* out) {
    double s = 0.0;
    for (int i = threadIdx.x; i < G; i += im::LANES) s += out[1 + i];
    s = wave_tree(s);
    if (threadIdx.x == 0) out[0] = s;
}

}  // namespace fusg

using namespace fusg;

// ------------------------------------------------------------------------------------------------ host side
static bool u8_image(const fusg_tensor* t) {
    return t && t->dtype == FUSG_U8 && t->n >= 0 && t->n < (1 << 16) && t->c >= 1 && t->c <= im::MAXC && t->h >= im::WIN && t->w >= im::WIN &&
           t->h < 32768 && t->w < 32768;
}

static int metrics_check(const fusg_tensor* a, const fusg_tensor* b, double* out, void* scratch, bool need_scratch, const char* what, MetricsK& k) {
    FUSG_CHECK(u8_image(a) && u8_image(b), "%s: a and b must be u8 [B, C, H, W] descriptors with C in 1..%d, H and W in %d..32767, B < 65536", what,
               im::MAXC, im::WIN);
    FUSG_CHECK(same_shape(*a, *b), "%s: a is [%lld, %lld, %lld, %lld], b is [%lld, %lld, %lld, %lld]", what, (long long)a->n, (long long)a->c,
               (long long)a->h, (long long)a->w, (long long)b->n, (long long)b->c, (long long)b->h, (long long)b->w);
    k.B = (int)a->n;
    if (k.B == 0) return FUSG_OK;
    FUSG_CHECK(a->data && b->data && out, "%s: a, b or out is null", what);
    k.a = u8in(*a); k.b = u8in(*b);
    k.H = (int)a->h; k.W = (int)a->w; k.C = (int)a->c;
    const im::Tiling tl = im::tiling(k.H, k.W);
    k.tiles_x = tl.tiles_x; k.tiles_y = tl.tiles_y;
    k.out = out;
    k.taps = im::gauss_taps();
    if (need_scratch) {
        FUSG_CHECK(scratch && (((uintptr_t)scratch) & 15) == 0, "%s: scratch must be 16-byte aligned (fusg_image_metrics_scratch_bytes)", what);
        const im::Scratch sl = im::scratch_layout(k.B, (long)tl.tiles_x * tl.tiles_y);
        char* sc = (char*)scratch;
        k.p_ssim = (double*)sc; k.p_sse = (unsigned long long*)(sc + sl.off_sse); k.p_nd = (unsigned*)(sc + sl.off_nd);
        k.p_mx = (unsigned*)(sc + sl.off_mx);
    }
    return FUSG_OK;
}

static int metrics_launch(MetricsK k, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(image_metrics_tile_kernel, dim3((unsigned)(k.tiles_x * k.tiles_y), (unsigned)k.B), dim3(im::NT), 0, st, k);
    hipLaunchKernelGGL(image_metrics_finish_kernel, dim3((unsigned)k.B), dim3(im::LANES), 0, st, k);
    FUSG_LAUNCH_CHECK("image_metrics_u8");
    return FUSG_OK;
}

extern "C" int64_t fusg_image_metrics_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t C) {
    if (B < 0 || B >= (1 << 16) || H < im::WIN || W < im::WIN || H >= 32768 || W >= 32768 || C < 1 || C > im::MAXC) return -1;
    const im::Tiling tl = im::tiling(H, W);
    return (int64_t)im::scratch_layout(B, (long)tl.tiles_x * tl.tiles_y).total;
}

extern "C" int fusg_image_metrics_u8(const fusg_tensor* a, const fusg_tensor* b, double* out, void* scratch, void* stream) {
    MetricsK k{};
    const int rc = metrics_check(a, b, out, scratch, true, "image_metrics_u8", k);
    if (rc != FUSG_OK || k.B == 0) return rc;
    return fusg::plan_dispatch(metrics_launch, stream, k);
}

// the host twin: the tiles, the positions of a tile and the sums in the kernel's order
extern "C" int fusg_image_metrics_host(const fusg_tensor* a, const fusg_tensor* b, double* out) {
    MetricsK k{};
    const int rc = metrics_check(a, b, out, nullptr, false, "image_metrics_host", k);
    if (rc != FUSG_OK || k.B == 0) return rc;
    constexpr int LT = im::LT, TILE = im::TILE, NW = im::NT / im::LANES;
    const int T = k.tiles_x * k.tiles_y;
    double* part = new double[T];
    im::Sums* hs = new im::Sums[LT * TILE];
    for (int r = 0; r < k.B; ++r) {
        uint64_t sse = 0, nd = 0;
        uint32_t mx = 0;
        for (int y = 0; y < k.H; ++y)
            for (int x = 0; x < k.W; ++x)
                for (int c = 0; c < k.C; ++c) {
                    const int va = px(k.a, r, y, x, c), vb = px(k.b, r, y, x, c);
                    const uint32_t d = (uint32_t)(va > vb ? va - vb : vb - va);
                    sse += (uint64_t)d * d;
                    nd += d != 0;
                    mx = d > mx ? d : mx;
                }
        for (int ti = 0; ti < T; ++ti) {
            const int tx0 = (ti % k.tiles_x) * TILE, ty0 = (ti / k.tiles_x) * TILE;
            double acc[im::NT];
            for (int t = 0; t < im::NT; ++t) acc[t] = 0.0;
            for (int c = 0; c < k.C; ++c) {
                for (int i = 0; i < LT * TILE; ++i) {
                    const int y = ty0 + i / TILE, x = tx0 + i % TILE;
                    const auto at = [&](const U8In& s, int q) { return y < k.H && x + q < k.W ? px(s, r, y, x + q, c) : 0; };
                    hs[i] = im::row_sums([&](int q) { return at(k.a, q); }, [&](int q) { return at(k.b, q); }, k.taps);
                }
                for (int t = 0; t < im::NT; ++t) {
                    const int ox = t % TILE, oy = t / TILE;
                    if (ty0 + oy < k.H - im::APRON && tx0 + ox < k.W - im::APRON)
                        acc[t] += im::ssim_px(im::col_sums([&](int q) { return hs[(oy + q) * TILE + ox]; }, k.taps));
                }
            }
            double s = im::tree64(acc);
            for (int w = 1; w < NW; ++w) s += im::tree64(acc + w * im::LANES);
            part[ti] = s;
        }
        double lanes[im::LANES];
        for (int l = 0; l < im::LANES; ++l) {
            lanes[l] = 0.0;
            for (int i = l; i < T; i += im::LANES) lanes[l] += part[i];
        }
        im::finish_row(im::tree64(lanes), sse, nd, mx, k.H, k.W, k.C, out + (long)r * im::COLS);
    }
    delete[] part;
    delete[] hs;
    return FUSG_OK;
}

// ---- edge counts
static int edge_check(const fusg_tensor* x, const fusg_tensor* y, int64_t* out, const char* what, EdgeK& k) {
    FUSG_CHECK(x && y && x->dtype == FUSG_F32 && y->dtype == FUSG_F32 && x->c == 1 && y->c == 1 && x->n >= 0 && x->n < (1 << 20) && x->h >= 1 &&
               x->w >= 1 && x->h < 32768 && x->w < 32768, "%s: x and y must be f32 [B, 1, H, W] descriptors, H and W in 1..32767", what);
    FUSG_CHECK(same_shape(*x, *y), "%s: x is [%lld, 1, %lld, %lld], y is [%lld, 1, %lld, %lld]", what, (long long)x->n, (long long)x->h,
               (long long)x->w, (long long)y->n, (long long)y->h, (long long)y->w);
    k.B = (int)x->n;
    if (k.B == 0) return FUSG_OK;
    FUSG_CHECK(x->data && y->data && out, "%s: x, y or out is null", what);
    k.x = f32in(*x); k.y = f32in(*y);
    k.H = (int)x->h; k.W = (int)x->w;
    k.out = (long long*)out;
    return FUSG_OK;
}

static int edge_launch(EdgeK k, void* stream) {
    hipLaunchKernelGGL(edge_counts_kernel, dim3((unsigned)k.B), dim3(256), 0, (hipStream_t)stream, k);
    FUSG_LAUNCH_CHECK("edge_counts");
    return FUSG_OK;
}

extern "C" int fusg_edge_counts(const fusg_tensor* x, const fusg_tensor* y, float threshold, int64_t* out, void* stream) {
    EdgeK k{};
    const int rc = edge_check(x, y, out, "edge_counts", k);
    if (rc != FUSG_OK || k.B == 0) return rc;
    k.thr = threshold;
    return fusg::plan_dispatch(edge_launch, stream, k);
}

extern "C" int fusg_edge_counts_host(const fusg_tensor* x, const fusg_tensor* y, float threshold, int64_t* out) {
    EdgeK k{};
    const int rc = edge_check(x, y, out, "edge_counts_host", k);
    if (rc != FUSG_OK || k.B == 0) return rc;
    for (int r = 0; r < k.B; ++r) {
        int64_t rel = 0, sel = 0, tp = 0;
        for (int yy = 0; yy < k.H; ++yy)
            for (int xx = 0; xx < k.W; ++xx) {
                const bool bx = k.x.p[(long)r * k.x.sn + (long)yy * k.x.sh + (long)xx * k.x.sw] > threshold;
                const bool by = k.y.p[(long)r * k.y.sn + (long)yy * k.y.sh + (long)xx * k.y.sw] > threshold;
                rel += bx; sel += by; tp += bx && by;
            }
        out[r * 3 + 0] = rel; out[r * 3 + 1] = sel; out[r * 3 + 2] = tp;
    }
    return FUSG_OK;
}

// ---- float sum of squared differences (PSNR of float tensors)
static int sq_diff_launch(const float* a, const float* b, int64_t n, double* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const long want = (n + SQ_PER_BLOCK - 1) / SQ_PER_BLOCK;
    const int G = (int)(want < 1 ? 1 : (want > SQ_MAX_BLOCKS ? SQ_MAX_BLOCKS : want));
    hipLaunchKernelGGL(sq_diff_partial_kernel, dim3((unsigned)G), dim3(256), 0, st, a, b, (long)n, out);
    hipLaunchKernelGGL(sq_diff_finish_kernel, dim3(1), dim3(im::LANES), 0, st, G, out);
    FUSG_LAUNCH_CHECK("sq_diff_sum_f32");
    return FUSG_OK;
}

extern "C" int fusg_sq_diff_sum_f32(const float* a, const float* b, int64_t n, double* out, void* stream) {
    FUSG_CHECK(n >= 0 && out && (n == 0 || (a && b)), "sq_diff_sum_f32: a, b (n floats, n >= 0) and out (%d doubles) must be given", 1 + SQ_MAX_BLOCKS);
    return fusg::plan_dispatch(sq_diff_launch, stream, a, b, n, out);
}
