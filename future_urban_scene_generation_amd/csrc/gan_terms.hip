// The per-row sums behind the GAN objectives and the count-excluding 3 x 3 stride-2 average pool on the device
// (include/fusg.h: fusg_gan_terms_rows_f32, fusg_avgpool3s2_f32), with host twins that walk the same order of sums
// (gan_terms.h states both).  Off every product pass: nothing calls these unless asked.
//   terms partial kernel  one workgroup of 256 per (row, chunk): five float64 sums per thread over its elements of the chunk,
//                         the wave's 64 by cross-lane shuffles, the four waves through LDS, ordinary stores to scratch.
//   terms finish kernel   one wave per row: the chunk partials in a fixed order, n into column 0.
//   pool kernel           one thread per (output pixel, 4 channels); a partial last quad goes channel by channel.
// No atomics anywhere: a row's bits depend on nothing but its own values, in a fixed order of sums.
#include <vector>
#include "common.h"
#include "gan_terms.h"

namespace fusg {

typedef float gt_f32x4 __attribute__((ext_vector_type(4)));

struct GtIn { const float* p; long sn, sc, sh, sw; };
struct GtK {
    GtIn x, m;
    int B, C, H, W, Hm, Wm, G, has_mask;
    long n, K;
    float sy, sx;
    double label;
    double* part; double* out;
};
struct PoolK { const float* x; float* dst; int xCs, dCs, C, H, W, Ho, Wo; long total; };

// element i of row r, order (y, x, c): its offset in pred and the mask value at its pixel
FUSG_HD void gt_fetch(const GtK& k, int r, long i, float& xv, float& mv) {
    const long c = i % k.C, q = i / k.C;
    const int y = (int)(q / k.W), xx = (int)(q % k.W);
    xv = k.x.p[(long)r * k.x.sn + (long)y * k.x.sh + (long)xx * k.x.sw + c * k.x.sc];
    mv = 1.f;
    if (k.has_mask)
        mv = k.m.p[(long)r * k.m.sn + (long)gt::nearest_src(y, k.sy, k.Hm) * k.m.sh + (long)gt::nearest_src(xx, k.sx, k.Wm) * k.m.sw];
}

// one output value of the pool: the taps inside the image added to +0 in raster order, one division
FUSG_HD float pool_at(const float* x, long row_pitch, long pix_pitch, int H, int W, int oy, int ox) {
    float s = 0.f;
    int cnt = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int y = 2 * oy + dy;
        if (y < 0 || y >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = 2 * ox + dx;
            if (xx < 0 || xx >= W) continue;
            const float v = x[(long)y * row_pitch + (long)xx * pix_pitch];
            s += v;
            ++cnt;
        }
    }
    return s / (float)cnt;
}

// ------------------------------------------------------------------------------------------------ device kernels
__device__ __forceinline__ double gt_wave_tree(double v) {        // lane 0: gt::tree64 of the wave's values
    for (int off = gt::LANES / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

__global__ __launch_bounds__(gt::WG) void gan_terms_partial_kernel(const GtK k) {
    __shared__ double w_sum[gt::WG / gt::LANES][gt::SUMS];
    const int t = threadIdx.x, r = blockIdx.y, g = blockIdx.x;
    const long i0 = (long)g * k.K, i1 = i0 + k.K < k.n ? i0 + k.K : k.n;
    double acc[gt::SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long i = i0 + t; i < i1; i += gt::WG) {
        float xv, mv;
        gt_fetch(k, r, i, xv, mv);
        gt::add_terms(acc, xv, mv, k.label);
    }
#pragma unroll
    for (int c = 0; c < gt::SUMS; ++c) {
        const double s = gt_wave_tree(acc[c]);
        if ((t & 63) == 0) w_sum[t >> 6][c] = s;
    }
    __syncthreads();
    if (t < gt::SUMS) k.part[((long)r * k.G + g) * gt::SUMS + t] = ((w_sum[0][t] + w_sum[1][t]) + w_sum[2][t]) + w_sum[3][t];
}

__global__ __launch_bounds__(gt::LANES) void gan_terms_finish_kernel(const GtK k) {
    const int r = blockIdx.x;
    for (int c = 0; c < gt::SUMS; ++c) {
        double s = 0.0;
        for (int i = threadIdx.x; i < k.G; i += gt::LANES) s += k.part[((long)r * k.G + i) * gt::SUMS + c];
        s = gt_wave_tree(s);
        if (threadIdx.x == 0) k.out[(long)r * gt::COLUMNS + 1 + c] = s;
    }
    if (threadIdx.x == 0) k.out[(long)r * gt::COLUMNS] = (double)k.n;
}

__global__ __launch_bounds__(256) void avgpool3s2_kernel(const PoolK k) {
    const int C4 = (k.C + 3) >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < k.total; i += (long)gridDim.x * 256) {
        const int q = (int)(i % C4);
        long pix = i / C4;
        const int ox = (int)(pix % k.Wo); pix /= k.Wo;
        const int oy = (int)(pix % k.Ho);
        const long b = pix / k.Ho;
        const float* xb = k.x + b * (long)k.H * k.W * k.xCs + q * 4;
        float* d = k.dst + ((b * k.Ho + oy) * (long)k.Wo + ox) * k.dCs + q * 4;
        if (q * 4 + 4 <= k.C) {
            gt_f32x4 s = {0.f, 0.f, 0.f, 0.f};
            int cnt = 0;
            for (int dy = -1; dy <= 1; ++dy) {
                const int y = 2 * oy + dy;
                if (y < 0 || y >= k.H) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = 2 * ox + dx;
                    if (xx < 0 || xx >= k.W) continue;
                    const gt_f32x4 v = *(const gt_f32x4*)(xb + ((long)y * k.W + xx) * k.xCs);
                    s = s + v;
                    ++cnt;
                }
            }
            *(gt_f32x4*)d = s / (float)cnt;
        } else {
            for (int c = 0; q * 4 + c < k.C; ++c) d[c] = pool_at(xb + c, (long)k.W * k.xCs, k.xCs, k.H, k.W, oy, ox);
        }
    }
}

}  // namespace fusg

using namespace fusg;

// ------------------------------------------------------------------------------------------------ host side
static bool gt_sizes_ok(long B, long Cn, long H, long W) {
    return B >= 0 && B < gt::MAX_B && Cn >= 1 && H >= 1 && W >= 1 && Cn < (1L << 31) && H < (1L << 31) && W < (1L << 31) &&
           Cn * H < (1L << 31) && Cn * H * W < (1L << 31);
}

static int gt_check(const fusg_tensor* pred, const fusg_tensor* mask, float label, double* out, void* scratch, bool need_scratch,
                    const char* what, GtK& k) {
    FUSG_CHECK(pred && pred->dtype == FUSG_F32, "%s: pred must be an f32 [B, C, H, W] descriptor", what);
    FUSG_CHECK(gt_sizes_ok(pred->n, pred->c, pred->h, pred->w), "%s: pred is [%lld, %lld, %lld, %lld]; C H W must be in 1..2^31 - 1, B < %d",
               what, (long long)pred->n, (long long)pred->c, (long long)pred->h, (long long)pred->w, gt::MAX_B);
    k.B = (int)pred->n;
    const bool hm = mask && mask->data;
    if (hm)
        FUSG_CHECK(mask->dtype == FUSG_F32 && mask->n == pred->n && mask->c == 1 && mask->h >= 1 && mask->w >= 1 && mask->h < (1L << 24) &&
                   mask->w < (1L << 24), "%s: mask must be f32 [%lld, 1, Hm, Wm], got [%lld, %lld, %lld, %lld]", what, (long long)pred->n,
                   (long long)mask->n, (long long)mask->c, (long long)mask->h, (long long)mask->w);
    if (k.B == 0) return FUSG_OK;
    FUSG_CHECK(pred->data && out, "%s: pred or out is null", what);
    k.x = GtIn{(const float*)pred->data, pred->sn, pred->sc, pred->sh, pred->sw};
    k.C = (int)pred->c; k.H = (int)pred->h; k.W = (int)pred->w;
    k.has_mask = hm ? 1 : 0;
    if (hm) {
        k.m = GtIn{(const float*)mask->data, mask->sn, mask->sc, mask->sh, mask->sw};
        k.Hm = (int)mask->h; k.Wm = (int)mask->w;
        k.sy = (float)k.Hm / (float)k.H; k.sx = (float)k.Wm / (float)k.W;
    }
    k.n = (long)pred->c * pred->h * pred->w;
    k.G = gt::groups(k.n); k.K = gt::chunk(k.n);
    k.label = (double)label;
    k.out = out;
    if (need_scratch) {
        FUSG_CHECK(scratch && (((uintptr_t)scratch) & 15) == 0, "%s: scratch must be 16-byte aligned (fusg_gan_terms_scratch_bytes)", what);
        k.part = (double*)scratch;
    }
    return FUSG_OK;
}

static int gt_launch(GtK k, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gan_terms_partial_kernel, dim3((unsigned)k.G, (unsigned)k.B), dim3(gt::WG), 0, st, k);
    hipLaunchKernelGGL(gan_terms_finish_kernel, dim3((unsigned)k.B), dim3(gt::LANES), 0, st, k);
    FUSG_LAUNCH_CHECK("gan_terms_rows_f32");
    return FUSG_OK;
}

extern "C" int64_t fusg_gan_terms_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    if (!gt_sizes_ok(B, C, H, W)) return -1;
    const int64_t n = (int64_t)B * gt::groups((long)C * H * W) * gt::SUMS * (int64_t)sizeof(double);
    return (n + 15) / 16 * 16;
}

extern "C" int32_t fusg_gan_terms_columns(void) { return gt::COLUMNS; }

extern "C" int64_t fusg_gan_terms_chunk(int64_t n) { return n >= 1 && n < (1L << 31) ? gt::chunk((long)n) : -1; }

extern "C" int fusg_gan_terms_rows_f32(const fusg_tensor* pred, const fusg_tensor* mask, float label, double* out, void* scratch,
                                       void* stream) {
    GtK k{};
    const int rc = gt_check(pred, mask, label, out, scratch, true, "gan_terms_rows_f32", k);
    if (rc != FUSG_OK || k.B == 0) return rc;
    return fusg::plan_dispatch(gt_launch, stream, k);
}

extern "C" int fusg_gan_terms_rows_f32_host(const fusg_tensor* pred, const fusg_tensor* mask, float label, double* out) {
    GtK k{};
    const int rc = gt_check(pred, mask, label, out, nullptr, false, "gan_terms_rows_f32_host", k);
    if (rc != FUSG_OK || k.B == 0) return rc;
    constexpr int NW = gt::WG / gt::LANES;
    std::vector<double> part((size_t)k.G * gt::SUMS);
    std::vector<double> acc((size_t)gt::WG * gt::SUMS);
    for (int r = 0; r < k.B; ++r) {
        for (int g = 0; g < k.G; ++g) {
            const long i0 = (long)g * k.K, i1 = i0 + k.K < k.n ? i0 + k.K : k.n;
            for (int t = 0; t < gt::WG; ++t) {
                double* a = acc.data() + (size_t)t * gt::SUMS;
                for (int c = 0; c < gt::SUMS; ++c) a[c] = 0.0;
                for (long i = i0 + t; i < i1; i += gt::WG) {
                    float xv, mv;
                    gt_fetch(k, r, i, xv, mv);
                    gt::add_terms(a, xv, mv, k.label);
                }
            }
            for (int c = 0; c < gt::SUMS; ++c) {
                double w[NW];
                for (int q = 0; q < NW; ++q) {
                    double lanes[gt::LANES];
                    for (int l = 0; l < gt::LANES; ++l) lanes[l] = acc[(size_t)(q * gt::LANES + l) * gt::SUMS + c];
                    w[q] = gt::tree64(lanes);
                }
                part[(size_t)g * gt::SUMS + c] = ((w[0] + w[1]) + w[2]) + w[3];
            }
        }
        for (int c = 0; c < gt::SUMS; ++c) {
            double lanes[gt::LANES];
            for (int l = 0; l < gt::LANES; ++l) {
                lanes[l] = 0.0;
                for (int i = l; i < k.G; i += gt::LANES) lanes[l] += part[(size_t)i * gt::SUMS + c];
            }
            out[(long)r * gt::COLUMNS + 1 + c] = gt::tree64(lanes);
        }
        out[(long)r * gt::COLUMNS] = (double)k.n;
    }
    return FUSG_OK;
}

// ---- average pool
static int pool_check(const fusg_tensor* src, const fusg_tensor* dst, bool device, const char* what, PoolK& k) {
    FUSG_CHECK(src && dst && src->dtype == FUSG_F32 && dst->dtype == FUSG_F32, "%s: src and dst must be f32 descriptors", what);
    FUSG_CHECK(src->n >= 0 && src->c >= 1 && src->h >= 1 && src->w >= 1 && src->h < (1L << 24) && src->w < (1L << 24) && src->c < (1L << 24),
               "%s: src is [%lld, %lld, %lld, %lld]", what, (long long)src->n, (long long)src->c, (long long)src->h, (long long)src->w);
    FUSG_CHECK(dst->n == src->n && dst->c == src->c && dst->h == gt::pool_out(src->h) && dst->w == gt::pool_out(src->w),
               "%s: dst must be [%lld, %lld, %d, %d], got [%lld, %lld, %lld, %lld]", what, (long long)src->n, (long long)src->c,
               gt::pool_out(src->h), gt::pool_out(src->w), (long long)dst->n, (long long)dst->c, (long long)dst->h, (long long)dst->w);
    if (src->n == 0) { k.total = 0; return FUSG_OK; }
    if (device) {
        FUSG_CHECK(is_nhwc(*src) && is_nhwc(*dst), "%s: src and dst must be NHWC-physical (channel stride 1, pitch a multiple of 4, 16-byte aligned)", what);
    } else {
        FUSG_CHECK(src->data && dst->data && (src->c == 1 || (src->sc == 1 && dst->sc == 1)) && src->sw >= src->c && dst->sw >= dst->c &&
                   (src->h == 1 || src->sh == src->w * src->sw) && (src->n == 1 || src->sn == src->h * src->w * src->sw) &&
                   (dst->h == 1 || dst->sh == dst->w * dst->sw) && (dst->n == 1 || dst->sn == dst->h * dst->w * dst->sw),
                   "%s: src and dst must be NHWC-physical", what);
    }
    k.x = (const float*)src->data; k.dst = (float*)dst->data; k.xCs = (int)src->sw; k.dCs = (int)dst->sw;
    k.C = (int)src->c; k.H = (int)src->h; k.W = (int)src->w; k.Ho = (int)dst->h; k.Wo = (int)dst->w;
    k.total = src->n * dst->h * dst->w * ((src->c + 3) / 4);
    return FUSG_OK;
}

static int pool_impl(const fusg_tensor* src, const fusg_tensor* dst, void* stream) {
    PoolK k{};
    const int rc = pool_check(src, dst, true, "avgpool3s2_f32", k);
    if (rc != FUSG_OK || k.total == 0) return rc;
    long nb = (k.total + 255) / 256;
    if (nb > 16384) nb = 16384;
    hipLaunchKernelGGL(avgpool3s2_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, k);
    FUSG_LAUNCH_CHECK("avgpool3s2_f32");
    return FUSG_OK;
}
extern "C" int fusg_avgpool3s2_f32(const fusg_tensor* src, const fusg_tensor* dst, void* stream) { return fusg::plan_dispatch(pool_impl, stream, src, dst); }

extern "C" int fusg_avgpool3s2_f32_host(const fusg_tensor* src, const fusg_tensor* dst) {
    PoolK k{};
    const int rc = pool_check(src, dst, false, "avgpool3s2_f32_host", k);
    if (rc != FUSG_OK || k.total == 0) return rc;
    for (long b = 0; b < src->n; ++b)
        for (int oy = 0; oy < k.Ho; ++oy)
            for (int ox = 0; ox < k.Wo; ++ox)
                for (int c = 0; c < k.C; ++c)
                    k.dst[((b * k.Ho + oy) * (long)k.Wo + ox) * k.dCs + c] =
                        pool_at(k.x + b * (long)k.H * k.W * k.xCs + c, (long)k.W * k.xCs, k.xCs, k.H, k.W, oy, ox);
    return FUSG_OK;
}
