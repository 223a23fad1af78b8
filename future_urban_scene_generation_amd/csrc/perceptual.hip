// The Gram matrix of an fp32 activation over its pixels and the per-row L1 distance of two fp32 tensors, on the device
// (include/fusg.h: fusg_gram_f32, fusg_abs_diff_rows_f32) with host twins that walk the same order of sums (perceptual.h
// states both orders).  Off every product pass: nothing calls these unless asked.
//   gram chunk kernel   one workgroup of 256 per (image, pixel chunk, pair (I, J) of 64-channel super tiles, I <= J).  A block
//                       of PB pixels x (64 channels of I | 64 channels of J) is staged in LDS once - the next block's loads
//                       are in flight while this one is contracted - and BOTH operands of v_mfma_f32_32x32x2_f32 come from
//                       it: lane (r = l & 31, h = l >> 5) of wave (si, sj) feeds channel 32 si + r of pixel 2 kk + h as A and
//                       channel 32 sj + r of the same pixel as B.  Pixels past the image and channels past C are staged as
//                       zeros.  The 64 x 64 fp32 partial goes to the caller's scratch with ordinary stores.
//   gram finish kernel  one thread per entry (i <= j): the chunk partials in ascending order in float64, / (H W C), one
//                       rounding to fp32, both triangles written.
//   abs-diff kernels    per-workgroup float64 partials of |a - b| through the strides, then one wave per row.
// No atomics anywhere: a row's bits depend on nothing but its own values, in a fixed order of sums.
#include <vector>
#include "common.h"
#include "perceptual.h"

namespace fusg {

typedef float pc_f32x16 __attribute__((ext_vector_type(16)));

struct GramK {
    const float* x; long sn, sh, sw;
    int B, C, H, W, T, NP, Kc, nch, dense;
    long HW;
    float* part; float* out;
};
struct AbsIn { const float* p; long sn, sc, sh, sw; };
struct AbsK { AbsIn a, b; int B, C, H, W, G; long n; double* part; double* out; };

FUSG_HD long abs_off(const AbsIn& t, int r, long i, int C, int W) {      // element i of row r, order (y, x, c)
    const long c = i % C, q = i / C;
    return (long)r * t.sn + (q / W) * t.sh + (q % W) * t.sw + c * t.sc;
}

// ------------------------------------------------------------------------------------------------ device kernels
__device__ __forceinline__ double wave_tree(double v) {           // lane 0: pc::tree64 of the wave's values
    for (int off = pc::LANES / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

__global__ __launch_bounds__(pc::WG) void gram_chunk_kernel(const GramK k) {
    constexpr int ST = pc::ST, SUB = pc::SUB, PB = pc::PB, PITCH = 2 * ST + 32, NQ = PB / 2;
    __shared__ float s[PB * PITCH];
    const int t = threadIdx.x, l = t & 63, w = t >> 6, si = w >> 1, sj = w & 1;
    const int b = blockIdx.y, pair = blockIdx.x % k.NP, ch = blockIdx.x / k.NP;
    int I = 0, rem = pair;
    while (rem >= k.T - I) { rem -= k.T - I; ++I; }
    const int J = I + rem;
    const bool diag = I == J;
    const int jb = diag ? 0 : ST;
    const long p0 = (long)ch * k.Kc, p1 = p0 + k.Kc < k.HW ? p0 + k.Kc : k.HW;
    // staging: thread t owns column t & 127 of rows (t >> 7), + 2, ...
    const int col = t & (2 * ST - 1), r0 = t >> 7;
    const int cch = col < ST ? I * ST + col : J * ST + col - ST;
    const bool col_ok = cch < k.C && (col < ST || !diag);
    const float* xb = k.x + (long)b * k.sn + cch;
    float v[NQ];
    auto load = [&](long pb) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const long p = pb + r0 + 2 * q;
            float f = 0.f;
            if (col_ok && p < p1) f = k.dense ? xb[p * k.sw] : xb[(p / k.W) * k.sh + (p % k.W) * k.sw];
            v[q] = f;
        }
    };
    pc_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const bool mine = !(diag && si > sj);
    const int arow = (l >> 5) * PITCH + si * SUB + (l & 31), brow = (l >> 5) * PITCH + jb + sj * SUB + (l & 31);
    load(p0);
    for (long pb = p0; pb < p1; pb += PB) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NQ; ++q) s[(r0 + 2 * q) * PITCH + col] = v[q];
        __syncthreads();
        if (pb + PB < p1) load(pb + PB);
        if (mine) {
#pragma unroll
            for (int kk = 0; kk < NQ; ++kk)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s[2 * kk * PITCH + arow], s[2 * kk * PITCH + brow], acc, 0, 0, 0);
        }
    }
    if (mine) {
        float* dst = k.part + ((((long)b * k.nch + ch) * k.NP + pair) * ST + si * SUB) * ST + sj * SUB + (l & 31);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) dst[((reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5)) * ST] = acc[reg];
    }
}

__global__ __launch_bounds__(pc::WG) void gram_finish_kernel(const GramK k) {
    constexpr int ST = pc::ST;
    const long idx = (long)blockIdx.x * pc::WG + threadIdx.x;
    const int b = blockIdx.y, i = (int)(idx / k.C), j = (int)(idx % k.C);
    if (i >= k.C || i > j) return;
    const long tile = (long)ST * ST;
    const float* p = k.part + (long)b * k.nch * k.NP * tile + ((long)pc::pair_index(i / ST, j / ST, k.T) * ST + i % ST) * ST + j % ST;
    double sum = 0.0;
    for (int ch = 0; ch < k.nch; ++ch) sum += (double)p[(long)ch * k.NP * tile];
    const float g = pc::gram_entry(sum, k.C, k.HW);
    float* o = k.out + (long)b * k.C * k.C;
    o[(long)i * k.C + j] = g;
    o[(long)j * k.C + i] = g;
}

__global__ __launch_bounds__(pc::WG) void abs_diff_partial_kernel(const AbsK k) {
    __shared__ double w_sum[pc::WG / pc::LANES];
    const int t = threadIdx.x, r = blockIdx.y;
    double s = 0.0;
    for (long i = (long)blockIdx.x * pc::WG + t; i < k.n; i += (long)k.G * pc::WG)
        s += fabs((double)k.a.p[abs_off(k.a, r, i, k.C, k.W)] - (double)k.b.p[abs_off(k.b, r, i, k.C, k.W)]);
    s = wave_tree(s);
    if ((t & 63) == 0) w_sum[t >> 6] = s;
    __syncthreads();
    if (t == 0) k.part[(long)r * k.G + blockIdx.x] = ((w_sum[0] + w_sum[1]) + w_sum[2]) + w_sum[3];
}

__global__ __launch_bounds__(pc::LANES) void abs_diff_finish_kernel(const AbsK k) {
    const int r = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < k.G; i += pc::LANES) s += k.part[(long)r * k.G + i];
    s = wave_tree(s);
    if (threadIdx.x == 0) k.out[r] = s;
}

}  // namespace fusg

using namespace fusg;

// ------------------------------------------------------------------------------------------------ host side
static bool gram_sizes_ok(long B, long Cn, long H, long W) {
    return B >= 0 && B < pc::MAX_B && Cn >= 1 && Cn <= pc::MAX_C && H >= 1 && W >= 1 && H <= pc::MAX_HW && W <= pc::MAX_HW &&
           H * W <= pc::MAX_HW;
}

static int gram_check(const fusg_tensor* x, float* out, void* scratch, bool need_scratch, const char* what, GramK& k) {
    FUSG_CHECK(x && x->dtype == FUSG_F32, "%s: x must be an f32 [B, C, H, W] descriptor", what);
    FUSG_CHECK(gram_sizes_ok(x->n, x->c, x->h, x->w), "%s: x is [%lld, %lld, %lld, %lld]; C must be in 1..%d, H W in 1..%d, B < %d", what,
               (long long)x->n, (long long)x->c, (long long)x->h, (long long)x->w, pc::MAX_C, pc::MAX_HW, pc::MAX_B);
    FUSG_CHECK(x->n == 0 || x->c == 1 || x->sc == 1, "%s: x must have channel stride 1 (the NHWC-physical layout), got %lld", what, (long long)x->sc);
    k.B = (int)x->n;
    if (k.B == 0) return FUSG_OK;
    FUSG_CHECK(x->data && out, "%s: x or out is null", what);
    k.x = (const float*)x->data; k.sn = x->sn; k.sh = x->sh; k.sw = x->sw;
    k.C = (int)x->c; k.H = (int)x->h; k.W = (int)x->w; k.HW = (long)x->h * x->w;
    k.T = pc::tiles(k.C); k.NP = pc::pairs(k.T);
    k.Kc = pc::gram_chunk(k.C, k.HW); k.nch = pc::gram_chunks(k.C, k.HW);
    k.dense = k.H == 1 || x->sh == x->w * x->sw;
    k.out = out;
    if (need_scratch) {
        FUSG_CHECK(scratch && (((uintptr_t)scratch) & 15) == 0, "%s: scratch must be 16-byte aligned (fusg_gram_scratch_bytes)", what);
        k.part = (float*)scratch;
    }
    return FUSG_OK;
}

static int gram_launch(GramK k, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gram_chunk_kernel, dim3((unsigned)(k.NP * k.nch), (unsigned)k.B), dim3(pc::WG), 0, st, k);
    hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)(((long)k.C * k.C + pc::WG - 1) / pc::WG), (unsigned)k.B), dim3(pc::WG), 0, st, k);
    FUSG_LAUNCH_CHECK("gram_f32");
    return FUSG_OK;
}

extern "C" int32_t fusg_gram_chunk_pixels(int32_t C, int64_t HW) {
    if (C < 1 || C > pc::MAX_C || HW < 1 || HW > pc::MAX_HW) return -1;
    return pc::gram_chunk(C, (long)HW);
}

extern "C" int64_t fusg_gram_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    if (!gram_sizes_ok(B, C, H, W)) return -1;
    const int64_t n = (int64_t)B * pc::gram_partials(C, (long)H * W) * (int64_t)sizeof(float);
    return (n + 15) / 16 * 16;
}

extern "C" int fusg_gram_f32(const fusg_tensor* x, float* out, void* scratch, void* stream) {
    GramK k{};
    const int rc = gram_check(x, out, scratch, true, "gram_f32", k);
    if (rc != FUSG_OK || k.B == 0) return rc;
    return fusg::plan_dispatch(gram_launch, stream, k);
}

// the host twin: per entry one fmaf chain per chunk in pixel order, the chunks in ascending order in float64
extern "C" int fusg_gram_f32_host(const fusg_tensor* x, float* out) {
    GramK k{};
    const int rc = gram_check(x, out, nullptr, false, "gram_f32_host", k);
    if (rc != FUSG_OK || k.B == 0) return rc;
    std::vector<float> xt((size_t)k.C * k.HW);                    // [channel][pixel]
    for (int b = 0; b < k.B; ++b) {
        for (long p = 0; p < k.HW; ++p)
            for (int c = 0; c < k.C; ++c) xt[(size_t)c * k.HW + p] = k.x[(long)b * k.sn + (p / k.W) * k.sh + (p % k.W) * k.sw + c];
        float* o = out + (long)b * k.C * k.C;
        for (int i = 0; i < k.C; ++i)
            for (int j = i; j < k.C; ++j) {
                const float* xi = xt.data() + (size_t)i * k.HW;
                const float* xj = xt.data() + (size_t)j * k.HW;
                double sum = 0.0;
                for (int ch = 0; ch < k.nch; ++ch) {
                    const long p0 = (long)ch * k.Kc, p1 = p0 + k.Kc < k.HW ? p0 + k.Kc : k.HW;
                    float acc = 0.f;
                    for (long p = p0; p < p1; ++p) acc = fmaf(xi[p], xj[p], acc);
                    sum += (double)acc;
                }
                const float g = pc::gram_entry(sum, k.C, k.HW);
                o[(long)i * k.C + j] = g;
                o[(long)j * k.C + i] = g;
            }
    }
    return FUSG_OK;
}

// ---- per-row L1
static bool abs_sizes_ok(long B, long Cn, long H, long W) {
    return B >= 0 && B < pc::MAX_B && Cn >= 1 && H >= 1 && W >= 1 && Cn < (1L << 31) && H < (1L << 31) && W < (1L << 31) &&
           Cn * H < (1L << 31) && Cn * H * W < (1L << 31);
}

static int abs_check(const fusg_tensor* a, const fusg_tensor* b, double* out, void* scratch, bool need_scratch, const char* what, AbsK& k) {
    FUSG_CHECK(a && b && a->dtype == FUSG_F32 && b->dtype == FUSG_F32, "%s: a and b must be f32 [B, C, H, W] descriptors", what);
    FUSG_CHECK(same_shape(*a, *b), "%s: a is [%lld, %lld, %lld, %lld], b is [%lld, %lld, %lld, %lld]", what, (long long)a->n, (long long)a->c,
               (long long)a->h, (long long)a->w, (long long)b->n, (long long)b->c, (long long)b->h, (long long)b->w);
    FUSG_CHECK(abs_sizes_ok(a->n, a->c, a->h, a->w), "%s: a is [%lld, %lld, %lld, %lld]; C H W must be in 1..2^31 - 1, B < %d", what,
               (long long)a->n, (long long)a->c, (long long)a->h, (long long)a->w, pc::MAX_B);
    k.B = (int)a->n;
    if (k.B == 0) return FUSG_OK;
    FUSG_CHECK(a->data && b->data && out, "%s: a, b or out is null", what);
    k.a = AbsIn{(const float*)a->data, a->sn, a->sc, a->sh, a->sw};
    k.b = AbsIn{(const float*)b->data, b->sn, b->sc, b->sh, b->sw};
    k.C = (int)a->c; k.H = (int)a->h; k.W = (int)a->w;
    k.n = (long)a->c * a->h * a->w;
    k.G = pc::abs_groups(k.n);
    k.out = out;
    if (need_scratch) {
        FUSG_CHECK(scratch && (((uintptr_t)scratch) & 15) == 0, "%s: scratch must be 16-byte aligned (fusg_abs_diff_rows_scratch_bytes)", what);
        k.part = (double*)scratch;
    }
    return FUSG_OK;
}

static int abs_launch(AbsK k, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(abs_diff_partial_kernel, dim3((unsigned)k.G, (unsigned)k.B), dim3(pc::WG), 0, st, k);
    hipLaunchKernelGGL(abs_diff_finish_kernel, dim3((unsigned)k.B), dim3(pc::LANES), 0, st, k);
    FUSG_LAUNCH_CHECK("abs_diff_rows_f32");
    return FUSG_OK;
}

extern "C" int64_t fusg_abs_diff_rows_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    if (!abs_sizes_ok(B, C, H, W)) return -1;
    const int64_t n = (int64_t)B * pc::abs_groups((long)C * H * W) * (int64_t)sizeof(double);
    return (n + 15) / 16 * 16;
}

extern "C" int fusg_abs_diff_rows_f32(const fusg_tensor* a, const fusg_tensor* b, double* out, void* scratch, void* stream) {
    AbsK k{};
    const int rc = abs_check(a, b, out, scratch, true, "abs_diff_rows_f32", k);
    if (rc != FUSG_OK || k.B == 0) return rc;
    return fusg::plan_dispatch(abs_launch, stream, k);
}

extern "C" int fusg_abs_diff_rows_f32_host(const fusg_tensor* a, const fusg_tensor* b, double* out) {
    AbsK k{};
    const int rc = abs_check(a, b, out, nullptr, false, "abs_diff_rows_f32_host", k);
    if (rc != FUSG_OK || k.B == 0) return rc;
    constexpr int NW = pc::WG / pc::LANES;
    std::vector<double> part(k.G);
    for (int r = 0; r < k.B; ++r) {
        for (int g = 0; g < k.G; ++g) {
            double acc[pc::WG];
            for (int t = 0; t < pc::WG; ++t) {
                double s = 0.0;
                for (long i = (long)g * pc::WG + t; i < k.n; i += (long)k.G * pc::WG)
                    s += fabs((double)k.a.p[abs_off(k.a, r, i, k.C, k.W)] - (double)k.b.p[abs_off(k.b, r, i, k.C, k.W)]);
                acc[t] = s;
            }
            double w[NW];
            for (int q = 0; q < NW; ++q) w[q] = pc::tree64(acc + q * pc::LANES);
            part[g] = ((w[0] + w[1]) + w[2]) + w[3];
        }
        double lanes[pc::LANES];
        for (int l = 0; l < pc::LANES; ++l) {
            lanes[l] = 0.0;
            for (int i = l; i < k.G; i += pc::LANES) lanes[l] += part[i];
        }
        out[r] = pc::tree64(lanes);
    }
    return FUSG_OK;
}
