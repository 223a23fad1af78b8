// fusg_up2_edge_fix: the outermost ring of nn.Upsample(2) -> ReflectionPad2d(2) -> 5x5, added onto the phase-form output
// (up2_edge.h has the identity and the data layout).  Exact fp32 on the matrix pipe; one kernel for every precision mode.
#include "up2_edge.h"

namespace fusg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Workgroup = 256 threads = 4 waves; it owns SEG = 16 RT consecutive output pixels of one side of one image and all Cout
// columns: wave v the column tiles [v CTW, (v + 1) CTW) of 16, for all RT row tiles (a wave past the last column tile only
// stages).  K runs over Cin in chunks of 32 channels: the SEG + 4 frame elements of the chunk are formed on the fly
// (f(a) - f(b), f applied to each before the subtraction) into one of two LDS buffers while the previous chunk is contracted,
// one barrier per chunk.  Nothing here depends on the batch: grid = (segments, 2 sides, B).
template <int RT, int CTW>
__global__ __launch_bounds__(256) void up2_edge_kernel(const Up2EdgeK p) {
    constexpr int SEG = RT * 16, NE = SEG + 4, ITEMS = NE * (UP2E_CH / 4), NIT = (ITEMS + 255) / 256;
    __shared__ __attribute__((aligned(16))) float lds[2][NE * UP2E_PITCH];
    __shared__ double red[2][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int seg = blockIdx.x, side = blockIdx.y, b = blockIdx.z;
    const int l = p.axis == 0 ? p.w : p.h, L = 2 * l;              // low-res / output pixels along the line
    const int la = p.axis == 0 ? p.h : p.w;                         // low-res extent across it
    const int a1 = side == 0 ? 1 : la - 2, a0 = side == 0 ? 0 : la - 1;
    const long s_al = p.axis == 0 ? p.ssw : p.ssh, s_ac = p.axis == 0 ? p.ssh : p.ssw;
    const float* s1 = p.src + (long)b * p.ssn + (long)a1 * s_ac;
    const float* s0 = p.src + (long)b * p.ssn + (long)a0 * s_ac;
    const int p0 = seg * SEG;
    const int q4 = (t & 7) * 4;                                     // this thread's four channels of a chunk

    // the frame elements this thread stages: the same ones in every chunk
    long off1[NIT], off0[NIT];
    bool live[NIT];
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        const int el = (t + 256 * k) >> 3;
        const int P = p0 - 2 + el;
        int j1 = 0, j0 = 0;
        bool ok = el < NE && P <= L + 1;
        if (P == -2) { j1 = 1; j0 = 0; ok = ok && p.axis == 0; }
        else if (P == L + 1) { j1 = l - 2; j0 = l - 1; ok = ok && p.axis == 0; }
        else if (ok) { const int c = P < 0 ? 0 : (P > L - 1 ? L - 1 : P); j1 = j0 = c >> 1; }
        live[k] = ok;
        off1[k] = (long)j1 * s_al + q4;
        off0[k] = (long)j0 * s_al + q4;
    }
    const float* sc_p = p.pre_relu_affine ? p.pre_scale + (long)b * p.pre_bstride + q4 : nullptr;
    const float* sh_p = p.pre_relu_affine ? p.pre_shift + (long)b * p.pre_bstride + q4 : nullptr;

    f32x4 v1[NIT], v0[NIT], sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    auto fetch = [&](int c) {
        const int c0 = c * UP2E_CH;
        if (p.pre_relu_affine) { sc = *(const f32x4*)(sc_p + c0); sh = *(const f32x4*)(sh_p + c0); }
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            if (live[k]) { v1[k] = *(const f32x4*)(s1 + off1[k] + c0); v0[k] = *(const f32x4*)(s0 + off0[k] + c0); }
        }
    };
    auto stage = [&](float* buf) {
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int el = (t + 256 * k) >> 3;
            if (el >= NE) continue;
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
            if (live[k]) {
                f32x4 a = v1[k], c = v0[k];
                if (p.pre_relu_affine) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { a[e] = fmaxf(fmaf(a[e], sc[e], sh[e]), 0.f); c[e] = fmaxf(fmaf(c[e], sc[e], sh[e]), 0.f); }
                }
                d = a - c;
            }
            *(f32x4*)(buf + el * UP2E_PITCH + q4) = d;
        }
    };

    const int nct = p.Cout >> 4, nc16 = p.Cin >> 4, nchunk = p.Cin / UP2E_CH;
    const int gside = 2 * p.axis + side;
    const bool active = wave * CTW < nct;
    f32x4 acc[RT][CTW];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < CTW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // The weights of a chunk (10 steps x CTW 16-byte loads per lane) are fetched a whole chunk ahead: with one workgroup per CU the
    // launch lives on loads in flight, and two loads per step kept it at a quarter of the matrix pipe's rate.  (CTW = 4 would
    // need 320 registers for two chunks: it fetches at the top of its own chunk.)
    constexpr bool AHEAD = CTW <= 2;
    f32x4 bw[5][2][CTW], bwn[5][2][CTW];
    auto fetch_w = [&](int c, f32x4 (&dstw)[5][2][CTW]) {
#pragma unroll
        for (int tap = 0; tap < 5; ++tap)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                for (int j = 0; j < CTW; ++j) {
                    const int ct = wave * CTW + j;
                    dstw[tap][hh][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (ct < nct)
                        dstw[tap][hh][j] = *(const f32x4*)(p.wedge + ((((long)(gside * 5 + tap) * nc16 + (2 * c + hh)) * nct + ct) * 64 + lane) * 4);
                }
    };

    if (active) fetch_w(0, bw);
    fetch(0);
    stage(lds[0]);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        if (c + 1 < nchunk) {
            fetch(c + 1);
            if (AHEAD && active) fetch_w(c + 1, bwn);
        }
        if (active) {
            const float* buf = lds[c & 1];
#pragma unroll
            for (int tap = 0; tap < 5; ++tap)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    f32x4 a[RT];
#pragma unroll
                    for (int i = 0; i < RT; ++i)
                        a[i] = *(const f32x4*)(buf + (i * 16 + (lane & 15) + tap) * UP2E_PITCH + hh * 16 + (lane >> 4) * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int i = 0; i < RT; ++i)
#pragma unroll
                            for (int j = 0; j < CTW; ++j)
                                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][e], bw[tap][hh][j][e], acc[i][j], 0, 0, 0);
                }
        }
        if (c + 1 < nchunk) {
            stage(lds[(c + 1) & 1]);
            if (active) {
                if (AHEAD) {
#pragma unroll
                    for (int tap = 0; tap < 5; ++tap)
#pragma unroll
                        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                            for (int j = 0; j < CTW; ++j) bw[tap][hh][j] = bwn[tap][hh][j];
                } else {
                    fetch_w(c + 1, bw);
                }
            }
        }
        __syncthreads();
    }

    // out += delta in place (accumulator row = (lane >> 4) * 4 + r, column = lane & 15), and the two moments of the change
    const long d_al = p.axis == 0 ? p.dsw : p.dsh;
    float* dline = p.dst + (long)b * p.dsn + (p.axis == 0 ? (side ? 2L * p.h - 1 : 0L) * p.dsh : (side ? 2L * p.w - 1 : 0L) * p.dsw);
    double sd = 0.0, sq = 0.0;
    if (active) {
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int j = 0; j < CTW; ++j) {
                const int ct = wave * CTW + j;
                if (ct >= nct) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pp = p0 + i * 16 + (lane >> 4) * 4 + r;
                    if (pp >= L) continue;
                    float* o = dline + (long)pp * d_al + ct * 16 + (lane & 15);
                    const float old = *o;
                    const float nw = old + acc[i][j][r];
                    *o = nw;
                    const double de = (double)nw - (double)old;        // the change as stored
                    sd += de;
                    sq += de * (2.0 * (double)old + de);
                }
            }
    }
    if (p.delta != nullptr) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { sd += __shfl_xor(sd, off, 64); sq += __shfl_xor(sq, off, 64); }
        if (lane == 0) { red[0][wave] = sd; red[1][wave] = sq; }
        __syncthreads();
        if (t == 0) {
            double* e = p.delta + ((long)b * p.n_entries + p.entry0 + side * p.nseg + seg) * 2;
            e[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
            e[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        }
    }
}

// pixels per workgroup along a line of L output pixels: by L alone
static inline int up2_edge_rt(long L) { return L >= 256 ? 4 : 2; }
static inline int up2_edge_nseg(long L) { const int seg = 16 * up2_edge_rt(L); return (int)((L + seg - 1) / seg); }

template <int RT>
static void up2_edge_launch_rt(const Up2EdgeK& k, dim3 grid, hipStream_t s) {
    if (k.Cout <= 64) hipLaunchKernelGGL((up2_edge_kernel<RT, 1>), grid, dim3(256), 0, s, k);
    else if (k.Cout <= 128) hipLaunchKernelGGL((up2_edge_kernel<RT, 2>), grid, dim3(256), 0, s, k);
    else hipLaunchKernelGGL((up2_edge_kernel<RT, 4>), grid, dim3(256), 0, s, k);
}

}  // namespace fusg

using namespace fusg;

static int up2_edge_impl(const fusg_tensor* src, int32_t pre_op, const float* pre_scale, const float* pre_shift, int64_t pre_bstride,
                         const float* wedge, const fusg_tensor* dst, double* delta, int32_t n_entries, void* stream) {
    FUSG_CHECK(src && dst && is_nhwc(*src) && is_nhwc(*dst) && wedge && (((uintptr_t)wedge) & 15) == 0, "up2_edge_fix: src / dst must be NHWC-physical, weights 16-byte aligned");
    FUSG_CHECK(src->h >= 2 && src->w >= 2 && src->h < (1 << 14) && src->w < (1 << 14) && src->n >= 1 && src->n <= 65535,
               "up2_edge_fix: low-res image %ld x %ld, batch %ld", (long)src->h, (long)src->w, (long)src->n);
    FUSG_CHECK(dst->n == src->n && dst->h == 2 * src->h && dst->w == 2 * src->w, "up2_edge_fix: dst is not the 2x image of src");
    FUSG_CHECK(src->c >= 32 && src->c % 32 == 0 && dst->c >= 16 && dst->c % 16 == 0 && dst->c <= 256,
               "up2_edge_fix: Cin %ld (multiple of 32) / Cout %ld (multiple of 16, <= 256)", (long)src->c, (long)dst->c);
    FUSG_CHECK(pre_op == FUSG_PRE_NONE || pre_op == FUSG_PRE_AFFINE_RELU, "up2_edge_fix: pre_op %d", pre_op);
    if (pre_op == FUSG_PRE_AFFINE_RELU)
        FUSG_CHECK(pre_scale && pre_shift && ((((uintptr_t)pre_scale) | ((uintptr_t)pre_shift)) & 15) == 0 && pre_bstride % 4 == 0 && pre_bstride >= 0,
                   "up2_edge_fix: affine pre-op needs 16-byte aligned scale / shift");
    const int nsw = up2_edge_nseg(2 * src->w), nsh = up2_edge_nseg(2 * src->h);
    FUSG_CHECK(!delta || (n_entries == 2 * nsw + 2 * nsh && (((uintptr_t)delta) & 7) == 0), "up2_edge_fix: delta buffer needs %d entries per image, got %d",
               2 * nsw + 2 * nsh, n_entries);
    Up2EdgeK k{};
    k.src = (const float*)src->data; k.ssn = src->sn; k.ssh = src->sh; k.ssw = src->sw;
    k.h = (int)src->h; k.w = (int)src->w; k.Cin = (int)src->c; k.Cout = (int)dst->c;
    k.pre_relu_affine = pre_op == FUSG_PRE_AFFINE_RELU;
    k.pre_scale = pre_scale; k.pre_shift = pre_shift; k.pre_bstride = pre_bstride;
    k.wedge = wedge;
    k.dst = (float*)dst->data; k.dsn = dst->sn; k.dsh = dst->sh; k.dsw = dst->sw;
    k.delta = delta; k.n_entries = n_entries;
    for (int axis = 0; axis < 2; ++axis) {                  // rows, then columns: a corner pixel is updated by both, in this order
        const long L = 2 * (axis == 0 ? src->w : src->h);
        k.axis = axis;
        k.nseg = axis == 0 ? nsw : nsh;
        k.entry0 = axis == 0 ? 0 : 2 * nsw;
        const dim3 grid((unsigned)k.nseg, 2, (unsigned)src->n);
        if (up2_edge_rt(L) == 4) up2_edge_launch_rt<4>(k, grid, (hipStream_t)stream);
        else up2_edge_launch_rt<2>(k, grid, (hipStream_t)stream);
        FUSG_LAUNCH_CHECK("up2_edge_fix");
    }
    return FUSG_OK;
}

extern "C" int fusg_up2_edge_entries(int32_t h, int32_t w) {
    if (h < 2 || w < 2) return 0;
    return 2 * up2_edge_nseg(2L * w) + 2 * up2_edge_nseg(2L * h);
}

extern "C" int fusg_up2_edge_fix(const fusg_tensor* src, int32_t pre_op, const float* pre_scale, const float* pre_shift, int64_t pre_bstride,
                                 const float* wedge, const fusg_tensor* dst, double* delta, int32_t n_entries, void* stream) {
    return fusg::plan_dispatch(up2_edge_impl, stream, src, pre_op, pre_scale, pre_shift, pre_bstride, wedge, dst, delta, n_entries);
}
