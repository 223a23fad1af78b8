// The plane homography fit of warp_learn/planes_utils.py (find_homography) written once for host and device, in double
// precision: Hartley normalisation, direct linear transform through a cyclic Jacobi eigen-decomposition of the 9 x 9
// A^T A, Levenberg-Marquardt refinement for more than four points, and the 3 x 3 inverse the warp consumes; plus the
// visibility / symmetry gate and the slot rule of warp_jobs / warp_planes_batch.
//
// One fit is one serial instruction stream.  Its matrices live in a caller-provided workspace that is addressed with a
// stride (Ws): on the host a dense array, on the device a slice of LDS in which lane l owns the doubles l, l + stride,
// ... (consecutive lanes hit consecutive banks), so nothing that is indexed at run time sits in scratch memory.  The
// small fixed-size arrays below (a DLT row, a Jacobian row, the 3 x 3 matrices) are only ever indexed by fully unrolled
// loops and stay in registers.  Only +, -, *, / and sqrt are used and the translation unit is compiled with
// -ffp-contract=off: all of them are correctly rounded on both sides, so the host and the device results are equal bit
// for bit (tests/test_gpu_homography.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HG_FN __host__ __device__ static inline
#else
#define HG_FN static inline
#endif
#define HG_UNROLL _Pragma("unroll")

namespace fusg {
namespace hg {

constexpr int MAXP = 8;                  // points per fit (planes_utils.MAX_VERTS)
constexpr int WS_DOUBLES = 194;          // 32 point coordinates + 2 x 81 (A^T A and its eigenvectors; reused by LM: 8 x 9)
constexpr double EPS = 2.220446049250313e-16;       // np.finfo(np.float64).eps
constexpr double TINY = 2.2250738585072014e-308;    // np.finfo(np.float64).tiny

#if defined(__HIPCC__)
#define HG_MEMBER __host__ __device__
#else
#define HG_MEMBER
#endif
struct WsView {                          // a piece of the strided workspace: w[i] = base[(off + i) * stride]
    double* p;
    int stride;
    HG_MEMBER double& operator[](int i) const { return p[(long)i * stride]; }
};
HG_FN WsView view(double* base, int stride, int off) { WsView v; v.p = base + (long)off * stride; v.stride = stride; return v; }

HG_FN double dabs(double x) { return x < 0.0 ? -x : x; }
HG_FN double dsqrt(double x) { return __builtin_sqrt(x); }

// Cyclic Jacobi on the symmetric n x n matrix A (row-major, both triangles kept); V receives the eigenvectors as columns
// and the eigenvalues end on A's diagonal.  A rotation (p, q) is chosen so that A[p][q] becomes 0 (set exactly); from the
// fourth sweep on, an element that no longer changes either of its diagonal entries when added 100-fold is set to 0
// without a rotation (Rutishauser's rule), so the off-diagonal sum reaches 0 exactly and the loop ends.
HG_FN void jacobi9(const WsView A, const WsView V) {
    constexpr int N = 9;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) V[i * N + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) off += dabs(A[p * N + q]);
        if (off == 0.0) break;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p * N + q];
                if (apq == 0.0) continue;
                const double app = A[p * N + p], aqq = A[q * N + q];
                const double g = 100.0 * dabs(apq);
                if (sweep > 3 && dabs(app) + g == dabs(app) && dabs(aqq) + g == dabs(aqq)) {
                    A[p * N + q] = 0.0;
                    A[q * N + p] = 0.0;
                    continue;
                }
                const double theta = (aqq - app) / (2.0 * apq);
                double t;
                if (dabs(theta) > 1e150) t = 0.5 / theta;                // theta^2 would overflow
                else {
                    t = 1.0 / (dabs(theta) + dsqrt(theta * theta + 1.0));
                    if (theta < 0.0) t = -t;
                }
                const double c = 1.0 / dsqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < N; ++k) {                            // A <- A J
                    const double akp = A[k * N + p], akq = A[k * N + q];
                    A[k * N + p] = c * akp - s * akq;
                    A[k * N + q] = s * akp + c * akq;
                }
                for (int k = 0; k < N; ++k) {                            // A <- J^T A
                    const double apk = A[p * N + k], aqk = A[q * N + k];
                    A[p * N + k] = c * apk - s * aqk;
                    A[q * N + k] = s * apk + c * aqk;
                }
                A[p * N + q] = 0.0;
                A[q * N + p] = 0.0;
                for (int k = 0; k < N; ++k) {                            // V <- V J
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - s * vkq;
                    V[k * N + q] = s * vkp + c * vkq;
                }
            }
    }
}

// Gaussian elimination with partial pivoting on the augmented n x (n + nrhs) matrix M (row pitch n + nrhs); the
// solutions replace the right-hand sides.  false when a pivot is zero or not a number.
HG_FN bool gauss(const WsView M, int n, int nrhs) {
    const int w = n + nrhs;
    for (int c = 0; c < n; ++c) {
        int piv = c;
        double best = dabs(M[c * w + c]);
        for (int i = c + 1; i < n; ++i) {
            const double a = dabs(M[i * w + c]);
            if (a > best) { best = a; piv = i; }
        }
        if (!(best > 0.0)) return false;
        if (piv != c)
            for (int j = 0; j < w; ++j) {
                const double a = M[c * w + j];
                M[c * w + j] = M[piv * w + j];
                M[piv * w + j] = a;
            }
        const double d = M[c * w + c];
        for (int i = c + 1; i < n; ++i) {
            const double f = M[i * w + c] / d;
            for (int j = c; j < w; ++j) M[i * w + j] = M[i * w + j] - f * M[c * w + j];
        }
    }
    for (int r = 0; r < nrhs; ++r)
        for (int i = n - 1; i >= 0; --i) {
            double s = M[i * w + n + r];
            for (int j = i + 1; j < n; ++j) s -= M[i * w + j] * M[j * w + n + r];
            M[i * w + n + r] = s / M[i * w + i];
        }
    return true;
}

HG_FN void mat3_mul(const double a[9], const double b[9], double o[9]) {
    HG_UNROLL
    for (int i = 0; i < 3; ++i)
        HG_UNROLL
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = (a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j];
}

// Inverse of a 3 x 3 matrix by LU with partial pivoting (solve H X = I); false when H is singular.  ws: 18 doubles.
HG_FN bool inverse3(const double H[9], double inv[9], const WsView ws) {
    HG_UNROLL
    for (int i = 0; i < 3; ++i)
        HG_UNROLL
        for (int j = 0; j < 3; ++j) { ws[i * 6 + j] = H[i * 3 + j]; ws[i * 6 + 3 + j] = i == j ? 1.0 : 0.0; }
    const bool ok = gauss(ws, 3, 3);
    HG_UNROLL
    for (int i = 0; i < 3; ++i)
        HG_UNROLL
        for (int j = 0; j < 3; ++j) inv[i * 3 + j] = ok ? ws[i * 6 + 3 + j] : 0.0;
    return ok;
}

// sum of squared reprojection residuals of the points under (h, 1)
HG_FN double lm_cost(const double h[8], const WsView pts, int n) {
    double c = 0.0;
    for (int i = 0; i < n; ++i) {
        const double sx = pts[i * 4], sy = pts[i * 4 + 1];
        const double p0 = (h[0] * sx + h[1] * sy) + h[2], p1 = (h[3] * sx + h[4] * sy) + h[5], pw = (h[6] * sx + h[7] * sy) + 1.0;
        const double rx = p0 / pw - pts[i * 4 + 2], ry = p1 / pw - pts[i * 4 + 3];
        c += rx * rx;
        c += ry * ry;
    }
    return c;
}

// find_homography(src, dst): src_xy / dst_xy = n points (x, y) as doubles.  false where the Python returns None (fewer
// than four points, a zero deviation, rank loss, a vanishing H[2][2]).  ws: WS_DOUBLES doubles of workspace.
template <class PX>
HG_FN bool find_homography(PX src_xy, PX dst_xy, int n, double H[9], double* ws_base, int ws_stride) {
    HG_UNROLL
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
    if (n < 4 || n > MAXP) return false;
    const WsView pts = view(ws_base, ws_stride, 0);            // [n][4]: sx, sy, dx, dy
    const WsView A = view(ws_base, ws_stride, 32), V = view(ws_base, ws_stride, 32 + 81);
    double cs0 = 0.0, cs1 = 0.0, cd0 = 0.0, cd1 = 0.0;
    for (int i = 0; i < n; ++i) {
        const double sx = (double)src_xy[2 * i], sy = (double)src_xy[2 * i + 1], dx = (double)dst_xy[2 * i], dy = (double)dst_xy[2 * i + 1];
        pts[i * 4] = sx; pts[i * 4 + 1] = sy; pts[i * 4 + 2] = dx; pts[i * 4 + 3] = dy;
        cs0 += sx; cs1 += sy; cd0 += dx; cd1 += dy;
    }
    const double dn = (double)n;
    cs0 /= dn; cs1 /= dn; cd0 /= dn; cd1 /= dn;
    double ss0 = 0.0, ss1 = 0.0, sd0 = 0.0, sd1 = 0.0;
    for (int i = 0; i < n; ++i) {
        ss0 += dabs(pts[i * 4] - cs0); ss1 += dabs(pts[i * 4 + 1] - cs1);
        sd0 += dabs(pts[i * 4 + 2] - cd0); sd1 += dabs(pts[i * 4 + 3] - cd1);
    }
    ss0 /= dn; ss1 /= dn; sd0 /= dn; sd1 /= dn;
    if (!(ss0 >= EPS && ss1 >= EPS && sd0 >= EPS && sd1 >= EPS)) return false;
    ss0 = 1.0 / ss0; ss1 = 1.0 / ss1; sd0 = 1.0 / sd0; sd1 = 1.0 / sd1;
    // ---- DLT: A^T A accumulated one equation at a time
    for (int i = 0; i < 81; ++i) A[i] = 0.0;
    for (int i = 0; i < n; ++i) {
        const double x = (pts[i * 4] - cs0) * ss0, y = (pts[i * 4 + 1] - cs1) * ss1;
        const double u = (pts[i * 4 + 2] - cd0) * sd0, v = (pts[i * 4 + 3] - cd1) * sd1;
        const double r0[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y, -u};
        const double r1[9] = {0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y, -v};
        HG_UNROLL
        for (int a = 0; a < 9; ++a)
            HG_UNROLL
            for (int b = 0; b < 9; ++b) A[a * 9 + b] = (A[a * 9 + b] + r0[a] * r0[b]) + r1[a] * r1[b];
    }
    jacobi9(A, V);
    int k0 = 0;
    double e0 = A[0], emax = A[0];
    for (int i = 1; i < 9; ++i) {
        const double e = A[i * 10];
        if (e < e0) { e0 = e; k0 = i; }
        if (e > emax) emax = e;
    }
    double e1 = emax;                                          // second smallest eigenvalue
    for (int i = 0; i < 9; ++i)
        if (i != k0 && A[i * 10] < e1) e1 = A[i * 10];
    if (e1 < 1e-12 * (emax > 1e-300 ? emax : 1e-300)) return false;
    double Hn[9];
    HG_UNROLL
    for (int i = 0; i < 9; ++i) Hn[i] = V[i * 9 + k0];
    const double Tdi[9] = {1.0 / sd0, 0.0, cd0, 0.0, 1.0 / sd1, cd1, 0.0, 0.0, 1.0};
    const double Ts[9] = {ss0, 0.0, -cs0 * ss0, 0.0, ss1, -cs1 * ss1, 0.0, 0.0, 1.0};
    double T[9], Hd[9];
    mat3_mul(Tdi, Hn, T);
    mat3_mul(T, Ts, Hd);
    if (dabs(Hd[8]) < TINY) return false;
    double h[8];
    HG_UNROLL
    for (int i = 0; i < 8; ++i) h[i] = Hd[i] / Hd[8];
    if (n > 4) {                                               // Levenberg-Marquardt on the 8 free parameters
        const WsView M = view(ws_base, ws_stride, 32);         // JtJ | -g as an 8 x 9 tableau, over the (finished) A
        const WsView JtJ = view(ws_base, ws_stride, 32 + 81);  // 8 x 8 + g[8]
        double lam = 1e-3;
        double cost = lm_cost(h, pts, n);
        for (int it = 0; it < 10; ++it) {
            for (int i = 0; i < 72; ++i) JtJ[i] = 0.0;
            for (int i = 0; i < n; ++i) {
                const double sx = pts[i * 4], sy = pts[i * 4 + 1];
                const double p0 = (h[0] * sx + h[1] * sy) + h[2], p1 = (h[3] * sx + h[4] * sy) + h[5], pw = (h[6] * sx + h[7] * sy) + 1.0;
                const double rx = p0 / pw - pts[i * 4 + 2], ry = p1 / pw - pts[i * 4 + 3];
                const double w2 = pw * pw;
                const double j0[8] = {sx / pw, sy / pw, 1.0 / pw, 0.0, 0.0, 0.0, -p0 * sx / w2, -p0 * sy / w2};
                const double j1[8] = {0.0, 0.0, 0.0, sx / pw, sy / pw, 1.0 / pw, -p1 * sx / w2, -p1 * sy / w2};
                HG_UNROLL
                for (int a = 0; a < 8; ++a) {
                    HG_UNROLL
                    for (int b = 0; b < 8; ++b) JtJ[a * 8 + b] = (JtJ[a * 8 + b] + j0[a] * j0[b]) + j1[a] * j1[b];
                    JtJ[64 + a] = (JtJ[64 + a] + j0[a] * rx) + j1[a] * ry;
                }
            }
            for (int a = 0; a < 8; ++a) {
                for (int b = 0; b < 8; ++b) M[a * 9 + b] = a == b ? JtJ[a * 8 + a] + lam * JtJ[a * 8 + a] : JtJ[a * 8 + b];
                M[a * 9 + 8] = -JtJ[64 + a];
            }
            if (!gauss(M, 8, 1)) break;                        // singular system: keep the parameters reached so far
            double h2[8], smax = 0.0;
            HG_UNROLL
            for (int a = 0; a < 8; ++a) {
                const double st = M[a * 9 + 8];
                h2[a] = h[a] + st;
                if (dabs(st) > smax) smax = dabs(st);
            }
            const double cost2 = lm_cost(h2, pts, n);
            if (cost2 <= cost) {
                HG_UNROLL
                for (int a = 0; a < 8; ++a) h[a] = h2[a];
                cost = cost2;
                lam *= 0.1;
                if (smax < 1e-13) break;
            } else {
                lam *= 10.0;
            }
        }
    }
    HG_UNROLL
    for (int i = 0; i < 8; ++i) H[i] = h[i];
    H[8] = 1.0;
    return true;
}

// The gate of warp_jobs: the destination slot of source plane i (its own, or for one of the two symmetric planes whose own
// destination is hidden, its partner's), -1 when plane i is not warped.  Visibilities are 0 / 1; sym_a = sym_b = -1: no
// symmetric pair.
HG_FN int gate(int i, const uint8_t* src_vis, const uint8_t* dst_vis, int sym_a, int sym_b) {
    if (!src_vis[i]) return -1;
    if (i == sym_a || i == sym_b) {
        const int other = i == sym_a ? sym_b : sym_a;
        if (dst_vis[i]) return i;
        return dst_vis[other] ? other : -1;
    }
    return dst_vis[i] ? i : -1;
}

// The slot rule of warp_planes_batch: the job that writes slot j is the one of the highest source plane among the jobs
// (target[i] == j, both fits valid) - a later job overwrites an earlier one.  -1: none.
template <class T, class B>
HG_FN int slot_source(int j, int P, const T* target, const B* job_ok) {
    for (int i = P - 1; i >= 0; --i)
        if (target[i] == j && job_ok[i]) return i;
    return -1;
}

enum { STATUS_NONE = 0, STATUS_JOB = 1, STATUS_FIT_INVALID = 2 };

}  // namespace hg
}  // namespace fusg
