// The stage between the plane corner points and the plane warp, on the device: fusg_plane_homographies (include/fusg.h)
// gates the planes of every vehicle as warp_jobs does, fits H12 and H21 of every gated plane (homography.h: the same code
// the host twins below run), resolves the destination slots and writes the fixed-size (minv, index) tables that
// fusg_warp_perspective_indexed_u8 reads - no host arithmetic, no compaction, no atomics.
//
// One workgroup per vehicle, one lane per (source plane, direction): at most 16 lanes of one wavefront, each a serial fit
// of a few ten thousand dependent double operations.  The stage is latency-bound (a frame of 64 vehicles is 640 fits on
// 64 CUs), so the lanes are spent on independent fits rather than on the inside of one 9 x 9 problem.  Each lane's
// matrices sit in LDS, lane-interleaved (24.8 KB per workgroup): the kernel uses no scratch memory.
#include "common.h"
#include "homography.h"

namespace fusg {

constexpr int HG_LANES = 2 * hg::MAXP;

struct PlaneHomK {
    const int32_t* src_pts; const int32_t* dst_pts; const int32_t* nverts; const uint8_t* src_vis; const uint8_t* dst_vis;
    double* minv; int32_t* index; double* H; int32_t* status;
    int V, P, sym_a, sym_b;
};

// the fit of source plane i of vehicle v onto slot j (dir 0: H12 = src -> dst, 1: H21 = dst -> src)
HG_FN bool fit_plane(const PlaneHomK& k, int v, int i, int j, int dir, double H[9], double* ws, int stride) {
    const int n = k.nverts[i];
    const int32_t* s = k.src_pts + ((long)v * k.P + i) * hg::MAXP * 2;
    const int32_t* d = k.dst_pts + ((long)v * k.P + j) * hg::MAXP * 2;
    if (k.nverts[j] != n) {                                       // find_homography: len(d) != n
        HG_UNROLL
        for (int a = 0; a < 9; ++a) H[a] = 0.0;
        return false;
    }
    return dir ? hg::find_homography(d, s, n, H, ws, stride) : hg::find_homography(s, d, n, H, ws, stride);
}

// the table row of slot j of vehicle v from the vehicle's fits: Hs [2 * P][9], inv [P][9], target [P], job_ok [P]
HG_FN void write_slot(const PlaneHomK& k, int v, int j, const double* Hs, const double* inv, const int* target, const uint8_t* job_ok) {
    const int src = hg::slot_source(j, k.P, target, job_ok);
    const long row = (long)v * k.P + j;
    k.index[2 * row] = src >= 0 ? (int32_t)(v * k.P + src) : -1;
    k.index[2 * row + 1] = (int32_t)row;
    for (int a = 0; a < 9; ++a) k.minv[row * 9 + a] = src >= 0 ? inv[src * 9 + a] : 0.0;
    if (k.H)
        for (int a = 0; a < 18; ++a) k.H[row * 18 + a] = src >= 0 ? Hs[src * 18 + a] : 0.0;
    if (k.status) {
        int st = src >= 0 ? hg::STATUS_JOB : hg::STATUS_NONE;
        if (src < 0)
            for (int i = 0; i < k.P; ++i)
                if (target[i] == j) st = hg::STATUS_FIT_INVALID;
        k.status[row] = st;
    }
}

__global__ __launch_bounds__(HG_LANES) void plane_homographies_kernel(const PlaneHomK k) {
    __shared__ double ws[hg::WS_DOUBLES * HG_LANES];
    __shared__ double Hs[HG_LANES * 9], inv[hg::MAXP * 9];
    __shared__ int target[hg::MAXP];
    __shared__ uint8_t fit_ok[HG_LANES], job_ok[hg::MAXP];
    const int v = blockIdx.x, t = threadIdx.x, i = t >> 1, dir = t & 1;
    if (t < k.P) target[t] = hg::gate(t, k.src_vis + (long)v * k.P, k.dst_vis + (long)v * k.P, k.sym_a, k.sym_b);
    fit_ok[t] = 0;
    __syncthreads();
    if (i < k.P && target[i] >= 0) {
        double H[9];
        bool ok = fit_plane(k, v, i, target[i], dir, H, ws + t, HG_LANES);
        if (dir == 0) {
            double m[9];
            ok = hg::inverse3(H, m, hg::view(ws + t, HG_LANES, 32)) && ok;
            HG_UNROLL
            for (int a = 0; a < 9; ++a) inv[i * 9 + a] = m[a];
        }
        HG_UNROLL
        for (int a = 0; a < 9; ++a) Hs[t * 9 + a] = H[a];
        fit_ok[t] = ok;
    }
    __syncthreads();
    if (t < k.P) job_ok[t] = fit_ok[2 * t] && fit_ok[2 * t + 1];
    __syncthreads();
    if (t < k.P) write_slot(k, v, t, Hs, inv, target, job_ok);
}

}  // namespace fusg

using namespace fusg;

static int plane_hom_check(const PlaneHomK& k, const char* what) {
    FUSG_CHECK(k.V == 0 || (k.src_pts && k.dst_pts && k.src_vis && k.dst_vis && k.minv && k.index), "%s: null pointer", what);
    FUSG_CHECK(k.nverts, "%s: nverts is null", what);
    FUSG_CHECK(k.V >= 0 && k.P >= 1 && k.P <= hg::MAXP && (long)k.V * k.P < (1L << 24), "%s: V %d (>= 0), P %d (1..%d), V * P < 2^24", what,
               k.V, k.P, hg::MAXP);
    FUSG_CHECK((k.sym_a == -1 && k.sym_b == -1) || (k.sym_a >= 0 && k.sym_a < k.P && k.sym_b >= 0 && k.sym_b < k.P && k.sym_a != k.sym_b),
               "%s: symmetric planes %d, %d: two different planes of 0..%d, or -1, -1 for none", what, k.sym_a, k.sym_b, k.P - 1);
    return FUSG_OK;
}

static int plane_homographies_impl(const int32_t* src_pts, const int32_t* dst_pts, const int32_t* nverts, const uint8_t* src_vis,
                                   const uint8_t* dst_vis, int32_t V, int32_t P, int32_t sym_a, int32_t sym_b, double* minv,
                                   int32_t* index, double* H, int32_t* status, void* stream) {
    const PlaneHomK k{src_pts, dst_pts, nverts, src_vis, dst_vis, minv, index, H, status, V, P, sym_a, sym_b};
    const int rc = plane_hom_check(k, "plane_homographies");
    if (rc != FUSG_OK || V == 0) return rc;
    hipLaunchKernelGGL(plane_homographies_kernel, dim3((unsigned)V), dim3(HG_LANES), 0, (hipStream_t)stream, k);
    FUSG_LAUNCH_CHECK("plane_homographies");
    return FUSG_OK;
}
extern "C" int fusg_plane_homographies(const int32_t* src_pts, const int32_t* dst_pts, const int32_t* nverts, const uint8_t* src_vis,
                                       const uint8_t* dst_vis, int32_t V, int32_t P, int32_t sym_a, int32_t sym_b, double* minv,
                                       int32_t* index, double* H, int32_t* status, void* stream) {
    return fusg::plan_dispatch(plane_homographies_impl, stream, src_pts, dst_pts, nverts, src_vis, dst_vis, V, P, sym_a, sym_b, minv, index,
                               H, status);
}

// ---- host twins: the same header's code on the CPU (no GPU needed)
extern "C" int fusg_plane_homographies_host(const int32_t* src_pts, const int32_t* dst_pts, const int32_t* nverts, const uint8_t* src_vis,
                                            const uint8_t* dst_vis, int32_t V, int32_t P, int32_t sym_a, int32_t sym_b, double* minv,
                                            int32_t* index, double* H, int32_t* status) {
    const PlaneHomK k{src_pts, dst_pts, nverts, src_vis, dst_vis, minv, index, H, status, V, P, sym_a, sym_b};
    const int rc = plane_hom_check(k, "plane_homographies_host");
    if (rc != FUSG_OK || V == 0) return rc;
    double ws[hg::WS_DOUBLES], Hs[HG_LANES * 9], inv[hg::MAXP * 9];
    int target[hg::MAXP];
    uint8_t job_ok[hg::MAXP];
    for (int v = 0; v < V; ++v) {
        for (int i = 0; i < P; ++i) {
            target[i] = hg::gate(i, src_vis + (long)v * P, dst_vis + (long)v * P, sym_a, sym_b);
            job_ok[i] = 0;
            if (target[i] < 0) continue;
            const bool ok12 = fit_plane(k, v, i, target[i], 0, Hs + i * 18, ws, 1);
            const bool oki = hg::inverse3(Hs + i * 18, inv + i * 9, hg::view(ws, 1, 32));
            const bool ok21 = fit_plane(k, v, i, target[i], 1, Hs + i * 18 + 9, ws, 1);
            job_ok[i] = ok12 && oki && ok21;
        }
        for (int j = 0; j < P; ++j) write_slot(k, v, j, Hs, inv, target, job_ok);
    }
    return FUSG_OK;
}

extern "C" int fusg_find_homography_host(const double* src_xy, const double* dst_xy, int32_t n, double* H_out, double* minv_out) {
    double ws[hg::WS_DOUBLES], H[9], m[9];
    if (!src_xy || !dst_xy || !H_out) return 0;
    bool ok = hg::find_homography(src_xy, dst_xy, n, H, ws, 1);
    ok = hg::inverse3(H, m, hg::view(ws, 1, 32)) && ok;
    for (int a = 0; a < 9; ++a) {
        H_out[a] = H[a];
        if (minv_out) minv_out[a] = m[a];
    }
    return ok ? 1 : 0;
}
