// Geometry mode's glue between the pose fit and the render, on the device: fusg_pose_geometry (include/fusg.h) selects and
// flips the fitted pose of every vehicle and derives what the render, the plane visibility, the plane cut-outs and the plane
// homographies read - extrinsic, render job, visibility polygons with their "nearer" masks, texture-plane corner points
// (pose_geometry.h: the same code the host twin below runs).
//
// One thread per vehicle: a vehicle is 12 keypoints and 12 small polygons, a few thousand dependent double operations and
// about 1.3 KB of results, and a frame holds at most a few hundred vehicles - the stage is one short latency-bound launch in
// front of the render, not a throughput kernel.  Every result is written with ordinary per-lane stores.
#include "common.h"
#include "pose_geometry.h"

namespace fusg {

constexpr int PG_BLOCK = 64;

__global__ __launch_bounds__(PG_BLOCK) void pose_geometry_kernel(const pg::Args a) {
    const int v = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (v < a.V) pg::vehicle(a, v);
}

}  // namespace fusg

using namespace fusg;

static int pose_geometry_check(const pg::Args& a, const char* what) {
    FUSG_CHECK(a.V >= 0 && a.V < (1 << 20), "%s: V %d (0 .. 2^20 - 1)", what, a.V);
    FUSG_CHECK(a.H >= 1 && a.W >= 1 && a.n_cad >= 1, "%s: H %d, W %d, n_cad %d must be positive", what, a.H, a.W, a.n_cad);
    const bool first = a.rvec && a.tvec && a.err && a.kp_xy && !a.pose_in && !a.steps;
    const bool later = !a.rvec && !a.tvec && !a.err && !a.kp_xy && a.pose_in && a.steps;
    FUSG_CHECK(first || later, "%s: pass either the raw fit (rvec, tvec, err) with kp_xy - a first frame - or pose_in with steps - a "
               "later frame -, the other four NULL", what);
    FUSG_CHECK(a.cad_idx && a.bank_kp3d && a.bank_v_off && a.bank_t_off, "%s: cad_idx or a bank table is null", what);
    FUSG_CHECK(a.pose && a.extrinsic && a.kp3d && a.jobs && a.vis_pts && a.vis_nv && a.nearer && a.tex_pts && a.tex_nv && a.status,
               "%s: an output pointer is null", what);
    return FUSG_OK;
}

static pg::Args pose_geometry_args(const float* rvec, const float* tvec, const float* err, const float* pose_in, const float* kp_xy,
                                   const double* steps, const int64_t* cad_idx, const float* bank_kp3d, const int32_t* bank_v_off,
                                   const int32_t* bank_t_off, int32_t n_cad, const double* K, int32_t H, int32_t W, int32_t V, float* pose,
                                   double* extrinsic, double* kp3d, fusg_render_job* jobs, int32_t* vis_pts, int32_t* vis_nv,
                                   int32_t* nearer, int32_t* tex_pts, int32_t* tex_nv, int32_t* status) {
    pg::Args a{rvec, tvec, err, pose_in, kp_xy, steps, cad_idx, bank_kp3d, bank_v_off, bank_t_off, n_cad, {0}, H, W, V, pose, extrinsic,
               kp3d, jobs, vis_pts, vis_nv, nearer, tex_pts, tex_nv, status};
    for (int i = 0; i < 9; ++i) a.K[i] = K ? K[i] : 0.0;
    return a;
}

// (K travels by value: the nine intrinsics are HOST numbers on both entry points)
static int pose_geometry_impl(pg::Args a, void* stream) {
    hipLaunchKernelGGL(pose_geometry_kernel, dim3((unsigned)((a.V + PG_BLOCK - 1) / PG_BLOCK)), dim3(PG_BLOCK), 0, (hipStream_t)stream, a);
    FUSG_LAUNCH_CHECK("pose_geometry");
    return FUSG_OK;
}

extern "C" int fusg_pose_geometry(const float* rvec, const float* tvec, const float* err, const float* pose_in, const float* kp_xy,
                                  const double* steps, const int64_t* cad_idx, const float* bank_kp3d, const int32_t* bank_v_off,
                                  const int32_t* bank_t_off, int32_t n_cad, const double* K, int32_t H, int32_t W, int32_t V, float* pose,
                                  double* extrinsic, double* kp3d, fusg_render_job* jobs, int32_t* vis_pts, int32_t* vis_nv,
                                  int32_t* nearer, int32_t* tex_pts, int32_t* tex_nv, int32_t* status, void* stream) {
    FUSG_CHECK(K, "pose_geometry: K is null");
    const pg::Args a = pose_geometry_args(rvec, tvec, err, pose_in, kp_xy, steps, cad_idx, bank_kp3d, bank_v_off, bank_t_off, n_cad, K, H, W,
                                          V, pose, extrinsic, kp3d, jobs, vis_pts, vis_nv, nearer, tex_pts, tex_nv, status);
    if (V == 0) return FUSG_OK;
    const int rc = pose_geometry_check(a, "pose_geometry");
    if (rc != FUSG_OK) return rc;
    return fusg::plan_dispatch(pose_geometry_impl, stream, a);
}

// ---- host twin: the same header's code on the CPU (no GPU needed)
extern "C" int fusg_pose_geometry_host(const float* rvec, const float* tvec, const float* err, const float* pose_in, const float* kp_xy,
                                       const double* steps, const int64_t* cad_idx, const float* bank_kp3d, const int32_t* bank_v_off,
                                       const int32_t* bank_t_off, int32_t n_cad, const double* K, int32_t H, int32_t W, int32_t V,
                                       float* pose, double* extrinsic, double* kp3d, fusg_render_job* jobs, int32_t* vis_pts,
                                       int32_t* vis_nv, int32_t* nearer, int32_t* tex_pts, int32_t* tex_nv, int32_t* status) {
    FUSG_CHECK(K, "pose_geometry_host: K is null");
    const pg::Args a = pose_geometry_args(rvec, tvec, err, pose_in, kp_xy, steps, cad_idx, bank_kp3d, bank_v_off, bank_t_off, n_cad, K, H, W,
                                          V, pose, extrinsic, kp3d, jobs, vis_pts, vis_nv, nearer, tex_pts, tex_nv, status);
    if (V == 0) return FUSG_OK;
    const int rc = pose_geometry_check(a, "pose_geometry_host");
    if (rc != FUSG_OK) return rc;
    for (int v = 0; v < V; ++v) pg::vehicle(a, v);
    return FUSG_OK;
}
