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

// fusg_pose_geometry_clips: one thread per row of several clips; the per-clip tables are kernel arguments, the cameras device memory.
__global__ __launch_bounds__(PG_BLOCK) void pose_geometry_clips_kernel(const pg::ClipsArgs t) {
    const int j = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (j < t.J) pg::clips_row(t, j);
}

// fusg_later_gate: one thread per (row, slot), GATE_SLOTS = 8 slots per row - a block of 64 lanes holds 8 whole rows, so a
// row's visibilities, its valid word and its box row are written by neighbouring lanes with ordinary stores.
__global__ __launch_bounds__(PG_BLOCK) void later_gate_kernel(const int32_t* counts, const int32_t* covered, int J, int P,
                                                              uint8_t* dst_vis, int32_t* valid, int32_t* box_rows) {
    const int t = blockIdx.x * PG_BLOCK + threadIdx.x;
    const int j = t / pg::GATE_SLOTS;
    if (j < J) pg::later_gate_slot(counts, covered, P, j, t % pg::GATE_SLOTS, dst_vis, valid, box_rows);
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

// ---- the later-frame branch for rows of several clips.  The five tables are HOST arrays, read and checked here, before anything is
// launched; `what` names the entry point in the messages.  Returns FUSG_OK with t filled; t.J == 0: nothing to do.
static int pose_geometry_clips_args(pg::ClipsArgs& t, const char* what, const float* const* poses, const int64_t* const* cad_idxs,
                                    const int32_t* const* src_pts, const int32_t* vehicles, const int32_t* row_first, int32_t n_clips,
                                    const double* steps, const double* cams, const float* bank_kp3d, const int32_t* bank_v_off,
                                    const int32_t* bank_t_off, int32_t n_cad, int32_t H, int32_t W, int32_t J, float* pose,
                                    double* extrinsic, double* kp3d, fusg_render_job* jobs, int32_t* vis_pts, int32_t* vis_nv,
                                    int32_t* nearer, int32_t* tex_pts, int32_t* tex_nv, int32_t* status, int32_t* src_pts_rows) {
    FUSG_CHECK(n_clips >= 1 && n_clips <= FUSG_MAX_FRAMES, "%s: n_clips = %d (1..%d)", what, n_clips, FUSG_MAX_FRAMES);
    FUSG_CHECK(J >= 0 && J < (1 << 20), "%s: J %d (0 .. 2^20 - 1)", what, J);
    FUSG_CHECK(poses && cad_idxs && src_pts && vehicles && row_first, "%s: a host table is null (poses, cad_idxs, src_pts, vehicles, row_first)",
               what);
    memset(&t, 0, sizeof(t));
    FUSG_CHECK(row_first[0] == 0, "%s: the row offsets start at %d, not at 0", what, row_first[0]);
    for (int c = 0; c < n_clips; ++c) {
        const int V = vehicles[c];
        const long cnt = (long)row_first[c + 1] - row_first[c];
        FUSG_CHECK(V >= 0, "%s: clip %d has %d vehicles", what, c, V);
        FUSG_CHECK(cnt >= 0, "%s: the row offsets decrease at clip %d (%d after %d)", what, c, row_first[c + 1], row_first[c]);
        FUSG_CHECK(V == 0 ? cnt == 0 : cnt % V == 0, "%s: clip %d owns %ld rows, not a multiple of its %d vehicles", what, c, cnt, V);
        FUSG_CHECK(cnt == 0 || (poses[c] && cad_idxs[c] && src_pts[c]), "%s: clip %d owns %ld rows and has a null table (pose, cad_idx, src_pts)",
                   what, c, cnt);
        t.pose[c] = poses[c];
        t.cad_idx[c] = cad_idxs[c];
        t.src_pts[c] = src_pts[c];
        t.vehicles[c] = V;
        t.row_first[c] = row_first[c];
    }
    for (int c = n_clips; c <= FUSG_MAX_FRAMES; ++c) t.row_first[c] = row_first[n_clips];
    FUSG_CHECK(row_first[n_clips] == J, "%s: the row offsets end at %d, J is %d", what, row_first[n_clips], J);
    t.n_clips = n_clips;
    t.J = J;
    if (J == 0) return FUSG_OK;
    FUSG_CHECK(H >= 1 && W >= 1 && n_cad >= 1, "%s: H %d, W %d, n_cad %d must be positive", what, H, W, n_cad);
    FUSG_CHECK(steps && cams && bank_kp3d && bank_v_off && bank_t_off, "%s: steps, cams or a bank table is null", what);
    FUSG_CHECK(pose && extrinsic && kp3d && jobs && vis_pts && vis_nv && nearer && tex_pts && tex_nv && status && src_pts_rows,
               "%s: an output pointer is null", what);
    t.steps = steps; t.cams = cams;
    t.bank_kp3d = bank_kp3d; t.bank_v_off = bank_v_off; t.bank_t_off = bank_t_off; t.n_cad = n_cad;
    t.H = H; t.W = W;
    t.pose_out = pose; t.extrinsic = extrinsic; t.kp3d = kp3d; t.jobs = jobs;
    t.vis_pts = vis_pts; t.vis_nv = vis_nv; t.nearer = nearer; t.tex_pts = tex_pts; t.tex_nv = tex_nv; t.status = status;
    t.src_pts_rows = src_pts_rows;
    return FUSG_OK;
}

static int pose_geometry_clips_impl(pg::ClipsArgs t, void* stream) {
    hipLaunchKernelGGL(pose_geometry_clips_kernel, dim3((unsigned)((t.J + PG_BLOCK - 1) / PG_BLOCK)), dim3(PG_BLOCK), 0, (hipStream_t)stream, t);
    FUSG_LAUNCH_CHECK("pose_geometry_clips");
    return FUSG_OK;
}

extern "C" int fusg_pose_geometry_clips(const float* const* poses, const int64_t* const* cad_idxs, const int32_t* const* src_pts,
                                        const int32_t* vehicles, const int32_t* row_first, int32_t n_clips, const double* steps,
                                        const double* cams, const float* bank_kp3d, const int32_t* bank_v_off, const int32_t* bank_t_off,
                                        int32_t n_cad, int32_t H, int32_t W, int32_t J, float* pose, double* extrinsic, double* kp3d,
                                        fusg_render_job* jobs, int32_t* vis_pts, int32_t* vis_nv, int32_t* nearer, int32_t* tex_pts,
                                        int32_t* tex_nv, int32_t* status, int32_t* src_pts_rows, void* stream) {
    pg::ClipsArgs t;
    const int rc = pose_geometry_clips_args(t, "pose_geometry_clips", poses, cad_idxs, src_pts, vehicles, row_first, n_clips, steps, cams,
                                            bank_kp3d, bank_v_off, bank_t_off, n_cad, H, W, J, pose, extrinsic, kp3d, jobs, vis_pts, vis_nv,
                                            nearer, tex_pts, tex_nv, status, src_pts_rows);
    if (rc != FUSG_OK || J == 0) return rc;
    return fusg::plan_dispatch(pose_geometry_clips_impl, stream, t);
}

// ---- host twin: every pointer, the tables' entries included, is a HOST pointer (no GPU needed)
extern "C" int fusg_pose_geometry_clips_host(const float* const* poses, const int64_t* const* cad_idxs, const int32_t* const* src_pts,
                                             const int32_t* vehicles, const int32_t* row_first, int32_t n_clips, const double* steps,
                                             const double* cams, const float* bank_kp3d, const int32_t* bank_v_off,
                                             const int32_t* bank_t_off, int32_t n_cad, int32_t H, int32_t W, int32_t J, float* pose,
                                             double* extrinsic, double* kp3d, fusg_render_job* jobs, int32_t* vis_pts, int32_t* vis_nv,
                                             int32_t* nearer, int32_t* tex_pts, int32_t* tex_nv, int32_t* status, int32_t* src_pts_rows) {
    pg::ClipsArgs t;
    const int rc = pose_geometry_clips_args(t, "pose_geometry_clips_host", poses, cad_idxs, src_pts, vehicles, row_first, n_clips, steps, cams,
                                            bank_kp3d, bank_v_off, bank_t_off, n_cad, H, W, J, pose, extrinsic, kp3d, jobs, vis_pts, vis_nv,
                                            nearer, tex_pts, tex_nv, status, src_pts_rows);
    if (rc != FUSG_OK) return rc;
    for (int j = 0; j < J; ++j) pg::clips_row(t, j);
    return FUSG_OK;
}

// ---- the later-frame gate: plane counts + covered counts -> gated visibilities, valid words, gated box rows
static int later_gate_check(const int32_t* counts, const int32_t* covered, int32_t J, int32_t P, const uint8_t* dst_vis,
                            const int32_t* valid, const char* what) {
    FUSG_CHECK(J >= 0 && J < (1 << 20), "%s: J %d (0 .. 2^20 - 1)", what, J);
    FUSG_CHECK(P >= 1 && P <= pg::NVIS, "%s: P %d (1 .. %d planes)", what, P, pg::NVIS);
    FUSG_CHECK(counts && covered && dst_vis && valid, "%s: counts, covered, dst_vis or valid is null", what);
    return FUSG_OK;
}

static int later_gate_impl(const int32_t* counts, const int32_t* covered, int32_t J, int32_t P, uint8_t* dst_vis, int32_t* valid,
                           int32_t* box_rows, void* stream) {
    const unsigned blocks = (unsigned)(((long)J * pg::GATE_SLOTS + PG_BLOCK - 1) / PG_BLOCK);
    hipLaunchKernelGGL(later_gate_kernel, dim3(blocks), dim3(PG_BLOCK), 0, (hipStream_t)stream, counts, covered, J, P, dst_vis, valid,
                       box_rows);
    FUSG_LAUNCH_CHECK("later_gate");
    return FUSG_OK;
}

extern "C" int fusg_later_gate(const int32_t* counts, const int32_t* covered, int32_t J, int32_t P, uint8_t* dst_vis, int32_t* valid,
                               int32_t* box_rows, void* stream) {
    const int rc = later_gate_check(counts, covered, J, P, dst_vis, valid, "later_gate");
    if (rc != FUSG_OK) return rc;
    if (J == 0) return FUSG_OK;
    return fusg::plan_dispatch(later_gate_impl, stream, counts, covered, J, P, dst_vis, valid, box_rows);
}

extern "C" int fusg_later_gate_host(const int32_t* counts, const int32_t* covered, int32_t J, int32_t P, uint8_t* dst_vis,
                                    int32_t* valid, int32_t* box_rows) {
    const int rc = later_gate_check(counts, covered, J, P, dst_vis, valid, "later_gate_host");
    if (rc != FUSG_OK) return rc;
    for (long j = 0; j < J; ++j) pg::later_gate_row(counts, covered, P, j, dst_vis, valid, box_rows);
    return FUSG_OK;
}
