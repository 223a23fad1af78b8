// The glue of geometry mode between the pose fit and the render, written once for host and device: per vehicle the
// select-and-flip epilogue of the fit (utils/pnp_utils.py select_and_flip), the extrinsic (render.rotations /
// extrinsics_from_poses), a later frame's moved and projected keypoints (render.vehicle_geometry, project_keypoints_batch),
// the texture-plane corner points (plane_corners_batch), the visibility polygons with their "nearer" masks
// (visibility_inputs_batch) and the fusg_render_job record (render_jobs) - the same IEEE operations in the order the numpy
// code takes them, float64 where numpy is float64 and float32 where it is float32 (the extrinsic of a float32 pose, the
// camera centre and, on a first frame, the plane means and distances).  Compiled with -ffp-contract=off.  Besides +, -, *,
// / and sqrt it calls cos, sin and acos, whose last bit may differ between libm, numpy and the device's math library: the
// float results agree to a few ulp, the truncated integers wherever the value is not within that of an integer.
//
// The camera centre is inv(E)[:3, 3].  E = [R(rvec) | t] with R from Rodrigues' formula is rigid by construction, so the
// centre is taken in closed form, -R^T t, in E's float32: it differs from LAPACK's float32 LU inverse by a few float32 ulp
// (neither is the exact centre), which only matters for two planes whose camera distances agree to that precision.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_FN __host__ __device__ static inline
#else
#define PG_FN static inline
#endif

#include "../../include/fusg.h"

namespace fusg {
namespace pg {

constexpr int NKP = 12, NVIS = 7, NTEX = 5, MAXP = 8;
constexpr int STATUS_BAD_CAD = 1;                   // cad_idx outside the bank: empty job, zero keypoints
constexpr double EPS = 2.220446049250313e-16;
constexpr double CLIP_PX = 1048576.0;

// plane -> keypoints (render.KP_NAMES order): the five texture planes (planes_utils.CAR_TEXTURE_PLANES), then front_bt, back_bt
struct PlaneTable { int n[NVIS]; int idx[NVIS][6]; };
PG_FN PlaneTable planes() {
    return PlaneTable{{6, 6, 4, 4, 4, 4, 4},
                      {{0, 1, 3, 2, 9, 8}, {4, 5, 7, 6, 11, 10}, {8, 9, 11, 10, 0, 0}, {2, 6, 11, 9, 0, 0}, {0, 4, 10, 8, 0, 0},
                       {2, 6, 7, 3, 0, 0}, {0, 4, 5, 1, 0, 0}}};
}

struct Args {
    // first frame: the raw fit rvec / tvec [V, 4, 3], err [V, 4] and kp_xy [V, 12, 2]; later frame: pose_in [V, 7] and steps [V, 4]
    const float* rvec; const float* tvec; const float* err; const float* pose_in; const float* kp_xy; const double* steps;
    const int64_t* cad_idx;
    const float* bank_kp3d; const int32_t* bank_v_off; const int32_t* bank_t_off; int n_cad;
    double K[9];
    int H, W, V;
    float* pose; double* extrinsic; double* kp3d; fusg_render_job* jobs;
    int32_t* vis_pts; int32_t* vis_nv; int32_t* nearer; int32_t* tex_pts; int32_t* tex_nv; int32_t* status;
};

PG_FN bool is_nan(double x) { return x != x; }
PG_FN int32_t trunc_i32(double x) {                 // numpy's float64 -> int32 cast: NaN and out of range give INT32_MIN
    return (x > -2147483649.0 && x < 2147483648.0) ? (int32_t)x : INT32_MIN;
}

// utils/pnp_utils.py rodrigues / render.rotations: rotation vector -> matrix, float64
PG_FN void rodrigues(const double r[3], double R[9]) {
    const double th = __builtin_sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    if (th < EPS) {
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double u[3] = {r[0] / th, r[1] / th, r[2] / th};
    const double c = cos(th), s = sin(th);
    const double skew[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            R[i * 3 + j] = (c * (i == j ? 1.0 : 0.0) + (1.0 - c) * (u[i] * u[j])) + s * skew[i * 3 + j];
}

// utils/pnp_utils.py rodrigues_inv: rotation matrix -> vector with cv2.Rodrigues' published branches, float64
PG_FN void rodrigues_inv(const double R[9], double out[3]) {
    const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double s = __builtin_sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1.0) * 0.5;
    if (-1.0 > c) c = -1.0;                         // Python's max(c, -1.0) and min(., 1.0): a NaN stays
    if (1.0 < c) c = 1.0;
    const double th = acos(c);
    if (s < 1e-5) {
        if (c > 0) {
            out[0] = out[1] = out[2] = 0.0;
            return;
        }
        double x = (R[0] + 1.0) * 0.5, y = (R[4] + 1.0) * 0.5, z = (R[8] + 1.0) * 0.5;
        x = __builtin_sqrt(0.0 > x ? 0.0 : x);
        y = __builtin_sqrt(0.0 > y ? 0.0 : y) * (R[1] < 0 ? -1.0 : 1.0);
        z = __builtin_sqrt(0.0 > z ? 0.0 : z) * (R[2] < 0 ? -1.0 : 1.0);
        const double ax = __builtin_fabs(x), ay = __builtin_fabs(y), az = __builtin_fabs(z);
        if (ax < ay && ax < az && ((R[5] > 0) != (y * z > 0))) z = -z;
        const double k = th / __builtin_sqrt((x * x + y * y) + z * z);
        out[0] = x * k; out[1] = y * k; out[2] = z * k;
        return;
    }
    const double k = th / (2.0 * s);
    out[0] = v[0] * k; out[1] = v[1] * k; out[2] = v[2] * k;
}

// select_and_flip: np.argmin over the four starts (first index on ties; the first NaN wins), sign flip through Rodrigues
PG_FN void select_and_flip(const float* rvec, const float* tvec, const float* err, float pose[7]) {
    int b = 0;
    for (int k = 1; k < 4; ++k)
        if (!is_nan(err[b]) && (is_nan(err[k]) || err[k] < err[b])) b = k;
    const float* r = rvec + b * 3;
    const float* t = tvec + b * 3;
    const float tz = t[2];
    const float sg = tz > 0.f ? 1.f : (tz < 0.f ? -1.f : (tz == 0.f ? 0.f : tz));      // np.sign: 0 -> 0, NaN -> NaN
    const double r64[3] = {(double)r[0], (double)r[1], (double)r[2]};
    double R[9], rf[3];
    rodrigues(r64, R);
    for (int j = 0; j < 6; ++j) R[j] *= (double)sg;
    rodrigues_inv(R, rf);
    pose[0] = err[b];
    for (int j = 0; j < 3; ++j) {
        pose[1 + j] = (float)rf[j];
        pose[4 + j] = t[j] * sg;
    }
}

// visibility_inputs_batch for one vehicle; T = the keypoints' dtype there (float32 on a first frame, float64 on a later one)
template <typename T>
PG_FN void visibility(const T kp[NKP][3], const float E32[12], const double K[9], int32_t* pts, int32_t* nv, int32_t* nearer) {
    const PlaneTable pt = planes();
    float cam[3];                                    // -R^T t in E's float32
    for (int j = 0; j < 3; ++j) cam[j] = -((E32[j] * E32[3] + E32[4 + j] * E32[7]) + E32[8 + j] * E32[11]);
    T dist[NVIS];
    for (int p = 0; p < NVIS; ++p) {
        T d2 = 0;
        T d[3];
        for (int j = 0; j < 3; ++j) {
            T m = kp[pt.idx[p][0]][j];
            for (int a = 1; a < pt.n[p]; ++a) m = m + kp[pt.idx[p][a]][j];
            m = m / (T)pt.n[p];
            d[j] = (T)cam[j] - m;
        }
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        dist[p] = (T)__builtin_sqrt((T)d2);
    }
    double M[12];                                    // K @ E[:3]
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j)
            M[i * 4 + j] = (K[i * 3] * (double)E32[j] + K[i * 3 + 1] * (double)E32[4 + j]) + K[i * 3 + 2] * (double)E32[8 + j];
    int32_t k2[NKP][2];
    for (int i = 0; i < NKP; ++i) {
        double q[3];
        for (int a = 0; a < 3; ++a)
            q[a] = ((M[a * 4] * (double)kp[i][0] + M[a * 4 + 1] * (double)kp[i][1]) + M[a * 4 + 2] * (double)kp[i][2]) + M[a * 4 + 3] * 1.0;
        for (int a = 0; a < 2; ++a) {
            double c = q[a] / q[2];
            c = c < -CLIP_PX ? -CLIP_PX : (c > CLIP_PX ? CLIP_PX : c);      // np.clip: a NaN stays
            k2[i][a] = trunc_i32(c);
        }
    }
    for (int p = 0; p < NVIS; ++p) {
        for (int a = 0; a < MAXP; ++a) {
            const bool in = a < pt.n[p];
            pts[(p * MAXP + a) * 2] = in ? k2[pt.idx[p][a < 6 ? a : 0]][0] : 0;
            pts[(p * MAXP + a) * 2 + 1] = in ? k2[pt.idx[p][a < 6 ? a : 0]][1] : 0;
        }
        nv[p] = pt.n[p];
        int32_t m = 0;
        for (int q_ = 0; q_ < NVIS; ++q_) m |= (dist[q_] < dist[p] ? 1 : 0) << q_;
        nearer[p] = m;
    }
}

// plane_corners_batch for one vehicle: divide by (W, H), multiply back, truncate
PG_FN void texture_corners(const double kp2[NKP][2], int H, int W, int32_t* pts, int32_t* nv) {
    const PlaneTable pt = planes();
    const double wh[2] = {(double)W, (double)H};
    for (int p = 0; p < NTEX; ++p) {
        for (int a = 0; a < MAXP; ++a)
            for (int c = 0; c < 2; ++c) {
                int32_t o = 0;
                if (a < pt.n[p]) o = trunc_i32((kp2[pt.idx[p][a < 6 ? a : 0]][c] / wh[c]) * wh[c]);
                pts[(p * MAXP + a) * 2 + c] = o;
            }
        nv[p] = pt.n[p];
    }
}

// everything of vehicle v.  Its CAD index and, on a later frame, its pose are read at row `src` of cad_idx / pose_in: v itself for
// fusg_pose_geometry, the vehicle's row in its clip's tables for fusg_pose_geometry_clips (clips_row below); steps and every output
// are rows v.
PG_FN void vehicle(const Args& a, int v, long src) {
    const bool later = a.steps != nullptr;
    float pose[7];
    if (later)
        for (int j = 0; j < 7; ++j) pose[j] = a.pose_in[src * 7 + j];
    else
        select_and_flip(a.rvec + (long)v * 12, a.tvec + (long)v * 12, a.err + (long)v * 4, pose);
    for (int j = 0; j < 7; ++j) a.pose[(long)v * 7 + j] = pose[j];

    // the extrinsic of the float32 pose: R in float64, stored in the pose's float32
    const double r64[3] = {(double)pose[1], (double)pose[2], (double)pose[3]};
    double Rm[9];
    rodrigues(r64, Rm);
    float E32[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) E32[i * 4 + j] = (float)Rm[i * 3 + j];
        E32[i * 4 + 3] = pose[4 + i];
    }
    for (int j = 0; j < 12; ++j) a.extrinsic[(long)v * 12 + j] = (double)E32[j];

    // the CAD model: its keypoints and its slices of the bank
    const int64_t m = a.cad_idx[src];
    const bool cad_ok = m >= 0 && m < (int64_t)a.n_cad;
    a.status[v] = cad_ok ? 0 : STATUS_BAD_CAD;
    float kp32[NKP][3];
    for (int i = 0; i < NKP; ++i)
        for (int j = 0; j < 3; ++j) kp32[i][j] = cad_ok ? a.bank_kp3d[((long)m * NKP + i) * 3 + j] : 0.f;

    fusg_render_job job;
    for (int j = 0; j < 9; ++j) job.R[j] = (j % 4 == 0) ? 1.0 : 0.0;
    for (int j = 0; j < 3; ++j) job.tr[j] = 0.0;
    double kp64[NKP][3], kp2[NKP][2];
    if (later) {
        const double th = a.steps[(long)v * 4];
        const double cz = cos(th), sz = sin(th);
        const double Rs[9] = {cz, -sz, 0.0, sz, cz, 0.0, 0.0, 0.0, 1.0};              // render.z_rot
        for (int j = 0; j < 9; ++j) job.R[j] = Rs[j];
        for (int j = 0; j < 3; ++j) job.tr[j] = a.steps[(long)v * 4 + 1 + j];
        for (int i = 0; i < NKP; ++i)                                                  // kp3d @ R_step + tr
            for (int j = 0; j < 3; ++j)
                kp64[i][j] = (((double)kp32[i][0] * Rs[j] + (double)kp32[i][1] * Rs[3 + j]) + (double)kp32[i][2] * Rs[6 + j]) + job.tr[j];
        for (int i = 0; i < NKP; ++i) {                                                // project_keypoints_batch
            double pc[3];
            for (int j = 0; j < 3; ++j)
                pc[j] = ((kp64[i][0] * Rm[j * 3] + kp64[i][1] * Rm[j * 3 + 1]) + kp64[i][2] * Rm[j * 3 + 2]) + (double)pose[4 + j];
            kp2[i][0] = a.K[0] * (pc[0] / pc[2]) + a.K[2];
            kp2[i][1] = a.K[4] * (pc[1] / pc[2]) + a.K[5];
        }
    } else {
        for (int i = 0; i < NKP; ++i) {
            for (int j = 0; j < 3; ++j) kp64[i][j] = (double)kp32[i][j];
            for (int c = 0; c < 2; ++c) kp2[i][c] = (double)a.kp_xy[((long)v * NKP + i) * 2 + c];
        }
    }
    for (int i = 0; i < NKP; ++i)
        for (int j = 0; j < 3; ++j) a.kp3d[((long)v * NKP + i) * 3 + j] = kp64[i][j];

    texture_corners(kp2, a.H, a.W, a.tex_pts + (long)v * NTEX * MAXP * 2, a.tex_nv + (long)v * NTEX);
    int32_t* vp = a.vis_pts + (long)v * NVIS * MAXP * 2;
    if (later)
        visibility<double>(kp64, E32, a.K, vp, a.vis_nv + (long)v * NVIS, a.nearer + (long)v * NVIS);
    else
        visibility<float>(kp32, E32, a.K, vp, a.vis_nv + (long)v * NVIS, a.nearer + (long)v * NVIS);

    for (int j = 0; j < 12; ++j) job.E[j] = (double)E32[j];
    job.fx = a.K[0];
    job.fy = a.K[4];
    job.cx = (double)a.W / 2 - 0.5;                                                    // Open3D's principal point, not K's
    job.cy = (double)a.H / 2 - 0.5;
    job.v_off = cad_ok ? a.bank_v_off[m] : 0;
    job.nv = cad_ok ? a.bank_v_off[m + 1] - a.bank_v_off[m] : 0;
    job.t_off = cad_ok ? a.bank_t_off[m] : 0;
    job.nt = cad_ok ? a.bank_t_off[m + 1] - a.bank_t_off[m] : 0;
    a.jobs[v] = job;
}

PG_FN void vehicle(const Args& a, int v) { vehicle(a, v, (long)v); }

// ---- the later-frame branch for rows of SEVERAL clips (fusg_pose_geometry_clips): clip-major rows, frame-major inside a clip - row
// row_first[c] + f * vehicles[c] + v is clip c, frame f, vehicle v.  The per-clip tables travel by value (three device pointers and
// two ints per clip, 2.3 KB of the 4 KB kernel-argument space); the cameras do not fit beside them and are read from device memory.
struct ClipsArgs {
    const float* pose[FUSG_MAX_FRAMES];              // [V_c][7]
    const int64_t* cad_idx[FUSG_MAX_FRAMES];         // [V_c]
    const int32_t* src_pts[FUSG_MAX_FRAMES];         // [V_c][NTEX][MAXP][2]
    int32_t vehicles[FUSG_MAX_FRAMES];
    int32_t row_first[FUSG_MAX_FRAMES + 1];
    int n_clips;
    const double* steps;                             // [J][4]
    const double* cams;                              // [n_clips][9], row-major K per clip
    const float* bank_kp3d; const int32_t* bank_v_off; const int32_t* bank_t_off; int n_cad;
    int H, W, J;
    float* pose_out; double* extrinsic; double* kp3d; fusg_render_job* jobs;
    int32_t* vis_pts; int32_t* vis_nv; int32_t* nearer; int32_t* tex_pts; int32_t* tex_nv; int32_t* status;
    int32_t* src_pts_rows;                           // [J][NTEX][MAXP][2]
};

// row j: `vehicle` with its clip's pose table, CAD indices and camera, and the row's copy of its source corner points.  The host has
// checked the offsets (0 .. J, non-decreasing, a clip's rows a multiple of its vehicles), so the scan ends and V > 0 here.
PG_FN void clips_row(const ClipsArgs& t, int j) {
    int c = 0;
    while (j >= t.row_first[c + 1]) ++c;
    const int v = (j - t.row_first[c]) % t.vehicles[c];
    Args a{nullptr, nullptr, nullptr, t.pose[c], nullptr, t.steps, t.cad_idx[c], t.bank_kp3d, t.bank_v_off, t.bank_t_off, t.n_cad, {0},
           t.H, t.W, t.J, t.pose_out, t.extrinsic, t.kp3d, t.jobs, t.vis_pts, t.vis_nv, t.nearer, t.tex_pts, t.tex_nv, t.status};
    for (int i = 0; i < 9; ++i) a.K[i] = t.cams[(long)c * 9 + i];
    vehicle(a, j, (long)v);
    constexpr int NPTS = NTEX * MAXP * 2;
    const int32_t* sp = t.src_pts[c] + (long)v * NPTS;
    for (int i = 0; i < NPTS; ++i) t.src_pts_rows[(long)j * NPTS + i] = sp[i];
}

// ---- the tail of a later frame's geometry stage (fusg_later_gate): what the frame driver decided on the host after reading the
// plane counts and covered-pixel counts back.  A row is one (frame, vehicle); it has GATE_SLOTS = 8 slots of independent work, the
// width of a paste box row, of which the first P <= 7 also own a plane.  The comparison is render.visible's float64 expression
// (online_visibility.py:145-148) as it stands, one multiply and one compare - not an integer restatement: parity is with what the
// per-frame path computes from the read-back counts.
constexpr int GATE_SLOTS = 8;

PG_FN void later_gate_slot(const int32_t* counts, const int32_t* covered, int P, long j, int s, uint8_t* dst_vis, int32_t* valid,
                           int32_t* box_rows) {
    const bool ok = covered[j] > 0;                                                    // an empty render: the reference's `except: break`
    if (s < P) {
        const int32_t* c = counts + (j * NVIS + s) * 2;                                // (absolute, occluded)
        dst_vis[j * P + s] = (ok && (double)c[1] > 0.9 * (double)c[0]) ? 1 : 0;
    }
    if (s == 0) valid[j] = ok ? 1 : 0;
    if (box_rows && !ok) box_rows[j * GATE_SLOTS + s] = 0;
}

PG_FN void later_gate_row(const int32_t* counts, const int32_t* covered, int P, long j, uint8_t* dst_vis, int32_t* valid,
                          int32_t* box_rows) {
    for (int s = 0; s < GATE_SLOTS; ++s) later_gate_slot(counts, covered, P, j, s, dst_vis, valid, box_rows);
}

}  // namespace pg
}  // namespace fusg
