// Device versions of the reference's per-vehicle geometry: the Open3D render of the posed CAD model into a
// normal-colour sketch and its mask (warp_learn/render_open3d.py:29-49) and the plane areas of compute_visibility
// (warp_learn/online_visibility.py:105-150).  The reference opens one GL window per vehicle and frame for the first and
// fills ~50 full-frame polygons with OpenCV for the second.  Both are integer / float64 work without matrix cores.
//
// Rasteriser (fusg_render_normals_u8), three launches per call:
//   project_kernel  one workgroup per job: every vertex of the job's mesh moved (p = v @ R + tr), put in the camera
//                   (E p), projected with fx, fy, cx, cy in float64 (no FP contraction: -ffp-contract=off in the Makefile,
//                   so the values equal numpy's), snapped to 1/256 px; vertex colour (n @ R + 1) / 2; the job's screen box
//                   (block reduction, no atomics).
//   raster_kernel   one workgroup per (16 x 16 screen tile, job).  A tile outside the job's box writes zeros.  Otherwise
//                   the mesh's triangles stream through LDS in chunks of 256: each lane sets up one triangle and tests its
//                   box against the tile; the survivors are compacted in triangle order (wave ballots + a 4-entry scan).
//                   Each lane (= pixel) then keeps the nearest fragment: largest interpolated 1/z, strict '>' in triangle
//                   order, so a depth tie goes to the lower triangle index (GL_LESS, first drawn).  Resolve in the same
//                   kernel: the winner's perspective-correct barycentrics interpolate the vertex colours.
//   No global atomics in the image, no binning pass: the bytes do not depend on scheduling.  The covered-pixel count per
//   job is one integer atomic per workgroup (integer sums are order-independent).
// Coverage: int64 edge functions on the snapped coordinates, pixel centres at integer (x, y) (x right, y down), top-left
// fill rule, both windings (no back-face culling).  A triangle with a vertex at Zc <= 1e-3 is dropped (no near-plane
// clipping - a divergence from GL), as is a zero-area one or one that names a vertex outside its mesh.
#include <math.h>
#include <algorithm>
#include "common.h"
#include "polygon.h"

namespace fusg {

constexpr int TILE = 16;
constexpr double NEAR_Z = 1e-3;
constexpr double MAX_PX = 2097152.0;     // |x|, |y| clamped to 2^21 px: snapped coordinates stay within 2^29, edge terms in int64

struct PV { int X, Y; double iz; double c[3]; };     // projected vertex: 1/256-px coordinates, 1/Zc (<= 0: invalid), colour
static_assert(sizeof(PV) == 40, "PV layout");
static_assert(sizeof(fusg_render_job) == 240, "fusg_render_job layout");

__global__ __launch_bounds__(256) void project_kernel(const double* __restrict__ verts, const double* __restrict__ normals,
                                                      long n_verts, const fusg_render_job* __restrict__ jobs, int max_nv,
                                                      int4* __restrict__ boxes, PV* __restrict__ pv) {
    const int j = blockIdx.x, tid = threadIdx.x;
    const fusg_render_job& jb = jobs[j];
    const bool ok = jb.nv >= 0 && jb.nv <= max_nv && jb.v_off >= 0 && (long)jb.v_off + jb.nv <= n_verts;
    const int nv = ok ? jb.nv : 0;
    PV* out = pv + (long)j * max_nv;
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -0x7fffffff, y1 = -0x7fffffff;
    for (int v = tid; v < nv; v += 256) {
        const double* a = verts + ((long)jb.v_off + v) * 3;
        const double* n = normals + ((long)jb.v_off + v) * 3;
        double p[3], c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {    // row vector times z_rot(theta), left to right (trajectory_inference.py:363)
            p[k] = a[0] * jb.R[k] + a[1] * jb.R[3 + k] + a[2] * jb.R[6 + k] + jb.tr[k];
            c[k] = (n[0] * jb.R[k] + n[1] * jb.R[3 + k] + n[2] * jb.R[6 + k] + 1.0) / 2.0;
        }
        const double Xc = jb.E[0] * p[0] + jb.E[1] * p[1] + jb.E[2] * p[2] + jb.E[3];
        const double Yc = jb.E[4] * p[0] + jb.E[5] * p[1] + jb.E[6] * p[2] + jb.E[7];
        const double Zc = jb.E[8] * p[0] + jb.E[9] * p[1] + jb.E[10] * p[2] + jb.E[11];
        PV r;
        if (Zc > NEAR_Z) {
            const double x = fmin(fmax(jb.fx * (Xc / Zc) + jb.cx, -MAX_PX), MAX_PX);
            const double y = fmin(fmax(jb.fy * (Yc / Zc) + jb.cy, -MAX_PX), MAX_PX);
            r.X = (int)rint(x * 256.0);
            r.Y = (int)rint(y * 256.0);
            r.iz = 1.0 / Zc;
            x0 = min(x0, r.X); x1 = max(x1, r.X); y0 = min(y0, r.Y); y1 = max(y1, r.Y);
        } else {
            r.X = r.Y = 0;
            r.iz = -1.0;
        }
        r.c[0] = c[0]; r.c[1] = c[1]; r.c[2] = c[2];
        out[v] = r;
    }
    __shared__ int red[4][4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o)); y0 = min(y0, __shfl_xor(y0, o));
        x1 = max(x1, __shfl_xor(x1, o)); y1 = max(y1, __shfl_xor(y1, o));
    }
    if ((tid & 63) == 0) { red[tid >> 6][0] = x0; red[tid >> 6][1] = y0; red[tid >> 6][2] = x1; red[tid >> 6][3] = y1; }
    __syncthreads();
    if (tid == 0) {
        int4 b = make_int4(red[0][0], red[0][1], red[0][2], red[0][3]);
        for (int w = 1; w < 4; ++w) {
            b.x = min(b.x, red[w][0]); b.y = min(b.y, red[w][1]); b.z = max(b.z, red[w][2]); b.w = max(b.w, red[w][3]);
        }
        boxes[j] = b;                    // 1/256-px units; empty (x0 > x1) when no vertex lies in front of the camera
    }
}

// One triangle ready for the edge functions: vertices reordered to positive area (the winding only decides the order, no
// culling).  e_i is the edge function of the edge opposite vertex i; sum e_i = area.
struct Tri { long X[3], Y[3]; double iz[3]; long area; int vi[3]; };

__device__ __forceinline__ bool tri_setup(const int* __restrict__ tris, int t_glob, int nv, const PV* __restrict__ pv, Tri& T) {
    int i0 = tris[(long)t_glob * 3], i1 = tris[(long)t_glob * 3 + 1], i2 = tris[(long)t_glob * 3 + 2];
    if ((unsigned)i0 >= (unsigned)nv || (unsigned)i1 >= (unsigned)nv || (unsigned)i2 >= (unsigned)nv) return false;
    PV a = pv[i0], b = pv[i1], c = pv[i2];
    if (!(a.iz > 0.0) || !(b.iz > 0.0) || !(c.iz > 0.0)) return false;
    long area = ((long)b.X - a.X) * ((long)c.Y - a.Y) - ((long)b.Y - a.Y) * ((long)c.X - a.X);
    if (area == 0) return false;
    if (area < 0) { PV s = b; b = c; c = s; int si = i1; i1 = i2; i2 = si; area = -area; }
    T.X[0] = a.X; T.X[1] = b.X; T.X[2] = c.X;
    T.Y[0] = a.Y; T.Y[1] = b.Y; T.Y[2] = c.Y;
    T.iz[0] = a.iz; T.iz[1] = b.iz; T.iz[2] = c.iz;
    T.vi[0] = i0; T.vi[1] = i1; T.vi[2] = i2;
    T.area = area;
    return true;
}

// edge i runs from vertex i+1 to vertex i+2.  With positive area in y-down coordinates a 'top' edge is horizontal with
// dx > 0 and a 'left' edge has dy < 0; a sample exactly on an edge belongs to the triangle only for those edges.
__device__ __forceinline__ bool tri_edges(const long* X, const long* Y, long px, long py, long e[3]) {
    bool in = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int a = i == 2 ? 0 : i + 1, b = i == 0 ? 2 : i - 1;
        const long dx = X[b] - X[a], dy = Y[b] - Y[a];
        e[i] = dx * (py - Y[a]) - dy * (px - X[a]);
        const bool tl = dy < 0 || (dy == 0 && dx > 0);
        in = in && (e[i] > 0 || (e[i] == 0 && tl));
    }
    return in;
}

struct SurvLds { long X[3], Y[3]; double iz[3]; double area; int tri; int _pad; };

__global__ __launch_bounds__(256) void raster_kernel(const int* __restrict__ tris, long n_tris, const fusg_render_job* __restrict__ jobs,
                                                     int max_nv, const int4* __restrict__ boxes, const PV* __restrict__ pv_all,
                                                     int H, int W, unsigned char* __restrict__ sketch, unsigned char* __restrict__ mask,
                                                     int* __restrict__ tri_id, int* __restrict__ covered) {
    __shared__ SurvLds surv[256];
    __shared__ int wcount[4];
    const int j = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * TILE, ty0 = blockIdx.y * TILE;
    const int px = tx0 + (tid & (TILE - 1)), py = ty0 + tid / TILE;
    const bool inside_frame = px < W && py < H;
    const fusg_render_job& jb = jobs[j];
    const bool ok = jb.nv >= 0 && jb.nv <= max_nv && jb.nt >= 0 && jb.t_off >= 0 && (long)jb.t_off + jb.nt <= n_tris;
    const int4 bx = boxes[j];
    // the tile in 1/256-px units, against the job's screen box (conservative: every vertex in front of the camera)
    const long tX0 = (long)tx0 * 256, tX1 = (long)(tx0 + TILE - 1) * 256, tY0 = (long)ty0 * 256, tY1 = (long)(ty0 + TILE - 1) * 256;
    const bool live = ok && bx.x <= bx.z && bx.z >= tX0 && bx.x <= tX1 && bx.w >= tY0 && bx.y <= tY1;
    const PV* pv = pv_all + (long)j * max_nv;
    double best = -1.0;
    int best_t = -1;
    if (live) {
        const long sx = (long)px * 256, sy = (long)py * 256;
        for (int base = 0; base < jb.nt; base += 256) {
            const int t = base + tid;
            Tri T;
            bool keep = false;
            if (t < jb.nt && tri_setup(tris, jb.t_off + t, jb.nv, pv, T)) {
                const long mnx = min(T.X[0], min(T.X[1], T.X[2])), mxx = max(T.X[0], max(T.X[1], T.X[2]));
                const long mny = min(T.Y[0], min(T.Y[1], T.Y[2])), mxy = max(T.Y[0], max(T.Y[1], T.Y[2]));
                keep = mxx >= tX0 && mnx <= tX1 && mxy >= tY0 && mny <= tY1;
            }
            const unsigned long long bal = __ballot(keep);
            if (lane == 0) wcount[wave] = __popcll(bal);
            __syncthreads();
            int off = 0, total = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { off += w < wave ? wcount[w] : 0; total += wcount[w]; }
            if (keep) {
                const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));     // triangle order preserved
                SurvLds& s = surv[pos];
#pragma unroll
                for (int k = 0; k < 3; ++k) { s.X[k] = T.X[k]; s.Y[k] = T.Y[k]; s.iz[k] = T.iz[k]; }
                s.area = (double)T.area;
                s.tri = t;
            }
            __syncthreads();
            for (int k = 0; k < total; ++k) {
                const SurvLds& s = surv[k];
                long e[3];
                if (!tri_edges(s.X, s.Y, sx, sy, e)) continue;
                const double iz = ((double)e[0] * s.iz[0] + (double)e[1] * s.iz[1] + (double)e[2] * s.iz[2]) / s.area;
                if (iz > best) { best = iz; best_t = s.tri; }
            }
            __syncthreads();                                                  // before the next chunk overwrites surv
        }
    }
    if (inside_frame) {
        const long o = ((long)j * H + py) * W + px;
        unsigned char rgb[3] = {0, 0, 0};
        if (best_t >= 0) {
            Tri T;
            tri_setup(tris, jb.t_off + best_t, jb.nv, pv, T);                 // same arithmetic as the chunk pass: true
            long e[3];
            tri_edges(T.X, T.Y, (long)px * 256, (long)py * 256, e);
            const double w0 = (double)e[0] * T.iz[0], w1 = (double)e[1] * T.iz[1], w2 = (double)e[2] * T.iz[2];
            const double ws = w0 + w1 + w2;
            const PV &a = pv[T.vi[0]], &b = pv[T.vi[1]], &c = pv[T.vi[2]];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double col = (w0 * a.c[ch] + w1 * b.c[ch] + w2 * c.c[ch]) / ws;
                const double q = rint(col * 255.0);
                rgb[ch] = (unsigned char)(q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q));
            }
        }
        sketch[o * 3] = rgb[0]; sketch[o * 3 + 1] = rgb[1]; sketch[o * 3 + 2] = rgb[2];
        mask[o] = best_t >= 0 ? 1 : 0;
        if (tri_id) tri_id[o] = best_t;
    }
    if (covered) {
        const unsigned long long bal = __ballot(inside_frame && best_t >= 0);
        __syncthreads();
        if (lane == 0) wcount[wave] = __popcll(bal);
        __syncthreads();
        if (tid == 0) {
            const int n = wcount[0] + wcount[1] + wcount[2] + wcount[3];
            if (n) atomicAdd(covered + j, n);
        }
    }
}

// ------------------------------------------------------------------------------------------------ plane visibility
// compute_visibility's areas (online_visibility.py:130-150) for 7 planes per job: absolute = pixels in polygon p,
// occluded = pixels in p and in no polygon q with dist[q] < dist[p] (draw_plane_occlusion paints those black).  Membership
// is poly_inside - the rule of fill_poly_planes_kernel.  Grid (blocks, job); each block strides over the frame-clipped
// union box of the job's polygons; wave reduction, one integer atomic per count and workgroup.
constexpr int NPL = 7;

__global__ __launch_bounds__(256) void plane_visibility_kernel(const int* __restrict__ pts_xy, const int* __restrict__ nverts,
                                                               const int* __restrict__ nearer, int H, int W, int* __restrict__ counts) {
    __shared__ int spx[NPL][MAXV], spy[NPL][MAXV], snv[NPL], snear[NPL];
    __shared__ int red[4][2 * NPL];
    const int j = blockIdx.y, tid = threadIdx.x;
    if (tid < NPL * MAXV) {
        const int p = tid / MAXV, i = tid % MAXV;
        spx[p][i] = pts_xy[(((long)j * NPL + p) * MAXV + i) * 2];
        spy[p][i] = pts_xy[(((long)j * NPL + p) * MAXV + i) * 2 + 1];
    }
    if (tid < NPL) {
        const int n = nverts[j * NPL + tid];
        snv[tid] = n < 0 ? 0 : (n > MAXV ? MAXV : n);
        snear[tid] = nearer[j * NPL + tid];
    }
    __syncthreads();
    int x0 = W, y0 = H, x1 = -1, y1 = -1;              // union box of the vertices (outline and interior lie inside it)
    for (int p = 0; p < NPL; ++p)
        for (int i = 0; i < snv[p]; ++i) {
            x0 = min(x0, spx[p][i]); x1 = max(x1, spx[p][i]); y0 = min(y0, spy[p][i]); y1 = max(y1, spy[p][i]);
        }
    x0 = max(x0, 0); y0 = max(y0, 0); x1 = min(x1, W - 1); y1 = min(y1, H - 1);
    int cnt[2 * NPL];
#pragma unroll
    for (int k = 0; k < 2 * NPL; ++k) cnt[k] = 0;
    if (x0 <= x1 && y0 <= y1) {
        const int bw = x1 - x0 + 1;
        const long total = (long)bw * (y1 - y0 + 1);
        for (long idx = (long)blockIdx.x * 256 + tid; idx < total; idx += (long)gridDim.x * 256) {
            const int x = x0 + (int)(idx % bw), y = y0 + (int)(idx / bw);
            int bits = 0;
#pragma unroll
            for (int p = 0; p < NPL; ++p) bits |= poly_inside(x, y, snv[p], spx[p], spy[p]) ? 1 << p : 0;
#pragma unroll
            for (int p = 0; p < NPL; ++p) {
                const int in = (bits >> p) & 1;
                cnt[2 * p] += in;
                cnt[2 * p + 1] += in & ((bits & snear[p]) == 0);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 2 * NPL; ++k) {
        int v = cnt[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < 2 * NPL) {
        const int v = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
        if (v) atomicAdd(counts + (long)j * 2 * NPL + tid, v);
    }
}

}  // namespace fusg

using namespace fusg;

static long render_workspace_bytes(int n_jobs, int max_nv) { return (long)n_jobs * (16 + (long)max_nv * (long)sizeof(PV)); }

static int render_impl(const double* verts, const double* normals, int64_t n_verts, const int32_t* tris, int64_t n_tris,
                       const fusg_render_job* jobs, int32_t n_jobs, int32_t max_nv, int32_t h, int32_t w, void* workspace,
                       int64_t workspace_bytes, uint8_t* sketch, uint8_t* mask, int32_t* tri_id, int32_t* covered, void* stream) {
    FUSG_CHECK(verts && normals && tris && jobs && sketch && mask && n_verts > 0 && n_tris > 0 && n_verts < (1L << 31) &&
               n_tris < (1L << 31) && n_jobs >= 0 && n_jobs <= 65535 && max_nv > 0 && h >= 1 && w >= 1 && h < 32768 && w < 32768,
               "render_normals_u8: arguments");
    FUSG_CHECK(workspace && workspace_bytes >= render_workspace_bytes(n_jobs, max_nv) && ((uintptr_t)workspace & 15) == 0,
               "render_normals_u8: workspace of %ld bytes needed (16-byte aligned)", render_workspace_bytes(n_jobs, max_nv));
    if (n_jobs == 0) return FUSG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (covered && hipMemsetAsync(covered, 0, sizeof(int32_t) * n_jobs, s) != hipSuccess) {
        set_error("render_normals_u8: memset");
        return FUSG_ERR_LAUNCH;
    }
    int4* boxes = (int4*)workspace;
    PV* pv = (PV*)((char*)workspace + 16L * n_jobs);
    hipLaunchKernelGGL(project_kernel, dim3(n_jobs), dim3(256), 0, s, verts, normals, (long)n_verts, jobs, (int)max_nv, boxes, pv);
    FUSG_LAUNCH_CHECK("render_normals_u8 (project)");
    hipLaunchKernelGGL(raster_kernel, dim3((w + TILE - 1) / TILE, (h + TILE - 1) / TILE, n_jobs), dim3(256), 0, s, (const int*)tris,
                       (long)n_tris, jobs, (int)max_nv, (const int4*)boxes, (const PV*)pv, (int)h, (int)w, (unsigned char*)sketch,
                       (unsigned char*)mask, (int*)tri_id, (int*)covered);
    FUSG_LAUNCH_CHECK("render_normals_u8 (raster)");
    return FUSG_OK;
}

extern "C" int fusg_render_normals_u8(const double* verts, const double* normals, int64_t n_verts, const int32_t* tris, int64_t n_tris,
                                      const fusg_render_job* jobs, int32_t n_jobs, int32_t max_nv, int32_t h, int32_t w,
                                      void* workspace, int64_t workspace_bytes, uint8_t* sketch, uint8_t* mask, int32_t* tri_id,
                                      int32_t* covered, void* stream) {
    return plan_dispatch(render_impl, stream, verts, normals, n_verts, tris, n_tris, jobs, n_jobs, max_nv, h, w, workspace,
                         workspace_bytes, sketch, mask, tri_id, covered);
}

static int plane_visibility_impl(const int32_t* pts_xy, const int32_t* nverts, const int32_t* nearer, int32_t n_jobs, int32_t h,
                                 int32_t w, int32_t* counts, void* stream) {
    FUSG_CHECK(pts_xy && nverts && nearer && counts && n_jobs >= 0 && n_jobs <= 65535 && h >= 1 && w >= 1 && h < 32768 && w < 32768,
               "plane_visibility: arguments");
    if (n_jobs == 0) return FUSG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(int32_t) * 2 * NPL * n_jobs, s) != hipSuccess) {
        set_error("plane_visibility: memset");
        return FUSG_ERR_LAUNCH;
    }
    const long px = (long)h * w;
    const int nb = (int)std::min(64L, std::max(1L, px / (256L * 16)));      // ~16 pixels per lane on a full-frame box
    hipLaunchKernelGGL(plane_visibility_kernel, dim3(nb, n_jobs), dim3(256), 0, s, pts_xy, nverts, nearer, (int)h, (int)w, (int*)counts);
    FUSG_LAUNCH_CHECK("plane_visibility");
    return FUSG_OK;
}

extern "C" int fusg_plane_visibility(const int32_t* pts_xy, const int32_t* nverts, const int32_t* nearer, int32_t n_jobs, int32_t h,
                                     int32_t w, int32_t* counts, void* stream) {
    return plan_dispatch(plane_visibility_impl, stream, pts_xy, nverts, nearer, n_jobs, h, w, counts);
}

extern "C" int fusg_sizeof_render_job(void) { return (int)sizeof(fusg_render_job); }
