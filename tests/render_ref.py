"""numpy restatement of the per-vehicle geometry kernels (csrc/render.hip) - a helper module of the tests, not a conftest.

`raster` is the rasteriser's arithmetic written out in float64 / int64 numpy, operation for operation as the kernel does
it (so bytes can be compared): vertex projection, 1/256-px snapping, int64 edge functions with the top-left rule, the
nearest fragment by interpolated 1/z with ties to the lower triangle index, perspective-correct colour.  `vis_counts` is
compute_visibility's areas with oracle.cv_host.fill_poly_mask as the polygon rule.  `rounded_box` / `box_around` make procedural bank
meshes: a subdivided, bevelled (rounded) box around a set of 3-D keypoints.  Parity of these rules with Open3D / OpenCV
themselves is unpinned."""
import numpy as np

from oracle.cv_host import fill_poly_mask

MAX_PX = 2097152.0
NEAR_Z = 1e-3


def project(verts, normals, R, tr, E, fx, fy, cx, cy):
    """-> X, Y (int64, 1/256 px), iz (1/Zc, -1 where Zc <= 1e-3), colour [n, 3]; the kernel's order of operations."""
    v, n = np.asarray(verts, np.float64), np.asarray(normals, np.float64)
    R, tr, E = np.asarray(R, np.float64).reshape(3, 3), np.asarray(tr, np.float64).reshape(3), np.asarray(E, np.float64)
    p = [v[:, 0] * R[0, k] + v[:, 1] * R[1, k] + v[:, 2] * R[2, k] + tr[k] for k in range(3)]
    c = np.stack([(n[:, 0] * R[0, k] + n[:, 1] * R[1, k] + n[:, 2] * R[2, k] + 1.0) / 2.0 for k in range(3)], 1)
    Xc, Yc, Zc = (E[r, 0] * p[0] + E[r, 1] * p[1] + E[r, 2] * p[2] + E[r, 3] for r in range(3))
    ok = Zc > NEAR_Z
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x = np.clip(fx * (Xc / Zc) + cx, -MAX_PX, MAX_PX)
        y = np.clip(fy * (Yc / Zc) + cy, -MAX_PX, MAX_PX)
        X = np.where(ok, np.rint(x * 256.0), 0).astype(np.int64)
        Y = np.where(ok, np.rint(y * 256.0), 0).astype(np.int64)
        iz = np.where(ok, 1.0 / Zc, -1.0)
    return X, Y, iz, c


def raster(verts, normals, tris, R, tr, E, fx, fy, cx, cy, H, W):
    """One job -> sketch uint8 [H, W, 3], mask uint8 [H, W], tri int32 [H, W] (-1 = background)."""
    X, Y, iz, col = project(verts, normals, R, tr, E, fx, fy, cx, cy)
    best = np.full((H, W), -1.0)
    tri = np.full((H, W), -1, np.int32)
    sketch = np.zeros((H, W, 3), np.uint8)
    for t, (i0, i1, i2) in enumerate(np.asarray(tris, np.int64)):
        if min(iz[i0], iz[i1], iz[i2]) <= 0:
            continue
        area = int((X[i1] - X[i0]) * (Y[i2] - Y[i0]) - (Y[i1] - Y[i0]) * (X[i2] - X[i0]))
        if area == 0:
            continue
        if area < 0:
            i1, i2, area = i2, i1, -area
        vi = (i0, i1, i2)
        xs, ys = [int(X[i]) for i in vi], [int(Y[i]) for i in vi]
        x0, x1 = max(-(-min(xs) // 256), 0), min(max(xs) // 256, W - 1)
        y0, y1 = max(-(-min(ys) // 256), 0), min(max(ys) // 256, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64) * 256
        inside = np.ones(px.shape, bool)
        e = []
        for i in range(3):
            a, b = (i + 1) % 3, (i + 2) % 3
            dx, dy = xs[b] - xs[a], ys[b] - ys[a]
            ei = dx * (py - ys[a]) - dy * (px - xs[a])
            tl = dy < 0 or (dy == 0 and dx > 0)
            inside &= (ei > 0) | ((ei == 0) & tl)
            e.append(ei.astype(np.float64))
        z = (e[0] * iz[vi[0]] + e[1] * iz[vi[1]] + e[2] * iz[vi[2]]) / float(area)
        sub = best[y0:y1 + 1, x0:x1 + 1]
        upd = inside & (z > sub)
        if not upd.any():
            continue
        sub[upd] = z[upd]
        tri[y0:y1 + 1, x0:x1 + 1][upd] = t
        w = [e[k][upd] * iz[vi[k]] for k in range(3)]
        ws = w[0] + w[1] + w[2]
        for ch in range(3):
            c = (w[0] * col[vi[0], ch] + w[1] * col[vi[1], ch] + w[2] * col[vi[2], ch]) / ws
            sketch[y0:y1 + 1, x0:x1 + 1, ch][upd] = np.clip(np.rint(c * 255.0), 0, 255).astype(np.uint8)
    return sketch, (tri >= 0).astype(np.uint8), tri


def render_bank_job(bank, job):
    """raster() of one fusg_render_job record (render.render_jobs) of `bank`."""
    m = int(np.searchsorted(bank.v_off, job["v_off"], side="right") - 1)
    return m, (bank.vertices[m], bank.normals[m], bank.triangles[m], job["R"], job["tr"], job["E"].reshape(3, 4),
               float(job["fx"]), float(job["fy"]), float(job["cx"]), float(job["cy"]))


def vis_counts(pts, nv, nearer, H, W):
    """(absolute, occluded) per plane [7, 2] of one job with oracle.cv_host.fill_poly_mask (draw_plane_simple /
    draw_plane_occlusion, online_visibility.py:75-100)."""
    masks = [fill_poly_mask((H, W), np.asarray(pts[p][:nv[p]])).astype(bool) if nv[p] else np.zeros((H, W), bool)
             for p in range(7)]
    out = np.zeros((7, 2), np.int64)
    for p in range(7):
        occ = masks[p].copy()
        for q in range(7):
            if (int(nearer[p]) >> q) & 1:
                occ &= ~masks[q]
        out[p] = masks[p].sum(), occ.sum()
    return out


# ---------------------------------------------------------------------------------------------- procedural meshes
def rounded_box(n=16, half=(1.0, 2.0, 0.7), center=(0.0, 0.0, 0.0), p=4.0):
    """A cube's six faces subdivided n x n (each face with vertices of its own), pushed onto the superellipsoid
    |x|^p + |y|^p + |z|^p = 1 (a bevelled box; p=None keeps the cube), scaled by `half` and moved to `center`:
    vertices [6 (n+1)^2, 3], triangles [12 n^2, 3]."""
    g = np.linspace(-1.0, 1.0, n + 1)
    u, v = np.meshgrid(g, g, indexing="ij")
    verts, tris = [], []
    faces = [(0, 1, 2, 1.0), (0, 2, 1, -1.0), (1, 2, 0, 1.0), (1, 0, 2, -1.0), (2, 0, 1, 1.0), (2, 1, 0, -1.0)]
    for a, b, c, s in faces:
        q = np.zeros(((n + 1) ** 2, 3))
        q[:, a], q[:, b], q[:, c] = u.ravel(), v.ravel(), s
        base = len(verts) * (n + 1) ** 2
        verts.append(q)
        idx = np.arange((n + 1) ** 2).reshape(n + 1, n + 1) + base
        quad = np.stack([idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]], -1).reshape(-1, 4)
        tris.append(np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]]))
    V = np.concatenate(verts)
    if p is not None:
        V = V / ((np.abs(V) ** p).sum(1, keepdims=True) ** (1.0 / p))
    return V * np.asarray(half) + np.asarray(center), np.concatenate(tris).astype(np.int64)


def car_keypoints(half=(1.0, 2.0, 0.7), center=(0.0, 0.0, 0.0)):
    """12 keypoints of a box car in KP_NAMES order (x = right, y = back, z = up)."""
    hx, hy, hz = half
    side = {"left": -hx, "right": hx}
    kp = []
    for s in ("left", "right"):
        x = side[s]
        kp += [(x, hy, 0.1 * hz), (x, 0.65 * hy, -0.9 * hz), (x, -hy, 0.1 * hz), (x, -0.65 * hy, -0.9 * hz)]
    for s in ("left", "right"):
        x = 0.8 * side[s]
        kp += [(x, 0.45 * hy, 0.95 * hz), (x, -0.3 * hy, 0.95 * hz)]
    return np.asarray(kp) + np.asarray(center)


def box_around(kp3d, n=16, margin=1.05):
    """A rounded box mesh enclosing keypoints kp3d [12, 3] (axis-aligned, centred on their box)."""
    kp = np.asarray(kp3d, np.float64)
    lo, hi = kp.min(0), kp.max(0)
    return rounded_box(n, tuple(np.maximum((hi - lo) / 2 * margin, 1e-3)), tuple((hi + lo) / 2))
