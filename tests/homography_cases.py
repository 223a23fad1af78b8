"""Seeded problems shared by tests/test_homography_cpu.py and tests/test_gpu_homography.py (no test in here)."""
import numpy as np

FRAME_HW = (720, 1280)
P = 5                                                     # left, right, roof, front, back
QUAD = np.float64([[150, 120], [1100, 90], [1150, 640], [120, 600]])
HEXA = np.float64([[150, 120], [640, 80], [1100, 110], [1150, 640], [640, 680], [120, 600]])


def apply_h(H, pts):
    q = np.c_[np.asarray(pts, np.float64), np.ones(len(pts))] @ np.asarray(H).T
    return q[:, :2] / q[:, 2:]


def rand_h(rng, shear=0.15, shift=60.0, persp=1.5e-4):
    H = np.eye(3)
    H[:2, :2] += rng.uniform(-shear, shear, (2, 2))
    H[:2, 2] = rng.uniform(-shift, shift, 2)
    H[2, :2] = rng.uniform(-persp, persp, 2)
    return H


def pixel_metric(Ha, Hb, pts, frame_hw=FRAME_HW):
    """Largest distance in pixels between Ha x and Hb x over the point set and the four corners of the frame."""
    h, w = frame_hw
    x = np.vstack([np.asarray(pts, np.float64).reshape(-1, 2), [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]])
    d = apply_h(Ha, x) - apply_h(Hb, x)
    return float(np.hypot(d[:, 0], d[:, 1]).max())


def solver_cases():
    """(name, src int32 [n, 2], dst int32 [n, 2]): corner points as plane_polygons produces them (truncated to int32) on a
    720 x 1280 frame.  The destination of a 'perspective' / 'hexagon' case is a projective image of the source truncated to
    whole pixels: exactly projective never, within one pixel always - so the 6-point fits run Levenberg-Marquardt to the
    rounding floor, where steps are rejected."""
    rng = np.random.default_rng(20240)
    q = np.int32(QUAD)
    cases = [("translation", q, q + np.int32([37, -21])), ("scale", q // 4, (q // 4) * 3)]
    for t in range(4):
        s = np.int32(QUAD + rng.uniform(-50, 50, (4, 2)))
        cases.append((f"perspective{t}", s, np.int32(apply_h(rand_h(rng), s))))
    for t in range(3):
        s = np.int32(HEXA + rng.uniform(-40, 40, (6, 2)))
        cases.append((f"hexagon{t}", s, np.int32(apply_h(rand_h(rng), s))))
    return cases


def frame_fixture(hw=(96, 128), seed=5):
    """V = 3 vehicles of 5 planes on a small frame, with visibilities that take every branch of the gate:
    vehicle 0: left -> right swap onto the slot the right plane also takes (two sources on one slot, the higher wins), roof
               not visible in the source, front's destination hidden, back plain;
    vehicle 1: right -> left swap onto left's own slot; the roof passes the gate but its destination corners are collinear
               (invalid fit); front and back plain, back's quadrilateral leaves the frame;
    vehicle 2: both symmetric destinations hidden, roof plain, front / back not visible in the source.
    Returns src_kp, dst_kp ([V][P] int32 [n, 2]), src_vis, dst_vis (uint8 [V, P]) and planes uint8 [V, P, h, w, 3]."""
    h, w = hw
    rng = np.random.default_rng(seed)
    cx, cy = w / 2, h / 2

    def poly(n, ox, oy, rx, ry):
        ang = np.linspace(0, 2 * np.pi, n, endpoint=False) + rng.uniform(-0.2, 0.2, n) + 0.4
        return np.stack([cx + ox + rx * np.cos(ang), cy + oy + ry * np.sin(ang)], 1)

    spec = [(6, -22, 0, 30, 34), (6, 22, 0, 30, 34), (4, 0, -18, 40, 20), (4, 0, 6, 36, 24), (4, 0, 20, 40, 18)]
    src_kp, dst_kp = [], []
    for v in range(3):
        s = [np.int32(poly(*sp)) for sp in spec]
        d = [np.int32(apply_h(rand_h(rng, 0.08, 6.0, 4e-4), p)) for p in s]
        src_kp.append(s)
        dst_kp.append(d)
    dst_kp[1][2] = np.int32([[10, 10], [20, 20], [30, 30], [40, 40]])            # collinear: no homography
    dst_kp[1][4] = dst_kp[1][4] + np.int32([70, 30])                               # most of the quadrilateral leaves the frame
    src_vis = np.uint8([[1, 1, 0, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 0, 0]])
    dst_vis = np.uint8([[0, 1, 1, 0, 1], [1, 0, 1, 1, 1], [0, 0, 1, 1, 1]])
    planes = rng.integers(1, 256, (3, P, h, w, 3), dtype=np.uint8)
    return dict(src_kp=src_kp, dst_kp=dst_kp, src_vis=src_vis, dst_vis=dst_vis, planes=planes, hw=hw)


# the table the fixture's visibilities give (source plane per (vehicle, slot), -1: none), derived by hand from warp_jobs
FIXTURE_SOURCES = np.int32([[-1, 1, -1, -1, 4], [1, -1, -1, 3, 4], [-1, -1, 2, -1, -1]])
FIXTURE_STATUS = np.int32([[0, 1, 0, 0, 1], [1, 0, 2, 1, 1], [0, 0, 1, 0, 0]])


def tables_from_jobs(jobs_per_vehicle, V, planes=P):
    """(index int32 [V * P, 2], minv float64 [V * P, 9]) as warp_planes_batch derives them from warp_jobs_frame's jobs: of two
    jobs on one slot the later (higher source plane) one stays; LAPACK inverse of its H12."""
    index = np.stack([np.full(V * planes, -1, np.int32), np.arange(V * planes, dtype=np.int32)], 1)
    minv = np.zeros((V * planes, 9))
    for v, jobs in enumerate(jobs_per_vehicle):
        for i, j, H12, _ in jobs:
            index[v * planes + j, 0] = v * planes + i
            minv[v * planes + j] = np.linalg.inv(H12).reshape(9)
    return index, minv


def warp_u8(src, minv, cv_host):
    """oracle.cv_host.warp_perspective_u8 from the INVERSE matrix (that function inverts H itself)."""
    h, w = src.shape[:2]
    sx, sy, alpha = cv_host.perspective_coords(np.asarray(minv, np.float64).reshape(3, 3), w, h)
    wt = cv_host.bilinear_tab_i()[alpha]
    acc = np.zeros((h, w, src.shape[2]), dtype=np.int64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = sy + dy, sx + dx
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        val = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64)
        acc += np.where(ok[..., None], val, 0) * wt[..., k:k + 1]
    return np.clip((acc + (1 << (cv_host.REMAP_COEF_BITS - 1))) >> cv_host.REMAP_COEF_BITS, 0, 255).astype(np.uint8)
