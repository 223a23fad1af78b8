"""Drop-in for the reference's ``warp_learn.planes_utils`` (+ ``get_icn_inputs`` of ``warp_learn.models``) with the
uint8 image work on the MI355X (§8f-1, §8f-2).

Same function names and argument meaning as the reference (``warp_learn/planes_utils.py:11-118``,
``warp_learn/models.py:323-366``).  Images may be numpy arrays (the reference's type: they are uploaded, processed by
the libfusg kernels of ``csrc/cvops.hip`` and downloaded again, so the functions stay call-compatible with
``trajectory_inference.py``) or CUDA ``torch.uint8`` tensors (then everything stays on the device and the returned
images are CUDA tensors - the point of moving these steps: 5 planes of 2.76 MB per vehicle and frame no longer cross
PCIe twice).  What stays on the host, as north_star says for the geometry: the homography fit
(``find_homography``: 4-6 point pairs) and the bounding-box arithmetic of ``square_crop_from_bbox``.

The arithmetic is OpenCV's (``warpPerspective``, ``fillPoly``, ``resize``, ``cvtColor`` Lab) in its published 8-bit
fixed-point form; the reference pins no OpenCV version and OpenCV is not available where this was built, so parity
with a particular OpenCV build is UNPINNED (oracle/cv_host.py states the algorithms; tests compare kernel and oracle
bit for bit and check OpenCV's documented invariants).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib as L
from .. import ops

Image = Union[np.ndarray, torch.Tensor]

# which keypoints bound each texture plane of a car, in the reference's key order (warp_learn/online_visibility.py:9-23)
CAR_TEXTURE_PLANES = {
    "left": ["left_back_trunk", "left_back_wheel", "left_front_wheel", "left_front_light", "upper_left_windshield",
             "upper_left_rearwindow"],
    "right": ["right_back_trunk", "right_back_wheel", "right_front_wheel", "right_front_light", "upper_right_windshield",
              "upper_right_rearwindow"],
    "roof": ["upper_left_rearwindow", "upper_left_windshield", "upper_right_windshield", "upper_right_rearwindow"],
    "front": ["left_front_light", "right_front_light", "upper_right_windshield", "upper_left_windshield"],
    "back": ["left_back_trunk", "right_back_trunk", "upper_right_rearwindow", "upper_left_rearwindow"],
}
pascal_texture_planes = {"car": CAR_TEXTURE_PLANES, "chair": {}}
MAX_VERTS = 8


# ---------------------------------------------------------------------------------------------- plumbing
def _device(device=None) -> torch.device:
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _to_dev(img: Image, device=None) -> Tuple[torch.Tensor, bool]:
    """uint8 image(s) -> contiguous CUDA tensor; second value: was it numpy (then results go back as numpy)."""
    if isinstance(img, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(img)).to(_device(device)), True
    ops._require_gpu(img, "image")
    if img.dtype != torch.uint8:
        raise TypeError(f"expected uint8 images, got {img.dtype}")
    return img.contiguous(), False


def _back(t: torch.Tensor, as_numpy: bool) -> Image:
    return t.cpu().numpy() if as_numpy else t


def _u8desc(t: torch.Tensor) -> L.Tensor:
    """fusg_tensor of a uint8 [n, h, w, c] tensor: logical NCHW extents, HWC strides."""
    assert t.dim() == 4 and t.dtype == torch.uint8, (t.shape, t.dtype)
    return ops.desc(t.permute(0, 3, 1, 2))


# ---------------------------------------------------------------------------------------------- host geometry
def find_homography(src_points, dst_points) -> Optional[np.ndarray]:
    """``cv2.findHomography(src, dst)[0]`` with the default method 0 (all points, least squares): Hartley-normalised
    direct linear transform - the eigenvector of the smallest eigenvalue of A^T A, as OpenCV solves it - followed by
    Levenberg-Marquardt refinement of the reprojection error when there are more than four points.  Host side by design
    (4-6 point pairs).  Returns None where OpenCV returns None (degenerate configuration)."""
    s = np.asarray(src_points, dtype=np.float64).reshape(-1, 2)
    d = np.asarray(dst_points, dtype=np.float64).reshape(-1, 2)
    n = len(s)
    if n < 4 or len(d) != n:
        return None
    cs, cd = s.mean(0), d.mean(0)
    ss, sd = np.abs(s - cs).mean(0), np.abs(d - cd).mean(0)
    if min(ss.min(), sd.min()) < np.finfo(np.float64).eps:
        return None
    ss, sd = 1.0 / ss, 1.0 / sd
    xs, xd = (s - cs) * ss, (d - cd) * sd
    A = np.zeros((2 * n, 9))
    A[0::2, 0:2], A[0::2, 2] = xs, 1.0
    A[0::2, 6:8], A[0::2, 8] = -xd[:, 0:1] * xs, -xd[:, 0]
    A[1::2, 3:5], A[1::2, 5] = xs, 1.0
    A[1::2, 6:8], A[1::2, 8] = -xd[:, 1:2] * xs, -xd[:, 1]
    ev, evec = np.linalg.eigh(A.T @ A)
    if ev[1] < 1e-12 * max(ev[-1], 1e-300):                           # rank loss: no unique homography
        return None
    Hn = evec[:, 0].reshape(3, 3)
    Td_inv = np.array([[1 / sd[0], 0, cd[0]], [0, 1 / sd[1], cd[1]], [0, 0, 1.0]])
    Ts = np.array([[ss[0], 0, -cs[0] * ss[0]], [0, ss[1], -cs[1] * ss[1]], [0, 0, 1.0]])
    H = Td_inv @ Hn @ Ts
    if abs(H[2, 2]) < np.finfo(np.float64).tiny:
        return None
    H = H / H[2, 2]
    if n > 4:                                                          # LM on the 8 free parameters
        h = H.reshape(-1)[:8].copy()
        lam = 1e-3

        def resid(hv):
            Hc = np.append(hv, 1.0).reshape(3, 3)
            p = np.c_[s, np.ones(n)] @ Hc.T
            return (p[:, :2] / p[:, 2:3] - d).reshape(-1), p

        r, p = resid(h)
        for _ in range(10):
            J = np.zeros((2 * n, 8))
            w = p[:, 2]
            J[0::2, 0], J[0::2, 1], J[0::2, 2] = s[:, 0] / w, s[:, 1] / w, 1 / w
            J[0::2, 6], J[0::2, 7] = -p[:, 0] * s[:, 0] / w ** 2, -p[:, 0] * s[:, 1] / w ** 2
            J[1::2, 3], J[1::2, 4], J[1::2, 5] = s[:, 0] / w, s[:, 1] / w, 1 / w
            J[1::2, 6], J[1::2, 7] = -p[:, 1] * s[:, 0] / w ** 2, -p[:, 1] * s[:, 1] / w ** 2
            JtJ, g = J.T @ J, J.T @ r
            step = np.linalg.solve(JtJ + lam * np.diag(np.diag(JtJ)), -g)
            r2, p2 = resid(h + step)
            if r2 @ r2 <= r @ r:
                h, r, p, lam = h + step, r2, p2, lam * 0.1
                if np.abs(step).max() < 1e-13:
                    break
            else:
                lam *= 10.0
        H = np.append(h, 1.0).reshape(3, 3)
    return H


def find_homography_batch(pairs: Sequence[Tuple[np.ndarray, np.ndarray]]) -> List[Optional[np.ndarray]]:
    """`find_homography` for many point sets at once - the same arithmetic per problem (normalised DLT through the symmetric
    eigen-decomposition, then Levenberg-Marquardt with the same acceptance rule), vectorised over the problems of equal point
    count: a frame of 8 vehicles needs ~46 fits, and one Python call per fit (150 us of numpy overhead each) was the largest
    host cost of `VehiclePipeline.run_frame`.  Returns one 3x3 matrix (or None) per pair, in order.  The matrices equal
    `find_homography`'s bit for bit on well-posed fits (tests/test_cv_host_cpu.py); on a near-degenerate one (condition number
    ~1e9: unrelated quadrilaterals) LAPACK's batched and single eigen-decompositions differ in the last place."""
    out: List[Optional[np.ndarray]] = [None] * len(pairs)
    groups: Dict[int, List[int]] = {}
    for i, (sp, dp) in enumerate(pairs):
        sp = np.asarray(sp, dtype=np.float64).reshape(-1, 2)
        dp = np.asarray(dp, dtype=np.float64).reshape(-1, 2)
        if len(sp) >= 4 and len(sp) == len(dp):
            groups.setdefault(len(sp), []).append(i)
    eps = np.finfo(np.float64).eps
    for n, idx in groups.items():
        s = np.stack([np.asarray(pairs[i][0], dtype=np.float64).reshape(-1, 2) for i in idx])      # [N, n, 2]
        d = np.stack([np.asarray(pairs[i][1], dtype=np.float64).reshape(-1, 2) for i in idx])
        N = len(idx)
        cs, cd = s.mean(1), d.mean(1)
        ss, sd = np.abs(s - cs[:, None]).mean(1), np.abs(d - cd[:, None]).mean(1)
        ok = np.minimum(ss.min(1), sd.min(1)) >= eps
        ss = 1.0 / np.where(ss >= eps, ss, 1.0)
        sd = 1.0 / np.where(sd >= eps, sd, 1.0)
        xs, xd = (s - cs[:, None]) * ss[:, None], (d - cd[:, None]) * sd[:, None]
        A = np.zeros((N, 2 * n, 9))
        A[:, 0::2, 0:2], A[:, 0::2, 2] = xs, 1.0
        A[:, 0::2, 6:8], A[:, 0::2, 8] = -xd[:, :, 0:1] * xs, -xd[:, :, 0]
        A[:, 1::2, 3:5], A[:, 1::2, 5] = xs, 1.0
        A[:, 1::2, 6:8], A[:, 1::2, 8] = -xd[:, :, 1:2] * xs, -xd[:, :, 1]
        ev, evec = np.linalg.eigh(np.matmul(A.transpose(0, 2, 1), A))
        ok &= ev[:, 1] >= 1e-12 * np.maximum(ev[:, -1], 1e-300)
        Hn = evec[:, :, 0].reshape(N, 3, 3)
        Td_inv = np.zeros((N, 3, 3))
        Td_inv[:, 0, 0], Td_inv[:, 0, 2], Td_inv[:, 1, 1], Td_inv[:, 1, 2], Td_inv[:, 2, 2] = 1 / sd[:, 0], cd[:, 0], 1 / sd[:, 1], cd[:, 1], 1.0
        Ts = np.zeros((N, 3, 3))
        Ts[:, 0, 0], Ts[:, 0, 2], Ts[:, 1, 1], Ts[:, 1, 2], Ts[:, 2, 2] = ss[:, 0], -cs[:, 0] * ss[:, 0], ss[:, 1], -cs[:, 1] * ss[:, 1], 1.0
        H = np.matmul(np.matmul(Td_inv, Hn), Ts)
        ok &= np.abs(H[:, 2, 2]) >= np.finfo(np.float64).tiny
        H = H / np.where(ok, H[:, 2, 2], 1.0)[:, None, None]
        if n > 4:                                                      # LM on the 8 free parameters, per-problem acceptance
            h = H.reshape(N, 9)[:, :8].copy()
            lam = np.full(N, 1e-3)
            live = ok.copy()
            sh = np.concatenate([s, np.ones((N, n, 1))], 2)            # homogeneous source points

            def resid(hv):
                Hc = np.concatenate([hv, np.ones((len(hv), 1))], 1).reshape(-1, 3, 3)
                pp = np.matmul(sh, Hc.transpose(0, 2, 1))
                return (pp[:, :, :2] / pp[:, :, 2:3] - d).reshape(len(hv), -1), pp

            with np.errstate(all="ignore"):
                r, pp = resid(h)
                for _ in range(10):
                    if not live.any():
                        break
                    w = pp[:, :, 2]
                    J = np.zeros((N, 2 * n, 8))
                    J[:, 0::2, 0], J[:, 0::2, 1], J[:, 0::2, 2] = s[:, :, 0] / w, s[:, :, 1] / w, 1 / w
                    J[:, 0::2, 6], J[:, 0::2, 7] = -pp[:, :, 0] * s[:, :, 0] / w ** 2, -pp[:, :, 0] * s[:, :, 1] / w ** 2
                    J[:, 1::2, 3], J[:, 1::2, 4], J[:, 1::2, 5] = s[:, :, 0] / w, s[:, :, 1] / w, 1 / w
                    J[:, 1::2, 6], J[:, 1::2, 7] = -pp[:, :, 1] * s[:, :, 0] / w ** 2, -pp[:, :, 1] * s[:, :, 1] / w ** 2
                    JtJ = np.matmul(J.transpose(0, 2, 1), J)
                    g = np.matmul(J.transpose(0, 2, 1), r[:, :, None])[:, :, 0]
                    M = JtJ + lam[:, None, None] * (JtJ * np.eye(8)[None])
                    M[~live] = np.eye(8)                               # finished / rejected problems: a harmless system
                    step = np.linalg.solve(M, -g[:, :, None])[:, :, 0]
                    r2, pp2 = resid(h + step)
                    better = live & ((r2 * r2).sum(1) <= (r * r).sum(1))
                    h[better] += step[better]
                    r[better], pp[better] = r2[better], pp2[better]
                    done = better & (np.abs(step).max(1) < 1e-13)
                    lam = np.where(better, lam * 0.1, np.where(live, lam * 10.0, lam))
                    live &= ~done
            H = np.concatenate([h, np.ones((N, 1))], 1).reshape(N, 3, 3)
        for k, i in enumerate(idx):
            out[i] = H[k] if ok[k] else None
    return out


def square_crop_geometry(image_hw: Tuple[int, int], bbox: Sequence[int]):
    """The window ``square_crop_from_bbox`` (utils/crop_utils.py:4-52, 'pascal' branch) cuts out of the zero-padded
    image, without copying pixels: ((x0, y0, x1, y1), pad_xy_before, pad_xy_after)."""
    image_h, image_w = image_hw
    x_min, y_min, x_max, y_max = [int(v) for v in bbox]
    side_x, side_y = x_max - x_min, y_max - y_min
    major = max(side_x, side_y) * 1.1
    cx, cy = x_min + side_x / 2, y_min + side_y / 2
    pad = {"xb": 0, "xa": 0, "yb": 0, "ya": 0}
    x0 = int(cx - major / 2.0)
    if x0 < 0:
        pad["xb"], x0 = int(np.ceil(abs(x0))), 0
    x1 = int(cx + major / 2.0) + pad["xb"]
    if x1 > image_w:
        pad["xa"] = int(np.ceil(abs(x1 - image_w)))
        x1 = image_w + pad["xa"]
    y0 = int(cy - major / 2.0)
    if y0 < 0:
        pad["yb"], y0 = int(np.ceil(abs(y0))), 0
    y1 = int(cy + major / 2.0) + pad["yb"]
    if y1 > image_h:
        pad["ya"] = int(np.ceil(abs(y1 - image_h)))
        y1 = image_h + pad["ya"]
    return (x0, y0, x1, y1), (pad["xb"], pad["yb"]), (pad["xa"], pad["ya"])


def _geom_row(win, pb, pa) -> List[int]:
    return [win[0], win[1], win[2], win[3], pb[0], pb[1], pa[0], pa[1]]


# ---------------------------------------------------------------------------------------------- W-2: get_planes
def plane_polygons(image_hw: Tuple[int, int], src_kpoint_dict: Dict[str, Sequence[float]], pascal_class: str = "car",
                   texture_planes=None) -> List[np.ndarray]:
    """int32 polygons of the texture planes in pixels: normalised keypoints * (w, h), truncated (planes_utils.py:20-27)."""
    h, w = image_hw
    table = (texture_planes or pascal_texture_planes)[pascal_class]
    polys = []
    for names in table.values():
        p = np.asarray([list(map(float, src_kpoint_dict[k])) for k in names])
        p[:, 0] *= w
        p[:, 1] *= h
        polys.append(np.int32(p))
    return polys


def fill_planes(image: torch.Tensor, polygons: Sequence[np.ndarray]) -> torch.Tensor:
    """image [H, W, 3] CUDA uint8, polygons: int32 [n_i, 2] -> [P, H, W, 3] = image * fillPoly mask of each polygon."""
    P = len(polygons)
    if not 1 <= P <= 8 or any(len(p) > MAX_VERTS for p in polygons):
        raise ValueError("fill_planes: 1..8 polygons of at most 8 vertices")
    pts = np.zeros((P, MAX_VERTS, 2), dtype=np.int32)
    nv = np.zeros(P, dtype=np.int32)
    for i, p in enumerate(polygons):
        nv[i] = len(p)
        pts[i, :len(p)] = np.asarray(p, dtype=np.int32).reshape(-1, 2)
    H, W, _ = image.shape
    out = torch.empty((P, H, W, 3), dtype=torch.uint8, device=image.device)
    with torch.cuda.device(image.device):
        L.check(L.lib().fusg_fill_poly_planes_u8(C.byref(_u8desc(image[None])), pts.ctypes.data, nv.ctypes.data, P,
                                                 C.byref(_u8desc(out)), ops.stream_ptr()), "fill_poly_planes_u8")
    return out


def fill_planes_batch(image: torch.Tensor, pts: torch.Tensor, nverts: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """`fill_planes` for V vehicles in one launch (fusg_fill_poly_planes_batch_u8): image [H, W, 3] CUDA uint8, pts DEVICE
    int32 [V, P, 8, 2] (or flat), nverts DEVICE int32 [V, P] (or flat), out uint8 [V, P, H, W, 3] (written, returned)."""
    V, P, H, W, _ = out.shape
    if out.dtype != torch.uint8 or not out.is_contiguous() or tuple(image.shape) != (H, W, 3):
        raise ValueError("fill_planes_batch: out must be a contiguous uint8 [V, P, H, W, 3] of the image's size")
    if pts.dtype != torch.int32 or nverts.dtype != torch.int32 or not (pts.is_contiguous() and nverts.is_contiguous()) or \
            pts.numel() != V * P * MAX_VERTS * 2 or nverts.numel() != V * P:
        raise ValueError("fill_planes_batch: pts int32 [V, P, 8, 2] and nverts int32 [V, P], contiguous")
    if V == 0:
        return out
    with torch.cuda.device(image.device):
        L.check(L.lib().fusg_fill_poly_planes_batch_u8(C.byref(_u8desc(image[None])), pts.data_ptr(), nverts.data_ptr(), V, P,
                                                       C.byref(_u8desc(out.view(V * P, H, W, 3))), ops.stream_ptr()),
                "fill_poly_planes_batch_u8")
    return out


def fill_planes_frames(frames: Sequence[torch.Tensor], frame_rows: Sequence[int], pts: torch.Tensor, nverts: torch.Tensor,
                       out: torch.Tensor) -> torch.Tensor:
    """`fill_planes_batch` for vehicles of F different images in ONE launch (fusg_fill_poly_planes_frames_u8): frames = F CUDA
    uint8 [H, W, 3] images of one size; frame_rows = F + 1 host offsets, vehicles [frame_rows[f], frame_rows[f + 1]) are cut from
    frames[f]; pts, nverts and out as there.  The bytes are those of F calls of `fill_planes_batch`; a frame without vehicles
    is not read."""
    from ..frame_ops import _frame_table
    V, P, H, W, _ = out.shape
    ptrs, offs, keep, hw = _frame_table(frames, frame_rows, V, "fill_planes_frames")
    if out.dtype != torch.uint8 or not out.is_contiguous() or hw != (H, W) or out.device != keep[0].device:
        raise ValueError("fill_planes_frames: out must be a contiguous uint8 [V, P, H, W, 3] of the frames' size, on their device")
    if pts.dtype != torch.int32 or nverts.dtype != torch.int32 or not (pts.is_contiguous() and nverts.is_contiguous()) or \
            pts.numel() != V * P * MAX_VERTS * 2 or nverts.numel() != V * P or not (pts.is_cuda and nverts.is_cuda):
        raise ValueError("fill_planes_frames: pts int32 [V, P, 8, 2] and nverts int32 [V, P], contiguous, on the device")
    with torch.cuda.device(out.device):
        L.check(L.lib().fusg_fill_poly_planes_frames_u8(ptrs, offs, len(keep), H, W, pts.data_ptr(), nverts.data_ptr(), V, P,
                                                        C.byref(_u8desc(out.view(V * P, H, W, 3))), ops.stream_ptr()),
                "fill_poly_planes_frames_u8")
    return out


def get_planes(image: Image, src_kpoint_dict, pascal_class: str, planes_visibility):
    """Reference signature (planes_utils.py:11-37): (planes [P, H, W, 3], polygon list, visibilities uint8 [P])."""
    img, as_np = _to_dev(image)
    polys = plane_polygons(tuple(img.shape[:2]), src_kpoint_dict, pascal_class)
    names = list(pascal_texture_planes[pascal_class].keys())
    vis = np.stack([planes_visibility[n] for n in names]).astype(np.uint8)
    return _back(fill_planes(img, polys), as_np), polys, vis


# ---------------------------------------------------------------------------------------------- W-1: warp
def warp_perspective(src: torch.Tensor, H: Sequence[np.ndarray], dsize: Tuple[int, int]) -> torch.Tensor:
    """``cv2.warpPerspective(src[i], H[i], dsize=(w, h))`` for a batch: src [N, h, w, 3] CUDA uint8, H: N 3x3 matrices
    (host, double; inverted here in double as OpenCV does) -> [N, dsize[1], dsize[0], 3]."""
    n = src.shape[0]
    minv = np.stack([np.linalg.inv(np.asarray(h, dtype=np.float64)) for h in H]).reshape(n, 9)
    minv_d = ops.h2d(minv, src.device)
    out = torch.empty((n, dsize[1], dsize[0], 3), dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        L.check(L.lib().fusg_warp_perspective_u8(C.byref(_u8desc(src)), minv_d.data_ptr(), C.byref(_u8desc(out)),
                                                 ops.stream_ptr()), "warp_perspective_u8")
    return out


def warp_jobs(src_planes_kpoints, dst_planes_kpoints, src_visibilities, dst_visibilities, pascal_class: str = "car",
              texture_planes=None):
    """The host half of warp_unwarp_planes (planes_utils.py:53-75): which planes are warped where, and their two
    homographies.  -> list of (source plane i, destination slot j, H12, H21)."""
    keys = list((texture_planes or pascal_texture_planes)[pascal_class].keys())
    sym = [keys.index("left"), keys.index("right")]
    jobs = []
    for i in range(len(keys)):
        if not src_visibilities[i]:
            continue
        if i not in sym and not dst_visibilities[i]:
            continue
        if i in sym and 1 not in [dst_visibilities[j] for j in sym]:
            continue
        j = i
        if i in sym and not dst_visibilities[i]:
            j = sym[0] if i == sym[1] else sym[1]
        H12 = find_homography(src_planes_kpoints[i], dst_planes_kpoints[j])
        H21 = find_homography(dst_planes_kpoints[j], src_planes_kpoints[i])
        if H12 is not None and H21 is not None:
            jobs.append((i, j, H12, H21))
    return jobs


def warp_jobs_frame(src_kp_v, dst_kp_v, src_vis_v, dst_vis_v, pascal_class: str = "car", texture_planes=None):
    """`warp_jobs` for every vehicle of a frame with ALL homographies fitted in one vectorised call
    (`find_homography_batch`): -> list (per vehicle) of lists of (source plane i, destination slot j, H12, H21)."""
    keys = list((texture_planes or pascal_texture_planes)[pascal_class].keys())
    sym = [keys.index("left"), keys.index("right")]
    want, pairs = [], []
    for v in range(len(src_kp_v)):
        sv, dv = src_vis_v[v], dst_vis_v[v]
        for i in range(len(keys)):
            if not sv[i]:
                continue
            if i not in sym and not dv[i]:
                continue
            if i in sym and 1 not in [dv[j] for j in sym]:
                continue
            j = i
            if i in sym and not dv[i]:
                j = sym[0] if i == sym[1] else sym[1]
            want.append((v, i, j))
            pairs.append((src_kp_v[v][i], dst_kp_v[v][j]))
            pairs.append((dst_kp_v[v][j], src_kp_v[v][i]))
    Hs = find_homography_batch(pairs)
    jobs = [[] for _ in range(len(src_kp_v))]
    for k, (v, i, j) in enumerate(want):
        H12, H21 = Hs[2 * k], Hs[2 * k + 1]
        if H12 is not None and H21 is not None:
            jobs[v].append((i, j, H12, H21))
    return jobs


def warp_planes_batch(src_planes: torch.Tensor, jobs_per_vehicle) -> torch.Tensor:
    """`planes_warped` of warp_unwarp_planes for every vehicle of a frame in ONE launch: src_planes CUDA uint8
    [V, P, H, W, 3], jobs_per_vehicle[v] = warp_jobs(...) of vehicle v -> [V, P, H, W, 3] (zeros where nothing is warped)."""
    V, P, H, W, _ = src_planes.shape
    flat = src_planes.reshape(V * P, H, W, 3)
    warped = torch.zeros_like(flat)
    minv_d, index, n = _job_tables(jobs_per_vehicle, P, _stack_starts([(1, V)], [0], P), flat.device)
    if n:                                                         # every job reads its plane and writes its slot in place
        flat = flat.contiguous()
        with torch.cuda.device(flat.device):
            L.check(L.lib().fusg_warp_perspective_indexed_u8(C.byref(_u8desc(flat)), minv_d.data_ptr(), index.data_ptr(), n,
                                                             C.byref(_u8desc(warped)), ops.stream_ptr()), "warp_perspective_indexed_u8")
    return warped.view(V, P, H, W, 3)


def _stack_starts(shape, offs, P: int) -> List[int]:
    """Row -> first source image of the row's plane stack.  Rows are clip-major and frame-major inside a clip (clip c of
    shape[c] = (F, V) starts at row offs[c]); every frame of a clip reads the clip's own V stacks of P planes, which start at
    image offs[c] * P.  A clip's tail is the one clip [(F, V)], a frame's vehicles the one frame [(1, V)]."""
    return [(offs[c] + k % V) * P for c, (F, V) in enumerate(shape) for k in range(F * V)]


def _job_table_host(jobs_per_row, P: int, src_first: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """The ONE job table of the three `warp_planes_*_batch` forms, on the host: jobs_per_row[r] = warp_jobs(...) of row r, whose
    destination stack starts at image r * P and whose source stack at image src_first[r] - the forms differ only in that mapping.
    In a row a later job on slot j overwrites an earlier one (plane order): the last job per slot is kept, slots in the order they
    were first written.  -> (minv float64 [n, 9]: inverses of the kept H12s, index int32 [n, 2]: (source, destination) image)."""
    idx, Hs = [], []
    for r, jobs in enumerate(jobs_per_row):
        last = {}
        for i, j, H12, _ in jobs:
            last[j] = (i, H12)
        for j, (i, H12) in last.items():
            idx.append((src_first[r] + i, r * P + j))
            Hs.append(H12)
    n = len(Hs)
    minv = np.linalg.inv(np.asarray(Hs, dtype=np.float64).reshape(n, 3, 3)).reshape(n, 9)      # LAPACK getrf/getri per matrix, as one call
    return minv, np.asarray(idx, dtype=np.int32).reshape(n, 2)


def _job_tables(jobs_per_row, P: int, src_first: Sequence[int], device):
    """`_job_table_host` uploaded: (minv_d, index, n_jobs), or (None, None, 0) when no row has a job."""
    minv, index = _job_table_host(jobs_per_row, P, src_first)
    if not len(index):
        return None, None, 0
    return ops.h2d(minv, device), ops.h2d(index, device), len(index)


# ---------------------------------------------------------------------------------------------- device homographies
def find_homography_host(src_points, dst_points) -> Optional[np.ndarray]:
    """`find_homography` computed by libfusg's host twin of the device solver (csrc/homography.h run on the CPU: the same
    normalised DLT, through a cyclic Jacobi eigen-decomposition instead of LAPACK's, and the same Levenberg-Marquardt loop).
    None where the twin reports the fit invalid.  Needs no GPU."""
    s = np.ascontiguousarray(np.asarray(src_points, dtype=np.float64).reshape(-1, 2))
    d = np.ascontiguousarray(np.asarray(dst_points, dtype=np.float64).reshape(-1, 2))
    if len(s) != len(d):
        return None
    H = np.zeros(9)
    ok = L.lib().fusg_find_homography_host(s.ctypes.data, d.ctypes.data, len(s), H.ctypes.data, None)
    return H.reshape(3, 3) if ok else None


def pack_plane_points(kp_v, P: int) -> Tuple[np.ndarray, np.ndarray]:
    """Per-vehicle lists of P corner-point arrays [n_p, 2] -> (int32 [V, P, MAX_VERTS, 2] zero-padded, int32 [V, P] counts)."""
    V = len(kp_v)
    pts = np.zeros((V, P, MAX_VERTS, 2), dtype=np.int32)
    nv = np.zeros((V, P), dtype=np.int32)
    for v in range(V):
        if len(kp_v[v]) != P:
            raise ValueError(f"vehicle {v}: {len(kp_v[v])} planes, expected {P}")
        for i in range(P):
            a = np.asarray(kp_v[v][i])
            if a.ndim != 2 or a.shape[1] != 2 or len(a) > MAX_VERTS or not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"vehicle {v} plane {i}: corner points must be integers [n <= {MAX_VERTS}, 2] (plane_polygons)")
            pts[v, i, :len(a)] = a
            nv[v, i] = len(a)
    return pts, nv


def _sym_planes(pascal_class: str = "car", texture_planes=None) -> Tuple[int, int, int]:
    keys = list((texture_planes or pascal_texture_planes)[pascal_class].keys())
    return len(keys), keys.index("left"), keys.index("right")


def plane_homographies_device(src_kp, dst_kp, src_vis, dst_vis, device=None, pascal_class: str = "car", texture_planes=None,
                              nverts=None, return_matrices: bool = False):
    """`warp_jobs_frame` + the inversion and slot rule of `warp_planes_batch` on the device (fusg_plane_homographies): the
    gate, both fits per plane and the inverse of H12 for every vehicle of a frame in one launch, nothing read back.

    src_kp / dst_kp: the host lists a scene carries ([V][P] of int32 [n, 2], `plane_polygons`; every vehicle has the same
    point count per plane) with src_vis / dst_vis host [V, P] - packed into ONE pinned upload -, or CUDA tensors already in
    the padded layout: int32 [V, P, 8, 2], uint8 [V, P], and `nverts` int32 [P].
    Returns (minv float64 [V * P, 9], index int32 [V * P, 2]): the tables `warp_planes_fitted` consumes; index[r, 0] = -1
    where slot r receives no plane.  return_matrices=True adds H float64 [V, P, 2, 3, 3] (H12, H21 of the slot's job) and
    status int32 [V, P] (0 nothing gated onto the slot, 1 job, 2 gated but the fit is invalid)."""
    P, sa, sb = _sym_planes(pascal_class, texture_planes)
    if isinstance(src_kp, torch.Tensor):
        sp, dp, sv, dv, nv = src_kp, dst_kp, src_vis, dst_vis, nverts
        dev = sp.device
        V = int(sp.shape[0])
        ok = all(isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.device == dev for t in (sp, dp, sv, dv, nv))
        if not ok or sp.dtype != torch.int32 or dp.dtype != torch.int32 or nv.dtype != torch.int32 or sv.dtype != torch.uint8 or \
                dv.dtype != torch.uint8 or tuple(sp.shape) != (V, P, MAX_VERTS, 2) or tuple(dp.shape) != (V, P, MAX_VERTS, 2) or \
                tuple(sv.shape) != (V, P) or tuple(dv.shape) != (V, P) or tuple(nv.shape) != (P,):
            raise ValueError("plane_homographies_device: device inputs are contiguous int32 [V, P, 8, 2] points, uint8 [V, P] "
                             "visibilities and int32 [P] nverts on one device")
    else:
        dev = _device(device)
        V = len(src_kp)
        spn, nvs = pack_plane_points(src_kp, P)
        dpn, nvd = pack_plane_points(dst_kp, P)
        nvn = nvs[0] if V else np.zeros(P, np.int32)
        if V and not ((nvs == nvn).all() and (nvd == nvn).all()):
            raise ValueError("plane_homographies_device: every vehicle must have the same number of corner points per plane")
        svn = (np.asarray(src_vis).reshape(V, P) != 0).astype(np.uint8)
        dvn = (np.asarray(dst_vis).reshape(V, P) != 0).astype(np.uint8)
        # one upload: [points src | points dst | nverts] as int32, then the visibility bytes (a multiple of 4 before them)
        words = np.concatenate([spn.reshape(-1), dpn.reshape(-1), nvn.reshape(-1)])
        blob = ops.h2d(np.concatenate([words.view(np.uint8), svn.reshape(-1), dvn.reshape(-1)]), dev)
        n_pts, n_vis = V * P * MAX_VERTS * 2, V * P
        iw = blob[:4 * words.size].view(torch.int32)
        sp, dp, nv = iw[:n_pts], iw[n_pts:2 * n_pts], iw[2 * n_pts:]
        sv, dv = blob[4 * words.size:4 * words.size + n_vis], blob[4 * words.size + n_vis:]
    minv = torch.empty((V * P, 9), dtype=torch.float64, device=dev)
    index = torch.empty((V * P, 2), dtype=torch.int32, device=dev)
    Hm = torch.empty((V, P, 2, 3, 3), dtype=torch.float64, device=dev) if return_matrices else None
    st = torch.empty((V, P), dtype=torch.int32, device=dev) if return_matrices else None
    with torch.cuda.device(dev):
        L.check(L.lib().fusg_plane_homographies(sp.data_ptr(), dp.data_ptr(), nv.data_ptr(), sv.data_ptr(), dv.data_ptr(), V, P, sa, sb,
                                                minv.data_ptr(), index.data_ptr(), Hm.data_ptr() if return_matrices else None,
                                                st.data_ptr() if return_matrices else None, ops.stream_ptr()), "plane_homographies")
    return (minv, index, Hm, st) if return_matrices else (minv, index)


def plane_homographies_host(src_kp, dst_kp, src_vis, dst_vis, pascal_class: str = "car", texture_planes=None):
    """The tables of `plane_homographies_device` computed on the CPU by the same code (fusg_plane_homographies_host): numpy
    (minv [V * P, 9], index [V * P, 2], H [V, P, 2, 3, 3], status [V, P]).  Needs no GPU; the device's tables equal these bit
    for bit."""
    P, sa, sb = _sym_planes(pascal_class, texture_planes)
    V = len(src_kp)
    sp, nvs = pack_plane_points(src_kp, P)
    dp, nvd = pack_plane_points(dst_kp, P)
    nv = np.ascontiguousarray(nvs[0]) if V else np.zeros(P, np.int32)
    if V and not ((nvs == nv).all() and (nvd == nv).all()):
        raise ValueError("plane_homographies_host: every vehicle must have the same number of corner points per plane")
    sv = np.ascontiguousarray((np.asarray(src_vis).reshape(V, P) != 0).astype(np.uint8))
    dv = np.ascontiguousarray((np.asarray(dst_vis).reshape(V, P) != 0).astype(np.uint8))
    minv, index = np.zeros((V * P, 9)), np.zeros((V * P, 2), np.int32)
    Hm, st = np.zeros((V, P, 2, 3, 3)), np.zeros((V, P), np.int32)
    L.check(L.lib().fusg_plane_homographies_host(sp.ctypes.data, dp.ctypes.data, nv.ctypes.data, sv.ctypes.data, dv.ctypes.data, V, P,
                                                 sa, sb, minv.ctypes.data, index.ctypes.data, Hm.ctypes.data, st.ctypes.data),
            "plane_homographies_host")
    return minv, index, Hm, st


def warp_planes_fitted(src_planes: torch.Tensor, minv: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """`warp_planes_batch` from the device tables of `plane_homographies_device`: src_planes CUDA uint8 [V, P, H, W, 3] ->
    [V, P, H, W, 3], zeros where nothing is warped.  One launch over the V * P rows; a row without a job writes nothing."""
    V, P, H, W, _ = src_planes.shape
    if minv.dtype != torch.float64 or index.dtype != torch.int32 or tuple(minv.shape) != (V * P, 9) or \
            tuple(index.shape) != (V * P, 2) or not (minv.is_contiguous() and index.is_contiguous()):
        raise ValueError("warp_planes_fitted: minv float64 [V * P, 9] and index int32 [V * P, 2], contiguous")
    flat = src_planes.reshape(V * P, H, W, 3).contiguous()
    warped = torch.zeros_like(flat)
    if V:
        with torch.cuda.device(flat.device):
            L.check(L.lib().fusg_warp_perspective_indexed_u8(C.byref(_u8desc(flat)), minv.data_ptr(), index.data_ptr(), V * P,
                                                             C.byref(_u8desc(warped)), ops.stream_ptr()), "warp_perspective_indexed_u8")
    return warped.view(V, P, H, W, 3)


def _warp_frames(flat: torch.Tensor, minv: torch.Tensor, index: torch.Tensor, jobs: int, frames: int) -> torch.Tensor:
    """fusg_warp_perspective_frames_u8: `jobs` rows of (minv, index) warp the S shared images of `flat` into frames * S zeroed ones."""
    S, H, W, _ = flat.shape
    warped = torch.zeros((frames * S, H, W, 3), dtype=torch.uint8, device=flat.device)
    if jobs:
        with torch.cuda.device(flat.device):
            L.check(L.lib().fusg_warp_perspective_frames_u8(C.byref(_u8desc(flat)), minv.data_ptr(), index.data_ptr(), int(jobs), int(frames),
                                                            C.byref(_u8desc(warped)), ops.stream_ptr()), "warp_perspective_frames_u8")
    return warped


def warp_planes_frames_batch(src_planes: torch.Tensor, jobs_per_row, frames: int) -> torch.Tensor:
    """`warp_planes_batch` for the F future frames of a clip in ONE launch, from ONE copy of the first frame's planes:
    src_planes CUDA uint8 [V, P, H, W, 3], jobs_per_row[f * V + v] = warp_jobs(...) of vehicle v in frame f (frame-major, F * V
    entries) -> [F * V, P, H, W, 3], zeros where nothing is warped."""
    V, P, H, W, _ = src_planes.shape
    if frames < 1 or len(jobs_per_row) != frames * V:
        raise ValueError(f"warp_planes_frames_batch: {len(jobs_per_row)} job lists for {frames} frames of {V} vehicles")
    flat = src_planes.reshape(V * P, H, W, 3).contiguous()
    minv_d, index, n = _job_tables(jobs_per_row, P, _stack_starts([(frames, V)], [0], P), flat.device)
    return _warp_frames(flat, minv_d, index, n, frames).view(frames * V, P, H, W, 3)


def warp_planes_frames_fitted(src_planes: torch.Tensor, minv: torch.Tensor, index: torch.Tensor, frames: int) -> torch.Tensor:
    """`warp_planes_fitted` for F frames from ONE copy of the first frame's planes: minv / index are the tables
    `plane_homographies_device` fits for the F * V (frame, vehicle) rows (the source corner points repeated per frame), whose
    source entries (row * P + i) the kernel folds back onto the V * P shared planes.  -> [F * V, P, H, W, 3]."""
    V, P, H, W, _ = src_planes.shape
    n = frames * V * P
    if frames < 1 or minv.dtype != torch.float64 or index.dtype != torch.int32 or tuple(minv.shape) != (n, 9) or \
            tuple(index.shape) != (n, 2) or not (minv.is_contiguous() and index.is_contiguous()):
        raise ValueError("warp_planes_frames_fitted: minv float64 [F * V * P, 9] and index int32 [F * V * P, 2], contiguous")
    flat = src_planes.reshape(V * P, H, W, 3).contiguous()
    return _warp_frames(flat, minv, index, n if V else 0, frames).view(frames * V, P, H, W, 3)


def _clips_layout(what: str, src_planes_per_clip, frames_per_clip):
    """What the several-clip warps check before any launch: (the clips' planes, [(F_c, V_c)], row offsets, P, H, W)."""
    planes, frames = list(src_planes_per_clip), [int(f) for f in frames_per_clip]
    if not 1 <= len(planes) <= L.MAX_FRAMES or len(frames) != len(planes):
        raise ValueError(f"{what}: {len(planes)} clips with {len(frames)} frame counts (1..{L.MAX_FRAMES} clips per launch, one count each)")
    first = planes[0]
    if not isinstance(first, torch.Tensor) or first.dim() != 5:
        raise ValueError(f"{what}: a clip's source planes are a CUDA uint8 tensor [V, P, H, W, 3]")
    P, H, W = (int(x) for x in first.shape[1:4])
    offs = [0]
    for c, (t, f) in enumerate(zip(planes, frames)):
        if not isinstance(t, torch.Tensor) or t.dim() != 5 or t.dtype != torch.uint8 or t.device != first.device or \
                tuple(t.shape[1:]) != (P, H, W, 3):
            raise ValueError(f"{what}: clip {c}'s source planes are {tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', None)}, "
                             f"expected uint8 [V, {P}, {H}, {W}, 3] on {first.device}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: clip {c}'s source planes are not contiguous (they are passed by pointer, not copied)")
        if f < 0:
            raise ValueError(f"{what}: clip {c} has {f} frames")
        offs.append(offs[-1] + f * int(t.shape[0]))
    return planes, [(f, int(t.shape[0])) for t, f in zip(planes, frames)], offs, P, H, W


def _warp_clips(planes, shape, offs, P: int, H: int, W: int, minv, index, jobs: int) -> torch.Tensor:
    """fusg_warp_perspective_clips_u8: `jobs` rows of (minv, index) warp each clip's own planes into its rows of offs[-1] * P zeroed images."""
    n = len(planes)
    warped = torch.zeros((offs[-1] * P, H, W, 3), dtype=torch.uint8, device=planes[0].device)
    if jobs:
        srcs = (C.c_void_p * n)(*[t.data_ptr() if t.shape[0] else None for t in planes])
        images = (C.c_int32 * n)(*[V * P for _, V in shape])
        first = (C.c_int32 * (n + 1))(*[o * P for o in offs])
        with torch.cuda.device(warped.device):
            L.check(L.lib().fusg_warp_perspective_clips_u8(srcs, images, first, n, H, W, minv.data_ptr(), index.data_ptr(), int(jobs),
                                                           C.byref(_u8desc(warped)), ops.stream_ptr()), "warp_perspective_clips_u8")
    return warped.view(offs[-1], P, H, W, 3)


def warp_planes_clips_batch(src_planes_per_clip, frames_per_clip, jobs_per_row) -> torch.Tensor:
    """`warp_planes_frames_batch` for the future frames of SEVERAL clips in ONE launch, every clip's planes passed by pointer
    (no copy of them is made): src_planes_per_clip[c] CUDA uint8 [V_c, P, H, W, 3] (contiguous), frames_per_clip[c] = F_c,
    jobs_per_row[r] = warp_jobs(...) of row r - clip-major, frame-major inside a clip: r = offs[c] + f * V_c + v
    -> [sum(F_c * V_c), P, H, W, 3], zeros where nothing is warped."""
    planes, shape, offs, P, H, W = _clips_layout("warp_planes_clips_batch", src_planes_per_clip, frames_per_clip)
    if len(jobs_per_row) != offs[-1]:
        raise ValueError(f"warp_planes_clips_batch: {len(jobs_per_row)} job lists for {offs[-1]} rows ((frames, vehicles) per clip: {shape})")
    minv_d, index, n = _job_tables(jobs_per_row, P, _stack_starts(shape, offs, P), planes[0].device)
    return _warp_clips(planes, shape, offs, P, H, W, minv_d, index, n)


def warp_planes_clips_fitted(src_planes_per_clip, frames_per_clip, minv: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """`warp_planes_frames_fitted` for the future frames of SEVERAL clips in ONE launch, every clip's planes passed by pointer:
    minv / index are the tables `plane_homographies_device` fits for all rows of the call (clip-major, frame-major inside a
    clip; the source corner points of a clip repeated per frame), whose source entries (row * P + i) the kernel folds back onto
    the row's own clip's V_c * P planes.  -> [sum(F_c * V_c), P, H, W, 3]."""
    planes, shape, offs, P, H, W = _clips_layout("warp_planes_clips_fitted", src_planes_per_clip, frames_per_clip)
    n = offs[-1] * P
    if not (isinstance(minv, torch.Tensor) and isinstance(index, torch.Tensor)) or minv.dtype != torch.float64 or \
            index.dtype != torch.int32 or tuple(minv.shape) != (n, 9) or tuple(index.shape) != (n, 2) or \
            not (minv.is_contiguous() and index.is_contiguous()) or minv.device != planes[0].device or index.device != planes[0].device:
        raise ValueError(f"warp_planes_clips_fitted: minv float64 [{n}, 9] and index int32 [{n}, 2], contiguous, on the planes' device")
    return _warp_clips(planes, shape, offs, P, H, W, minv, index, n)


def warp_unwarp_planes(src_planes: Image, src_planes_kpoints: List[np.ndarray], dst_planes_kpoints: List[np.ndarray],
                       src_visibilities, dst_visibilities, pascal_class: str, pascal_texture_planes=pascal_texture_planes,
                       unwarp: bool = True):
    """Reference signature (planes_utils.py:40-82): visibility / symmetry gating and the homography fits on the host,
    both warps of all selected planes in two batched launches.  `unwarp=False` skips the second warp (its result is
    discarded by the reference's only caller, trajectory_inference.py:171) and returns None for it."""
    planes, as_np = _to_dev(src_planes)
    jobs = warp_jobs(src_planes_kpoints, dst_planes_kpoints, src_visibilities, dst_visibilities, pascal_class,
                     pascal_texture_planes)
    warped = torch.zeros_like(planes)
    unwarped = torch.zeros_like(planes) if unwarp else None
    if jobs:
        h, w = planes.shape[1:3]
        src_idx = torch.tensor([i for i, _, _, _ in jobs], device=planes.device)
        w1 = warp_perspective(planes[src_idx], [H12 for _, _, H12, _ in jobs], (w, h))
        # the reference assigns in plane order: a later job writing the same slot j overwrites an earlier one
        for k, (_, j, _, _) in enumerate(jobs):
            warped[j] = w1[k]
        if unwarp:
            w2 = warp_perspective(w1, [H21 for _, _, _, H21 in jobs], (w, h))
            for k, (i, _, _, _) in enumerate(jobs):
                unwarped[i] = w2[k]
    return _back(warped, as_np), (None if unwarped is None else _back(unwarped, as_np))


# ---------------------------------------------------------------------------------------------- W-3: ICN inputs
def icn_inputs_batch(planes: torch.Tensor, sketches: torch.Tensor, centrals: torch.Tensor, bboxes: Sequence[Sequence[int]],
                     icn_w: int = 256, icn_h: int = 256):
    """Batched, device-resident ICN input assembly: planes [B, P, H, W, 3] (BGR), sketches [B, H, W, 3] (RGB), centrals
    [B, icn_h, icn_w, 3] (RGB) CUDA uint8; bboxes: per vehicle [x_min, y_min, x_max, y_max] of its sketch mask.
    Returns (float32 [B, 3 * (P + 2), icn_h, icn_w] NHWC-physical - what G_Resnet's stem reads without a copy -,
    list of crop_info dicts)."""
    B, P, H, W, _ = planes.shape
    geom, infos = [], []
    for bb in bboxes:
        win, pb, pa = square_crop_geometry((H, W), bb)
        geom.append(_geom_row(win, pb, pa))
        infos.append({"crop_xy_min": (win[0], win[1]), "pad_xy_before": pb, "pad_xy_after": pa,
                      "crop_size_orig": (win[3] - win[1], win[2] - win[0])})
    geom_d = torch.tensor(geom, dtype=torch.int32, device=planes.device)
    out = ops.nhwc_empty(B, 3 * (P + 2), icn_h, icn_w, planes.device, zero=True)
    with torch.cuda.device(planes.device):
        L.check(L.lib().fusg_icn_inputs(C.byref(_u8desc(sketches.contiguous())), C.byref(_u8desc(centrals.contiguous())),
                                        C.byref(_u8desc(planes.reshape(B * P, H, W, 3).contiguous())), geom_d.data_ptr(),
                                        C.byref(ops.desc(out)), ops.stream_ptr()), "icn_inputs")
    return out, infos


def icn_inputs_device(planes: torch.Tensor, sketches: torch.Tensor, centrals: torch.Tensor, geom: torch.Tensor,
                      icn_w: int = 256, icn_h: int = 256, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """icn_inputs_batch with the crop geometry already on the device (frame_ops.mask_bbox_geom): nothing is read back.
    out: an earlier result's buffer to overwrite (every real channel of every pixel is written)."""
    B, P, H, W, _ = planes.shape
    if out is None:
        out = ops.nhwc_empty(B, 3 * (P + 2), icn_h, icn_w, planes.device, zero=True)
    else:
        assert tuple(out.shape) == (B, 3 * (P + 2), icn_h, icn_w) and out.dtype == torch.float32 and out.stride(1) == 1
    with torch.cuda.device(planes.device):
        L.check(L.lib().fusg_icn_inputs(C.byref(_u8desc(sketches.contiguous())), C.byref(_u8desc(centrals.contiguous())),
                                        C.byref(_u8desc(planes.reshape(B * P, H, W, 3).contiguous())), geom.data_ptr(),
                                        C.byref(ops.desc(out)), ops.stream_ptr()), "icn_inputs")
    return out


def get_icn_inputs(planes: Image, sketch_normal: Image, sketch_mask, central_crop: Image, icn_w: int, icn_h: int):
    """Reference signature (warp_learn/models.py:323-366): -> (float32 [1, 21, icn_h, icn_w] on the device, crop_info)."""
    pl, _ = _to_dev(planes)
    sk, _ = _to_dev(sketch_normal, pl.device)
    cc, _ = _to_dev(central_crop, pl.device)
    if isinstance(sketch_mask, torch.Tensor):
        ys, xs = torch.nonzero(sketch_mask, as_tuple=True)
        bbox = [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]
    else:
        ys, xs = np.nonzero(sketch_mask)
        bbox = [int(np.min(xs)), int(np.min(ys)), int(np.max(xs)), int(np.max(ys))]
    out, infos = icn_inputs_batch(pl[None], sk[None], cc[None], [bbox], icn_w, icn_h)
    return out, infos[0]


def planes_to_torch(planes: Image, to_LAB: bool) -> torch.Tensor:
    """Reference signature (planes_utils.py:85-93): uint8 [P, H, W, 3] (BGR) -> float32 [P, 3, H, W] in [-1, 1]."""
    pl, _ = _to_dev(planes)
    P, H, W, _ = pl.shape
    if not to_LAB:
        x = pl.permute(0, 3, 1, 2).to(torch.float32)
        return (x / 255.0 - 0.5) / 0.5
    # full-frame window: crop == frame, no resize; the sketch / central slots are computed and dropped
    geom = torch.tensor([[0, 0, W, H, 0, 0, 0, 0]], dtype=torch.int32, device=pl.device)
    dst = ops.nhwc_empty(1, 3 * (P + 2), H, W, pl.device, zero=True)
    with torch.cuda.device(pl.device):
        L.check(L.lib().fusg_icn_inputs(C.byref(_u8desc(pl[:1])), C.byref(_u8desc(pl[:1])), C.byref(_u8desc(pl)),
                                        geom.data_ptr(), C.byref(ops.desc(dst)), ops.stream_ptr()), "icn_inputs")
    return dst[0, 6:].reshape(P, 3, H, W)


# ---------------------------------------------------------------------------------------------- W-10 / f-2: way back
def lab2bgr(img: torch.Tensor) -> torch.Tensor:
    """``cv2.cvtColor(img, cv2.COLOR_LAB2BGR)`` on CUDA uint8 [N, H, W, 3]."""
    out = torch.empty_like(img)
    with torch.cuda.device(img.device):
        L.check(L.lib().fusg_lab2bgr_u8(C.byref(_u8desc(img)), C.byref(_u8desc(out)), ops.stream_ptr()), "lab2bgr_u8")
    return out


def to_image(x, from_LAB: bool):
    """Reference signature (planes_utils.py:96-118): [3, H, W] in [-1, 1] -> uint8 [H, W, 3] BGR, as numpy (what the
    reference returns).  `to_image_device` keeps the result on the GPU."""
    if isinstance(x, np.ndarray):                                    # the reference's "already numpy" branch: HWC in
        x = torch.from_numpy(np.ascontiguousarray(np.transpose(x, (2, 0, 1))))
        x = x.to(_device())
    assert x.dim() == 3, f"Unsupported image shape {tuple(x.shape)}"
    return to_image_device(x.detach()[None], from_LAB)[0].cpu().numpy()


def to_image_device(x: torch.Tensor, from_LAB: bool) -> torch.Tensor:
    """[B, 3, H, W] float32 in [-1, 1] (CUDA) -> uint8 [B, H, W, 3]: trunc(clip((x + 1) / 2 * 255)) [+ Lab -> BGR]."""
    u8 = ops.to_image_u8(x.to(torch.float32))
    return lab2bgr(u8) if from_LAB else u8


def paste_back_device(frame: torch.Tensor, net_images: torch.Tensor, geom: torch.Tensor, masks: torch.Tensor,
                      box_images: Optional[torch.Tensor] = None, box_geom: Optional[torch.Tensor] = None) -> torch.Tensor:
    """paste_back with device geometry rows (int32 [V, 8]) and device masks (uint8 [V, H, W]); returns a new frame tensor.
    box_images uint8 [V, h, w, 3] + box_geom int32 [V, 8] (x0, y0, x1, y1, ...): the --inpaint form - every vehicle first
    writes its inpainted box image, resized to its rectangle, then its masked network image (fusg_paste_layers_u8)."""
    fr = frame.contiguous().clone()
    V, H, W = masks.shape
    with torch.cuda.device(fr.device):
        if box_images is None:
            L.check(L.lib().fusg_paste_back_u8(C.byref(_u8desc(net_images.contiguous())), C.byref(ops.desc(masks.contiguous().view(V, 1, H, W))),
                                               geom.data_ptr(), C.byref(_u8desc(fr[None])), ops.stream_ptr()), "paste_back_u8")
        else:
            assert box_geom is not None and box_geom.dtype == torch.int32 and tuple(box_geom.shape) == (V, 8) and box_images.shape[0] == V
            L.check(L.lib().fusg_paste_layers_u8(C.byref(_u8desc(net_images.contiguous())), C.byref(ops.desc(masks.contiguous().view(V, 1, H, W))),
                                                 geom.data_ptr(), C.byref(_u8desc(box_images.contiguous())), box_geom.contiguous().data_ptr(),
                                                 C.byref(_u8desc(fr[None])), ops.stream_ptr()), "paste_layers_u8")
    return fr


def _check_paste(what: str, bases, hw, dev, net_images, geom, masks, box_images, box_geom, rows: str, bad_rows: bool, counts: str):
    """What both several-frame paste wrappers check before the launch, under the wrapper's name: the bases (uint8 [H, W, 3] on
    dev), one crop and one int32 geom row per mask (`bad_rows`: the wrapper's own condition on the masks, `counts`: its message),
    box_images paired with box_geom (`rows`: its name for the row count).  -> the contiguous bases, kept until the launch is queued."""
    N, (H, W) = int(masks.shape[0]), hw
    keep = [b.contiguous() for b in bases]
    if any(tuple(b.shape) != (H, W, 3) or b.dtype != torch.uint8 or b.device != dev for b in keep):
        raise ValueError(f"{what}: every base image is uint8 {(H, W, 3)} on {dev}")
    if bad_rows or net_images.shape[0] != N or geom.dtype != torch.int32 or tuple(geom.shape) != (N, 8):
        raise ValueError(f"{what}: {counts}")
    if (box_images is None) != (box_geom is None) or (box_images is not None and (
            box_images.shape[0] != N or box_geom.dtype != torch.int32 or tuple(box_geom.shape) != (N, 8))):
        raise ValueError(f"{what}: box_images [{rows}, h, w, 3] come with box_geom int32 [{rows}, 8]")
    return keep


def paste_back_frames_device(bases: Sequence[torch.Tensor], net_images: torch.Tensor, geom: torch.Tensor, masks: torch.Tensor,
                             box_images: Optional[torch.Tensor] = None, box_geom: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`paste_back_device` for F frames in ONE launch (fusg_paste_layers_frames_u8): bases = F CUDA uint8 [H, W, 3] images, the
    one frame f's composite starts from (read, not copied first: the kernel writes every pixel of the result); net_images
    [F * V, h, w, 3], geom int32 [F * V, 8], masks uint8 [F * V, H, W] (and box_images / box_geom) frame-major, row f * V + v =
    frame f, vehicle v.  -> uint8 [F, H, W, 3]."""
    F = len(bases)
    if F < 1:
        raise ValueError("paste_back_frames_device: at least one frame")
    N, H, W = masks.shape
    dev = masks.device
    keep = _check_paste("paste_back_frames_device", bases, (H, W), dev, net_images, geom, masks, box_images, box_geom, "F * V",
                        N % F != 0, f"{N} masks, {net_images.shape[0]} crops, geom {tuple(geom.shape)} for {F} frames")
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    table = ops.h2d(np.asarray([b.data_ptr() for b in keep], dtype=np.int64), dev)
    with torch.cuda.device(dev):
        L.check(L.lib().fusg_paste_layers_frames_u8(
            C.byref(_u8desc(net_images.contiguous())), C.byref(ops.desc(masks.contiguous().view(N, 1, H, W))), geom.contiguous().data_ptr(),
            C.byref(_u8desc(box_images.contiguous())) if box_images is not None else None,
            box_geom.contiguous().data_ptr() if box_geom is not None else None, table.data_ptr(), F, C.byref(_u8desc(out)),
            ops.stream_ptr()), "paste_layers_frames_u8")
    return out


def paste_back_ragged_device(bases: Sequence[torch.Tensor], frame_rows: Sequence[int], net_images: torch.Tensor, geom: torch.Tensor,
                             masks: torch.Tensor, box_images: Optional[torch.Tensor] = None,
                             box_geom: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`paste_back_frames_device` with another number of layers per frame (fusg_paste_layers_ragged_u8): frame f's layers are rows
    [frame_rows[f], frame_rows[f + 1]) of net_images [rows, h, w, 3], geom int32 [rows, 8], masks uint8 [rows, H, W] (and
    box_images / box_geom), in row order; frame_rows = F + 1 host offsets from 0 to rows.  A frame without layers is a copy of its
    base; the bases are read, never written.  At most L.MAX_FRAMES frames per launch.  -> uint8 [F, H, W, 3]."""
    F = len(bases)
    if F < 1 or F > L.MAX_FRAMES:
        raise ValueError(f"paste_back_ragged_device: {F} frames (1..{L.MAX_FRAMES} per launch)")
    H, W = int(bases[0].shape[0]), int(bases[0].shape[1])
    dev = bases[0].device
    N = int(masks.shape[0])
    offs = [int(r) for r in frame_rows]
    if len(offs) != F + 1:
        raise ValueError(f"paste_back_ragged_device: {len(offs)} row offsets for {F} frames (one more than frames)")
    keep = _check_paste("paste_back_ragged_device", bases, (H, W), dev, net_images, geom, masks, box_images, box_geom, "rows",
                        tuple(masks.shape[1:]) != (H, W),
                        f"masks {tuple(masks.shape)}, {net_images.shape[0]} crops, geom {tuple(geom.shape)} for frames of {(H, W)}")
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    ptrs = (C.c_void_p * F)(*[b.data_ptr() for b in keep])
    with torch.cuda.device(dev):
        L.check(L.lib().fusg_paste_layers_ragged_u8(
            C.byref(_u8desc(net_images.contiguous())), C.byref(ops.desc(masks.contiguous().view(N, 1, H, W))), geom.contiguous().data_ptr(),
            C.byref(_u8desc(box_images.contiguous())) if box_images is not None else None,
            box_geom.contiguous().data_ptr() if box_geom is not None else None, ptrs, (C.c_int32 * (F + 1))(*offs), F,
            C.byref(_u8desc(out)), ops.stream_ptr()), "paste_layers_ragged_u8")
    return out


def paste_back(frame: Image, net_images: torch.Tensor, crop_infos: Sequence[dict], paste_masks: Image) -> Image:
    """The "revert and stitch" of trajectory_inference.py:184-198 for V vehicles in one launch: net_images [V, h, w, 3]
    uint8 (CUDA), their crop_infos (from get_icn_inputs) and paste masks [V, H, W] (bool / uint8; the reference's
    `dst_sketch_mask`); later vehicles overwrite earlier ones, exactly as the reference's loop does.  Returns the
    updated frame (a new array / tensor)."""
    fr, as_np = _to_dev(frame, net_images.device)
    fr = fr.clone()
    if isinstance(paste_masks, np.ndarray):
        masks = torch.from_numpy(np.ascontiguousarray(paste_masks.astype(np.uint8))).to(fr.device)
    else:
        masks = paste_masks.to(torch.uint8).contiguous()
    geom = []
    for ci in crop_infos:
        (x0, y0), pb, pa = ci["crop_xy_min"], ci["pad_xy_before"], ci["pad_xy_after"]
        hh, ww = ci["crop_size_orig"]
        geom.append([x0, y0, x0 + ww, y0 + hh, pb[0], pb[1], pa[0], pa[1]])
    geom_d = torch.tensor(geom, dtype=torch.int32, device=fr.device)
    V, H, W = masks.shape
    with torch.cuda.device(fr.device):
        L.check(L.lib().fusg_paste_back_u8(C.byref(_u8desc(net_images.contiguous())), C.byref(ops.desc(masks.view(V, 1, H, W))),
                                           geom_d.data_ptr(), C.byref(_u8desc(fr[None])), ops.stream_ptr()), "paste_back_u8")
    return _back(fr, as_np)
