"""Per-vehicle geometry on the MI355X: the posed CAD model rendered into a normal-colour sketch and its mask, the plane
visibilities and the plane corner points - what the reference computes between the pose fit and the plane warp
(warp_learn/vehicle_utils.py:12-32) with an Open3D window per vehicle and frame (warp_learn/render_open3d.py:29-49) and
OpenCV polygon fills (warp_learn/online_visibility.py:105-150).  The image work runs in ``csrc/render.hip``
(``fusg_render_normals_u8``, ``fusg_plane_visibility``); the host keeps what is a few numbers per vehicle (the pose ->
extrinsic, the 3-D keypoint projections, the plane distances).

Conventions (each restated from the reference line given):
  - vertices are scaled x5 at load (run_test.py:148-151), the 3-D keypoints too, in float32 (trajectory_inference.py:87-90);
  - the mesh moves as a row vector, p = v @ z_rot(theta) + tr (trajectory_inference.py:363), the camera is E[:3, :3] p + E[:3, 3];
  - the render uses Open3D's default principal point (W/2 - 0.5, H/2 - 0.5), not K's cx, cy ("this must be left as they
    are", render_open3d.py:20); the keypoint projections use K.  The mismatch is the reference's and is kept;
  - vertex normals as Open3D's compute_vertex_normals: unnormalised face cross products summed per vertex, then normalised;
    computed once per bank mesh in float64 and rotated per job by z_rot(theta); colour (n + 1) / 2 -> round(255 c);
  - a plane is visible when its uncovered area is more than 0.9 of its area (online_visibility.py:145-148), in float64;
    camera position = inv(E)[:3, 3], plane distance = |camera - mean of the plane's 3-D keypoints| (:58-72).
Parity with Open3D / OpenCV themselves is unpinned (neither is a dependency); tests pin the kernels to a numpy
restatement of these conventions (tests/render_ref.py).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ops
from .warp_learn import planes_utils as pu

KP_NAMES = ("left_back_trunk", "left_back_wheel", "left_front_light", "left_front_wheel", "right_back_trunk", "right_back_wheel",
            "right_front_light", "right_front_wheel", "upper_left_rearwindow", "upper_left_windshield", "upper_right_rearwindow",
            "upper_right_windshield")                                # utils/keypoint_utils.py:9-13 (_KP_NAMES)
# compute_visibility's planes: the five texture planes plus the two it adds for occlusion only (online_visibility.py:107-113)
VIS_PLANES = dict(pu.CAR_TEXTURE_PLANES,
                  front_bt=["left_front_light", "right_front_light", "right_front_wheel", "left_front_wheel"],
                  back_bt=["left_back_trunk", "right_back_trunk", "right_back_wheel", "left_back_wheel"])
TEXTURE_PLANES = tuple(pu.CAR_TEXTURE_PLANES.keys())
SCALE = 5.0                                                          # _____SCALE_F (run_test.py:148)
NEAR_Z = 1e-3                                                        # csrc/render.hip: triangles with a vertex nearer are dropped
JOB_DTYPE = np.dtype([("R", "<f8", 9), ("tr", "<f8", 3), ("E", "<f8", 12), ("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"),
                      ("cy", "<f8"), ("v_off", "<i4"), ("nv", "<i4"), ("t_off", "<i4"), ("nt", "<i4")])   # fusg_render_job


def z_rot(alpha: float) -> np.ndarray:
    """utils/geometry.py:80-110 (counter-clockwise rotation about Z, numpy form)."""
    cz, sz = np.cos(alpha), np.sin(alpha)
    return np.asarray([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])


def vertex_normals(vertices: np.ndarray, triangles: np.ndarray) -> np.ndarray:
    """Open3D's TriangleMesh.compute_vertex_normals in float64: per face the unnormalised cross product
    (v1 - v0) x (v2 - v0), summed onto its three vertices in face order, then normalised (a zero sum stays zero)."""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)
    fn = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, t[:, k], fn)
    norm = np.sqrt((n * n).sum(1, keepdims=True))
    return np.where(norm > 0, n / np.where(norm > 0, norm, 1.0), n)


# ---------------------------------------------------------------------------------------------- PLY
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """vertices float64 [n, 3] (x, y, z) and triangles int64 [m, 3] (face vertex_indices) of an ascii or
    binary_little_endian PLY file - what o3d.io.read_triangle_mesh gives the reference (utils/cad_utils.py:24).  Faces
    of more than three vertices are fanned (0, i, i + 1).  Other properties are read past and ignored."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data[data.index(b"\n", end) + 1:]
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property" and elements:
            if w[1] == "list":
                elements[-1][2].append((w[4], "list", _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]))
            else:
                elements[-1][2].append((w[2], _PLY_TYPES[w[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} not supported (ascii, binary_little_endian)")
    verts, faces = None, []
    if fmt == "ascii":
        toks = body.split()
        pos = 0
        for name, count, props in elements:
            rows = []
            for _ in range(count):
                row = {}
                for p in props:
                    if p[1] == "list":
                        n = int(toks[pos]); pos += 1
                        row[p[0]] = [int(x) for x in toks[pos:pos + n]]; pos += n
                    else:
                        row[p[0]] = float(toks[pos]); pos += 1
                rows.append(row)
            if name == "vertex":
                verts = np.array([[r["x"], r["y"], r["z"]] for r in rows], np.float64).reshape(-1, 3)
            elif name == "face":
                faces = [r.get("vertex_indices", r.get("vertex_index", [])) for r in rows]
    else:
        pos = 0
        for name, count, props in elements:
            if all(p[1] != "list" for p in props):
                dt = np.dtype([(p[0], "<" + p[1]) for p in props])
                arr = np.frombuffer(body, dt, count, pos)
                pos += count * dt.itemsize
                if name == "vertex":
                    verts = np.stack([arr["x"], arr["y"], arr["z"]], 1).astype(np.float64)
                continue
            rows = []
            for _ in range(count):
                row = {}
                for p in props:
                    if p[1] == "list":
                        ct, it = np.dtype("<" + p[2]), np.dtype("<" + p[3])
                        n = int(np.frombuffer(body, ct, 1, pos)[0]); pos += ct.itemsize
                        row[p[0]] = np.frombuffer(body, it, n, pos).astype(np.int64).tolist(); pos += n * it.itemsize
                    else:
                        dt = np.dtype("<" + p[1])
                        row[p[0]] = np.frombuffer(body, dt, 1, pos)[0]; pos += dt.itemsize
                rows.append(row)
            if name == "face":
                faces = [r.get("vertex_indices", r.get("vertex_index", [])) for r in rows]
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    tris = [(f[0], f[i], f[i + 1]) for f in faces for i in range(1, len(f) - 1)]
    return verts, np.array(tris, np.int64).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------- CAD bank
class CadBank:
    """The CAD models of a run (run_test.py:146-151): per model the vertices (x5), triangles, unit vertex normals of the
    unmoved mesh and the 12 3-D keypoints (x5, float32, in KP_NAMES order).  Uploaded once per device (`device_arrays`)."""

    def __init__(self, meshes: Sequence[Tuple[np.ndarray, np.ndarray, object]], scale: float = SCALE):
        """meshes: (vertices [n, 3], triangles [m, 3], kp3d) per model, in the file's units; kp3d a dict name -> xyz (the
        yaml's kpoints_3d) or an array [12, 3] in KP_NAMES order.  Triangle indices are checked here."""
        self.vertices, self.triangles, self.normals, kps = [], [], [], []
        for i, (v, t, kp) in enumerate(meshes):
            v = np.asarray(v, np.float64).reshape(-1, 3) * scale
            t = np.asarray(t).reshape(-1, 3)
            if len(v) == 0 or len(t) == 0:
                raise ValueError(f"CadBank: model {i} has no vertices or no triangles")
            if t.min() < 0 or t.max() >= len(v):
                raise ValueError(f"CadBank: model {i} has a triangle index outside [0, {len(v)})")
            if isinstance(kp, dict):
                kp = [kp[n] for n in KP_NAMES]
            kp = np.asarray(kp, np.float32).reshape(len(KP_NAMES), 3)
            self.vertices.append(np.ascontiguousarray(v))
            self.triangles.append(np.ascontiguousarray(t, dtype=np.int32))
            self.normals.append(vertex_normals(v, t))
            kps.append(kp * np.float32(scale))                      # float32 arithmetic, as trajectory_inference.py:87-90
        self.kp3d = np.stack(kps)                                   # float32 [M, 12, 3]
        self.v_off = np.cumsum([0] + [len(v) for v in self.vertices])
        self.t_off = np.cumsum([0] + [len(t) for t in self.triangles])
        self._dev: Dict[torch.device, Dict[str, torch.Tensor]] = {}

    @classmethod
    def from_files(cls, cad_root: str, indices: Sequence[int] = range(10), pascal_class: str = "car") -> "CadBank":
        """The reference's file layout (utils/cad_utils.py:8-24): pascal_<class>_cad_NNN.ply with pascal_<class>_cad_NNN.yaml
        holding 'kpoints_3d'."""
        import yaml
        meshes = []
        for i in indices:
            stem = os.path.join(str(cad_root), f"pascal_{pascal_class}_cad_{i:03d}")
            v, t = read_ply(stem + ".ply")
            with open(stem + ".yaml") as f:
                kp = yaml.safe_load(f)["kpoints_3d"]
            meshes.append((v, t, kp))
        return cls(meshes)

    def __len__(self) -> int:
        return len(self.vertices)

    def device_arrays(self, device) -> Dict[str, torch.Tensor]:
        dev = torch.device(device)
        if dev not in self._dev:
            # C order: the kernels index rows of 3 (np.concatenate keeps the Fortran order of an F-ordered input)
            self._dev[dev] = {k: torch.from_numpy(np.ascontiguousarray(np.concatenate(a))).to(dev)
                              for k, a in (("verts", self.vertices), ("normals", self.normals), ("tris", self.triangles))}
            # the tables fusg_pose_geometry looks a vehicle's model up in
            self._dev[dev].update(kp3d=torch.from_numpy(np.ascontiguousarray(self.kp3d, dtype=np.float32)).to(dev),
                                  v_off=torch.from_numpy(self.v_off.astype(np.int32)).to(dev),
                                  t_off=torch.from_numpy(self.t_off.astype(np.int32)).to(dev))
        return self._dev[dev]

    @property
    def max_nv(self) -> int:
        """The largest vertex count of a model: sizes the render's workspace without reading a job back."""
        return int(np.diff(self.v_off).max())


def extrinsic_from_pose(rvec, tvec) -> np.ndarray:
    """utils/geometry.py:203-220: 4x4 [R(rvec) | tvec] in the vectors' dtype (float32 after select_and_flip)."""
    from .utils.pnp_utils import rodrigues
    r = np.asarray(rvec).reshape(3)
    E = np.eye(4, dtype=r.dtype)
    E[:3, :3] = rodrigues(r)
    E[:3, 3] = np.asarray(tvec).reshape(3)
    return E


def render_jobs(bank: CadBank, mesh_idx: Sequence[int], E: Sequence[np.ndarray], fx: float, fy: float, frame_hw: Tuple[int, int],
                R: Optional[Sequence[np.ndarray]] = None, tr: Optional[Sequence[np.ndarray]] = None) -> np.ndarray:
    """fusg_render_job records (host); R / tr default to the unmoved mesh; principal point = Open3D's default."""
    H, W = frame_hw
    J = len(mesh_idx)
    jobs = np.zeros(J, JOB_DTYPE)
    if J == 0:
        return jobs
    m = np.asarray(mesh_idx, np.int64).reshape(J)
    bad = (m < 0) | (m >= len(bank))
    if bad.any():
        raise IndexError(f"render: mesh {int(m[bad][0])} not in a bank of {len(bank)}")
    jobs["R"] = np.broadcast_to(np.eye(3).reshape(9), (J, 9)) if R is None else np.asarray(R, np.float64).reshape(J, 9)
    jobs["tr"] = 0.0 if tr is None else np.asarray(tr, np.float64).reshape(J, 3)
    jobs["E"] = np.asarray(E, np.float64).reshape(J, -1, 4)[:, :3, :4].reshape(J, 12)
    jobs["fx"], jobs["fy"] = fx, fy
    jobs["cx"], jobs["cy"] = W / 2 - 0.5, H / 2 - 0.5              # render_open3d.py:20: Open3D's, not K's
    jobs["v_off"], jobs["nv"] = bank.v_off[m], np.diff(bank.v_off)[m]
    jobs["t_off"], jobs["nt"] = bank.t_off[m], np.diff(bank.t_off)[m]
    return jobs


def render_vehicles(bank: CadBank, mesh_idx: Sequence[int], E: Sequence[np.ndarray], fx: float, fy: float,
                    frame_hw: Tuple[int, int], device, R=None, tr=None, tri_id: bool = False) -> Dict[str, torch.Tensor]:
    """get_rendered (render_open3d.py:29-49) for J posed meshes in one launch: 'sketch' uint8 [J, H, W, 3], 'mask' uint8
    [J, H, W] (1 = vehicle: the complement of the reference's object_mask), 'covered' int32 [J] (device tensors), and
    with tri_id=True 'tri' int32 [J, H, W] (winning triangle within its mesh, -1 = background)."""
    dev = torch.device(device)
    H, W = frame_hw
    jobs = render_jobs(bank, mesh_idx, E, fx, fy, frame_hw, R, tr)
    J = len(jobs)
    out = {"sketch": torch.zeros((J, H, W, 3), dtype=torch.uint8, device=dev),
           "mask": torch.zeros((J, H, W), dtype=torch.uint8, device=dev),
           "covered": torch.zeros((J,), dtype=torch.int32, device=dev)}
    if tri_id:
        out["tri"] = torch.full((J, H, W), -1, dtype=torch.int32, device=dev)
    if J == 0:
        return out
    arr = bank.device_arrays(dev)
    max_nv = int(jobs["nv"].max())
    ws_bytes = J * (16 + 40 * max_nv)
    with torch.cuda.device(dev):
        jobs_d = ops.h2d(np.frombuffer(jobs.tobytes(), np.uint8), dev)
        ws = torch.empty((ws_bytes + 15) // 16 * 2, dtype=torch.float64, device=dev)
        L.check(L.lib().fusg_render_normals_u8(arr["verts"].data_ptr(), arr["normals"].data_ptr(), arr["verts"].shape[0],
                                               arr["tris"].data_ptr(), arr["tris"].shape[0], jobs_d.data_ptr(), J, max_nv, H, W,
                                               ws.data_ptr(), ws.numel() * 8, out["sketch"].data_ptr(), out["mask"].data_ptr(),
                                               out["tri"].data_ptr() if tri_id else None, out["covered"].data_ptr(),
                                               ops.stream_ptr()), "render_normals_u8")
    return out


# ---------------------------------------------------------------------------------------------- visibility
def project_points(points_3d: np.ndarray, K: np.ndarray, E: np.ndarray) -> np.ndarray:
    """online_visibility.py:27-55 (pin-hole with K): [n, 3] -> [n, 2]."""
    p = np.asarray(points_3d)
    ph = np.concatenate([p, np.ones((p.shape[0], 1))], 1)
    q = np.asarray(K) @ np.asarray(E)[:3, :] @ ph.T
    q /= q[2, :]
    return q.T[:, :2]


def visibility_inputs(kp3d: np.ndarray, E: np.ndarray, K: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The host part of compute_visibility for one vehicle: kp3d [12, 3] (KP_NAMES order, already moved), E 4x4, K 3x3 ->
    polygons int32 [7, 8, 2] (the keypoints projected with K one at a time and int()-truncated, :76-77, :127-131), vertex
    counts int32 [7] and per plane the bitmask of the planes strictly nearer the camera (:58-72, :96-100)."""
    kp = {n: np.asarray(kp3d[i]) for i, n in enumerate(KP_NAMES)}
    cam = np.linalg.inv(E)[:3, -1][np.newaxis]
    names = list(VIS_PLANES)
    dist = [float(np.linalg.norm(cam - np.mean([kp[k] for k in VIS_PLANES[p]], 0), axis=1)[0]) for p in names]
    k2 = {n: project_points(np.asarray(kp[n])[np.newaxis], K, E)[0] for n in KP_NAMES}
    pts = np.zeros((7, pu.MAX_VERTS, 2), np.int32)
    nv = np.zeros(7, np.int32)
    nearer = np.zeros(7, np.int32)
    for i, p in enumerate(names):
        # int() as the reference; clipped to +-2^20 px (a keypoint near the camera plane projects arbitrarily far:
        # the polygon rule's int32 arithmetic needs the bound, the clip leaves the frame's pixels unchanged for any sane pose)
        v = [tuple(int(min(max(c, -1048576.0), 1048576.0)) for c in k2[k]) for k in VIS_PLANES[p]]
        pts[i, :len(v)] = v
        nv[i] = len(v)
        nearer[i] = sum(1 << q for q in range(7) if dist[q] < dist[i])
    return pts, nv, nearer


def plane_visibility(kp3d: Sequence[np.ndarray], E: Sequence[np.ndarray], K: np.ndarray, frame_hw: Tuple[int, int],
                     device) -> torch.Tensor:
    """compute_visibility's areas for J vehicles in one launch: counts int32 [J, 7, 2] = (absolute, occluded) on the
    device, planes in VIS_PLANES order.  `visible` turns them into the reference's booleans."""
    dev = torch.device(device)
    H, W = frame_hw
    J = len(kp3d)
    counts = torch.zeros((J, 7, 2), dtype=torch.int32, device=dev)
    if J == 0:
        return counts
    ins = [visibility_inputs(kp3d[j], E[j], K) for j in range(J)]
    with torch.cuda.device(dev):
        pts, nv, nearer = (ops.h2d(np.stack([i[k] for i in ins]), dev) for k in range(3))
        L.check(L.lib().fusg_plane_visibility(pts.data_ptr(), nv.data_ptr(), nearer.data_ptr(), J, H, W, counts.data_ptr(),
                                              ops.stream_ptr()), "plane_visibility")
    return counts


def visible(counts) -> np.ndarray:
    """counts [J, 7, 2] (host) -> bool [J, 7]: occluded > 0.9 * absolute in float64 (online_visibility.py:145-148; an empty
    plane, 0 > 0, is not visible)."""
    c = np.asarray(counts).astype(np.float64)
    return c[..., 1] > 0.9 * c[..., 0]


# ---------------------------------------------------------------------------------------------- the scene keys
def plane_corners(kp_xy: np.ndarray, frame_hw: Tuple[int, int]) -> List[np.ndarray]:
    """get_planes' corner points from frame-pixel keypoints [12, 2]: normalised by (W, H) (vehicle_utils.py:23-25,
    normalize_kpoints) and handed to planes_utils.plane_polygons (* (W, H), int32)."""
    H, W = frame_hw
    k = np.array(kp_xy, np.float64).reshape(len(KP_NAMES), 2)
    k[:, 0] /= W
    k[:, 1] /= H
    return pu.plane_polygons((H, W), {n: k[i] for i, n in enumerate(KP_NAMES)})


def project_keypoints(kp3d: np.ndarray, rvec, tvec, K: np.ndarray) -> np.ndarray:
    """cv2.projectPoints(kp3d, rvec, tvec, K, zero distortion) (trajectory_inference.py:364-367): [n, 3] -> [n, 2]."""
    from .utils.pnp_utils import rodrigues
    X = np.asarray(kp3d, np.float64).reshape(-1, 3)
    Rm = rodrigues(np.asarray(rvec, np.float64).reshape(3))
    pc = X @ Rm.T + np.asarray(tvec, np.float64).reshape(1, 3)
    K = np.asarray(K, np.float64)
    return np.stack([K[0, 0] * (pc[:, 0] / pc[:, 2]) + K[0, 2], K[1, 1] * (pc[:, 1] / pc[:, 2]) + K[1, 2]], 1)


def intrinsic(focals, centers) -> np.ndarray:
    f, c = np.asarray(focals, np.float64).reshape(2), np.asarray(centers, np.float64).reshape(2)
    return np.array([[f[0], 0.0, c[0]], [0.0, f[1], c[1]], [0.0, 0.0, 1.0]])


# ---------------------------------------------------------------------------------------------- the same, V vehicles at once
# Vectorised forms of the per-vehicle functions above, equal to them bit for bit (tests/test_geometry_batch_cpu.py).  Every
# elementwise step is the same IEEE operation in the same order; the matrix products are numpy matmuls of the same per-slice
# shapes and layouts (one BLAS call per slice either way), np.linalg.inv is the same LAPACK solve per matrix, and the means and
# norms reduce over <= 6 contiguous terms, which numpy sums in order.  Two pieces stay per vehicle: the norm of a rotation
# vector (np.linalg.norm of a 1-D array is a BLAS dot) and the cos / sin of its angle (a scalar call may round differently
# from an array one), both as `rodrigues` takes them.
_VIS_IDX = [[KP_NAMES.index(k) for k in names] for names in VIS_PLANES.values()]
_TEX_IDX = [[KP_NAMES.index(k) for k in names] for names in pu.CAR_TEXTURE_PLANES.values()]
_CLIP_PX = 1048576.0


def rotations(rvecs) -> np.ndarray:
    """`rodrigues` of V rotation vectors: [V, 3] (any float dtype) -> float64 [V, 3, 3]."""
    r = np.asarray(rvecs, np.float64).reshape(-1, 3)
    V = r.shape[0]
    th = np.array([float(np.linalg.norm(r[v])) for v in range(V)], np.float64)
    cs = np.array([[np.cos(float(t)), np.sin(float(t))] for t in th], np.float64).reshape(V, 2)
    small = th < 2.220446049250313e-16
    u = r / np.where(small, 1.0, th)[:, None]
    z = np.zeros(V)
    skew = np.stack([z, -u[:, 2], u[:, 1], u[:, 2], z, -u[:, 0], -u[:, 1], u[:, 0], z], 1).reshape(V, 3, 3)
    c, sn = cs[:, 0, None, None], cs[:, 1, None, None]
    Rm = c * np.eye(3) + (1.0 - c) * (u[:, :, None] * u[:, None, :]) + sn * skew
    Rm[small] = np.eye(3)
    return Rm


def extrinsics_from_poses(poses: Sequence[Tuple[np.ndarray, np.ndarray]], Rm: Optional[np.ndarray] = None) -> np.ndarray:
    """`extrinsic_from_pose` of V poses (rvec, tvec): [V, 4, 4] in the vectors' dtype; Rm = `rotations` of the rvecs if known."""
    V = len(poses)
    if V == 0:
        return np.zeros((0, 4, 4), np.float32)
    dts = {np.asarray(r).dtype for r, _ in poses}
    if len(dts) > 1:
        return np.stack([extrinsic_from_pose(r, t) for r, t in poses])
    dt = dts.pop()
    E = np.zeros((V, 4, 4), dt)
    E[:] = np.eye(4, dtype=dt)
    E[:, :3, :3] = rotations([np.asarray(r).reshape(3) for r, _ in poses]) if Rm is None else Rm
    E[:, :3, 3] = np.stack([np.asarray(t).reshape(3) for _, t in poses])
    return E


def visibility_inputs_batch(kp3d: np.ndarray, E: np.ndarray, K: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`visibility_inputs` of V vehicles: kp3d [V, 12, 3], E [V, 4, 4], K 3x3 -> pts int32 [V, 7, 8, 2], nv int32 [V, 7],
    nearer int32 [V, 7].  (A keypoint that projects to NaN - the per-vehicle int() raises there - gives INT32_MIN.)"""
    kp = np.asarray(kp3d)
    E = np.asarray(E)
    V = kp.shape[0]
    pts = np.zeros((V, 7, pu.MAX_VERTS, 2), np.int32)
    nv = np.zeros((V, 7), np.int32)
    nearer = np.zeros((V, 7), np.int32)
    if V == 0:
        return pts, nv, nearer
    cam = np.linalg.inv(E)[:, :3, -1]                                                  # [V, 3]
    mean = np.stack([np.mean(kp[:, idx], axis=1) for idx in _VIS_IDX], 1)             # [V, 7, 3]
    dist = np.linalg.norm(cam[:, None, :] - mean, axis=2)                              # [V, 7]
    ph = np.concatenate([kp, np.ones(kp.shape[:2] + (1,))], 2)[..., None]            # [V, 12, 4, 1]
    q = (np.asarray(K) @ E[:, :3, :])[:, None] @ ph                                    # [V, 12, 3, 1]
    q /= q[:, :, 2:3, :]
    k2 = q[:, :, :2, 0]                                                                # [V, 12, 2]
    with np.errstate(invalid="ignore"):
        k2i = np.clip(k2, -_CLIP_PX, _CLIP_PX).astype(np.int32)
    for i, idx in enumerate(_VIS_IDX):
        pts[:, i, :len(idx)] = k2i[:, idx]
        nv[:, i] = len(idx)
        nearer[:, i] = sum((dist[:, q_] < dist[:, i]).astype(np.int32) << q_ for q_ in range(7))
    return pts, nv, nearer


def plane_corners_batch(kp_xy: np.ndarray, frame_hw: Tuple[int, int]) -> List[np.ndarray]:
    """`plane_corners` of V vehicles: kp_xy [V, 12, 2] -> per texture plane int32 [V, n, 2] (`corner_lists` gives the
    per-vehicle lists)."""
    H, W = frame_hw
    k = np.array(kp_xy, np.float64).reshape(-1, len(KP_NAMES), 2)
    k[..., 0] /= W
    k[..., 1] /= H
    out = []
    for idx in _TEX_IDX:
        p = k[:, idx]
        p[..., 0] *= W
        p[..., 1] *= H
        out.append(np.int32(p))
    return out


def corner_lists(planes: Sequence[np.ndarray]) -> List[List[np.ndarray]]:
    """Per texture plane [V, n, 2] -> per vehicle, per plane [n, 2] (the scene keys' form)."""
    V = planes[0].shape[0] if planes else 0
    return [[p[v] for p in planes] for v in range(V)]


def corner_arrays(planes: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """Per texture plane [V, n, 2] -> the polygons of fusg_fill_poly_planes_batch_u8: pts int32 [V, P, 8, 2], nv int32 [V, P]."""
    V, P = planes[0].shape[0], len(planes)
    pts = np.zeros((V, P, pu.MAX_VERTS, 2), np.int32)
    nv = np.zeros((V, P), np.int32)
    for i, p in enumerate(planes):
        pts[:, i, :p.shape[1]] = p
        nv[:, i] = p.shape[1]
    return pts, nv


def project_keypoints_batch(kp3d: np.ndarray, Rm: np.ndarray, tvecs: np.ndarray, K: np.ndarray) -> np.ndarray:
    """`project_keypoints` of V vehicles: kp3d [V, n, 3], Rm = `rotations` of the rvecs [V, 3, 3], tvecs [V, 3] -> [V, n, 2]."""
    X = np.asarray(kp3d, np.float64)
    pc = X @ np.asarray(Rm).transpose(0, 2, 1) + np.asarray(tvecs, np.float64).reshape(-1, 1, 3)
    K = np.asarray(K, np.float64)
    return np.stack([K[0, 0] * (pc[..., 0] / pc[..., 2]) + K[0, 2], K[1, 1] * (pc[..., 1] / pc[..., 2]) + K[1, 2]], -1)


def vehicle_geometry(bank: CadBank, frame: torch.Tensor, mesh_idx: Sequence[int], poses: Sequence[Tuple[np.ndarray, np.ndarray]],
                     K: np.ndarray, kp_xy: Optional[np.ndarray] = None, steps: Optional[Sequence[Tuple[float, np.ndarray]]] = None
                     ) -> Dict:
    """get_vehicle_information (vehicle_utils.py:12-32) for the V vehicles of a frame, rendered and counted on the device
    with ONE device-to-host copy (the plane counts and covered-pixel counts).  poses: (rvec, tvec) per vehicle (the
    first frame's, after select_and_flip); K: 3x3 intrinsics.

    First frame (steps None): the unmoved meshes; plane corners from the detected keypoints kp_xy [V, 12, 2] (frame
    pixels); returns the scene keys of `VehiclePipeline.run_frame`: 'masks', 'src_sketch' = 'dst_sketch', 'src_planes',
    'src_kp' = 'dst_kp', 'src_vis' = 'dst_vis' (the reference calls get_vehicle_information twice with the same inputs,
    trajectory_inference.py:166-169).
    Later frame (steps = (theta, tr) per vehicle, `trajectory_steps`): meshes and 3-D keypoints moved by v @ z_rot(theta)
    + tr, rendered at the first frame's extrinsic, the moved keypoints projected with K (:359-376); returns 'masks',
    'dst_sketch', 'dst_kp', 'dst_vis'.
    Both also return 'covered' (host int [V]: pixels of each render; 0 = the reference's `except: continue`), 'kp3d'
    (the moved 3-D keypoints, float64 or float32 [V, 12, 3]) and 'extrinsic' [V, 4, 4]."""
    H, W = int(frame.shape[0]), int(frame.shape[1])
    dev = frame.device
    V = len(mesh_idx)
    mesh = np.asarray(mesh_idx, np.int64).reshape(V)
    Rm = rotations([np.asarray(r).reshape(3) for r, _ in poses])
    E = extrinsics_from_poses(poses, Rm)
    if steps is None:
        Rs, trs = None, None
        kp3d = bank.kp3d[mesh]
    else:
        Rs = np.stack([z_rot(th) for th, _ in steps]) if V else np.zeros((0, 3, 3))
        trs = np.stack([np.asarray(t, np.float64).reshape(3) for _, t in steps]) if V else np.zeros((0, 3))
        kp3d = bank.kp3d[mesh] @ Rs + trs[:, None, :]                                  # :360-362
    if steps is None:
        corners = plane_corners_batch(kp_xy, (H, W)) if V else []
    else:
        tv = np.stack([np.asarray(t, np.float64).reshape(3) for _, t in poses]) if V else np.zeros((0, 3))
        corners = plane_corners_batch(project_keypoints_batch(kp3d, Rm, tv, K), (H, W)) if V else []
    kp = corner_lists(corners) if V else []
    with torch.cuda.device(dev):
        r = render_vehicles(bank, mesh, E, float(K[0, 0]), float(K[1, 1]), (H, W), dev, Rs, trs)
        counts = torch.zeros((V, 7, 2), dtype=torch.int32, device=dev)
        planes = torch.empty((V, len(TEXTURE_PLANES), H, W, 3), dtype=torch.uint8, device=dev)
        if V:
            # one H2D of every polygon of the frame: the visibility planes, then (first frame) the texture planes
            vpts, vnv, near = visibility_inputs_batch(kp3d, E, K)
            parts = [vpts.reshape(-1), vnv.reshape(-1), near.reshape(-1)]
            if steps is None:
                fpts, fnv = corner_arrays(corners)
                parts += [fpts.reshape(-1), fnv.reshape(-1)]
            buf = ops.h2d(np.concatenate(parts), dev)
            off = np.cumsum([0] + [len(a) for a in parts])
            seg = [buf[off[i]:off[i + 1]] for i in range(len(parts))]
            L.check(L.lib().fusg_plane_visibility(seg[0].data_ptr(), seg[1].data_ptr(), seg[2].data_ptr(), V, H, W,
                                                  counts.data_ptr(), ops.stream_ptr()), "plane_visibility")
        host = torch.cat([counts.view(V, 14), r["covered"].view(V, 1)], 1).cpu().numpy()
        if V and steps is None:                                   # queued after the read-back: it does not wait for the planes
            pu.fill_planes_batch(frame, seg[3], seg[4], planes)
    return _geometry_result(r, host[:, :14].reshape(V, 7, 2), host[:, 14], kp3d if V else np.zeros((0, 12, 3)), E, kp, planes,
                            steps is None)


def _geometry_result(r: Dict[str, torch.Tensor], counts: np.ndarray, covered: np.ndarray, kp3d: np.ndarray, E: np.ndarray, kp: List,
                     planes: torch.Tensor, first: bool) -> Dict:
    """The tail `vehicle_geometry` and `vehicle_geometry_device` share: the read-back plane counts [V, 7, 2] and covered-pixel
    counts [V] (host) -> the visibilities and the result dict of either."""
    vis = visible(counts)[:, :len(TEXTURE_PLANES)].astype(np.uint8)
    out = {"masks": r["mask"], "covered": np.asarray(covered).astype(np.int64), "kp3d": kp3d, "extrinsic": E, "counts": counts}
    if first:
        out.update(src_sketch=r["sketch"], dst_sketch=r["sketch"], src_planes=planes, src_kp=kp, dst_kp=kp, src_vis=vis, dst_vis=vis)
    else:
        out.update(dst_sketch=r["sketch"], dst_kp=kp, dst_vis=vis)
    return out


# ---------------------------------------------------------------------------------------------- the same, derived on the device
_TEX_NV = [len(i) for i in _TEX_IDX]
# fusg_pose_geometry's per-vehicle outputs: name, dtype, elements per vehicle
_PG_OUT = (("jobs", np.uint8, JOB_DTYPE.itemsize), ("extrinsic", np.float64, 12), ("kp3d", np.float64, 36), ("pose", np.float32, 7),
           ("vis_pts", np.int32, 7 * pu.MAX_VERTS * 2), ("vis_nv", np.int32, 7), ("nearer", np.int32, 7),
           ("tex_pts", np.int32, len(_TEX_IDX) * pu.MAX_VERTS * 2), ("tex_nv", np.int32, len(_TEX_IDX)), ("status", np.int32, 1))
_PG_CALL = ("pose", "extrinsic", "kp3d", "jobs", "vis_pts", "vis_nv", "nearer", "tex_pts", "tex_nv", "status")   # the ABI's order


def _pack_layout(parts) -> Tuple[Dict[str, Tuple[int, np.dtype, int]], int]:
    """One buffer for several small arrays, parts = (name, dtype, elements): name -> (byte offset, dtype, elements) and the
    buffer's bytes; each part 8-byte aligned."""
    lay, off = {}, 0
    for name, dt, n in parts:
        lay[name] = (off, np.dtype(dt), n)
        off += (n * np.dtype(dt).itemsize + 7) // 8 * 8
    return lay, off


def _pg_layout(V: int, extra=()) -> Tuple[Dict[str, Tuple[int, np.dtype, int]], int]:
    """One buffer for every small per-vehicle array: name -> (byte offset, dtype, elements); each part 8-byte aligned."""
    return _pack_layout((name, dt, V * per) for name, dt, per in tuple(_PG_OUT) + tuple(extra))


def pose_geometry_host(bank: CadBank, cad_idx, K: np.ndarray, frame_hw: Tuple[int, int], raw=None, kp_xy=None, pose=None,
                       steps=None) -> Dict[str, np.ndarray]:
    """fusg_pose_geometry_host: the device path's per-vehicle arithmetic on the CPU (no GPU needed), numpy in and out.  A first
    frame gives raw = (rvec [V, 4, 3], tvec [V, 4, 3], err [V, 4]) and kp_xy [V, 12, 2]; a later frame pose [V, 7] (a first
    frame's 'pose') and steps [V, 4] = (theta, tr).  Returns fusg_pose_geometry's outputs by name ('jobs' as JOB_DTYPE)."""
    H, W = frame_hw
    cad = np.ascontiguousarray(np.asarray(cad_idx, np.int64).reshape(-1))
    V = cad.shape[0]
    f32 = lambda a, sh: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape((V,) + sh))   # noqa: E731
    rv, tv, er = (None, None, None) if raw is None else (f32(raw[0], (4, 3)), f32(raw[1], (4, 3)), f32(raw[2], (4,)))
    ins = [rv, tv, er, f32(pose, (7,)), f32(kp_xy, (12, 2)),
           None if steps is None else np.ascontiguousarray(np.asarray(steps, np.float64).reshape(V, 4)), cad]
    tabs = [np.ascontiguousarray(bank.kp3d, dtype=np.float32), bank.v_off.astype(np.int32), bank.t_off.astype(np.int32)]
    Kc = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
    out = {name: np.zeros(V * per, dt) for name, dt, per in _PG_OUT}
    ptr = lambda a: None if a is None else a.ctypes.data     # noqa: E731
    L.check(L.lib().fusg_pose_geometry_host(*(ptr(a) for a in ins), *(ptr(a) for a in tabs), len(bank), ptr(Kc), H, W, V,
                                            *(ptr(out[k]) for k in _PG_CALL)), "pose_geometry_host")
    shapes = {"extrinsic": (V, 12), "kp3d": (V, 12, 3), "pose": (V, 7), "vis_pts": (V, 7, pu.MAX_VERTS, 2), "vis_nv": (V, 7),
              "nearer": (V, 7), "tex_pts": (V, len(_TEX_IDX), pu.MAX_VERTS, 2), "tex_nv": (V, len(_TEX_IDX)), "status": (V,)}
    res = {k: out[k].reshape(sh) for k, sh in shapes.items()}
    res["jobs"] = out["jobs"].view(JOB_DTYPE)
    return res


_PG_SHAPES = {"extrinsic": (12,), "kp3d": (12, 3), "pose": (7,), "vis_pts": (7, pu.MAX_VERTS, 2), "vis_nv": (7,), "nearer": (7,),
              "tex_pts": (len(_TEX_IDX), pu.MAX_VERTS, 2), "tex_nv": (len(_TEX_IDX),), "status": ()}


def pose_geometry_clips_host(bank: CadBank, frame_hw: Tuple[int, int], clips: Sequence[Dict]) -> Dict[str, np.ndarray]:
    """fusg_pose_geometry_clips_host: the several-clip later-frame stage's per-row arithmetic on the CPU (no GPU needed), numpy in
    and out.  clips[c] = {'pose' [V_c, 7], 'cad_idx' [V_c], 'src_pts' int32 [V_c, 5, 8, 2], 'K' 3 x 3, 'steps' [F_c * V_c, 4] (frame-
    major)}; rows clip-major.  Returns fusg_pose_geometry's outputs by name at J = sum(F_c * V_c) rows ('jobs' as JOB_DTYPE) and
    'src_pts_rows' int32 [J, 5, 8, 2]."""
    import ctypes as C
    H, W = frame_hw
    n, P = len(clips), len(_TEX_IDX)
    pose = [np.ascontiguousarray(np.asarray(cl["pose"], np.float32).reshape(-1, 7)) for cl in clips]
    cad = [np.ascontiguousarray(np.asarray(cl["cad_idx"], np.int64).reshape(-1)) for cl in clips]
    pts = [np.ascontiguousarray(np.asarray(cl["src_pts"], np.int32).reshape(-1, P, pu.MAX_VERTS, 2)) for cl in clips]
    steps = [np.asarray(cl["steps"], np.float64).reshape(-1, 4) for cl in clips]
    first = [0]
    for s in steps:
        first.append(first[-1] + s.shape[0])
    J = first[-1]
    steps_all = np.ascontiguousarray(np.concatenate(steps)) if n else np.zeros((0, 4))
    cams = np.ascontiguousarray(np.concatenate([np.asarray(cl["K"], np.float64).reshape(9) for cl in clips])) if n else np.zeros(0)
    tabs = [np.ascontiguousarray(bank.kp3d, dtype=np.float32), bank.v_off.astype(np.int32), bank.t_off.astype(np.int32)]
    out = {name: np.zeros(J * per, dt) for name, dt, per in _PG_OUT}
    rows = np.zeros((J, P, pu.MAX_VERTS, 2), np.int32)
    tab = lambda arrs: (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])     # noqa: E731
    L.check(L.lib().fusg_pose_geometry_clips_host(tab(pose), tab(cad), tab(pts), (C.c_int32 * max(n, 1))(*[len(a) for a in cad]),
                                                  (C.c_int32 * (n + 1))(*first), n, steps_all.ctypes.data, cams.ctypes.data,
                                                  *(a.ctypes.data for a in tabs), len(bank), H, W, J,
                                                  *(out[k].ctypes.data for k in _PG_CALL), rows.ctypes.data), "pose_geometry_clips_host")
    res = {k: out[k].reshape((J,) + sh) for k, sh in _PG_SHAPES.items()}
    res["jobs"] = out["jobs"].view(JOB_DTYPE)
    res["src_pts_rows"] = rows
    return res


def steps_array(steps: Sequence[Tuple[float, np.ndarray]]) -> np.ndarray:
    """(theta, tr) per vehicle (`trajectory_steps`) -> float64 [V, 4], fusg_pose_geometry's form."""
    return np.array([[float(th), *np.asarray(t, np.float64).reshape(3)] for th, t in steps], np.float64).reshape(-1, 4)


def vehicle_geometry_device(bank: CadBank, frame: torch.Tensor, cad_idx_d: torch.Tensor, K: np.ndarray, raw_d=None, pose_d=None,
                            kp_xy_d: Optional[torch.Tensor] = None, steps=None) -> Dict:
    """`vehicle_geometry` with the pose selected and its geometry derived on the device (fusg_pose_geometry): nothing of the
    fit is read back before the render is queued.  cad_idx_d: CUDA int64 [V].  First frame: raw_d = `cpc_fit_device`'s (rvec
    [V, 4, 3], tvec, err [V, 4]) and kp_xy_d float32 [V, 12, 2], both on the device; later frame: pose_d CUDA float32 [V, 7]
    (a first frame's 'pose_d') and steps = (theta, tr) per vehicle (host).  Order of work: fusg_pose_geometry -> render of the
    device jobs -> plane visibility -> ONE device-to-host copy of every small
    result (`ops.d2h`) -> the plane cut-outs, queued behind that read-back.
    Returns `vehicle_geometry`'s keys (host values from the read-back: within the last bits of the numpy path's, the integer
    ones equal wherever no coordinate sits within that of an integer) and 'pose' float32 [V, 7] (error, rvec, tvec: host),
    'pose_d' (the same, device), 'cad_idx' (host int64 [V]), 'status' (host int32 [V]), 'tex_pts_d' / 'tex_nv_d' (the corner
    points as the device tensors `plane_homographies_device` takes: int32 [V, 5, 8, 2], [5]).  A cad_idx outside the bank
    raises IndexError after the read-back (its job is empty: nothing was read out of range).
    The render's workspace is sized by the bank's largest model, V * (16 + 40 * bank.max_nv) bytes, whichever models are in
    view (the jobs are not read back to size it), and comes from torch's caching allocator on every frame: a bank with one very
    large mesh pays for it on every frame."""
    H, W = int(frame.shape[0]), int(frame.shape[1])
    dev = frame.device
    V = int(cad_idx_d.shape[0])
    first = steps is None
    P = len(TEXTURE_PLANES)
    with torch.cuda.device(dev):
        planes = torch.empty((V, P, H, W, 3), dtype=torch.uint8, device=dev)
        st = _device_stage(bank, (H, W), dev, cad_idx_d, K, raw_d=raw_d, pose_d=pose_d, kp_xy_d=kp_xy_d,
                           steps_d=None if first or not V else ops.h2d(steps_array(steps), dev))
        host = ops.d2h(st["buf"]) if V else np.zeros(0, np.uint8)       # the one blocking copy of the stage
        if V and first:                                           # queued after the read-back: it does not wait for the planes
            pu.fill_planes_batch(frame, st["d"]["tex_pts"], st["d"]["tex_nv"], planes)
    return _device_stage_result(bank, st, host, planes, first)


_TORCH_DT = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64,
             np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
_STAGE_EXTRA = (("counts", np.int32, 14), ("covered", np.int32, 1), ("cad_idx", np.int64, 1))


def _device_stage(bank: CadBank, frame_hw: Tuple[int, int], dev, cad_idx_d: torch.Tensor, K: np.ndarray, raw_d=None, pose_d=None,
                  kp_xy_d=None, steps_d=None, extra=(), K_runs=None) -> Dict:
    """The launches `vehicle_geometry_device` and `later_geometry_batch_device` share, for V rows on the current stream:
    fusg_pose_geometry -> fusg_render_normals_u8 of the device jobs -> fusg_plane_visibility, every small result in ONE zeroed
    buffer (`_pg_layout` + counts, covered, cad_idx + `extra`).  A first frame gives raw_d and kp_xy_d, a later frame pose_d and
    steps_d (CUDA float64 [V, 4]).  Returns 'lay' / 'nbytes' (the layout), 'buf' (the buffer), 'd' (its parts as device views),
    'r' ('sketch' uint8 [V, H, W, 3], 'mask' uint8 [V, H, W]) and 'V'.  Nothing is read back.  K_runs (rows of several cameras):
    [(lo, hi, K)] covering the rows in order - fusg_pose_geometry takes one host K, so it is launched once per run into the row
    slices of the same buffers; None: one launch with `K`."""
    H, W = frame_hw
    V = int(cad_idx_d.shape[0])
    first = steps_d is None and pose_d is None
    st = _stage_buffers(V, frame_hw, dev, extra)
    d = st["d"]
    if V:
        if cad_idx_d.dtype != torch.int64 or not cad_idx_d.is_cuda:
            raise ValueError("vehicle_geometry_device: cad_idx_d is a CUDA int64 [V]")
        arr = bank.device_arrays(dev)
        f32 = lambda t, sh: t.to(torch.float32).contiguous().view((V,) + sh)        # noqa: E731
        if first:
            ins = [f32(raw_d[0], (4, 3)), f32(raw_d[1], (4, 3)), f32(raw_d[2], (4,)), None, f32(kp_xy_d, (12, 2)), None]
        else:
            ins = [None, None, None, f32(pose_d, (7,)), None, steps_d]
        cad_c = cad_idx_d.contiguous()
        d["cad_idx"].copy_(cad_c)
        lib = L.lib()
        per = {name: n for name, _, n in _PG_OUT}
        row = lambda t, lo: None if t is None else t.data_ptr() + lo * (t.numel() // V) * t.element_size()   # noqa: E731
        for lo, hi, Kr in ([(0, V, K)] if K_runs is None else K_runs):
            Kc = np.ascontiguousarray(np.asarray(Kr, np.float64).reshape(9))
            L.check(lib.fusg_pose_geometry(*(row(t, lo) for t in ins), row(cad_c, lo), arr["kp3d"].data_ptr(), arr["v_off"].data_ptr(),
                                           arr["t_off"].data_ptr(), len(bank), Kc.ctypes.data, H, W, hi - lo,
                                           *(d[k].data_ptr() + lo * per[k] * d[k].element_size() for k in _PG_CALL), ops.stream_ptr()),
                    "pose_geometry")
        _stage_render(bank, st, frame_hw, dev)
    return st


def _stage_buffers(V: int, frame_hw: Tuple[int, int], dev, extra=()) -> Dict:
    """The buffers of a device stage of V rows, zeroed: `_device_stage`'s result before anything is launched."""
    H, W = frame_hw
    lay, nbytes = _pg_layout(V, _STAGE_EXTRA + tuple(extra))
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    d = {k: buf[o:o + n * dt.itemsize].view(_TORCH_DT[dt]) for k, (o, dt, n) in lay.items()}
    r = {"sketch": torch.zeros((V, H, W, 3), dtype=torch.uint8, device=dev),
         "mask": torch.zeros((V, H, W), dtype=torch.uint8, device=dev)}
    return {"lay": lay, "nbytes": nbytes, "buf": buf, "d": d, "r": r, "V": V}


def _stage_render(bank: CadBank, st: Dict, frame_hw: Tuple[int, int], dev) -> None:
    """What follows the pose geometry in every device stage, for the V > 0 rows of `st` (`_stage_buffers`, its jobs and visibility
    polygons written): fusg_render_normals_u8 of the device jobs -> fusg_plane_visibility, on the current stream."""
    H, W = frame_hw
    V, d, r = st["V"], st["d"], st["r"]
    arr, lib = bank.device_arrays(dev), L.lib()
    max_nv = bank.max_nv
    ws = torch.empty((V * (16 + 40 * max_nv) + 15) // 16 * 2, dtype=torch.float64, device=dev)
    L.check(lib.fusg_render_normals_u8(arr["verts"].data_ptr(), arr["normals"].data_ptr(), arr["verts"].shape[0],
                                       arr["tris"].data_ptr(), arr["tris"].shape[0], d["jobs"].data_ptr(), V, max_nv, H, W,
                                       ws.data_ptr(), ws.numel() * 8, r["sketch"].data_ptr(), r["mask"].data_ptr(), None,
                                       d["covered"].data_ptr(), ops.stream_ptr()), "render_normals_u8")
    L.check(lib.fusg_plane_visibility(d["vis_pts"].data_ptr(), d["vis_nv"].data_ptr(), d["nearer"].data_ptr(), V, H, W,
                                      d["counts"].data_ptr(), ops.stream_ptr()), "plane_visibility")


def _stage_gate(st: Dict, box_rows: Optional[torch.Tensor]) -> None:
    """fusg_later_gate over the V > 0 rows of a stage made with the extras 'dst_vis' and 'valid' (box_rows: zeroed in place where
    the render is empty)."""
    d = st["d"]
    L.check(L.lib().fusg_later_gate(d["counts"].data_ptr(), d["covered"].data_ptr(), st["V"], len(TEXTURE_PLANES), d["dst_vis"].data_ptr(),
                                    d["valid"].data_ptr(), None if box_rows is None else box_rows.data_ptr(), ops.stream_ptr()),
            "later_gate")


def _stage_host_valid(bank: CadBank, st: Dict, read: np.ndarray, planes: Optional[torch.Tensor], first: bool) -> Dict:
    """`_device_stage_result` of a gated stage's read-back bytes plus 'valid' (host int32 [V])."""
    out = _device_stage_result(bank, st, read, planes, first)
    o, dt, n = st["lay"]["valid"]
    out["valid"] = read[o:o + n * dt.itemsize].view(dt).copy()
    return out


def _device_stage_result(bank: CadBank, st: Dict, host: np.ndarray, planes: Optional[torch.Tensor], first: bool) -> Dict:
    """`_device_stage`'s read-back bytes `host` -> `vehicle_geometry_device`'s result (IndexError for a cad_idx outside the bank)."""
    V, d, r, P = st["V"], st["d"], st["r"], len(TEXTURE_PLANES)
    h = {k: host[o:o + n * dt.itemsize].view(dt) for k, (o, dt, n) in st["lay"].items()}
    bad = np.flatnonzero(h["status"] != 0)
    if len(bad):
        raise IndexError(f"render: mesh {int(h['cad_idx'][bad[0]])} not in a bank of {len(bank)}")
    tex = h["tex_pts"].reshape(V, P, pu.MAX_VERTS, 2)
    kp = corner_lists([tex[:, i, :n].copy() for i, n in enumerate(_TEX_NV)]) if V else []
    E = np.zeros((V, 4, 4), np.float32)
    E[:] = np.eye(4, dtype=np.float32)
    E[:, :3, :] = h["extrinsic"].reshape(V, 3, 4)                 # (float32 values carried in float64: the cast is exact)
    kp3d = h["kp3d"].reshape(V, 12, 3)
    out = _geometry_result(r, h["counts"].reshape(V, 7, 2).copy(), h["covered"], kp3d.astype(np.float32) if first else kp3d.copy(),
                           E, kp, planes, first)
    out.update(pose=h["pose"].reshape(V, 7).copy(), pose_d=d["pose"].view(V, 7), cad_idx=h["cad_idx"].copy(), status=h["status"].copy(),
               tex_pts_d=d["tex_pts"].view(V, P, pu.MAX_VERTS, 2), tex_nv_d=d["tex_nv"][:P] if V else d["tex_nv"])
    return out


def later_geometry_batch_device(bank: CadBank, frame_hw: Tuple[int, int], cad_idx_d: torch.Tensor, pose_d: torch.Tensor, K: np.ndarray,
                                steps_per_frame: Sequence[Sequence[Tuple[float, np.ndarray]]], box_rows: Optional[torch.Tensor] = None
                                ) -> Dict:
    """`vehicle_geometry_device`'s later-frame branch for the F frames of a clip at once, WITHOUT its read-back: F * V rows,
    frame-major (row f * V + v = frame f, vehicle v: `pipeline.later_batch_row`).  cad_idx_d CUDA int64 [V] and pose_d CUDA
    float32 [V, 7] (a first frame's) are repeated F times on the device; steps_per_frame[f] = (theta, tr) per vehicle, one
    [F * V, 4] upload.  Order of work, all on the current stream: fusg_pose_geometry -> fusg_render_normals_u8 ->
    fusg_plane_visibility -> fusg_later_gate, which turns the plane counts and covered counts into what the host decided after
    the read-back: 'valid_d' int32 [F * V] (the render is not empty) and 'dst_vis_d' uint8 [F * V, 5], the visibilities with
    the rows of an empty render zeroed - `plane_homographies_device` then gives such a row no job.  box_rows: CUDA int32
    [F * V, 8] paste box rows, zeroed in place where the render is empty.
    Returns the device tensors 'mask' uint8 [F * V, H, W], 'sketch' uint8 [F * V, H, W, 3], 'tex_pts_d' int32 [F * V, 5, 8, 2],
    'tex_nv_d' int32 [5], 'dst_vis_d', 'valid_d'; 'buf', the one small packed buffer (`_pg_layout` + counts, covered, cad_idx,
    the gate's outputs) to read back whenever the caller likes (`ops.d2h`), and 'host' = a function of the read-back bytes that
    gives the host keys of `vehicle_geometry_device` ('dst_kp', 'dst_vis' = `visible(counts)`, UN-gated as the per-frame path
    reports it, 'kp3d', 'covered', 'status', ...; IndexError for a cad_idx outside the bank) plus 'valid' (host int32 [F * V])."""
    H, W = frame_hw
    dev = cad_idx_d.device
    V, F, P = int(cad_idx_d.shape[0]), len(steps_per_frame), len(TEXTURE_PLANES)
    if any(len(s) != V for s in steps_per_frame):
        raise ValueError(f"later_geometry_batch_device: every frame carries (theta, tr) for the {V} vehicles")
    N = F * V
    if box_rows is not None and (not box_rows.is_cuda or box_rows.dtype != torch.int32 or tuple(box_rows.shape) != (N, 8)
                                 or not box_rows.is_contiguous()):
        raise ValueError("later_geometry_batch_device: box_rows is a contiguous CUDA int32 [F * V, 8]")
    with torch.cuda.device(dev):
        steps_d = ops.h2d(np.concatenate([steps_array(s) for s in steps_per_frame]).reshape(N, 4), dev) if N else None
        st = _device_stage(bank, (H, W), dev, cad_idx_d.repeat(F), K, pose_d=pose_d.to(torch.float32).reshape(V, 7).repeat(F, 1),
                           steps_d=steps_d, extra=(("dst_vis", np.uint8, P), ("valid", np.int32, 1)))
        if N:
            _stage_gate(st, box_rows)
    return _later_stage_result(st, lambda read: _stage_host_valid(bank, st, read, None, False))


def _later_stage_result(st: Dict, host) -> Dict:
    """What a gated later-frame stage of N rows hands its driver: `later_geometry_batch_device`'s keys."""
    d, N, P = st["d"], st["V"], len(TEXTURE_PLANES)
    return {"mask": st["r"]["mask"], "sketch": st["r"]["sketch"], "tex_pts_d": d["tex_pts"].view(N, P, pu.MAX_VERTS, 2),
            "tex_nv_d": d["tex_nv"][:P], "dst_vis_d": d["dst_vis"].view(N, P), "valid_d": d["valid"], "buf": st["buf"], "host": host}


def later_geometry_clips_device(bank: CadBank, frame_hw: Tuple[int, int], clips: Sequence[Dict],
                                box_rows: Optional[torch.Tensor] = None) -> Dict:
    """`later_geometry_batch_device` for the future frames of SEVERAL clips at once: J = sum(F_c * V_c) rows, clip-major and
    frame-major inside a clip (row `pipeline.clip_batch_offsets`[c] + f * V_c + v = clip c, frame f, vehicle v).  clips[c] =
    {'cad_idx_d' CUDA int64 [V_c], 'pose_d' CUDA float32 [V_c, 7], 'src_kp_d' CUDA int32 [V_c, 5, 8, 2] (the first frame's
    corner points), 'src_vis' host [V_c, 5], 'K' the clip's 3 x 3 intrinsics (host), 'steps_per_frame' [F_c][V_c] of (theta, tr);
    optional 'cad_idx' host int64 [V_c], what the host result reports (without it the device copy is read when 'host' is called)}.
    At most `_lib.MAX_FRAMES` clips.  Nothing per clip is repeated or concatenated on the device: each clip's tables are passed
    by pointer (fusg_pose_geometry_clips), and ONE upload carries everything the host knows - the steps of all rows, the
    cameras, the source visibilities repeated per frame (`_pack_layout`).  Order of work, all on the current stream: that upload
    -> fusg_pose_geometry_clips -> fusg_render_normals_u8 -> fusg_plane_visibility -> fusg_later_gate, once each at J rows;
    nothing is read back.  box_rows: CUDA int32 [J, 8] paste box rows, zeroed in place where the render is empty.
    Returns `later_geometry_batch_device`'s keys at J rows, and 'src_kp_d' int32 [J, 5, 8, 2] (each row's source corner points,
    written by the same launch), 'src_vis_d' uint8 [J, 5] and 'kp_nv_d' int32 [5] as `plane_homographies_device` takes them."""
    import ctypes as C
    H, W = frame_hw
    clips = list(clips)
    n, P = len(clips), len(TEXTURE_PLANES)
    if not 1 <= n <= L.MAX_FRAMES:
        raise ValueError(f"later_geometry_clips_device: {n} clips (1..{L.MAX_FRAMES} per launch)")
    dev = clips[0]["cad_idx_d"].device
    veh, first, steps, vis = [], [0], [], []
    for c, cl in enumerate(clips):
        V = int(cl["cad_idx_d"].shape[0])
        if any(len(s) != V for s in cl["steps_per_frame"]):
            raise ValueError(f"later_geometry_clips_device: every frame of clip {c} carries (theta, tr) for its {V} vehicles")
        for k, dt, sh in (("cad_idx_d", torch.int64, (V,)), ("pose_d", torch.float32, (V, 7)), ("src_kp_d", torch.int32, (V, P, pu.MAX_VERTS, 2))):
            t = cl[k]
            if not (torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == dt and tuple(t.shape) == sh and t.is_contiguous()):
                raise ValueError(f"later_geometry_clips_device: clip {c}'s {k!r} is a contiguous CUDA {dt} {list(sh)} (it is passed "
                                 "by pointer, not copied)")
        F = len(cl["steps_per_frame"])
        veh.append(V)
        first.append(first[-1] + F * V)
        if F * V:
            steps.extend(steps_array(s) for s in cl["steps_per_frame"])
            vis.append(np.tile((np.asarray(cl["src_vis"]).reshape(V, P) != 0).astype(np.uint8), (F, 1)))
    J = first[-1]
    if box_rows is not None and (not box_rows.is_cuda or box_rows.dtype != torch.int32 or tuple(box_rows.shape) != (J, 8)
                                 or not box_rows.is_contiguous()):
        raise ValueError("later_geometry_clips_device: box_rows is a contiguous CUDA int32 [J, 8]")
    with torch.cuda.device(dev):
        st = _stage_buffers(J, frame_hw, dev, (("dst_vis", np.uint8, P), ("valid", np.int32, 1), ("src_pts", np.int32, P * pu.MAX_VERTS * 2)))
        d = st["d"]
        up_lay, up_bytes = _pack_layout((("steps", np.float64, J * 4), ("cams", np.float64, n * 9), ("src_vis", np.uint8, J * P)))
        up = {}
        if J:
            blob = np.zeros(up_bytes, np.uint8)
            part = lambda k: blob[up_lay[k][0]:up_lay[k][0] + up_lay[k][2] * up_lay[k][1].itemsize].view(up_lay[k][1])   # noqa: E731
            part("steps")[:] = np.concatenate(steps).reshape(-1)
            part("cams")[:] = np.concatenate([np.asarray(cl["K"], np.float64).reshape(9) for cl in clips])
            part("src_vis")[:] = np.concatenate(vis).reshape(-1)
            blob_d = ops.h2d(blob, dev)                               # the one upload of the call
            up = {k: blob_d[o:o + m * dt.itemsize].view(_TORCH_DT[dt]) for k, (o, dt, m) in up_lay.items()}
            arr = bank.device_arrays(dev)
            live = [first[c + 1] > first[c] for c in range(n)]
            tab = lambda k: (C.c_void_p * n)(*[cl[k].data_ptr() if own else None for cl, own in zip(clips, live)])   # noqa: E731
            L.check(L.lib().fusg_pose_geometry_clips(tab("pose_d"), tab("cad_idx_d"), tab("src_kp_d"), (C.c_int32 * n)(*veh),
                                                     (C.c_int32 * (n + 1))(*first), n, up["steps"].data_ptr(), up["cams"].data_ptr(),
                                                     arr["kp3d"].data_ptr(), arr["v_off"].data_ptr(), arr["t_off"].data_ptr(), len(bank),
                                                     H, W, J, *(d[k].data_ptr() for k in _PG_CALL), d["src_pts"].data_ptr(),
                                                     ops.stream_ptr()), "pose_geometry_clips")
            _stage_render(bank, st, frame_hw, dev)
            _stage_gate(st, box_rows)

    def host(read: np.ndarray) -> Dict:
        o, dt, m = st["lay"]["cad_idx"]                             # (the launch reads each clip's own table: the buffer's rows are filled here)
        read = read.copy()
        rows = [np.tile(np.asarray(cl["cad_idx"] if cl.get("cad_idx") is not None else ops.d2h(cl["cad_idx_d"]), np.int64).reshape(-1),
                        len(cl["steps_per_frame"])) for cl in clips]
        read[o:o + m * dt.itemsize].view(dt)[:] = np.concatenate(rows)
        return _stage_host_valid(bank, st, read, None, False)

    out = _later_stage_result(st, host)
    out.update(src_kp_d=d["src_pts"].view(J, P, pu.MAX_VERTS, 2), src_vis_d=up["src_vis"].view(J, P) if J else d["dst_vis"].view(J, P),
               kp_nv_d=d["tex_nv"][:P])
    return out


def camera_runs(Ks: Sequence[np.ndarray], offs: Sequence[int]) -> List[Tuple[int, int, np.ndarray]]:
    """(row lo, row hi, K) per maximal run of consecutive scenes whose K has equal focals and centers, rows scene-major by the
    offsets `offs`; runs without rows are dropped.  A one-camera video is one run."""
    key = lambda K: tuple(float(np.asarray(K, np.float64)[i, j]) for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))   # noqa: E731
    runs: List[Tuple[int, int, np.ndarray]] = []
    for f, K in enumerate(Ks):
        lo, hi = int(offs[f]), int(offs[f + 1])
        if hi == lo:
            continue
        if runs and runs[-1][1] == lo and key(runs[-1][2]) == key(K):
            runs[-1] = (runs[-1][0], hi, runs[-1][2])
        else:
            runs.append((lo, hi, np.asarray(K, np.float64)))
    return runs


def first_geometry_batch_device(bank: CadBank, frames: Sequence[torch.Tensor], offs: Sequence[int], cad_idx_d: torch.Tensor,
                                Ks: Sequence[np.ndarray], raw_d, kp_xy_d: torch.Tensor, box_rows: Optional[torch.Tensor] = None) -> Dict:
    """`vehicle_geometry_device`'s first-frame branch for the vehicles of SEVERAL scenes at once, WITHOUT its read-back: N =
    offs[-1] rows, scene-major (rows offs[f] .. offs[f + 1] are scene f's vehicles, cut from frames[f]: CUDA uint8 [H, W, 3] of one
    size).  cad_idx_d CUDA int64 [N]; raw_d = `cpc_fit_device`'s (rvec [N, 4, 3], tvec, err [N, 4]) and kp_xy_d float32 [N, 12, 2]
    on the device; Ks[f] = scene f's 3 x 3 intrinsics (host).  Order of work, all on the current stream: fusg_pose_geometry once
    per run of scenes with one camera (`camera_runs`) -> fusg_render_normals_u8 -> fusg_plane_visibility -> fusg_later_gate (on a
    first frame src_vis = dst_vis, so its one gated table serves both; box_rows: CUDA int32 [N, 8] paste box rows, zeroed in place
    where the render is empty) -> the plane cut-outs of every row from its own frame (`planes_utils.fill_planes_frames`).
    Returns the device tensors 'mask' uint8 [N, H, W], 'sketch' uint8 [N, H, W, 3], 'planes' uint8 [N, 5, H, W, 3], 'tex_pts_d'
    int32 [N, 5, 8, 2], 'tex_nv_d' int32 [5], 'vis_d' uint8 [N, 5] (gated), 'valid_d' int32 [N], 'pose_d' float32 [N, 7]; 'buf',
    the one small packed buffer to read back whenever the caller likes (`ops.d2h`), and 'host' = a function of the read-back bytes
    that gives the host keys of `vehicle_geometry_device` ('src_vis' = 'dst_vis' = `visible(counts)`, UN-gated as the per-frame
    path reports it; 'src_planes' = 'planes'; IndexError for a cad_idx outside the bank) plus 'valid' (host int32 [N])."""
    if len(frames) < 1 or len(offs) != len(frames) + 1 or len(Ks) != len(frames):
        raise ValueError(f"first_geometry_batch_device: {len(frames)} frames, {len(offs)} offsets, {len(Ks)} intrinsics")
    H, W = int(frames[0].shape[0]), int(frames[0].shape[1])
    dev = frames[0].device
    N, P = int(offs[-1]), len(TEXTURE_PLANES)
    if int(cad_idx_d.shape[0]) != N:
        raise ValueError(f"first_geometry_batch_device: {int(cad_idx_d.shape[0])} CAD indices for {N} rows")
    if box_rows is not None and (not box_rows.is_cuda or box_rows.dtype != torch.int32 or tuple(box_rows.shape) != (N, 8)
                                 or not box_rows.is_contiguous()):
        raise ValueError("first_geometry_batch_device: box_rows is a contiguous CUDA int32 [N, 8]")
    with torch.cuda.device(dev):
        planes = torch.empty((N, P, H, W, 3), dtype=torch.uint8, device=dev)
        runs = camera_runs(Ks, offs)
        st = _device_stage(bank, (H, W), dev, cad_idx_d, runs[0][2] if runs else Ks[0], raw_d=raw_d, kp_xy_d=kp_xy_d,
                           extra=(("dst_vis", np.uint8, P), ("valid", np.int32, 1)), K_runs=runs)
        d = st["d"]
        if N:
            _stage_gate(st, box_rows)
            pu.fill_planes_frames(frames, offs, d["tex_pts"], d["tex_nv"], planes)

    def host(read: np.ndarray) -> Dict:
        return _stage_host_valid(bank, st, read, planes, True)

    return {"mask": st["r"]["mask"], "sketch": st["r"]["sketch"], "planes": planes, "tex_pts_d": d["tex_pts"].view(N, P, pu.MAX_VERTS, 2),
            "tex_nv_d": d["tex_nv"][:P] if N else d["tex_nv"], "vis_d": d["dst_vis"].view(N, P), "valid_d": d["valid"],
            "pose_d": d["pose"].view(N, 7), "buf": st["buf"], "host": host}


# ---------------------------------------------------------------------------------------------- trajectories
def tracking_box(row, shape, scale=None, img_scale=1.0) -> Tuple[int, int, int, int]:
    """The reference's box of a tracker's row (frame, id, x, y, w, h) as it is used everywhere a row becomes pixels
    (utils/bounding_box.py through GUI/app_interface.py:194 and utils/gps_utils.py:28): x, y, w, h times img_scale, each cut to an
    integer towards zero; x1 = x0 + w; with a scale, width and height grow by int(size * scale - size), half of it (floored) on
    each side; then x is clipped to [0, shape[0] - 1] and y to [0, shape[1] - 1] - shape is (width, height), as the reference
    passes it.  -> (x0, y0, x1, y1), Python integers."""
    x, y, w, h = (np.asarray(row, np.float64)[2:6] * img_scale).tolist()
    x0, y0 = int(x), int(y)
    x1, y1 = x0 + int(w), y0 + int(h)
    if scale is not None:
        if not scale > 0.0:
            raise ValueError(f"tracking_box: scale = {scale} must be positive")
        dw = int((x1 - x0) * scale - (x1 - x0))
        x0, x1 = x0 - dw // 2, x1 + dw // 2
        dh = int((y1 - y0) * scale - (y1 - y0))
        y0, y1 = y0 - dh // 2, y1 + dh // 2
    return max(0, x0), max(0, y0), min(shape[0] - 1, x1), min(shape[1] - 1, y1)


def _geodesic_m(p1, p2) -> float:
    """utils/gps_utils.py:7-16: the haversine distance of two (latitude, longitude) points in metres, Earth radius 6371 km."""
    dlon = np.radians(p1[1]) - np.radians(p2[1])
    dlat = np.radians(p1[0]) - np.radians(p2[0])
    a = np.sin(dlat / 2) ** 2 + np.cos(np.radians(p2[0])) * np.cos(np.radians(p1[0])) * np.sin(dlon / 2) ** 2
    return 6371.0 * (2 * np.arctan2(np.sqrt(a), np.sqrt(1 - a))) * 1000


def trajectories_to_meters(car_track, inv_homography, scale, shape, img_scale) -> np.ndarray:
    """utils/gps_utils.py:19-57 in its 'traj' mode: one vehicle's tracker rows [n, 6] -> its positions in metres [n, 2], float64,
    the same operations in the same order.  Per row the middle of the lower edge of `tracking_box` (x0 + (x1 - x0) // 2, y1) goes
    through the inverse homography to (latitude, longitude); the metres are each coordinate's share of the trajectory's own extent
    times the geodesic length of that extent's side.  A trajectory without extent in a coordinate divides zero by zero there: the
    values come back non-finite, as the reference's do."""
    H = np.asarray(inv_homography)
    gps = []
    for row in np.asarray(car_track):
        x0, _, x1, y1 = tracking_box(row, shape, scale, img_scale)
        mid = np.asarray([[x0 + (x1 - x0) // 2, y1, 1]])
        proj = (H @ mid.transpose()).transpose()[0]
        proj = proj / proj[2]
        gps.append(np.asarray(proj[:-1]))
    gps = np.asarray(gps)
    lo = [np.min(gps[:, 0]), np.min(gps[:, 1])]
    hi = [np.max(gps[:, 0]), np.max(gps[:, 1])]
    side = [_geodesic_m(hi, [lo[0], hi[1]]), _geodesic_m(hi, [hi[0], lo[1]])]
    meters = np.zeros(gps.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        meters[:, 0] = ((gps[:, 0] - lo[0]) / (hi[0] - lo[0])) * side[0]
        meters[:, 1] = ((gps[:, 1] - lo[1]) / (hi[1] - lo[1])) * side[1]
    return meters


def future_trajectories(trajectories, frame_id, ids, stride: int = 2, horizon: int = 5) -> List[np.ndarray]:
    """GUI/app_interface.py:225-234: per selected id the rows of that vehicle from frame_id on, every stride-th of them up to
    horizon future ones (rows 0, 2, ..., 10 of the vehicle's remaining rows: positions in its own table, so a vehicle the tracker
    lost for a frame is not re-timed) -> one [n, 6] array per id, n <= horizon + 1, shorter where the track ends early."""
    tr = np.asarray(trajectories, np.float64).reshape(-1, 6)
    out = []
    for i in ids:
        rows = tr[np.bitwise_and(tr[:, 1] == i, tr[:, 0] >= frame_id)]
        out.append(rows[0:stride * horizon + 1:stride])
    return out


def clip_from_trajectories(trajectories, frame_id, inv_homography, shape, bbox_scale=1.0, img_scale=1.0, stride: int = 2,
                           horizon: int = 5) -> Dict:
    """What a geometry-mode clip needs from a tracker's table (`VehiclePipeline.track_vehicles`' 'trajectories', or a parsed
    tracking file) at frame_id: {'ids' int64 [V] and 'bboxes' int64 [V, 4] (`tracking_box`, x0, y0, x1, y1) of the vehicles in
    that frame, in table order; 'steps': per future frame n = 1 .. the longest future, a list over the V vehicles of
    `trajectory_steps`' (theta, tr) for `trajectories_to_meters` of the vehicle's `future_trajectories` rows, None where the
    vehicle has no step n; 'rows': those rows per vehicle; 'skipped': the vehicles (positions in ids) with fewer than two rows or
    metres that are not finite (no extent in a coordinate, e.g. a vehicle that stands), which have no steps at all}.  The scene
    of future frame n takes scene['steps'] = the entries of steps[n - 1] of the vehicles it keeps."""
    tr = np.asarray(trajectories, np.float64).reshape(-1, 6)
    now = tr[tr[:, 0] == frame_id]
    ids = now[:, 1].astype(np.int64)
    bboxes = np.asarray([tracking_box(r, shape, bbox_scale, img_scale) for r in now], dtype=np.int64).reshape(-1, 4)
    rows = future_trajectories(tr, frame_id, ids, stride, horizon)
    per, skipped = [], []
    for v, r in enumerate(rows):
        m = trajectories_to_meters(r, inv_homography, bbox_scale, shape, img_scale) if len(r) >= 2 else None
        if m is None or not np.all(np.isfinite(m)):
            skipped.append(v)
            per.append([])
        else:
            per.append(trajectory_steps(m))
    n_future = max([len(p) for p in per], default=0)
    steps = [[p[n] if n < len(p) else None for p in per] for n in range(n_future)]
    return {"ids": ids, "bboxes": bboxes, "steps": steps, "rows": rows, "skipped": skipped}


def trajectory_steps(meter_coords) -> List[Tuple[float, np.ndarray]]:
    """trajectory_inference.py:256-297: a vehicle's future positions in metres [N, 2] (row 0 = now) -> (theta, tr) per
    future step n = 1 .. N-1, for `v @ z_rot(theta) + tr` (:360-363).  theta = heading of the step relative to the mean
    heading of the first 19 steps; tr = (0, -distance, 0) @ z_rot(theta), or @ z_rot(0) where the turn is sharp (the
    reference's +-20 degree gates: the step's instant turn for interior steps, theta itself for the first and the last two).
    `trajectories_to_meters` below gives the metres from a tracker's rows."""
    mc = np.asarray(meter_coords, np.float64).reshape(-1, 2)
    x_start, y_start = mc[0]
    theta_start = np.arctan2(np.mean(mc[1:20, 1] - y_start), np.mean(mc[1:20, 0] - x_start))
    last = len(mc[1:])
    steps = []
    for n, cur in enumerate(mc[1:], 1):
        distance = np.linalg.norm(mc[0] - cur)
        x_cur, y_cur = cur
        theta = np.arctan2(y_cur - y_start, x_cur - x_start) - theta_start
        delta_t = np.zeros(3)
        delta_t[1] = -distance                                       # get_delta_t_vec('y', -distance)
        if 1 < n < last - 1:
            cur_theta = np.degrees(np.arctan2(y_cur - mc[n - 1, 1], x_cur - mc[n - 1, 0]))
            next_theta = np.degrees(np.arctan2(mc[n + 1, 1] - y_cur, mc[n + 1, 0] - x_cur))
            straight = -20 < cur_theta - next_theta < 20
        else:
            straight = -20 < np.degrees(theta) < 20
        steps.append((float(theta), delta_t @ z_rot(theta if straight else 0)))
    return steps
