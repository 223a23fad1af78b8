"""GPU: geometry mode (VehiclePipeline(cad_bank=...), scenes without 'masks') on the frame drivers - the batched plane cut-out
kernel, the vectorised vehicle_geometry, recorded-plan replay, run_frames / run_clip_frames with one frame in flight and the
fp32 redo of a frame whose range status is raised.  Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from future_urban_scene_generation_amd import render as R
from future_urban_scene_generation_amd.warp_learn import planes_utils as pu
from test_gpu_render import DEV, _geometry_setup

KEYS = ("kp_idx", "kp_xy", "icn_u8", "vunet_u8", "frame_icn", "frame_vunet")


def _same(a, b, tag=""):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), (tag, k)
    assert a["skipped"] == b["skipped"], tag
    assert len(a["pose"]) == len(b["pose"]), tag
    for p, q in zip(a["pose"], b["pose"]):
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(p, q)), tag


def _same_later(a, b, tag=""):
    for k in ("icn_u8", "vunet_u8", "frame_icn", "frame_vunet", "geom"):
        assert torch.equal(a[k], b[k]), (tag, k)
    assert a["skipped"] == b["skipped"], tag


def _with_empty_vehicle(pipe, bank, scene, v_empty):
    """The scene with vehicle v_empty drawn with a copy of its CAD model whose mesh lies 10^5 units away from its keypoints:
    same pose fit, empty render."""
    meshes = [(bank.vertices[m] / R.SCALE, bank.triangles[m], bank.kp3d[m] / R.SCALE) for m in range(len(bank))]
    m = int(scene["cad_idx"][v_empty])
    meshes.append((bank.vertices[m] / R.SCALE + 2e4, bank.triangles[m], bank.kp3d[m] / R.SCALE))
    pipe.cad_bank = R.CadBank(meshes)
    cad = np.array(scene["cad_idx"])
    cad[v_empty] = len(meshes) - 1
    return dict(scene, cad_idx=cad)


def _later_scenes(scene, out, n_frames=2, behind=1):
    """Later scenes along one trajectory; in the second, vehicle `behind` is moved behind the camera (renders empty)."""
    V = len(scene["bboxes"])
    steps = R.trajectory_steps(np.c_[np.arange(6.0) * 0.8, 0.05 * np.arange(6.0) ** 2])
    E = [R.extrinsic_from_pose(p[1], p[2]) for p in out["pose"]]
    res = []
    for n in range(n_frames):
        st = [steps[n]] * V
        if n == 1:
            st[behind] = (steps[n][0], -200.0 * np.asarray(E[behind][2, :3], np.float64))
        res.append({"frame": scene["frame"], "steps": st, "vehicle_seeds": [900 + 10 * n + v for v in range(V)]})
    return res


def _polygons(g, n_jobs, H, W):
    pts = np.zeros((n_jobs, 5, 8, 2), np.int32)
    nv = np.zeros((n_jobs, 5), np.int32)
    for j in range(n_jobs):
        for p in range(5):
            kind = (j * 5 + p) % 7
            n = int(g.integers(3, 9))
            c = g.uniform([-0.2 * W, -0.2 * H], [1.2 * W, 1.2 * H])
            v = c + g.normal(0, 0.15 * max(H, W), (n, 2))
            if kind == 1:                                             # off the frame
                v += np.array([3 * W, -2 * H])
            elif kind == 2:                                           # zero area: one point / a segment
                v = np.repeat(c[None], n, 0) if n % 2 else c + np.outer(np.arange(n), [3.0, 1.0])
            elif kind == 3:                                           # self-touching: a bow tie
                n = 4
                v = c + np.array([[0, 0], [40, 30], [40, 0], [0, 30]])
            elif kind == 4:                                           # covers the whole frame
                n = 4
                v = np.array([[-5, -5], [W + 5, -5], [W + 5, H + 5], [-5, H + 5]], np.float64)
            elif kind == 5:                                           # far off, large coordinates
                v = v * 64 - 1e6
            pts[j, p, :n] = np.int32(v[:n])
            nv[j, p] = n
    return pts, nv


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(720, 1280), (97, 131)])
def test_fill_poly_planes_batch_equals_per_job(hw):
    H, W = hw
    g = np.random.default_rng(H)
    frame = torch.from_numpy(g.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(DEV)
    for n_jobs in (7, 0):
        pts, nv = _polygons(g, n_jobs, H, W)
        out = torch.full((n_jobs, 5, H, W, 3), 77, dtype=torch.uint8, device=DEV)
        pu.fill_planes_batch(frame, torch.from_numpy(pts).to(DEV), torch.from_numpy(nv).to(DEV), out)
        again = torch.full_like(out, 13)
        pu.fill_planes_batch(frame, torch.from_numpy(pts).to(DEV), torch.from_numpy(nv).to(DEV), again)
        assert torch.equal(out, again)
        for j in range(n_jobs):
            want = pu.fill_planes(frame, [pts[j, p, :nv[j, p]] for p in range(5)])
            assert torch.equal(out[j], want), j
        if n_jobs:
            assert int(out.flatten(2).amax(2).min()) == 0 and int(out.max()) > 0     # empty planes and filled ones
            # a frame that is a strided view (every other column of a wider image) is read through its strides
            wide = torch.from_numpy(g.integers(0, 256, (H, 2 * W, 3), dtype=np.uint8)).to(DEV)[:, ::2]
            pu.fill_planes_batch(wide, torch.from_numpy(pts).to(DEV), torch.from_numpy(nv).to(DEV), out)
            assert torch.equal(out[3], pu.fill_planes(wide.contiguous(), [pts[3, p, :nv[3, p]] for p in range(5)]))


def _old_vehicle_geometry(bank, frame, mesh, poses, K, kp_xy=None, steps=None):
    """The per-vehicle form vehicle_geometry had before it was vectorised: extrinsics, visibility inputs, plane corners and
    one fill_planes per vehicle."""
    H, W = int(frame.shape[0]), int(frame.shape[1])
    V = len(mesh)
    E = [R.extrinsic_from_pose(r, t) for r, t in poses]
    if steps is None:
        Rs = trs = None
        kp3d = [bank.kp3d[int(m)] for m in mesh]
    else:
        Rs = [R.z_rot(th) for th, _ in steps]
        trs = [np.asarray(t, np.float64).reshape(3) for _, t in steps]
        kp3d = [bank.kp3d[int(m)] @ Rs[v] + trs[v] for v, m in enumerate(mesh)]
    r = R.render_vehicles(bank, mesh, E, float(K[0, 0]), float(K[1, 1]), (H, W), DEV, Rs, trs)
    ins = [R.visibility_inputs(kp3d[v], E[v], K) for v in range(V)]
    pts, nv, near = (torch.from_numpy(np.stack([i[k] for i in ins])).to(DEV) for k in range(3))
    counts = torch.zeros((V, 7, 2), dtype=torch.int32, device=DEV)
    from future_urban_scene_generation_amd import _lib as L, ops
    L.check(L.lib().fusg_plane_visibility(pts.data_ptr(), nv.data_ptr(), near.data_ptr(), V, H, W, counts.data_ptr(),
                                          ops.stream_ptr()), "plane_visibility")
    vis = R.visible(counts.cpu().numpy())[:, :5].astype(np.uint8)
    out = {"masks": r["mask"], "covered": r["covered"].cpu().numpy().astype(np.int64), "kp3d": np.stack(kp3d),
           "extrinsic": np.stack(E), "counts": counts.cpu().numpy()}
    if steps is None:
        kp = [R.plane_corners(kp_xy[v], (H, W)) for v in range(V)]
        out.update(src_sketch=r["sketch"], dst_sketch=r["sketch"], src_planes=torch.stack([pu.fill_planes(frame, k) for k in kp]),
                   src_kp=kp, dst_kp=kp, src_vis=vis, dst_vis=vis)
    else:
        kp = [R.plane_corners(R.project_keypoints(kp3d[v], *poses[v], K), (H, W)) for v in range(V)]
        out.update(dst_sketch=r["sketch"], dst_kp=kp, dst_vis=vis)
    return out


def _geq(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for k in a:
        x, y = a[k], b[k]
        if torch.is_tensor(x):
            assert torch.equal(x, y), k
        elif isinstance(x, list):
            assert len(x) == len(y), k
            for u, w in zip(x, y):
                assert all(np.array_equal(p, q) and p.dtype == q.dtype for p, q in zip(u, w)), k
        else:
            assert np.asarray(x).dtype == np.asarray(y).dtype and np.array_equal(x, y), k


@pytest.mark.gpu
def test_vehicle_geometry_equals_per_vehicle_path():
    pipe, bank, scene = _geometry_setup(V=6, seed=33)
    out = pipe.run_frame(scene)
    K = R.intrinsic(scene["focals"], scene["centers"])
    mesh = list(scene["cad_idx"])
    poses = [(p[1], p[2]) for p in out["pose"]]
    kp_xy = out["kp_xy"].cpu().numpy()
    _geq(R.vehicle_geometry(bank, scene["frame"], mesh, poses, K, kp_xy=kp_xy),
         _old_vehicle_geometry(bank, scene["frame"], mesh, poses, K, kp_xy=kp_xy))
    for later in _later_scenes(scene, out):
        _geq(R.vehicle_geometry(bank, scene["frame"], mesh, poses, K, steps=later["steps"]),
             _old_vehicle_geometry(bank, scene["frame"], mesh, poses, K, steps=later["steps"]))
    g0 = R.vehicle_geometry(bank, scene["frame"], [], [], K, kp_xy=np.zeros((0, 12, 2), np.float32))
    assert g0["src_planes"].shape[0] == 0 and g0["masks"].shape[0] == 0


@pytest.mark.gpu
def test_geometry_replay_equals_eager():
    pipe, bank, scene = _geometry_setup()
    eager = pipe.run_frame(scene)
    laters = _later_scenes(scene, eager)
    eager_l = [pipe.run_later_frame(sc, eager["state"]) for sc in laters]
    for rep in range(2):                                              # the second replay hits the recorded plan
        got = pipe.run_frame(scene, replay=True)
        _same(got, eager, f"first replay {rep}")
        for n, sc in enumerate(laters):
            _same_later(pipe.run_later_frame(sc, got["state"], replay=True), eager_l[n], f"later {n} replay {rep}")
    assert any(k[0] == 4 and "kp_given" in k for k in pipe._frame_plans if isinstance(k[0], int))
    # a vehicle whose render is empty: 3 kept vehicles, another plan
    sc2 = _with_empty_vehicle(pipe, bank, scene, 2)
    eager2 = pipe.run_frame(sc2)
    assert eager2["skipped"] == [2] and eager2["icn_u8"].shape[0] == 3
    _same(pipe.run_frame(sc2, replay=True), eager2, "empty vehicle")
    assert any(k[0] == 3 and "kp_given" in k for k in pipe._frame_plans if isinstance(k[0], int))


@pytest.mark.gpu
def test_geometry_run_frames_and_clip_frames():
    pipe, bank, scene = _geometry_setup()
    sc_b = dict(scene, vehicle_seeds=[50 + v for v in range(4)])
    sc_c = _with_empty_vehicle(pipe, bank, scene, 0)
    scenes = [scene, sc_c, sc_b]
    want = [pipe.run_frame(sc) for sc in scenes]
    assert want[1]["skipped"] == [0]
    for replay in (False, True):
        got = list(pipe.run_frames(scenes, replay=replay))
        assert len(got) == 3
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"run_frames {i} replay={replay}")
    got = list(pipe.run_frames(iter(scenes), replay=True))          # scenes drawn one by one
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"run_frames iterator {i}")
    first = pipe.run_frame(scene)
    laters = _later_scenes(scene, first)
    want_l = [pipe.run_later_frame(sc, first["state"]) for sc in laters]
    assert want_l[1]["skipped"] == [1]
    for replay in (False, True):
        clip = list(pipe.run_clip_frames(scene, laters, replay=replay))
        assert len(clip) == 3
        _same(clip[0], first, "clip first")
        for n in range(2):
            _same_later(clip[1 + n], want_l[n], f"clip later {n} replay={replay}")
        got_l = list(pipe.run_later_frames(laters, clip[0]["state"], replay=replay))
        for n in range(2):
            _same_later(got_l[n], want_l[n], f"later frames {n} replay={replay}")


@pytest.mark.gpu
def test_geometry_run_frames_redoes_an_out_of_range_frame_in_fp32():
    from future_urban_scene_generation_amd import ops
    pipe, bank, scene = _geometry_setup()
    with ops.precision("f32"):
        f32 = pipe.run_frame(scene, check=None)
    h16 = pipe.run_frame(scene)
    calls = {"n": 0}
    orig = pipe._run_frame

    def flagged(sc, replay=False):                                    # raise the networks' status on the 2nd frame only
        out = orig(sc, replay)
        calls["n"] += 1
        if calls["n"] == 2:
            ops.status_word(DEV)[0] = 1
        return out

    pipe._run_frame = flagged
    try:
        got = list(pipe.run_frames([scene, scene, scene]))
    finally:
        pipe._run_frame = orig
    _same(got[0], h16, "frame 0")
    _same(got[2], h16, "frame 2")
    _same(got[1], f32, "frame 1 (fp32)")
    # the same through the geometry stage's own status word (the keypoint stage of the 2nd frame)
    front = pipe._geometry_front
    calls["n"] = 0

    def flagged_front(sc, check):
        out = front(sc, check)
        calls["n"] += 1
        if calls["n"] == 2:
            ops.status_word(DEV)[0] = 1
        return out

    pipe._geometry_front = flagged_front
    try:
        got = list(pipe.run_frames([scene, scene, scene]))
    finally:
        del pipe._geometry_front
    _same(got[0], h16, "frame 0 (front)")
    _same(got[2], h16, "frame 2 (front)")
    _same(got[1], f32, "frame 1 (front, fp32)")
    # later frames of a geometry clip: the 2nd one redone in fp32
    laters = _later_scenes(scene, h16) + _later_scenes(scene, h16)[:1]
    with ops.precision("f32"):
        want1 = pipe.run_later_frame(laters[1], h16["state"], check=None)
    want = [pipe.run_later_frame(sc, h16["state"]) for sc in laters]
    orig_l = pipe._run_later_frame
    calls["n"] = 0

    def flagged_l(sc, st, replay=False):
        out = orig_l(sc, st, replay)
        calls["n"] += 1
        if calls["n"] == 2:
            ops.status_word(DEV)[0] = 1
        return out

    pipe._run_later_frame = flagged_l
    try:
        got = list(pipe.run_later_frames(laters, h16["state"]))
    finally:
        pipe._run_later_frame = orig_l
    _same_later(got[0], want[0], "later 0")
    _same_later(got[2], want[2], "later 2")
    _same_later(got[1], want1, "later 1 (fp32)")
