"""GPU: fusg_pose_geometry against its host twin on the cases of tests/pose_geometry_cases.py, and geometry mode with
VehiclePipeline(device_pose=True) against device_pose=False - run_frame, run_later_frame, with device_homography, replayed
and pipelined, no vehicles, and the count of blocking device-to-host copies of the front stage.

The tolerances are measured ones (profiles/pose_geometry_parity.json, written by tools/pose_geometry_parity.py from these very
cases and scenes): floats device vs host twin 8 x the largest difference seen, rendered bytes flag on vs off 10 x the share of
differing bytes seen (the ratio of DESIGN.md §7).  Every measured difference is 0 - the kernel equals its host twin bit for bit
and the two paths render the same bytes - so every bar is 0 and equality is asserted."""
import numpy as np
import pytest
import torch

import pose_geometry_cases as pc
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import ops
from future_urban_scene_generation_amd import render as R
from test_gpu_geometry_drivers import _later_scenes, _with_empty_vehicle
from test_gpu_render import DEV, _geometry_setup

# profiles/pose_geometry_parity.json, "device_vs_host" -> "bar_abs": 8 x the measured maximum absolute difference per output.
# All measured 0 (the device's cos / sin / acos gave glibc's bits on every case), so: equality.
DEVICE_BAR_ABS = {"extrinsic": 0.0, "kp3d": 0.0, "job.R": 0.0, "job.tr": 0.0, "job.E": 0.0, "job.fx": 0.0, "job.fy": 0.0, "job.cx": 0.0,
                  "job.cy": 0.0}
DEVICE_POSE_ULP = 1                     # float32 ulps between the device's pose and the host twin's (the issue's bound; measured 0)
# profiles/pose_geometry_parity.json, "flag_on_vs_off" -> "bar_share": 10 x the measured share of differing bytes per output.
# All measured 0 (first frame, later frame, with and without device_homography), so: equality ('masks' included, below 1e-3).
BYTE_BAR = {"masks": 0.0, "src_sketch": 0.0, "dst_sketch": 0.0, "src_planes": 0.0, "icn_u8": 0.0, "vunet_u8": 0.0, "frame_icn": 0.0,
            "frame_vunet": 0.0}
POSE_BAR_ULP = 1                        # run_frame's pose, flag on vs off: float32 ulps (the issue's bound; measured 0)
EMPTY = 1                               # the vehicle of the scene whose render is empty


def device_outputs(case):
    """fusg_pose_geometry on a case of pose_geometry_cases: the host twin's dict, computed by the kernel."""
    b = pc.bank()
    V = len(case["cad_idx"])
    arr = b.device_arrays(DEV)
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(DEV)      # noqa: E731
    raw = case["raw"] or (None, None, None)
    ins = [up(raw[0], np.float32), up(raw[1], np.float32), up(raw[2], np.float32), up(case["pose"], np.float32),
           up(case["kp_xy"], np.float32), up(case["steps"], np.float64)]
    cad = up(case["cad_idx"], np.int64)
    lay, nbytes = R._pg_layout(V)
    buf = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device=DEV)
    tdt = {"uint8": torch.uint8, "int32": torch.int32, "float32": torch.float32, "float64": torch.float64}
    d = {k: buf[o:o + n * dt.itemsize].view(tdt[dt.name]) for k, (o, dt, n) in lay.items()}
    K = np.ascontiguousarray(case["K"].reshape(9))
    ptr = lambda t: None if t is None else t.data_ptr()                                                               # noqa: E731
    with torch.cuda.device(DEV):
        L.check(L.lib().fusg_pose_geometry(*(ptr(t) for t in ins), cad.data_ptr(), arr["kp3d"].data_ptr(), arr["v_off"].data_ptr(),
                                           arr["t_off"].data_ptr(), len(b), K.ctypes.data, pc.H, pc.W, V,
                                           *(d[k].data_ptr() for k in R._PG_CALL), ops.stream_ptr()), "pose_geometry")
        host = buf.cpu().numpy()
    h = {k: host[o:o + n * dt.itemsize].view(dt) for k, (o, dt, n) in lay.items()}
    shapes = {"extrinsic": (V, 12), "kp3d": (V, 12, 3), "pose": (V, 7), "vis_pts": (V, 7, 8, 2), "vis_nv": (V, 7), "nearer": (V, 7),
              "tex_pts": (V, 5, 8, 2), "tex_nv": (V, 5), "status": (V,)}
    res = {k: h[k].reshape(sh) for k, sh in shapes.items()}
    res["jobs"] = h["jobs"].view(R.JOB_DTYPE)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(pc.cases()))
def test_kernel_matches_host_twin(name):
    case = pc.cases()[name]
    pc.reference(case)                                       # the precondition for comparing truncated integers exactly
    want, got = pc.host(case), device_outputs(case)
    for k in pc.INT_KEYS + ("status",):
        assert np.array_equal(got[k], want[k]), (name, k)
    for k in pc.JOB_INT:
        assert np.array_equal(got["jobs"][k], want["jobs"][k]), (name, k)
    fg, fw = pc.float_outputs(got), pc.float_outputs(want)
    print(f"{name}: pose ulp {pc.ulp32(fg['pose'], fw['pose'])}")
    assert pc.ulp32(fg["pose"], fw["pose"]) <= DEVICE_POSE_ULP, name
    for k in fg:
        if k == "pose":
            continue                                         # (float32: bounded in ulps above)
        ad, rel = pc.diffs(fg[k], fw[k])
        print(f"{name}: {k}: max abs {ad:.3g} rel {rel:.3g} (bar {DEVICE_BAR_ABS[k]:.3g})")
        assert ad <= DEVICE_BAR_ABS[k], (name, k, ad)


# ------------------------------------------------------------------------------------------------ the frame drivers
def byte_diff(a, b):
    """(share of differing bytes, largest level difference) of two uint8 tensors of one shape."""
    assert a.shape == b.shape and a.dtype == b.dtype == torch.uint8, (a.shape, b.shape)
    if a.numel() == 0:
        return 0.0, 0
    d = (a.to(torch.int16) - b.to(torch.int16)).abs()
    return float((d != 0).float().mean()), int(d.max())


def frame_bytes(out):
    """The rendered uint8 outputs of a run_frame / run_later_frame result by name."""
    g = out["geometry"]
    res = {k: g[k] for k in ("masks", "src_sketch", "dst_sketch", "src_planes") if k in g}
    res.update({k: out[k] for k in ("icn_u8", "vunet_u8", "frame_icn", "frame_vunet")})
    return res


def runs():
    """One pipeline, the flag switched between the runs (the networks and their packed weights are shared): first frame and one
    later frame with device_pose off / on / on with device_homography, V = 3 with vehicle EMPTY rendering empty."""
    pipe, bank, scene = _geometry_setup(V=3)
    scene = _with_empty_vehicle(pipe, bank, scene, EMPTY)
    res = {"pipe": pipe, "scene": scene}
    for tag, pose, hom in (("off", False, False), ("on", True, False), ("on_hom", True, True)):
        pipe.device_pose, pipe.device_homography = pose, hom
        first = pipe.run_frame(scene)
        if tag == "off":
            res["later_scene"] = _later_scenes(scene, first, n_frames=1)[0]
        res[tag] = first
        res[tag + "_later"] = pipe.run_later_frame(res["later_scene"], first["state"])
    pipe.device_pose, pipe.device_homography = False, False
    return res


@pytest.fixture(scope="module")
def frames():
    return runs()


def pose_rows(pose):
    return np.array([np.concatenate([[e], np.ravel(r), np.ravel(t)]) for e, r, t in pose], np.float32).reshape(len(pose), 7)


def same_host_keys(a, b, later, tag):
    assert a["skipped"] == b["skipped"] == [EMPTY], tag
    assert torch.equal(a["geom"], b["geom"]), tag
    ga, gb = a["geometry"], b["geometry"]
    for k in ("dst_kp",) + (() if later else ("src_kp",)):
        assert len(ga[k]) == len(gb[k]) == (2 if later else 3)        # (a later frame holds the vehicles the first one kept)
        for pa, pb in zip(ga[k], gb[k]):
            assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(pa, pb)), (tag, k)
    for k in ("dst_vis",) + (() if later else ("src_vis",)):
        assert np.array_equal(ga[k], gb[k]) and np.asarray(ga[k]).dtype == np.asarray(gb[k]).dtype, (tag, k)
    if not later:
        assert torch.equal(a["kp_idx"], b["kp_idx"]) and torch.equal(a["kp_xy"], b["kp_xy"]), tag
        assert np.array_equal(ga["cad_idx"], gb["cad_idx"]) and np.array_equal(ga["kp3d"], gb["kp3d"]), tag
        u = pc.ulp32(pose_rows(a["pose"]), pose_rows(b["pose"]))
        print(f"{tag}: pose ulp {u}")
        assert u <= POSE_BAR_ULP, tag
        assert all(p[1].shape == (3, 1) and p[1].dtype == np.float32 and p[2].shape == (3, 1) for p in a["pose"])


def same_bytes(a, b, tag):
    fa, fb = frame_bytes(a), frame_bytes(b)
    assert set(fa) == set(fb)
    for k in fa:
        share, level = byte_diff(fa[k], fb[k])
        print(f"{tag}: {k}: share of differing bytes {share:.3g}, max level difference {level} (bar {BYTE_BAR[k]:.3g})")
        assert BYTE_BAR["masks"] < 1e-3
        if BYTE_BAR[k] == 0:
            assert torch.equal(fa[k], fb[k]), (tag, k)
        else:
            assert share <= BYTE_BAR[k], (tag, k, share)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["on", "on_hom"])
def test_run_frame_flag_on_matches_off(frames, tag):
    same_host_keys(frames[tag], frames["off"], False, tag)
    same_bytes(frames[tag], frames["off"], tag)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["on", "on_hom"])
def test_run_later_frame_flag_on_matches_off(frames, tag):
    same_host_keys(frames[tag + "_later"], frames["off_later"], True, tag + "_later")
    same_bytes(frames[tag + "_later"], frames["off_later"], tag + "_later")
    st = frames[tag]["state"]["geometry"]
    assert st["pose_d"].is_cuda and st["cad_idx_d"].is_cuda and st["pose_d"].shape == (2, 7)      # kept on the device ...
    assert len(st["pose"]) == 2 and len(st["cad_idx"]) == 2                                        # ... beside the host copies
    assert np.array_equal(st["pose_d"].cpu().numpy(), pose_rows(st["pose"]))


@pytest.mark.gpu
def test_state_of_either_path_serves_the_other(frames):
    """A state made with the flag off drives a later frame with the flag on (its host copies are uploaded), and the reverse."""
    pipe = frames["pipe"]
    try:
        pipe.device_pose = True
        a = pipe.run_later_frame(frames["later_scene"], frames["off"]["state"])
        pipe.device_pose = False
        b = pipe.run_later_frame(frames["later_scene"], frames["on"]["state"])
    finally:
        pipe.device_pose = False
    same_host_keys(a, frames["off_later"], True, "off-state, flag on")
    same_bytes(a, frames["off_later"], "off-state, flag on")
    same_host_keys(b, frames["off_later"], True, "on-state, flag off")
    same_bytes(b, frames["off_later"], "on-state, flag off")


@pytest.mark.gpu
def test_replayed_and_pipelined_equal_run_frame(frames):
    """run_frames over two frames and run_frame(replay=True) with the flag: the same kernels in the same order as run_frame -
    byte for byte; run_later_frames likewise."""
    pipe, scene = frames["pipe"], frames["scene"]
    want = frames["on"]
    try:
        pipe.device_pose = True
        got = [pipe.run_frame(scene, replay=True)] + list(pipe.run_frames([scene, scene], replay=True))
        later = list(pipe.run_later_frames([frames["later_scene"]], want["state"], replay=True))
    finally:
        pipe.device_pose = False
    for i, o in enumerate(got):
        for k in ("kp_idx", "kp_xy", "icn_u8", "vunet_u8", "frame_icn", "frame_vunet", "geom"):
            assert torch.equal(o[k], want[k]), (i, k)
        for k in ("masks", "src_sketch", "src_planes"):
            assert torch.equal(o["geometry"][k], want["geometry"][k]), (i, k)
        assert o["skipped"] == [EMPTY] and np.array_equal(pose_rows(o["pose"]), pose_rows(want["pose"])), i
    assert len(later) == 1
    for k in ("icn_u8", "vunet_u8", "frame_icn", "frame_vunet", "geom"):
        assert torch.equal(later[0][k], frames["on_later"][k]), k
    assert later[0]["skipped"] == [EMPTY]


@pytest.mark.gpu
def test_no_vehicles_launches_nothing(frames, monkeypatch):
    pipe, scene = frames["pipe"], frames["scene"]
    empty = dict(scene, bboxes=np.zeros((0, 4), np.int64), cad_idx=np.zeros(0, np.int64), vehicle_seeds=[])
    lib = L.lib()
    launches = []
    for fn in ("fusg_pose_geometry", "fusg_render_normals_u8", "fusg_plane_visibility", "fusg_fill_poly_planes_batch_u8", "fusg_pnp_cpc"):
        real = getattr(lib, fn)
        monkeypatch.setattr(lib, fn, lambda *a, _r=real, _n=fn: (launches.append(_n), _r(*a))[1])
    copies = []
    real_d2h = ops.d2h
    monkeypatch.setattr(ops, "d2h", lambda t: (copies.append(1), real_d2h(t))[1])
    try:
        pipe.device_pose = True
        out = pipe.run_frame(empty)
    finally:
        pipe.device_pose = False
    assert launches == [] and copies == []
    assert out["pose"] == [] and out["skipped"] == [] and out["kp_idx"].shape[0] == 0 and out["icn_u8"].shape[0] == 0
    assert torch.equal(out["frame_icn"], scene["frame"]) and torch.equal(out["frame_vunet"], scene["frame"])
    assert out["geometry"]["masks"].shape[0] == 0 and "state" not in out          # (as with the flag off: nothing to carry on)


@pytest.mark.gpu
def test_front_stage_has_one_blocking_copy(frames, monkeypatch):
    """The front stage as the pipelined drivers issue it (`_issue_guarded`: no range-guard read-back of its own): every launch through the plane
    cut-outs around ONE blocking device-to-host copy - `ops.d2h` is called once, and nothing else in the stage brings a CUDA
    tensor to the host (Tensor.cpu / item / tolist are counted too).  With the flag off the same count is three or more."""
    pipe, scene = frames["pipe"], frames["scene"]
    counts = {"d2h": 0, "other": 0, "in_d2h": False, "after_d2h": []}
    real_d2h = ops.d2h

    def d2h(t):
        counts["d2h"] += 1
        counts["in_d2h"] = True
        try:
            return real_d2h(t)
        finally:
            counts["in_d2h"] = False

    def counted(name):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.is_cuda and not counts["in_d2h"]:
                counts["other"] += 1
            return real(self, *a, **k)
        return f

    monkeypatch.setattr(ops, "d2h", d2h)
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, counted(name))
    lib = L.lib()
    real_fill = lib.fusg_fill_poly_planes_batch_u8
    monkeypatch.setattr(lib, "fusg_fill_poly_planes_batch_u8", lambda *a: (counts["after_d2h"].append(counts["d2h"]), real_fill(*a))[1])

    def front(fn):
        """fn() issued as `_issue_geometry_front` issues a front stage: under the deferred range check of `_issue_guarded` (the
        status word follows through a pinned, non-blocking copy), then the ticket redeemed outside the count."""
        out, ticket = pipe._issue_guarded(fn, pipe._geo_word)
        seen = dict(counts)
        pipe._status_raised(ticket)
        counts.update(d2h=seen["d2h"], other=seen["other"])
        return out

    try:
        pipe.device_pose = True
        with torch.cuda.device(DEV):
            f = front(lambda: pipe._geometry_front(scene, None))
            assert (counts["d2h"], counts["other"]) == (1, 0), counts
            assert counts["after_d2h"] == [1]               # the plane cut-outs are queued behind the read-back
            st = pipe._geometry_state(f)
            st.update(appearance=[torch.zeros(2, 1, device=DEV)] * 2, central=torch.zeros(2, 1, device=DEV))
            front(lambda: pipe._geometry_later_front(frames["later_scene"],
                                                     {"geometry": st, "appearance": st["appearance"], "central": st["central"]}))
            assert (counts["d2h"], counts["other"]) == (2, 0), counts
        pipe.device_pose = False
        with torch.cuda.device(DEV):
            front(lambda: pipe._geometry_front(scene, None))
        assert counts["d2h"] == 2 and counts["other"] >= 3, counts
    finally:
        pipe.device_pose = False
    assert f["keep"] == [0, 2] and f["raw"] is None


@pytest.mark.gpu
def test_cad_idx_outside_the_bank_raises_after_the_read_back(frames):
    """`vehicle_geometry_device` with an index past the bank and a negative one: the kernel flags them, the render and the plane
    visibility run on their empty jobs (nv = nt = 0, nothing read out of range), and IndexError names the first after the one
    read-back - as `render_jobs` raises on the host path.  The same call with the indices in the bank goes through."""
    case = pc.cases()["bad_cad"]
    b = pc.bank()
    frame = torch.zeros((pc.H // 4, pc.W // 4, 3), dtype=torch.uint8, device=DEV)
    raw_d = tuple(torch.from_numpy(a).to(DEV) for a in case["raw"])
    kp_d = torch.from_numpy(case["kp_xy"]).to(DEV)
    call = lambda cad: R.vehicle_geometry_device(b, frame, torch.as_tensor(cad, dtype=torch.int64, device=DEV), case["K"],    # noqa: E731
                                                 raw_d=raw_d, kp_xy_d=kp_d)
    with pytest.raises(IndexError, match=f"mesh {len(b)} not in a bank of {len(b)}"):
        call(case["cad_idx"])
    g = call([1, 0, 2])
    assert g["status"].tolist() == [0, 0, 0] and g["cad_idx"].tolist() == [1, 0, 2] and g["masks"].shape[0] == 3
