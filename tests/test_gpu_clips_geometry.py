"""GPU: the future frames of SEVERAL geometry-mode clips as ONE batched, read-back-free pass
(VehiclePipeline.run_later_clips_batched_geometry, render.later_geometry_clips_device, fusg_pose_geometry_clips).  The kernel equals
its host twin byte for byte; the several-clip stage equals the one-clip stage (`render.later_geometry_batch_device`) on each clip's rows, one
clip on a second camera and one row inert; the derived keys fed back as explicit given-geometry clips of the same rows give the
same bytes (that path is tied to the CPU oracle by tests/test_gpu_clips_batch.py and tests/test_gpu_later_batch.py); one
device-to-host copy per group; replay shares the given-geometry plan; the range guard; inpainting; whole clips."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pose_geometry_cases as pc                                           # noqa: E402
from future_urban_scene_generation_amd import _lib as L                    # noqa: E402
from future_urban_scene_generation_amd import ops                          # noqa: E402
from future_urban_scene_generation_amd import pipeline as pl               # noqa: E402
from future_urban_scene_generation_amd import render as R                  # noqa: E402
from test_clips_geometry_cpu import OUT_KEYS, PER, make_clips              # noqa: E402
from test_gpu_later_geometry_batch import _explicit_scenes, _later_scenes, _same_as_explicit, _setup   # noqa: E402

DEV = "cuda:0"
HW = (360, 640)
KEYS = ("icn_u8", "vunet_u8", "geom", "frame_icn", "frame_vunet")
SHAPES = [(2, 2), (1, 3), (3, 1), (0, 2)]                                    # (F_c, V_c): 10 rows, and a clip without frames
VEHICLES = [[0, 1], [1, 2, 3], [2], [0, 3]]                                  # the setup scene's vehicles each clip's first frame holds
CAMERA2, INERT = 0, (1, 0, 1)                                                # the clip on a second camera; (clip, frame, vehicle) behind the camera
N = sum(f * v for f, v in SHAPES)


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _device_rows(clips, guard=1):
    """fusg_pose_geometry_clips on host-array clips (test_clips_geometry_cpu.make_clips): the host twin's dict, computed by the
    kernel into buffers with `guard` rows of 0x5A behind each output; returns (outputs, guard rows)."""
    b = pc.bank()
    arr = b.device_arrays(DEV)
    n = len(clips)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(DEV)             # noqa: E731
    pose, cad, pts = ([up(cl[k], dt) for cl in clips] for k, dt in (("pose", np.float32), ("cad_idx", np.int64), ("src_pts", np.int32)))
    first = [0]
    for cl in clips:
        first.append(first[-1] + cl["steps"].shape[0])
    J = first[-1]
    steps = up(np.concatenate([cl["steps"] for cl in clips]).reshape(-1, 4), np.float64)
    cams = up(np.concatenate([np.asarray(cl["K"], np.float64).reshape(9) for cl in clips]), np.float64)
    names = OUT_KEYS + ("src_pts_rows",)
    outs = {k: torch.full(((J + guard) * PER[k][1] * np.dtype(PER[k][0]).itemsize,), 0x5A, dtype=torch.uint8, device=DEV) for k in names}
    tab = lambda ts: (C.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in ts])              # noqa: E731
    with torch.cuda.device(DEV):
        L.check(L.lib().fusg_pose_geometry_clips(tab(pose), tab(cad), tab(pts), (C.c_int32 * n)(*[int(t.shape[0]) for t in cad]),
                                                 (C.c_int32 * (n + 1))(*first), n, steps.data_ptr(), cams.data_ptr(), arr["kp3d"].data_ptr(),
                                                 arr["v_off"].data_ptr(), arr["t_off"].data_ptr(), len(b), pc.H, pc.W, J,
                                                 *(outs[k].data_ptr() for k in names), ops.stream_ptr()), "pose_geometry_clips")
        host = {k: o.cpu().numpy() for k, o in outs.items()}
    got, tail = {}, {}
    for k in names:
        nb = J * PER[k][1] * np.dtype(PER[k][0]).itemsize
        got[k], tail[k] = host[k][:nb], host[k][nb:]
    return got, tail


@pytest.mark.parametrize("J, shapes", [(1, [(1, 1)]), (64, [(2, 2), (1, 3), (3, 1), (0, 2), (2, 0), (54, 1)]),
                                       (65, [(0, 3), (2, 2), (1, 3), (3, 1), (11, 5)]), (200, [(5, 3)] * 13 + [(5, 1)])],
                         ids=["J1", "J64", "J65", "J200"])
def test_kernel_equals_the_host_twin(J, shapes):
    """One row; 64 and 65 rows (one whole block of 64 threads, and one row into the next); 200 rows of 14 clips (four blocks)."""
    clips = make_clips(shapes, seed=J)
    assert sum(f * v for f, v in shapes) == J
    want = R.pose_geometry_clips_host(pc.bank(), (pc.H, pc.W), clips)
    got, tail = _device_rows(clips)
    for k in OUT_KEYS + ("src_pts_rows",):
        assert np.array_equal(got[k], np.ascontiguousarray(want[k]).reshape(-1).view(np.uint8)), (J, k)
        assert tail[k].size and (tail[k] == 0x5A).all(), (J, k)
    assert (want["status"] == 0).all()


# ------------------------------------------------------------------------------------------------ the clips
def _sub_scene(scene, idx, second_camera=False):
    """The setup scene restricted to the vehicles `idx`; second_camera: centers shifted by a few pixels, focals scaled by 2 %."""
    sc = {"frame": scene["frame"], "bboxes": np.asarray(scene["bboxes"])[idx], "focals": np.asarray(scene["focals"], np.float64),
          "centers": np.asarray(scene["centers"], np.float64), "cad_idx": np.asarray(scene["cad_idx"])[idx],
          "vehicle_seeds": [scene["vehicle_seeds"][v] for v in idx]}
    if second_camera:
        sc["focals"] = sc["focals"] * 1.02
        sc["centers"] = sc["centers"] + np.array([3.0, -2.0])
    return sc


def _clip_later(sub, first, c):
    """Clip c's later scenes: `_later_scenes` on its own images and seeds, the inert vehicle where INERT says."""
    F, V = SHAPES[c]
    later = _later_scenes(sub, first, F, V, INERT[1:] if c == INERT[0] else (-1, 0))
    for n, sc in enumerate(later):
        sc["frame"] = torch.roll(sc["frame"], shifts=11 * (c + 1), dims=0).contiguous()
        sc["vehicle_seeds"] = [1000 * (c + 1) + s for s in sc["vehicle_seeds"]]
    return later


def _explicit_clips(env, got):
    return [(_explicit_scenes(later, g, first), dict(st, geometry=None))
            for (later, st), g, first in zip(env["clips"], got, env["firsts"])]


def _same_clips(got, want, tag, keys=KEYS):
    assert len(got) == len(want)
    for c, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), (tag, c)
        for f, (x, y) in enumerate(zip(a, b)):
            assert x["skipped"] == y["skipped"], (tag, c, f)
            for k in keys:
                assert x[k].shape == y[k].shape and torch.equal(x[k], y[k]), (tag, c, f, k)


@pytest.fixture(scope="module")
def env():
    """One geometry-mode pipeline (device_pose and device_homography on); four first frames over the vehicles VEHICLES of one
    scene, clip CAMERA2's on a second camera; their tails of SHAPES frames with INERT behind the camera; and - computed once - the
    batched result, the explicit clips built from it and their given-geometry result."""
    pipe, bank, scene = _setup(4)
    subs = [_sub_scene(scene, idx, c == CAMERA2) for c, idx in enumerate(VEHICLES)]
    firsts = [pipe.run_frame(sc) for sc in subs]
    for c, f in enumerate(firsts):
        assert f["skipped"] == [] and f["state"]["geometry"].get("pose_d") is not None, c
        assert int(f["state"]["central"].shape[0]) == len(VEHICLES[c]) == SHAPES[c][1]
    K = [R.intrinsic(f["state"]["geometry"]["focals"], f["state"]["geometry"]["centers"]) for f in firsts]
    assert not np.array_equal(K[CAMERA2], K[1]) and np.array_equal(K[1], K[2])
    clips = [(_clip_later(sub, f, c), f["state"]) for c, (sub, f) in enumerate(zip(subs, firsts))]
    assert [len(scs) for scs, _ in clips] == [f for f, _ in SHAPES]
    e = dict(pipe=pipe, bank=bank, scene=scene, subs=subs, firsts=firsts, clips=clips)
    e["got"] = pipe.run_later_clips_batched_geometry(clips)
    e["explicit"] = _explicit_clips(e, e["got"])
    e["ex"] = pipe.run_later_clips_batched(e["explicit"])
    return e


def _inert_row():
    c, f, v = INERT
    offs = pl.clip_batch_offsets(*zip(*SHAPES))
    return pl.clip_batch_row(offs, [v_ for _, v_ in SHAPES], c, f, v)


# ------------------------------------------------------------------------------------------------ 2. the stage
def _per_clip_stage(pipe, scs, st):
    """The one-clip device stage of a clip's tail (`render.later_geometry_batch_device` at F * V rows, frame-major) and what the
    plane homographies need besides: the state's source corner points and visibilities repeated F times."""
    gs = st["geometry"]
    veh, F = list(gs["vehicles"]), len(scs)
    sd = pipe._geometry_state_device(gs)
    one = R.later_geometry_batch_device(pipe.cad_bank, HW, sd["cad_idx_d"], sd["pose_d"], R.intrinsic(gs["focals"], gs["centers"]),
                                        [[sc["steps"][v] for v in veh] for sc in scs])
    vis = torch.from_numpy((np.asarray(gs["src_vis"]).reshape(len(veh), -1) != 0).astype(np.uint8)).to(DEV)
    one.update(src_kp_d=sd["src_kp_d"].repeat(F, 1, 1, 1), src_vis_d=vis.repeat(F, 1), kp_nv_d=sd["kp_nv_d"])
    return one


def test_stage_equals_the_per_clip_stage(env):
    pipe, clips = env["pipe"], env["clips"]
    live = [(scs, st) for scs, st in clips if scs]
    n = []
    orig = ops.d2h
    ops.d2h = lambda t: (n.append(int(t.numel())), orig(t))[1]
    try:
        geo = pipe._later_clips_geometry_stage(live)
    finally:
        ops.d2h = orig
    assert n == []                                                # the stage reads nothing back
    host = geo["host"](ops.d2h(geo["buf"]))
    assert tuple(geo["mask"].shape) == (N,) + HW and tuple(geo["sketch"].shape) == (N,) + HW + (3,)
    assert tuple(geo["src_kp_d"].shape) == (N, 5, 8, 2) and tuple(geo["src_vis_d"].shape) == (N, 5) and tuple(geo["kp_nv_d"].shape) == (5,)
    assert np.array_equal(host["status"], np.zeros(N, np.int32))
    offs = pl.clip_batch_offsets(*zip(*SHAPES))
    for c, (scs, st) in enumerate(live):
        F, V = SHAPES[c]
        sl = slice(offs[c], offs[c + 1])
        one = _per_clip_stage(pipe, scs, st)
        h1 = one["host"](ops.d2h(one["buf"]))
        for k in ("mask", "sketch", "tex_pts_d", "dst_vis_d", "valid_d", "src_kp_d", "src_vis_d"):
            a = geo[k][sl]
            assert a.shape == one[k].shape and a.dtype == one[k].dtype and torch.equal(a, one[k]), (c, k)
        assert torch.equal(geo["kp_nv_d"], one["kp_nv_d"]) and torch.equal(geo["tex_nv_d"], one["tex_nv_d"])
        for k in ("dst_vis", "kp3d", "covered", "valid", "cad_idx", "pose"):
            a = np.asarray(host[k])[sl]
            assert a.dtype == np.asarray(h1[k]).dtype and np.array_equal(a, h1[k]), (c, k)
        for r in range(F * V):
            assert len(host["dst_kp"][sl][r]) == len(h1["dst_kp"][r]) == 5
            for a, b in zip(host["dst_kp"][sl][r], h1["dst_kp"][r]):
                assert a.dtype == b.dtype and np.array_equal(a, b), (c, r)
    r = _inert_row()
    valid, gated = geo["valid_d"].cpu().numpy(), geo["dst_vis_d"].cpu().numpy()
    assert int(valid[r]) == 0 and int(host["covered"][r]) == 0 and not gated[r].any()
    assert not geo["mask"][r].any() and not geo["sketch"][r].any()
    assert valid.sum() == N - 1 and gated.any()


# ------------------------------------------------------------------------------------------------ 3. the explicit clips
def test_derived_keys_fed_back_as_explicit_clips_give_the_same_bytes(env):
    """The same rows at the same row count through the given-geometry several-clip path: no tolerance."""
    c, f, v = INERT
    e = env["explicit"][c][0][f]
    assert e["dst_vis"][v].sum() == 0 and not e["masks"][v].any()
    assert len(env["ex"]) == len(SHAPES) and env["ex"][3] == []
    for c, (F, V) in enumerate(SHAPES):
        assert all(tuple(x["icn_u8"].shape) == (V, 256, 256, 3) for x in env["ex"][c])
        _same_as_explicit(env["got"][c], env["ex"][c], V, f"clip {c}")
    assert not torch.equal(env["got"][0][0]["frame_icn"], env["got"][2][0]["frame_icn"])


# ------------------------------------------------------------------------------------------------ 4. the result's shape
def test_results_have_the_one_clip_shape(env):
    pipe, got = env["pipe"], env["got"]
    assert isinstance(got, list) and len(got) == len(SHAPES) and got[3] == []
    for c, (scs, st) in enumerate(env["clips"]):
        want = pipe.run_later_frames_batched_geometry(scs, st)
        assert len(got[c]) == len(want) == SHAPES[c][0]
        for f, (a, b) in enumerate(zip(got[c], want)):
            assert set(a) == set(b) == set(KEYS) | {"geometry", "skipped"} and a["skipped"] == b["skipped"], (c, f)
            assert a["skipped"] == ([INERT[2]] if (c, f) == INERT[:2] else [])
            for k in KEYS:
                assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (c, f, k)
            assert set(a["geometry"]) == set(b["geometry"]) == {"masks", "dst_sketch", "dst_kp", "dst_vis", "kp3d"}
            for k in ("masks", "dst_sketch"):
                assert torch.equal(a["geometry"][k], b["geometry"][k]), (c, f, k)
            for k in ("dst_vis", "kp3d"):
                assert np.array_equal(a["geometry"][k], b["geometry"][k]), (c, f, k)
    assert not any(k[0] in ("later_rows", "later_batch") for k in pipe._frame_plans)      # the eager form records nothing


# ------------------------------------------------------------------------------------------------ 5. the read-back
def test_one_read_back_per_group(env):
    pipe, clips = env["pipe"], env["clips"]
    groups = pl.clip_batch_groups(*zip(*SHAPES), 6)
    assert groups == [(0, 1, False), (1, 4, False)]
    n = []
    orig = ops.d2h
    ops.d2h = lambda t: (n.append(int(t.numel())), orig(t))[1]
    try:
        pipe.run_later_clips_batched_geometry(clips)
        one = list(n)
        del n[:]
        two_res = pipe.run_later_clips_batched_geometry(clips, max_batch=6)
        two = list(n)
        del n[:]
        for scs, st in clips:
            pipe.run_later_frames_batched_geometry(scs, st)
        per_clip = list(n)
    finally:
        ops.d2h = orig
    assert len(one) == 1 and len(two) == len(groups) and one[0] > two[1] > two[0]
    assert len(per_clip) == 3                                     # clip by clip: one blocking copy per clip that has frames
    for c in range(len(SHAPES)):                                  # the groups in clip order, the stage's bytes unchanged
        for a, b in zip(two_res[c], env["got"][c]):
            assert a["skipped"] == b["skipped"] and torch.equal(a["geometry"]["masks"], b["geometry"]["masks"])
    ex = pipe.run_later_clips_batched(env["explicit"], max_batch=6)
    for c, (F, V) in enumerate(SHAPES):
        _same_as_explicit(two_res[c], ex[c], V, f"max_batch 6 clip {c}")


# ------------------------------------------------------------------------------------------------ 6. replay
def test_replay_equals_padded_eager_and_shares_the_given_geometry_plan(env):
    pipe, clips = env["pipe"], env["clips"]
    key = ("later_rows", 16, ops.PRECISION)
    assert pl.frame_batch_pad(N) == 16 and not any(k[0] == "later_rows" for k in pipe._frame_plans)
    eager = pipe.run_later_clips_batched_geometry(clips, pad=True)
    assert not any(k[0] == "later_rows" for k in pipe._frame_plans)
    r1 = pipe.run_later_clips_batched_geometry(clips, replay=True)
    assert [k for k in pipe._frame_plans if k[0] == "later_rows"] == [key]
    plan = pipe._frame_plans[key]
    r2 = pipe.run_later_clips_batched_geometry(clips, replay=True)
    ex = pipe.run_later_clips_batched(_explicit_clips(env, eager), replay=True)    # a given-geometry group of the same padded shape
    assert [k for k in pipe._frame_plans if k[0] == "later_rows"] == [key] and pipe._frame_plans[key] is plan
    _same_clips(r1, eager, "first replay")
    _same_clips(r2, eager, "second replay")
    for c, (F, V) in enumerate(SHAPES):
        _same_as_explicit(eager[c], ex[c], V, f"replayed explicit clip {c}")
    pipe._frame_plans.pop(key)


# ------------------------------------------------------------------------------------------------ 7. the range guard
def test_range_guard_redoes_the_group_in_fp32(env):
    """An appearance code outside the split-fp16 range: the status word is raised once, and the results are those of an
    exact-fp32 run of the same rows, bit for bit."""
    pipe = env["pipe"]
    hot = dict(env["clips"][2][1])
    hot["appearance"] = [t.clone() for t in hot["appearance"]]
    hot["appearance"][1][0, 0, 0, 0] = 6e4
    clips = [cl if c != 2 else (cl[0], hot) for c, cl in enumerate(env["clips"])]
    with ops.precision("f32"):
        f32 = pipe.run_later_clips_batched_geometry(clips, check=None)
    raised = []
    orig = ops.range_exceeded
    ops.range_exceeded = lambda *a, **k: (raised.append(orig(*a, **k)), raised[-1])[1]
    try:
        got = pipe.run_later_clips_batched_geometry(clips)
    finally:
        ops.range_exceeded = orig
    assert raised == [True]                                       # one status word, read once, for the whole group
    _same_clips(got, f32, "fp32 redo")
    assert any(not torch.equal(a["vunet_u8"], b["vunet_u8"]) for a, b in zip(got[2], env["got"][2]))
    assert not ops.range_exceeded(DEV) and not ops.range_exceeded(DEV, word=pipe.status_word())


# ------------------------------------------------------------------------------------------------ 8. an oversized clip
def test_an_oversized_clip_goes_through_the_one_clip_method(env):
    pipe, clips = env["pipe"], env["clips"]
    assert pl.clip_batch_groups([2, 3], [2, 1], 3) == [(0, 1, True), (1, 2, False)]
    calls = []
    orig = pipe._run_later_clips
    pipe._run_later_clips = lambda cl, *a: (calls.append((len(cl[0][0]), a[3] if len(a) > 3 else None)), orig(cl, *a))[1]
    try:
        got = pipe.run_later_clips_batched_geometry([clips[0], clips[2]], max_batch=3)
    finally:
        del pipe._run_later_clips
    # clip 0 (4 rows) is no group of the several-clip driver: the one-clip method splits it by frames, under its own plan key;
    # clip 2 alone is a group of the several-clip driver, under the default key
    assert calls == [(1, ("later_batch", 1, 2)), (1, ("later_batch", 1, 2)), (3, None)]
    want = pipe.run_later_frames_batched_geometry(*clips[0], max_batch=3)
    _same_clips([got[0]], [want], "oversized")
    _same_clips([got[1]], pipe.run_later_clips_batched_geometry([clips[2]]), "the clip behind it")


def test_a_state_without_device_copies_uploads_its_host_tables(env):
    pipe = env["pipe"]
    drop = ("pose_d", "cad_idx_d", "src_kp_d", "kp_nv_d")
    clips = [(scs, dict(st, geometry={k: v for k, v in st["geometry"].items() if k not in drop})) for scs, st in env["clips"]]
    _same_clips(pipe.run_later_clips_batched_geometry(clips), env["got"], "host-only states")


def test_a_clip_without_vehicles_between_live_clips(env):
    """V_c = 0: the no-vehicle shape of the one-clip method, its composites equal to their base; the clips around it are the bytes
    of the same rows without it."""
    pipe, clips = env["pipe"], env["clips"]
    empty = _sub_scene(env["scene"], [])
    first = pipe.run_frames_batched_geometry([empty])[0]
    state = first["state"]
    assert int(state["central"].shape[0]) == 0 and list(state["geometry"]["vehicles"]) == []
    later = [{"frame": torch.roll(env["scene"]["frame"], shifts=19 * (n + 1), dims=1).contiguous(), "steps": [], "vehicle_seeds": []}
             for n in range(2)]
    got = pipe.run_later_clips_batched_geometry([clips[2], (later, state), clips[1]])
    want = pipe.run_later_frames_batched_geometry(later, state)
    assert len(got[1]) == len(want) == 2
    for a, b, sc in zip(got[1], want, later):
        assert set(a) == set(b) and a["skipped"] == b["skipped"] == [] and set(a["geometry"]) == set(b["geometry"])
        for k in KEYS:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        assert a["icn_u8"].shape[0] == 0 and torch.equal(a["frame_icn"], sc["frame"]) and torch.equal(a["frame_vunet"], sc["frame"])
    _same_clips([got[0], got[2]], pipe.run_later_clips_batched_geometry([clips[2], clips[1]]), "around the empty clip")
    # only clips without rows: nothing is launched for them either
    assert pipe.run_later_clips_batched_geometry([(later, state), clips[3]])[1] == []


# ------------------------------------------------------------------------------------------------ 10. whole clips, fallbacks
def test_whole_clips_and_fallbacks(env):
    pipe, subs, clips = env["pipe"], env["subs"], env["clips"]
    pairs = [(sub, scs) for sub, (scs, _) in zip(subs, clips)]
    whole = pipe.run_clips_batched_geometry(pairs)
    firsts = pipe.run_frames_batched_geometry(subs)
    tails = pipe.run_later_clips_batched_geometry([(scs, f["state"]) for (scs, _), f in zip(clips, firsts)])
    assert [len(w) for w in whole] == [1 + f for f, _ in SHAPES]
    for c, w in enumerate(whole):
        assert w[0]["skipped"] == firsts[c]["skipped"]
        for k in ("kp_idx", "icn_u8", "vunet_u8", "frame_icn", "frame_vunet"):
            assert torch.equal(w[0][k], firsts[c][k]), (c, k)
    _same_clips([w[1:] for w in whole], tails, "whole clips")
    # batch_geometry=False: `run_later_clips_batched`, which takes geometry-mode clips one by one, frame by frame
    two = [clips[1], clips[3]]
    _same_clips(pipe.run_later_clips_batched_geometry(two, batch_geometry=False), pipe.run_later_clips_batched(two), "fallback")
    # a given-geometry list ignores the flag
    ex = [env["explicit"][0], env["explicit"][2]]
    a, b = pipe.run_later_clips_batched_geometry(ex), pipe.run_later_clips_batched(ex)
    for x, y in zip(a, b):
        for p, q in zip(x, y):
            assert set(p) == set(q) == set(KEYS) and all(torch.equal(p[k], q[k]) for k in KEYS)
    with pytest.raises(ValueError, match="mixes geometry-mode"):
        pipe.run_later_clips_batched_geometry([clips[0], env["explicit"][2]])
    assert pipe.run_later_clips_batched_geometry([]) == []


# ------------------------------------------------------------------------------------------------ 9. inpainting
def test_inpainted_clips():
    """Two clips of (2, 2) and (1, 1) with 'box_masks', vehicle 1 of clip 0's frame 1 inert: frames and the kept rows' merged boxes
    equal the explicit several-clip path with the inert row's box set to (0, 0, 0, 0)."""
    shapes, vehs, inert = [(2, 2), (1, 1)], [[0, 1], [1]], (0, 1, 1)
    pipe, bank, scene = _setup(2, inpaint=True)
    H, W = HW
    boxes0 = np.asarray(pl.synth_inpaint_boxes(np.asarray(scene["bboxes"]).tolist(), HW), np.int64)

    def inpaint_of(boxes):
        planes = torch.zeros((len(boxes), 1, H, W), dtype=torch.uint8)
        for v, (x0, y0, x1, y1) in enumerate(boxes):                            # a stand-in detection: the middle of the box
            planes[v, 0, y0 + (y1 - y0) // 4:y1 - (y1 - y0) // 4, x0 + (x1 - x0) // 4:x1 - (x1 - x0) // 4] = 255
        return {"boxes": boxes, "box_masks": [m.to(DEV) for m in pl.synth_box_masks(planes, boxes)]}

    clips, firsts, boxes = [], [], []
    for c, idx in enumerate(vehs):
        sub = _sub_scene(scene, idx)
        first = pipe.run_frame(dict(sub, inpaint=inpaint_of(boxes0[idx])))
        assert first["skipped"] == []
        later = _later_scenes(sub, first, shapes[c][0], shapes[c][1], inert[1:] if c == inert[0] else (-1, 0))
        bs = [boxes0[idx] + np.array([2 * n + 1, n, 2 * n + 1, n]) * (boxes0[idx][:, 2:3] < W - 8) for n in range(len(later))]
        for sc, b in zip(later, bs):
            sc["inpaint"] = inpaint_of(b)
        clips.append((later, first["state"]))
        firsts.append(first)
        boxes.append(bs)
    got = pipe.run_later_clips_batched_geometry(clips)
    assert [[g["skipped"] for g in one] for one in got] == [[[], [inert[2]]], [[]]]
    explicit = []
    for c, ((later, st), first) in enumerate(zip(clips, firsts)):
        ex = _explicit_scenes(later, got[c], first)
        for f, (e, sc) in enumerate(zip(ex, later)):
            b, pieces = boxes[c][f].copy(), list(sc["inpaint"]["box_masks"])
            if (c, f) == inert[:2]:                                              # the gate's doing, by hand
                b[inert[2]] = 0
                pieces[inert[2]] = torch.zeros((0, 0), dtype=torch.uint8, device=DEV)
            e["inpaint"] = {"boxes": b, "box_masks": pieces}
        explicit.append((ex, dict(st, geometry=None)))
    want = pipe.run_later_clips_batched(explicit)
    for c, (F, V) in enumerate(shapes):
        _same_as_explicit(got[c], want[c], V, f"inpaint clip {c}", keys=("geom", "icn_u8", "vunet_u8", "inpaint_u8"))
    # the inert vehicle's real box keeps the frame's pixels where no kept vehicle's mask or box lies
    c, f, v = inert
    x0, y0, x1, y1 = boxes[c][f][v]
    free = torch.zeros((H, W), dtype=torch.bool, device=DEV)
    free[y0:y1, x0:x1] = True
    o = 1 - v
    free[boxes[c][f][o][1]:boxes[c][f][o][3], boxes[c][f][o][0]:boxes[c][f][o][2]] = False
    free &= ~got[c][f]["geometry"]["masks"][o].bool()
    assert free.any()
    for k in ("frame_icn", "frame_vunet"):
        assert torch.equal(got[c][f][k][free], clips[c][0][f]["frame"][free]), k
