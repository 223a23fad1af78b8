"""GPU: scene['inpaint'] on FUTURE frames (trajectory_inference.py:301-350) - `run_later_frame` and every driver built on it
- against the vehicle-serial reference of tests/later_inpaint_ref.py, and bit for bit across the three scene forms, eager /
replayed / pipelined / clip drivers and geometry mode.  (The two-rank form lives in test_frame_later_inpaint_shard_gpu.py: its
worker processes are started only from a process that has not initialised HIP, so its file sorts before the test_gpu_* ones.)"""
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

import later_inpaint_ref as lr                                             # noqa: E402
import oracle                                                              # noqa: E402
from conftest import record, synth_sd                                      # noqa: E402
from future_urban_scene_generation_amd import ops                          # noqa: E402
from future_urban_scene_generation_amd import pipeline as pl               # noqa: E402

DEV = "cuda:0"
HW = (360, 640)
KEYS = ("icn_u8", "vunet_u8", "inpaint_u8", "frame_icn", "frame_vunet", "geom")


def _same(a, b, tag, keys=KEYS):
    for k in keys:
        assert torch.equal(a[k], b[k]), (tag, k)


def later_inpaint_scenes(first, dev, shift=(5, -7), seed=9, step=1):
    """A later scene of `first` (2 vehicles moved by `shift` = (dy, dx) pixels, as test_run_later_frame_matches_the_oracle
    moves them) with this frame's boxes - each reaching into the other vehicle's mask - in the three forms of scene['inpaint'];
    also the host planes."""
    g = np.random.default_rng(seed)
    later = {k: v for k, v in first.items() if k != "inpaint"}
    later["masks"] = torch.roll(first["masks"], shifts=shift, dims=(1, 2))
    later["dst_sketch"] = torch.roll(first["dst_sketch"], shifts=shift, dims=(1, 2))
    later["dst_kp"] = [[np.int32(p + np.array([shift[1], shift[0]]) + g.integers(-2, 3, p.shape)) for p in veh] for veh in first["dst_kp"]]
    later["vehicle_seeds"] = [int(s) * 64 + step for s in first["vehicle_seeds"]]
    masks = later["masks"].cpu().numpy()
    V = masks.shape[0]
    boxes = lr.overlapping_boxes(masks, pl.synth_inpaint_boxes(np.asarray(first["bboxes"]).tolist(), HW, [(shift[1], shift[0])] * V))
    planes = pl.synth_det_masks(list(masks), boxes.tolist())
    det = planes.to(dev)
    forms = {"none": later,
             "det_masks": dict(later, inpaint={"boxes": boxes, "det_masks": det}),
             "box_masks": dict(later, inpaint={"boxes": boxes, "box_masks": [m.to(dev) for m in pl.synth_box_masks(planes, boxes)]}),
             "given": dict(later, inpaint=dict(ops.inpaint_inputs(later["frame"], det, boxes), boxes=boxes))}
    return forms, planes.numpy(), boxes, masks


@pytest.fixture(scope="module")
def env():
    """One pipeline with all five networks, a first frame with inpainting, one later frame in every form, the frame the eager
    driver gives for it and (computed once, on 16 host threads) the reference."""
    ops.set_precision("f16x3")
    sds = {n: synth_sd(n) for n in ("hg", "icn", "vunet", "edge", "inpaint")}
    pipe = pl.VehiclePipeline(DEV, inpaint=True, state_dicts=sds)
    first = pl.synth_frame(2, HW, DEV, seed=41, inpaint="masks")
    first["vehicle_seeds"] = [11, 12]
    forms, planes, boxes, masks = later_inpaint_scenes(first, DEV)
    # each box covers part of the OTHER vehicle's mask, and box 1 part of vehicle 0's mask that vehicle 1's own mask leaves alone
    for v, o in ((0, 1), (1, 0)):
        x0, y0, x1, y1 = boxes[v]
        assert masks[o][y0:y1, x0:x1].any(), v
    x0, y0, x1, y1 = boxes[1]
    assert (masks[0].astype(bool) & ~masks[1].astype(bool))[y0:y1, x0:x1].any()
    f0 = pipe.run_frame(first)
    got = pipe.run_later_frame(forms["box_masks"], f0["state"])
    nt = torch.get_num_threads()
    torch.set_num_threads(min(16, max(1, len(os.sched_getaffinity(0)))))
    try:
        plain = {k: v for k, v in sds.items() if k in ("hg", "icn", "vunet")}
        o0 = oracle.frame_pass(plain, lr.scene_cpu({k: v for k, v in first.items() if k != "inpaint"}))
        cpu = lr.scene_cpu(forms["none"])
        four = ops.inpaint_inputs_host(cpu["frame"], planes, boxes)
        ref = lr.later_inpaint_pass(sds, cpu, o0["state"], four, boxes)
    finally:
        torch.set_num_threads(nt)
    return dict(sds=sds, pipe=pipe, first=first, forms=forms, boxes=boxes, masks=masks, f0=f0, got=got, ref=ref, cpu=cpu, four=four)


def test_later_frame_with_inpainting_matches_the_reference(env):
    """The project's bars for the same arithmetic on first frames and on later frames without inpainting: merged and VUnet crops
    within 1 LSB, composited frames SSIM >= 0.999, the frame's own bytes outside every box and mask, within 2 in the boxes outside
    the masks (the resize of a 1-LSB image)."""
    got, ref, cpu = env["got"], env["ref"], env["cpu"]
    assert float(env["four"]["mask"].mean()) > 0 and float(env["four"]["edge"].sum()) > 0
    assert "inpaint_u8" in got and tuple(got["inpaint_u8"].shape) == (2, 256, 256, 3)
    assert np.array_equal(got["geom"].cpu().numpy(), ref["geom"])
    for k in ("inpaint_u8", "vunet_u8"):
        d = int(np.abs(got[k].cpu().numpy().astype(int) - ref[k].astype(int)).max())
        print(f"later_inpaint {k} max diff {d}")
        record(f"later_inpaint_{k}_max_diff", d)
        assert d <= 1, (k, d)
    any_mask = cpu["masks"].max(0).astype(bool)
    cover = any_mask.copy()
    for x0, y0, x1, y1 in env["boxes"]:
        cover[y0:y1, x0:x1] = True
    for k in ("frame_icn", "frame_vunet"):
        a = got[k].cpu().numpy()
        sv = oracle.ssim(a, ref[k])
        d = int(np.abs(a.astype(int) - ref[k].astype(int))[~any_mask].max())
        print(f"later_inpaint {k} ssim {sv} max diff in boxes outside masks {d}")
        record(f"later_inpaint_{k}_ssim", sv)
        assert sv >= 0.999, (k, sv)
        assert np.array_equal(a[~cover], cpu["frame"][~cover]), k
        assert d <= 2, (k, d)
        # the boxes really replaced the frame: without the feature they would hold the real vehicle
        x0, y0, x1, y1 = env["boxes"][0]
        assert not np.array_equal(a[y0:y1, x0:x1], cpu["frame"][y0:y1, x0:x1]), k


def test_the_three_scene_forms_give_the_same_bits(env):
    pipe, st = env["pipe"], env["f0"]["state"]
    _same(pipe.run_later_frame(env["forms"]["det_masks"], st), env["got"], "det_masks")
    _same(pipe.run_later_frame(env["forms"]["given"], st), env["got"], "given")
    packed = dict(env["forms"]["box_masks"])
    pcs = packed["inpaint"]["box_masks"]
    offs = np.zeros(len(pcs), np.int64)
    offs[1:] = np.cumsum([int(m.numel()) for m in pcs])[:-1]
    packed["inpaint"] = dict(packed["inpaint"], box_masks=(torch.cat([m.reshape(-1) for m in pcs]), offs))
    _same(pipe.run_later_frame(packed, st), env["got"], "packed pair")
    fl = dict(env["forms"]["box_masks"])
    fl["inpaint"] = dict(fl["inpaint"], box_masks=[m.cpu().float() / 255 for m in pcs])        # float32 host pieces
    _same(pipe.run_later_frame(fl, st), env["got"], "float host pieces")
    # 'background' is ignored with inpainting (:340), as on the first frame
    _same(pipe.run_later_frame(dict(env["forms"]["box_masks"], background=torch.zeros_like(env["first"]["frame"])), st), env["got"], "background")


def test_replay_gives_the_eager_bits_and_hands_out_copies(env):
    pipe, st, sc = env["pipe"], env["f0"]["state"], env["forms"]["box_masks"]
    r1 = pipe.run_later_frame(sc, st, replay=True)
    keep = {k: r1[k].clone() for k in KEYS}
    r2 = pipe.run_later_frame(sc, st, replay=True)
    r3 = pipe.run_later_frame(env["forms"]["given"], st, replay=True)
    for tag, r in (("first replay", r1), ("second replay", r2), ("given, replayed", r3)):
        _same(r, env["got"], tag)
    _same(r1, keep, "the first result after later replays")
    assert len({r["inpaint_u8"].data_ptr() for r in (r1, r2, r3)}) == 3 and len({r["vunet_u8"].data_ptr() for r in (r1, r2, r3)}) == 3
    assert ("later", 2, ops.PRECISION, "inpaint") in pipe._frame_plans


def test_no_inpaint_key_is_the_pipeline_without_inpainting(env):
    """A later scene without 'inpaint' on the inpaint pipeline == a pipeline built with inpaint=False (which also ignores the key),
    eager and replayed - after the inpaint plan of the same vehicle count has been recorded."""
    pipe, st, sc = env["pipe"], env["f0"]["state"], env["forms"]["none"]
    plain = pl.VehiclePipeline(DEV, state_dicts={k: v for k, v in env["sds"].items() if k in ("hg", "icn", "vunet")})
    keys = ("icn_u8", "vunet_u8", "frame_icn", "frame_vunet", "geom")
    bg = dict(sc, background=torch.full_like(sc["frame"], 9))
    for rp in (False, True):
        pipe.run_later_frame(env["forms"]["box_masks"], st, replay=rp)
        for tag, s in (("no key", sc), ("background", bg)):
            want = plain.run_later_frame(s, st, replay=rp)
            got = pipe.run_later_frame(s, st, replay=rp)
            assert "inpaint_u8" not in got and "inpaint_u8" not in want
            _same(got, want, (tag, rp), keys)
        _same(plain.run_later_frame(env["forms"]["box_masks"], st, replay=rp), plain.run_later_frame(sc, st, replay=rp), ("ignored", rp), keys)
    assert ("later", 2, ops.PRECISION) in pipe._frame_plans and ("later", 2, ops.PRECISION, "inpaint") not in plain._frame_plans


def test_pipelined_later_frames_and_clips(env):
    """run_later_frames([a, b, a]) with one frame in flight == three synchronous calls, eager and replayed (b: other boxes, so other
    box extents through the same recorded plan); run_clip_frames with an inpaint first scene and two later scenes."""
    pipe, st = env["pipe"], env["f0"]["state"]
    a = env["forms"]["box_masks"]
    b = pl.synth_later_frame(env["forms"]["none"], 3, inpaint="box_masks")
    assert not np.array_equal(b["inpaint"]["boxes"], a["inpaint"]["boxes"])
    for rp in (False, True):
        want = [pipe.run_later_frame(s, st, replay=rp) for s in (a, b, a)]
        seq = list(pipe.run_later_frames([a, b, a], st, replay=rp))
        assert len(seq) == 3
        for i, (x, y) in enumerate(zip(seq, want)):
            _same(x, y, (rp, i))
        _same(seq[0], env["got"], rp)
        assert not torch.equal(seq[1]["frame_icn"], seq[0]["frame_icn"])
        clip = list(pipe.run_clip_frames(env["first"], [a, b], replay=rp))
        assert len(clip) == 3 and "inpaint_u8" in clip[0]
        _same(clip[1], want[0], ("clip 1", rp))
        _same(clip[2], want[1], ("clip 2", rp))
        for k in ("kp_idx", "inpaint_u8", "frame_icn", "frame_vunet"):
            assert torch.equal(clip[0][k], env["f0"][k]), (k, rp)
    # a frame outside the split-fp16 range is redone whole - EdgeConnect included - in fp32: the synchronous call's result
    hot_state = dict(st)
    hot_state["appearance"] = [t.clone() for t in st["appearance"]]
    hot_state["appearance"][1][0, 0, 0, 0] = 6e4
    want = [pipe.run_later_frame(s, hot_state) for s in (a, b)]
    seq = list(pipe.run_later_frames([a, b], hot_state))
    for i, (x, y) in enumerate(zip(seq, want)):
        _same(x, y, ("hot", i))
    assert not ops.range_exceeded(DEV)


def test_malformed_scenes_and_no_vehicles(env):
    pipe, st, sc = env["pipe"], env["f0"]["state"], env["forms"]["box_masks"]
    with pytest.raises(ValueError, match="box_masks"):
        pipe.run_later_frame(dict(sc, inpaint=dict(sc["inpaint"], det_masks=env["forms"]["det_masks"]["inpaint"]["det_masks"])), st)
    with pytest.raises(ValueError, match="inpaint=True"):
        pipe.run_later_frame(dict(sc, inpaint={"boxes": env["boxes"]}), st)
    with pytest.raises(ValueError, match=r"box_masks\[0\]"):
        pipe.run_later_frame(dict(sc, inpaint=dict(sc["inpaint"], box_masks=[m[:-1] for m in sc["inpaint"]["box_masks"]])), st)
    H, W = HW
    e = lambda *sh: torch.empty(sh, dtype=torch.uint8, device=DEV)           # noqa: E731
    none = {"frame": sc["frame"], "masks": e(0, H, W), "dst_sketch": e(0, H, W, 3), "src_planes": e(0, 5, H, W, 3), "src_kp": [],
            "dst_kp": [], "src_vis": np.zeros((0, 5), np.uint8), "dst_vis": np.zeros((0, 5), np.uint8),
            "inpaint": {"boxes": np.zeros((0, 4), np.int64), "box_masks": []}, "background": torch.zeros_like(sc["frame"])}
    st0 = {"appearance": [t[:0] for t in st["appearance"]], "central": st["central"][:0], "shard": (0, 0, 0), "sharded": False}
    for rp in (False, True):
        o = pipe.run_later_frame(none, st0, replay=rp)
        assert o["inpaint_u8"].shape == (0, 256, 256, 3) and o["icn_u8"].shape == (0, 256, 256, 3)
        assert torch.equal(o["frame_icn"], sc["frame"]) and torch.equal(o["frame_vunet"], sc["frame"])


def test_geometry_mode_later_frame_with_box_masks(env):
    """Geometry mode on one rank (the sizes of tests/test_gpu_render.py): a later frame with 'box_masks' == the derived geometry fed
    back as an explicit scene with the same 'inpaint'; a vehicle that renders empty is not inpainted; sharded: ValueError."""
    from future_urban_scene_generation_amd import render as R
    from test_gpu_render import _explicit, _geometry_setup
    V = 3
    _, bank, scene = _geometry_setup(V=V)
    pipe = pl.VehiclePipeline(DEV, inpaint=True, state_dicts=env["sds"], cad_bank=bank)
    boxes0 = np.asarray(pl.synth_inpaint_boxes(np.asarray(scene["bboxes"]).tolist(), HW), np.int64)
    H, W = HW
    g = torch.Generator().manual_seed(3)

    def inpaint_of(boxes):
        planes = torch.zeros((V, 1, H, W), dtype=torch.uint8)
        for v, (x0, y0, x1, y1) in enumerate(boxes):                            # a stand-in detection: the middle of the box
            planes[v, 0, y0 + (y1 - y0) // 4:y1 - (y1 - y0) // 4, x0 + (x1 - x0) // 4:x1 - (x1 - x0) // 4] = 255
        return {"boxes": boxes, "box_masks": [m.to(DEV) for m in pl.synth_box_masks(planes, boxes)]}

    out = pipe.run_frame(dict(scene, inpaint=inpaint_of(boxes0)))
    assert out["skipped"] == [] and out["inpaint_u8"].shape[0] == V
    geo = out["geometry"]
    E = [R.extrinsic_from_pose(p[1], p[2]) for p in out["pose"]]
    steps = R.trajectory_steps(np.c_[np.arange(6.0) * 0.8, 0.05 * np.arange(6.0) ** 2])
    for n in (0, 1):
        st = [steps[n]] * V
        if n == 1:                                                              # vehicle 1 behind the camera: renders empty
            st[1] = (steps[n][0], -200.0 * np.asarray(E[1][2, :3], np.float64))
        boxes = boxes0 + np.array([2 * n + 1, n, 2 * n + 1, n]) * (boxes0[:, 2:3] < W - 8)
        inp = inpaint_of(boxes)
        later = {"frame": scene["frame"], "steps": st, "vehicle_seeds": [900 + 10 * n + v for v in range(V)], "inpaint": inp}
        lo = pipe.run_later_frame(later, out["state"])
        keep = [v for v in range(V) if not (n == 1 and v == 1)]
        assert lo["skipped"] == [v for v in range(V) if v not in keep] and lo["inpaint_u8"].shape[0] == len(keep)
        lg = lo["geometry"]
        ex_sc = _explicit({"frame": scene["frame"], "vehicle_seeds": [later["vehicle_seeds"][v] for v in keep]}, lg, keep,
                          ("masks", "dst_sketch", "dst_kp", "dst_vis"))
        ex_sc = _explicit(ex_sc, geo, keep, ("src_planes", "src_kp", "src_vis"))
        ex_sc["inpaint"] = {"boxes": boxes[keep], "box_masks": [inp["box_masks"][v] for v in keep]}
        st_sub = dict(out["state"], geometry=None, appearance=[a[keep] for a in out["state"]["appearance"]],
                      central=out["state"]["central"][keep])
        ex = pipe.run_later_frame(ex_sc, st_sub)
        _same(lo, ex, n)
        _same(pipe.run_later_frame(later, out["state"], replay=True), ex, (n, "replay"))
        if n == 1:                                                              # the skipped vehicle's box keeps the frame's pixels
            x0, y0, x1, y1 = boxes[1]
            free = torch.ones((H, W), dtype=torch.bool, device=DEV)
            for v in keep:
                free[boxes[v][1]:boxes[v][3], boxes[v][0]:boxes[v][2]] = False
            free &= ~ex_sc["masks"].max(0).values.bool()
            assert torch.equal(lo["frame_icn"][free], scene["frame"][free])
    seq = list(pipe.run_later_frames([later, later], out["state"]))
    _same(seq[0], lo, "pipelined 0")
    _same(seq[1], lo, "pipelined 1")
    sharded = dict(out["state"], sharded=True)
    import torch.distributed as dist
    assert not (dist.is_available() and dist.is_initialized())
    # the combination is refused where it would run: the sharded geometry driver, reached here without a process group
    with pytest.raises(ValueError, match="sharded geometry-mode later frame"):
        pipe._geometry_later_sharded(later, sharded, "sync", False)
