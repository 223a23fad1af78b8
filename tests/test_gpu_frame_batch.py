"""GPU: the first frames of several scenes as ONE batched pass (VehiclePipeline.run_frames_batched, fusg_crop_resize_frames_u8,
fusg_vunet_inputs_frames, fusg_paste_layers_ragged_u8).  The three frame-indexed kernels equal their one-frame siblings byte for
byte; a scene cut into slices that share its frame gives `run_frame`'s bits (the same batch: the same routing); scenes with
frames of their own are compared with the vehicle-serial CPU oracle under the bars of tests/test_gpu_frame.py (not with
per-frame device passes: a batch of 3 and a batch of 2 may route convolutions differently)."""
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
from future_urban_scene_generation_amd import frame_ops as fo              # noqa: E402
from future_urban_scene_generation_amd import ops                          # noqa: E402
from future_urban_scene_generation_amd import pipeline as pl               # noqa: E402
from future_urban_scene_generation_amd.warp_learn import planes_utils as pu   # noqa: E402
from oracle import cv_host as C                                            # noqa: E402

DEV = "cuda:0"
HW = (360, 640)
KEYS = ("kp_idx", "kp_xy", "geom", "icn_u8", "vunet_u8", "frame_icn", "frame_vunet")


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host_threads():
    return min(16, max(1, len(os.sched_getaffinity(0))))


def _pose_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for p, q in zip(a, b) for x, y in zip(p, q))


# ------------------------------------------------------------------------------------------------ 1: the two input kernels
def _three_frames(H, W, seed=3):
    g = np.random.default_rng(seed)
    frames = [_d(g.integers(0, 256, (H, W, 3), dtype=np.uint8)) for _ in range(3)]
    assert not torch.equal(frames[0], frames[1]) and not torch.equal(frames[1], frames[2])
    return frames


def _windows(H, W, rows, out_hw):
    """`rows` geometry rows: an ordinary box, one clipped at two frame borders (the window pads on two sides), a zero-extent
    window (an all-zero row), one whose window is exactly out_hw (the copy path), another ordinary one."""
    oh, ow = out_hw
    side = min(oh, ow)
    boxes = [(W // 3, H // 4, W // 3 + 45, H // 4 + 30), (-10, -8, 50, 40), None, (20, 10, 20 + side, 10 + side), (W - 60, H - 40, W - 5, H - 3)]
    if rows == 1:
        boxes = [boxes[1]]
    geom = np.zeros((rows, 8), np.int32)
    for r, bb in enumerate(boxes[:rows]):
        if bb is not None:
            win, pb, pa = C.square_crop_geometry((H, W), bb)
            geom[r] = [win[0], win[1], win[2], win[3], pb[0], pb[1], pa[0], pa[1]]
    if rows > 3:
        geom[3] = [20, 10, 20 + side, 10 + side, 0, 0, 0, 0]                         # (the window itself, not a box it is grown from)
    return geom


@pytest.mark.parametrize("counts", [[2, 0, 3], [1]], ids=["2_0_3", "1"])
@pytest.mark.parametrize("H,W", [(77, 131), (90, 150)])
def test_crop_resize_frames_equals_the_per_frame_kernel(H, W, counts):
    """fusg_crop_resize_frames_u8 == fusg_crop_resize_u8 per frame, concatenated, in modes 0, 1 and 2: frames that differ, odd
    widths, more than one block per row (40 x 56 outputs = 9 blocks, the last one partial), a frame without rows."""
    frames = _three_frames(H, W)[:len(counts)]
    offs = pl.frame_batch_offsets(counts)
    out_hw = (40, 56)
    geom_h = _windows(H, W, offs[-1], (40, 40))
    geom = _d(geom_h)
    assert geom_h[0 if offs[-1] == 1 else 1, 4:6].all(), "the clipped window pads on two sides"
    for mode, norm in ((0, {}), (1, dict(mean=fo.IMAGENET_MEAN, std=fo.IMAGENET_STD)), (2, {})):
        got = fo.crop_resize_frames(frames, offs, geom, out_hw, mode, **norm)
        want = torch.cat([fo.crop_resize(frames[f], geom[offs[f]:offs[f + 1]].contiguous(), out_hw, mode, **norm)
                          for f in range(len(counts)) if counts[f]])
        assert got.shape == want.shape and got.dtype == want.dtype, mode
        assert torch.equal(got, want), mode
        if offs[-1] > 1:
            assert not got[2].any() if mode == 0 else True                          # the zero-extent window writes zeros
            assert got[0].float().abs().sum() > 0
    # the square window of exactly the output's size is a copy of the frame's pixels
    if offs[-1] > 1:
        sq = fo.crop_resize_frames(frames, offs, geom, (40, 40), 0)
        x0, y0 = int(geom_h[3, 0]), int(geom_h[3, 1])
        assert geom_h[3, 2] - geom_h[3, 0] == 40 and torch.equal(sq[3], frames[2][y0:y0 + 40, x0:x0 + 40])


@pytest.mark.parametrize("counts", [[2, 0, 3], [1]], ids=["2_0_3", "1"])
@pytest.mark.parametrize("H,W", [(77, 131), (90, 150)])
def test_vunet_inputs_frames_equals_the_per_frame_kernel(H, W, counts):
    """fusg_vunet_inputs_frames == fusg_vunet_inputs per frame: a mask whose box window is clipped at two borders, an empty mask
    (its crop row is all zero: a zero-extent window), another frame per group of rows."""
    frames = _three_frames(H, W, seed=4)[:len(counts)]
    offs = pl.frame_batch_offsets(counts)
    N = offs[-1]
    g = np.random.default_rng(6)
    masks = np.zeros((N, H, W), np.uint8)
    spots = [(0, 0, 34, 27), (W // 2, H // 3, W // 2 + 40, H // 3 + 22), None, (W - 50, H - 30, W, H), (10, H // 2, 48, H // 2 + 30)]
    for r, bb in enumerate(spots[:N]):
        if bb is not None:
            masks[r, bb[1]:bb[3], bb[0]:bb[2]] = 1
    ssk = g.integers(0, 256, (N, H, W, 3), dtype=np.uint8) * masks[..., None]
    dsk = g.integers(0, 256, (N, H, W, 3), dtype=np.uint8) * masks[..., None]
    masks, ssk, dsk = _d(masks), _d(ssk), _d(dsk)
    _, geom = fo.mask_bbox_geom(masks)
    gh = geom.cpu().numpy()
    assert gh[0, 4:6].all(), "the first mask's window pads on two sides"
    if N > 1:
        assert not gh[2].any(), "the empty mask gives a zero-extent window"
    res = 40
    x, y = fo.vunet_inputs_frames(frames, offs, masks, ssk, dsk, geom, res)
    want = [fo.vunet_inputs(frames[f], masks[offs[f]:offs[f + 1]], ssk[offs[f]:offs[f + 1]], dsk[offs[f]:offs[f + 1]],
                            geom[offs[f]:offs[f + 1]].contiguous(), res) for f in range(len(counts)) if counts[f]]
    assert torch.equal(x, torch.cat([w[0] for w in want])) and torch.equal(y, torch.cat([w[1] for w in want]))
    assert tuple(x.shape) == (N, 6, res, res) and tuple(y.shape) == (N, 3, res, res)
    if N > 1:                                                                       # the rows of frame 2 really read frame 2
        other = fo.vunet_inputs(frames[0], masks[offs[2]:], ssk[offs[2]:], dsk[offs[2]:], geom[offs[2]:].contiguous(), res)[0]
        assert not torch.equal(x[offs[2]:], other)


def test_the_wrappers_refuse_what_the_library_cannot_see():
    frames = _three_frames(77, 131)
    geom = _d(np.zeros((2, 8), np.int32))
    with pytest.raises(ValueError, match="every frame"):
        fo.crop_resize_frames([frames[0], frames[1][:70]], [0, 1, 2], geom, (8, 8))
    with pytest.raises(ValueError, match="row offsets"):
        fo.crop_resize_frames(frames[:2], [0, 2], geom, (8, 8))
    with pytest.raises(ValueError, match="frames"):
        fo.crop_resize_frames([], [0], geom[:0], (8, 8))
    assert tuple(fo.crop_resize_frames(frames[:2], [0, 0, 0], geom[:0], (8, 8)).shape) == (0, 8, 8, 3)   # rows = 0: a no-op


# ------------------------------------------------------------------------------------------------ 2: the ragged paste
def _ragged_case(counts, H, W, R=32, seed=5):
    """Frames of counts[f] vehicles whose masks overlap in the middle of the frame (the row order decides pixels there), a base
    image per frame; the last row's crop window leaves the frame."""
    g = np.random.default_rng(seed)
    F, N = len(counts), sum(counts)
    offs = pl.frame_batch_offsets(counts)
    bases = g.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    nets = g.integers(0, 256, (N, R, R, 3), dtype=np.uint8)
    boxes_img = g.integers(0, 256, (N, R, R, 3), dtype=np.uint8)
    masks = np.zeros((N, H, W), np.uint8)
    geom, rects = np.zeros((N, 8), np.int32), np.zeros((N, 8), np.int32)
    for f in range(F):
        for v in range(counts[f]):
            r = offs[f] + v
            x0, y0 = W // 2 - 30 + 9 * v + int(g.integers(-3, 4)), H // 2 - 25 + 7 * v + 2 * f
            bb = [x0, y0, x0 + int(g.integers(28, 45)), y0 + int(g.integers(22, 36))]
            if r == N - 1:
                bb = [W - 30, -4, W + 6, 28]                                      # the square window pads on two sides
            masks[r, max(0, bb[1] - 3):bb[3] + 2, max(0, bb[0] - 2):min(W, bb[2] + 3)] = 1
            win, pb, pa = C.square_crop_geometry((H, W), bb)
            geom[r] = [win[0], win[1], win[2], win[3], pb[0], pb[1], pa[0], pa[1]]
            rects[r, :4] = [max(0, bb[0] - 9), max(0, bb[1] - 7), min(W - 1, bb[2] + 11), min(H - 1, bb[3] + 6)]
    return dict(bases=bases, nets=nets, boxes_img=boxes_img, masks=masks, geom=geom, rects=rects, counts=counts, offs=offs)


def _ragged_both(c, boxes, reverse=False):
    """(one ragged launch, one call of the existing paste per frame); reverse: every frame's layers in the opposite order."""
    counts, offs = c["counts"], c["offs"]
    rows = np.concatenate([np.arange(offs[f], offs[f + 1])[::-1] if reverse else np.arange(offs[f], offs[f + 1]) for f in range(len(counts))])
    t = {k: _d(c[k][rows]) for k in ("nets", "masks", "geom", "boxes_img", "rects")}
    bases = [_d(c["bases"][f]) for f in range(len(counts))]
    box = dict(box_images=t["boxes_img"], box_geom=t["rects"]) if boxes else {}
    got = pu.paste_back_ragged_device(bases, offs, t["nets"], t["geom"], t["masks"], **box)
    want = []
    for f, n in enumerate(counts):
        sl = slice(offs[f], offs[f + 1])
        bx = dict(box_images=t["boxes_img"][sl], box_geom=t["rects"][sl].contiguous()) if boxes else {}
        want.append(pu.paste_back_device(bases[f], t["nets"][sl], t["geom"][sl].contiguous(), t["masks"][sl], **bx) if n else bases[f])
    for f in range(len(counts)):                                                  # the bases are read, never written
        assert np.array_equal(bases[f].cpu().numpy(), c["bases"][f])
    return got, torch.stack(want)


@pytest.mark.parametrize("boxes", [True, False], ids=["box_layers", "plain"])
@pytest.mark.parametrize("H,W", [(120, 200), (77, 131)])
def test_ragged_paste_equals_the_per_frame_paste(H, W, boxes):
    """fusg_paste_layers_ragged_u8 == one call of fusg_paste_layers_u8 / fusg_paste_back_u8 per frame, byte for byte, for 3, 0, 1
    and 2 layers: overlapping vehicles whose order decides pixels (the same layers reversed give other pixels), a frame without
    layers (a copy of its base), a crop clipped at the frame border, widths that are no multiple of 16."""
    counts = [3, 0, 1, 2]
    c = _ragged_case(counts, H, W)
    m = c["masks"].astype(bool)
    assert (m[0] & m[1]).any() and (m[1] & m[2]).any(), "the overlap is not empty"
    assert c["geom"][-1, 4:].any(), "the clipped crop pads"
    got, want = _ragged_both(c, boxes)
    assert tuple(got.shape) == (4, H, W, 3) and got.dtype == torch.uint8
    assert torch.equal(got, want)
    assert np.array_equal(got[1].cpu().numpy(), c["bases"][1])                    # no layers: the base
    rev, rev_want = _ragged_both(c, boxes, reverse=True)
    assert torch.equal(rev, rev_want)
    assert not torch.equal(got[0], rev[0]) and torch.equal(got[2], rev[2])        # 3 layers: the order decides; 1 layer: nothing to reorder
    for f, n in enumerate(counts):                                                # the layers replaced pixels, the rest is the base
        if n:
            cover = m[c["offs"][f]:c["offs"][f + 1]].max(0)
            if boxes:
                for x0, y0, x1, y1 in c["rects"][c["offs"][f]:c["offs"][f + 1], :4]:
                    cover[y0:y1, x0:x1] = True
            a = got[f].cpu().numpy()
            assert np.array_equal(a[~cover], c["bases"][f][~cover]) and not np.array_equal(a[cover], c["bases"][f][cover])


def test_ragged_paste_without_any_layer():
    c = _ragged_case([0, 0], 77, 131)
    got, want = _ragged_both(c, False)
    assert torch.equal(got, want) and np.array_equal(got.cpu().numpy(), c["bases"])


# ------------------------------------------------------------------------------------------------ the driver
def _whole_state_rows(state, lo, hi):
    return {"appearance": [t[lo:hi] for t in state["appearance"]], "central": state["central"][lo:hi], "shard": (0, hi - lo, hi - lo),
            "sharded": False}


@pytest.fixture(scope="module")
def env():
    """One pipeline; a scene of 5 vehicles cut into slices of 2, 0 and 3 that share its frame, with `run_frame`'s result for
    the whole; three scenes of 2, 1 and 3 vehicles with frames of their own (seeds whose plane fits are well posed: the oracle's
    per-plane solver raises on the degenerate quadrilaterals some seeds draw, and on an ill-conditioned one it and the vectorised
    host fit part ways, for `run_frame` as for the batch - seed 17 with 2 vehicles is the scene of
    test_run_frame_with_inpainting_matches_the_oracle, seed 11 is test_run_frame_against_the_oracle_chain's, whose first vehicle
    this takes, seed 49 with 3 is tests/test_gpu_later_batch.py's first frame: on all three the warped planes equal the oracle's
    byte for byte) and, computed once on 16 host threads, the oracle's result for each."""
    ops.set_precision("f16x3")
    sds = {n: synth_sd(n) for n in ("hg", "icn", "vunet")}
    pipe = pl.VehiclePipeline(DEV, state_dicts=sds)
    whole = pl.synth_frame(5, HW, DEV, seed=7)
    whole["vehicle_seeds"] = [70 + v for v in range(5)]
    cuts = [(0, 2), (2, 2), (2, 5)]
    slices = [pl.slice_scene(whole, lo, hi) for lo, hi in cuts]
    w = pipe.run_frame(whole)
    own = []
    for V, seed, base in ((2, 17, 11), (1, 11, 31), (3, 49, 51)):
        sc = pl.synth_frame(V, HW, DEV, seed=seed)
        sc["vehicle_seeds"] = [base + v for v in range(V)]
        own.append(sc)
    assert not torch.equal(own[0]["frame"], own[1]["frame"]) and not torch.equal(own[1]["frame"], own[2]["frame"])
    nt = torch.get_num_threads()
    torch.set_num_threads(_host_threads())
    try:
        cpus = [lr.scene_cpu(sc) for sc in own]
        refs = [oracle.frame_pass(sds, c) for c in cpus]
    finally:
        torch.set_num_threads(nt)
    return dict(sds=sds, pipe=pipe, whole=whole, cuts=cuts, slices=slices, w=w, own=own, cpus=cpus, refs=refs)


def _bars(got, ref, cpu, tag, base=None):
    """The bars of test_run_frame_against_the_oracle_chain: keypoint indices, keypoints in frame pixels, crop rows and every
    frame pixel outside the masks exact; the VUnet crop within 1 LSB; the crops and both composited frames SSIM >= 0.999."""
    assert np.array_equal(got["kp_idx"].cpu().numpy(), ref["kp_idx"]), tag
    assert np.array_equal(got["kp_xy"].cpu().numpy(), ref["kp_xy"]), tag
    assert np.array_equal(got["geom"].cpu().numpy(), ref["geom"]), tag
    d = int(np.abs(got["vunet_u8"].cpu().numpy().astype(int) - ref["vunet_u8"].astype(int)).max())
    print(f"{tag}: vunet_u8 max diff {d}")
    record("frame_batch_vunet_u8_max_diff", d)
    assert d <= 1, (tag, d)
    for k in ("icn_u8", "vunet_u8", "frame_icn", "frame_vunet"):
        sv = oracle.ssim(got[k].cpu().numpy(), ref[k])
        print(f"{tag}: {k} ssim {sv}")
        record(f"frame_batch_{k}_ssim", sv, worst=min)
        assert sv >= 0.999, (tag, k, sv)
    cover = cpu["masks"].max(0).astype(bool)
    base = cpu["frame"] if base is None else base
    for k in ("frame_icn", "frame_vunet"):
        a = got[k].cpu().numpy()
        assert np.array_equal(a[~cover], base[~cover]), (tag, k)
        assert not np.array_equal(a[cover], base[cover]), (tag, k)
    assert len(got["pose"]) == len(ref["pose"])


def test_slices_of_one_scene_equal_run_frame_bit_for_bit(env):
    """3: scenes of 2, 0 and 3 vehicles that share a frame, eager and unpadded: the pass is `run_frame`'s pass of the 5 vehicles
    (the same batch, so the same routing) - every per-vehicle output, the pose and the state equal it bit for bit; each composite
    is the paste of that scene's own rows onto the frame."""
    pipe, w, cuts = env["pipe"], env["w"], env["cuts"]
    got = pipe.run_frames_batched(env["slices"])
    assert isinstance(got, list) and len(got) == 3
    for k in ("kp_idx", "kp_xy", "geom", "icn_u8", "vunet_u8"):
        assert torch.equal(torch.cat([g[k] for g in got]), w[k]), k
    assert _pose_equal([p for g in got for p in g["pose"]], w["pose"])
    assert torch.equal(torch.cat([g["state"]["central"] for g in got]), w["state"]["central"])
    for i in range(2):
        assert torch.equal(torch.cat([g["state"]["appearance"][i] for g in got]), w["state"]["appearance"][i]), i
    frame = env["whole"]["frame"]
    for g, (lo, hi) in zip(got, cuts):
        n = hi - lo
        assert g["state"]["shard"] == (0, n, n) and g["state"]["sharded"] is False
        assert set(g) == (set(KEYS) | {"pose", "state"} if n else set(pipe.run_frame(env["slices"][1])) | {"state"})
        assert tuple(g["kp_idx"].shape) == (n, 12) and tuple(g["icn_u8"].shape) == (n, 256, 256, 3) and tuple(g["geom"].shape) == (n, 8)
        assert tuple(g["kp_xy"].shape) == (n, 12, 2) and len(g["pose"]) == n and tuple(g["frame_icn"].shape) == HW + (3,)
        for k, c in (("frame_icn", "icn_u8"), ("frame_vunet", "vunet_u8")):
            if n:
                want = pu.paste_back_device(frame, w[c][lo:hi], w["geom"][lo:hi].contiguous(), env["whole"]["masks"][lo:hi])
                assert torch.equal(g[k], want) and not torch.equal(g[k], frame), k
            else:
                assert torch.equal(g[k], frame), k                                  # the empty scene: its base
    assert not any(k[0] == "frame_batch" for k in pipe._frame_plans)               # the eager form records nothing


def test_scenes_with_their_own_frames_match_the_oracle(env):
    """4: two scenes of 2 and 1 vehicles, another frame and other seeds each, against oracle.frame_pass; a 'background' on one
    scene changes that scene's base only."""
    pipe, own = env["pipe"], env["own"]
    got = pipe.run_frames_batched(own[:2])
    assert len(got) == 2
    for f in range(2):
        _bars(got[f], env["refs"][f], env["cpus"][f], f"scene {f}")
    bg = torch.full_like(own[1]["frame"], 77)
    withbg = pipe.run_frames_batched([own[0], dict(own[1], background=bg)])
    for k in KEYS:
        assert torch.equal(withbg[0][k], got[0][k]), k                             # the neighbour: untouched
    cover = env["cpus"][1]["masks"].max(0).astype(bool)
    for k in ("frame_icn", "frame_vunet"):
        a = withbg[1][k].cpu().numpy()
        assert (a[~cover] == 77).all() and np.array_equal(a[cover], got[1][k].cpu().numpy()[cover]), k


def test_replay_equals_the_padded_eager_pass_and_keeps_one_plan(env):
    """5: replay=True == pad=True eager, bit for bit; vehicle-count sequences (2, 1), (1, 1, 1) and (3,) all replay the ONE
    ("frame_batch", 4, ...) plan; the frame drivers' other plans are untouched; results survive later replays."""
    pipe, whole = env["pipe"], env["whole"]
    cut = lambda *edges: [pl.slice_scene(whole, lo, hi) for lo, hi in zip(edges, edges[1:])]      # noqa: E731
    seqs = [cut(0, 2, 3), cut(2, 3, 4, 5), cut(1, 4)]
    pipe.run_frame(pl.slice_scene(whole, 0, 3), replay=True)                       # the per-frame plan of 3 vehicles exists
    before = {k: id(v) for k, v in pipe._frame_plans.items() if k[0] != "frame_batch"}
    key = ("frame_batch", 4, ops.PRECISION)
    assert (3, ops.PRECISION) in before
    pipe._frame_plans.pop(key, None)
    eager = [pipe.run_frames_batched(s, pad=True) for s in seqs]
    assert key not in pipe._frame_plans                                           # pad=True alone records nothing
    r0 = pipe.run_frames_batched(seqs[0], replay=True)
    plan = pipe._frame_plans[key]
    keep = [{k: r0[f][k].clone() for k in KEYS} for f in range(2)]
    rest = [pipe.run_frames_batched(s, replay=True) for s in seqs[1:]]
    again = pipe.run_frames_batched(seqs[0], replay=True)
    assert pipe._frame_plans[key] is plan                                         # recorded once, replayed since
    assert [k for k in pipe._frame_plans if k[0] == "frame_batch"] == [key]
    for rep, eag in zip([r0, again] + rest, [eager[0], eager[0]] + eager[1:]):
        assert len(rep) == len(eag)
        for a, b in zip(rep, eag):
            for k in KEYS:
                assert torch.equal(a[k], b[k]), k
            assert _pose_equal(a["pose"], b["pose"])
            assert torch.equal(a["state"]["central"], b["state"]["central"])
            assert all(torch.equal(x, y) for x, y in zip(a["state"]["appearance"], b["state"]["appearance"]))
    for f in range(2):
        for k in KEYS:
            assert torch.equal(r0[f][k], keep[f][k]), (f, k)                      # handed out as copies: later replays leave them
    assert {k: id(v) for k, v in pipe._frame_plans.items() if k[0] != "frame_batch"} == before


def test_a_replay_zeroes_the_padding_row_an_earlier_group_filled(env):
    """A group of 4 real rows replayed, then 3 real rows of other scenes under the same ("frame_batch", 4, ...) plan: the plan's
    reused input buffers hold the first group's row 3, which the second group pads - every output of the second call equals the
    padded eager pass of the same scenes, bit for bit."""
    pipe, whole = env["pipe"], env["whole"]
    key = ("frame_batch", 4, ops.PRECISION)
    pipe._frame_plans.pop(key, None)
    pipe.run_frames_batched([pl.slice_scene(whole, 0, 2), pl.slice_scene(whole, 2, 4)], replay=True)
    plan = pipe._frame_plans[key]
    scenes = [pl.slice_scene(whole, 4, 5), dict(pl.slice_scene(whole, 1, 3), frame=whole["frame"] ^ 1)]
    got = pipe.run_frames_batched(scenes, replay=True)
    assert pipe._frame_plans[key] is plan                                         # replayed, not recorded again
    want = pipe.run_frames_batched(scenes, replay=False, pad=True)
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        assert set(a) == set(b)
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k
        assert _pose_equal(a["pose"], b["pose"])
        assert torch.equal(a["state"]["central"], b["state"]["central"])
        assert all(torch.equal(x, y) for x, y in zip(a["state"]["appearance"], b["state"]["appearance"]))


def test_chunked_passes_meet_the_same_bars_in_scene_order(env):
    """6: counts (2, 1, 3) with max_batch 3: two groups, (2, 1) and (3); scene f's result sits at position f."""
    pipe, own = env["pipe"], env["own"]
    assert pl.frame_batch_groups([2, 1, 3], 3) == [(0, 2), (2, 3)]
    calls = []
    orig = pipe._run_frame_batch
    pipe._run_frame_batch = lambda scenes, replay=False, rows=None: (calls.append([len(sc["bboxes"]) for sc in scenes]), orig(scenes, replay, rows))[1]
    try:
        got = pipe.run_frames_batched(own, max_batch=3)
    finally:
        del pipe._run_frame_batch
    assert calls == [[2, 1], [3]]
    assert len(got) == 3
    # the first group is the pass test_scenes_with_their_own_frames_match_the_oracle holds against the oracle: the same bits, at
    # positions 0 and 1; the second group's scene, at position 2, against the oracle here
    first = pipe.run_frames_batched(own[:2])
    for f in range(2):
        for k in KEYS:
            assert torch.equal(got[f][k], first[f][k]), (f, k)
        assert _pose_equal(got[f]["pose"], first[f]["pose"])
    _bars(got[2], env["refs"][2], env["cpus"][2], "max_batch 3 scene 2")


def test_range_guard_redoes_one_group_in_fp32(env):
    """7: the status word raised behind the first of two groups: that group comes back as an exact-fp32 run of the same group,
    bit for bit, the other stays split-fp16, and the word is clear afterwards."""
    pipe, own = env["pipe"], env["own"]
    scenes = own[:2]
    assert pl.frame_batch_groups([2, 1], 2) == [(0, 1), (1, 2)]
    with ops.precision("f32"):
        f32 = pipe.run_frames_batched(scenes[:1], check=None)
    h16 = [pipe.run_frames_batched([sc])[0] for sc in scenes]
    calls = {"n": 0}
    orig = pipe._run_frame_batch

    def flagged(sc, replay=False, rows=None):                                     # raise the status behind the 1st group only
        out = orig(sc, replay, rows)
        calls["n"] += 1
        if calls["n"] == 1:
            ops.status_word(DEV)[0] = 1
        return out

    pipe._run_frame_batch = flagged
    try:
        got = pipe.run_frames_batched(scenes, max_batch=2)
    finally:
        del pipe._run_frame_batch
    assert calls["n"] == 3                                                        # group 0, its redo, group 1
    for k in KEYS:
        assert torch.equal(got[0][k], f32[0][k]), k
        assert torch.equal(got[1][k], h16[1][k]), k
    assert _pose_equal(got[0]["pose"], f32[0]["pose"])
    assert any(not torch.equal(got[0][k], h16[0][k]) for k in ("icn_u8", "vunet_u8"))
    assert not ops.range_exceeded(DEV) and not ops.range_exceeded(DEV, word=pipe.status_word())


def test_the_state_serves_the_later_frame_drivers(env):
    """10: run_later_frame with a scene's state == run_later_frame with the same rows of the whole scene's state."""
    pipe, whole, w = env["pipe"], env["whole"], env["w"]
    got = pipe.run_frames_batched(env["slices"])
    later = pl.synth_later_frame(whole, 1)
    for g, (lo, hi) in zip(got, env["cuts"]):
        if hi == lo:
            continue
        sc = pl.slice_scene(later, lo, hi)
        a = pipe.run_later_frame(sc, g["state"])
        b = pipe.run_later_frame(sc, _whole_state_rows(w["state"], lo, hi))
        for k in ("icn_u8", "vunet_u8", "geom", "frame_icn", "frame_vunet"):
            assert torch.equal(a[k], b[k]), (lo, k)
    batched = pipe.run_later_frames_batched([pl.slice_scene(later, 2, 5)] * 2, got[2]["state"])
    want = pipe.run_later_frames_batched([pl.slice_scene(later, 2, 5)] * 2, _whole_state_rows(w["state"], 2, 5))
    for k in ("icn_u8", "vunet_u8", "frame_vunet"):
        assert torch.equal(batched[1][k], want[1][k]), k


def test_errors_and_the_empty_list(env):
    """11: mixed frame sizes and partial seeds raise before anything is launched; [] -> []; a list of scenes without vehicles."""
    pipe, own = env["pipe"], env["own"]
    assert pipe.run_frames_batched([]) == []
    small = pl.synth_frame(1, (180, 320), DEV, seed=2)
    small["vehicle_seeds"] = [1]
    with pytest.raises(ValueError, match="one size"):
        pipe.run_frames_batched([own[0], small])
    with pytest.raises(ValueError, match="vehicle_seeds"):
        pipe.run_frames_batched([own[0], {k: v for k, v in own[1].items() if k != "vehicle_seeds"}])
    with pytest.raises(ValueError, match="vehicle_seeds"):
        pipe.run_frames_batched([own[0], dict(own[1], vehicle_seeds=[1, 2])])
    with pytest.raises(ValueError, match="max_batch"):
        pipe.run_frames_batched(own[:2], max_batch=0)
    empty = pl.slice_scene(env["whole"], 2, 2)
    out = pipe.run_frames_batched([empty, dict(empty, background=torch.full_like(empty["frame"], 9))])
    assert len(out) == 2 and all(o["pose"] == [] and tuple(o["kp_idx"].shape) == (0, 12) and tuple(o["icn_u8"].shape) == (0, 256, 256, 3)
                                 for o in out)
    assert torch.equal(out[0]["frame_icn"], empty["frame"]) and bool((out[1]["frame_vunet"] == 9).all())
    want = pipe.run_frame(empty)
    assert set(out[0]) == set(want) | {"state"} and out[0]["state"]["shard"] == (0, 0, 0)
    later = pipe.run_later_frame(pl.slice_scene(pl.synth_later_frame(env["whole"], 1), 2, 2), out[0]["state"])
    assert tuple(later["icn_u8"].shape) == (0, 256, 256, 3) and torch.equal(later["frame_icn"], empty["frame"])


def test_geometry_mode_scenes_fall_back_to_run_frames(env):
    """11: a geometry-mode list goes through `run_frames` - the results of today - and records no frame_batch plan; a list that
    mixes both kinds of scene is refused."""
    from test_gpu_render import _geometry_setup
    pipe, _, scene = _geometry_setup(V=2)
    scenes = [scene, dict(scene, vehicle_seeds=[70, 71])]
    want = list(pipe.run_frames(scenes, replay=False))
    got = pipe.run_frames_batched(scenes)
    assert len(got) == 2 and not any(k[0] == "frame_batch" for k in pipe._frame_plans)
    for a, b in zip(got, want):
        for k in ("kp_idx", "icn_u8", "vunet_u8", "frame_icn", "frame_vunet"):
            assert torch.equal(a[k], b[k]), k
    with pytest.raises(ValueError, match="mixes"):
        pipe.run_frames_batched([scene, env["own"][1]])


# ------------------------------------------------------------------------------------------------ 8: inpainting
def _as_box_masks(sc):
    """A scene of synth_frame(inpaint="masks") with its detector masks cut to their boxes (the 'box_masks' form)."""
    inp = sc["inpaint"]
    return dict(sc, inpaint={"boxes": inp["boxes"], "box_masks": [m.to(DEV) for m in pl.synth_box_masks(inp["det_masks"].cpu(), inp["boxes"].tolist())]})


def test_inpainted_batch_matches_the_oracle_and_builds_its_inputs_per_scene():
    """Two scenes of 2 and 1 vehicles with scene['inpaint'] = {'boxes', 'box_masks'}: EdgeConnect's batched inputs are byte-equal to
    the per-scene op's, each scene's rows built from ITS image; the first scene meets the bars of
    test_run_frame_with_inpainting_matches_the_oracle (seed 17, that test's scene); presence is all-or-none."""
    ops.set_precision("f16x3")
    sds = {n: synth_sd(n) for n in ("hg", "icn", "vunet", "edge", "inpaint")}
    pipe = pl.VehiclePipeline(DEV, inpaint=True, state_dicts=sds)
    scenes = []
    for V, seed, base in ((2, 17, 40), (1, 41, 50)):
        sc = _as_box_masks(pl.synth_frame(V, HW, DEV, seed=seed, inpaint="masks"))
        sc["vehicle_seeds"] = [base + v for v in range(V)]
        scenes.append(sc)
    per_scene = [ops.inpaint_inputs_boxed(sc["frame"], sc["inpaint"]["box_masks"], sc["inpaint"]["boxes"]) for sc in scenes]
    ec, join = pipe._inpaint_inputs_rows(scenes, [0, 2, 3], 4, {})
    join()
    for k in ops.INPAINT_KEYS:
        assert torch.equal(ec[k][:3], torch.cat([four[k] for four in per_scene])), k
        assert not ec[k][3:].any(), k                                             # the padding row: zeros
    got = pipe.run_frames_batched(scenes)
    assert len(got) == 2 and tuple(got[0]["inpaint_u8"].shape) == (2, 256, 256, 3) and tuple(got[1]["inpaint_u8"].shape) == (1, 256, 256, 3)
    cpu = lr.scene_cpu({k: v for k, v in scenes[0].items() if k != "inpaint"})
    cpu["inpaint"] = dict(boxes=np.asarray(scenes[0]["inpaint"]["boxes"]), **{k: per_scene[0][k].cpu().numpy() for k in ops.INPAINT_KEYS})
    nt = torch.get_num_threads()
    torch.set_num_threads(_host_threads())
    try:
        ref = oracle.frame_pass(sds, cpu)
    finally:
        torch.set_num_threads(nt)
    g = got[0]
    d = int(np.abs(g["inpaint_u8"].cpu().numpy().astype(int) - ref["inpaint_u8"].astype(int)).max())
    record("frame_batch_inpaint_u8_max_diff", d)
    assert d <= 1
    assert np.array_equal(g["kp_idx"].cpu().numpy(), ref["kp_idx"])
    any_mask = cpu["masks"].max(0).astype(bool)
    cover = any_mask.copy()
    for x0, y0, x1, y1 in cpu["inpaint"]["boxes"]:
        cover[y0:y1, x0:x1] = True
    for k in ("frame_icn", "frame_vunet"):
        a = g[k].cpu().numpy()
        sv = oracle.ssim(a, ref[k])
        record(f"frame_batch_inpaint_{k}_ssim", sv, worst=min)
        assert sv >= 0.999, (k, sv)
        assert np.array_equal(a[~cover], cpu["frame"][~cover]), k
        assert int(np.abs(a.astype(int) - ref[k].astype(int))[~any_mask].max()) <= 2, k     # boxes: resize of a 1-LSB image
    rep = [pipe.run_frames_batched(scenes, replay=True) for _ in range(2)]        # recorded, then replayed into the plan's inputs
    assert ("frame_batch", 4, ops.PRECISION, "inpaint") in pipe._frame_plans
    pad = pipe.run_frames_batched(scenes, pad=True)
    for r in rep:
        for f in range(2):
            for k in KEYS + ("inpaint_u8",):
                assert torch.equal(r[f][k], pad[f][k]), (f, k)
    # presence is all-or-none among the scenes that have vehicles; a scene without vehicles decides nothing
    with pytest.raises(ValueError, match="inpaint"):
        pipe.run_frames_batched([scenes[0], {k: v for k, v in scenes[1].items() if k != "inpaint"}])
    with pytest.raises(ValueError, match="inpaint=True"):
        pipe.run_frames_batched([scenes[0], dict(scenes[1], inpaint={"boxes": scenes[1]["inpaint"]["boxes"]})])
    empty = {k: v for k, v in pl.slice_scene(scenes[1], 0, 0).items() if k != "inpaint"}
    mixed = pipe.run_frames_batched([scenes[0], empty, scenes[1]])
    for k in KEYS + ("inpaint_u8",):
        assert torch.equal(mixed[0][k], got[0][k]) and torch.equal(mixed[2][k], got[1][k]), k
    assert torch.equal(mixed[1]["frame_icn"], scenes[1]["frame"])
    with pytest.raises(ValueError, match="inpaint=True"):                         # no scene carries the key: `run_frame`'s refusal
        pipe.run_frames_batched([{k: v for k, v in sc.items() if k != "inpaint"} for sc in scenes])


# ------------------------------------------------------------------------------------------------ 9: the CAD classifier
def test_cad_indices_and_bank_keypoints_are_run_frames():
    """A pipeline built with cad=True, one scene of 3 vehicles with 'kp3d_bank' cut into slices of 2 and 1: 'cad_idx', and the
    pose fitted against the bank's chosen keypoints, are `run_frame`'s of the whole scene, bit for bit."""
    from future_urban_scene_generation_amd.cad_classifier import vgg19_schema
    from future_urban_scene_generation_amd.synth import synth_state_dict
    ops.set_precision("f16x3")
    sds = {n: synth_sd(n) for n in ("hg", "icn", "vunet")}
    sds["vgg"] = synth_state_dict("vgg", vgg19_schema(10), 0)
    pipe = pl.VehiclePipeline(DEV, state_dicts=sds, cad=True)
    sc = pl.synth_frame(3, HW, DEV, seed=23)
    sc["vehicle_seeds"] = [7, 8, 9]
    g = np.random.default_rng(4)
    sc["kp3d_bank"] = (g.uniform(-1, 1, (10, 12, 3)) * np.array([0.9, 0.5, 2.0]) * 5).astype(np.float32)
    w = pipe.run_frame(sc)
    got = pipe.run_frames_batched([pl.slice_scene(sc, 0, 2), pl.slice_scene(sc, 2, 3)])
    assert torch.equal(torch.cat([o["cad_idx"] for o in got]), w["cad_idx"]) and got[0]["cad_idx"].dtype == torch.int64
    for k in ("kp_idx", "kp_xy", "icn_u8", "vunet_u8"):
        assert torch.equal(torch.cat([o[k] for o in got]), w[k]), k
    assert _pose_equal([p for o in got for p in o["pose"]], w["pose"])
    # a scene that carries its own 'kp3d' beside one with the bank: each row is fitted against its own scene's points
    own_kp = dict(pl.slice_scene(sc, 2, 3))
    own_kp.pop("kp3d_bank")
    mixed = pipe.run_frames_batched([pl.slice_scene(sc, 0, 2), own_kp])
    assert _pose_equal(mixed[0]["pose"], w["pose"][:2])
    alone = pipe.run_frame(own_kp)
    assert _pose_equal(mixed[1]["pose"], alone["pose"])
    rep = pipe.run_frames_batched([pl.slice_scene(sc, 0, 2), pl.slice_scene(sc, 2, 3)], replay=True)
    assert ("frame_batch", 4, ops.PRECISION, "cad") in pipe._frame_plans
    pad = pipe.run_frames_batched([pl.slice_scene(sc, 0, 2), pl.slice_scene(sc, 2, 3)], pad=True)
    for a, b in zip(rep, pad):
        assert torch.equal(a["cad_idx"], b["cad_idx"]) and torch.equal(a["vunet_u8"], b["vunet_u8"])
