"""CPU: EdgeConnect's inputs from detector masks in BOX coordinates.  fusg_inpaint_inputs_boxed_host (the code the device
kernels run) against fusg_inpaint_inputs_host on the same masks scattered into frame-sized planes, byte for byte; the float
binarisation; the host twin's bounds checks; the third scene form; ragged slicing; the default later scene unchanged."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from future_urban_scene_generation_amd import _lib as L                    # noqa: E402
from future_urban_scene_generation_amd import ops                          # noqa: E402
from future_urban_scene_generation_amd import pipeline as pl               # noqa: E402

H, W = 64, 96
# (x0, y0, x1, y1), w x h: 5 x 7; 33 x 9, which crosses the 32 x 8 dilate tile in both directions; one that ends at the right
# and bottom frame border; one zero-extent
BOXES = np.array([[3, 2, 8, 9], [20, 4, 53, 13], [80, 50, 96, 64], [40, 30, 40, 30]], dtype=np.int64)


def boxed_case(seed=0):
    """frame, per-vehicle u8 pieces (values 0, 255 and others) and the same masks as frame-sized planes (garbage outside the
    box: it must not be read)."""
    g = np.random.default_rng(seed)
    frame = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    pieces, planes = [], g.integers(0, 256, (len(BOXES), 1, H, W), dtype=np.uint8)
    for v, (x0, y0, x1, y1) in enumerate(BOXES):
        h, w = y1 - y0, x1 - x0
        m = np.zeros((h, w), np.uint8)                                         # a blob in the middle: holes and non-holes both exist
        m[h // 3:h // 3 + max(h // 4, 1), w // 3:w // 3 + max(w // 4, 1)] = g.choice(
            np.array([0, 255, 255, 7, 128, 254], dtype=np.uint8), size=m[h // 3:h // 3 + max(h // 4, 1), w // 3:w // 3 + max(w // 4, 1)].shape)
        pieces.append(np.ascontiguousarray(m))
        planes[v, 0, y0:y1, x0:x1] = m
    return frame, pieces, planes


@pytest.fixture(scope="module")
def case():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    frame, pieces, planes = boxed_case()
    return dict(frame=frame, pieces=pieces, planes=planes, ref=ops.inpaint_inputs_host(frame, planes, BOXES),
                boxed=ops.inpaint_inputs_boxed_host(frame, pieces, BOXES))


def test_exports():
    lib = L.lib()
    for name in ("fusg_inpaint_inputs_boxed", "fusg_inpaint_inputs_boxed_host"):
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert lib.fusg_version() == 118


def test_boxed_u8_is_byte_equal_to_the_frame_form(case):
    for k in ops.INPAINT_KEYS:
        assert case["boxed"][k].dtype == np.float32 and case["boxed"][k].shape == case["ref"][k].shape
        assert case["boxed"][k].tobytes() == case["ref"][k].tobytes(), (k, int((case["boxed"][k] != case["ref"][k]).sum()))
    # not vacuous: holes, edges and non-hole pixels exist, a 128 that dilates but does not whiten is in play, and the
    # zero-extent box gives zeros
    assert 0 < case["ref"]["mask"][:3].mean() < 1 and case["ref"]["edge"][:3].sum() > 0
    assert all(float(np.abs(case["boxed"][k][3]).max()) == 0.0 for k in ops.INPAINT_KEYS)
    assert any(((p != 0) & (p != 255)).any() for p in case["pieces"])


def test_packed_pair_and_3d_pieces_equal_the_list(case):
    offs = np.zeros(len(BOXES), np.int64)
    offs[1:] = np.cumsum([p.size for p in case["pieces"]])[:-1]
    buf = np.concatenate([p.reshape(-1) for p in case["pieces"]])
    a = ops.inpaint_inputs_boxed_host(case["frame"], (buf, offs), BOXES)
    b = ops.inpaint_inputs_boxed_host(case["frame"], [p[None] for p in case["pieces"]], BOXES)
    # the pieces in another order inside the buffer, with a gap in front
    order = [2, 0, 3, 1]
    offs2, parts, at = np.zeros(len(BOXES), np.int64), [np.full(5, 99, np.uint8)], 5
    for v in order:
        offs2[v] = at
        parts.append(case["pieces"][v].reshape(-1))
        at += case["pieces"][v].size
    c = ops.inpaint_inputs_boxed_host(case["frame"], (np.concatenate(parts), offs2), BOXES)
    for k in ops.INPAINT_KEYS:
        assert a[k].tobytes() == case["boxed"][k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


def test_f32_masks_binarise_as_the_reference_does(case):
    g = np.random.default_rng(5)
    fl = []
    for p in case["pieces"]:
        m = np.where(p > 0, g.choice(np.array([1.0, 0.5, 1e-30, -0.25, -0.0], dtype=np.float32), size=p.shape), 0).astype(np.float32)
        if m.size:
            m.flat[0], m.flat[m.size // 2], m.flat[-1] = np.nan, -1.0, np.float32(1e-40)      # NaN, negative, a denormal
        fl.append(m)
    with np.errstate(invalid="ignore"):
        u8 = [np.where(m * np.float32(255.0) > 0, 255, 0).astype(np.uint8) for m in fl]
    assert all(u[0, 0] == 0 for u in u8 if u.size)                                             # the NaN gives 0
    a = ops.inpaint_inputs_boxed_host(case["frame"], fl, BOXES)
    b = ops.inpaint_inputs_boxed_host(case["frame"], u8, BOXES)
    for k in ops.INPAINT_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert 0 < b["mask"][:3].mean() < 1


def test_host_twin_refuses_masks_outside_the_buffer(case):
    offs = np.zeros(len(BOXES), np.int64)
    offs[1:] = np.cumsum([p.size for p in case["pieces"]])[:-1]
    buf = np.concatenate([p.reshape(-1) for p in case["pieces"]])
    with pytest.raises(L.FusgError, match="leaves the buffer"):                # a short buffer
        ops.inpaint_inputs_boxed_host(case["frame"], (buf[:-1].copy(), offs), BOXES)
    neg = offs.copy()
    neg[1] = -1
    with pytest.raises(L.FusgError, match="leaves the buffer"):                # a negative offset
        ops.inpaint_inputs_boxed_host(case["frame"], (buf, neg), BOXES)
    far = offs.copy()
    far[3] = buf.size + 1                                                      # even for a zero-extent box
    with pytest.raises(L.FusgError, match="leaves the buffer"):
        ops.inpaint_inputs_boxed_host(case["frame"], (buf, far), BOXES)
    ok = offs.copy()
    ok[3] = buf.size                                                           # ... whose mask may end exactly at the end
    ops.inpaint_inputs_boxed_host(case["frame"], (buf, ok), BOXES)


def test_ops_validation(case):
    wrong = list(case["pieces"])
    wrong[1] = np.zeros((9, 34), np.uint8)
    with pytest.raises(ValueError, match=r"box_masks\[1\] is 9 x 34"):
        ops.inpaint_inputs_boxed_host(case["frame"], wrong, BOXES)
    with pytest.raises(ValueError, match="all uint8 or all float32"):
        ops.inpaint_inputs_boxed_host(case["frame"], [case["pieces"][0].astype(np.float32)] + case["pieces"][1:], BOXES)
    with pytest.raises(ValueError, match="all uint8 or all float32"):
        ops.inpaint_inputs_boxed_host(case["frame"], [p.astype(np.int32) for p in case["pieces"]], BOXES)
    with pytest.raises(ValueError, match=r"\[h, w\] or \[1, h, w\]"):
        ops.inpaint_inputs_boxed_host(case["frame"], [p[None, None] for p in case["pieces"]], BOXES)
    with pytest.raises(ValueError, match="boxes"):
        ops.inpaint_inputs_boxed_host(case["frame"], case["pieces"][:3], BOXES)
    with pytest.raises(ValueError, match="leaves the"):
        ops.inpaint_inputs_boxed_host(case["frame"], case["pieces"], BOXES + np.array([0, 0, 40, 0]))
    empty = ops.inpaint_inputs_boxed_host(case["frame"], [], np.zeros((0, 4), np.int64))
    assert empty["img"].shape == (0, 3, 256, 256) and empty["edge"].shape == (0, 1, 256, 256)


def test_scene_form_accepts_box_masks_and_rejects_mixtures():
    t = object()
    four = dict(img=t, gray=t, edge=t, mask=t)
    assert pl.inpaint_scene_form({"boxes": t, "box_masks": [t]}) == "box_masks"
    assert pl.inpaint_scene_form({"boxes": t, "det_masks": t}) == "det_masks"
    assert pl.inpaint_scene_form({"boxes": t, **four}) == "given"
    for bad in ({"boxes": t, "box_masks": [t], "det_masks": t}, {"boxes": t, "box_masks": [t], **four}, {"box_masks": [t]},
                {"boxes": t, "box_masks": [t], "img": t}, {"boxes": t}, None):
        with pytest.raises(ValueError, match="box_masks"):
            pl.inpaint_scene_form(bad)


def test_slice_and_select_of_ragged_box_masks():
    pieces = [np.full((2 + v, 3 + v), v, np.uint8) for v in range(5)]
    boxes = np.arange(20).reshape(5, 4)
    scene = {"frame": None, "bboxes": np.zeros((5, 4), np.int64), "inpaint": {"boxes": boxes, "box_masks": pieces}}
    sub = pl.slice_scene(scene, 1, 4)
    assert [p.shape for p in sub["inpaint"]["box_masks"]] == [(3, 4), (4, 5), (5, 6)]
    assert all(a is b for a, b in zip(sub["inpaint"]["box_masks"], pieces[1:4])) and np.array_equal(sub["inpaint"]["boxes"], boxes[1:4])
    assert pl.slice_scene(scene, 5, 5)["inpaint"]["box_masks"] == []
    buf, offs = np.arange(100, dtype=np.uint8), np.array([0, 6, 18, 38, 68], np.int64)
    for off in (offs, torch.from_numpy(offs)):
        scene["inpaint"]["box_masks"] = (buf, off)
        b2, o2 = pl.slice_scene(scene, 2, 5)["inpaint"]["box_masks"]
        assert b2 is buf and np.array_equal(np.asarray(o2), offs[2:5])
        kept = pl.VehiclePipeline._select(scene, [4, 1], ("bboxes", "inpaint"))["inpaint"]
        assert kept["box_masks"][0] is buf and np.array_equal(np.asarray(kept["box_masks"][1]), offs[[4, 1]])
        assert np.array_equal(kept["boxes"], boxes[[4, 1]])
    scene["inpaint"]["box_masks"] = pieces
    kept = pl.VehiclePipeline._select(scene, [3, 0], ("bboxes", "inpaint"))["inpaint"]
    assert kept["box_masks"][0] is pieces[3] and kept["box_masks"][1] is pieces[0] and len(kept["box_masks"]) == 2


def host_scene(V=3, hw=(48, 64)):
    """What `synth_later_frame` reads of a `synth_frame` scene, on the host."""
    g = np.random.default_rng(3)
    Hh, Ww = hw
    masks = np.zeros((V, Hh, Ww), np.uint8)
    bboxes = []
    for v in range(V):
        x0, y0 = 4 + 14 * v, 6 + 5 * v
        masks[v, y0 + 2:y0 + 12, x0 + 2:x0 + 16] = 1
        bboxes.append([x0, y0, x0 + 18, y0 + 14])
    return {"frame": torch.from_numpy(g.integers(0, 256, (Hh, Ww, 3), dtype=np.uint8)), "bboxes": np.asarray(bboxes, np.int64),
            "masks": torch.from_numpy(masks), "src_sketch": torch.from_numpy(g.integers(0, 256, (V, Hh, Ww, 3), dtype=np.uint8)),
            "dst_sketch": torch.zeros((V, Hh, Ww, 3), dtype=torch.uint8),
            "src_kp": [[np.int32(g.integers(0, 40, (4, 2))) for _ in range(5)] for _ in range(V)], "vehicle_seeds": [5, 6, 7][:V]}


def test_synth_later_frame_default_is_unchanged_and_forms_are_consistent():
    sc = host_scene()
    a = pl.synth_later_frame(sc, 3)
    # today's scene, restated: every key compared
    g = np.random.default_rng(1003)
    want = dict(sc)
    want["dst_kp"] = [[np.int32(p + g.normal(0, 3.0, p.shape)) for p in veh] for veh in sc["src_kp"]]
    want["dst_sketch"] = sc["src_sketch"]
    want["vehicle_seeds"] = [int(sd) * 64 + 3 for sd in sc["vehicle_seeds"]]
    assert set(a) == set(want) and "inpaint" not in a
    for k in want:
        if k == "dst_kp":
            assert all(np.array_equal(p, q) and p.dtype == q.dtype for va, vb in zip(a[k], want[k]) for p, q in zip(va, vb))
        elif k in ("src_kp", "vehicle_seeds"):
            assert a[k] == want[k] if k == "vehicle_seeds" else a[k] is want[k]
        else:
            assert a[k] is want[k], k
    # a first frame's entry passes through untouched
    first = dict(sc, inpaint={"boxes": 1})
    assert pl.synth_later_frame(first, 3)["inpaint"] is first["inpaint"]
    # the three forms describe the same boxes and masks, and leave the rest of the scene as it is
    forms = {f: pl.synth_later_frame(sc, 3, inpaint=f) for f in ("given", "masks", "box_masks")}
    for f, s in forms.items():
        assert pl.inpaint_scene_form(s["inpaint"]) == {"given": "given", "masks": "det_masks", "box_masks": "box_masks"}[f]
        assert np.array_equal(s["inpaint"]["boxes"], forms["masks"]["inpaint"]["boxes"])
        assert all(np.array_equal(p, q) for va, vb in zip(s["dst_kp"], a["dst_kp"]) for p, q in zip(va, vb))
    boxes, planes = forms["masks"]["inpaint"]["boxes"], forms["masks"]["inpaint"]["det_masks"]
    assert tuple(planes.shape) == (3, 1, 48, 64) and planes.dtype == torch.uint8 and int(planes.max()) == 255
    for v, (x0, y0, x1, y1) in enumerate(boxes):
        assert 0 <= x0 < x1 <= 64 and 0 <= y0 < y1 <= 48
        assert torch.equal(forms["box_masks"]["inpaint"]["box_masks"][v], planes[v, 0, y0:y1, x0:x1])
    fl = pl.synth_box_masks(planes, boxes, torch.float32)
    assert all(p.dtype == torch.float32 and float(p.max()) <= 1.0 and torch.equal((p * 255 > 0), q > 0)
               for p, q in zip(fl, forms["box_masks"]["inpaint"]["box_masks"]))
    assert not np.array_equal(pl.synth_later_frame(sc, 4, inpaint="masks")["inpaint"]["boxes"], boxes)       # the boxes move
    with pytest.raises(ValueError, match="inpaint"):
        pl.synth_later_frame(sc, 3, inpaint="other")
