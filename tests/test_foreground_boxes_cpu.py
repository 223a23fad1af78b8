"""CPU: vehicle boxes from the background (ops.foreground_boxes, VehiclePipeline.detect_vehicles / bootstrap_background) without
a device - the numpy restatement of the definition equals SciPy's label + find_objects; the host twin, which runs the kernel's
code (csrc/foreground_boxes.h), equals the restatement on every case, bit for bit, inside canaries; the cases have the answers
written beside them and tell the right rule from four wrong ones; the library refuses every bad argument on the host; and the two
pipeline methods are pure Python over ops."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import foreground_boxes_cases as bc
from conftest import REPO
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import ops
from future_urban_scene_generation_amd import pipeline as pl

NEW = {"fusg_foreground_boxes_u8": 20, "fusg_foreground_boxes_scratch_bytes": 4, "fusg_foreground_boxes_host": 18}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def test_the_new_exports_are_declared_bound_and_built(lib):
    hdr = open(os.path.join(REPO, "include", "fusg.h")).read()
    declared = set(re.findall(r"\b(fusg_[a-z0-9_]+)\s*\(", hdr))
    for name, nargs in NEW.items():
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
        assert len(L._SIGS[name][1]) == nargs, name
    assert lib.fusg_version() == 118
    mk = open(os.path.join(REPO, "future_urban_scene_generation_amd", "csrc", "Makefile")).read()
    assert " foreground_boxes.hip" in mk and re.search(r"^foreground_boxes\.o:.* foreground_boxes\.h", mk, re.M)
    assert re.search(r"^foreground_boxes\.o: CXXFLAGS \+= -Rpass-analysis=kernel-resource-usage", mk, re.M)


def host_run(c):
    """The host twin's three tables for a case, CANARY-filled before."""
    T, K = len(c["frames"]), c["params"]["max_boxes"]
    out = tuple(np.full(s, bc.CANARY, dtype=np.int32) for s in ((T, K, 4), (T, K, 2), (T, 4)))
    got = ops.foreground_boxes_host(c["frames"], c["backgrounds"], out=out, **c["params"])
    assert all(g is o for g, o in zip(got, out))
    return got


@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_host_twin_equals_the_restatement(lib, name):
    c = bc.BY_NAME[name]
    for what, got, want in zip(("boxes", "box_stats", "stats"), host_run(c), bc.expected(name)):
        assert got.dtype == np.int32 and np.array_equal(got, want), (what, got, want)
    boxes, box_stats, stats = host_run(c)
    for f in range(len(c["frames"])):                             # the rows past the last box are zeros, not the canary
        v = min(int(stats[f, 0]), c["params"]["max_boxes"])
        assert not boxes[f, v:].any() and not box_stats[f, v:].any()
        assert np.all(boxes[f, :v, 2] > boxes[f, :v, 0]) and np.all(box_stats[f, :v] > 0)


@pytest.mark.parametrize("name", [c["name"] for c in bc.CASES if c["want_stats"] is not None])
def test_the_restatement_gives_the_answers_written_beside_the_cases(name):
    c = bc.BY_NAME[name]
    boxes, _, stats = bc.expected(name)
    n_kept, n_exam, flags = c["want_stats"]
    assert (int(stats[0, 0]), int(stats[0, 1]), int(stats[0, 3])) == (n_kept, n_exam, flags)
    if c["want"] is not None:
        assert np.array_equal(boxes[0, :len(c["want"])], c["want"]) and not boxes[0, len(c["want"]):].any()


def test_the_named_cases_are_what_they_say():
    x = {n: bc.expected(n) for n in bc.CASE_NAMES}
    assert [bc.grid(np.zeros(c["frames"][0].shape[:2], bool), 4)[0].shape[1] for c in map(bc.BY_NAME.get, ("seam_37x70", "seam_37x133", "seam_21x260"))] \
        == [18, 34, 65]
    for n in ("seam_37x70", "seam_37x133", "seam_21x260"):
        assert x[n][2][0, 0] >= 3 and x[n + "_open1_close1"][2][0, 0] >= 1
        assert not np.array_equal(x[n][0], x[n + "_open1_close1"][0])
    assert np.array_equal(x["all_foreground"][0][0, 0], bc.roi_of(bc.BY_NAME["all_foreground"]))
    assert x["checkerboard_288"][2][0].tolist() == [256, 256, 288 * 16, 3]
    assert x["spiral"][1][0, 0, 1] == int(bc._spiral(15).sum()) > 100
    three = x["three_frames_one_background"]
    assert three[2].shape == (3, 4) and len({three[0][f].tobytes() for f in range(3)}) == 3 and np.all(three[2][:, 0] >= 1)
    c3 = bc.BY_NAME["three_frames_one_background"]
    assert c3["backgrounds"][0] is c3["backgrounds"][1] is c3["backgrounds"][2]
    assert x["cell8"][2][0, 0] >= 2 and x["cell16"][2][0, 0] >= 1
    # the cells the closing added - the gap's two columns and, the blob being one cell from the frame edge whose outside counts as
    # 1, column 0 - bring no pixels: n_cells counts them, area and the box do not
    assert x["close_joins_gap2_not_gap3"][1][0, 0].tolist() == [2 * 9 * 16, 3 * 9]


@pytest.mark.parametrize("wrong, name", [("eight", "diagonal_touch"), ("gt", "count_edge"), ("cellbox", "tight_box"), ("close0", "close_at_edge")])
def test_a_wrong_restatement_fails_its_named_case(lib, wrong, name):
    c = bc.BY_NAME[name]
    bad, good, got = bc.reference(c, wrong), bc.expected(name), host_run(c)
    assert not all(np.array_equal(a, b) for a, b in zip(bad, good)), "the case does not tell the wrong rule from the right one"
    assert all(np.array_equal(a, b) for a, b in zip(got, good))


@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_restatement_is_scipy_label_and_find_objects(name):
    """Components, their order and their tight boxes: scipy.ndimage.label (4-connected by default, labels in raster order of the
    first cell) on G2, and find_objects on the P pixels numbered by the label of their cell."""
    ndi = pytest.importorskip("scipy.ndimage")
    c = bc.BY_NAME[name]
    p = dict(c["params"], min_area=1, min_w=1, min_h=1, max_boxes=bc.MAX_COMPONENTS)
    for fr, bg in zip(c["frames"], c["backgrounds"]):
        cnt, pad = bc.grid(bc.pixels(fr, bg, p["thr"], p["roi"]), p["cell"])
        G2 = bc.g2_of(cnt, p)
        lab, n = ndi.label(G2)
        comps, more = bc.components(G2)
        assert more == (n > bc.MAX_COMPONENTS) and len(comps) == min(n, bc.MAX_COMPONENTS)
        for q, comp in enumerate(comps):
            assert np.array_equal(comp, lab == q + 1)
        up = np.repeat(np.repeat(lab, p["cell"], axis=0), p["cell"], axis=1) * pad
        want = [(s[1].start, s[0].start, s[1].stop, s[0].stop) for s in ndi.find_objects(up, max_label=len(comps)) if s is not None]
        boxes, box_stats, stats = bc.frame_reference(fr, bg, p)
        assert stats[0] == len(want) and boxes[:len(want)].tolist() == [list(w) for w in want]
        assert box_stats[:len(want), 0].tolist() == [int(v) for v in ndi.sum(pad, up, [q + 1 for q in range(len(comps))]) if v > 0]


def test_label_order_is_raster_first_order_on_random_grids():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    for _ in range(300):
        G = rng.random((int(rng.integers(1, 13)), int(rng.integers(1, 40)))) < rng.uniform(0.2, 0.7)
        lab, n = ndi.label(G)
        comps, _ = bc.components(G)
        assert len(comps) == n and all(np.array_equal(comp, lab == q + 1) for q, comp in enumerate(comps))


def _raw(c, **kw):
    """The library's argument list for frame 0 of a case, host pointers, with replacements by name."""
    p = c["params"]
    H, W = c["frames"][0].shape[:2]
    K = kw.get("K", p["max_boxes"])
    keep = dict(fp=(C.c_void_p * 1)(c["frames"][0].ctypes.data), gp=(C.c_void_p * 1)(c["backgrounds"][0].ctypes.data),
                roi=(C.c_int32 * 4)(*bc.roi_of(c)), boxes=np.zeros((max(K, 1), 4), np.int32), box_stats=np.zeros((max(K, 1), 2), np.int32),
                stats=np.zeros((4,), np.int32))
    a = dict(frames=keep["fp"], backgrounds=keep["gp"], T=1, H=H, W=W, thr=p["thr"], cell=p["cell"], min_count=p["min_count"],
             open_r=p["open_r"], close_r=p["close_r"], min_area=p["min_area"], min_w=p["min_w"], min_h=p["min_h"], roi=keep["roi"], K=K,
             boxes=keep["boxes"].ctypes.data, box_stats=keep["box_stats"].ctypes.data, stats=keep["stats"].ctypes.data)
    a.update(kw)
    return list(a.values()), keep


def test_the_library_checks_its_arguments_on_the_host(lib):
    """Both entry points, the device one included, refuse every bad range and table before anything is launched or touched:
    nothing here is a device pointer."""
    c = bc.BY_NAME["tight_box"]                                    # 24 x 28
    a, keep = _raw(c)
    assert lib.fusg_foreground_boxes_host(*a) == 0 and keep["stats"][0] == 1
    i4 = lambda *v: (C.c_int32 * 4)(*v)  # noqa: E731
    bad = [dict(T=0), dict(T=65), dict(frames=None), dict(backgrounds=None), dict(frames=(C.c_void_p * 1)(None)),
           dict(backgrounds=(C.c_void_p * 1)(None)), dict(H=0), dict(W=0), dict(H=32768), dict(W=32768), dict(thr=-1), dict(thr=255),
           dict(cell=0), dict(cell=2), dict(cell=5), dict(cell=32), dict(min_count=0), dict(min_count=17), dict(cell=8, min_count=65),
           dict(open_r=-1), dict(open_r=4), dict(close_r=-1), dict(close_r=8), dict(min_area=0), dict(min_w=0), dict(min_h=0), dict(K=0),
           dict(K=65), dict(roi=None), dict(roi=i4(-1, 0, 28, 24)), dict(roi=i4(0, -1, 28, 24)), dict(roi=i4(0, 0, 29, 24)),
           dict(roi=i4(0, 0, 28, 25)), dict(roi=i4(9, 0, 8, 24)), dict(roi=i4(0, 9, 28, 8)), dict(boxes=None), dict(box_stats=None),
           dict(stats=None)]
    scratch = np.zeros((64,), np.int32)
    for kw in bad:
        a, _ = _raw(c, **kw)
        assert lib.fusg_foreground_boxes_host(*a) == -1, kw
        assert lib.fusg_last_error()
        assert lib.fusg_foreground_boxes_u8(*a, scratch.ctypes.data, None) == -1, kw
    a, _ = _raw(c)
    assert lib.fusg_foreground_boxes_u8(*a, None, None) == -1 and b"scratch" in lib.fusg_last_error()
    assert lib.fusg_foreground_boxes_u8(*a, scratch.ctypes.data + 2, None) == -1 and b"aligned" in lib.fusg_last_error()
    # the grid's planes against the LDS budget: 2 planes of gh * words(gw) words and 512 bytes must fit 64 KiB
    for H, W, cell, ok in ((720, 1280, 4, True), (4 * 254, 4 * 1024, 4, True), (4 * 255, 4 * 1024, 4, False), (32767, 32767, 16, False),
                           (16 * 254, 16 * 1024, 16, True)):
        a, _ = _raw(c, H=H, W=W, cell=cell, roi=i4(0, 0, 1, 1))
        a[0] = a[1] = (C.c_void_p * 1)(1)                          # never read: an accepted call is stopped at the null scratch
        rc, msg = lib.fusg_foreground_boxes_u8(*a, None, None), lib.fusg_last_error()
        assert rc == -1 and ((b"scratch" in msg) if ok else (b"raise cell" in msg)), (H, W, cell, msg)
    sb = lib.fusg_foreground_boxes_scratch_bytes
    assert sb(1, 720, 1280, 4) == 4 * 180 * 320 and sb(3, 37, 70, 4) == 3 * 4 * 10 * 18 and sb(2, 17, 17, 16) == 2 * 4 * 2 * 2
    assert sb(0, 8, 8, 4) == -1 and sb(65, 8, 8, 4) == -1 and sb(1, 0, 8, 4) == -1 and sb(1, 8, 32768, 4) == -1 and sb(1, 8, 8, 3) == -1


def test_ops_validation(lib):
    c = bc.BY_NAME["tight_box"]
    fr, bg = c["frames"][0], c["backgrounds"][0]
    for kw, err in ((dict(thr=1.5), ValueError), (dict(roi=(0, 0, 5)), ValueError), (dict(roi=(0.0, 0, 5, 5)), ValueError),
                    (dict(max_boxes=0), ValueError), (dict(max_boxes=65), ValueError), (dict(cell=5), L.FusgError), (dict(min_area=0), L.FusgError)):
        with pytest.raises(err):
            ops.foreground_boxes_host(fr, bg, **kw)
    with pytest.raises(ValueError):
        ops.foreground_boxes_host(fr, bg[:, :-1])
    with pytest.raises(ValueError):
        ops.foreground_boxes_host([fr, fr], [bg])
    with pytest.raises(ValueError):
        ops.foreground_boxes_host(fr, bg, out=(np.zeros((1, 64, 4), np.int64), np.zeros((1, 64, 2), np.int32), np.zeros((1, 4), np.int32)))
    a = ops.foreground_boxes_host(np.stack([fr, fr]), bg, min_count=1, min_area=1, min_w=1, min_h=1, cell=4)   # a stack, one background
    assert a[0].shape == (2, 64, 4) and a[0][0, 0].tolist() == [6, 5, 21, 18] and np.array_equal(a[0][0], a[0][1])


def test_pipeline_methods_are_pure_python_over_ops(monkeypatch):
    """detect_vehicles: the tables of every chunk of 64 scenes, ONE read-back, the rows that hold a box; bootstrap_background: the
    median without boxes, the detection against it, the median with the boxes (inclusive ends), in that order."""
    calls, K = [], 3

    def boxes_op(frames, backgrounds, **kw):
        T = len(frames)
        calls.append(("boxes", T, backgrounds, kw))
        boxes, box_stats, stats = torch.zeros((T, K, 4), dtype=torch.int32), torch.zeros((T, K, 2), dtype=torch.int32), torch.zeros((T, 4), dtype=torch.int32)
        for f in range(T):
            v = int(frames[f][0, 0, 0]) % 5                        # n_kept 0..4, K = 3: the last one overflows
            stats[f] = torch.tensor([v, v + 1, 100 + f, 1 if v > K else 0])
            for k in range(min(v, K)):
                boxes[f, k] = torch.tensor([10 * k, f, 10 * k + 5, f + 7])
                box_stats[f, k] = torch.tensor([50 + k, 4])
        return boxes, box_stats, stats

    def d2h(t):
        calls.append(("d2h", tuple(t.shape)))
        return t.numpy()

    def median(frames, boxes=None, margin=0, min_valid=1, out=None):
        calls.append(("median", len(frames), None if boxes is None else [np.asarray(b).tolist() for b in boxes], margin, min_valid))
        return torch.full((8, 8, 3), sum(c[0] == "median" for c in calls), dtype=torch.uint8), "count"
    monkeypatch.setattr(ops, "foreground_boxes", boxes_op)
    monkeypatch.setattr(ops, "d2h", d2h)
    monkeypatch.setattr(ops, "background_median", median)
    pipe = object.__new__(pl.VehiclePipeline)
    scenes = [{"frame": torch.full((8, 8, 3), f % 5, dtype=torch.uint8)} for f in range(70)]
    keys = [set(s) for s in scenes]
    bg = torch.zeros((8, 8, 3), dtype=torch.uint8)
    out = pipe.detect_vehicles(scenes, bg, thr=30)
    assert [c[:2] for c in calls] == [("boxes", 64), ("boxes", 6), ("d2h", (70, 6 * K + 4))]
    assert calls[0][2] is bg and calls[0][3] == {"thr": 30}
    assert len(out) == 70 and [set(o) for o in out] == [{"bboxes", "area", "stats"}] * 70
    for f, o in enumerate(out):
        v = f % 5
        assert o["bboxes"].dtype == np.int64 and o["bboxes"].shape == (min(v, K), 4) and o["area"].dtype == np.int64
        assert o["bboxes"].tolist() == [[10 * k, f % 64, 10 * k + 5, f % 64 + 7] for k in range(min(v, K))]
        assert o["area"].tolist() == [50 + k for k in range(min(v, K))]
        assert o["stats"].tolist() == [v, v + 1, 100 + f % 64, 1 if v > K else 0]
    assert [set(s) for s in scenes] == keys
    assert pipe.detect_vehicles([], bg) == []
    per_scene = torch.zeros((70, 8, 8, 3), dtype=torch.uint8)
    del calls[:]
    pipe.detect_vehicles(scenes, per_scene)
    assert [len(c[2]) for c in calls[:2]] == [64, 6] and calls[1][2][0].data_ptr() == per_scene[64].data_ptr()
    del calls[:]
    got = pipe.bootstrap_background(scenes[:9], margin=5, thr=20)
    assert [c[0] for c in calls] == ["median", "boxes", "d2h", "median"]
    assert calls[0] == ("median", 9, None, 5, 1) and int(calls[1][2][0, 0, 0]) == 1 and calls[1][3] == {"thr": 20}
    want = [[[10 * k, f, 10 * k + 5, f + 7] for k in range(min(f % 5, K))] for f in range(9)]
    assert calls[3] == ("median", 9, [[[b[0], b[1], b[2] - 1, b[3] - 1] for b in w] for w in want], 5, 1)
    assert set(got) == {"background", "count", "frames", "min_valid", "bboxes"} and int(got["background"][0, 0, 0]) == 2 and got["frames"] == list(range(9))
    assert [b.tolist() for b in got["bboxes"]] == want and [set(s) for s in scenes] == keys
    del calls[:]
    got = pipe.bootstrap_background(scenes[:4], rounds=2, min_valid=2)
    assert [c[0] for c in calls] == ["median", "boxes", "d2h", "median", "boxes", "d2h", "median"] and int(calls[4][2][0, 0, 0]) == 2 and int(got["background"][0, 0, 0]) == 3
    assert got["min_valid"] == 2 and calls[0][4] == 2
