"""CPU: the background estimator (ops.background_median, VehiclePipeline.estimate_background) without a device - the host twin,
which runs the kernel's per-dword code (csrc/background.h), equals the numpy restatement of the definition on every case, bit for
bit; the restatement equals np.median where the two definitions meet, and the cases tell the right rule from two wrong ones;
every validation error is raised before anything runs; the new symbols are declared, bound and built; the frame-sampling rule
of estimate_background is pure Python."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import background_cases as bc
from conftest import REPO
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import ops
from future_urban_scene_generation_amd import pipeline as pl

NEW = ("fusg_background_median_u8", "fusg_background_median_host")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def test_the_new_exports_are_declared_bound_and_built(lib):
    hdr = open(os.path.join(REPO, "include", "fusg.h")).read()
    declared = set(re.findall(r"\b(fusg_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert len(L._SIGS[NEW[0]][1]) == 11 and len(L._SIGS[NEW[1]][1]) == 10
    assert lib.fusg_version() == 118
    mk = open(os.path.join(REPO, "future_urban_scene_generation_amd", "csrc", "Makefile")).read()
    assert " background.hip" in mk and " background.h " in mk


@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_host_twin_equals_the_reference(lib, name):
    c = bc.BY_NAME[name]
    bg, count = ops.background_median_host(c["frames"], c["boxes"], c["margin"], c["min_valid"])
    ebg, ecount = bc.expected(name)
    assert bg.dtype == np.uint8 and count.dtype == np.uint8 and bg.shape == ebg.shape and count.shape == ecount.shape
    assert np.array_equal(count, ecount)
    assert np.array_equal(bg, ebg)


def test_host_twin_takes_a_stack_and_separate_frames_alike(lib):
    c = bc.BY_NAME["t9_33x130"]
    a = ops.background_median_host(np.stack(c["frames"]), c["boxes"], c["margin"], c["min_valid"])
    b = bc.expected("t9_33x130")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("T", [1, 3, 9, 17, 33, 63])
def test_reference_is_np_median_for_odd_t_without_boxes(T):
    """The definition, not the code: with an odd number of samples the lower median is the median."""
    r = np.random.default_rng(T)
    frames = r.integers(0, 256, (T, 6, 9, 3)).astype(np.uint8)
    bg, count = bc.reference(list(frames))
    assert np.array_equal(bg, np.median(frames, axis=0).astype(np.uint8)) and np.all(count == T)


def test_value_occurred_and_channels_pick_different_frames():
    bg, _ = bc.expected("channels_differ")
    assert np.all(bg == np.asarray([20, 21, 22], dtype=np.uint8))               # frame 1's, frame 2's and frame 0's
    c = bc.BY_NAME["n_even_odd"]
    bg, _ = bc.expected("n_even_odd")
    st = np.stack(c["frames"])
    assert np.all((st == bg[None]).any(axis=0))                                  # never an average


def test_the_cases_do_not_pass_vacuously():
    """A reference with the upper median, or with half-open box ends, disagrees with the right one on named cases - so a host twin
    or a kernel with either mistake cannot pass them."""
    for name in ("n_even_odd", "t2_5x7", "t64_1x1", "min_valid_1_n5_t8"):
        c = bc.BY_NAME[name]
        wrong, _ = bc.reference(c["frames"], c["boxes"], c["margin"], c["min_valid"], upper=True)
        assert not np.array_equal(wrong, bc.expected(name)[0]), name
    for name in ("borders", "t2_1x1_box", "fallback_and_one", "outside"):
        c = bc.BY_NAME[name]
        wrong = bc.reference(c["frames"], c["boxes"], c["margin"], c["min_valid"], exclusive=True)
        assert not np.array_equal(wrong[1], bc.expected(name)[1]), name
    # and the table holds what it claims: fallback pixels, pixels one frame sees, even and odd n
    _, n = bc.expected("fallback_and_one")
    assert (n == 0).any() and (n == 1).any() and (n == 9).any()
    _, n = bc.expected("n_even_odd")
    assert (n == 6).any() and (n == 5).any()
    _, n = bc.expected("margin_past_frame")
    assert np.all(n == 3)
    _, n = bc.expected("min_valid_6_n5_t8")
    assert (n == 5).any() and (n == 8).any()
    a, b = bc.expected("min_valid_5_n5_t8")[0], bc.expected("min_valid_6_n5_t8")[0]
    assert not np.array_equal(a, b)                                              # n + 1 turns the region into fallback pixels
    assert np.array_equal(bc.expected("min_valid_6_n5_t8")[0], bc.expected("min_valid_8_n5_t8")[0])


F = [np.zeros((4, 6, 3), np.uint8) for _ in range(3)]
NOBOX = [np.zeros((0, 4), np.int64)] * 3


@pytest.mark.parametrize("kwargs, match", [
    (dict(frames=[f.astype(np.int8) for f in F]), "uint8"),
    (dict(frames=[np.zeros((4, 6, 4), np.uint8)] * 3), "uint8 \\[H, W, 3\\]"),
    (dict(frames=[F[0], F[1], np.zeros((4, 7, 3), np.uint8)]), "frame 2 is"),
    (dict(frames=[F[0], np.zeros((4, 12, 3), np.uint8)[:, ::2]]), "not contiguous"),
    (dict(frames=np.zeros((3, 4, 12, 3), np.uint8)[:, :, ::2]), "not contiguous"),
    (dict(frames=[]), "0 frames"),
    (dict(frames=[F[0]] * 65), "65 frames"),
    (dict(frames=np.zeros((4, 6, 3), np.uint8)), "stack"),
    (dict(frames=F, boxes=NOBOX[:2]), "2 box lists for 3 frames"),
    (dict(frames=F, boxes=[np.zeros((65, 4), np.int64)] + NOBOX[:2]), "65 boxes"),
    (dict(frames=F, boxes=[np.zeros((2, 4), np.float32)] + NOBOX[:2]), "integer"),
    (dict(frames=F, boxes=[np.zeros((2, 3), np.int64)] + NOBOX[:2]), "integer \\[n, 4\\]"),
    (dict(frames=F, boxes=[np.asarray([[0, 0, 2 ** 31, 1]])] + NOBOX[:2]), "int32"),
    (dict(frames=F, margin=-1), "margin"),
    (dict(frames=F, margin=32768), "margin"),
    (dict(frames=F, min_valid=0), "min_valid"),
    (dict(frames=F, min_valid=4), "min_valid"),
])
def test_validation_raises_before_anything_runs(lib, monkeypatch, kwargs, match):
    def no_call(*a):
        raise AssertionError("the library was called")
    monkeypatch.setattr(ops.L, "lib", lambda: type("NoLib", (), {"fusg_background_median_host": no_call, "fusg_background_median_u8": no_call})())
    with pytest.raises(ValueError, match=match):
        ops.background_median_host(**kwargs)
    # the device entry point shares the checks: the same arguments as CPU tensors fail the same way, before the device is asked for
    tk = dict(kwargs)
    fr = tk["frames"]
    tk["frames"] = [torch.from_numpy(f) for f in fr] if isinstance(fr, list) else torch.from_numpy(fr)
    with pytest.raises(ValueError, match=match):
        ops.background_median(**tk)


def test_size_limits_are_refused_by_wrapper_and_library(lib):
    for shape in ((1, 32768, 3), (32768, 1, 3)):
        with pytest.raises(ValueError, match="1..32767"):
            ops.background_median_host([np.zeros(shape, np.uint8)])
    buf, out_bg, out_count = np.zeros(64, np.uint8), np.zeros(12, np.uint8), np.zeros(4, np.uint8)
    ptrs = (C.c_void_p * 64)(*[buf.ctypes.data] * 64)
    offs = (C.c_int32 * 65)()

    def call(T=2, H=2, W=2, boxes=None, box_offs=offs, margin=0, mv=1, frames=ptrs, bg=out_bg.ctypes.data, count=out_count.ctypes.data):
        return lib.fusg_background_median_host(frames, T, H, W, boxes, box_offs, margin, mv, bg, count)
    assert call() == 0
    for bad in (dict(T=0), dict(T=65), dict(H=0), dict(W=32768), dict(H=32768), dict(margin=-1), dict(margin=32768), dict(mv=0), dict(mv=3),
                dict(frames=None), dict(bg=None), dict(count=None), dict(frames=(C.c_void_p * 2)(buf.ctypes.data, None))):
        assert call(**bad) == -1, bad
        assert lib.fusg_last_error()
    for table, why in (((1, 1, 1), "start"), ((0, 2, 1), "decrease"), ((0, 65, 65), "65 boxes"), ((0, 1, 2), "null box table")):
        assert call(box_offs=(C.c_int32 * 3)(*table)) == -1, why
    # the device entry point checks the same tables on the host, before any launch: nothing here is a device pointer
    assert lib.fusg_background_median_u8(ptrs, 0, 2, 2, None, offs, 0, 1, buf.ctypes.data, buf.ctypes.data, None) == -1
    assert lib.fusg_background_median_u8(ptrs, 2, 2, 2, None, (C.c_int32 * 3)(0, 65, 65), 0, 1, buf.ctypes.data, buf.ctypes.data, None) == -1
    assert lib.fusg_background_median_u8(ptrs, 2, 2, 2, None, offs, 0, 3, buf.ctypes.data, buf.ctypes.data, None) == -1


@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_estimate_background_samples_the_scenes_by_the_index_rule(monkeypatch, n):
    seen = {}

    def stub(frames, boxes=None, margin=0, min_valid=1, out=None):
        seen.update(frames=list(frames), boxes=boxes, margin=margin, min_valid=min_valid)
        return "bg", "count"
    monkeypatch.setattr(ops, "background_median", stub)
    scenes = [{"frame": i, "bboxes": np.full((i % 3, 4), i, dtype=np.int64)} for i in range(n)]
    pipe = object.__new__(pl.VehiclePipeline)
    out = pipe.estimate_background(scenes)
    want = list(range(n)) if n <= 64 else [(i * n) // 64 for i in range(64)]
    assert out["frames"] == want and seen["frames"] == want and out["background"] == "bg" and out["count"] == "count"
    assert len(set(want)) == len(want) and want[0] == 0 and want[-1] < n
    assert seen["margin"] == 8 and seen["min_valid"] == max(1, len(want) // 8) == out["min_valid"]
    assert all(b.shape == (i % 3, 4) and np.all(b == i) for i, b in zip(want, seen["boxes"]))
    # fewer frames on request, an explicit min_valid
    out = pipe.estimate_background(scenes, max_frames=5, margin=2, min_valid=1)
    want = list(range(n)) if n <= 5 else [(i * n) // 5 for i in range(5)]
    assert out["frames"] == want and seen["margin"] == 2 and seen["min_valid"] == 1
    with pytest.raises(ValueError):
        pipe.estimate_background(scenes, max_frames=65)
    with pytest.raises(ValueError):
        pipe.estimate_background([])
