"""CPU: the batched later-frame pass (VehiclePipeline.run_later_frames_batched) without a device - its two exports are declared,
bound and built; their host-side validation refuses bad arguments before any launch; the frame-major row / seed / slice
bookkeeping and the max_batch grouping rule are pure Python."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import pipeline as pl

NEW = ("fusg_paste_layers_frames_u8", "fusg_warp_perspective_frames_u8")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def _u8(a: np.ndarray) -> L.Tensor:
    """fusg_tensor of a host uint8 [n, h, w, c] array: logical NCHW extents, HWC strides (never dereferenced here)."""
    d = L.Tensor()
    d.data = a.ctypes.data
    d.n, d.h, d.w, d.c = a.shape
    d.sn, d.sh, d.sw, d.sc = (s // a.itemsize for s in a.strides)
    d.dtype = L.U8
    return d


def test_the_new_exports_are_declared_bound_and_built(lib):
    hdr = open(os.path.join(REPO, "include", "fusg.h")).read()
    declared = set(re.findall(r"\b(fusg_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.fusg_version() == 118
    # the symbols that were there keep their argument lists
    assert len(L._SIGS["fusg_warp_perspective_indexed_u8"][1]) == 6 and len(L._SIGS["fusg_paste_layers_u8"][1]) == 7


def test_paste_frames_validation_without_a_device(lib):
    F, V, H, W, R = 2, 3, 8, 16, 4
    net = np.zeros((F * V, R, R, 3), np.uint8)
    masks = np.zeros((F * V, H, W, 1), np.uint8)
    dst = np.zeros((F, H, W, 3), np.uint8)
    geom = np.zeros((F * V, 8), np.int32)
    bases = np.zeros(F, np.int64)
    nt, mk, ds = _u8(net), _u8(masks), _u8(dst)
    g, b = geom.ctypes.data, bases.ctypes.data
    call = lib.fusg_paste_layers_frames_u8

    def refused(*a, word):
        assert call(*a, None) == -1, word
        assert word.encode() in lib.fusg_last_error(), (word, lib.fusg_last_error())

    refused(C.byref(nt), C.byref(mk), g, None, None, b, 0, C.byref(ds), word="frames")            # F = 0
    refused(C.byref(nt), C.byref(mk), g, None, None, b, -1, C.byref(ds), word="frames")
    refused(C.byref(nt), C.byref(mk), None, None, None, b, F, C.byref(ds), word="null")           # null tables
    refused(C.byref(nt), C.byref(mk), g, None, None, None, F, C.byref(ds), word="null")
    refused(C.byref(_u8(net[:5])), C.byref(_u8(masks[:5])), g, None, None, b, F, C.byref(ds), word="5 crops")   # 5 rows, 2 frames
    refused(C.byref(nt), C.byref(_u8(masks[:4])), g, None, None, b, F, C.byref(ds), word="4 masks")   # masks != crops
    refused(C.byref(nt), C.byref(mk), g, None, None, b, 3, C.byref(ds), word="shapes")            # dst holds 2 frames, not 3
    refused(C.byref(nt), C.byref(mk), g, C.byref(nt), None, b, F, C.byref(ds), word="rectangles")  # boxes without their rows
    refused(C.byref(nt), C.byref(mk), g, C.byref(_u8(net[:3])), g, b, F, C.byref(ds), word="rectangles")
    refused(None, C.byref(mk), g, None, None, b, F, C.byref(ds), word="shapes")


def test_warp_frames_validation_without_a_device(lib):
    S, F, H, W = 5, 3, 8, 16
    src = np.zeros((S, H, W, 3), np.uint8)
    dst = np.zeros((F * S, H, W, 3), np.uint8)
    minv = np.zeros((F * S, 9), np.float64)
    index = np.zeros((F * S, 2), np.int32)
    s, d, m, i = _u8(src), _u8(dst), minv.ctypes.data, index.ctypes.data
    call = lib.fusg_warp_perspective_frames_u8
    assert call(C.byref(s), m, None, F * S, F, C.byref(d), None) == -1 and b"null" in lib.fusg_last_error()
    assert call(C.byref(s), None, i, F * S, F, C.byref(d), None) == -1 and b"null" in lib.fusg_last_error()
    assert call(C.byref(s), m, i, F * S, 0, C.byref(d), None) == -1 and b"frames" in lib.fusg_last_error()
    assert call(C.byref(s), m, i, F * S, 2, C.byref(d), None) == -1            # dst holds 3 * S images, not 2 * S
    assert call(C.byref(s), m, i, F * S + 1, F, C.byref(d), None) == -1        # more jobs than destination images
    assert call(C.byref(s), m, i, -1, F, C.byref(d), None) == -1
    assert call(C.byref(s), m, i, 0, F, C.byref(d), None) == 0                 # nothing to warp: no launch


CASES = [(5, 8, None), (5, 8, 8), (5, 8, 20), (3, 1, 2), (1, 3, 1)]
WANT = {(5, 8, None): [(0, 5)], (5, 8, 8): [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], (5, 8, 20): [(0, 2), (2, 4), (4, 5)],
        (3, 1, 2): [(0, 2), (2, 3)], (1, 3, 1): [(0, 1)]}


@pytest.mark.parametrize("F,V,max_batch", CASES)
def test_grouping_rule(F, V, max_batch):
    """Consecutive groups of max(1, max_batch // V) frames: every frame exactly once, in order, at most max_batch rows per
    pass unless a single frame already has more (max_batch < V: one frame per pass)."""
    groups = pl.later_batch_groups(F, V, max_batch)
    assert groups == WANT[(F, V, max_batch)]
    assert [f for lo, hi in groups for f in range(lo, hi)] == list(range(F))
    cap = pl.LATER_MAX_BATCH if max_batch is None else max_batch
    per = max(1, cap // V)
    assert all(hi - lo == per for lo, hi in groups[:-1]) and 1 <= groups[-1][1] - groups[-1][0] <= per
    assert all((hi - lo) * V <= cap or hi - lo == 1 for lo, hi in groups)


def test_grouping_edges():
    assert pl.LATER_MAX_BATCH == 64
    assert pl.later_batch_groups(0, 8) == [] and pl.later_batch_groups(0, 0) == []
    assert pl.later_batch_groups(4, 0) == [(0, 4)]                             # no vehicles: nothing to bound
    assert pl.later_batch_groups(5, 64) == [(f, f + 1) for f in range(5)]      # a frame of 64 vehicles fills a pass
    assert pl.later_batch_groups(5, 65) == [(f, f + 1) for f in range(5)]
    with pytest.raises(ValueError):
        pl.later_batch_groups(3, 2, 0)


@pytest.mark.parametrize("F,V,max_batch", CASES)
def test_rows_slices_and_seeds_are_frame_major(F, V, max_batch):
    rows = [[pl.later_batch_row(f, v, V) for v in range(V)] for f in range(F)]
    assert [r for fr in rows for r in fr] == list(range(F * V))                # a bijection onto the rows, frame by frame
    for f in range(F):
        assert list(range(F * V))[pl.later_batch_slice(f, V)] == rows[f]
    per_frame = [[1000 * f + v for v in range(V)] for f in range(F)]
    seeds = pl.later_batch_seeds(per_frame, V)
    assert len(seeds) == F * V and all(seeds[pl.later_batch_row(f, v, V)] == 1000 * f + v for f in range(F) for v in range(V))
    # the rows of a group, renumbered from the group's first frame, carry that group's seeds
    for lo, hi in pl.later_batch_groups(F, V, max_batch):
        assert pl.later_batch_seeds(per_frame[lo:hi], V) == seeds[lo * V:hi * V]


def test_seed_presence_is_all_or_none():
    assert pl.later_batch_seeds([None, None], 2) is None and pl.later_batch_seeds([], 2) is None
    with pytest.raises(ValueError, match="vehicle_seeds"):
        pl.later_batch_seeds([[1, 2], None], 2)
    with pytest.raises(ValueError, match="vehicle_seeds"):
        pl.later_batch_seeds([[1, 2], [3]], 2)


def test_public_interface():
    sig = inspect.signature(pl.VehiclePipeline.run_later_frames_batched)
    assert list(sig.parameters) == ["self", "scenes", "state", "replay", "check", "max_batch"]
    assert sig.parameters["replay"].default is False and sig.parameters["check"].default == "sync" and sig.parameters["max_batch"].default is None
    clip = inspect.signature(pl.VehiclePipeline.run_clip_frames)
    assert clip.parameters["batched"].default is False and list(clip.parameters)[:4] == ["self", "first_scene", "later_scenes", "replay"]


def test_one_group_runner():
    """A group of later frames has ONE runner: the one-clip bodies are gone, and `_run_later_clips` takes the plan key its caller
    records under (the one-clip drivers': ("later_batch", F, V), the several-clip default: ("later_rows", B))."""
    for name in ("_run_later_batch", "_later_batch_stages", "_later_batch_local", "_later_batch_finish", "_later_geometry_stage",
                 "_run_later_geometry_batch"):
        assert not hasattr(pl.VehiclePipeline, name), name
    sig = inspect.signature(pl.VehiclePipeline._run_later_clips)
    assert list(sig.parameters) == ["self", "clips", "replay", "rows", "geometry", "plan_key"] and sig.parameters["plan_key"].default is None
    src = inspect.getsource(pl.VehiclePipeline._later_one_clip_groups)
    assert '"later_batch"' in src and "_run_later_clips" in src and '"later_rows"' in inspect.getsource(pl.VehiclePipeline._run_later_clips)
