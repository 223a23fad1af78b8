"""CPU: the batched first-frame pass (VehiclePipeline.run_frames_batched) without a device - its three exports are declared,
bound and built; their host-side validation refuses bad tables and row counts before any launch (the tables are host arrays, so
everything can be checked here with pointers that are never dereferenced); the scene-major grouping, offsets, padding and seed
bookkeeping are pure Python."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import pipeline as pl

NEW = ("fusg_crop_resize_frames_u8", "fusg_vunet_inputs_frames", "fusg_paste_layers_ragged_u8")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def _desc(a: np.ndarray, dtype) -> L.Tensor:
    """fusg_tensor of a host [n, h, w, c] array: logical NCHW extents, HWC strides (never dereferenced here)."""
    d = L.Tensor()
    d.data = a.ctypes.data
    d.n, d.h, d.w, d.c = a.shape
    d.sn, d.sh, d.sw, d.sc = (s // a.itemsize for s in a.strides)
    d.dtype = dtype
    return d


def _u8(a):
    return _desc(a, L.U8)


def _f32(a):
    return _desc(a, L.F32)


def _tab(ptrs, offs):
    return (C.c_void_p * len(ptrs))(*ptrs), (C.c_int32 * len(offs))(*offs)


def test_the_new_exports_are_declared_bound_and_built(lib):
    hdr = open(os.path.join(REPO, "include", "fusg.h")).read()
    declared = set(re.findall(r"\b(fusg_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.fusg_version() == 118
    assert int(re.search(r"#define FUSG_MAX_FRAMES (\d+)", hdr).group(1)) == 64 == L.MAX_FRAMES
    # the symbols that were there keep their argument lists
    assert len(L._SIGS["fusg_crop_resize_u8"][1]) == 7 and len(L._SIGS["fusg_vunet_inputs"][1]) == 8
    assert len(L._SIGS["fusg_paste_layers_frames_u8"][1]) == 9


# one refusal per rule of the tables, shared by the three entry points: (frame pointers, offsets, n_frames, word in the message)
H, W, R, ROWS = 8, 16, 4, 5
IMG = np.zeros((3, H, W, 3), np.uint8)
P = [IMG[f].ctypes.data for f in range(3)]
BAD_TABLES = [
    (P, [0, 2, 2, ROWS], 0, "n_frames"),
    (P * 22, [0] * 65 + [ROWS], 65, "n_frames"),
    ([P[0], None, P[2]], [0, 2, 2, ROWS], 3, "null pointer"),
    (P, [0, 3, 2, ROWS], 3, "decrease"),
    (P, [1, 2, 2, ROWS], 3, "start"),
    (P, [0, 2, 2, ROWS - 1], 3, "end"),
    (P, [0, 2, 2, ROWS + 1], 3, "end"),
]


def _refused(lib, rc, word):
    assert rc == -1, word
    assert word.encode() in lib.fusg_last_error(), (word, lib.fusg_last_error())


def test_crop_resize_frames_validation_without_a_device(lib):
    geom = np.zeros((ROWS, 8), np.int32)
    dst8 = np.zeros((ROWS, R, R, 3), np.uint8)
    dstf = np.zeros((ROWS, R, R, 4), np.float32)[..., :3]
    call = lib.fusg_crop_resize_frames_u8
    for ptrs, offs, n, word in BAD_TABLES:
        fr, ro = _tab(ptrs, offs)
        _refused(lib, call(fr, ro, n, H, W, geom.ctypes.data, C.byref(_u8(dst8)), 0, None, None, None), word)
    fr, ro = _tab(P, [0, 2, 2, ROWS])
    _refused(lib, call(None, ro, 3, H, W, geom.ctypes.data, C.byref(_u8(dst8)), 0, None, None, None), "null")
    _refused(lib, call(fr, None, 3, H, W, geom.ctypes.data, C.byref(_u8(dst8)), 0, None, None, None), "null")
    _refused(lib, call(fr, ro, 3, H, W, None, C.byref(_u8(dst8)), 0, None, None, None), "geom")
    _refused(lib, call(fr, ro, 3, H, W, geom.ctypes.data, C.byref(_u8(dst8[:4])), 0, None, None, None), "end")   # 4 rows, offsets to 5
    _refused(lib, call(fr, ro, 3, H, W, geom.ctypes.data, C.byref(_u8(dst8)), 3, None, None, None), "mode")
    _refused(lib, call(fr, ro, 3, H, W, geom.ctypes.data, C.byref(_u8(dst8)), 1, None, None, None), "modes 1")   # u8 dst for a float mode
    _refused(lib, call(fr, ro, 3, H, W, geom.ctypes.data, C.byref(_f32(dstf)), 1, None, None, None), "mean")
    _refused(lib, call(fr, ro, 3, 0, W, geom.ctypes.data, C.byref(_u8(dst8)), 0, None, None, None), "frames of")
    # rows = 0: nothing to cut, no launch
    fr0, ro0 = _tab(P, [0, 0, 0, 0])
    assert call(fr0, ro0, 3, H, W, None, C.byref(_u8(dst8[:0])), 0, None, None, None) == 0


def test_vunet_inputs_frames_validation_without_a_device(lib):
    geom = np.zeros((ROWS, 8), np.int32)
    masks = np.zeros((ROWS, H, W, 1), np.uint8)
    sk = np.zeros((ROWS, H, W, 3), np.uint8)
    x = np.zeros((ROWS, R, R, 8), np.float32)[..., :6]
    y = np.zeros((ROWS, R, R, 4), np.float32)[..., :3]
    call = lib.fusg_vunet_inputs_frames

    def go(fr, ro, n, m=masks, s1=sk, s2=sk, g=geom.ctypes.data, xx=x, yy=y):
        return call(fr, ro, n, C.byref(_u8(m)), C.byref(_u8(s1)), C.byref(_u8(s2)), g, C.byref(_f32(xx)), C.byref(_f32(yy)), None)

    for ptrs, offs, n, word in BAD_TABLES:
        _refused(lib, go(*_tab(ptrs, offs), n), word)
    fr, ro = _tab(P, [0, 2, 2, ROWS])
    _refused(lib, go(fr, ro, 3, s1=sk[:4]), "row counts differ")
    _refused(lib, go(fr, ro, 3, s2=sk[:4]), "row counts differ")
    _refused(lib, go(fr, ro, 3, xx=x[:4]), "row counts differ")
    _refused(lib, go(fr, ro, 3, yy=y[:3]), "row counts differ")
    _refused(lib, go(fr, ro, 3, m=masks[:4]), "end")                              # the offsets end at 5, the masks hold 4
    _refused(lib, go(fr, ro, 3, g=None), "geom")
    _refused(lib, go(fr, ro, 3, s1=np.zeros((ROWS, H, W + 1, 3), np.uint8)), "sketches")
    fr0, ro0 = _tab(P, [0, 0, 0, 0])
    assert go(fr0, ro0, 3, m=masks[:0], s1=sk[:0], s2=sk[:0], xx=x[:0], yy=y[:0], g=None) == 0    # rows = 0: no launch


def test_paste_ragged_validation_without_a_device(lib):
    net = np.zeros((ROWS, R, R, 3), np.uint8)
    masks = np.zeros((ROWS, H, W, 1), np.uint8)
    dst = np.zeros((3, H, W, 3), np.uint8)
    geom = np.zeros((ROWS, 8), np.int32)
    g = geom.ctypes.data
    call = lib.fusg_paste_layers_ragged_u8

    def go(fr, ro, n, nt=net, mk=masks, gg=g, rect=None, rg=None, ds=dst):
        return call(C.byref(_u8(nt)), C.byref(_u8(mk)), gg, None if rect is None else C.byref(_u8(rect)), rg, fr, ro, n, C.byref(_u8(ds)), None)

    for ptrs, offs, n, word in BAD_TABLES:
        _refused(lib, go(*_tab(ptrs, offs), n), word)
    fr, ro = _tab(P, [0, 2, 2, ROWS])
    _refused(lib, go(None, ro, 3), "null")
    _refused(lib, go(fr, ro, 3, mk=masks[:4]), "row counts differ")
    _refused(lib, go(fr, ro, 3, rect=net), "rectangles")                          # box images without their rows
    _refused(lib, go(fr, ro, 3, rg=g), "rectangles")                              # ... and rows without images
    _refused(lib, go(fr, ro, 3, rect=net[:3], rg=g), "rectangles")
    _refused(lib, go(fr, ro, 3, gg=None), "geom")
    _refused(lib, go(fr, ro, 3, ds=dst[:2]), "dst")                               # dst holds 2 frames, the table 3
    _refused(lib, go(fr, ro, 3, mk=np.zeros((ROWS, H + 1, W, 1), np.uint8)), "shapes")
    inplace, ro1 = _tab([dst[1].ctypes.data, P[1], P[2]], [0, 2, 2, ROWS])
    _refused(lib, go(inplace, ro1, 3), "overlaps")                                # a base inside dst: the bases are read only


EXAMPLE = ([2, 0, 3, 8, 1], 8, [(0, 3), (3, 4), (4, 5)])
GROUPS = [EXAMPLE,
          ([0, 0, 0], 4, [(0, 3)]),                                               # no vehicles anywhere: one group
          ([0, 4, 0, 0, 4, 0], 4, [(0, 4), (4, 6)]),                              # zeros ride with whatever group is open
          ([9, 1, 1], 4, [(0, 1), (1, 3)]),                                       # a scene larger than max_batch: a group of its own
          ([1, 9, 1], 4, [(0, 1), (1, 2), (2, 3)]),
          ([3, 3, 3], None, [(0, 3)]),
          ([64, 1], None, [(0, 1), (1, 2)]),
          ([], 4, [])]


@pytest.mark.parametrize("counts,max_batch,want", GROUPS)
def test_grouping_rule(counts, max_batch, want):
    groups = pl.frame_batch_groups(counts, max_batch)
    assert groups == want
    assert [f for lo, hi in groups for f in range(lo, hi)] == list(range(len(counts)))       # every scene once, in order
    cap = pl.LATER_MAX_BATCH if max_batch is None else max_batch
    assert all(sum(counts[lo:hi]) <= cap or hi - lo == 1 or sum(1 for c in counts[lo:hi] if c) == 1 for lo, hi in groups)
    for (lo, hi), nxt in zip(groups, groups[1:]):                                  # greedy: the next scene did not fit
        assert sum(counts[lo:hi]) + counts[nxt[0]] > cap


def test_grouping_edges():
    assert pl.FRAME_BATCH_MAX_FRAMES == 64 == L.MAX_FRAMES
    assert pl.frame_batch_groups([1] * 7, 64, max_frames=3) == [(0, 3), (3, 6), (6, 7)]      # the max_frames cut
    assert pl.frame_batch_groups([0] * 130) == [(0, 64), (64, 128), (128, 130)]            # ... which also bounds empty scenes
    assert pl.frame_batch_groups([2] * 40) == [(0, 32), (32, 40)]                          # the default max_batch: 64 rows
    for bad in (0, -1):
        with pytest.raises(ValueError, match="max_batch"):
            pl.frame_batch_groups([1, 2], bad)
    with pytest.raises(ValueError, match="max_frames"):
        pl.frame_batch_groups([1, 2], 4, max_frames=0)


def test_offsets_are_scene_major():
    assert pl.frame_batch_offsets([2, 0, 3]) == [0, 2, 2, 5]
    assert pl.frame_batch_offsets([]) == [0] and pl.frame_batch_offsets([0]) == [0, 0]
    counts = EXAMPLE[0]
    for lo, hi in pl.frame_batch_groups(counts, 8):                                # a group's offsets restart at 0
        offs = pl.frame_batch_offsets(counts[lo:hi])
        assert offs[0] == 0 and offs[-1] == sum(counts[lo:hi]) and len(offs) == hi - lo + 1
        assert all(b - a == c for a, b, c in zip(offs, offs[1:], counts[lo:hi]))


def test_padding_rule():
    for (rows, cap), want in {(3, 64): 4, (5, 64): 8, (33, 48): 48, (70, 64): 70, (0, 64): 0}.items():
        assert pl.frame_batch_pad(rows, cap) == want, (rows, cap)
    assert pl.frame_batch_pad(0) == 0 and pl.frame_batch_pad(1) == 4 and pl.frame_batch_pad(4) == 4 and pl.frame_batch_pad(64) == 64
    # the default max_batch: five shapes, whatever the count
    assert sorted({pl.frame_batch_pad(r) for r in range(1, 65)}) == [4, 8, 16, 32, 64]
    assert all(pl.frame_batch_pad(r, 48) >= r for r in range(0, 100))


def test_seed_presence_is_all_or_none():
    assert pl.frame_batch_seeds([None, None], [2, 1]) is None and pl.frame_batch_seeds([], []) is None
    assert pl.frame_batch_seeds([[1, 2], None, [3, 4, 5]], [2, 0, 3]) == [1, 2, 3, 4, 5]      # an empty scene decides nothing
    assert pl.frame_batch_seeds([[1, 2], [], [3]], [2, 0, 1]) == [1, 2, 3]
    assert pl.frame_batch_seeds([None, None], [0, 0]) is None
    with pytest.raises(ValueError, match="vehicle_seeds"):
        pl.frame_batch_seeds([[1, 2], None], [2, 1])
    with pytest.raises(ValueError, match="vehicle_seeds"):
        pl.frame_batch_seeds([[1, 2], [3]], [2, 2])
    with pytest.raises(ValueError, match="vehicle_seeds"):
        pl.frame_batch_seeds([[1, 2, 3], [4]], [2, 1])


def test_public_interface():
    sig = inspect.signature(pl.VehiclePipeline.run_frames_batched)
    assert list(sig.parameters) == ["self", "scenes", "replay", "check", "max_batch", "pad"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["replay"] is False and d["check"] == "sync" and d["max_batch"] is None and d["pad"] is None
    # the drivers it stands beside keep their parameter lists
    assert list(inspect.signature(pl.VehiclePipeline.run_frame).parameters) == ["self", "scene", "check", "replay"]
    assert list(inspect.signature(pl.VehiclePipeline.run_frames).parameters) == ["self", "scenes", "replay"]
