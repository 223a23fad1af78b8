"""CPU: the later-frame gate (fusg_later_gate / fusg_later_gate_host, csrc/pose_geometry.h) without a device - both exports are
declared, bound and built; the host twin equals `render.visible(counts)[:, :P] & (covered > 0)` on counts constructed around
the comparison's rounding ties; box rows are zeroed exactly on the invalid rows; bad arguments are refused before any launch;
and the batched geometry-mode driver refuses what it cannot batch before it issues anything."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import pipeline as pl
from future_urban_scene_generation_amd import render as R

NEW = ("fusg_later_gate", "fusg_later_gate_host")


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
    assert len(L._SIGS["fusg_later_gate"][1]) == 8 and len(L._SIGS["fusg_later_gate_host"][1]) == 7
    # the stages it sits behind keep their argument lists
    assert len(L._SIGS["fusg_plane_visibility"][1]) == 8 and len(L._SIGS["fusg_plane_homographies"][1]) == 14


def gate_host(lib, counts, covered, P, box_rows=None):
    """fusg_later_gate_host on numpy arrays: (dst_vis uint8 [J, P], valid int32 [J], box_rows or None)."""
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    covered = np.ascontiguousarray(covered, dtype=np.int32)
    J = counts.shape[0]
    vis = np.full((J, P), 7, np.uint8)                                          # (every element is overwritten)
    valid = np.full(J, -3, np.int32)
    box = None if box_rows is None else np.ascontiguousarray(box_rows, dtype=np.int32).copy()
    rc = lib.fusg_later_gate_host(counts.ctypes.data, covered.ctypes.data, J, P, vis.ctypes.data, valid.ctypes.data,
                                  None if box is None else box.ctypes.data)
    assert rc == 0, lib.fusg_last_error()
    return vis, valid, box


def gate_cases(seed=5):
    """counts int32 [J, 7, 2] = (absolute, occluded) and covered int32 [J]: rows of seven planes each, built around the rule
    occluded > 0.9 * absolute - zeros; absolute a multiple of 10 with occluded = 9 * absolute / 10 - 1, + 0, + 1 (the tie
    10 * occ == 9 * abs, where 0.9 * abs may round either way); absolute up to a 720 x 1280 frame's 921 600 pixels and up to
    2^31 - 1; occluded > absolute; each row once with covered 0, 1 and a large count."""
    g = np.random.default_rng(seed)
    planes = [(0, 0), (0, 1), (1, 0), (1, 1)]
    tens = [10, 20, 30, 70, 100, 110, 1000, 4090, 921600, 921590, 2147483640, 1073741820] + \
        [int(10 * k) for k in g.integers(1, 92160, 40)] + [int(10 * k) for k in g.integers(92160, 214748364, 40)]
    for a in tens:
        for d in (-1, 0, 1):
            planes.append((a, 9 * (a // 10) + d))
    for a in [int(x) for x in g.integers(1, 921601, 60)] + [int(x) for x in g.integers(921601, 2 ** 31 - 1, 60)] + [2 ** 31 - 1]:
        planes.append((a, int(np.floor(0.9 * a))))
        planes.append((a, min(2 ** 31 - 1, int(np.floor(0.9 * a)) + 1)))
        planes.append((a, int(g.integers(0, a + 1))))
    planes += [(5, 9), (100, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 0)]              # occluded > absolute, extremes
    while len(planes) % 7:
        planes.append((0, 0))
    rows = np.asarray(planes, np.int64).reshape(-1, 7, 2)
    assert rows.min() >= 0 and rows.max() <= 2 ** 31 - 1
    counts = np.concatenate([rows, rows, rows]).astype(np.int32)
    covered = np.concatenate([np.zeros(len(rows)), np.ones(len(rows)), np.full(len(rows), 921600)]).astype(np.int32)
    return counts, covered


@pytest.mark.parametrize("P", [5, 7])
def test_host_twin_equals_render_visible(lib, P):
    counts, covered = gate_cases()
    want = R.visible(counts)[:, :P] & (covered > 0)[:, None]
    vis, valid, _ = gate_host(lib, counts, covered, P)
    assert np.array_equal(vis, want.astype(np.uint8))
    assert np.array_equal(valid, (covered > 0).astype(np.int32))
    # not vacuous: both outcomes, both kinds of row, and tie planes (10 * occ == 9 * abs) with their two neighbours
    live = covered > 0
    assert want[live].any() and (~want[live]).any() and not want[~live].any() and R.visible(counts)[~live].any()
    a, o = counts[..., 0].astype(np.int64), counts[..., 1].astype(np.int64)
    tie = ((10 * o == 9 * a) & (a > 0))[live][:, :P]
    above = (10 * (o - 1) == 9 * a)[live][:, :P]
    assert tie.any() and above.any()
    # (the double 0.9 lies above 9 / 10, so at a tie the product is the integer itself or the next double: not visible)
    assert not want[live][tie].any() and want[live][above].all()
    print(f"P={P}: {int(tie.sum())} tie planes, {int(want[live].sum())} of {want[live].size} live planes visible")
    assert (o > a)[live][:, :P].any() and (a == 2 ** 31 - 1).any() and (a == 921600).any()


def test_box_rows_are_zeroed_exactly_on_the_invalid_rows(lib):
    counts, covered = gate_cases()
    J = counts.shape[0]
    box = np.arange(1, J * 8 + 1, dtype=np.int32).reshape(J, 8)
    vis, valid, got = gate_host(lib, counts, covered, 5, box)
    want = np.where((covered > 0)[:, None], box, 0)
    assert np.array_equal(got, want) and (got[covered > 0] != 0).all() and (covered == 0).any()
    vis2, valid2, none = gate_host(lib, counts, covered, 5)                     # without box rows: the same visibilities
    assert none is None and np.array_equal(vis, vis2) and np.array_equal(valid, valid2)


def test_empty_and_bad_arguments(lib):
    c, v = np.zeros((2, 7, 2), np.int32), np.ones(2, np.int32)
    d, ok = np.zeros((2, 5), np.uint8), np.zeros(2, np.int32)
    cp, vp, dp, op = c.ctypes.data, v.ctypes.data, d.ctypes.data, ok.ctypes.data
    for call, tail in ((lib.fusg_later_gate, (None,)), (lib.fusg_later_gate_host, ())):
        assert call(cp, vp, 0, 5, dp, op, None, *tail) == 0                     # J = 0: nothing to do, no launch
        for args, word in (((None, vp, 2, 5, dp, op, None), b"null"), ((cp, None, 2, 5, dp, op, None), b"null"),
                           ((cp, vp, 2, 5, None, op, None), b"null"), ((cp, vp, 2, 5, dp, None, None), b"null"),
                           ((cp, vp, 2, 0, dp, op, None), b"P 0"), ((cp, vp, 2, 8, dp, op, None), b"P 8"),
                           ((cp, vp, -1, 5, dp, op, None), b"J -1")):
            assert call(*args, *tail) == -1, (call, args)                        # FUSG_ERR_INVALID before any launch
            assert word in lib.fusg_last_error(), (word, lib.fusg_last_error())
    assert lib.fusg_later_gate_host(cp, vp, 2, 7, np.zeros((2, 7), np.uint8).ctypes.data, op, None) == 0


# ------------------------------------------------------------------------------------------------ the driver's refusals
def _scene(V=3, **kw):
    return dict({"frame": None, "steps": [(0.0, np.zeros(3))] * V}, **kw)


def test_batching_needs_the_device_pose_and_device_homography_paths():
    scenes = [_scene(), _scene()]
    with pytest.raises(ValueError, match="device_pose=True and device_homography=True"):
        pl.later_geometry_batch_rows(scenes, [0, 2], False, True)
    with pytest.raises(ValueError, match="device_pose=True and device_homography=True"):
        pl.later_geometry_batch_rows(scenes, [0, 2], True, False)
    assert pl.later_geometry_batch_rows(scenes, [0, 2], True, True) == (None, False)


class _NoDevice:
    """Stands where a state's tensors would: any use before the refusal fails the test with an AttributeError."""


@pytest.mark.parametrize("flags", [dict(device_pose=False, device_homography=True), dict(device_pose=True, device_homography=False)])
def test_the_pipeline_refuses_before_any_launch(flags):
    """`batch_geometry=True` on a pipeline without one of the flags: ValueError from the public methods with nothing but the
    flags set - no network, no device, no state tensor is touched on the way there."""
    pipe = object.__new__(pl.VehiclePipeline)
    pipe.group, pipe.cad_bank, pipe.inpaint = None, object(), False
    pipe.device_pose, pipe.device_homography = flags["device_pose"], flags["device_homography"]
    state = {"geometry": {"vehicles": [0, 1, 2]}, "central": _NoDevice(), "appearance": _NoDevice()}
    with pytest.raises(ValueError, match="device_pose=True and device_homography=True"):
        pipe.run_later_frames_batched_geometry([_scene(), _scene()], state)
    first = {"state": state, "frame": None}
    pipe.run_frame = lambda scene, replay=False: first
    clip = pipe.run_clip_frames({}, [_scene(), _scene()], batched=True, batch_geometry=True)
    assert next(clip) is first
    with pytest.raises(ValueError, match="device_pose=True and device_homography=True"):
        next(clip)


def test_seed_and_inpaint_presence_is_all_or_none():
    veh = [0, 2]
    seeded = _scene(vehicle_seeds=[10, 11, 12])
    with pytest.raises(ValueError, match="vehicle_seeds"):
        pl.later_geometry_batch_rows([seeded, _scene()], veh, True, True)
    # per first-frame vehicle, selected to the state's vehicles, frame-major
    assert pl.later_geometry_batch_rows([seeded, _scene(vehicle_seeds=[20, 21, 22])], veh, True, True) == ([10, 12, 20, 22], False)
    with pytest.raises(ValueError, match="vehicle_seeds"):
        pl.later_geometry_batch_rows([_scene(vehicle_seeds=[10, 11])], veh, True, True)           # does not reach vehicle 2
    boxed = _scene(inpaint={"boxes": np.zeros((3, 4), np.int32), "det_masks": None})
    with pytest.raises(ValueError, match="'inpaint'"):
        pl.later_geometry_batch_rows([boxed, _scene()], veh, True, True, inpaint=True)
    assert pl.later_geometry_batch_rows([boxed, boxed], veh, True, True, inpaint=True) == (None, True)
    assert pl.later_geometry_batch_rows([boxed, _scene()], veh, True, True, inpaint=False) == (None, False)   # no networks: ignored
    with pytest.raises(ValueError, match="geometry-mode"):
        pl.later_geometry_batch_rows([_scene(masks=None)], veh, True, True)


def test_public_interface():
    sig = inspect.signature(pl.VehiclePipeline.run_later_frames_batched_geometry)
    assert list(sig.parameters) == ["self", "scenes", "state", "replay", "check", "max_batch", "batch_geometry"]
    assert sig.parameters["batch_geometry"].default is True and sig.parameters["max_batch"].default is None
    clip = inspect.signature(pl.VehiclePipeline.run_clip_frames)
    assert clip.parameters["batch_geometry"].default is False and clip.parameters["batched"].default is False
    assert list(inspect.signature(R.later_geometry_batch_device).parameters) == \
        ["bank", "frame_hw", "cad_idx_d", "pose_d", "K", "steps_per_frame", "box_rows"]
