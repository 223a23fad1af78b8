"""GPU: fusg_inpaint_inputs against its host twin (the same csrc/inpaint_inputs.h code on the CPU, pinned to the numpy
restatement by tests/test_inpaint_inputs_cpu.py), byte for byte, and the frame driver fed a detector mask against the
frame driver fed the four tensors the op builds from it."""
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

import inpaint_ref as ir                                                   # noqa: E402
from conftest import synth_sd                                              # noqa: E402
from future_urban_scene_generation_amd import ops                          # noqa: E402

DEV = "cuda:0"


def _device(fx, order=None):
    order = list(range(len(fx["boxes"]))) if order is None else order
    out = ops.inpaint_inputs(torch.from_numpy(fx["frame"]).to(DEV), torch.from_numpy(np.ascontiguousarray(fx["det_masks"][order])).to(DEV),
                             fx["boxes"][order])
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("which", [0, 1], ids=["96x160", "300x420"])
def test_device_equals_host_twin(which):
    """V = 6 in one call: byte-equal to the host twin, to a second call, and - permuted - to a call with the vehicles permuted."""
    fx = ir.fixtures()[which]
    host = ops.inpaint_inputs_host(fx["frame"], fx["det_masks"], fx["boxes"])
    got, again = _device(fx), _device(fx)
    order = [3, 0, 5, 1, 4, 2]
    perm = _device(fx, order)
    for k in ops.INPAINT_KEYS:
        for v in range(6):
            assert got[k][v].tobytes() == host[k][v].tobytes(), (fx["name"], k, v, int((got[k][v] != host[k][v]).sum()))
        assert again[k].tobytes() == got[k].tobytes(), k
        assert perm[k].tobytes() == got[k][order].tobytes(), k


def test_device_boxes_and_strided_outputs():
    """Boxes already on the device (the frame bounds the scratch) and outputs written into channel slices of a wider buffer."""
    fx = ir.fixtures()[0]
    host = ops.inpaint_inputs_host(fx["frame"], fx["det_masks"], fx["boxes"])
    buf = torch.full((6, 6, 256, 256), 7.0, device=DEV)
    out = {"img": buf[:, 0:3], "gray": buf[:, 3:4], "edge": buf[:, 4:5], "mask": buf[:, 5:6]}
    ops.inpaint_inputs(torch.from_numpy(fx["frame"]).to(DEV), torch.from_numpy(fx["det_masks"]).to(DEV),
                       torch.from_numpy(fx["boxes"].astype(np.int32)).to(DEV), out=out)
    for k in ops.INPAINT_KEYS:
        assert out[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    bad = fx["boxes"].astype(np.int32).copy()
    bad[0] = (150, 0, 170, 20)                                             # leaves the frame: a device box nobody checked has no pixels
    got = ops.inpaint_inputs(torch.from_numpy(fx["frame"]).to(DEV), torch.from_numpy(fx["det_masks"]).to(DEV), torch.from_numpy(bad).to(DEV))
    assert not got["img"][0].any() and not got["edge"][0].any() and got["gray"][1:].cpu().numpy().tobytes() == host["gray"][1:].tobytes()
    empty = ops.inpaint_inputs(torch.from_numpy(fx["frame"]).to(DEV), torch.from_numpy(fx["det_masks"][:0]).to(DEV), fx["boxes"][:0])
    assert empty["img"].shape == (0, 3, 256, 256)


def test_run_frame_from_detector_masks():
    """run_frame fed {'boxes', 'det_masks'} = run_frame fed the four tensors ops.inpaint_inputs builds from them, bit for bit:
    eager, replayed and through run_frames; and a frame without vehicles goes through."""
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline, synth_frame
    ops.set_precision("f16x3")
    sds = {n: synth_sd(n) for n in ("hg", "icn", "vunet", "edge", "inpaint")}
    pipe = VehiclePipeline(DEV, inpaint=True, state_dicts=sds)
    sc = synth_frame(2, (360, 640), DEV, seed=17, inpaint="masks")
    sc["vehicle_seeds"] = [40, 41]
    assert set(sc["inpaint"]) == {"boxes", "det_masks"} and sc["inpaint"]["det_masks"].shape == (2, 1, 360, 640)
    built = ops.inpaint_inputs(sc["frame"], sc["inpaint"]["det_masks"], sc["inpaint"]["boxes"])
    assert 0 < float(built["mask"].mean()) < 1 and float(built["edge"].sum()) > 0
    given = dict(sc, inpaint=dict(built, boxes=sc["inpaint"]["boxes"]))
    want = pipe.run_frame(given)
    keys = ("inpaint_u8", "frame_icn", "frame_vunet", "kp_idx", "icn_u8", "vunet_u8")
    runs = {"eager": pipe.run_frame(sc), "replay": pipe.run_frame(sc, replay=True), "replay again": pipe.run_frame(sc, replay=True)}
    seq = list(pipe.run_frames([sc, sc]))
    runs.update({"run_frames 0": seq[0], "run_frames 1": seq[1]})
    for name, got in runs.items():
        for k in keys:
            assert torch.equal(got[k], want[k]), (name, k)
    with pytest.raises(ValueError, match="det_masks"):
        pipe.run_frame(dict(sc, inpaint=dict(given["inpaint"], det_masks=sc["inpaint"]["det_masks"])))
    H, W = 360, 640
    e = lambda *sh: torch.empty(sh, dtype=torch.uint8, device=DEV)           # noqa: E731
    none = {"frame": sc["frame"], "bboxes": np.zeros((0, 4), np.int64), "masks": e(0, H, W), "src_sketch": e(0, H, W, 3),
            "dst_sketch": e(0, H, W, 3), "src_planes": e(0, 5, H, W, 3), "src_kp": [], "dst_kp": [], "src_vis": np.zeros((0, 5), np.uint8),
            "dst_vis": np.zeros((0, 5), np.uint8), "kp3d": np.zeros((0, 12, 3), np.float32), "focals": sc["focals"], "centers": sc["centers"],
            "inpaint": {"boxes": np.zeros((0, 4), np.int64), "det_masks": e(0, 1, H, W)}}
    for o in (pipe.run_frame(none), pipe.run_frame(none, replay=True)):
        assert o["inpaint_u8"].shape == (0, 256, 256, 3) and torch.equal(o["frame_icn"], sc["frame"])
