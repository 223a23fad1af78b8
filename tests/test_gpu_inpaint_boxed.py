"""GPU: fusg_inpaint_inputs_boxed against its host twin (pinned to the frame form by tests/test_inpaint_boxed_cpu.py), bit
for bit: uint8 and float32 masks, from a packed pair and from host pieces; the device-side bounds guard; strided outputs."""
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

from test_inpaint_boxed_cpu import BOXES, boxed_case                       # noqa: E402
from future_urban_scene_generation_amd import ops                          # noqa: E402

DEV = "cuda:0"


def _pack(pieces):
    offs = np.zeros(len(pieces), np.int64)
    offs[1:] = np.cumsum([p.size for p in pieces])[:-1]
    return np.concatenate([p.reshape(-1) for p in pieces]), offs


@pytest.fixture(scope="module")
def case():
    """The CPU test's frame and pieces, a float32 version with a NaN, a negative and a denormal entry, and both host results."""
    frame, pieces, _ = boxed_case()
    g = np.random.default_rng(5)
    fl = []
    for p in pieces:
        m = np.where(p > 0, g.choice(np.array([1.0, 0.5, 1e-30, -0.25], dtype=np.float32), size=p.shape), 0).astype(np.float32)
        if m.size:
            m.flat[0], m.flat[m.size // 2], m.flat[-1] = np.nan, -1.0, np.float32(1e-40)
        fl.append(m)
    host = {"u8": ops.inpaint_inputs_boxed_host(frame, pieces, BOXES), "f32": ops.inpaint_inputs_boxed_host(frame, fl, BOXES)}
    assert 0 < host["u8"]["mask"][:3].mean() < 1 and 0 < host["f32"]["mask"][:3].mean() < 1
    return dict(frame=frame, frame_d=torch.from_numpy(frame).to(DEV), u8=pieces, f32=fl, host=host)


def _same(got, host, what):
    for k in ops.INPAINT_KEYS:
        a = got[k].cpu().numpy()
        assert a.tobytes() == host[k].tobytes(), (what, k, int((a != host[k]).sum()))


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_device_equals_host_twin(case, kind):
    """From a packed (buffer, offsets) pair with device and with host offsets, from host pieces (one pinned upload), from
    device pieces (one cat) and from [1, h, w] pieces; with host boxes and with device boxes."""
    pieces, host = case[kind], case["host"][kind]
    buf, offs = _pack(pieces)
    buf_d = torch.from_numpy(buf).to(DEV)
    boxes_d = torch.from_numpy(BOXES.astype(np.int32)).to(DEV)
    _same(ops.inpaint_inputs_boxed(case["frame_d"], (buf_d, torch.from_numpy(offs).to(DEV)), BOXES), host, "pair, device offsets")
    _same(ops.inpaint_inputs_boxed(case["frame_d"], (buf_d, offs), boxes_d), host, "pair, host offsets, device boxes")
    _same(ops.inpaint_inputs_boxed(case["frame_d"], pieces, BOXES), host, "host pieces")
    _same(ops.inpaint_inputs_boxed(case["frame_d"], [torch.from_numpy(p) for p in pieces], BOXES), host, "host tensors")
    _same(ops.inpaint_inputs_boxed(case["frame_d"], [torch.from_numpy(p)[None].to(DEV) for p in pieces], boxes_d), host, "device pieces")


def test_a_mask_past_the_buffer_is_a_zero_extent_box(case):
    """The guard's result, with device boxes and offsets (the host cannot look): a vehicle whose mask would end past n_elems,
    or start before 0, writes zeros to all four outputs and the others are right; nothing outside the buffer is read."""
    pieces, host = case["u8"], case["host"]["u8"]
    buf, offs = _pack(pieces)
    buf_d = torch.from_numpy(buf).to(DEV)
    boxes_d = torch.from_numpy(BOXES.astype(np.int32)).to(DEV)
    for v, off in ((1, buf.size - pieces[1].size + 1), (2, -1), (0, 1 << 40)):
        bad = offs.copy()
        bad[v] = off
        got = ops.inpaint_inputs_boxed(case["frame_d"], (buf_d, torch.from_numpy(bad).to(DEV)), boxes_d)
        for k in ops.INPAINT_KEYS:
            a = got[k].cpu().numpy()
            assert not a[v].any(), (v, off, k)
            others = [i for i in range(len(BOXES)) if i != v]
            assert a[others].tobytes() == host[k][others].tobytes(), (v, off, k)
    # the same offsets on the host are refused before any launch
    bad = offs.copy()
    bad[1] = buf.size
    with pytest.raises(ValueError, match="leaves the buffer"):
        ops.inpaint_inputs_boxed(case["frame_d"], (buf_d, bad), BOXES)
    with pytest.raises(ValueError, match=r"box_masks\[1\]"):
        ops.inpaint_inputs_boxed(case["frame_d"], [pieces[0], pieces[1][:, :-1]] + pieces[2:], BOXES)


def test_strided_outputs_and_no_vehicles(case):
    host = case["host"]["u8"]
    V = len(BOXES)
    wide = torch.full((V, 6, 256, 256), 7.0, device=DEV)
    out = {"img": wide[:, 0:3], "gray": wide[:, 3:4], "edge": wide[:, 4:5], "mask": wide[:, 5:6]}
    got = ops.inpaint_inputs_boxed(case["frame_d"], case["u8"], BOXES, out=out)
    assert all(got[k] is out[k] for k in ops.INPAINT_KEYS)
    _same(out, host, "strided out=")
    empty = ops.inpaint_inputs_boxed(case["frame_d"], [], np.zeros((0, 4), np.int64))
    assert empty["img"].shape == (0, 3, 256, 256)
