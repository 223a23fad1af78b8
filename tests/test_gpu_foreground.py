"""GPU: the foreground-mask kernel (fusg_foreground_masks_u8) equals its host twin bit for bit, masks and stats, on every case of
tests/foreground_cases.py, inside canaries and with every refused box's bytes intact; the LDS and scratch variants agree; the
erase equals its twin; ops.inpaint_inputs_boxed takes the device pair as it is; one run_frame fed by foreground_inpaint equals
the run fed the same masks as pieces; and a recorded launch replays to the same bytes."""
import numpy as np
import pytest
import torch

import foreground_cases as fc
from conftest import synth_sd
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import ops
from future_urban_scene_generation_amd import pipeline as pl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(c):
    """The host twin's (buffer, stats) for a case, the buffer CANARY-filled before (through the library for a 'raw' case)."""
    buf = np.full(fc.buf_len_of(c), fc.CANARY, dtype=np.uint8)
    offs = fc.offsets_of(c)
    if not c.get("raw"):
        _, stats = ops.foreground_masks_host(c["frames"], c["backgrounds"], c["boxes"], c["cores"], frame_rows=c["frame_rows"],
                                             max_box=c.get("max_box"), out=(buf, offs), **c["params"])
        return buf, stats
    bx, cr = c["boxes"].astype(np.int32), c["cores"].astype(np.int32)
    stats = np.full((len(bx), 4), -1, dtype=np.int32)
    args = fc.raw_args(c, [f.ctypes.data for f in c["frames"]], [g.ctypes.data for g in c["backgrounds"]], bx.ctypes.data, cr.ctypes.data,
                       offs.ctypes.data, buf.ctypes.data, stats.ctypes.data)
    assert L.lib().fusg_foreground_masks_host(*args) == 0
    return buf, stats


def _device(c, max_box=None):
    """The kernel's (buffer, stats) as numpy: the masks go into the middle of a buffer full of CANARY, PAD bytes of it on both
    sides, which are checked."""
    n = fc.buf_len_of(c)
    whole = torch.full((PAD + n + PAD,), fc.CANARY, dtype=torch.uint8, device=DEV)
    mid, offs = whole[PAD:PAD + n], fc.offsets_of(c)
    frames, bgs = [_dev(f) for f in c["frames"]], [_dev(g) for g in c["backgrounds"]]
    if not c.get("raw"):
        (b, o), stats = ops.foreground_masks(frames, bgs, c["boxes"], c["cores"], frame_rows=c["frame_rows"],
                                             max_box=max_box if max_box is not None else c.get("max_box"), out=(mid, offs), **c["params"])
        assert b.data_ptr() == mid.data_ptr() and o.dtype == torch.int64 and np.array_equal(o.cpu().numpy(), offs)
    else:
        bx, cr, od = _dev(c["boxes"].astype(np.int32)), _dev(c["cores"].astype(np.int32)), _dev(offs)
        stats = torch.full((len(c["boxes"]), 4), -1, dtype=torch.int32, device=DEV)
        args = fc.raw_args(c, [f.data_ptr() for f in frames], [g.data_ptr() for g in bgs], bx.data_ptr(), cr.data_ptr(), od.data_ptr(),
                           mid.data_ptr(), stats.data_ptr())
        assert L.lib().fusg_foreground_masks_scratch_bytes(len(bx), *fc.max_box_of(c)) == 0
        L.check(L.lib().fusg_foreground_masks_u8(*args, None, ops.stream_ptr()), "foreground_masks_u8")
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert np.all(got[:PAD] == fc.CANARY) and np.all(got[PAD + n:] == fc.CANARY), "a byte outside the mask buffer was written"
    return got[PAD:PAD + n], stats.cpu().numpy()


@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_device_equals_host_twin_inside_canaries(name):
    c = fc.BY_NAME[name]
    buf, stats = _device(c)
    hbuf, hstats = _host(c)
    assert stats.dtype == np.int32 and np.array_equal(stats, hstats)
    assert np.array_equal(buf, hbuf)
    ebuf, estats = fc.expected(name)
    assert np.array_equal(hstats, estats) and np.array_equal(hbuf, ebuf)         # refused boxes and gaps still hold the canary


@pytest.mark.parametrize("name", ["seams_default", "seams_open0_close0_grow2", "comb_rows", "comb_cols", "holes", "ragged64",
                                  "corners_and_overlap", "leaves_buffer"])
def test_lds_and_scratch_variants_agree(name):
    """The same small boxes with the bound of the launch at 600 x 1000: the planes move from LDS to the scratch buffer."""
    c = fc.BY_NAME[name]
    lib = L.lib()
    assert lib.fusg_foreground_masks_scratch_bytes(len(c["boxes"]), *fc.max_box_of(c)) == 0
    assert lib.fusg_foreground_masks_scratch_bytes(len(c["boxes"]), 600, 1000) == len(c["boxes"]) * 2 * 600 * 32 * 4
    a, sa = _device(c)
    b, sb = _device(c, max_box=(600, 1000))
    assert np.array_equal(sa, sb) and np.array_equal(a, b)
    assert np.array_equal(sb, fc.expected(name)[1]) and np.array_equal(b, fc.expected(name)[0])


def test_erase_equals_host_twin_and_leaves_the_rest_of_the_frame():
    c = fc.BY_NAME["corners_and_overlap"]
    fr, bg = c["frames"][0], c["backgrounds"][0]
    p = dict(c["params"], grow=4)
    (buf, offs), _ = ops.foreground_masks(_dev(fr), _dev(bg), c["boxes"], c["cores"], **p)
    (hbuf, hoffs), _ = ops.foreground_masks_host(fr, bg, c["boxes"], c["cores"], **p)
    want = ops.erase_to_background_host(fr, bg, (hbuf, hoffs), c["boxes"])
    whole = torch.full((PAD + fr.size + PAD,), fc.CANARY, dtype=torch.uint8, device=DEV)
    out = whole[PAD:PAD + fr.size].view(fr.shape)
    got = ops.erase_to_background(_dev(fr), _dev(bg), (buf, offs), c["boxes"], out=out)
    assert got is out
    w = whole.cpu().numpy()
    assert np.all(w[:PAD] == fc.CANARY) and np.all(w[PAD + fr.size:] == fc.CANARY)
    got = got.cpu().numpy()
    assert np.array_equal(got, want)
    outside = np.ones(fr.shape[:2], dtype=bool)
    for x0, y0, x1, y1 in c["boxes"]:
        outside[y0:y1, x0:x1] = False
    assert outside.any() and np.array_equal(got[outside], fr[outside]) and not np.array_equal(got, fr)
    # host offsets, an unaligned output, no boxes
    odd = torch.empty((fr.size + 1,), dtype=torch.uint8, device=DEV)[1:].view(fr.shape)
    assert np.array_equal(ops.erase_to_background(_dev(fr), _dev(bg), (buf, hoffs), c["boxes"], out=odd).cpu().numpy(), want)
    none = ops.erase_to_background(_dev(fr), _dev(bg), (buf[:0], hoffs[:0]), np.zeros((0, 4), np.int64))
    assert np.array_equal(none.cpu().numpy(), fr)


def test_inpaint_inputs_boxed_takes_the_device_pair():
    c = fc.BY_NAME["grow4"]
    fr = c["frames"][0]
    pair, _ = ops.foreground_masks(_dev(fr), _dev(c["backgrounds"][0]), c["boxes"], c["cores"], **c["params"])
    hpair, _ = ops.foreground_masks_host(fr, c["backgrounds"][0], c["boxes"], c["cores"], **c["params"])
    a = ops.inpaint_inputs_boxed(_dev(fr), pair, c["boxes"])
    b = ops.inpaint_inputs_boxed(_dev(fr), (_dev(hpair[0]), hpair[1]), c["boxes"])
    for k in ops.INPAINT_KEYS:
        assert torch.equal(a[k], b[k]), k
    assert 0 < float(a["mask"].mean()) < 1


def test_run_frame_fed_by_foreground_inpaint():
    """scene['inpaint'] = foreground_inpaint(...) runs, and its inpainted boxes are those of the run fed the same masks as pieces."""
    ops.set_precision("f16x3")
    sds = {n: synth_sd(n) for n in ("hg", "icn", "vunet", "edge", "inpaint")}
    pipe = pl.VehiclePipeline(DEV, inpaint=True, state_dicts=sds)
    sc = pl.synth_frame(2, (360, 640), DEV, seed=17, inpaint="masks")
    sc["vehicle_seeds"] = [40, 41]
    bg = sc["frame"].clone()
    for x0, y0, x1, y1 in np.asarray(sc["bboxes"]).tolist():                     # the "vehicle": what differs from the background
        bg[y0 + 2:y1 - 2, x0 + 2:x1 - 2] = bg[y0 + 2:y1 - 2, x0 + 2:x1 - 2].to(torch.int16).add(70).remainder(256).to(torch.uint8)
    keys = set(sc)
    inp = pipe.foreground_inpaint(sc, bg)
    assert set(sc) == keys and set(inp) == {"boxes", "box_masks", "stats"}
    stats = inp["stats"].cpu().numpy()
    assert np.all(stats[:, 1] > 0) and np.all(stats[:, 3] & ops.FOREGROUND_REFUSED == 0)
    got = pipe.run_frame(dict(sc, inpaint=inp))
    buf, offs = inp["box_masks"]
    o = offs.cpu().numpy()
    pieces = [buf[o[v]:o[v] + (y1 - y0) * (x1 - x0)].view(y1 - y0, x1 - x0) for v, (x0, y0, x1, y1) in enumerate(inp["boxes"].tolist())]
    want = pipe.run_frame(dict(sc, inpaint={"boxes": inp["boxes"], "box_masks": pieces}))
    assert got["inpaint_u8"].shape == (2, 256, 256, 3) and torch.equal(got["inpaint_u8"], want["inpaint_u8"])
    assert torch.equal(got["frame_icn"], want["frame_icn"])
    erased = pipe.erase_vehicles(sc, bg)
    assert erased.shape == sc["frame"].shape and set(sc) == keys
    hole = erased != sc["frame"]
    assert hole.any() and torch.equal(erased[hole], bg[hole])


def test_a_recorded_launch_replays_to_the_same_bytes():
    c = fc.BY_NAME["ragged64_grow3_max_box_frame"]
    frames, bgs = [_dev(f) for f in c["frames"]], [_dev(g) for g in c["backgrounds"]]
    n = fc.buf_len_of(c)
    buf = torch.zeros((n,), dtype=torch.uint8, device=DEV)
    erased = torch.zeros(c["frames"][0].shape, dtype=torch.uint8, device=DEV)
    rows = c["frame_rows"]
    lib = L.lib()
    rec = ops.PlanRecorder()
    L.check(lib.fusg_plan_begin(rec.handle), "plan_begin")
    ops.RECORDER = rec
    try:
        (b, offs), stats = ops.foreground_masks(frames, bgs, c["boxes"], c["cores"], frame_rows=rows, max_box=c["max_box"],
                                                out=(buf, fc.offsets_of(c)), **c["params"])
        ops.erase_to_background(frames[0], bgs[0], (buf, offs[:rows[1]]), c["boxes"][:rows[1]], out=erased)
    finally:
        ops.RECORDER = None
        L.check(lib.fusg_plan_end(rec.handle), "plan_end")
    torch.cuda.synchronize()
    assert lib.fusg_plan_size(rec.handle) == 2
    first = (buf.cpu().numpy().copy(), stats.cpu().numpy().copy(), erased.cpu().numpy().copy())
    assert np.array_equal(first[0], fc.expected(c["name"])[0]) and np.array_equal(first[1], fc.expected(c["name"])[1])
    buf.fill_(7)
    stats.fill_(-1)
    erased.fill_(9)
    L.check(lib.fusg_plan_run(rec.handle), "plan_run")
    torch.cuda.synchronize()
    for a, t in zip(first, (buf, stats, erased)):
        assert np.array_equal(a, t.cpu().numpy())
    lib.fusg_plan_destroy(rec.handle)
