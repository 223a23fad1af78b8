#!/usr/bin/env python3
"""What the vehicle masks from the background, and the erase that uses them, cost on the device (GPU box)
-> profiles/foreground_time.json.

One 720 x 1280 frame: a seeded blocky background, +-6 of noise, and per box a body of about two thirds of the box with a
background-coloured window in it.  Three configurations: 8 boxes of about 200 x 150 (planes in LDS), 64 such boxes, and one
560 x 700 box (planes in the scratch buffer).  Defaults 24 / 1 / 3, grow 4.  Medians of `--reps` after a warm-up:
  mask_ms     the launch alone: fusg_foreground_masks_u8 on tables prepared once, between two HIP events around `--inner`
              back-to-back calls, per call.  ONE workgroup per box: with 8 boxes 8 of the 256 CUs work
  mask_op_ms  one ops.foreground_masks call (checks, the upload of the tables, the launch) and a synchronise, host wall time
  erase_ms    fusg_erase_boxes_u8 (its two launches), timed as mask_ms is
  copy_ms     for scale: a device-to-device copy of the frame's H W 3 bytes, timed the same way
  host_ms     what a user without the kernel does: read frame and background back (readback_ms), then the host twin
              (ops.foreground_masks_host) over the boxes on `--threads` threads (twin_ms)
What this replaces in the reference - one Mask R-CNN run per vehicle and frame - is not measured: torchvision's detector is not
part of this package's environment."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from future_urban_scene_generation_amd import _lib as L  # noqa: E402
from future_urban_scene_generation_amd import ops  # noqa: E402


def scene(H, W, boxes, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(20, 200, (H // 8 + 1, W // 8 + 1, 3))
    bg = np.repeat(np.repeat(base, 8, axis=0), 8, axis=1)[:H, :W]
    fr = bg + rng.integers(-6, 7, (H, W, 3))
    cores = []
    for x0, y0, x1, y1 in boxes:
        w, h = x1 - x0, y1 - y0
        bx0, by0, bx1, by1 = x0 + w // 6, y0 + h // 6, x1 - w // 6, y1 - h // 6
        body = fr[by0:by1, bx0:bx1]
        body[...] = (body + 90) % 256
        wx0, wy0 = bx0 + (bx1 - bx0) // 3, by0 + (by1 - by0) // 4
        fr[wy0:wy0 + (by1 - by0) // 4, wx0:wx0 + (bx1 - bx0) // 3] = bg[wy0:wy0 + (by1 - by0) // 4, wx0:wx0 + (bx1 - bx0) // 3]
        cores.append([x0 + w // 4, y0 + h // 4, x1 - w // 4, y1 - h // 4])
    return np.clip(fr, 0, 255).astype(np.uint8), bg.astype(np.uint8), np.asarray(cores, dtype=np.int64)


def grid_boxes(n, H, W, seed):
    rng = np.random.default_rng(seed)
    cols = 8 if n > 8 else 4
    out = []
    for i in range(n):
        w, h = int(rng.integers(180, 221)), int(rng.integers(130, 171))
        x0 = min(W - w, (i % cols) * (W // cols) + int(rng.integers(0, 20)))
        y0 = min(H - h, (i // cols) * ((H - 170) // max(1, (n - 1) // cols)) + int(rng.integers(0, 10)))
        out.append([x0, y0, x0 + w, y0 + h])
    return np.asarray(out, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=2, default=[720, 1280], metavar=("H", "W"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("-o", "--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                        "foreground_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("foreground_time: needs a HIP device (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    H, W = args.size
    par = dict(thr=24, open_r=1, close_r=3, grow=4, fallback=True)
    res = {"device": torch.cuda.get_device_name(0), "size": [H, W], "params": par, "reps": args.reps, "inner": args.inner,
           "threads": args.threads, "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "configs": {}}
    med = statistics.median
    lib = L.lib()

    def events(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.inner

    configs = (("boxes_8", grid_boxes(8, H, W, 1)), ("boxes_64", grid_boxes(64, H, W, 2)),
               ("box_560x700", np.asarray([[100, 80, 800, 640]], dtype=np.int64)))
    with ThreadPoolExecutor(args.threads) as pool:
        for name, boxes in configs:
            fr, bg, cores = scene(H, W, boxes.tolist(), 7)
            dfr, dbg = torch.from_numpy(fr).to(dev), torch.from_numpy(bg).to(dev)
            n = len(boxes)
            mb = (int((boxes[:, 3] - boxes[:, 1]).max()), int((boxes[:, 2] - boxes[:, 0]).max()))

            def twin(f, g):
                cuts = [c for c in np.array_split(np.arange(n), args.threads) if len(c)]
                parts = list(pool.map(lambda c: ops.foreground_masks_host(f, g, boxes[c], cores[c], **par), cuts))
                return np.concatenate([p[0][0] for p in parts]), np.concatenate([p[1] for p in parts])
            for _ in range(2):                                    # warm-up: code objects, allocator, thread pool
                (buf, offs), stats = ops.foreground_masks(dfr, dbg, boxes, cores, **par)
                erased = ops.erase_to_background(dfr, dbg, (buf, offs), boxes)
                copy = dfr.clone()
                want = twin(fr, bg)
            same = bool(np.array_equal(buf.cpu().numpy(), want[0]) and np.array_equal(stats.cpu().numpy(), want[1]))
            same = same and bool(np.array_equal(erased.cpu().numpy(), ops.erase_to_background_host(fr, bg, (want[0], offs.cpu().numpy()), boxes)))
            # the launches alone: the tables the ops build per call, built once
            tab = ops.h2d(np.concatenate([boxes, cores]).astype(np.int32), dev)
            sb = int(lib.fusg_foreground_masks_scratch_bytes(n, mb[0], mb[1]))
            scratch = torch.empty((max(sb, 4),), dtype=torch.uint8, device=dev)
            fp, gp = (C.c_void_p * 1)(dfr.data_ptr()), (C.c_void_p * 1)(dbg.data_ptr())
            rows = (C.c_int32 * 2)(0, n)
            st = ops.stream_ptr()

            def mask_launch():
                L.check(lib.fusg_foreground_masks_u8(fp, gp, rows, 1, H, W, tab[:n].data_ptr(), tab[n:].data_ptr(), offs.data_ptr(), n, par["thr"],
                                                     par["open_r"], par["close_r"], par["grow"], 1, mb[0], mb[1], buf.data_ptr(),
                                                     int(buf.numel()), stats.data_ptr(), scratch.data_ptr(), st), "foreground_time")

            def erase_launch():
                L.check(lib.fusg_erase_boxes_u8(dfr.data_ptr(), dbg.data_ptr(), H, W, buf.data_ptr(), int(buf.numel()), offs.data_ptr(),
                                                tab[:n].data_ptr(), n, erased.data_ptr(), st), "foreground_time")
            t = {k: [] for k in ("mask", "op", "erase", "copy", "host", "rb", "tw")}
            for _ in range(args.reps):
                t["mask"].append(events(mask_launch))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ops.foreground_masks(dfr, dbg, boxes, cores, **par)
                torch.cuda.synchronize()
                t["op"].append((time.perf_counter() - t0) * 1e3)
                t["erase"].append(events(erase_launch))
                t["copy"].append(events(lambda: copy.copy_(dfr)))
                t0 = time.perf_counter()
                back = (dfr.cpu().numpy(), dbg.cpu().numpy())
                t1 = time.perf_counter()
                twin(*back)
                t2 = time.perf_counter()
                t["rb"].append((t1 - t0) * 1e3)
                t["tw"].append((t2 - t1) * 1e3)
                t["host"].append((t2 - t0) * 1e3)
            res["configs"][name] = {
                "boxes": n, "max_box": list(mb), "box_pixels": int(((boxes[:, 3] - boxes[:, 1]) * (boxes[:, 2] - boxes[:, 0])).sum()),
                "planes": "lds" if sb == 0 else "scratch", "scratch_bytes": sb, "mask_ms": med(t["mask"]),
                "mask_ms_min_max": [min(t["mask"]), max(t["mask"])], "mask_op_ms": med(t["op"]), "erase_ms": med(t["erase"]),
                "erase_ms_min_max": [min(t["erase"]), max(t["erase"])], "copy_ms": med(t["copy"]), "host_ms": med(t["host"]),
                "host_ms_min_max": [min(t["host"]), max(t["host"])], "readback_ms": med(t["rb"]), "twin_ms": med(t["tw"]),
                "mask_pixels": int(want[1][:, 2].sum()), "flags_or": int(np.bitwise_or.reduce(want[1][:, 3])), "results_agree": same}
            print(name, json.dumps(res["configs"][name]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
