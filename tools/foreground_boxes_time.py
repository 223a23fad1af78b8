#!/usr/bin/env python3
"""What the vehicle boxes from the background cost on the device (GPU box) -> profiles/foreground_boxes_time.json.

720 x 1280 frames: a seeded blocky background, +-6 of noise, and per vehicle a body that differs by 90; frame f shifts the
vehicles by f pixels.  Configurations: 1 and 64 frames with about 8 (200 x 150) and about 64 (70 x 45) vehicles at the defaults
(thr 24, cell 8, min_count 16, close_r 1), and the worst case for the label pass: the 96 x 96 frame whose 24 x 24 cells of 4 are
a checkerboard - 288 components, 256 of them examined one after the other by ONE workgroup.  Medians of `--reps` after a warm-up:
  call_ms     fusg_foreground_boxes_u8 on buffers prepared once (its two launches), between two HIP events around `--inner`
              back-to-back calls, per call
  cell_ms, label_ms   the two kernels apart, from the device times torch.profiler reports for them over reps x inner calls
              (null where the profiler gives no kernel events); the label pass is one workgroup per frame
  op_ms       one ops.foreground_boxes call (checks, buffers, the launches) and a synchronise, host wall time
  copy_ms     the cell pass's bandwidth yardstick: a device-to-device copy of the bytes it reads (frames and backgrounds, 6 per
              pixel), timed as call_ms is
  host_ms     what a user without the kernels does: read the frames back (readback_ms), then the host twin
              (ops.foreground_boxes_host) over the frames on `--threads` threads (twin_ms)
No detector or tracker is part of this package's environment: what the boxes replace is not measured."""
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


def vehicles(n, H, W):
    cols = 8 if n > 8 else 4
    rows = -(-n // cols)
    w, h = (70, 45) if n > 8 else (200, 150)
    return [((i % cols) * (W // cols) + 10, (i // cols) * ((H - h - 70) // max(1, rows - 1)) + 4, w, h) for i in range(n)]


def scene(T, H, W, n, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(20, 160, (H // 8 + 1, W // 8 + 1, 3))
    bg = np.repeat(np.repeat(base, 8, axis=0), 8, axis=1)[:H, :W].astype(np.uint8)
    frames = np.empty((T, H, W, 3), dtype=np.uint8)
    for f in range(T):
        fr = bg.astype(np.int16) + rng.integers(-6, 7, (H, W, 3), dtype=np.int16)
        for x, y, w, h in vehicles(n, H, W):
            fr[y + f % 60:y + f % 60 + h, x + f % 60:x + f % 60 + w] += 90
        frames[f] = np.clip(fr, 0, 255)
    return frames, bg


def checkerboard():
    bg = np.full((96, 96, 3), 50, dtype=np.uint8)
    fr = bg.copy()
    on = (np.add.outer(np.arange(96) // 4, np.arange(96) // 4) % 2) == 0
    fr[on] = 150
    return fr[None], bg


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=2, default=[720, 1280], metavar=("H", "W"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("-o", "--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                        "foreground_boxes_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("foreground_boxes_time: needs a HIP device (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    H, W = args.size
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, "threads": args.threads,
           "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "configs": {}}
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

    def kernels(fn):
        """Device milliseconds of the two kernels, every call of reps x inner; ([], []) without a working profiler."""
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(args.reps * args.inner):
                    fn()
                torch.cuda.synchronize()
            by = {"cells": [], "label": []}
            for e in prof.events():
                for key in by:
                    us = getattr(e, "device_time", None) or getattr(e, "cuda_time", 0)
                    if f"foreground_{key}_kernel" in e.name and us > 0:
                        by[key].append(us / 1e3)
            return by["cells"], by["label"]
        except Exception as e:  # noqa: BLE001 - the figures are optional, the reason is kept
            res.setdefault("profiler_error", repr(e))
            return [], []

    default = dict(thr=24, cell=8, min_count=16, open_r=0, close_r=1, min_area=400, min_w=12, min_h=12, max_boxes=64)
    worst = dict(default, cell=4, close_r=0, min_area=1, min_w=1, min_h=1)
    configs = [(f"frames_{T}_vehicles_{n}", (T, n), default) for T in (1, 64) for n in (8, 64)] + [("checkerboard_288", None, worst)]
    with ThreadPoolExecutor(args.threads) as pool:
        for name, tn, par in configs:
            frames, bg = checkerboard() if tn is None else scene(tn[0], H, W, tn[1], 7)
            T, h, w = frames.shape[:3]
            dfr, dbg = torch.from_numpy(frames).to(dev), torch.from_numpy(bg).to(dev)

            def twin(fr):
                cuts = [c for c in np.array_split(np.arange(T), args.threads) if len(c)]
                parts = list(pool.map(lambda c: ops.foreground_boxes_host(fr[c], bg, **par), cuts))
                return [np.concatenate([p[i] for p in parts]) for i in range(3)]
            for _ in range(2):                                    # warm-up: code objects, allocator, thread pool
                out = ops.foreground_boxes(dfr, dbg, **par)
                want = twin(frames)
            same = all(bool(np.array_equal(o.cpu().numpy(), t)) for o, t in zip(out, want))
            src = torch.cat([dfr.reshape(-1), dbg.reshape(-1).repeat(T)])
            dst = torch.empty_like(src)
            K = par["max_boxes"]
            scratch = torch.empty((int(lib.fusg_foreground_boxes_scratch_bytes(T, h, w, par["cell"])) // 4,), dtype=torch.int32, device=dev)
            fp = (C.c_void_p * T)(*[dfr[f].data_ptr() for f in range(T)])
            gp = (C.c_void_p * T)(*[dbg.data_ptr()] * T)
            roi = (C.c_int32 * 4)(0, 0, w, h)
            st = ops.stream_ptr()

            def call():
                L.check(lib.fusg_foreground_boxes_u8(fp, gp, T, h, w, par["thr"], par["cell"], par["min_count"], par["open_r"], par["close_r"],
                                                     par["min_area"], par["min_w"], par["min_h"], roi, K, out[0].data_ptr(), out[1].data_ptr(),
                                                     out[2].data_ptr(), scratch.data_ptr(), st), "foreground_boxes_time")
            t = {k: [] for k in ("call", "op", "copy", "host", "rb", "tw")}
            for _ in range(args.reps):
                t["call"].append(events(call))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ops.foreground_boxes(dfr, dbg, **par)
                torch.cuda.synchronize()
                t["op"].append((time.perf_counter() - t0) * 1e3)
                t["copy"].append(events(lambda: dst.copy_(src)))
                t0 = time.perf_counter()
                back = dfr.cpu().numpy()
                t1 = time.perf_counter()
                twin(back)
                t2 = time.perf_counter()
                t["rb"].append((t1 - t0) * 1e3)
                t["tw"].append((t2 - t1) * 1e3)
                t["host"].append((t2 - t0) * 1e3)
            cells, label = kernels(call)
            stats = want[2]
            res["configs"][name] = {
                "frames": T, "size": [h, w], "params": par, "input_bytes": int(src.numel()), "call_ms": med(t["call"]),
                "call_ms_min_max": [min(t["call"]), max(t["call"])], "cell_ms": med(cells) if cells else None,
                "label_ms": med(label) if label else None, "label_ms_min_max": [min(label), max(label)] if label else None,
                "kernel_samples": len(cells), "op_ms": med(t["op"]), "copy_ms": med(t["copy"]), "host_ms": med(t["host"]),
                "host_ms_min_max": [min(t["host"]), max(t["host"])], "readback_ms": med(t["rb"]), "twin_ms": med(t["tw"]),
                "kept_per_frame": [int(stats[:, 0].min()), int(stats[:, 0].max())], "examined_max": int(stats[:, 1].max()),
                "flags_or": int(np.bitwise_or.reduce(stats[:, 3])), "results_agree": same}
            print(name, json.dumps(res["configs"][name]))
            del src, dst, dfr
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
