#!/usr/bin/env python3
"""What estimating a video's background frame on the device costs (GPU box) -> profiles/background_time.json.

T = 64 frames of 720 x 1280 x 3 uint8 (a seeded background, +-6 of noise per frame, eight 60 x 40 .. 180 x 120 rectangles per frame
that drift), as separate allocations, with the rectangles' boxes (margin 8, min_valid 8) and without boxes.  Medians of 9 after a
warm-up, the arms alternating:
  kernel_ms   the launch alone: fusg_background_median_u8 on tables prepared once, between two HIP events around `--inner`
              back-to-back calls, per call
  op_ms       one ops.background_median call (its checks, the upload of the box table, the launch) and a synchronise, wall time
              of the host thread: what a caller pays
  copy_ms     (a) the traffic floor: a device-to-device copy of the same T H W 3 bytes (one [T, H, W, 3] stack into another),
              timed as kernel_ms is; floor_ratio = kernel_ms / copy_ms.  The copy also writes what it reads, the kernel writes
              4 H W bytes, so a kernel at the floor would sit below 1
  host_ms     (b) what a user does today: read the frames back, then the host twin (ops.background_median_host) over bands of
              rows on `--threads` threads; readback_ms / twin_ms: its two parts
The 177 MB of frames fit the 256 MiB Infinity Cache, for the kernel and for the copy alike."""
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


def video(T, H, W, nb, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H // 8 + 1, W // 8 + 1, 3))
    base = np.repeat(np.repeat(base, 8, axis=0), 8, axis=1)[:H, :W]
    x0, y0 = rng.integers(0, W, nb), rng.integers(0, H, nb)
    w, h = rng.integers(60, 181, nb), rng.integers(40, 121, nb)
    vx, vy = rng.integers(-9, 10, nb), rng.integers(-3, 4, nb)
    rgb = rng.integers(0, 256, (nb, 3))
    frames, boxes = [], []
    for t in range(T):
        f = np.clip(base + rng.integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)
        bt = []
        for i in range(nb):
            xa, ya = int(x0[i] + vx[i] * t), int(y0[i] + vy[i] * t)
            xb, yb = xa + int(w[i]) - 1, ya + int(h[i]) - 1
            f[max(ya, 0):max(min(yb, H - 1) + 1, 0), max(xa, 0):max(min(xb, W - 1) + 1, 0)] = rgb[i]
            bt.append([xa, ya, xb, yb])
        frames.append(f)
        boxes.append(np.asarray(bt, dtype=np.int64).reshape(-1, 4))
    return frames, boxes


def host_twin(frames, boxes, margin, min_valid, pool, threads):
    """The host twin over `threads` bands of rows: a band's pixels see the boxes moved up by the band's first row."""
    H = frames[0].shape[0]
    cuts = [c for c in np.array_split(np.arange(H), threads) if len(c)]

    def band(c):
        y0, y1 = int(c[0]), int(c[-1]) + 1
        bx = None if boxes is None else [b - np.asarray([0, y0, 0, y0]) for b in boxes]
        return ops.background_median_host([f[y0:y1] for f in frames], bx, margin, min_valid)
    parts = list(pool.map(band, cuts))
    return np.concatenate([p[0] for p in parts], axis=0), np.concatenate([p[1] for p in parts], axis=0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, nargs=2, default=[720, 1280], metavar=("H", "W"))
    ap.add_argument("--boxes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("-o", "--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                        "background_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("background_time: needs a HIP device (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    T, (H, W) = args.frames, args.size
    margin, min_valid = 8, max(1, T // 8)
    frames, boxes = video(T, H, W, args.boxes, 64)
    dframes = [torch.from_numpy(f).to(dev) for f in frames]
    src = torch.stack(dframes)
    dst = torch.empty_like(src)
    read_bytes, write_bytes = T * H * W * 3, H * W * 4
    res = {"device": torch.cuda.get_device_name(0), "frames": T, "size": [H, W], "boxes_per_frame": args.boxes, "margin": margin,
           "min_valid": min_valid, "reps": args.reps, "inner": args.inner, "threads": args.threads, "read_bytes": read_bytes,
           "write_bytes": write_bytes, "arms": {}}
    med = statistics.median

    def events(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.inner

    with ThreadPoolExecutor(args.threads) as pool:
        for arm, bx in (("boxes", boxes), ("no_boxes", None)):
            out = (torch.empty((H, W, 3), dtype=torch.uint8, device=dev), torch.empty((H, W), dtype=torch.uint8, device=dev))
            for _ in range(2):                                    # warm-up: code objects, allocator, thread pool
                ops.background_median(dframes, bx, margin, min_valid, out=out)
                dst.copy_(src)
                want = host_twin(frames, bx, margin, min_valid, pool, args.threads)
            same = bool(np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[1].cpu().numpy(), want[1]))
            # the launch alone: the tables ops.background_median builds per call, built once
            flat, offs, _, _ = ops._background_args(T, bx, margin, min_valid, "background_time")
            dbox = ops.h2d(flat, dev) if flat.shape[0] else None
            ptrs = (C.c_void_p * T)(*[f.data_ptr() for f in dframes])
            lib, st = L.lib(), ops.stream_ptr()

            def launch():
                L.check(lib.fusg_background_median_u8(ptrs, T, H, W, dbox.data_ptr() if dbox is not None else None, offs.ctypes.data, margin,
                                                      min_valid, out[0].data_ptr(), out[1].data_ptr(), st), "background_time")
            t_dev, t_op, t_copy, t_host, t_rb, t_tw = [], [], [], [], [], []
            for _ in range(args.reps):
                t_dev.append(events(launch))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ops.background_median(dframes, bx, margin, min_valid, out=out)
                torch.cuda.synchronize()
                t_op.append((time.perf_counter() - t0) * 1e3)
                t_copy.append(events(lambda: dst.copy_(src)))
                t0 = time.perf_counter()
                back = [f.cpu().numpy() for f in dframes]
                t1 = time.perf_counter()
                host_twin(back, bx, margin, min_valid, pool, args.threads)
                t2 = time.perf_counter()
                t_rb.append((t1 - t0) * 1e3)
                t_tw.append((t2 - t1) * 1e3)
                t_host.append((t2 - t0) * 1e3)
            d, c = med(t_dev), med(t_copy)
            same = same and bool(np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[1].cpu().numpy(), want[1]))
            res["arms"][arm] = {"kernel_ms": d, "kernel_ms_min_max": [min(t_dev), max(t_dev)], "op_ms": med(t_op), "copy_ms": c,
                                "copy_ms_min_max": [min(t_copy), max(t_copy)], "floor_ratio": d / c,
                                "kernel_read_GBps": read_bytes / d / 1e6, "copy_read_GBps": read_bytes / c / 1e6,
                                "host_ms": med(t_host), "host_ms_min_max": [min(t_host), max(t_host)], "readback_ms": med(t_rb),
                                "twin_ms": med(t_tw), "results_agree": same,
                                "fallback_pixels": int((want[1] < min_valid).sum())}
            print(arm, json.dumps(res["arms"][arm]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
