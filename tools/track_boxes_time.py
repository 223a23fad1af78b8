#!/usr/bin/env python
"""What linking the boxes of 64 frames costs on the device (GPU box) -> profiles/track_boxes_time.json.

Per workload - 64 frames with 8 and with 64 vehicles a frame (K = 64), for 1 video and for 16 videos in one launch - medians of 9
after a warm-up, arms alternating:
  call_ms     fusg_link_boxes on tables prepared once, the state zeroed before every launch, between two HIP events around
              `--inner` launches (each with its own zeroing copy, which is inside the events)
  op_ms       one ops.link_boxes call (checks, buffers, the launch) and a synchronise, host wall time
  host_ms     the route without the kernel: read the box tables back (ops.d2h of boxes and stats) and run the host twin
              (ops.link_boxes_host) over the videos on `--threads` threads, host wall time; twin_ms is the twin alone
The vehicles are synthetic: boxes of 40 x 24 that drift 3 to 6 pixels a frame on lanes, one frame in ten missing."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from future_urban_scene_generation_amd import _lib as L  # noqa: E402
from future_urban_scene_generation_amd import ops  # noqa: E402


def video(V, T, K, seed):
    rng = np.random.default_rng(seed)
    boxes, stats = np.zeros((T, K, 4), np.int32), np.zeros((T, 4), np.int32)
    x, v, y = rng.integers(0, 1200, V), rng.integers(3, 7, V) * rng.choice([-1, 1], V), 30 * np.arange(V) % 700 + 40 * (np.arange(V) // 24)
    for t in range(T):
        seen = [i for i in range(V) if rng.random() > 0.1]
        for k, i in enumerate(seen):
            x0 = int(x[i] + v[i] * t) % 1240
            boxes[t, k] = (x0, y[i], x0 + 40, y[i] + 24)
        stats[t, 0] = len(seen)
    return boxes, stats


def median(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(REPO, "profiles", "track_boxes_time.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_boxes_time: needs a HIP device (a CPU run measures nothing)")
    dev, T, K, N = torch.device("cuda:0"), 64, 64, 1024
    lib = L.lib()
    res = {"device": torch.cuda.get_device_name(0), "frames": T, "K": K, "max_tracks": N, "reps": a.reps, "inner": a.inner, "threads": a.threads,
           "params": {"iou": [3, 10], "max_gap": 2, "predict": 1}, "workloads": []}
    pool = ThreadPoolExecutor(a.threads)
    for V in (8, 64):
        for S in (1, 16):
            vids = [video(V, T, K, 100 * V + s) for s in range(S)]
            db, ds = [torch.from_numpy(b).to(dev) for b, _ in vids], [torch.from_numpy(s).to(dev) for _, s in vids]
            cb, cs = torch.cat(db), torch.cat(ds)
            first, t0 = np.arange(S + 1, dtype=np.int32) * T, np.zeros((S,), np.int32)
            state, zero = torch.zeros((S, ops.LINK_BOXES_STATE_WORDS), dtype=torch.int32, device=dev), torch.zeros((S, ops.LINK_BOXES_STATE_WORDS), dtype=torch.int32, device=dev)
            ids, tracks, ost = (torch.empty(s, dtype=torch.int32, device=dev) for s in ((S * T, K), (S, N, 4), (S, 4)))

            def call():
                state.copy_(zero)
                L.check(lib.fusg_link_boxes(cb.data_ptr(), cs.data_ptr(), first.ctypes.data, t0.ctypes.data, S, K, 3, 10, 2, 1, N, state.data_ptr(),
                                            ids.data_ptr(), tracks.data_ptr(), ost.data_ptr(), ops.stream_ptr()), "track_boxes_time")

            def host():
                hb, hs = ops.d2h(cb), ops.d2h(cs)
                t1 = time.perf_counter()
                out = list(pool.map(lambda s: ops.link_boxes_host(hb[s * T:(s + 1) * T], hs[s * T:(s + 1) * T], max_tracks=N), range(S)))
                return out, time.perf_counter() - t1
            call()
            got = [t.cpu().numpy() for t in (ids, tracks, ost)]
            want, _ = host()
            same = all(np.array_equal(got[0][s * T:(s + 1) * T], want[s][0]) and np.array_equal(got[1][s], want[s][1]) and np.array_equal(got[2][s], want[s][2])
                       for s in range(S))
            call_ms, op_ms, host_ms, twin_ms = [], [], [], []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.inner):
                    call()
                e1.record()
                torch.cuda.synchronize()
                call_ms.append(e0.elapsed_time(e1) / a.inner)
                t1 = time.perf_counter()
                ops.link_boxes(db, ds, max_tracks=N)
                torch.cuda.synchronize()
                op_ms.append(1e3 * (time.perf_counter() - t1))
                t1 = time.perf_counter()
                _, tw = host()
                host_ms.append(1e3 * (time.perf_counter() - t1))
                twin_ms.append(1e3 * tw)
            w = {"vehicles": V, "videos": S, "device_equals_twin": bool(same), "n_tracks": got[2][:, 0].tolist(), "flags": got[2][:, 3].tolist(),
                 "call_ms": median(call_ms), "call_ms_range": [min(call_ms), max(call_ms)], "op_ms": median(op_ms), "op_ms_range": [min(op_ms), max(op_ms)],
                 "host_ms": median(host_ms), "host_ms_range": [min(host_ms), max(host_ms)], "twin_ms": median(twin_ms)}
            print(json.dumps(w))
            res["workloads"].append(w)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
