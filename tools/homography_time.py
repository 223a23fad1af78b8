#!/usr/bin/env python3
"""What fitting the plane homographies on the device is worth (GPU box) -> profiles/homography_time.json.

For 8 and 64 vehicles on a 720 x 1280 frame:
  host_stage_ms    the host path of the stage: warp_jobs_frame + the LAPACK inversion + the pinned upload of (minv, index),
                   wall time of the host thread with an idle GPU (median of N)
  device_stage_ms  the new stage: one pinned upload of the corner points and visibilities + fusg_plane_homographies, between
                   two HIP events (median of N); device_stage_host_ms: what the host thread spends issuing it
  frame_ms         run_frames (12 frames, two scenes alternating, one frame in flight: bench.py's "frame_mode") with
                   device_homography off and on, the two arms alternating in one process, median over the rounds
The 8-vehicle "off" arm is bench.py's frame_mode figure (same scenes, same loop)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from future_urban_scene_generation_amd import ops  # noqa: E402
from future_urban_scene_generation_amd.pipeline import VehiclePipeline, synth_frame  # noqa: E402
from future_urban_scene_generation_amd.warp_learn import planes_utils as pu  # noqa: E402


def host_stage(sc, dev):
    jobs = pu.warp_jobs_frame(sc["src_kp"], sc["dst_kp"], sc["src_vis"], sc["dst_vis"])
    Hs = [H12 for jb in jobs for _, _, H12, _ in jb]
    idx = [[v * 5 + i, v * 5 + j] for v, jb in enumerate(jobs) for i, j, _, _ in jb]
    minv = np.linalg.inv(np.asarray(Hs, dtype=np.float64).reshape(len(Hs), 3, 3)).reshape(len(Hs), 9)
    return ops.h2d(minv, dev), ops.h2d(np.asarray(idx, np.int32), dev)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--vehicles", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("-o", "--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                        "homography_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    pipe = VehiclePipeline(dev)
    res = {"device": torch.cuda.get_device_name(0), "frame": "720x1280", "rounds": a.rounds, "reps": a.reps, "vehicles": {}}
    for V in a.vehicles:
        sc = synth_frame(V, (720, 1280), dev, seed=3)
        sc["vehicle_seeds"] = list(range(V))
        sc2 = synth_frame(V, (720, 1280), dev, seed=4)
        sc2["vehicle_seeds"] = list(range(100, 100 + V))
        args = (sc["src_kp"], sc["dst_kp"], sc["src_vis"], sc["dst_vis"])
        for _ in range(3):
            host_stage(sc, dev)
            pu.plane_homographies_device(*args, dev)
        torch.cuda.synchronize()
        th, td, tdh = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            host_stage(sc, dev)
            th.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            pu.plane_homographies_device(*args, dev)
            e1.record()
            tdh.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            td.append(e0.elapsed_time(e1))
        minv, index = pu.plane_homographies_device(*args, dev)
        frames = {False: [], True: []}
        NF = 12 if V <= 8 else 4
        for flag in (False, True):                                             # warm-up: plans recorded, workspaces made
            pipe.device_homography = flag
            for _ in pipe.run_frames([sc, sc2, sc]):
                pass
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for flag in (False, True):
                pipe.device_homography = flag
                t0 = time.perf_counter()
                for _ in pipe.run_frames([sc, sc2] * (NF // 2)):
                    pass
                torch.cuda.synchronize()
                frames[flag].append((time.perf_counter() - t0) / NF * 1e3)
        pipe.device_homography = False
        med = statistics.median
        res["vehicles"][str(V)] = {
            "jobs": int((index[:, 0] >= 0).sum()), "rows": int(index.shape[0]),
            "host_stage_ms": round(med(th), 4), "host_stage_ms_min_max": [round(min(th), 4), round(max(th), 4)],
            "device_stage_ms": round(med(td), 4), "device_stage_ms_min_max": [round(min(td), 4), round(max(td), 4)],
            "device_stage_host_ms": round(med(tdh), 4),
            "frames_per_round": NF,
            "frame_ms_off": round(med(frames[False]), 3), "frame_ms_on": round(med(frames[True]), 3),
            "frame_ms_off_rounds": [round(x, 3) for x in frames[False]], "frame_ms_on_rounds": [round(x, 3) for x in frames[True]]}
        print(V, json.dumps(res["vehicles"][str(V)]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
