#!/usr/bin/env python3
"""GPU box, analysis tool: the first frames of a video (720 x 1280, f16x3, replay=True in both arms) frame by frame with one
frame in flight (`run_frames(replay=True)`, the path of the parent commit) against batched passes (`run_frames_batched(replay=True)`:
groups of at most 64 rows, padded to 4 / 8 / 16 / 32 / 64).  Workloads: 16 frames x 2 vehicles, 8 frames x 8 vehicles and a ragged
mix of 20 frames with 0..5 vehicles (38 rows: one group, padded to 64 - the padding cost is in its figure).  Every scene has a frame
of its own.  The arms alternate video by video in one process after a warm-up of both; each video ends in a device synchronise;
the medians of --reps (default 9) go to --out (default profiles/frame_batch_time.json) with the device's name and the date.

--geometry: the same videos as GEOMETRY-MODE scenes (a frame, boxes, intrinsics and an index into one CAD bank of boxes around
well-posed keypoints; device_pose and device_homography on): `run_frames(replay=True)` against
`run_frames_batched_geometry(replay=True)`, the same protocol, plus the `ops.d2h` calls per frame of either arm; to
profiles/frame_batch_geometry_time.json.

    python tools/frame_batch_time.py
    python tools/frame_batch_time.py --workloads 16x2          # one workload
    python tools/frame_batch_time.py --geometry"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HW = (720, 1280)
WORKLOADS = {"16x2": [2] * 16, "8x8": [8] * 8, "ragged": [1, 3, 0, 2, 1, 4, 2, 1, 0, 3, 1, 2, 5, 1, 2, 3, 0, 1, 4, 2]}
ARMS = ("frames_replay", "batched_replay")
GEOMETRY_ARMS = ("frames_replay", "batched_geometry_replay")


def geometry(args):
    """The --geometry table: one geometry-mode pipeline and one CAD bank per workload."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    import torch

    import oracle
    import render_ref as RR
    from future_urban_scene_generation_amd import ops
    from future_urban_scene_generation_amd import pipeline as pl
    from future_urban_scene_generation_amd import render as R
    if not torch.cuda.is_available():
        raise SystemExit("frame_batch_time: needs a HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops.set_precision("f16x3")
    pipe = pl.VehiclePipeline(dev, device_pose=True, device_homography=True)
    copies = []
    orig = ops.d2h
    ops.d2h = lambda t: (copies.append(1), orig(t))[1]
    table = []
    for name in args.workloads:
        counts = WORKLOADS[name]
        scenes, meshes = [], []
        pipe.cad_bank = None
        for f, V in enumerate(counts):                                # the given-geometry videos' frames, boxes and cameras
            sc = pl.synth_frame(max(V, 1), HW, dev, seed=100 + f)
            geo = {"frame": sc["frame"], "bboxes": sc["bboxes"][:V], "focals": sc["focals"], "centers": sc["centers"],
                   "cad_idx": len(meshes) + np.arange(V), "vehicle_seeds": [1000 * f + v for v in range(V)]}
            if V:
                kp = pipe.run_frame(pl.slice_scene(sc, 0, V))["kp_xy"].cpu().numpy()
                kp3d = oracle.frame.well_posed_kp3d(kp, sc["focals"], sc["centers"], seed=2)
                for v in range(V):
                    mv, mt = RR.box_around(kp3d[v], n=13)
                    meshes.append((mv / R.SCALE, mt, kp3d[v] / R.SCALE))
            scenes.append(geo)
            del sc
        pipe._frame_plans.clear()
        pipe.cad_bank = R.CadBank(meshes)
        groups = pl.frame_batch_groups(counts)
        padded = [pl.frame_batch_pad(sum(counts[lo:hi])) for lo, hi in groups]
        arms = {"frames_replay": lambda: list(pipe.run_frames(scenes, replay=True)),
                "batched_geometry_replay": lambda: pipe.run_frames_batched_geometry(scenes, replay=True)}
        ms = {n: [] for n in GEOMETRY_ARMS}
        d2h = {n: [] for n in GEOMETRY_ARMS}
        skipped = None
        for rep in range(args.warmup + args.reps):
            for n in GEOMETRY_ARMS:                                   # the arms alternate video by video
                torch.cuda.synchronize()
                del copies[:]
                t0 = time.perf_counter()
                out = arms[n]()
                torch.cuda.synchronize()
                assert len(out) == len(counts)
                if rep >= args.warmup:
                    ms[n].append((time.perf_counter() - t0) * 1e3)
                    d2h[n].append(len(copies))
                skipped = sum(len(o["skipped"]) for o in out)
        row = {"workload": name, "frames": len(counts), "vehicles_per_frame": counts, "rows": sum(counts), "groups": groups,
               "padded_rows_per_group": padded, "frame_hw": list(HW), "precision": "f16x3", "replay": True, "reps": args.reps,
               "device_pose": True, "device_homography": True, "skipped_vehicles": skipped,
               "recorded_plans": sorted(str(k) for k in pipe._frame_plans)}
        for n in GEOMETRY_ARMS:
            med = statistics.median(ms[n])
            row[n] = {"ms_per_video": med, "ms_per_frame": med / len(counts), "min": min(ms[n]), "max": max(ms[n]),
                      "d2h_calls_per_video": statistics.median(d2h[n]), "d2h_calls_per_frame": statistics.median(d2h[n]) / len(counts)}
        row["batched_geometry_replay_over_frames_replay"] = row["batched_geometry_replay"]["ms_per_video"] / row["frames_replay"]["ms_per_video"]
        print(json.dumps(row), flush=True)
        table.append(row)
        del scenes, out
        pipe._frame_plans.clear()
        torch.cuda.empty_cache()
    ops.d2h = orig
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/frame_batch_time.py --geometry", "device": torch.cuda.get_device_name(0),
                   "date": datetime.date.today().isoformat(), "table": table}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/frame_batch_time.json (--geometry: profiles/frame_batch_geometry_time.json)")
    ap.add_argument("--geometry", action="store_true", help="time geometry-mode first frames: frame by frame against the batched pass")
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "frame_batch_geometry_time.json" if args.geometry else "frame_batch_time.json")
    if args.geometry:
        return geometry(args)

    import torch
    from future_urban_scene_generation_amd import ops
    from future_urban_scene_generation_amd import pipeline as pl
    if not torch.cuda.is_available():
        raise SystemExit("frame_batch_time: needs a HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops.set_precision("f16x3")
    pipe = pl.VehiclePipeline(dev)
    table = []
    for name in args.workloads:
        counts = WORKLOADS[name]
        scenes = []
        for f, V in enumerate(counts):
            sc = pl.synth_frame(max(V, 1), HW, dev, seed=100 + f)          # (a frame of its own per scene)
            sc = pl.slice_scene(sc, 0, V)
            sc["vehicle_seeds"] = [1000 * f + v for v in range(V)]
            scenes.append(sc)
        groups = pl.frame_batch_groups(counts)
        padded = [pl.frame_batch_pad(sum(counts[lo:hi])) for lo, hi in groups]
        arms = {"frames_replay": lambda: list(pipe.run_frames(scenes, replay=True)),
                "batched_replay": lambda: pipe.run_frames_batched(scenes, replay=True)}
        ms = {n: [] for n in ARMS}
        for rep in range(args.warmup + args.reps):
            for n in ARMS:                                            # the arms alternate video by video
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = arms[n]()
                torch.cuda.synchronize()
                assert len(out) == len(counts)
                if rep >= args.warmup:
                    ms[n].append((time.perf_counter() - t0) * 1e3)
        plans = sorted(str(k) for k in pipe._frame_plans)
        row = {"workload": name, "frames": len(counts), "vehicles_per_frame": counts, "rows": sum(counts), "groups": groups,
               "padded_rows_per_group": padded, "frame_hw": list(HW), "precision": "f16x3", "replay": True, "reps": args.reps,
               "recorded_plans": plans}
        for n in ARMS:
            med = statistics.median(ms[n])
            row[n] = {"ms_per_video": med, "ms_per_frame": med / len(counts), "min": min(ms[n]), "max": max(ms[n])}
        row["batched_replay_over_frames_replay"] = row["batched_replay"]["ms_per_video"] / row["frames_replay"]["ms_per_video"]
        print(json.dumps(row), flush=True)
        table.append(row)
        del scenes, out
        pipe._frame_plans.clear()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/frame_batch_time.py", "device": torch.cuda.get_device_name(0),
                   "date": datetime.date.today().isoformat(), "table": table}, f, indent=1)


if __name__ == "__main__":
    main()
