#!/usr/bin/env python3
"""GPU box, analysis tool: a clip's tail (F = 5 future frames, 720 x 1280, f16x3) frame by frame with one frame in flight
(`run_later_frames(replay=True)`, the path of the parent commit) against ONE batched pass (`run_later_frames_batched`, replayed and
eager), at 8 and 64 vehicles, with and without scene['inpaint'].  The arms alternate clip by clip in one process after a warm-up of
every arm; each clip tail ends in a device synchronise; the medians go to --out (default profiles/later_batch_time.json).

    python tools/later_batch_time.py                                  # the timing table
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/later_batch_time.py --arm batched_replay --vehicles 8
    python tools/later_batch_time.py --fold DIR/.../*_kernel_stats.csv  # adds the batched arm's per-kernel split to --out
    python tools/later_batch_time.py --geometry                       # a GEOMETRY-MODE clip tail -> profiles/later_batch_geometry_time.json

(The profiler slows the host: the split is taken in a run of its own, the times never under it.)

--geometry: the same clip tail in geometry mode (a CAD bank built around well-posed keypoints of the first hourglass run, as
tools/geometry_frame_time.py; scenes with 'steps', device_pose and device_homography on, replay=True) - `run_later_frames`, frame by
frame with its blocking read-back per frame (what the parent commit does for this input), against
`run_later_frames_batched_geometry`, one read-back per group.  Besides the medians it records, per arm, the number of `ops.d2h`
calls per clip tail, the host time spent inside them and (batched arm) the host time until the read-back is reached, i.e. the
time to queue the whole group."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

F, HW = 5, (720, 1280)
ARMS = ("frames_replay", "batched_replay", "batched_eager")


def fold(args):
    with open(args.fold) as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    clips = args.warmup + args.reps
    split = [{"kernel": r["Name"][:96], "calls_per_clip": int(r["Calls"]) / clips, "ms_per_clip": float(r["TotalDurationNs"]) / clips / 1e6,
              "share": float(r["TotalDurationNs"]) / total} for r in rows[:args.top]]
    rest = rows[args.top:]
    split.append({"kernel": f"({len(rest)} others)", "calls_per_clip": sum(int(r["Calls"]) for r in rest) / clips,
                  "ms_per_clip": sum(float(r["TotalDurationNs"]) for r in rest) / clips / 1e6,
                  "share": sum(float(r["TotalDurationNs"]) for r in rest) / total})
    with open(args.out) as f:
        doc = json.load(f)
    doc["batched_replay_kernel_split"] = {"vehicles": args.vehicles[0], "inpaint": bool(args.inpaint), "clips_profiled": clips,
                                          "gpu_ms_per_clip_tail": total / clips / 1e6,
                                          "launches_per_clip_tail": sum(int(r["Calls"]) for r in rows) / clips, "kernels": split}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["batched_replay_kernel_split"], indent=1))


GEOMETRY_ARMS = ("frames_replay", "batched_geometry_replay")


def geometry(args):
    """The --geometry table: one geometry-mode pipeline, per vehicle count a first frame and F later scenes along a trajectory."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    import torch

    import oracle
    import render_ref as RR
    from future_urban_scene_generation_amd import ops
    from future_urban_scene_generation_amd import render as R
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline, synth_frame
    if not torch.cuda.is_available():
        raise SystemExit("later_batch_time: needs a HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops.set_precision("f16x3")
    pipe = VehiclePipeline(dev, device_pose=True, device_homography=True)
    steps = R.trajectory_steps(np.c_[np.arange(F + 1.0) * 0.8, 0.05 * np.arange(F + 1.0) ** 2])
    waits = []                                                    # (entry time, seconds inside) of every ops.d2h
    orig = ops.d2h

    def d2h(t):
        t0 = time.perf_counter()
        a = orig(t)
        waits.append((t0, time.perf_counter() - t0))
        return a

    ops.d2h = d2h
    table = []
    for V in args.vehicles:
        sc = synth_frame(V, HW, dev, seed=3)
        pipe.cad_bank = None
        kp = pipe.run_frame(sc)["kp_xy"].cpu().numpy()
        kp3d = oracle.frame.well_posed_kp3d(kp, sc["focals"], sc["centers"], seed=2)
        meshes = []
        for v in range(V):
            mv, mt = RR.box_around(kp3d[v], n=13)
            meshes.append((mv / R.SCALE, mt, kp3d[v] / R.SCALE))
        pipe.cad_bank = R.CadBank(meshes)
        first = {"frame": sc["frame"], "bboxes": sc["bboxes"], "focals": sc["focals"], "centers": sc["centers"], "cad_idx": np.arange(V),
                 "vehicle_seeds": list(range(V))}
        f0 = pipe.run_frame(first, replay=True)
        state = f0["state"]
        laters = [{"frame": torch.roll(sc["frame"], shifts=37 * (n + 1), dims=1).contiguous(), "steps": [steps[n]] * V,
                   "vehicle_seeds": [1000 * (n + 1) + v for v in range(V)]} for n in range(F)]
        arms = {"frames_replay": lambda: list(pipe.run_later_frames(laters, state, replay=True)),
                "batched_geometry_replay": lambda: pipe.run_later_frames_batched_geometry(laters, state, replay=True)}
        ms = {n: [] for n in GEOMETRY_ARMS}
        host = {n: {"d2h_calls": [], "d2h_wait_ms": [], "issue_ms": []} for n in GEOMETRY_ARMS}
        skipped = None
        for rep in range(args.warmup + args.reps):
            for n in GEOMETRY_ARMS:                               # the arms alternate clip by clip
                torch.cuda.synchronize()
                del waits[:]
                t0 = time.perf_counter()
                out = arms[n]()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    ms[n].append((time.perf_counter() - t0) * 1e3)
                    host[n]["d2h_calls"].append(len(waits))
                    host[n]["d2h_wait_ms"].append(sum(w for _, w in waits) * 1e3)
                    host[n]["issue_ms"].append((waits[0][0] - t0) * 1e3)          # until the first read-back is reached
                skipped = [o["skipped"] for o in out]
        row = {"vehicles": V, "kept_first_frame": int(state["central"].shape[0]), "frames": F, "frame_hw": list(HW), "precision": "f16x3",
               "reps": args.reps, "device_pose": True, "device_homography": True, "replay": True, "skipped_per_frame": skipped}
        for n in GEOMETRY_ARMS:
            med = statistics.median(ms[n])
            row[n] = {"ms_per_clip_tail": med, "ms_per_frame": med / F, "min": min(ms[n]), "max": max(ms[n]),
                      "d2h_calls_per_clip_tail": statistics.median(host[n]["d2h_calls"]),
                      "host_ms_inside_d2h": statistics.median(host[n]["d2h_wait_ms"]),
                      "host_ms_until_first_d2h": statistics.median(host[n]["issue_ms"])}
        row["batched_geometry_replay_over_frames_replay"] = row["batched_geometry_replay"]["ms_per_clip_tail"] / row["frames_replay"]["ms_per_clip_tail"]
        print(json.dumps(row), flush=True)
        table.append(row)
        del laters, sc, state, f0
        pipe._frame_plans.clear()
        torch.cuda.empty_cache()
    ops.d2h = orig
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/later_batch_time.py --geometry", "device": torch.cuda.get_device_name(0), "table": table}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/later_batch_time.json (--geometry: profiles/later_batch_geometry_time.json)")
    ap.add_argument("--geometry", action="store_true", help="time a geometry-mode clip tail: frame by frame against the batched pass")
    ap.add_argument("--vehicles", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--inpaint", type=int, nargs="+", default=None, help="0 / 1; default both (with --arm: 0)")
    ap.add_argument("--seed", type=int, default=4, help="synth_frame's seed of the given-geometry table (seed 3 draws, at 64 vehicles, a "
                    "plane whose host-fitted homography is singular: every arm raises LinAlgError on it)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arm", choices=ARMS, default=None, help="run this arm alone and write nothing (for a profiler)")
    ap.add_argument("--fold", default=None, help="a rocprofv3 kernel_stats.csv of an --arm batched_replay run")
    ap.add_argument("--top", type=int, default=14)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "later_batch_geometry_time.json" if args.geometry else "later_batch_time.json")
    if args.geometry:
        return geometry(args)
    if args.fold:
        args.inpaint = (args.inpaint or [0])[0]
        return fold(args)

    import torch
    from future_urban_scene_generation_amd import ops
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline, synth_frame, synth_later_frame
    if not torch.cuda.is_available():
        raise SystemExit("later_batch_time: needs a HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops.set_precision("f16x3")
    inpaints = [bool(i) for i in (args.inpaint if args.inpaint is not None else ([0] if args.arm else [0, 1]))]
    table = []
    for inp in inpaints:
        pipe = VehiclePipeline(dev, inpaint=inp)
        for V in args.vehicles:
            scene = synth_frame(V, HW, dev, seed=args.seed, inpaint="masks" if inp else False)
            scene["vehicle_seeds"] = list(range(V))
            laters = [synth_later_frame(scene, s, inpaint="box_masks" if inp else None) for s in range(1, F + 1)]
            state = pipe.run_frame(scene, replay=True)["state"]
            arms = {"frames_replay": lambda: list(pipe.run_later_frames(laters, state, replay=True)),
                    "batched_replay": lambda: pipe.run_later_frames_batched(laters, state, replay=True),
                    "batched_eager": lambda: pipe.run_later_frames_batched(laters, state, replay=False)}
            names = [args.arm] if args.arm else list(ARMS)
            ms = {n: [] for n in names}
            for rep in range(args.warmup + args.reps):
                for n in names:                                   # the arms alternate clip by clip
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    arms[n]()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        ms[n].append((time.perf_counter() - t0) * 1e3)
            row = {"vehicles": V, "frames": F, "frame_hw": list(HW), "inpaint": inp, "precision": "f16x3", "reps": args.reps}
            for n in names:
                med = statistics.median(ms[n])
                row[n] = {"ms_per_clip_tail": med, "ms_per_frame": med / F, "min": min(ms[n]), "max": max(ms[n])}
            if not args.arm:
                row["batched_replay_over_frames_replay"] = row["batched_replay"]["ms_per_clip_tail"] / row["frames_replay"]["ms_per_clip_tail"]
            print(json.dumps(row), flush=True)
            table.append(row)
            del laters, scene, state
            pipe._frame_plans.clear()
            torch.cuda.empty_cache()
    if not args.arm:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/later_batch_time.py", "device": torch.cuda.get_device_name(0), "table": table}, f, indent=1)


if __name__ == "__main__":
    main()
