#!/usr/bin/env python3
"""GPU box, analysis tool: the clip tails of a video (every clip 1 + F frames, F = 5 future frames, 720 x 1280, f16x3) clip by clip
(`run_later_frames_batched(replay=True)` per clip: the best the parent commit has for this input) against
`run_later_clips_batched(replay=True)`, which packs whole clips into passes of up to 64 rows.  Three videos: 16 clips x 2 vehicles,
8 clips x 8 vehicles, and a ragged mix of 20 clips with 0-5 vehicles, some with fewer than 5 future frames.  The arms alternate
video by video in one process after a warm-up of every arm, each arm on a pipeline (and so a plan cache) of its own; each video
ends in a device synchronise.  Per arm it records the medians, the network passes per video and the plan recordings per video (a
video whose (F, V) mix exceeds the plan cache re-records plans in the per-clip arm).  The table goes to --out (default profiles/clips_batch_time.json).

    python tools/clips_batch_time.py
    python tools/clips_batch_time.py --videos 16x2 --reps 3"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

F, HW = 5, (720, 1280)
BASE_VEHICLES = 8
ARMS = ("per_clip_replay", "clips_replay")
# (frames, vehicles) per clip
VIDEOS = {
    "16x2": [(F, 2)] * 16,
    "8x8": [(F, 8)] * 8,
    "ragged20": [(5, 1), (5, 2), (3, 1), (5, 0), (5, 3), (5, 1), (2, 2), (5, 5), (5, 1), (4, 2), (5, 2), (5, 0), (5, 1), (1, 4), (5, 2),
                 (5, 1), (3, 3), (5, 2), (5, 1), (5, 4)],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clips_batch_time.json"))
    ap.add_argument("--videos", nargs="+", default=list(VIDEOS), choices=list(VIDEOS))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch
    from future_urban_scene_generation_amd import ops
    from future_urban_scene_generation_amd import pipeline as pl
    if not torch.cuda.is_available():
        raise SystemExit("clips_batch_time: needs a HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops.set_precision("f16x3")

    def counted(pipe):
        """The pipeline with its network passes and plan recordings counted."""
        count = {"passes": 0, "recordings": 0}
        nets, replay = pipe._later_nets, pipe._replay
        pipe._later_nets = lambda *a, **k: (count.__setitem__("passes", count["passes"] + 1), nets(*a, **k))[1]

        def counted_replay(key, *a, **k):
            count["passes"] += 1
            count["recordings"] += pipe._plan(key) is None
            before = count["passes"]
            out = replay(key, *a, **k)
            count["passes"] = before                              # (a recording runs the pass function once: still one pass)
            return out

        pipe._replay = counted_replay
        return count

    # a pipeline per arm (the same synthetic weights): each arm keeps its own plan cache, as a video run through one driver would
    pipes = {n: pl.VehiclePipeline(dev) for n in ARMS}
    counts = {n: counted(pipes[n]) for n in ARMS}
    pipe = pipes[ARMS[0]]
    # the scene tools/later_batch_time.py times (synth_frame seed 3, 8 vehicles, its five later poses: every plane fit is well-posed);
    # a clip is a run of its vehicles
    base = pl.synth_frame(BASE_VEHICLES, HW, dev, seed=3)
    moved = [pl.synth_later_frame(base, s) for s in range(1, F + 1)]
    table = []
    for name in args.videos:
        shape = VIDEOS[name]
        clips = []
        for c, (Fc, V) in enumerate(shape):
            n, lo = max(V, 1), c % (BASE_VEHICLES - max(V, 1) + 1)
            scene = pl.slice_scene(base, lo, lo + n)             # its own vehicles, image, planes and seeds per clip
            scene.update(frame=torch.roll(base["frame"], shifts=53 * (c + 1), dims=1).contiguous(), src_planes=scene["src_planes"].clone(),
                         vehicle_seeds=[100 * c + v for v in range(n)])
            state = pipe.run_frame(scene, replay=True)["state"]
            later = [dict(pl.slice_scene(moved[s], lo, lo + n), frame=torch.roll(scene["frame"], shifts=37 * (s + 1), dims=1).contiguous(),
                          src_planes=scene["src_planes"], vehicle_seeds=[100 * c + 10 * (s + 1) + v for v in range(n)]) for s in range(Fc)]
            if V == 0:                                            # a selected frame without vehicles: the scenes and the state cut to none
                later = [pl.slice_scene(sc, 0, 0) for sc in later]
                state = {"appearance": [t[:0] for t in state["appearance"]], "central": state["central"][:0], "shard": (0, 0, 0),
                         "sharded": False}
            clips.append((later, state))
        arms = {"per_clip_replay": lambda: [pipes["per_clip_replay"].run_later_frames_batched(scs, st, replay=True) for scs, st in clips],
                "clips_replay": lambda: pipes["clips_replay"].run_later_clips_batched(clips, replay=True)}
        ms = {n: [] for n in ARMS}
        seen = {n: {"passes": [], "recordings": []} for n in ARMS}
        for rep in range(args.warmup + args.reps):
            for n in ARMS:                                        # the arms alternate video by video
                torch.cuda.synchronize()
                count = counts[n]
                count["passes"] = count["recordings"] = 0
                t0 = time.perf_counter()
                arms[n]()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    ms[n].append((time.perf_counter() - t0) * 1e3)
                    seen[n]["passes"].append(count["passes"])
                    seen[n]["recordings"].append(count["recordings"])
        tails = sum(1 for Fc, _ in shape if Fc)
        rows = sum(Fc * V for Fc, V in shape)
        row = {"video": name, "clips": len(shape), "clip_shapes_frames_vehicles": [list(s) for s in shape], "rows": rows, "frame_hw": list(HW),
               "precision": "f16x3", "reps": args.reps, "warmup": args.warmup, "plan_cache": pl.FRAME_PLANS,
               "groups": [[lo, hi, big] for lo, hi, big in pl.clip_batch_groups([s[0] for s in shape], [s[1] for s in shape])]}
        for n in ARMS:
            med = statistics.median(ms[n])
            row[n] = {"ms_per_video": med, "ms_per_clip_tail": med / tails, "ms_per_row": med / rows, "min": min(ms[n]), "max": max(ms[n]),
                      "passes_per_video": statistics.median(seen[n]["passes"]),
                      "plan_recordings_per_video": statistics.median(seen[n]["recordings"])}
        row["clips_replay_over_per_clip_replay"] = row["clips_replay"]["ms_per_video"] / row["per_clip_replay"]["ms_per_video"]
        print(json.dumps(row), flush=True)
        table.append(row)
        del clips
        for p in pipes.values():
            p._frame_plans.clear()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/clips_batch_time.py", "device": torch.cuda.get_device_name(0), "table": table}, f, indent=1)


if __name__ == "__main__":
    main()
