#!/usr/bin/env python3
"""What building EdgeConnect's inputs on the device costs (GPU box) -> profiles/inpaint_inputs_time.json.

For 8 and 64 vehicles on a 720 x 1280 frame (synth_frame(inpaint="masks"): stand-in detector masks):
  stage_ms       ops.inpaint_inputs alone (the pinned upload of the boxes + the five launches) between two HIP events,
                 median of N; stage_host_ms: what the host thread spends issuing it
  frame_ms       run_frames of a pipeline built with inpaint=True (two scenes alternating, one frame in flight), with the four
                 tensors GIVEN (built once, outside the timed loop) and BUILT per frame from the detector masks, the two arms
                 alternating in one process, median over the rounds
--stage-only N: only N calls of the stage at --vehicles (what a kernel trace is taken of)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from future_urban_scene_generation_amd import ops  # noqa: E402
from future_urban_scene_generation_amd.pipeline import VehiclePipeline, synth_frame  # noqa: E402


def scenes(V, dev, seed):
    """(the scene with detector masks, the same scene with the four tensors built from them)."""
    sc = synth_frame(V, (720, 1280), dev, seed=seed, inpaint="masks")
    sc["vehicle_seeds"] = list(range(100 * seed, 100 * seed + V))
    built = ops.inpaint_inputs(sc["frame"], sc["inpaint"]["det_masks"], sc["inpaint"]["boxes"])
    return sc, dict(sc, inpaint=dict(built, boxes=sc["inpaint"]["boxes"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--vehicles", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--stage-only", type=int, default=0)
    ap.add_argument("-o", "--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                        "inpaint_inputs_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    if a.stage_only:
        for V in a.vehicles:
            sc = synth_frame(V, (720, 1280), dev, seed=3, inpaint="masks")
            for _ in range(a.stage_only):
                ops.inpaint_inputs(sc["frame"], sc["inpaint"]["det_masks"], sc["inpaint"]["boxes"])
            torch.cuda.synchronize()
        return
    pipe = VehiclePipeline(dev, inpaint=True)
    res = {"device": torch.cuda.get_device_name(0), "frame": "720x1280", "rounds": a.rounds, "reps": a.reps, "vehicles": {}}
    med = statistics.median
    for V in a.vehicles:
        (m1, g1), (m2, g2) = scenes(V, dev, 3), scenes(V, dev, 4)
        inp = m1["inpaint"]
        for _ in range(3):
            ops.inpaint_inputs(m1["frame"], inp["det_masks"], inp["boxes"])
        torch.cuda.synchronize()
        td, th = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            ops.inpaint_inputs(m1["frame"], inp["det_masks"], inp["boxes"])
            e1.record()
            th.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            td.append(e0.elapsed_time(e1))
        arms = {"given": (g1, g2), "built": (m1, m2)}
        frames = {k: [] for k in arms}
        NF = 12 if V <= 8 else 4
        for pair in arms.values():                                             # warm-up: plans recorded, workspaces made
            for _ in pipe.run_frames([pair[0], pair[1], pair[0]]):
                pass
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, pair in arms.items():
                t0 = time.perf_counter()
                for _ in pipe.run_frames(list(pair) * (NF // 2)):
                    pass
                torch.cuda.synchronize()
                frames[k].append((time.perf_counter() - t0) / NF * 1e3)
        boxes = inp["boxes"]
        res["vehicles"][str(V)] = {
            "max_box_hw": [int((boxes[:, 3] - boxes[:, 1]).max()), int((boxes[:, 2] - boxes[:, 0]).max())],
            "stage_ms": round(med(td), 4), "stage_ms_min_max": [round(min(td), 4), round(max(td), 4)], "stage_host_ms": round(med(th), 4),
            "frames_per_round": NF,
            "frame_ms_given": round(med(frames["given"]), 3), "frame_ms_built": round(med(frames["built"]), 3),
            "frame_ms_given_rounds": [round(x, 3) for x in frames["given"]], "frame_ms_built_rounds": [round(x, 3) for x in frames["built"]]}
        print(V, json.dumps(res["vehicles"][str(V)]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
