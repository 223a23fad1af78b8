#!/usr/bin/env python3
"""What selecting the pose and deriving its geometry on the device is worth (GPU box) -> profiles/pose_geometry_time.json.

Geometry mode (a CAD bank of boxes around well-posed keypoints, as the tests build it) for 8 and 64 vehicles on a 720 x 1280
frame, VehiclePipeline.device_pose off and on alternating in one process and one build (off is the unchanged numpy path):
  front_ms   the geometry front stage alone (`_geometry_front`: keypoints, pose fit, geometry, render, visibility, cut-outs),
             wall time of the host thread from an idle GPU to an idle GPU, median of the repetitions
  frame_ms   run_frames over a few frames (two scenes alternating, one frame in flight, replay), per frame, median over rounds
and the ratio on / off of each.  There is no bar: the flag stays opt-in whatever comes out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle  # noqa: E402
import oracle.frame  # noqa: E402
from future_urban_scene_generation_amd import ops  # noqa: E402
from future_urban_scene_generation_amd import render as R  # noqa: E402
from future_urban_scene_generation_amd.pipeline import VehiclePipeline, load_schema, synth_frame  # noqa: E402
from future_urban_scene_generation_amd.synth import synth_state_dict  # noqa: E402


def setup(V, dev, sds, seed):
    """A geometry-mode scene of V vehicles and its bank: per vehicle a box mesh around keypoints that fit the hourglass's."""
    import render_ref as RR
    sc = synth_frame(V, (720, 1280), dev, seed=seed)
    cpu = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in sc.items()}
    kp = oracle.frame.frame_keypoints(sds, cpu)
    kp3d = oracle.frame.well_posed_kp3d(kp, sc["focals"], sc["centers"], seed=2)
    meshes = []
    for v in range(V):
        mv, mt = RR.box_around(kp3d[v], n=12)
        meshes.append((mv / R.SCALE, mt, kp3d[v] / R.SCALE))
    scene = {"frame": sc["frame"], "bboxes": sc["bboxes"], "focals": sc["focals"], "centers": sc["centers"],
             "vehicle_seeds": list(range(V))}
    return meshes, scene


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--vehicles", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "pose_geometry_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops.set_precision("f16x3")
    sds = {n: synth_state_dict(n, load_schema(n), 0) for n in ("hg", "icn", "vunet")}
    res = {"device": torch.cuda.get_device_name(0), "frame": "720x1280", "rounds": a.rounds, "reps": a.reps, "vehicles": {}}
    med = statistics.median
    for V in a.vehicles:
        m1, s1 = setup(V, dev, sds, 3)
        m2, s2 = setup(V, dev, sds, 4)
        bank = R.CadBank(m1 + m2)                                            # one bank for both scenes
        s1["cad_idx"], s2["cad_idx"] = np.arange(V), np.arange(V, 2 * V)
        pipe = VehiclePipeline(dev, state_dicts=sds, cad_bank=bank)
        NF = 6 if V <= 8 else 4
        for flag in (False, True):                                           # warm-up: plans recorded, workspaces made
            pipe.device_pose = flag
            for _ in pipe.run_frames([s1, s2, s1]):
                pass
        torch.cuda.synchronize()
        front, frames = {False: [], True: []}, {False: [], True: []}
        for _ in range(a.reps):
            for flag in (False, True):
                pipe.device_pose = flag
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.cuda.device(dev):
                    f = pipe._geometry_front(s1, None)
                torch.cuda.synchronize()
                front[flag].append((time.perf_counter() - t0) * 1e3)
        kept = len(f["keep"])
        for _ in range(a.rounds):
            for flag in (False, True):
                pipe.device_pose = flag
                t0 = time.perf_counter()
                for _ in pipe.run_frames([s1, s2] * (NF // 2)):
                    pass
                torch.cuda.synchronize()
                frames[flag].append((time.perf_counter() - t0) / NF * 1e3)
        pipe.device_pose = False
        r = {"rendered_vehicles": kept, "frames_per_round": NF,
             "front_ms_off": round(med(front[False]), 3), "front_ms_on": round(med(front[True]), 3),
             "frame_ms_off": round(med(frames[False]), 3), "frame_ms_on": round(med(frames[True]), 3),
             "front_ms_off_reps": [round(x, 3) for x in front[False]], "front_ms_on_reps": [round(x, 3) for x in front[True]],
             "frame_ms_off_rounds": [round(x, 3) for x in frames[False]], "frame_ms_on_rounds": [round(x, 3) for x in frames[True]]}
        r["front_ratio_on_off"] = round(r["front_ms_on"] / r["front_ms_off"], 4)
        r["frame_ratio_on_off"] = round(r["frame_ms_on"] / r["frame_ms_off"], 4)
        res["vehicles"][str(V)] = r
        print(V, json.dumps(r), flush=True)
        del pipe
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
