#!/usr/bin/env python3
"""Geometry-mode frame timing (GPU box): ms per frame on a 720 x 1280 frame at 8 and 64 vehicles for run_frame eager,
run_frame replayed and run_frames pipelined (one frame in flight), with the given-geometry run_frames figure at 8 vehicles
beside them.  Synthetic weights; the CAD bank is built around well-posed keypoints of the first hourglass run (as
tools/render_time.py).  Prints JSON; --out writes it too."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle  # noqa: E402
import render_ref as RR  # noqa: E402
from future_urban_scene_generation_amd import ops  # noqa: E402
from future_urban_scene_generation_amd import render as R  # noqa: E402
from future_urban_scene_generation_amd.pipeline import VehiclePipeline, synth_frame  # noqa: E402

dev = torch.device("cuda:0")
torch.set_grad_enabled(False)
ops.set_precision("f16x3")
H, W = 720, 1280
N = 8


def timed(fn, n=N):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / n * 1e3, 3)


def timed_frames(pipe, scenes, replay):
    list(pipe.run_frames(scenes[:2], replay=replay))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in pipe.run_frames(scenes, replay=replay):
        pass
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / len(scenes) * 1e3, 3)


res = {"frame_hw": [H, W], "precision": "f16x3", "frames_timed": N}
pipe = VehiclePipeline(dev)
for V in (8, 64):
    sc = synth_frame(V, (H, W), dev, seed=3)
    kp = pipe.run_frame(sc)["kp_xy"].cpu().numpy()
    kp3d = oracle.frame.well_posed_kp3d(kp, sc["focals"], sc["centers"], seed=2)
    meshes = []
    for v in range(V):
        mv, mt = RR.box_around(kp3d[v], n=13)
        meshes.append((mv / R.SCALE, mt, kp3d[v] / R.SCALE))
    pipe.cad_bank = R.CadBank(meshes)
    g = {"frame": sc["frame"], "bboxes": sc["bboxes"], "focals": sc["focals"], "centers": sc["centers"], "cad_idx": np.arange(V),
         "vehicle_seeds": list(range(V))}
    res[f"skipped_{V}veh"] = pipe.run_frame(g)["skipped"]
    res[f"geometry_run_frame_eager_ms_{V}veh"] = timed(lambda: pipe.run_frame(g))
    res[f"geometry_run_frame_replay_ms_{V}veh"] = timed(lambda: pipe.run_frame(g, replay=True))
    res[f"geometry_run_frames_pipelined_ms_{V}veh"] = timed_frames(pipe, [g] * N, True)
    if V == 8:
        pipe.cad_bank = None
        res["given_geometry_run_frames_ms_8veh"] = timed_frames(pipe, [sc] * N, True)
    pipe._frame_plans.clear()
    torch.cuda.empty_cache()
print(json.dumps(res))
if len(sys.argv) > 2 and sys.argv[1] == "--out":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(res, f, indent=1)
