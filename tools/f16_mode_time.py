#!/usr/bin/env python3
"""GPU box: what the single-pass fp16 mode ("f16") costs and buys on the crop pass of bench.py - B = 32 crops at 256 x 256 through
hourglass -> ICN -> VUnet, bench.py's warm-up and step counts (15 / 30), its batch, seeds and issue mode (check="async").

The three arms f16x3 / bf16 / f16 run in ONE process and alternate (round r measures the arms in an order rotated by r), so that a
drift of the card's clock falls on all of them; 9 measurements per arm, median and range.  Then compare_precisions of f16 and of
bf16 against f16x3 on the same batch: worst SSIM, PSNR and largest uint8 difference of each image output.

usage: tools/f16_mode_time.py [--out profiles/f16_mode_time.json] [--rounds 9] [--steps 30] [--warmup 15]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ARMS = ("f16x3", "bf16", "f16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "f16_mode_time.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--settle-s", type=float, default=0.6)
    a = ap.parse_args()
    import numpy as np
    import torch
    from future_urban_scene_generation_amd import ops
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline, synth_batch
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    pipe = VehiclePipeline(dev)
    batch = synth_batch(a.batch, a.res, dev, seed=0, nhwc=True)
    seeds = [1000 + i for i in range(a.batch)]

    def step():
        return pipe.run(batch, vehicle_seeds=seeds, check="async")

    before = ops.PRECISION
    for arm in ARMS:                                               # lazy initialisation and the clock settle, once per arm
        ops.set_precision(arm)
        step()
        torch.cuda.synchronize()
        t_s = time.perf_counter()
        while time.perf_counter() - t_s < a.settle_s:
            step()
            torch.cuda.synchronize()
    ms = {arm: [] for arm in ARMS}
    flagged = {arm: 0 for arm in ARMS}
    for r in range(a.rounds):
        for k in range(len(ARMS)):
            arm = ARMS[(r + k) % len(ARMS)]
            ops.set_precision(arm)
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            pipe.finish()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            ms[arm].append((time.perf_counter() - t0) * 1e3 / a.steps)
            flagged[arm] += int(bool(pipe.finish()))
    ops.set_precision(before)
    res = {"what": "crop pass of bench.py (hourglass -> ICN -> VUnet), one process, arms alternating", "batch": a.batch, "res": a.res,
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "arms": {}}
    for arm in ARMS:
        v = ms[arm]
        med = statistics.median(v)
        res["arms"][arm] = {"ms_per_step_median": med, "ms_per_step_min": min(v), "ms_per_step_max": max(v), "ms_per_step": v,
                            "crops_per_s_median": a.batch / med * 1e3, "range_guard_fired": flagged[arm]}
    m = {arm: res["arms"][arm]["ms_per_step_median"] for arm in ARMS}
    res["f16_over_f16x3"] = m["f16"] / m["f16x3"]
    res["f16_over_bf16"] = m["f16"] / m["bf16"]
    res["accepted_f16_median_below_f16x3_median"] = bool(m["f16"] < m["f16x3"])
    res["quality_vs_f16x3"] = {}
    for arm in ("bf16", "f16"):
        rep = pipe.compare_precisions(batch, seeds, arm)
        q = {"kp_equal_min_of_12": int(np.min(rep["kp_equal"]))}
        for k in ("icn_u8", "vunet_u8"):
            q[k] = {"ssim_min": float(np.min(rep[k]["ssim"])), "psnr_min_db": float(np.min(rep[k]["psnr"])),
                    "max_abs_u8": int(np.max(rep[k]["max_abs"]))}
        res["quality_vs_f16x3"][arm] = q
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    brief = {k: res[k] for k in ("f16_over_f16x3", "f16_over_bf16", "accepted_f16_median_below_f16x3_median", "quality_vs_f16x3")}
    brief["ms_median"] = m
    print(json.dumps(brief))
    return 0


if __name__ == "__main__":
    sys.exit(main())
