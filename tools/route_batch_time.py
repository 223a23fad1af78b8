#!/usr/bin/env python3
"""GPU box, analysis tool: what a routing batch costs (ops.route_batch; DESIGN.md, batch-invariant routing).  `pipe.run`'s
crop pass (hourglass + ICN + VUnet, 256 x 256, f16x3) as a recorded plan at B = 1, 8, 32, once per arm
route_batch = off, 1, 8, 32.  The arms alternate window by window in one process after a warm-up of all of them; a window is
--passes replays ending in a device synchronise (100 / 30 / 10 passes at B = 1 / 8 / 32: about 0.2 s); the medians of --reps
(default 9) windows go to --out (default profiles/route_batch_time.json) with the device's name and the date.  Every arm also
reports the sequence of conv kernel families (fusg_last_conv_kernel) of one eager pass, as a count and a digest.

--parent-tree DIR: a built checkout of the parent commit.  The `off` arm is then also timed there, in child processes that
alternate with child processes on this tree (two each), and the kernel-family sequences of the two trees are compared: the
off arm runs the parent's launches, so a gap between the two is measurement spread and is reported as such.

    python tools/route_batch_time.py
    python tools/route_batch_time.py --parent-tree ../parent --batches 1 8"""
import argparse
import datetime
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = {1: 100, 8: 30, 32: 10}
ARMS = ("off", "1", "8", "32")


def _routed(ops, arm):
    """The context of an arm; `off` touches nothing (it is also what runs on a tree without the switch)."""
    import contextlib
    return contextlib.nullcontext() if arm == "off" else ops.route_batch(int(arm))


def measure(tree, batches, arms, reps, warmup):
    """The table of one tree, in this process."""
    sys.path.insert(0, tree)
    import torch
    from future_urban_scene_generation_amd import ops
    from future_urban_scene_generation_amd import pipeline as pl
    if not torch.cuda.is_available():
        raise SystemExit("route_batch_time: needs a HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ops.set_precision("f16x3")
    pipe = pl.VehiclePipeline(dev)
    families = []
    launchers = ("conv", "bottleneck", "respair", "entry_nin")
    orig = {n: getattr(ops, n) for n in launchers}

    def noting(fn):
        def call(*a, **k):
            out = fn(*a, **k)
            families.append(ops.last_conv_kernel())
            return out
        return call

    table = []
    for B in batches:
        batch = pl.synth_batch(B, 256, dev, seed=B)
        seeds = [100 * B + v for v in range(B)]
        plans, seqs = {}, {}
        for arm in arms:
            with _routed(ops, arm):
                for n in launchers:                                   # one eager pass: which kernel families it launches
                    setattr(ops, n, noting(orig[n]))
                try:
                    del families[:]
                    pipe.run(batch, seeds)
                    seqs[arm] = list(families)
                finally:
                    for n in launchers:
                        setattr(ops, n, orig[n])
                plans[arm] = pipe.compile(batch, seeds)
        ms = {arm: [] for arm in arms}
        for rep in range(warmup + reps):
            for arm in arms:                                          # the arms alternate window by window
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(PASSES[B]):
                    plans[arm].run(batch, seeds, check="async")
                torch.cuda.synchronize()
                if rep >= warmup:
                    ms[arm].append((time.perf_counter() - t0) * 1e3 / PASSES[B])
        assert not pipe.finish(), "a pass left the split-fp16 range"
        row = {"batch": B, "precision": "f16x3", "replay": True, "passes_per_window": PASSES[B], "reps": reps, "arms": {}}
        for arm in arms:
            med = statistics.median(ms[arm])
            row["arms"][arm] = {"ms_per_pass": med, "min": min(ms[arm]), "max": max(ms[arm]), "crops_per_s": 1e3 * B / med,
                                "conv_launches": len(seqs[arm]),
                                "family_sequence_sha1": hashlib.sha1(",".join(map(str, seqs[arm])).encode()).hexdigest(),
                                "recorded_operations": plans[arm].size}
            if arm != "off" and "off" in ms:
                row["arms"][arm]["over_off"] = med / statistics.median(ms["off"])
        print(json.dumps(row), flush=True)
        table.append(row)
        del plans
        torch.cuda.empty_cache()
    return {"device": torch.cuda.get_device_name(0), "table": table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "route_batch_time.json"))
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8, 32], choices=sorted(PASSES))
    ap.add_argument("--arms", nargs="+", default=list(ARMS), choices=ARMS)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: time its `off` arm as well")
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:                                                    # one tree's table as JSON on the last line
        print("CHILD " + json.dumps(measure(os.path.abspath(args.tree), args.batches, args.arms, args.reps, args.warmup)), flush=True)
        return
    result = {"tool": "tools/route_batch_time.py", "date": datetime.date.today().isoformat()}
    result.update(measure(HERE, args.batches, args.arms, args.reps, args.warmup))
    if args.parent_tree:
        # fresh processes, this tree and the parent's in turn (a library is loaded once per process)
        runs = {"parent": [], "this": []}
        for _ in range(2):
            for name, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", HERE)):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--arms", "off", "--reps", str(args.reps),
                       "--warmup", str(args.warmup), "--batches"] + [str(b) for b in args.batches]
                env = dict(os.environ)
                env.pop("FUSG_LIB", None)
                env.pop("FUSG_ROUTE_BATCH", None)
                out = subprocess.run(cmd, check=True, capture_output=True, text=True, env=env, cwd=tree).stdout
                runs[name].append(json.loads([ln for ln in out.splitlines() if ln.startswith("CHILD ")][-1][6:])["table"])
        rows = []
        for i, B in enumerate(args.batches):
            p = [r[i]["arms"]["off"] for r in runs["parent"]]
            t = [r[i]["arms"]["off"] for r in runs["this"]]
            same = len({a["family_sequence_sha1"] for a in p + t}) == 1
            rows.append({"batch": B, "parent_ms_per_pass": [a["ms_per_pass"] for a in p], "this_ms_per_pass": [a["ms_per_pass"] for a in t],
                         "this_over_parent": statistics.mean(a["ms_per_pass"] for a in t) / statistics.mean(a["ms_per_pass"] for a in p),
                         "conv_launches": t[0]["conv_launches"], "same_kernel_family_sequence": same,
                         "recorded_operations": [p[0]["recorded_operations"], t[0]["recorded_operations"]]})
            print(json.dumps(rows[-1]), flush=True)
        result["off_arm_against_parent"] = {"protocol": "child processes, parent tree and this tree in turn, two each; arm off",
                                            "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
