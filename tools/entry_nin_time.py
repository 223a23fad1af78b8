"""Sustained time of the VUnet's entry NiN computed inside residual_0 (ops.entry_nin) against the two fusg_conv2d launches it
replaces - the 6 -> 128 pointwise NiN and the 128 -> 128 3x3 ELU Residual of app_encoder_1 - at the benchmark's size, and a
bit-for-bit check of the two at that size.

    python tools/entry_nin_time.py [--batch 32] [--res 256] [--iters 100] [--json out.json]

Each arm is timed as `iters` back-to-back launches between two events after 5 warm-up launches, into preallocated outputs
(sustained clocks: the arms alternate three times, every round is printed).  Inputs are seeded; weights are random layers."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from future_urban_scene_generation_amd import _lib as L       # noqa: E402
from future_urban_scene_generation_amd import ops, pack       # noqa: E402

DEV = "cuda:0"


def plans(cin=6, c=128):
    g = torch.Generator().manual_seed(1313)
    return (pack.pack_conv(torch.randn(c, cin, 1, 1, generator=g) / cin ** 0.5, torch.randn(c, generator=g) * 0.1),
            pack.pack_conv(torch.randn(c, c, 3, 3, generator=g) / (3.0 * c ** 0.5), torch.randn(c, generator=g) * 0.1, pad=1))


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    nin, res = plans()
    with torch.no_grad():
        g = torch.Generator().manual_seed(a.res)
        u = ops.as_nhwc(torch.randn(a.batch, 6, a.res, a.res, generator=g).to(DEV))
        form = ops.entry_nin_form(nin, res, u)
        if form == 0:
            print("this shape does not fuse (ops.entry_nin_form == 0)")
            return 1
        x0 = ops.nhwc_empty(a.batch, 128, a.res, a.res, DEV)
        s_two, s_one = (ops.nhwc_empty(a.batch, 128, a.res, a.res, DEV) for _ in range(2))

        def two():
            ops.conv(nin, u, pre_op=L.PRE_ELU, out=x0)
            ops.conv(res, x0, pre_op=L.PRE_ELU, res0=x0, out=s_two)

        def one():
            ops.entry_nin(nin, res, u, out=s_one)

        two()
        one()
        equal = torch.equal(s_two, s_one)
        hit = ops.range_exceeded(DEV)
        rounds = []
        for rnd in range(3):
            t_nin = timed(lambda: ops.conv(nin, u, pre_op=L.PRE_ELU, out=x0), a.iters)
            t_res = timed(lambda: ops.conv(res, x0, pre_op=L.PRE_ELU, res0=x0, out=s_two), a.iters)
            t_two = timed(two, a.iters)
            t_one = timed(one, a.iters)
            rounds.append({"round": rnd, "nin_ms": round(t_nin, 4), "residual_ms": round(t_res, 4), "two_launches_ms": round(t_two, 4),
                           "fused_ms": round(t_one, 4)})
            print(json.dumps(rounds[-1]), flush=True)
        row = {"batch": a.batch, "res": a.res, "form": {1: "m_split_128", 2: "k_split_32"}[form], "bit_equal": equal, "range_status": hit,
               "rounds": rounds}
        print(json.dumps({k: v for k, v in row.items() if k != "rounds"}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
