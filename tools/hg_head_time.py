"""Sustained time of the fused hourglass head (ops.hg_head: fc, score and join of one stack as one launch) against the sum of
the fusg_conv2d launches it replaces, in both forms (with the join; the last stack's, which stops after score) at the
benchmark's size, and a bit-for-bit check of the two at that size.

    python tools/hg_head_time.py [--batch 32] [--res 64] [--iters 300] [--rounds 3] [--json out.json]

Each arm is timed as `iters` back-to-back launches between two events after 5 warm-up launches; the arms alternate `rounds`
times and every round is reported.  Inputs are seeded; weights are random layers packed as the network packs them."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from future_urban_scene_generation_amd import _lib as L       # noqa: E402
from future_urban_scene_generation_amd import ops, pack       # noqa: E402

DEV = "cuda:0"
C, NC = 256, 12


def plans():
    g = torch.Generator().manual_seed(2024)
    rn = lambda *s: torch.randn(*s, generator=g)              # noqa: E731
    wf, bf = pack.fold_bn_after_conv(rn(C, C, 1, 1) / C ** 0.5, rn(C) * 0.1, 1.0 + 0.1 * rn(C), 0.1 * rn(C))
    w_s, b_s = rn(NC, C, 1, 1) / C ** 0.5, rn(NC) * 0.1
    ws32, bs32 = torch.zeros(32, C, 1, 1), torch.zeros(32)
    ws32[:NC], bs32[:NC] = w_s, b_s
    return (pack.pack_conv(wf, bf), pack.pack_conv(ws32, bs32), pack.pack_conv(w_s, b_s),
            pack.pack_conv(rn(C, C + NC, 1, 1) / (C + NC) ** 0.5, rn(C) * 0.1, c_split=(C, NC), cin_pad=32))


def unfused(P, y_in, x, join):
    fc, s32, s12, jn = P
    y = ops.conv(fc, y_in, act=L.ACT_RELU)
    if not join:
        return ops.conv(s12, y), None
    s = ops.conv(s32, y)
    return s, ops.conv(jn, y, s[:, :NC], res0=x)


def fused(P, y_in, x, join):
    fc, s32, s12, jn = P
    return ops.hg_head(fc, s32, y_in, jn, x) if join else ops.hg_head(fc, s12, y_in)


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
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    P = plans()
    rows = []
    with torch.no_grad():
        g = torch.Generator().manual_seed(a.res)
        y_in, x = (ops.as_nhwc(torch.randn(a.batch, C, a.res, a.res, generator=g).to(DEV)) for _ in range(2))
        for join in (True, False):
            assert ops.hg_head_ok(P[0], P[1] if join else P[2], y_in, P[3] if join else None, x if join else None)
            want, got = unfused(P, y_in, x, join), fused(P, y_in, x, join)
            equal = all(torch.equal(p, q) for p, q in zip(got, want) if p is not None)
            hit = ops.range_exceeded(DEV)
            del want, got
            t = {"unfused": [], "fused": []}
            for _ in range(a.rounds):
                t["unfused"].append(round(timed(lambda: unfused(P, y_in, x, join), a.iters), 4))
                t["fused"].append(round(timed(lambda: fused(P, y_in, x, join), a.iters), 4))
            row = {"form": "join" if join else "last", "batch": a.batch, "res": a.res, "launches_replaced": 3 if join else 2,
                   "unfused_ms": t["unfused"], "fused_ms": t["fused"], "bit_equal": equal, "range_status": hit}
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0 if all(r["bit_equal"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
