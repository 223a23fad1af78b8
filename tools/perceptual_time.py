#!/usr/bin/env python3
"""What the feature-space distances cost on the device, and how far they are from float64 (GPU box)
-> profiles/perceptual_time.json.

Timing: `edgeconnect.loss.feature_distances` on 32 pairs of 256 x 256 crops (64 stacked rows, synthetic VGG weights), medians
of 9 after a warm-up, HIP events around `--inner` back-to-back calls, per call:
  total_ms   the whole call               vgg_ms   the convolutions and pools up to relu5_2 (VGG19.taps on the 64 rows)
  gram_ms    the four ops.gram calls      l1_ms    the nine ops.abs_diff_rows calls (five on taps, four on Gram matrices)
and the Gram kernel alone on the four style-tap shapes at 64 rows: ms, the rate of the matrix work it issues (tile pairs
i0 <= j0 only, padded channels included) and of the full C x C product it stands for, each as a share of the 157.3 TFLOP/s
fp32 matrix peak.
Errors: for every fixture pair (tests/golden/perceptual_*.npz, generated from the reference's own edgeconnect.loss) the relative
error of the device's perceptual and style scalars against the fixture's float64 table, per precision, next to E_ref."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import perceptual_cases as pc  # noqa: E402

from future_urban_scene_generation_amd import ops  # noqa: E402
from future_urban_scene_generation_amd.edgeconnect import loss  # noqa: E402

PEAK_TFLOPS = 157.3


def timed(fn, reps, inner):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return {"ms": statistics.median(out), "min_max": [min(out), max(out)]}


def errors(vgg):
    res = {"E_ref": {}, "device": {}}
    for case in pc.FIXTURES:
        with np.load(os.path.join(REPO, "tests", "golden", f"perceptual_{case}.npz")) as z:
            g = {k: z[k] for k in z.files}
        for kind in pc.PAIRS:
            t64 = g[f"{kind}_table64"]
            want = {"perceptual": t64[:, :5].sum(1).mean(), "style": t64[:, 5:].sum(1).mean()}
            res["E_ref"][f"{case}/{kind}"] = {q: float(g[f"{kind}_E_{q}"]) for q in want}
            x, y = (t.to("cuda:0") for t in pc.image_pair(case, kind))
            for prec in ("f16x3", "f32"):
                with ops.precision(prec):
                    t = loss.feature_distances(vgg, x, y).cpu().numpy()
                got = {"perceptual": t[:, :5].sum(1).mean(), "style": t[:, 5:].sum(1).mean()}
                res["device"].setdefault(prec, {})[f"{case}/{kind}"] = {q: float(abs(got[q] - want[q]) / want[q]) for q in want}
    res["E_ref_max"] = {q: max(v[q] for v in res["E_ref"].values()) for q in ("perceptual", "style")}
    res["device_max"] = {p: {q: max(v[q] for v in d.values()) for q in ("perceptual", "style")} for p, d in res["device"].items()}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("-o", "--out", default=os.path.join(REPO, "profiles", "perceptual_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perceptual_time: needs a HIP device (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    B, R = args.pairs, args.res
    vgg = loss.VGG19().to(dev)
    g = torch.Generator().manual_seed(1)
    x = torch.rand((B, 3, R, R), generator=g).to(dev)
    y = (x + 0.05 * torch.randn((B, 3, R, R), generator=g).to(dev)).clamp(0, 1)
    rows = torch.cat([x, y], 0)
    res = {"device": torch.cuda.get_device_name(0), "pairs": B, "res": R, "reps": args.reps, "inner": args.inner, "precision": ops.PRECISION,
           "peak_tflops": PEAK_TFLOPS}
    with torch.no_grad():
        for _ in range(2):                                        # warm-up: weight upload, code objects, allocator
            table = loss.feature_distances(vgg, x, y)
        with ops.defer_range_check():
            taps = vgg.taps(rows)
            grams = {n: ops.gram(taps[n]) for n in loss.STYLE_TAPS}
            res["total"] = timed(lambda: loss.feature_distances(vgg, x, y), args.reps, args.inner)
            res["vgg"] = timed(lambda: vgg.taps(rows), args.reps, args.inner)
            res["gram"] = timed(lambda: [ops.gram(taps[n]) for n in loss.STYLE_TAPS], args.reps, args.inner)
            res["l1"] = timed(lambda: [ops.abs_diff_rows(taps[n][:B], taps[n][B:]) for n in loss.PERCEPTUAL_TAPS]
                              + [ops.abs_diff_rows(grams[n][:B], grams[n][B:]) for n in loss.STYLE_TAPS], args.reps, args.inner)
            res["gram_alone"] = {}
            for n in loss.STYLE_TAPS:
                t = taps[n]
                rb, c, h, w = t.shape
                tl = (c + 63) // 64
                sub = tl * 3 + tl * (tl - 1) // 2 * 4             # 32 x 32 sub-tiles issued: 3 per diagonal pair, 4 per other
                r = timed(lambda: ops.gram(t), args.reps, args.inner * 4)
                issued, full = 2.0 * rb * h * w * sub * 1024, 2.0 * rb * h * w * c * c
                r.update(shape=[rb, c, h, w], chunk=ops.gram_chunk(c, h * w), tflops_issued=issued / r["ms"] / 1e9,
                         tflops_full_product=full / r["ms"] / 1e9)
                r["share_of_peak_issued"], r["share_of_peak_full_product"] = r["tflops_issued"] / PEAK_TFLOPS, r["tflops_full_product"] / PEAK_TFLOPS
                res["gram_alone"][n] = r
        parts = {k: res[k]["ms"] for k in ("vgg", "gram", "l1")}
        res["dominant"] = max(parts, key=parts.get)
        res["table_mean"] = [float(v) for v in table.mean(0).cpu()]
        res["errors"] = errors(vgg)
    print(json.dumps(res, indent=1, sort_keys=True))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
