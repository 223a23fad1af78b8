#!/usr/bin/env python3
"""GPU box: time of the uint8 glue entries whose kernels a refactor of csrc/cvops.hip re-shaped, on this tree or (`--repo`) on a
built checkout of another commit -> one JSON per run; `--join` folds the runs of two commits into a verdict per entry
-> profiles/glue_kernels_time.json.

Frames of 720 x 1280.  The one-frame entries (`fill_planes_batch`, `crop_resize` in modes 0 and 1) take 8 and 64 rows of one
frame; the several-frame entries (`crop_resize_frames`, `vunet_inputs_frames`, `paste_back_frames_device`,
`paste_back_ragged_device`) take 8 frames x 1 row and 8 frames x 8 rows.  Per entry: HIP events around `--inner` (20) back-to-back
calls of the public wrapper, per call, the median of `--reps` (9) after a warm-up.  Public wrappers only, like
tools/glue_digest.py.

    python tools/glue_kernels_time.py --out tree_1.json
    python tools/glue_kernels_time.py --repo PARENT_CHECKOUT --out parent_1.json
    python tools/glue_kernels_time.py --join parent=parent_1.json,parent_2.json tree=tree_1.json,tree_2.json --out profiles/glue_kernels_time.json

Run the arms alternating (parent, tree, parent, tree), each in a process of its own.  The yardstick is the parent's own
run-to-run difference: a tree median above the parent's slower run by more than that difference is a regression."""
import argparse
import json
import os
import statistics
import sys

HW, R = (720, 1280), 256


def join(args):
    runs = {a.split("=", 1)[0]: [json.load(open(p)) for p in a.split("=", 1)[1].split(",")] for a in args.join}
    parent, tree = runs["parent"], runs["tree"]
    entries = {}
    for k in parent[0]["ms"]:
        p, t = [r["ms"][k] for r in parent], [r["ms"][k] for r in tree]
        spread = max(p) - min(p)
        bound = max(p) + spread
        entries[k] = {"parent_ms": p, "tree_ms": t, "parent_run_to_run_ms": spread, "bound_ms": bound,
                      "tree_over_bound_ms": [max(0.0, x - bound) for x in t], "verdict": "regression" if max(t) > bound else "ok"}
    res = {"what": __doc__.split("\n\n")[1].replace("\n", " "), "device": tree[0]["device"], "reps": tree[0]["reps"], "inner": tree[0]["inner"],
           "yardstick": "per entry the parent's own run-to-run difference: a tree median above the parent's slower run by more than "
                        "that difference is a regression",
           "regressions": sorted(k for k, e in entries.items() if e["verdict"] != "ok"), "entries": entries}
    if args.stats:
        # rocprofv3 --kernel-trace --stats of one run per arm (the same calls in the same order): device time per glue kernel
        import csv
        trace = {}
        for a in args.stats:
            arm, path = a.split("=", 1)
            for row in csv.DictReader(open(path)):
                name = row["Name"].split("(")[0].replace("fusg::", "")
                if any(s in name for s in ("fill_poly_planes", "crop_resize", "vunet_inputs", "paste_")):
                    trace.setdefault(name, {})[arm] = {"calls": int(row["Calls"]), "total_us": int(row["TotalDurationNs"]) / 1e3,
                                                       "mean_us": float(row["AverageNs"]) / 1e3}
        res["kernel_trace"] = {"what": "rocprofv3 --kernel-trace --stats, one run of each arm alone with --reps 3", "kernels": trace}
    if args.note:
        res["note"] = args.note
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k, e in entries.items():
        print(f"{k:48s} parent {e['parent_ms'][0]:.4f} {e['parent_ms'][1]:.4f}  tree {e['tree_ms'][0]:.4f} {e['tree_ms'][1]:.4f}  {e['verdict']}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the built checkout to import")
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--join", nargs="+", metavar="ARM=FILE,FILE", help="no GPU: parent=... tree=... -> the verdict per entry")
    ap.add_argument("--stats", nargs="+", metavar="ARM=KERNEL_STATS_CSV", help="with --join: add each arm's device time per glue kernel")
    ap.add_argument("--note", help="with --join: a remark kept in the file, e.g. what the kernel trace says about a flagged entry")
    args = ap.parse_args()
    if args.join:
        return join(args)
    sys.path.insert(0, args.repo)
    import numpy as np
    import torch

    from future_urban_scene_generation_amd import frame_ops as fo
    from future_urban_scene_generation_amd.warp_learn import planes_utils as pu
    if not torch.cuda.is_available():
        sys.exit("glue_kernels_time: needs a HIP device")
    print("glue_kernels_time: the wrappers of", os.path.abspath(pu.__file__), flush=True)
    dev = torch.device("cuda:0")
    H, W = HW
    g = np.random.default_rng(7)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                          # noqa: E731
    frames = [d(g.integers(0, 256, (H, W, 3), dtype=np.uint8)) for _ in range(8)]
    ms = {}

    def timed(name, fn):
        for _ in range(3):
            fn()
        t = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / args.inner)
        ms[name] = statistics.median(t)
        print(f"{name:48s} {ms[name]:.4f} ms", flush=True)

    def rows(N):
        """N vehicles: detector-sized boxes spread over the frame, their crop rows, masks, sketches, crops and polygons."""
        boxes = [[int(x0), int(y0), int(x0 + g.integers(120, 360)), int(y0 + g.integers(90, 260))]
                 for x0, y0 in zip(g.integers(-20, W - 200, N), g.integers(-20, H - 150, N))]
        geom = d(np.asarray([pu._geom_row(*pu.square_crop_geometry(HW, bb)) for bb in boxes], np.int32))
        masks, rects = np.zeros((N, H, W), np.uint8), np.zeros((N, 8), np.int32)
        pts, nv = np.zeros((N, 5, 8, 2), np.int32), np.full((N, 5), 4, np.int32)
        for r, (x0, y0, x1, y1) in enumerate(boxes):
            masks[r, max(0, y0):y1, max(0, x0):x1] = 1
            rects[r, :4] = [max(0, x0 - 20), max(0, y0 - 10), min(W - 1, x1 + 20), min(H - 1, y1 + 10)]
            for p in range(5):
                ax, ay = x0 + (x1 - x0) * p // 6, y0 + (y1 - y0) * p // 8
                pts[r, p, :4] = [(ax, ay), (ax + (x1 - x0) // 2, ay + 5), (ax + (x1 - x0) // 2 - 9, ay + (y1 - y0) // 2), (ax + 4, ay + (y1 - y0) // 2)]
        u8 = lambda *sh: d(g.integers(0, 256, sh, dtype=np.uint8))                           # noqa: E731
        return dict(geom=geom, masks=d(masks), rects=d(rects), pts=d(pts), nv=d(nv), ssk=u8(N, H, W, 3), dsk=u8(N, H, W, 3),
                    nets=u8(N, R, R, 3), box=u8(N, R, R, 3))

    for N in (8, 64):                                                                        # one frame, N rows
        c = rows(N)
        planes = torch.empty((N, 5, H, W, 3), dtype=torch.uint8, device=dev)
        timed(f"fill_planes_batch/rows_{N}", lambda: pu.fill_planes_batch(frames[0], c["pts"], c["nv"], planes))
        del planes
        for mode, kw in ((0, {}), (1, dict(mean=fo.IMAGENET_MEAN, std=fo.IMAGENET_STD))):
            out = None if mode == 0 else fo.crop_resize(frames[0], c["geom"], (R, R), mode, **kw)
            timed(f"crop_resize/mode_{mode}/rows_{N}", lambda: fo.crop_resize(frames[0], c["geom"], (R, R), mode, out=out, **kw))
        del c
    for V in (1, 8):                                                                         # 8 frames, V rows each
        N, offs = 8 * V, [V * f for f in range(9)]
        c = rows(N)
        tag = f"frames_8x{V}"
        planes = torch.empty((N, 5, H, W, 3), dtype=torch.uint8, device=dev)
        timed(f"fill_planes_frames/{tag}", lambda: pu.fill_planes_frames(frames, offs, c["pts"], c["nv"], planes))
        del planes
        for mode, kw in ((0, {}), (1, dict(mean=fo.IMAGENET_MEAN, std=fo.IMAGENET_STD))):
            out = None if mode == 0 else fo.crop_resize_frames(frames, offs, c["geom"], (R, R), mode, **kw)
            timed(f"crop_resize_frames/mode_{mode}/{tag}", lambda: fo.crop_resize_frames(frames, offs, c["geom"], (R, R), mode, out=out, **kw))
        xy = fo.vunet_inputs_frames(frames, offs, c["masks"], c["ssk"], c["dsk"], c["geom"], res=R)
        timed(f"vunet_inputs_frames/{tag}", lambda: fo.vunet_inputs_frames(frames, offs, c["masks"], c["ssk"], c["dsk"], c["geom"], res=R, out=xy))
        for name, box in (("plain", {}), ("boxes", dict(box_images=c["box"], box_geom=c["rects"]))):
            timed(f"paste_back_frames_device/{name}/{tag}", lambda: pu.paste_back_frames_device(frames, c["nets"], c["geom"], c["masks"], **box))
            timed(f"paste_back_ragged_device/{name}/{tag}", lambda: pu.paste_back_ragged_device(frames, offs, c["nets"], c["geom"], c["masks"], **box))
        del c, xy
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, "ms": ms}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
