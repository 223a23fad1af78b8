#!/usr/bin/env python3
"""Measure the tolerances of the device-pose tests -> profiles/pose_geometry_parity.json.

  host_vs_numpy     fusg_pose_geometry_host against the numpy chain of the frame driver, over the cases of
                    tests/pose_geometry_cases.py: per float output the largest absolute and relative difference, the float32
                    pose in ulps; bar_abs = 8 x the largest absolute difference (tests/test_pose_geometry_cpu.py)
  device_vs_host    the kernel against the host twin on the same cases (GPU box), same figures (tests/test_gpu_pose_geometry.py)
  flag_on_vs_off    geometry-mode run_frame / run_later_frame with device_pose on against off, on the scenes of
                    tests/test_gpu_pose_geometry.py: per rendered uint8 output the share of differing bytes and the largest
                    level difference; bar_share = 10 x the share (DESIGN.md §7's ratio), 0 = equality
Without a GPU only the first block is measured; the other two are kept from the file as it is.  Every block carries
"measured" = the time and host of the run that produced it, so a block carried over is recognisable."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pose_geometry_cases as pc  # noqa: E402


def float_block(pairs):
    """pairs: case name -> (got, want, rows of got to compare) -> the per-output maxima and bars."""
    out, ulp = {}, 0
    for name, (got, want, rows) in pairs.items():
        fg, fw = pc.float_outputs(got, rows), pc.float_outputs(want)
        ulp = max(ulp, pc.ulp32(fg["pose"], fw["pose"]))
        for k in fg:
            ad, rel = pc.diffs(fg[k], fw[k])
            o = out.setdefault(k, {"max_abs": 0.0, "max_rel": 0.0})
            o["max_abs"], o["max_rel"] = max(o["max_abs"], ad), max(o["max_rel"], rel)
    return {"cases": list(pairs), "outputs": out, "pose_ulp32": ulp, "bar_abs": {k: 8 * v["max_abs"] for k, v in out.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "pose_geometry_parity.json"))
    a = ap.parse_args()
    src = os.path.join(ROOT, "profiles", "pose_geometry_parity.json")
    res = json.load(open(src)) if os.path.exists(src) else {}
    cases = pc.cases()
    refs = {n: pc.reference(c) for n, c in cases.items()}
    hosts = {n: pc.host(c) for n, c in cases.items()}
    import datetime
    import platform
    stamp = {"utc": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ"), "numpy": np.__version__,
             "torch": torch.__version__, "machine": platform.machine()}
    res["host_vs_numpy"] = float_block({n: (hosts[n], refs[n], refs[n]["valid"]) for n in cases})
    res["host_vs_numpy"]["measured"] = stamp
    if torch.cuda.is_available():
        import test_gpu_pose_geometry as tg                  # (the scenes and helpers of the test that asserts these figures)
        stamp = dict(stamp, device=torch.cuda.get_device_name(0))
        res["device"] = torch.cuda.get_device_name(0)
        res["device_vs_host"] = float_block({n: (tg.device_outputs(c), hosts[n], None) for n, c in cases.items()})
        fr = tg.runs()
        blk = {}
        for tag in ("on", "on_hom", "on_later", "on_hom_later"):
            a_, b_ = tg.frame_bytes(fr[tag]), tg.frame_bytes(fr["off_later" if tag.endswith("later") else "off"])
            for k in a_:
                share, level = tg.byte_diff(a_[k], b_[k])
                o = blk.setdefault(k, {"share": 0.0, "max_level": 0, "bytes": int(a_[k].numel())})
                o["share"], o["max_level"] = max(o["share"], share), max(o["max_level"], level)
        res["flag_on_vs_off"] = {"runs": ["on", "on_hom", "on_later", "on_hom_later"], "frame": "360x640", "vehicles": 3, "outputs": blk,
                                 "pose_ulp32": pc.ulp32(tg.pose_rows(fr["on"]["pose"]), tg.pose_rows(fr["off"]["pose"])),
                                 "bar_share": {k: 10 * v["share"] for k, v in blk.items()}}
        res["device_vs_host"]["measured"] = res["flag_on_vs_off"]["measured"] = stamp
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
