#!/usr/bin/env python3
"""Build-time check of the single-pass fp16 mode's kernels (needs hipcc, no GPU): compiles the halo and tap-unit translation
units with -Rpass-analysis=kernel-resource-usage and compares every MODE 3 instantiation with its MODE 1 (bf16) sibling -
scratch 0, no VGPR spill, at least the sibling's occupancy.  Writes the table (default profiles/f16_mode_resources.txt) and exits
non-zero when an instantiation misses.

usage: tools/f16_mode_resources.py [--out FILE] [--logs DIR]     (--logs: parse remark logs NAME.log made earlier instead of compiling)"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "future_urban_scene_generation_amd", "csrc")
UNITS = ["conv_halo_128", "conv_halo_64", "conv_halo_32", "conv_halo_64k", "conv_halo_32k",
         "conv_tapunit_128", "conv_tapunit_64", "conv_tapunit_32"]
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-ffp-contract=off",
         "-Rpass-analysis=kernel-resource-usage"]                     # csrc/Makefile's CXXFLAGS + the remarks
PK = {0: "none", 1: "elu", 2: "affine"}


def compile_unit(unit, outdir):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc] + FLAGS + ["-c", unit + ".hip", "-o", os.path.join(outdir, unit + ".o")], cwd=CSRC,
                       capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(f"{unit}: hipcc failed\n{p.stderr[-3000:]}")
    return p.stderr


def parse(text):
    """{(kernel, template args): {vgprs, agprs, scratch, occupancy, spill}} of one remark log."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            name = body.split(":", 1)[1].strip()
            k = re.match(r"_ZN4fusg\d+(conv_halo_h3|conv_tapunit_h3)I(.*?)EEv", name)
            cur = None
            if k:
                args = tuple(int(a[2:].replace("n", "-")) for a in re.findall(r"Li-?n?\d+", k.group(2)))
                cur = out.setdefault((k.group(1), args), {})
            continue
        if cur is None:
            continue
        key, _, val = body.partition(":")
        key = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occ",
               "VGPRs Spill": "vspill", "SGPRs Spill": "sspill"}.get(key.strip())
        if key:
            cur[key] = int(val)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "f16_mode_resources.txt"))
    ap.add_argument("--logs")
    a = ap.parse_args()
    if a.logs:
        logs = {u: open(os.path.join(a.logs, u + ".log")).read() for u in UNITS}
    else:
        with tempfile.TemporaryDirectory() as td, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            logs = dict(zip(UNITS, ex.map(lambda u: compile_unit(u, td), UNITS)))
    rows, bad = [], []
    for unit in UNITS:
        ks = parse(logs[unit])
        halo = unit.startswith("conv_halo")
        mi = 6                                                         # MODE's place in both templates' argument lists
        for (kern, args), r in sorted(ks.items()):
            if args[mi] != 3:
                continue
            sib = ks.get((kern, args[:mi] + (1,) + args[mi + 1:]))
            what = (f"TM{args[0]} TN{args[1]} WM{args[2]} WN{args[3]} pre={PK[args[4]]:6s} " +
                    (f"NI={args[5]:<2d} KS={args[7]}" if halo else f"U={args[5]}"))
            # (SGPR spills go to VGPR lanes, not to memory, and MODE 1 has them too: not part of the check)
            two = halo and args[7] == 1 and args[5] >= 10 and ((args[0], args[4]) in ((4, 1), (2, 2)))    # halo_bf16_dense's MODE 3 exceptions
            ok = sib is not None and r["scratch"] == 0 and r["vspill"] == 0 and (r["occ"] >= sib["occ"] or (two and r["occ"] >= 2))
            if two:
                what += " *"
            rows.append(f"{unit:17s} {what:46s} {r['vgprs']:5d} {r['agprs']:5d} {r['scratch']:7d} {r['occ']:4d}   |"
                        f" {sib['vgprs'] if sib else -1:5d} {sib['scratch'] if sib else -1:7d} {sib['occ'] if sib else -1:4d}   {'ok' if ok else 'MISS'}")
            if not ok:
                bad.append(rows[-1])
    head = ["Single-pass fp16 mode (MODE 3) of the halo and tap-unit kernels against the bf16 mode (MODE 1) of the same instantiation.",
            "hipcc " + " ".join(FLAGS) + "   (tools/f16_mode_resources.py; gfx950, no GPU needed)",
            "ok = scratch 0, no VGPR spill, occupancy (waves per SIMD) at least the MODE 1 sibling's.  The 128-column instantiations that would",
            "spill at 168 VGPRs keep two waves in both modes (conv_kernel_halo.h, halo_bf16_dense); * marks the two that spill at 168 in MODE 3",
            "only (it carries the range guard's running maximum, one register more) and keep two waves there.", "",
            f"{'unit':17s} {'instantiation':46s} {'VGPR':>5s} {'AGPR':>5s} {'scratch':>7s} {'occ':>4s}   | {'VGPR1':>5s} {'scratch1':>7s} {'occ1':>4s}"]
    text = "\n".join(head + rows + ["", f"{len(rows)} MODE 3 instantiations, {len(bad)} missing the check"]) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 1 if bad or not rows else 0


if __name__ == "__main__":
    sys.exit(main())
