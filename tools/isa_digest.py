#!/usr/bin/env python3
"""Digest of the device code of every kernel in libfusg: what a kernel refactor compares against.

    isa_digest.py CSRC_DIR [-o OUT.json]    compile every translation unit of the Makefile's SRCS with the
                                            Makefile's flags plus -save-temps (temporary directory, <= 16 jobs)
                                            and write, per kernel symbol: sha256 of its instruction text
                                            (comments and trailing blanks stripped, the symbol's own lines
                                            only), vgpr_count, sgpr_count, private_segment_fixed_size,
                                            group_segment_fixed_size
    isa_digest.py --diff A.json B.json      print the symbols added, removed or changed; exit 1 if there are any

CSRC_DIR must sit in a whole tree (a worktree or `git archive` of the commit): common.h includes ../../include/fusg.h.
No GPU is needed: hipcc cross-compiles.  The committed profiles/isa_digest.json is the digest of the tree it
is committed with, so the next refactor has its parent's figures without rebuilding the parent.
"""
import argparse
import concurrent.futures
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

# local labels carry the ordinal of their function in the translation unit (.LBB12_3): not part of the instructions
LOCAL = re.compile(r"\.L(BB|JTI|CPI)\d+_")
FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def make_vars(csrc):
    """The Makefile's simple assignments, $(VAR) references expanded; the environment wins over `?=`."""
    raw = {}
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"^(\w+)\s*(\?=|=)\s*(.*)$", line.rstrip("\n"))
        if m:
            name, op, val = m.groups()
            raw[name] = os.environ.get(name, val) if op == "?=" else val

    def expand(v, depth=0):
        return v if depth > 8 else re.sub(r"\$\((\w+)\)", lambda r: expand(raw.get(r.group(1), ""), depth + 1), v)
    return {k: expand(v) for k, v in raw.items()}


def compile_tu(hipcc, flags, src, tmp):
    stem = os.path.splitext(os.path.basename(src))[0]
    work = os.path.join(tmp, stem)
    os.makedirs(work)
    cmd = [hipcc] + flags + ["-save-temps", "-c", src, "-o", os.path.join(work, stem + ".o")]
    r = subprocess.run(cmd, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), r.stdout))
    asm = [f for f in os.listdir(work) if "amdgcn" in f and f.endswith(".s")]
    if len(asm) != 1:
        raise RuntimeError("%s: expected one device assembly file, found %r" % (src, asm))
    return digest_asm(open(os.path.join(work, asm[0])).read(), os.path.basename(src))


def digest_asm(text, tu):
    """{kernel symbol: {tu, sha256, resource numbers}} of one device assembly file."""
    meta, cur = {}, None
    for line in text.splitlines():                       # the amdhsa.kernels metadata: one `- .args:` item per kernel
        s = line.strip()
        if s.startswith("- .") and not line.startswith("      "):
            cur = {}
            s = s[2:]
        m = re.match(r"^\.(\w+):\s+(\S+)$", s)
        if cur is not None and m and not line.startswith("      "):
            if m.group(1) == "name":
                meta[m.group(2).strip("'\"")] = cur
            elif m.group(1) in FIELDS:
                cur[m.group(1)] = int(m.group(2))
    out, lines, i = {}, text.splitlines(), 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", lines[i])
        if m and m.group(1) in meta and m.group(1) not in out:
            h, i = hashlib.sha256(), i + 1
            while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
                s = LOCAL.sub(r".L\1_", lines[i].split(";", 1)[0].rstrip())
                if s:
                    h.update(s.encode() + b"\n")
                i += 1
            missing = [f for f in FIELDS if f not in meta[m.group(1)]]
            if missing:
                raise RuntimeError("%s: %s has no %s" % (tu, m.group(1), missing))
            out[m.group(1)] = dict(tu=tu, sha256=h.hexdigest(), **meta[m.group(1)])
        i += 1
    if set(out) != set(meta):
        raise RuntimeError("%s: no code found for %r" % (tu, sorted(set(meta) - set(out))))
    return out


def build_digest(csrc, jobs):
    csrc = os.path.abspath(csrc)
    v = make_vars(csrc)
    srcs = [os.path.join(csrc, s) for s in v["SRCS"].split()]
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(min(jobs, 16)) as pool:
        for d in pool.map(lambda s: compile_tu(v["HIPCC"], v["CXXFLAGS"].split(), s, tmp), srcs):
            dup = set(d) & set(kernels)
            if dup:
                raise RuntimeError("kernel symbols defined twice: %r" % sorted(dup))
            kernels.update(d)
    return {"flags": v["CXXFLAGS"], "kernels": dict(sorted(kernels.items()))}


def diff(a_path, b_path):
    a, b = (json.load(open(p))["kernels"] for p in (a_path, b_path))
    n = 0
    for sym in sorted(set(a) | set(b)):
        if sym not in b:
            print("removed  %s (%s)" % (sym, a[sym]["tu"]))
        elif sym not in a:
            print("added    %s (%s)" % (sym, b[sym]["tu"]))
        else:
            ch = [k for k in ("sha256",) + FIELDS if a[sym][k] != b[sym][k]]
            if not ch:
                continue
            print("changed  %s (%s): %s" % (sym, b[sym]["tu"], ", ".join(
                k if k == "sha256" else "%s %d -> %d" % (k, a[sym][k], b[sym][k]) for k in ch)))
        n += 1
    print("%d kernel symbols in A, %d in B, %d differ" % (len(a), len(b), n))
    return 1 if n else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("csrc", nargs="?", help="directory with the Makefile and the .hip files")
    ap.add_argument("-o", "--out", help="write the JSON here (default: stdout)")
    ap.add_argument("-j", "--jobs", type=int, default=16)
    ap.add_argument("--diff", nargs=2, metavar=("A.json", "B.json"))
    a = ap.parse_args()
    if a.diff:
        return diff(*a.diff)
    if not a.csrc:
        ap.error("a csrc directory or --diff is required")
    text = json.dumps(build_digest(a.csrc, a.jobs), indent=1) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
