"""GPU: the routing sweep of fusg_conv2d (tests/conv_sweep.py).  Every case - the edge table (both sides of every condition the
router tests) and a seeded random draw from the space it admits - runs at f32, f16x3 and bf16 with the planner's K split, and
each launch is judged against float64 by the one comparator, at the bar of the family that actually ran.  A case also checks
the family the router picked (the edge table's record, the restated router's prediction), the range status, a bit-identical
repeat, the next family in the router's order (the per-call off-switch of the family it landed on), explicit tiles / K splits
on the generic gathers, the small-image kernel's K ranges (FUSG_SMALL_KSPLIT=1) and batch invariance.  The switches cached
once per process (FUSG_HALO_MINWG, FUSG_NO_KSPLIT) are covered by the halo subset in fresh child processes."""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import conv_sweep as cs

pytestmark = pytest.mark.gpu

from future_urban_scene_generation_amd import _lib as L          # noqa: E402
from future_urban_scene_generation_amd import ops                 # noqa: E402

SENTINEL = cs.SENTINEL
PER_CALL = ("FUSG_NO_SMALL", "FUSG_NO_POINTWISE", "FUSG_NO_F32_HALO", "FUSG_NO_BF16_TAPUNIT", "FUSG_SMALL_KSPLIT")
HALO_FAMILIES = (cs.HALO, cs.HALO_S2D, cs.HALO_BF16, cs.HALO_F32)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


class _env:
    """Per-call switches set for the duration of one launch (libfusg reads them per call)."""

    def __init__(self, env):
        self.env = dict(env or {})

    def __enter__(self):
        assert set(self.env) <= set(PER_CALL), self.env
        self.old = {k: os.environ.get(k) for k in PER_CALL}
        for k in PER_CALL:
            os.environ.pop(k, None)
        os.environ.update(self.env)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


_PREP = {}


def _prepare(c: cs.Case, sample=None):
    """Plan, device operands and the float64 reference of a case (of one of its samples: `sample`), cached."""
    key = (c.tag, sample)
    if key in _PREP:
        return _PREP[key]
    inp = cs.inputs(c)
    ref, den = cs.reference(c, inp)
    plan = cs.make_plan(c, inp["w"], inp["b"])
    sl = slice(None) if sample is None else slice(sample, sample + 1)
    d = dev()
    S = {"plan": plan, "ref": cs.window(c, ref[sl]), "den": cs.window(c, den[sl]), "B": ref[sl].shape[0]}
    rb = cs.reference_bf16(c, inp)
    S["ref_bf16"] = None if rb is None else (cs.window(c, rb[0][sl]), cs.window(c, rb[1][sl]))
    S["x0"] = ops.as_nhwc(inp["x0"][sl].contiguous().to(d), cpad=c.cin_pad)
    S["x1"] = ops.as_nhwc(inp["x1"][sl].contiguous().to(d), cpad=c.cin_pad) if c.c1 else None
    if c.pre.startswith("affine"):
        ctot = plan.c0k + plan.c1k

        def lay(v):                                       # logical channels -> the K layout's (src0 padded to c0k, then src1)
            v = v[sl] if c.per_sample else v
            o = torch.zeros(*v.shape[:-1], ctot)
            o[..., :c.c0] = v[..., :c.c0]
            o[..., plan.c0k:plan.c0k + c.c1] = v[..., c.c0:]
            return o.contiguous().to(d)
        S["pre"] = (lay(inp["scale"]), lay(inp["shift"]))
        S["pre_bstride"] = ctot if c.per_sample else 0
    S["res"] = [ops.as_nhwc(r[sl].contiguous().to(d)) for r in inp["res"]]
    _PREP[key] = S
    return S


def _launch(c: cs.Case, S: dict, prec: str, env=None, ksplit=None, tile=L.TILE_AUTO):
    """One ops.conv launch of the case -> (result in the reference's layout, float64 on the CPU; family; what it wrote
    outside the result, which must be untouched)."""
    kw, guard = cs.launch_kwargs(c, S["B"], dev(), prec, pre=S.get("pre"), pre_bstride=S.get("pre_bstride", 0), res=S["res"],
                                 ksplit=ksplit, tile=tile)
    with _env(env):
        y = ops.conv(S["plan"], S["x0"], S["x1"], **kw)
        fam = ops.last_conv_kernel()
    y = y.cpu().double()
    rest = torch.empty(0, dtype=torch.float64)
    if guard is not None:                                  # a misaligned output: the sentinels on both sides of it
        rest = cs.guard_elements(guard)
    if c.out == "slice":
        rest = torch.cat([y[:, :c.out_c_off].flatten(), y[:, c.out_c_off + c.cout:].flatten()])
        y = y[:, c.out_c_off:c.out_c_off + c.cout]
    if c.qwin:
        oy, ox, h, w = c.qwin
        mask = torch.ones(y.shape, dtype=torch.bool)
        mask[:, :, oy:oy + h, ox:ox + w] = False
        rest = y[mask]
        y = cs.window(c, y)
    return y.contiguous(), fam, rest


# ---- observations: worst error and landings per family ----------------------------------------------------------------
OBS = {}
_DONE = set()


def _observe(fam, err, where, landed=False):
    o = OBS.setdefault(fam, {"cases": 0, "worst": 0.0, "at": ""})
    o["cases"] += 1 if landed else 0
    if err > o["worst"] or not o["at"]:
        o["worst"], o["at"] = max(err, o["worst"]), where


def _check(c, S, prec, fails, env=None, ksplit=None, tile=L.TILE_AUTO, what="main", expect=None):
    """Launch, judge against float64 at the bar of the family that ran; returns (result, family)."""
    y, fam, rest = _launch(c, S, prec, env=env, ksplit=ksplit, tile=tile)
    err = cs.norm_err(y, S["ref"], S["den"])
    where = f"{c.tag}/{prec}/{what}"
    _observe(fam, err, where, landed=what == "main")
    if err > cs.bar(fam):
        fails.append(f"{where}: family {fam} error {err:.3e} > bar {cs.bar(fam):.3e}")
    if fam in (cs.HALO_BF16, cs.TAPUNIT_BF16) and S["ref_bf16"] is not None:      # the bf16 kernels' own arithmetic
        eb = cs.norm_err(y, *S["ref_bf16"])
        _observe(("bf16_operands", fam), eb, where)
        if eb > cs.BAR_FP32:
            fails.append(f"{where}: family {fam} differs from the bf16-operand reference by {eb:.3e} > {cs.BAR_FP32:.3e}")
    if rest.numel() and not bool((rest == SENTINEL).all()):
        fails.append(f"{where}: wrote outside its output")
    if expect is not None and fam != expect:
        fails.append(f"{where}: ran family {fam}, expected {expect}")
    if ops.range_exceeded(dev()):
        fails.append(f"{where}: range status raised")
    return y, fam


def run_case(c: cs.Case, precisions=cs.PRECISIONS, extras=True):
    """Every check of one case; returns the list of failures (empty: passed)."""
    fails = []
    S = _prepare(c)
    ops.range_exceeded(dev())                                  # (a clean status word)
    for i, prec in enumerate(precisions):
        pred = cs.predict_family(c, prec)
        want = c.expect[cs.PRECISIONS.index(prec)] if c.expect else pred
        if c.expect and pred != want:
            fails.append(f"{c.tag}/{prec}: restated router says {pred}, table says {want}")
        y, fam = _check(c, S, prec, fails, expect=want)
        y2, _, _ = _launch(c, S, prec)
        if not torch.equal(y, y2):
            fails.append(f"{c.tag}/{prec}: repeat launch not bit-identical")
        if not extras:
            continue
        sw = cs.off_switch(fam, c)                             # the next family in the router's order, same data
        if sw is not None:
            env, ks = sw
            _check(c, S, prec, fails, env=env, ksplit=ks, what="off%d" % fam,
                   expect=cs.predict_family(c, prec, env=env, ksplit=ks))
        if fam in (cs.GEN_F32, cs.GEN_F16X3):                 # explicit tiles and K splits of the generic gathers
            cp, nk = S["plan"].cout_pad, S["plan"].k_pad // 32
            tiles = [L.TILE_128x32] + ([L.TILE_64x64] if cp % 64 == 0 else []) + ([L.TILE_64x128, L.TILE_128x128] if cp % 128 == 0 else [])
            for t in tiles:
                for ks in sorted({1, min(3, nk), min(8, nk)}):
                    _check(c, S, prec, fails, ksplit=ks, tile=t, what=f"tile{t}_ks{ks}",
                           expect=cs.predict_family(c, prec, ksplit=ks, tile=t))
        if prec != "f32" and fam != cs.SMALL and cs.predict_family(c, prec, env={"FUSG_SMALL_KSPLIT": "1"}) == cs.SMALL:
            _check(c, S, prec, fails, env={"FUSG_SMALL_KSPLIT": "1"}, what="small_ksplit", expect=cs.SMALL)
        if c.B >= 2 and prec != "bf16" and not c.qwin:         # batch invariance: the last sample launched alone
            b = c.B - 1
            Sb = _prepare(c, sample=b)
            yb, famb, _ = _launch(c, Sb, prec)
            e = cs.norm_err(yb, y[b:b + 1], S["den"][b:b + 1])
            if e > cs.bar(fam):
                fails.append(f"{c.tag}/{prec}: sample {b} alone (family {famb}) differs from the batch by {e:.3e}")
    _DONE.add(c.tag)
    return fails


@pytest.mark.parametrize("c", cs.all_cases(), ids=lambda c: c.tag)
def test_conv_sweep(c):
    fails = run_case(c)
    assert not fails, "\n".join(fails)


def test_sweep_covers_every_family():
    """After the sweep: every family was reached; the worst normalised error per family goes to the parity log."""
    from conftest import record
    for c in cs.edge_cases():
        if c.tag not in _DONE:
            run_case(c, extras=False)
    assert set(cs.FAMILIES) <= set(OBS), sorted(k for k in OBS if isinstance(k, int))
    for fam, o in OBS.items():
        if isinstance(fam, tuple):                             # the bf16 families against their own operand rounding
            record(f"family{fam[1]}_bf16_operands_err_max", o["worst"])
            assert o["worst"] <= cs.BAR_FP32, (fam, o)
            continue
        record(f"family{fam}_err_max", o["worst"])
        record(f"family{fam}_cases", o["cases"])
        assert o["worst"] <= cs.bar(fam), (fam, o)


# ---- the switches cached per process: the halo subset in fresh child processes ----------------------------------------
def halo_subset():
    return [c for c in cs.all_cases() if any(cs.predict_family(c, p) in HALO_FAMILIES for p in cs.PRECISIONS)]


def _child(out_path):
    rows = []
    for c in halo_subset():
        S = _prepare(c)
        for prec in cs.PRECISIONS:
            y, fam, _ = _launch(c, S, prec)
            y2, _, _ = _launch(c, S, prec)
            eb = cs.norm_err(y, *S["ref_bf16"]) if fam == cs.HALO_BF16 and S["ref_bf16"] is not None else 0.0
            rows.append({"tag": c.tag, "prec": prec, "family": fam, "expect": cs.predict_family(c, prec),
                         "err": cs.norm_err(y, S["ref"], S["den"]), "err_bf16_operands": eb,
                         "repeat_equal": bool(torch.equal(y, y2)), "range": bool(ops.range_exceeded(dev()))})
    with open(out_path, "w") as f:
        json.dump(rows, f)


@pytest.mark.parametrize("switch", ["FUSG_HALO_MINWG=1", "FUSG_NO_KSPLIT=1"])
def test_halo_subset_under_process_switches(switch):
    """FUSG_HALO_MINWG=1 keeps the widest column tile on small grids (the 128-column tile); FUSG_NO_KSPLIT=1 turns off the K
    split over the waves of the narrow tiles.  Both are read once per process: one fresh child each, one at a time."""
    from conftest import record
    k, v = switch.split("=")
    env = {kk: vv for kk, vv in os.environ.items() if kk not in PER_CALL}
    env[k] = v
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "rows.json")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", out]
        p = subprocess.run(cmd, env=env, timeout=300, capture_output=True, text=True,
                           cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
        with open(out) as f:
            rows = json.load(f)
    assert len(rows) == 3 * len(halo_subset())
    fails = []
    for r in rows:
        record(f"family{r['family']}_err_max", r["err"])
        if (r["family"] != r["expect"] or r["err"] > cs.bar(r["family"]) or r["err_bf16_operands"] > cs.BAR_FP32
                or not r["repeat_equal"] or r["range"]):
            fails.append(r)
    assert not fails, fails


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        with torch.no_grad():
            _child(sys.argv[2])
    else:
        sys.exit("usage: test_gpu_conv_sweep.py --child OUT.json")
