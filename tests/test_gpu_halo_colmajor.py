"""GPU: the column-major tap order of the 128-column halo tile (csrc/conv_kernel_halo.h, CM; conv_kernel_halo_body.inc).

Dense 3x3 dil 1 split-fp16 launches of that tile read the ten staged halo rows of a tap COLUMN once and issue the three ky taps
from them; FUSG_NO_HALO_COLMAJOR (read per call) keeps the tap-major loop.  Inputs, the float64 reference and the comparator are
tests/conv_sweep.py's, at the halo family's bar (cs.BAR_FP32); the statistics comparator is tests/stats_sweep.py's.  The shapes
are the smallest at which the loop can go wrong: one patch whose every halo row and column is padding (8 x 16), patches that
share edges (16 x 32, 24 x 16), one chunk and two (the column state must start over at the chunk boundary), two sources, one
and two column blocks.  Grids this small only get the 128-column tile under FUSG_HALO_MINWG=1, which the library reads once per
process: every launch of this file runs in ONE fresh child process, and the tests judge the rows it returns."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys
import tempfile
from dataclasses import replace

import pytest
import torch
import torch.nn.functional as F

import conv_sweep as cs
import stats_sweep as ss

pytestmark = pytest.mark.gpu

from future_urban_scene_generation_amd import _lib as L          # noqa: E402
from future_urban_scene_generation_amd import ops, pack          # noqa: E402

SWITCH = "FUSG_NO_HALO_COLMAJOR"
SENTINEL = 1234.5
HALO_FAMILIES = (cs.HALO, cs.HALO_S2D)
PAD_NAMES = {L.PAD_ZERO: "zero", L.PAD_REFLECT: "reflect", L.PAD_REPLICATE: "replicate"}


def _case(tag, B, c0, c1, cout, H, W, **kw):
    return cs.Case(tag=tag, B=B, c0=c0, c1=c1, cout=cout, kh=3, kw=3, H=H, W=W, pad=1, ksplit=1, **kw)


def grid_cases():
    """Shape x padding x pre-op in full; batch, channels (one chunk, two chunks, two sources) and column blocks cycle through them
    so that every value meets every shape, padding mode and pre-op."""
    shapes, pads = [(8, 16), (16, 32), (24, 16)], [L.PAD_ZERO, L.PAD_REFLECT, L.PAD_REPLICATE]
    pres = [("none", False), ("elu", False), ("affine_relu", True)]
    chans = [(32, 0), (64, 0), (32, 32)]
    out = []
    for i, ((s, (H, W)), (p, pm), (q, (pre, ps))) in enumerate(itertools.product(enumerate(shapes), enumerate(pads), enumerate(pres))):
        c0, c1 = chans[(s + p + q) % 3]
        B, cout = (1, 3)[i % 2], (128, 256)[(i // 2 + s) % 2]
        out.append(_case(f"g{H}x{W}_{PAD_NAMES[pm]}_{pre}_b{B}_c{c0}+{c1}_n{cout}", B, c0, c1, cout, H, W, pm=pm, pre=pre,
                         per_sample=ps, seed=i))
    return out


def epilogue_cases():
    return [_case("res_zero", 3, 64, 0, 128, 16, 32, res=1, pre="elu", seed=40),
            _case("res_reflect_two_src", 1, 32, 32, 256, 24, 16, res=1, pm=L.PAD_REFLECT, pre="affine_relu", per_sample=True, seed=41),
            _case("slice_sentinel", 3, 64, 0, 128, 16, 32, out="slice", out_c_off=4, pm=L.PAD_REPLICATE, seed=42)]


def stats_cases():
    return [_case("stats_zero", 3, 64, 0, 128, 16, 32, seed=50),
            _case("stats_reflect", 1, 32, 32, 256, 8, 16, pm=L.PAD_REFLECT, pre="affine_relu", per_sample=True, seed=51)]


def neighbour_cases():
    """Halo launches that keep the tap-major loop: dilated 3x3, 5x5 and stride 2 (the quadrant form) on the 128-column tile, and a
    1x1, which the router caps at the 64-column tile (NEIGHBOUR_TILES)."""
    base = dict(B=2, c0=64, c1=0, cout=128, H=16, W=32, ksplit=1)
    return [cs.Case(tag="nb_dil2", kh=3, kw=3, pad=2, dil=2, pm=L.PAD_REFLECT, seed=60, **base),
            cs.Case(tag="nb_1x1", kh=1, kw=1, seed=61, **base),
            cs.Case(tag="nb_5x5", kh=5, kw=5, pad=2, pm=L.PAD_REFLECT, seed=62, **base),
            cs.Case(tag="nb_s2", kh=3, kw=3, pad=1, stride=2, seed=63, **base)]


NEIGHBOUR_TILES = {"nb_dil2": 128, "nb_1x1": 64, "nb_5x5": 128, "nb_s2": 128}
ROUTE_ON, ROUTE_OFF = [cs.HALO, 128, 1, 2], [cs.HALO, 128, 1, 0]      # fusg_conv2d_route_order: (family, tile, ksplit, ksw / column-major)
TAP_PADS = (L.PAD_ZERO, L.PAD_REFLECT, L.PAD_REPLICATE)
D2S_SHAPES = ((1, 32, 8, 16), (3, 64, 16, 32))      # B, cin, H, W of the low-resolution input; 32 output channels x 4 phases


# ---- the child process: every launch, one row of figures per check ---------------------------------------------------------
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


class _order:
    """The tap order of the launches issued inside: column-major (the default) or tap-major (the switch set)."""

    def __init__(self, colmajor):
        self.colmajor = colmajor

    def __enter__(self):
        self.old = os.environ.pop(SWITCH, None)
        if not self.colmajor:
            os.environ[SWITCH] = "1"

    def __exit__(self, *exc):
        os.environ.pop(SWITCH, None)
        if self.old is not None:
            os.environ[SWITCH] = self.old
        return False


def _operands(c, inp, plan, sl=slice(None)):
    d = dev()
    S = {"x0": ops.as_nhwc(inp["x0"][sl].contiguous().to(d)), "x1": ops.as_nhwc(inp["x1"][sl].contiguous().to(d)) if c.c1 else None,
         "kw": {}}
    if c.pre.startswith("affine"):
        ctot = plan.c0k + plan.c1k
        S["kw"].update(pre=tuple(v[sl].contiguous().to(d) if c.per_sample else v.to(d) for v in (inp["scale"], inp["shift"])),
                       pre_bstride=ctot if c.per_sample else 0)
    for i, r in enumerate(inp["res"]):
        S["kw"]["res%d" % i] = ops.as_nhwc(r[sl].contiguous().to(d))
    return S


def _route(plan, x0, x1, colmajor, **kw):
    """fusg_conv2d_route_order of the launch ops.conv would make: [family, tile, ksplit, 1 K split over waves / 2 column-major / 0]."""
    d, _ = ops._conv_desc(plan, x0, x1, **kw)
    L.lib().fusg_conv2d_plan(C.byref(d))
    out = (C.c_int32 * 4)()
    with _order(colmajor):
        rc = L.lib().fusg_conv2d_route_order(C.byref(d), C.byref(out))
    assert rc == 0, (rc, L.lib().fusg_last_error())
    return list(out)


def _routes(c, plan, S, **extra):
    kw = dict(pre_op=cs.PRE[c.pre], act=c.act, precision="f16x3", ksplit=c.ksplit, **S["kw"], **extra)
    return {"route_on": _route(plan, S["x0"], S["x1"], True, **kw), "route_off": _route(plan, S["x0"], S["x1"], False, **kw)}


def _run(c, plan, S, B, colmajor=True, **extra):
    """One f16x3 launch -> (result NCHW float64 on the CPU, family, what lies around a sliced output)."""
    kw = dict(pre_op=cs.PRE[c.pre], act=c.act, precision="f16x3", ksplit=c.ksplit, **S["kw"], **extra)
    ho, wo = c.full_hw()
    if c.out == "slice":
        out = ops.nhwc_empty(B, c.out_c_off + c.cout + 4, ho, wo, dev())
        out.fill_(SENTINEL)
        kw.update(out=out, out_c_off=c.out_c_off)
    with _order(colmajor):
        y = ops.conv(plan, S["x0"], S["x1"], **kw)
        fam = ops.last_conv_kernel()
    stats = None
    if isinstance(y, tuple):
        y, stats = y
    y = y.cpu().double()
    rest = torch.empty(0, dtype=torch.float64)
    if c.out == "slice":
        rest = torch.cat([y[:, :c.out_c_off].flatten(), y[:, c.out_c_off + c.cout:].flatten()])
        y = y[:, c.out_c_off:c.out_c_off + c.cout]
    return y.contiguous(), fam, rest, stats


def _conv_rows(c, kind):
    """Both orders of one case against float64, a repeat launch, the range status, the sentinel; for B = 3 sample 0 alone."""
    inp = cs.inputs(c)
    ref, den = cs.reference(c, inp)
    plan = cs.make_plan(c, inp["w"], inp["b"])
    S = _operands(c, inp, plan)
    row = {"kind": kind, "tag": c.tag, "bar": cs.bar(cs.HALO), **_routes(c, plan, S)}
    ops.range_exceeded(dev())
    ys = {}
    for name, cm in (("on", True), ("off", False)):
        y, fam, rest, _ = _run(c, plan, S, c.B, cm)
        y2 = _run(c, plan, S, c.B, cm)[0]
        ys[name] = y
        row[name] = {"family": fam, "err": cs.norm_err(y, ref, den), "repeat_equal": bool(torch.equal(y, y2)),
                     "range": bool(ops.range_exceeded(dev())), "sentinel_ok": bool((rest == SENTINEL).all())}
    row["orders_equal"] = bool(torch.equal(ys["on"], ys["off"]))
    if c.B == 3:                                                # sample 0 launched alone, the routing batch held at 3
        S1 = _operands(c, inp, plan, slice(0, 1))
        with ops.route_batch(3):
            yb = _run(c, plan, S, 3)[0]
            y1 = _run(c, plan, S1, 1)[0]
        row["batch_invariant"] = bool(torch.equal(y1, yb[0:1]))
    return row


def _stats_rows(c):
    inp = cs.inputs(c)
    ref, den = cs.reference(c, inp)
    plan = cs.make_plan(c, inp["w"], inp["b"])
    S = _operands(c, inp, plan)
    row = {"kind": "stats", "tag": c.tag, "bar": cs.bar(cs.HALO), **_routes(c, plan, S)}
    for name, cm in (("on", True), ("off", False)):
        y, fam, _, slots = _run(c, plan, S, c.B, cm, want_stats=True)
        assert slots is not None, "the launch must qualify for the fused statistics"
        over = ss.over_bars(ss.stat_errs(ss.combine(slots.cpu()), ss.direct(y)))
        with _order(cm):                                        # the same launch through ops.conv_in: same output bytes
            y_in, (scale, shift) = ops.conv_in(plan, S["x0"], x1=S["x1"], pre_op=cs.PRE[c.pre], precision="f16x3", ksplit=1, **S["kw"])
        finite = bool(torch.isfinite(scale).all()) and bool(torch.isfinite(shift).all())
        row[name] = {"family": fam, "err": cs.norm_err(y, ref, den), "stats_over_bars": {k: float(v) for k, v in over.items()},
                     "conv_in_equal": bool(torch.equal(y_in.cpu().double(), y)), "conv_in_finite": finite}
    return row


def _d2s(t, cout):
    """[B, 4 cout, H, W] with phase 2 py + px in channel block (2 py + px) cout -> [B, cout, 2H, 2W]."""
    B, _, H, W = t.shape
    return t.reshape(B, 2, 2, cout, H, W).permute(0, 3, 4, 1, 5, 2).reshape(B, cout, 2 * H, 2 * W)


def _d2s_rows(B, cin, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    w5 = torch.randn(32, cin, 5, 5, generator=g) / (cin * 25) ** 0.5
    b = torch.randn(32, generator=g)
    plan = pack.pack_conv_up2_d2s(w5, b)
    c = _case(f"d2s_b{B}_c{cin}_{H}x{W}", B, cin, 0, 128, H, W, pm=L.PAD_REPLICATE, pre="affine_relu", per_sample=True, seed=seed)
    inp = cs.inputs(c)
    inp["w"], inp["b"] = torch.cat(pack.up2_phase_weights(w5), 0).float(), b.repeat(4)
    ref, den = cs.reference(c, inp)
    ref, den = _d2s(ref, 32), _d2s(den, 32)
    S = _operands(c, inp, plan)
    row = {"kind": "d2s", "tag": c.tag, "bar": cs.bar(cs.HALO), **_routes(c, plan, S, store=L.STORE_D2S)}
    for name, cm in (("on", True), ("off", False)):
        y, fam, _, _ = _run(c, plan, S, B, cm, store=L.STORE_D2S)
        y2 = _run(c, plan, S, B, cm, store=L.STORE_D2S)[0]
        row[name] = {"family": fam, "err": cs.norm_err(y, ref, den), "repeat_equal": bool(torch.equal(y, y2)),
                     "range": bool(ops.range_exceeded(dev())), "sentinel_ok": True}
    return row


def _tap_rows(pm):
    """For each of the nine taps: weights that copy channel n % 64 of the input at that tap and nothing else; small integers are
    exact in the fp16 split, so the output must be the shifted padded input bit for bit."""
    B, cin, cout, H, W = 2, 64, 128, 16, 32
    g = torch.Generator().manual_seed(70 + pm)
    x = torch.randint(-8, 9, (B, cin, H, W), generator=g).float()
    xp = F.pad(x, (1, 1, 1, 1)) if pm == L.PAD_ZERO else F.pad(x, (1, 1, 1, 1), mode="reflect" if pm == L.PAD_REFLECT else "replicate")
    xd = ops.as_nhwc(x.to(dev()))
    rows = []
    for ky in range(3):
        for kx in range(3):
            w = torch.zeros(cout, cin, 3, 3)
            w[torch.arange(cout), torch.arange(cout) % cin, ky, kx] = 1.0
            plan = pack.pack_conv(w, None, stride=1, pad=1, pad_mode=pm)
            want = xp[:, :, ky:ky + H, kx:kx + W].repeat(1, cout // cin, 1, 1)
            row = {"kind": "tap", "tag": f"tap{ky}{kx}_{PAD_NAMES[pm]}",
                   "route_on": _route(plan, xd, None, True, precision="f16x3", ksplit=1),
                   "route_off": _route(plan, xd, None, False, precision="f16x3", ksplit=1)}
            for name, cm in (("on", True), ("off", False)):
                with _order(cm):
                    y = ops.conv(plan, xd, precision="f16x3", ksplit=1)
                    fam = ops.last_conv_kernel()
                row[name] = {"family": fam, "equal": bool(torch.equal(y.cpu(), want)), "range": bool(ops.range_exceeded(dev()))}
            rows.append(row)
    return rows


def _neighbour_row(c):
    inp = cs.inputs(c)
    ref, den = cs.reference(c, inp)
    plan = cs.make_plan(c, inp["w"], inp["b"])
    S = _operands(c, inp, plan)
    on, fam_on = _run(c, plan, S, c.B, True)[:2]
    off, fam_off = _run(c, plan, S, c.B, False)[:2]
    return {"kind": "neighbour", "tag": c.tag, "bar": cs.bar(cs.HALO), "family_on": fam_on, "family_off": fam_off, **_routes(c, plan, S),
            "err": cs.norm_err(on, ref, den), "orders_equal": bool(torch.equal(on, off)), "range": bool(ops.range_exceeded(dev()))}


def _range_row():
    """An operand the split cannot represent raises the status word under both orders; in range it stays clear."""
    c = _case("range", 1, 64, 0, 128, 16, 32, seed=80)
    inp = cs.inputs(c)
    plan = cs.make_plan(c, inp["w"], inp["b"])
    bad = dict(inp, x0=inp["x0"].clone())
    bad["x0"][0, 40, 9, 17] = 1e5                               # second chunk, an inner pixel
    row = {"kind": "range", "tag": c.tag, **_routes(c, plan, _operands(c, inp, plan))}
    ops.range_exceeded(dev())
    for name, cm in (("on", True), ("off", False)):
        _run(c, plan, _operands(c, inp, plan), 1, cm)
        clear = not ops.range_exceeded(dev())
        _, fam, _, _ = _run(c, plan, _operands(c, bad, plan), 1, cm)
        raised = ops.range_exceeded(dev())
        row[name] = {"family": fam, "clear_in_range": bool(clear), "raised": bool(raised), "cleared_by_read": not ops.range_exceeded(dev())}
    return row


def _child(out_path):
    rows = [_conv_rows(c, "grid") for c in grid_cases()] + [_conv_rows(c, "epilogue") for c in epilogue_cases()]
    rows += [_stats_rows(c) for c in stats_cases()]
    rows += [_d2s_rows(*shape, seed=90 + i) for i, shape in enumerate(D2S_SHAPES)]
    for pm in TAP_PADS:
        rows += _tap_rows(pm)
    rows += [_neighbour_row(c) for c in neighbour_cases()] + [_range_row()]
    with open(out_path, "w") as f:
        json.dump(rows, f)


# ---- the tests --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows():
    env = {k: v for k, v in os.environ.items() if k not in (SWITCH, "FUSG_NO_SMALL", "FUSG_HALO_BN", "FUSG_NO_KSPLIT", "FUSG_NO_HALO")}
    env["FUSG_HALO_MINWG"] = "1"                                # the widest column tile on grids this small
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "rows.json")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", out]
        p = subprocess.run(cmd, env=env, timeout=600, capture_output=True, text=True,
                           cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
        with open(out) as f:
            return json.load(f)


def _of(rows, kind):
    got = [r for r in rows if r["kind"] == kind]
    assert got, kind
    return got


def _launch_fails(r, arms=("on", "off")):
    fails = []
    for a in arms:
        o = r[a]
        if o["family"] != cs.HALO:
            fails.append(f"{r['tag']}/{a}: family {o['family']}")
        if not o["err"] <= r["bar"]:
            fails.append(f"{r['tag']}/{a}: error {o['err']:.3e} > bar {r['bar']:.3e}")
        if not o.get("repeat_equal", True):
            fails.append(f"{r['tag']}/{a}: repeat launch not bit-identical")
        if o.get("range", False):
            fails.append(f"{r['tag']}/{a}: range status raised")
        if not o.get("sentinel_ok", True):
            fails.append(f"{r['tag']}/{a}: wrote outside its output")
    return fails


def test_every_case_ran(rows):
    n = len(grid_cases()) + len(epilogue_cases()) + len(stats_cases()) + len(D2S_SHAPES) + 9 * len(TAP_PADS) + len(neighbour_cases()) + 1
    assert len(rows) == n, (len(rows), n)
    print("worst normalised error, column-major / tap-major: %.3e / %.3e (bar %.3e)" % (
        max(r["on"]["err"] for r in rows if "on" in r and "err" in r["on"]),
        max(r["off"]["err"] for r in rows if "off" in r and "err" in r["off"]), cs.BAR_FP32))


def test_every_case_takes_the_loop_it_names(rows):
    """Per case, from the router's dry run: with the switch unset the launch is the 128-column tile's column-major instantiation
    (fusg_conv2d_route_order: tile 128, last entry 2), with it set the same tile tap-major (0) - no case tests one loop twice."""
    bad = [(r["tag"], r["route_on"], r["route_off"]) for r in rows if r["kind"] != "neighbour"
           and (r["route_on"] != ROUTE_ON or r["route_off"] != ROUTE_OFF)]
    assert not bad, bad


def test_grid_both_orders_against_float64(rows):
    """Shapes x padding x pre-ops, one and two chunks, two sources, one and two column blocks: both orders meet the halo family's
    bar, repeat bit for bit and leave the range status clear."""
    fails = [f for r in _of(rows, "grid") for f in _launch_fails(r)]
    assert not fails, "\n".join(fails)


def test_orders_are_two_different_summation_orders(rows):
    """The switch does select another loop: somewhere in the grid the two orders differ in the last bits (a case with a single
    chunk of K = 288 may well agree; all of them agreeing would mean the switch is not wired)."""
    assert not all(r["orders_equal"] for r in _of(rows, "grid"))


def test_residual_and_sliced_output(rows):
    fails = [f for r in _of(rows, "epilogue") for f in _launch_fails(r)]
    assert not fails, "\n".join(fails)


def test_batch_invariance(rows):
    """Sample 0 launched alone equals sample 0 of the batch of 3 bit for bit under a fixed routing batch."""
    got = [r for r in rows if "batch_invariant" in r]
    assert len(got) >= 10
    assert all(r["batch_invariant"] for r in got), [r["tag"] for r in got if not r["batch_invariant"]]


def test_fused_statistics_epilogue(rows):
    fails = []
    for r in _of(rows, "stats"):
        fails += _launch_fails(r)
        for a in ("on", "off"):
            o = r[a]
            if o["stats_over_bars"] or not o["conv_in_equal"] or not o["conv_in_finite"]:
                fails.append(f"{r['tag']}/{a}: {o}")
    assert not fails, "\n".join(fails)


def test_depth_to_space_store(rows):
    fails = [f for r in _of(rows, "d2s") for f in _launch_fails(r)]
    assert not fails, "\n".join(fails)


def test_tap_probe(rows):
    """Every (row, tap) pairing, exactly: one-hot weights at each of the nine taps copy the shifted padded input."""
    taps = _of(rows, "tap")
    bad = [(r["tag"], a) for r in taps for a in ("on", "off")
           if r[a]["family"] != cs.HALO or not r[a]["equal"] or r[a]["range"]]
    assert len(taps) == 9 * len(TAP_PADS) and not bad, bad


def test_neighbours_keep_their_loop(rows):
    """Dilated 3x3, 1x1, 5x5 and the stride-2 quadrant form run the halo family and do not depend on the switch."""
    for r in _of(rows, "neighbour"):
        assert r["family_on"] in HALO_FAMILIES and r["family_on"] == r["family_off"], r
        assert r["route_on"] == r["route_off"] == [r["family_on"], NEIGHBOUR_TILES[r["tag"]], 1, 0], r
        assert r["orders_equal"] and r["err"] <= r["bar"] and not r["range"], r


def test_range_guard(rows):
    (r,) = _of(rows, "range")
    for a in ("on", "off"):
        assert r[a] == {"family": cs.HALO, "clear_in_range": True, "raised": True, "cleared_by_read": True}, r


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        with torch.no_grad():
            _child(sys.argv[2])
    else:
        sys.exit("usage: test_gpu_halo_colmajor.py --child OUT.json")
