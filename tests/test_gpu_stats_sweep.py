"""GPU: the norm statistics of every conv epilogue (fused path) and of the streaming pass, against float64 (tests/stats_sweep.py).

Fused: every case of stats_sweep.stat_cases() at every precision it serves runs three times - plain, with statistics into a
caller's buffer at a slot offset (stats_into), with want_stats - and the combined slots are judged against the float64
statistics of the launch's own output under the derived bars; the slot finalisers are judged against float64 from the same
slots.  The launches that must not write statistics fall back (want_stats) or are rejected on the host (stats_into).
Streaming: fusg_chan_stats through the C ABI at the test's own chunk counts, the finalisers alone on synthetic slots."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import conv_sweep as cs
import stats_sweep as ss

pytestmark = pytest.mark.gpu

from future_urban_scene_generation_amd import _lib as L          # noqa: E402
from future_urban_scene_generation_amd import ops, pack           # noqa: E402

SENTINEL = 1234.5
FIRST, TAIL = 3, 2
NAME = {cs.GEN_F32: "gen_f32", cs.GEN_F16X3: "gen_f16x3", cs.HALO: "halo", cs.HALO_S2D: "halo_s2d", cs.HALO_F32: "halo_f32",
        cs.HALO_BF16: "halo_bf16", cs.TAPUNIT: "tapunit", cs.TAPUNIT_F32: "tapunit_f32", cs.TAPUNIT_BF16: "tapunit_bf16",
        cs.POINTWISE: "pointwise", cs.SMALL: "small", ss.HALO_F16: "halo_f16", ss.TAPUNIT_F16: "tapunit_f16"}
PER_CALL = ("FUSG_NO_SMALL", "FUSG_NO_POINTWISE", "FUSG_NO_F32_HALO", "FUSG_NO_BF16_TAPUNIT", "FUSG_SMALL_KSPLIT")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


class _env:
    """Per-call switches set for the duration of one launch (libfusg reads them per call)."""

    def __init__(self, env):
        self.env = dict(env or {})

    def __enter__(self):
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


def _prepare(tag: str, c: cs.Case, inp: dict):
    """Plan and device operands of a case, cached by tag."""
    if tag in _PREP:
        return _PREP[tag]
    plan = cs.make_plan(c, inp["w"], inp["b"])
    d = dev()
    S = {"plan": plan, "B": c.B}
    S["x0"] = ops.as_nhwc(inp["x0"].contiguous().to(d), cpad=c.cin_pad)
    S["x1"] = ops.as_nhwc(inp["x1"].contiguous().to(d), cpad=c.cin_pad) if c.c1 else None
    if c.pre.startswith("affine"):
        ctot = plan.c0k + plan.c1k

        def lay(v):                                       # logical channels -> the K layout's (src0 padded to c0k, then src1)
            o = torch.zeros(*v.shape[:-1], ctot)
            o[..., :c.c0] = v[..., :c.c0]
            o[..., plan.c0k:plan.c0k + c.c1] = v[..., c.c0:]
            return o.contiguous().to(d)
        S["pre"] = (lay(inp["scale"]), lay(inp["shift"]))
        S["pre_bstride"] = ctot if c.per_sample else 0
    S["res"] = [ops.as_nhwc(r.contiguous().to(d)) for r in inp["res"]]
    _PREP[tag] = S
    return S


def _kwargs(c: cs.Case, S: dict, prec: str, tile: int, ksplit: int, store: int = L.STORE_NORMAL, tiles: bool = False):
    """ops.conv's keywords of one launch of the case, with a fresh sentinel-filled destination where the case names one."""
    ho, wo = c.full_hw()
    kw = dict(pre_op=cs.PRE[c.pre], act=c.act, precision=prec, ksplit=ksplit, tile=tile, store=store)
    if "pre" in S:
        kw.update(pre=S["pre"], pre_bstride=S["pre_bstride"])
    for i, r in enumerate(S["res"]):
        kw["res%d" % i] = r
    if c.out == "nchw":
        kw["nchw_out"] = True
    elif c.out == "slice":
        out = ops.nhwc_empty(c.B, c.out_c_off + c.cout + 4, ho, wo, dev())
        out.fill_(SENTINEL)
        kw.update(out=out, out_c_off=c.out_c_off)
    elif c.out == "misaligned":
        buf = torch.full((c.B * ho * wo * c.cout + 1,), SENTINEL, device=dev())
        kw["out"] = buf[1:].view(c.B, ho, wo, c.cout).permute(0, 3, 1, 2)
        assert kw["out"].data_ptr() % 16 != 0
    if c.qwin or tiles:
        out = ops.nhwc_empty(c.B, c.cout, ho, wo, dev())
        out.fill_(SENTINEL)
        kw["out"] = out
        if c.qwin:
            kw["q_window"] = c.qwin
        if tiles:
            kw["tiles"] = ops.border_tiles(ho, wo, dev())
    return kw


def _result(c: cs.Case, raw: torch.Tensor) -> torch.Tensor:
    """The launch's own values [B, cout, qh, qw] out of what ops.conv returned, float64 on the CPU."""
    y = raw.detach().cpu().double()
    if c.out == "slice":
        y = y[:, c.out_c_off:c.out_c_off + c.cout]
    return cs.window(c, y).contiguous()


def _finalize_slots(stats: torch.Tensor, gamma=None, beta=None):
    b, n, ch, _ = stats.shape
    out = torch.empty((2, b, ch), device=stats.device, dtype=torch.float32)
    if gamma is None:
        L.check(L.lib().fusg_in_finalize_slots(stats.data_ptr(), b, n, ch, ss.EPS, out[0].data_ptr(), out[1].data_ptr(),
                                               ops.stream_ptr()), "in_finalize_slots")
    else:
        L.check(L.lib().fusg_ln_finalize_slots(stats.data_ptr(), b, n, ch, ss.EPS, gamma.data_ptr(), beta.data_ptr(),
                                               out[0].data_ptr(), out[1].data_ptr(), ops.stream_ptr()), "ln_finalize_slots")
    return out[0], out[1]


def _gamma_beta(ch: int):
    g = torch.Generator().manual_seed(ch)
    gamma, beta = torch.randn(ch, generator=g) + 1.5, torch.randn(ch, generator=g)
    return gamma, beta


RSTD_CONST = float(np.float32(1.0 / np.sqrt(np.float64(ss.EPS))))          # a constant channel's InstanceNorm scale

OBS = {}
_DONE = set()
PAIRS = [(sc, p) for sc in ss.stat_cases() for p in sc.precs]


def run_fused(sc: ss.StatCase, prec: str):
    """Every check of one case at one precision; returns the list of failures (empty: passed)."""
    from conftest import record
    fails = []
    c = sc.case
    S = _prepare(sc.tag.split("+tile")[0], c, ss.stat_inputs(sc))
    plan, x0, x1 = S["plan"], S["x0"], S["x1"]
    qh, qw = c.q_hw()
    n = qh * qw // 32
    where = f"{sc.tag}/{prec}"
    ops.range_exceeded(dev())                                   # (a clean status word)
    # ---- A: no statistics (with the families that refuse statistics switched off when it landed on one: same kernel as B)
    kw = _kwargs(c, S, prec, sc.tile, 1)
    out_a = ops.conv(plan, x0, x1, **kw)
    fam_a = ops.last_conv_kernel()
    env = {}
    if fam_a in ss.NO_STAT_FAMILIES:
        env = ss.STATS_ENV
        kw = _kwargs(c, S, prec, sc.tile, 1)
        with _env(env):
            out_a = ops.conv(plan, x0, x1, **kw)
            fam_a = ops.last_conv_kernel()
    raw_a = out_a.detach().cpu()
    y = _result(c, out_a)
    want_fam = ss.predict_stats_family(c, prec, sc.tile)
    if fam_a != want_fam:
        fails.append(f"{where}: ran family {fam_a}, the restated router says {want_fam}")
    # ---- B: statistics into a caller's buffer at a slot offset
    buf = torch.full((c.B, FIRST + n + TAIL, c.cout, 2), SENTINEL, device=dev())
    kw = _kwargs(c, S, prec, sc.tile, 1)
    out_b = ops.conv(plan, x0, x1, stats_into=(buf, FIRST), **kw)
    fam_b = ops.last_conv_kernel()
    if fam_b in ss.NO_STAT_FAMILIES or fam_b != fam_a:
        fails.append(f"{where}: with statistics family {fam_b}, without {fam_a}")
    if not torch.equal(out_b.detach().cpu(), raw_a):
        fails.append(f"{where}: output with stats_into not bit-equal to the plain launch")
    hb = buf.cpu()
    if not bool((hb[:, :FIRST] == SENTINEL).all() and (hb[:, FIRST + n:] == SENTINEL).all()):
        fails.append(f"{where}: wrote slots outside [first, first + n)")
    inner = hb[:, FIRST:FIRST + n]
    if bool((inner == SENTINEL).any()):
        fails.append(f"{where}: {int((inner == SENTINEL).sum())} slot values never written")
    if not bool(torch.isfinite(inner).all()) or float(inner[..., 1].min()) < 0.0:
        fails.append(f"{where}: M2 not finite / negative")
    if ops.range_exceeded(dev()):
        fails.append(f"{where}: range status raised")
    # ---- C: want_stats (the Python gate must agree with the library), independent of stats_slots
    kw = _kwargs(c, S, prec, sc.tile, 1)
    with _env(env):
        out_c, stats = ops.conv(plan, x0, x1, want_stats=True, **kw)
        fam_c = ops.last_conv_kernel()
    if stats is None:
        fails.append(f"{where}: ops.conv(want_stats=True) fell back on a launch that qualifies")
        return fails
    if fam_c != fam_b or not torch.equal(out_c.detach().cpu(), raw_a):
        fails.append(f"{where}: want_stats launch differs (family {fam_c})")
    if tuple(stats.shape) != (c.B, n, c.cout, 2) or not torch.equal(stats.cpu(), inner):
        fails.append(f"{where}: want_stats slots not bit-equal to the stats_into slots")
    # ---- the combined slots against the float64 statistics of the launch's own output
    hs = stats.cpu()
    got, ref = ss.combine(hs), ss.direct(y)
    e = ss.stat_errs(got, ref)
    print(f"{where}: family {NAME[fam_b]} errs {e}")
    o = OBS.setdefault((fam_b, prec), {"mean": 0.0, "var": 0.0, "cases": 0, "tiles": set(), "ksw": set()})
    o["mean"], o["var"] = max(o["mean"], e["mean"], e["ln_mean"]), max(o["var"], e["var"], e["ln_var"])
    o["cases"] += 1
    o["tiles"].add(sc.tile)
    o["ksw"].add(ss.halo_takes_ksplit(c, prec))
    record(f"stats_mean_{NAME[fam_b]}", max(e["mean"], e["ln_mean"]))
    record(f"stats_var_{NAME[fam_b]}", max(e["var"], e["ln_var"]))
    bad = ss.over_bars(e)
    if bad:
        fails.append(f"{where}: family {NAME[fam_b]} statistics over the bars: {bad}")
    if sc.variant == "zero_ch" and float(got["var"][:, ss.ZERO_CH].abs().max()) != 0.0:
        fails.append(f"{where}: constant channel's variance {float(got['var'][:, ss.ZERO_CH].abs().max()):.3e} != 0")
    # ---- the slot finalisers against float64 from the same slots
    gamma, beta = _gamma_beta(c.cout)
    gd, bd = gamma.to(dev()), beta.to(dev())
    in_ss = _finalize_slots(stats)
    ln_ss = _finalize_slots(stats, gd, bd)
    fe = ss.final_errs(*in_ss, ss.in_scale_shift(got["mean"], got["var"]))
    fl = ss.final_errs(*ln_ss, ss.ln_scale_shift(got["ln_mean"], got["ln_var"], gamma, beta))
    record("stats_finalize_slots", max(fe + fl))
    if max(fe + fl) > ss.BAR_FINAL:
        fails.append(f"{where}: slot finalisers off by {fe} (IN) {fl} (LN) > {ss.BAR_FINAL:.3e}")
    if sc.variant == "zero_ch":
        sc_const = in_ss[0].cpu()[:, ss.ZERO_CH]
        st = ops.instnorm_stats(out_a if c.out != "slice" else out_a[:, c.out_c_off:c.out_c_off + c.cout])[0].cpu()[:, ss.ZERO_CH]
        if not bool((sc_const == RSTD_CONST).all()) or not bool((st == RSTD_CONST).all()):
            fails.append(f"{where}: constant channel's scale {sc_const.tolist()} (fused) {st.tolist()} (streaming) != {RSTD_CONST!r}")
    # ---- conv_in / conv_ln on the same operands: the same (scale, shift), bit for bit
    with _env(env):
        _, ci = ops.conv_in(plan, x0, ss.EPS, **dict(_kwargs(c, S, prec, sc.tile, 1), x1=x1))
        _, cl = ops.conv_ln(plan, x0, gd, bd, ss.EPS, **dict(_kwargs(c, S, prec, sc.tile, 1), x1=x1))
    for name, a, b in (("conv_in", ci, in_ss), ("conv_ln", cl, ln_ss)):
        if not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])):
            fails.append(f"{where}: ops.{name} differs from finalising the launch's statistics")
    _DONE.add((sc.tag, prec))
    return fails


@pytest.mark.parametrize("sc,prec", PAIRS, ids=[f"{sc.tag}-{p}" for sc, p in PAIRS])
def test_fused_stats(sc, prec):
    fails = run_fused(sc, prec)
    assert not fails, "\n".join(fails)


def test_fused_stats_cover_every_family():
    """After the sweep: every family that can write statistics did, at each precision it serves and - the generic gathers - on
    each tile; both epilogues of the halo body ran; the worst errors per family go to the parity log."""
    from conftest import record
    for sc, prec in PAIRS:
        if (sc.tag, prec) not in _DONE and sc.variant == "plain":
            run_fused(sc, prec)
    want = {(cs.GEN_F32, "f32"), (cs.GEN_F16X3, "f16x3"), (cs.GEN_F16X3, "bf16"), (cs.HALO, "f16x3"), (cs.HALO_S2D, "f16x3"),
            (cs.HALO_F32, "f32"), (cs.HALO_BF16, "bf16"), (cs.TAPUNIT, "f16x3"), (cs.TAPUNIT_F32, "f32"),
            (cs.TAPUNIT_BF16, "bf16"), (ss.HALO_F16, "f16"), (ss.TAPUNIT_F16, "f16")}
    assert want <= set(OBS), want - set(OBS)
    assert not any(f in ss.NO_STAT_FAMILIES for f, _ in OBS)
    for (fam, prec), o in sorted(OBS.items()):
        record(f"stats_mean_{NAME[fam]}_{prec}", o["mean"])
        record(f"stats_var_{NAME[fam]}_{prec}", o["var"])
        record(f"stats_cases_{NAME[fam]}_{prec}", o["cases"])
        print(f"{NAME[fam]}/{prec}: {o}")
        assert o["mean"] <= ss.BAR_MEAN and o["var"] <= ss.BAR_VAR, (fam, prec, o)
    for prec, fam in (("f32", cs.GEN_F32), ("f16x3", cs.GEN_F16X3)):
        assert {1, 2, 3, 4, 5} <= OBS[(fam, prec)]["tiles"], OBS[(fam, prec)]["tiles"]
    for key in ((cs.HALO, "f16x3"), (cs.HALO_F32, "f32"), (cs.HALO_BF16, "bf16"), (ss.HALO_F16, "f16")):
        assert {True, False} <= OBS[key]["ksw"], (key, OBS[key]["ksw"])


# ---- the wide column tiles of the halo body: a switch cached per process, so a fresh child process ------------------------
HALO_FAMILIES = (cs.HALO, cs.HALO_S2D, cs.HALO_F32, cs.HALO_BF16, ss.HALO_F16)


def halo_pairs():
    return [(sc, p) for sc, p in PAIRS if sc.tag.startswith("st_") and ss.predict_stats_family(sc.case, p, sc.tile) in HALO_FAMILIES]


def _child(out_path):
    fails = []
    for sc, prec in halo_pairs():
        fails += run_fused(sc, prec)
    obs = {f"{NAME[f]}/{p}": {"mean": o["mean"], "var": o["var"], "cases": o["cases"]} for (f, p), o in OBS.items()}
    with open(out_path, "w") as f:
        json.dump({"fails": fails, "obs": obs}, f)


def test_halo_stats_on_the_wide_column_tiles():
    """On grids this small the launcher narrows the halo kernel's column tile to 32 (FUSG_HALO_MINWG, default 512
    workgroups), so the sweep above runs the 32-column instantiations only.  FUSG_HALO_MINWG=1 (read once per process) keeps
    the widest tile: the 64- and 128-column instantiations - other shuffle strides in epilogue_rows, the 64-column K-split
    epilogue, and the bf16 kernel's tile that leaves in two halves - run the halo rows of the table in one fresh child."""
    from conftest import record
    env = {k: v for k, v in os.environ.items() if k not in PER_CALL}
    env["FUSG_HALO_MINWG"] = "1"
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "rows.json")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", out]
        p = subprocess.run(cmd, env=env, timeout=300, capture_output=True, text=True,
                           cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
        with open(out) as f:
            res = json.load(f)
    assert not res["fails"], "\n".join(res["fails"])
    assert {"halo/f16x3", "halo_s2d/f16x3", "halo_f32/f32", "halo_bf16/bf16", "halo_f16/f16"} <= set(res["obs"]), sorted(res["obs"])
    for k, o in res["obs"].items():
        record(f"stats_mean_wide_{k.replace('/', '_')}", o["mean"])
        record(f"stats_var_wide_{k.replace('/', '_')}", o["var"])
        assert o["mean"] <= ss.BAR_MEAN and o["var"] <= ss.BAR_VAR and o["cases"] > 0, (k, o)


# ---- launches that must not write statistics ---------------------------------------------------------------------------
NEG = [(n, c, kw, p) for n, c, kw in ss.negative_cases() for p in cs.PRECISIONS]


@pytest.mark.parametrize("name,c,extra,prec", NEG, ids=[f"{n}-{p}" for n, _, _, p in NEG])
def test_non_qualifying_launch_falls_back_or_is_rejected(name, c, extra, prec):
    """want_stats: (out, None) with the plain launch's bits.  stats_into: rejected on the host, nothing written."""
    S = _prepare(c.tag, c, cs.inputs(c))
    plan, x0 = S["plan"], S["x0"]
    store, tiles = extra.get("store", L.STORE_NORMAL), bool(extra.get("tiles"))
    assert not ss.qualifies(c, ksplit=c.ksplit, prec=prec, store=store, tiles=tiles)
    out = ops.conv(plan, x0, **_kwargs(c, S, prec, 0, c.ksplit, store, tiles))
    fam = ops.last_conv_kernel()
    out2, stats = ops.conv(plan, x0, want_stats=True, **_kwargs(c, S, prec, 0, c.ksplit, store, tiles))
    assert stats is None, name
    assert ops.last_conv_kernel() == fam and torch.equal(out2.cpu(), out.cpu())
    qh, qw = c.q_hw()
    buf = torch.full((c.B, max(1, qh * qw // 32), plan.cout, 2), SENTINEL, device=dev())
    with pytest.raises((L.FusgError, AssertionError)):
        ops.conv(plan, x0, stats_into=(buf, 0), **_kwargs(c, S, prec, 0, c.ksplit, store, tiles))
    assert bool((buf == SENTINEL).all())
    assert not ops.range_exceeded(dev())


# ---- transposed conv: four phase launches into one buffer ----------------------------------------------------------------
@pytest.mark.parametrize("prec", cs.PRECISIONS)
@pytest.mark.parametrize("hw", [(8, 16), (16, 32)], ids=lambda s: "%dx%d" % s)
def test_transposed_conv_phase_stats(hw, prec):
    from conftest import record
    H, W = hw
    g = torch.Generator().manual_seed(H)
    x = torch.randn(2, 32, H, W, generator=g)
    w = torch.randn(32, 48, 4, 4, generator=g) * 0.09
    b = torch.randn(48, generator=g) * 3                      # (mean a few std)
    phases = pack.pack_conv_transpose_k4s2p1_phases(w, b)
    xd = ops.as_nhwc(x.to(dev()))
    plain = ops.conv_transpose_phases(phases, xd, precision=prec)
    out, stats = ops.conv_transpose_phases(phases, xd, want_stats=True, precision=prec)
    fam = ops.last_conv_kernel()
    assert fam == {"f32": cs.HALO_F32, "f16x3": cs.HALO, "bf16": cs.HALO_BF16}[prec]
    assert stats is not None and tuple(stats.shape) == (2, 4 * H * W // 32, 48, 2)
    assert torch.equal(out.cpu(), plain.cpu())
    hs = stats.cpu()
    assert bool(torch.isfinite(hs).all()) and float(hs[..., 1].min()) >= 0.0
    got = ss.combine(hs)
    e = ss.stat_errs(got, ss.direct(out.cpu().double()))
    print(f"transposed {H}x{W}/{prec}: {e}")
    record(f"stats_mean_transposed_{NAME[fam]}", max(e["mean"], e["ln_mean"]))
    record(f"stats_var_transposed_{NAME[fam]}", max(e["var"], e["ln_var"]))
    assert not ss.over_bars(e), e
    _, (sc, sh) = ops.conv_in(phases, xd, ss.EPS, precision=prec)
    fe = ss.final_errs(sc, sh, ss.in_scale_shift(got["mean"], got["var"]))
    assert max(fe) <= ss.BAR_FINAL, fe
    assert not ops.range_exceeded(dev())


# ---- the slot finalisers alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ss.FINAL_SHAPES, ids=lambda s: "b%d_n%d_c%d" % s)
def test_slot_finalisers_on_synthetic_slots(shape):
    """fusg_in_finalize_slots / fusg_ln_finalize_slots against float64 InstanceNorm / the ICN's LayerNorm of values whose
    exact slot statistics are the uploaded fp32 slots (mean up to 1000 std, a constant channel; nslots below and above the 16
    slot lanes, C off the 16-channel block, nslots * C below and above the LayerNorm block's 1024 threads)."""
    from conftest import record
    B, n, ch = shape
    slots, y = ss.synthetic_slots(B, n, ch)
    ref = ss.direct(y)
    sd = slots.to(dev())
    guard = torch.full((2, B, ch + 8), SENTINEL, device=dev())          # (the c >= C guard: nothing past channel C - 1)
    L.check(L.lib().fusg_in_finalize_slots(sd.data_ptr(), B, n, ch, ss.EPS, guard[0].data_ptr(), guard[1].data_ptr(),
                                           ops.stream_ptr()), "in_finalize_slots")
    flat = guard.cpu().reshape(2, -1)
    assert bool((flat[:, B * ch:] == SENTINEL).all())
    sc, sh = flat[0, :B * ch].reshape(B, ch), flat[1, :B * ch].reshape(B, ch)
    fe = ss.final_errs(sc, sh, ss.in_scale_shift(ref["mean"], ref["var"]))
    assert bool((sc[:, ss.CONST_CH] == RSTD_CONST).all()), sc[:, ss.CONST_CH].tolist()
    gamma, beta = _gamma_beta(ch)
    lsc, lsh = _finalize_slots(sd, gamma.to(dev()), beta.to(dev()))
    fl = ss.final_errs(lsc, lsh, ss.ln_scale_shift(ref["ln_mean"], ref["ln_var"], gamma, beta))
    print(f"finalisers b{B} n{n} c{ch}: IN {fe} LN {fl}")
    record("finalize_slots_in", max(fe))
    record("finalize_slots_ln", max(fl))
    assert max(fe) <= ss.BAR_FINAL and max(fl) <= ss.BAR_FINAL, (fe, fl)


# ---- the streaming path through the C ABI --------------------------------------------------------------------------------
def _chan_device(cc: ss.ChanCase, x: torch.Tensor) -> torch.Tensor:
    xd = x.to(dev())
    if cc.kind == "cpad32":
        t = ops.as_nhwc(xd, cpad=32)
        assert t.stride(3) == 32 and t.shape[1] == cc.C
        return t
    if cc.kind == "slice":
        h, w = x.shape[2:]
        wide = ops.nhwc_empty(cc.B, cc.C + 16, h, w, dev())
        wide.fill_(1e6)
        t = wide[:, 8:8 + cc.C]
        t.copy_(xd)
        return t
    return ops.as_nhwc(xd)


def _chan_partial(xd: torch.Tensor, n: int):
    B, ch = xd.shape[:2]
    flat = torch.full((B * n * ch * 2 + 64,), SENTINEL, device=dev())
    L.check(L.lib().fusg_chan_stats(C.byref(ops.desc(xd)), flat.data_ptr(), n, ops.stream_ptr()), "chan_stats")
    return flat, flat[:B * n * ch * 2].view(B, n, ch, 2)


def _chan_finalize(xd, partial, n, gamma=None, beta=None):
    B, ch = xd.shape[:2]
    out = torch.empty((2, B, ch), device=dev(), dtype=torch.float32)
    if gamma is None:
        L.check(L.lib().fusg_in_finalize(C.byref(ops.desc(xd)), partial.data_ptr(), n, ss.EPS, out[0].data_ptr(),
                                         out[1].data_ptr(), ops.stream_ptr()), "in_finalize")
    else:
        L.check(L.lib().fusg_ln_finalize(C.byref(ops.desc(xd)), partial.data_ptr(), n, ss.EPS, gamma.data_ptr(), beta.data_ptr(),
                                         out[0].data_ptr(), out[1].data_ptr(), ops.stream_ptr()), "ln_finalize")
    return out[0], out[1]


@pytest.mark.parametrize("cc", ss.chan_cases(), ids=lambda cc: cc.tag)
def test_chan_stats_at_the_tests_own_nchunk(cc):
    from conftest import record
    x = ss.chan_input(cc)
    xd = _chan_device(cc, x)
    one = cc.C * cc.hw == 1
    gamma, beta = _gamma_beta(cc.C)
    gd, bd = gamma.to(dev()), beta.to(dev())
    worst, fails = 0.0, []
    for n in ss.chan_nchunks(cc.hw):
        flat, partial = _chan_partial(xd, n)
        hp = flat.cpu()
        assert bool((hp[-64:] == SENTINEL).all()), f"nchunk {n}: wrote past the partial sums"
        hp = hp[:-64].view(cc.B, n, cc.C, 2)
        assert not bool((hp == SENTINEL).any()) and bool(torch.isfinite(hp).all()), f"nchunk {n}: partial sums missing"
        got = ss.chan_combine(hp, x)
        e = ss.chan_errs(got, x)
        if one:
            e = {k: v for k, v in e.items() if not k.startswith("ln_")}
        worst = max(worst, *e.values())
        if max(e.values()) > ss.BAR_CHAN:
            fails.append(f"nchunk {n}: {e}")
        fe = ss.final_errs(*_chan_finalize(xd, partial, n), ss.in_scale_shift(got["mean"], got["var"]))
        fl = (0.0, 0.0) if one else ss.final_errs(*_chan_finalize(xd, partial, n, gd, bd),
                                                  ss.ln_scale_shift(got["ln_mean"], got["ln_var"], gamma, beta))
        record("chan_finalize", max(fe + fl))
        if max(fe + fl) > ss.BAR_FINAL:
            fails.append(f"nchunk {n}: finalisers IN {fe} LN {fl}")
    print(f"{cc.tag}: worst {worst:.3e}")
    record("chan_stats_pivot_outlier" if cc.kind == "outlier" else "chan_stats", worst)
    assert not fails, "\n".join(fails)


def _wrapper_errs(cc: ss.ChanCase):
    x = ss.chan_input(cc)
    xd = _chan_device(cc, x)
    gamma, beta = _gamma_beta(cc.C)
    gd, bd = gamma.to(dev()), beta.to(dev())
    _, partial = _chan_partial(xd, 1)
    ref = ss.direct(x)
    rstd = 1.0 / torch.sqrt(ref["var"] + ss.EPS)
    a = [t.cpu().double() for t in _chan_finalize(xd, partial, 1)]
    e_in = ss.final_errs(*ops.instnorm_stats(xd, ss.EPS), (a[0], a[1], ref["mean"].abs() * rstd))
    b = [t.cpu().double() for t in _chan_finalize(xd, partial, 1, gd, bd)]
    e_ln = ss.final_errs(*ops.layernorm_stats(xd, gd, bd, ss.EPS),
                         (b[0], b[1], ref["ln_mean"].abs()[:, None] * b[0].abs() + beta.double().abs()[None]))
    return e_in, e_ln


@pytest.mark.parametrize("shape", ss.WRAPPER_SHAPES, ids=lambda s: "c%d_hw%d" % s)
def test_wrappers_nchunk_against_the_direct_abi(shape):
    """ops.instnorm_stats / ops.layernorm_stats (their own nchunk > 1) against the direct ABI at nchunk = 1, on the inputs for
    which one chunk is a fair reference (stats_sweep.WRAPPER_SHAPES: the derivation).  The plain inputs of the same shapes are
    measured and recorded: there the one-chunk run's own fp32 error is of the size of the bar (up to 4.7e-6 at C = 260,
    HW = 4096 against 9.5e-7), which says nothing about the wrappers."""
    from conftest import record
    C_, hw = shape
    assert ops._nchunk(2, C_, hw) > 1
    e_in, e_ln = _wrapper_errs(ss.ChanCase(C_, hw, 2, "centred"))
    p_in, p_ln = _wrapper_errs(ss.ChanCase(C_, hw, 2))
    print(f"wrappers c{C_} hw{hw}: centred IN {e_in} LN {e_ln}; plain IN {p_in} LN {p_ln}")
    record("chan_stats_wrapper_vs_nchunk1", max(e_in + e_ln))
    record("chan_stats_wrapper_vs_nchunk1_plain_input", max(p_in + p_ln))
    assert max(e_in + e_ln) <= ss.BAR_WRAPPER, (e_in, e_ln)


def test_streaming_arguments_are_checked_on_the_host():
    d = dev()
    partial = torch.full((2 * 8 * 2 * 8,), SENTINEL, device=d)
    x6 = ops.as_nhwc(torch.zeros(2, 6, 4, 4, device=d))
    x8 = ops.as_nhwc(torch.ones(2, 8, 4, 4, device=d))
    for xd, n in ((x6, 1), (x8, 0), (x8, 4097), (x8, -1)):
        rc = L.lib().fusg_chan_stats(C.byref(ops.desc(xd)), partial.data_ptr(), n, ops.stream_ptr())
        with pytest.raises(L.FusgError):
            L.check(rc, "chan_stats")
    x1 = ops.as_nhwc(torch.ones(2, 1, 1, 1, device=d))
    out = torch.full((2, 2, 4), SENTINEL, device=d)
    gb = torch.ones(4, device=d)
    rc = L.lib().fusg_ln_finalize(C.byref(ops.desc(x1)), partial.data_ptr(), 1, ss.EPS, gb.data_ptr(), gb.data_ptr(),
                                  out[0].data_ptr(), out[1].data_ptr(), ops.stream_ptr())
    with pytest.raises(L.FusgError):
        L.check(rc, "ln_finalize")
    torch.cuda.synchronize()
    assert bool((partial == SENTINEL).all()) and bool((out == SENTINEL).all())


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        with torch.no_grad():
            _child(sys.argv[2])
    else:
        sys.exit("usage: test_gpu_stats_sweep.py --child OUT.json")
