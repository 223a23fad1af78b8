"""GPU: the single-pass fp16 precision mode ("f16", FUSG_PREC_F16: the halo kernel's MODE 3 and the tap-unit kernel's).

On a launch that takes family 15 / 16 the result is held to the mode's OWN arithmetic (f16_cases.reference_f16: operands
rounded to fp16, exact products) at conv_sweep.BAR_FP32, the project's bar for "same operands, fp32 accumulation order" -
tests/test_f16_mode_cpu.py shows that this reference is > 10 bars away from the exact result on every shape of the table, so
a kernel that ran f16x3 instead cannot pass.  ELU rows (no operand-exact reference) are held to the exact result at the
operand-rounding bound (1 + 2^-11)^2 - 1.  On every other family the launch must be the f16x3 launch, bit for bit.  Then the
range guard, the module-level fp32 redo, the image networks against the reference's golden vectors (no worse than bf16, SSIM
>= 0.999), the hourglass (f16x3 inside: same bytes) and the pipeline's compare_precisions.

The instantiation table (f16_cases.tile_cases; tests/test_f16_mode_cpu.py shows what it reaches and how sharp its references are)
runs in this process and in one fresh child process per non-empty set of f16_cases.SWITCH_SETS - the library reads
FUSG_HALO_MINWG / FUSG_NO_KSPLIT once per process - so that each of the 63 MODE 3 kernel instantiations is launched and judged
against the mode's own arithmetic.  Then the operand scales (fp16 subnormal activations), the NaN rule, and the DepthToSpace /
SpaceToDepth / tile-list launches under both single-pass modes."""
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
import f16_cases as fc

pytestmark = pytest.mark.gpu

from conftest import load_golden, record                          # noqa: E402
from test_gpu_conv_sweep import SENTINEL, _launch, _prepare, dev   # noqa: E402
from future_urban_scene_generation_amd import _lib as L           # noqa: E402
from future_urban_scene_generation_amd import ops, pack           # noqa: E402

EXTRA = fc.EXTRA
WORST = {}


def _same_launch_f16x3(c, S, fam):
    """The f16x3 launch of the case with the tile and K split the f16 launch planned: ops.conv plans an "f16" launch with the
    bf16 rule (128-row tiles), and on the generic gathers the tile and the K split fix the order of the sums."""
    if fam in (cs.SMALL, cs.POINTWISE):                        # (these plan their own tile; K whole)
        return _launch(c, S, "f16x3")
    ho, wo = c.q_hw()
    tile, ks = cs.plan_ksplit(S["B"] * ho * wo, S["plan"].cout_pad, S["plan"].k_pad, False, 0, c.ksplit)
    return _launch(c, S, "f16x3", ksplit=ks, tile=tile)


@pytest.mark.parametrize("c", cs.edge_cases() + fc.table_cases() + EXTRA, ids=lambda c: c.tag)
def test_f16_sweep(c):
    S = _prepare(c)
    ops.range_exceeded(dev())
    want = fc.predict_family(c)
    y, fam, rest = _launch(c, S, "f16")
    assert fam == want, (fam, want)
    assert not ops.range_exceeded(dev()), "range status raised"
    assert not rest.numel() or bool((rest == SENTINEL).all()), "wrote outside its output"
    y2, fam2, rest2 = _launch(c, S, "f16")
    assert fam2 == fam and torch.equal(y, y2), "repeat launch not bit-identical"
    assert bool((rest2 == SENTINEL).all()), "repeat launch wrote outside its output"
    exact = cs.norm_err(y, S["ref"], S["den"])
    print(f"{c.tag}: family {fam}, error against the exact reference {exact:.3e}")
    if fam in fc.F16_FAMILIES:
        rf = fc.reference_f16(c, cs.inputs(c))
        if rf is None:                                         # ELU: the operand-rounding bound against the exact result
            print(f"{c.tag}: ELU row, bound {fc.BAR_F16:.3e}")
            WORST[("elu", fam)] = max(WORST.get(("elu", fam), 0.0), exact)
            record(f"family{fam}_elu_err_vs_exact", exact)
            assert exact <= fc.BAR_F16, (c.tag, exact)
        else:
            e = cs.norm_err(y, cs.window(c, rf[0]), cs.window(c, rf[1]))
            print(f"{c.tag}: error against the fp16-operand reference {e:.3e} (bar {cs.BAR_FP32:.3e})")
            WORST[("ops", fam)] = max(WORST.get(("ops", fam), 0.0), e)
            record(f"family{fam}_f16_operands_err", e)
            record(f"family{fam}_err_vs_exact", exact)
            assert e <= cs.BAR_FP32, (c.tag, fam, e)
            assert exact <= fc.BAR_F16, (c.tag, exact)
    else:
        y3, fam3, _ = _same_launch_f16x3(c, S, fam)
        assert fam3 == fam, (fam3, fam)
        assert torch.equal(y, y3), f"family {fam}: not the f16x3 launch's bytes"
        assert exact <= cs.BAR_FP32, (c.tag, exact)
    if fam == fc.TAPUNIT_F16:                                  # the switch keeps the stem on the split-fp16 kernel
        import os
        os.environ["FUSG_NO_F16_TAPUNIT"] = "1"
        try:
            y4, fam4, _ = _launch(c, S, "f16")
        finally:
            del os.environ["FUSG_NO_F16_TAPUNIT"]
        assert fam4 == cs.TAPUNIT and cs.norm_err(y4, S["ref"], S["den"]) <= cs.BAR_FP32


def test_f16_sweep_reached_both_families():
    for fam in fc.F16_FAMILIES:
        assert ("ops", fam) in WORST, WORST
        record(f"family{fam}_f16_operands_err_max", WORST[("ops", fam)])
        assert WORST[("ops", fam)] <= cs.BAR_FP32


def _one_patch():
    g = torch.Generator().manual_seed(77)
    w = torch.randn(32, 32, 3, 3, generator=g) * 0.05
    x = torch.randn(1, 32, 8, 16, generator=g)
    return pack.pack_conv(w, None, pad=1), x


def test_range_guard_on_the_one_patch_layer():
    """f16x3's rule, unchanged: a staged |a| >= 2^15 or a non-finite one raises the status word, taken after the pre-op and a
    fused ReLU's floor; nothing below 2^15 does.  (The flagged launch's bytes are unspecified.)"""
    plan, x = _one_patch()

    def run(v, pre=L.PRE_NONE):
        xx = x.clone()
        xx[0, 17, 4, 5] = v
        ops.range_exceeded(dev())
        y = ops.conv(plan, ops.as_nhwc(xx.to(dev())), pre_op=pre, precision="f16", ksplit=1)
        assert ops.last_conv_kernel() == fc.HALO_F16
        return y, ops.range_exceeded(dev())
    assert run(40000.0)[1]
    y, hit = run(30000.0)
    assert not hit and bool(torch.isfinite(y).all())
    y, hit = run(-40000.0, L.PRE_RELU)
    assert not hit and bool(torch.isfinite(y).all())
    assert run(-40000.0)[1]
    assert run(float("inf"))[1]
    assert run(float("-inf"))[1]
    assert not run(1.0)[1]
    assert not ops.range_exceeded(dev())


def test_module_redo_in_fp32_from_the_new_mode():
    """The existing guard, reached from "f16": the ICN on inputs scaled until a staged operand passes 2^15 returns the bytes of
    the same call in exact fp32."""
    from test_gpu_nets import model
    from future_urban_scene_generation_amd.synth import synth_inputs
    icn = model("icn")
    x = synth_inputs("icn", 2, 64)["x"]
    xs = (x * (40000.0 / float(x.abs().max()))).to(dev())
    assert float(xs.abs().max()) >= 2.0 ** 15
    ops.range_exceeded(dev())
    with ops.precision("f16"), ops.defer_range_check():
        icn(xs)
        assert ops.range_exceeded(dev()), "the scaled input did not leave the range"
    with ops.precision("f16"):
        got = icn(xs)
    with ops.precision("f32"):
        want = icn(xs)
    assert torch.equal(got, want)
    assert not ops.range_exceeded(dev())


def _errs(out, gold):
    d = out.detach().cpu().double() - torch.as_tensor(gold).double()
    top = float(np.abs(gold).max())
    return float(d.abs().max()) / top, float(d.pow(2).mean().sqrt()) / top


def test_networks_no_worse_than_bf16_and_within_the_image_bar(monkeypatch):
    """ICN, VUnet first frame and EdgeConnect on the 256 x 256 fixtures (seeds and call sequence of test_gpu_nets.
    test_reduced_precision_evidence) under "bf16" and "f16", against the reference's golden vectors: each network puts at least
    one launch on family 15, every float output's relative max error and RMS error under f16 are no larger than under bf16
    (11 significant bits per operand against 8: the expected ratio is ~1/8, left as margin), and every uint8 output keeps the
    bar the suite states for bf16, SSIM >= 0.999."""
    import oracle
    from test_gpu_nets import manifest_seed, model
    from conftest import synth_sd
    from future_urban_scene_generation_amd.edgeconnect.models import EdgeModel, InpaintingModel
    from future_urban_scene_generation_amd.synth import synth_inputs
    DEV = dev()
    fams = []
    real_conv = ops.conv

    def conv(*a, **k):
        y = real_conv(*a, **k)
        fams.append(ops.last_conv_kernel())
        return y
    monkeypatch.setattr(ops, "conv", conv)
    g, gv, ge = load_golden("icn_b1_r256"), load_golden("vunet_b1_r256"), load_golden("ec_b1_r256")
    x = synth_inputs("icn", 1, 256)["x"].to(DEV)
    vu, i = model("vunet"), synth_inputs("vunet", 1, 256)
    e = synth_inputs("edge", 1, 256)
    em, im = EdgeModel(None), InpaintingModel(None)
    em.generator.load_state_dict(synth_sd("edge"))
    im.generator.load_state_dict(synth_sd("inpaint"))
    em, im = em.to(DEV).eval(), im.to(DEV).eval()
    res = {}
    for prec, halo in (("bf16", cs.HALO_BF16), ("f16", fc.HALO_F16)):
        with ops.precision(prec):
            del fams[:]
            out = model("icn")(x)
            assert halo in fams, (prec, "icn", sorted(set(fams)))
            del fams[:]
            torch.manual_seed(manifest_seed("vunet_b1_r256"))
            eo, es = vu.forward_enc_up(i["x"].to(DEV))
            mu_app, _ = vu.forward_enc_down(eo, es)
            do, ds = vu.forward_dec_up(i["y_tilde"].to(DEV))
            xt = vu.forward_dec_down(do, ds, mu_app)[0]
            assert halo in fams, (prec, "vunet", sorted(set(fams)))
            del fams[:]
            ed = em(e["gray"].to(DEV), e["edge"].to(DEV), e["mask"].to(DEV))
            pp = im(e["img"].to(DEV), ed, e["mask"].to(DEV))
            assert halo in fams, (prec, "edgeconnect", sorted(set(fams)))
            mu8 = ops.merge_u8(pp, e["img"].to(DEV), e["mask"].to(DEV)).cpu().numpy()
        imgs = {"icn": (ops.to_image_u8(out).cpu().numpy(), g["img_u8"]), "vunet": (ops.to_image_u8(xt).cpu().numpy(), gv["img_u8"]),
                "inpaint": (mu8, ge["merged_u8"])}
        flt = {"icn": _errs(out, g["out"]), "vunet": _errs(xt, gv["x_tilde"]), "inpaint": _errs(pp, ge["inpaint_out"])}
        res[prec] = {}
        for k in imgs:
            a, b = imgs[k]
            ss, d = float(oracle.ssim(a, b)), int(np.abs(a.astype(int) - b.astype(int)).max())
            res[prec][k] = (flt[k][0], flt[k][1], ss, d)
            print(f"{prec} {k}: rel max err {flt[k][0]:.3e}  rms err {flt[k][1]:.3e}  ssim {ss:.6f}  u8 max diff {d}")
            record(f"{prec}_{k}_rel_err", flt[k][0])
            record(f"{prec}_{k}_rms_err", flt[k][1])
            record(f"{prec}_{k}_ssim", ss, worst=min)
            record(f"{prec}_{k}_u8_max_diff", d)
    for k in ("icn", "vunet", "inpaint"):
        f, b = res["f16"][k], res["bf16"][k]
        assert f[0] <= b[0] and f[1] <= b[1], (k, f, b)
        assert f[2] >= 0.999, (k, f)


def test_hourglass_keeps_f16x3_under_f16():
    from test_gpu_nets import model
    from future_urban_scene_generation_amd.synth import synth_inputs
    gh = load_golden("hg_b1_r256")
    hx = synth_inputs("hg", 1, 256)["x"].to(dev())
    with ops.precision("f16x3"):
        a = model("hg")(hx)["heatmaps"]
    with ops.precision("f16"):
        b = model("hg")(hx)["heatmaps"]
        assert ops.PRECISION == "f16"
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    ia, ib = ops.argmax_hw(a[-1]).cpu().numpy(), ops.argmax_hw(b[-1]).cpu().numpy()
    assert np.array_equal(ia, ib) and np.array_equal(ib.astype(np.int64), gh["argmax"])


def test_pipeline_compare_precisions_f16():
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline, synth_batch
    pipe = VehiclePipeline(dev())
    batch = synth_batch(2, 256, dev())
    before = ops.PRECISION
    rep = pipe.compare_precisions(batch, [7, 8], "f16")
    assert ops.PRECISION == before
    assert rep["kp_equal"].tolist() == [12, 12]                # kp_idx identical in both passes
    for k in ("icn_u8", "vunet_u8"):
        assert rep[k]["ssim"].shape == (2,) and np.isfinite(rep[k]["ssim"]).all() and np.isfinite(rep[k]["max_abs"]).all()
        assert not np.isnan(rep[k]["psnr"]).any()
        print(k, "f16 vs f16x3: ssim", rep[k]["ssim"], "psnr", rep[k]["psnr"], "max_abs", rep[k]["max_abs"])
        record(f"{k}_ssim_f16_vs_f16x3", rep[k]["ssim"].min(), worst=min)
        record(f"{k}_max_abs_f16_vs_f16x3", rep[k]["max_abs"].max())
        assert rep["worst"][k]["ssim"] >= 0.999


# ---- the instantiation table under the process-wide switches -------------------------------------------------------------
class _capture:
    """Keeps the descriptor of the ops.conv launch issued inside (planned by ops.conv before the launch)."""

    def __enter__(self):
        self.real, self.d = ops._conv_desc, None

        def desc(*a, **k):
            d, out = self.real(*a, **k)
            self.d = d
            return d, out
        ops._conv_desc = desc
        return self

    def __exit__(self, *exc):
        ops._conv_desc = self.real
        return False

    def route_order(self):
        out = (C.c_int32 * 4)()
        rc = L.lib().fusg_conv2d_route_order(C.byref(self.d), C.byref(out))
        assert rc == 0, (rc, L.lib().fusg_last_error())
        return [int(v) for v in out]


def _routed_launch(c, S, prec="f16"):
    with _capture() as cap:
        y, fam, rest = _launch(c, S, prec)
        return y, fam, rest, cap.route_order()


def table_row(c):
    """Every figure the table's checks need from one row: the launch, its repeat, and for B >= 2 the last sample alone."""
    S = _prepare(c)
    ops.range_exceeded(dev())
    pred = fc.cpu_route_order(c)                                # the library's dry run on CPU tensors, this process's switches
    y, fam, rest, route = _routed_launch(c, S)
    rng = bool(ops.range_exceeded(dev()))
    y2, fam2, rest2 = _launch(c, S, "f16")
    inst, pinst = fc.instantiation(c, route), fc.instantiation(c, pred)
    # slice, q-window and misaligned outputs come with sentinels (a misaligned one: cs.GUARD + 1 before it, cs.GUARD after it),
    # read back after the launch and after its repeat; the other outputs are ops.conv's own allocation
    guarded = c.out in ("slice", "misaligned") or bool(c.qwin)
    assert bool(rest.numel()) == bool(rest2.numel()) == guarded, (c.tag, rest.numel(), rest2.numel())
    row = {"tag": c.tag, "family": fam, "route": route, "pred": pred, "inst": None if inst is None else list(inst),
           "pred_inst": None if pinst is None else list(pinst), "range": rng,
           "sentinel_ok": bool((rest == SENTINEL).all()) and bool((rest2 == SENTINEL).all()),
           "repeat_equal": bool(fam2 == fam and torch.equal(y, y2)), "err_exact": cs.norm_err(y, S["ref"], S["den"]), "err_ops": None}
    if fam in fc.F16_FAMILIES:
        rf = fc.reference_f16(c, cs.inputs(c))
        if rf is not None:
            row["err_ops"] = cs.norm_err(y, cs.window(c, rf[0]), cs.window(c, rf[1]))
    if c.B >= 2 and fam in fc.F16_FAMILIES:
        b = c.B - 1
        yb, famb, _, routeb = _routed_launch(c, _prepare(c, sample=b))
        row["batch"] = {"family": famb, "route": routeb, "err": cs.norm_err(yb, y[b:b + 1], S["den"][b:b + 1]),
                        "equal": bool(torch.equal(yb, y[b:b + 1]))}
    return row


def judge_table(rows, where):
    """The failures of one run of the table (empty: passed)."""
    fails = []
    cases = {c.tag: c for c in fc.coverage_rows()}
    if [r["tag"] for r in rows] != list(cases):
        fails.append(f"{where}: ran {len(rows)} rows, the table has {len(cases)}")
    for r in rows:
        c, at = cases[r["tag"]], f"{where}/{r['tag']}"
        if r["family"] != fc.predict_family(c) or r["route"] != r["pred"] or r["inst"] != r["pred_inst"] or r["route"][0] != r["family"]:
            fails.append(f"{at}: family {r['family']} route {r['route']}, predicted on the CPU {r['pred']} (restated router: {fc.predict_family(c)})")
        if r["range"]:
            fails.append(f"{at}: range status raised")
        if not r["sentinel_ok"]:
            fails.append(f"{at}: wrote outside its output")
        if not r["repeat_equal"]:
            fails.append(f"{at}: repeat launch not bit-identical")
        if r["family"] not in fc.F16_FAMILIES:                  # (the two ragged rows: f16x3's launch, held by test_f16_sweep)
            if not r["err_exact"] <= cs.BAR_FP32:
                fails.append(f"{at}: family {r['family']} error {r['err_exact']:.3e} > {cs.BAR_FP32:.3e}")
            continue
        if (r["err_ops"] is None) != (c.pre == "elu"):
            fails.append(f"{at}: no operand-exact figure")
        if r["err_ops"] is not None and not r["err_ops"] <= cs.BAR_FP32:
            fails.append(f"{at}: {r['inst']} differs from the fp16-operand reference by {r['err_ops']:.3e} > {cs.BAR_FP32:.3e}")
        if not r["err_exact"] <= fc.BAR_F16:
            fails.append(f"{at}: {r['inst']} differs from the exact result by {r['err_exact']:.3e} > {fc.BAR_F16:.3e}")
        if c.B >= 2:
            bt = r["batch"]
            if bt["family"] != r["family"] or not bt["err"] <= cs.BAR_FP32:
                fails.append(f"{at}: last sample alone (family {bt['family']}) differs from its batch row by {bt['err']:.3e}")
            if bt["route"] == r["route"] and not bt["equal"]:
                fails.append(f"{at}: last sample alone takes the batch's route {r['route']} but not its bits")
    return fails


def _child(out_path):
    rows = [table_row(c) for c in fc.coverage_rows()]
    with open(out_path, "w") as f:
        json.dump(rows, f)


def test_every_instantiation_against_its_own_arithmetic():
    """The table in this process (default switches), then in one fresh child per further switch set, one after another and each
    under its own time limit; the first child that does not exit cleanly ends the test, so that nothing more is started on the
    device after a fault.  Per launch: family and instantiation as the CPU dry run predicts, <= BAR_FP32 from reference_f16,
    <= BAR_F16 from the exact result, sentinels, a bit-identical repeat, a clear range status, batch invariance.  After the four
    runs: all 63 instantiations launched; the worst error of each goes to the parity log."""
    assert not any(os.environ.get(k) for k in ("FUSG_HALO_MINWG", "FUSG_NO_KSPLIT", "FUSG_HALO_BN", "FUSG_NO_HALO", "FUSG_NO_F16_TAPUNIT"))
    runs = {fc.switch_name({}): [table_row(c) for c in fc.coverage_rows()]}
    base = {k: v for k, v in os.environ.items() if k not in ("FUSG_NO_SMALL", "FUSG_NO_POINTWISE", "FUSG_NO_F32_HALO",
                                                              "FUSG_NO_BF16_TAPUNIT", "FUSG_SMALL_KSPLIT")}
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        for env in fc.SWITCH_SETS[1:]:
            out = os.path.join(td, "rows.json")
            cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", out]
            p = subprocess.run(cmd, env=dict(base, **env), timeout=300, capture_output=True, text=True, cwd=repo)
            assert p.returncode == 0, (env, p.returncode, p.stderr[-3000:])
            with open(out) as f:
                runs[fc.switch_name(env)] = json.load(f)
    fails, worst = [], {}
    for name, rows in runs.items():
        fails += judge_table(rows, name)
        for r in rows:
            if r["inst"] is not None:
                key, e = tuple(r["inst"]), r["err_exact"] if r["err_ops"] is None else r["err_ops"]
                worst[key] = max(worst.get(key, 0.0), e)
    for (unit, kind, n), e in sorted(worst.items()):
        print(f"{unit} pre={kind} {n}: worst {e:.3e} ({'exact result, BAR_F16' if kind == 'elu' else 'fp16 operands, BAR_FP32'})")
        record(f"f16_{unit}_{kind}_{n}_err", e)
    for unit in fc.HALO_UNITS + fc.TAP_UNITS:
        record(f"f16_{unit}_operands_err_max", max(e for (u, k, _), e in worst.items() if u == unit and k != "elu"))
        record(f"f16_{unit}_elu_err_max", max(e for (u, k, _), e in worst.items() if u == unit and k == "elu"))
    assert not fails, "\n".join(fails)
    assert set(worst) == set(fc.INSTANTIATIONS) and len(worst) == 63, sorted(set(fc.INSTANTIATIONS) - set(worst))


# ---- operand scales: fp16 subnormal activations ------------------------------------------------------------------------------
def test_scale_rows_follow_fp16_rounding_with_gradual_underflow():
    """MODE 3 stages activations unscaled, so at sx <= 1e-4 they are fp16 subnormals: the kernel must follow RTN_fp16 WITH
    gradual underflow, as reference_f16 (torch .half()) does - held at BAR_FP32 at every scale, status clear; a kernel (or a
    matrix unit) that flushed them would miss the sx = 1e-2 rows by 36 bars and the sx = 1e-4 rows by ~27 000
    (tests/test_f16_mode_cpu.py).  One row scaled past 2^15 sets the status."""
    fails = []
    for c in fc.scale_cases():
        S = _prepare(c)
        ops.range_exceeded(dev())
        y, fam, _ = _launch(c, S, "f16")
        rf = fc.reference_f16(c, cs.inputs(c))
        e = cs.norm_err(y, *rf)
        exact = cs.norm_err(y, S["ref"], S["den"])
        print(f"{c.tag}: family {fam}, {e / cs.BAR_FP32:.3f} bars from the fp16-operand reference, {exact / fc.BAR_F16:.3f} of BAR_F16 from the exact result")
        record(f"f16_scale_{'sub' if c.sx <= 1e-2 else 'normal'}_operands_err", e)
        if fam != fc.predict_family(c) or fam not in fc.F16_FAMILIES:
            fails.append(f"{c.tag}: family {fam}")
        if not e <= cs.BAR_FP32:
            fails.append(f"{c.tag}: {e / cs.BAR_FP32:.2f} bars from the fp16-operand reference")
        if ops.range_exceeded(dev()):
            fails.append(f"{c.tag}: range status raised")
    assert not fails, "\n".join(fails)
    c = fc.OVER_RANGE
    _, fam, _ = _launch(c, _prepare(c), "f16")
    assert fam == fc.HALO_F16 and ops.range_exceeded(dev()) and not ops.range_exceeded(dev())


def test_nan_inputs_propagate_except_through_a_fused_relu_under_f16():
    """test_gpu_ops.test_nan_inputs_propagate_except_through_a_fused_relu on a family-15 launch: a NaN activation reaches every
    output it feeds - except through a fused ReLU, where fmaxf(NaN, 0) = 0 and the result is that of the input with a zero there,
    to the mode's own arithmetic.  As there, what the range status says after a launch that staged a NaN outside a fused ReLU
    is not part of the rule (the output carries the NaN): it is read back and cleared, not judged."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(61)
    x = torch.randn(1, 64, 16, 16, generator=g)
    x[0, 5, 8, 8] = float("nan")
    w = torch.randn(32, 64, 3, 3, generator=g) * 0.05
    plan = pack.pack_conv(w, None, pad=1)
    xd = ops.as_nhwc(x.to(dev()))
    ops.range_exceeded(dev())
    for pre in (L.PRE_NONE, L.PRE_ELU):
        got = ops.conv(plan, xd, pre_op=pre, precision="f16", ksplit=1).cpu()
        assert ops.last_conv_kernel() == fc.HALO_F16
        assert bool(torch.isnan(got[0, :, 7:10, 7:10]).all()), pre
        assert int(torch.isnan(got).sum()) == 32 * 9
    ops.range_exceeded(dev())
    got = ops.conv(plan, xd, pre_op=L.PRE_RELU, precision="f16", ksplit=1).cpu()
    assert ops.last_conv_kernel() == fc.HALO_F16
    xz = x.clone()
    xz[0, 5, 8, 8] = 0.0
    ref = F.conv2d(F.relu(xz).float().half().double(), fc.f16_weights(w), None, padding=1)
    den = F.conv2d(F.relu(xz).double(), w.double().abs(), None, padding=1) + 1e-300
    assert not bool(torch.isnan(got).any())
    assert cs.norm_err(got, ref, den) <= cs.BAR_FP32
    assert not ops.range_exceeded(dev())


def test_fused_block_predicates_on_device_tensors():
    """The GPU twin of test_f16_mode_cpu's predicate test: on device tensors all five predicates say yes under f16x3 - so the no
    that entry_nin_ok, respair_ok, bottleneck_ok and hg_head_ok give under "f16", as under "bf16", is the precision's doing."""
    got = fc.fused_block_predicates(dev())
    assert got["f16x3"] == (True, True, True, True, True), got
    assert got["f16"] == got["bf16"] == (False, False, False, False, True), got


# ---- store modes and tile lists under both single-pass modes ---------------------------------------------------------------
STORE_LAYER = cs.Case(tag="f16_store_layer", B=3, c0=64, c1=0, cout=64, kh=3, kw=3, H=16, W=32, pad=1, ksplit=1, pre="relu", seed=340)
# a tile-list launch never splits its K over the waves (csrc/conv_igemm.hip: ksw needs !tile_list), so its NORMAL launch has the
# same summation order only where that launch does not either: fewer than 4 taps on a 32-column unit
TILES_LAYER = cs.Case(tag="f16_tiles_layer", B=3, c0=64, c1=0, cout=64, kh=1, kw=3, H=16, W=48, pad=0, pad_w=1, ksplit=1,
                      pre="relu", seed=341)


@pytest.mark.parametrize("prec,family", [("bf16", cs.HALO_BF16), ("f16", fc.HALO_F16)])
@pytest.mark.parametrize("what", ["s2d", "d2s", "tiles"])
def test_store_modes_and_tile_lists_equal_the_normal_store(what, prec, family):
    """A SpaceToDepth store, a DepthToSpace store (64 -> 64 3 x 3) and a tile-list launch (64 -> 64 1 x 3, four of six patches)
    at 3 images of several patches each, against the NORMAL-store launch of the same layer after the layout permutation: the same
    route (fusg_conv2d_route_order), bit for bit.  The NORMAL launch itself is held to the operand-rounded reference at BAR_FP32."""
    c = TILES_LAYER if what == "tiles" else STORE_LAYER
    S = _prepare(c)
    plan, x0 = S["plan"], S["x0"]
    ops.range_exceeded(dev())
    kw = dict(pre_op=cs.PRE[c.pre], precision=prec, ksplit=1)
    with _capture() as cap:
        normal = ops.conv(plan, x0, **kw)
        route = cap.route_order()
    assert ops.last_conv_kernel() == family == route[0]
    inp = cs.inputs(c)
    rf = cs.reference_bf16(c, inp) if prec == "bf16" else fc.reference_f16(c, inp)
    assert cs.norm_err(normal, *rf) <= cs.BAR_FP32
    with _capture() as cap:
        if what == "tiles":
            out = ops.nhwc_empty(c.B, c.cout, c.H, c.W, dev())
            out.fill_(SENTINEL)
            tiles = torch.tensor([0, 2, 3, 5], dtype=torch.int32, device=dev())      # of the 2 x 3 patch grid
            got = ops.conv(plan, x0, out=out, tiles=tiles, **kw)
            want = torch.full_like(normal, SENTINEL)
            for t in tiles.cpu().tolist():
                py, px = divmod(t, c.W // 16)
                want[:, :, 8 * py:8 * py + 8, 16 * px:16 * px + 16] = normal[:, :, 8 * py:8 * py + 8, 16 * px:16 * px + 16]
        else:
            got = ops.conv(plan, x0, store=L.STORE_S2D if what == "s2d" else L.STORE_D2S, **kw)
            want = cs.s2d(normal) if what == "s2d" else cs.d2s(normal)
        assert cap.route_order() == route, (cap.route_order(), route)
    assert ops.last_conv_kernel() == family
    assert tuple(got.shape) == tuple(want.shape) and torch.equal(got.cpu(), want.cpu())
    assert not ops.range_exceeded(dev())


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        with torch.no_grad():
            _child(sys.argv[2])
    else:
        sys.exit("usage: test_gpu_f16_mode.py --child OUT.json")
