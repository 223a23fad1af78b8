"""GPU: the single-pass fp16 precision mode ("f16", FUSG_PREC_F16: the halo kernel's MODE 3 and the tap-unit kernel's).

On a launch that takes family 15 / 16 the result is held to the mode's OWN arithmetic (f16_cases.reference_f16: operands
rounded to fp16, exact products) at conv_sweep.BAR_FP32, the project's bar for "same operands, fp32 accumulation order" -
tests/test_f16_mode_cpu.py shows that this reference is > 10 bars away from the exact result on every shape of the table, so
a kernel that ran f16x3 instead cannot pass.  ELU rows (no operand-exact reference) are held to the exact result at the
operand-rounding bound (1 + 2^-11)^2 - 1.  On every other family the launch must be the f16x3 launch, bit for bit.  Then the
range guard, the module-level fp32 redo, the image networks against the reference's golden vectors (no worse than bf16, SSIM
>= 0.999), the hourglass (f16x3 inside: same bytes) and the pipeline's compare_precisions."""
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

# staging shapes that DO land on the halo kernel: several patches with zero padding on every side of the image, and two sources
# into 48 outputs (cout_pad 64: the padded columns' stores must be masked) - beside the issue's ragged ones, which take the
# generic gather and must therefore equal f16x3
EXTRA = [cs.Case(tag="f16_patches_2x16x32", B=2, c0=32, c1=0, cout=32, kh=3, kw=3, H=16, W=32, pad=1, ksplit=1, seed=61),
         cs.Case(tag="f16_two_src_cout48_8x16", B=2, c0=64, c1=32, cout=48, kh=3, kw=3, H=8, W=16, pad=1, ksplit=1, seed=62,
                 pre="affine_relu", per_sample=True, res=1)]
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
    y2, fam2, _ = _launch(c, S, "f16")
    assert fam2 == fam and torch.equal(y, y2), "repeat launch not bit-identical"
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
