"""CPU: the single-pass fp16 precision mode ("f16", FUSG_PREC_F16) up to the launch - the header's constants and the Python
ones, the precision switch, the weights the mode multiplies with (pack.f16_mode_weights), the library's router as a dry run
(fusg_conv2d_route on the descriptors ops.conv builds) under the new precision and, unchanged, under the three existing ones,
and the references of the GPU test: every shape of its table must tell the mode's operand rounding from f16x3."""
import os
import re

import pytest
import torch

import conv_sweep as cs
import f16_cases as fc
from test_conv_sweep_cpu import _route
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import ops, pack

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_python_constants_agree():
    with open(os.path.join(REPO, "include", "fusg.h")) as f:
        hdr = f.read()
    enum = re.search(r"typedef enum fusg_precision \{(.*?)\} fusg_precision;", hdr, re.S).group(1)
    vals = {k: int(v) for k, v in re.findall(r"(FUSG_PREC_\w+)\s*=\s*(\d+)", enum)}
    assert vals["FUSG_PREC_F16"] == 5 == L.PREC_F16
    assert vals == {"FUSG_PREC_F32": L.PREC_F32, "FUSG_PREC_F16X3": L.PREC_F16X3, "FUSG_PREC_EMU_BF16": L.PREC_EMU_BF16,
                    "FUSG_PREC_EMU_BF16X2": L.PREC_EMU_BF16X2, "FUSG_PREC_BF16": L.PREC_BF16, "FUSG_PREC_F16": L.PREC_F16}
    fam = {k: int(v) for k, v in re.findall(r"(FUSG_CONV_\w+)\s*=\s*(\d+)", hdr)}
    assert fam["FUSG_CONV_HALO_F16"] == 15 == L.CONV_HALO_F16 == fc.HALO_F16
    assert fam["FUSG_CONV_TAPUNIT_F16"] == 16 == L.CONV_TAPUNIT_F16 == fc.TAPUNIT_F16
    assert len(set(fam.values())) == len(fam)                  # no family number given twice
    assert ops._PREC["f16"] == L.PREC_F16


def test_precision_switch_accepts_f16():
    prev = ops.PRECISION
    try:
        with ops.precision("f16"):
            assert ops.PRECISION == "f16" and ops.range_guarded() and ops.halo_precision()
        assert ops.PRECISION == prev
        ops.set_precision("f16")
        assert ops.PRECISION == "f16" and ops.range_guarded()
    finally:
        ops.set_precision(prev)
    with pytest.raises(ValueError):
        ops.set_precision("f16x2")


def test_f16_mode_weights_are_the_hi_half():
    """Every value times s_n is exactly representable in fp16 and equals split_f16x3's hi - on channels of very different
    magnitude, a channel with one dominant weight, and an all-zero channel."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(1, 8, 96, generator=g)
    w[0, 0] *= 1e-6
    w[0, 1] *= 3e4
    w[0, 2] *= 1e-20
    w[0, 3, 0] = 1e3                                           # one weight 2^10 above the rest of its channel
    w[0, 4] = 0.0
    w[0, 5] *= 7e11
    got = pack.f16_mode_weights(w)
    assert got.dtype == torch.float32 and got.shape == w.shape
    wsplit, inv_s = pack.split_f16x3(w)
    s = 1.0 / inv_s.double()
    scaled = got.double() * s[None, :, None]
    assert torch.equal(scaled, wsplit[:, 0].double())          # hi, bit for bit
    assert torch.equal(scaled.half().double(), scaled)         # representable in fp16
    assert torch.equal(got[0, 4], torch.zeros(96)) and float(inv_s[4]) == 1.0
    # hi is w rounded to 11 significant bits at the channel's scale: within half an fp16 ulp of the channel's largest |w| 2^-10
    err = (got.double() - w.double()).abs().amax(dim=2)[0]
    top = w.double().abs().amax(dim=2)[0]
    assert bool((err <= top * 2.0 ** -11).all()), (err / top.clamp_min(1e-300)).tolist()
    assert float(err[3] / top[3]) > 2.0 ** -24                 # (and it IS a rounding: the small weights of channel 3 lose bits)


def test_router_under_f16_and_unchanged_elsewhere():
    """fusg_conv2d_route: under FUSG_PREC_F16 every case of the sweep lands on its bf16 family mapped 5 -> 15, 11 -> 16 (so a
    layer that does not qualify runs the f16x3 kernel it runs today); FUSG_NO_F16_TAPUNIT keeps the stems on the split-fp16
    tap-unit kernel; the routes of f32 / f16x3 / bf16 are what the restated router says, with and without the new switch."""
    seen = set()
    for c in cs.all_cases():
        plan = cs.make_plan(c, torch.zeros(c.cout, c.cin, c.kh, c.kw), torch.zeros(c.cout))
        bf = cs.predict_family(c, "bf16")
        want = fc.f16_family(bf)
        assert want == {cs.HALO_BF16: 15, cs.TAPUNIT_BF16: 16}.get(bf, bf)
        assert _route(c, plan, "f16") == want == fc.predict_family(c), (c.tag, want)
        seen.add(want)
        os.environ["FUSG_NO_F16_TAPUNIT"] = "1"
        try:
            off = _route(c, plan, "f16")
            assert off == (cs.TAPUNIT if want == fc.TAPUNIT_F16 else want) == fc.predict_family(c, env={"FUSG_NO_F16_TAPUNIT": "1"}), c.tag
            for p in cs.PRECISIONS:                             # the new switch means nothing to the existing precisions
                assert _route(c, plan, p) == cs.predict_family(c, p), (c.tag, p)
        finally:
            del os.environ["FUSG_NO_F16_TAPUNIT"]
        for p in cs.PRECISIONS:
            assert _route(c, plan, p) == cs.predict_family(c, p), (c.tag, p)
        # the off-switch of the family it landed on (K split in two: the next family in the router's order)
        sw = cs.off_switch(bf, c)
        if sw is not None and want in fc.F16_FAMILIES and sw[1] is not None:
            assert _route(c, plan, "f16", sw[0], sw[1]) == fc.predict_family(c, env=sw[0], ksplit=sw[1]), c.tag
    assert set(fc.F16_FAMILIES) <= seen and cs.HALO_BF16 not in seen and cs.TAPUNIT_BF16 not in seen
    stems = [c for c in cs.all_cases() if fc.predict_family(c) == fc.TAPUNIT_F16]
    assert len(stems) >= 5


def test_route_order_reports_the_new_families():
    import ctypes as C
    c = next(c for c in cs.edge_cases() if c.tag == "halo_cout128_ks1")
    plan = cs.make_plan(c, torch.zeros(c.cout, c.cin, c.kh, c.kw), torch.zeros(c.cout))
    x0 = torch.zeros(c.B, c.H, c.W, c.c0).permute(0, 3, 1, 2)
    with ops.status_scope(torch.zeros(4, dtype=torch.int32)):
        d, _ = ops._conv_desc(plan, x0, None, precision="f16", ksplit=1, res0=torch.zeros(c.B, c.H, c.W, c.cout).permute(0, 3, 1, 2),
                              res1=torch.zeros(c.B, c.H, c.W, c.cout).permute(0, 3, 1, 2))
        lib = L.lib()
        lib.fusg_conv2d_plan(C.byref(d))
        out = (C.c_int32 * 4)()
        assert lib.fusg_conv2d_route_order(C.byref(d), C.byref(out)) == 0
    assert out[0] == fc.HALO_F16 and out[1] in (32, 64, 128) and out[2] == 1 and out[3] in (0, 1)     # never column-major


@pytest.mark.parametrize("c", fc.table_cases(), ids=lambda c: c.tag)
def test_references_discriminate(c):
    """The GPU test holds families 15 / 16 to reference_f16 at BAR_FP32.  That only proves the single-pass arithmetic if the
    reference is far from the exact result: more than 10 x BAR_FP32 on every shape of its table - a kernel that silently
    ran f16x3 (error <= BAR_FP32 against the exact result) cannot pass.  And it stays within the operand-rounding bound."""
    cs.validate(c)
    inp = cs.inputs(c)
    ref, den = cs.reference(c, inp)
    rf = fc.operand_rounded(c, inp)
    assert (fc.reference_f16(c, inp) is None) == (c.pre == "elu")
    e = cs.norm_err(rf[0], ref, den)
    assert 10 * cs.BAR_FP32 < e <= fc.BAR_F16, (c.tag, e)
    # and it is 8 x finer than bf16's, as 11 significant bits against 8 are
    eb = cs.norm_err(cs.reference(c, inp, w=inp["w"].bfloat16().double(), xp=cs.pre_input(c, inp).float().bfloat16().double())[0], ref, den)
    assert e < eb / 2, (c.tag, e, eb)


def test_f16_bar_is_what_two_fp16_roundings_can_reach():
    """BAR_F16 (ELU rows against the exact reference) bounds the operand-rounded reference of every sweep case."""
    worst = 0.0
    for c in cs.edge_cases():
        inp = cs.inputs(c)
        ref, den = cs.reference(c, inp)
        e = cs.norm_err(fc.operand_rounded(c, inp)[0], ref, den)
        assert e <= fc.BAR_F16, (c.tag, e)
        worst = max(worst, e)
    assert worst > 2.0 ** -13, worst
