"""CPU: the single-pass fp16 precision mode ("f16", FUSG_PREC_F16) up to the launch - the header's constants and the Python
ones, the precision switch, the weights the mode multiplies with (pack.f16_mode_weights), the library's router as a dry run
(fusg_conv2d_route on the descriptors ops.conv builds) under the new precision and, unchanged, under the three existing ones,
and the references of the GPU test: every shape of its table must tell the mode's operand rounding from f16x3.

Then the instantiation table (f16_cases.tile_cases): the 63 MODE 3 kernel instantiations of profiles/f16_mode_resources.txt, the
library's router dry-run in fresh CPU child processes under the four process-wide switch sets to show that the table reaches all
of them, and the table's references shown to be sharp - every row discriminates the mode from f16x3, the comparator rejects the
sweep's mutations of the fp16-operand arithmetic, and four wrong readings of the mode fail the rows named for them.

What ELU rows prove, and what they do not: the device exp differs from torch's in the last bits, enough to flip an operand's fp16
rounding, so an ELU row has no operand-exact reference and is held to the exact result at the operand-rounding bound BAR_F16 only.
That bound is ~2000 times BAR_FP32: on its own an ELU row cannot tell a kernel that mis-sums in the last bits from a right one.
Each `elu` instantiation is therefore reached by an ELU row AND its indexing is shared with the twin row of the same shape with
pre="relu" (the `none` kind, operand-exact); the ELU arithmetic itself is pinned by the sweep's edge table."""
import json
import os
import re
import subprocess
import sys
import tempfile

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


# ---- the instantiation table --------------------------------------------------------------------------------------------------
def test_instantiation_list_is_the_resources_profile():
    """INSTANTIATIONS = the lines of profiles/f16_mode_resources.txt: 63, parsed."""
    with open(os.path.join(REPO, "profiles", "f16_mode_resources.txt")) as f:
        lines = re.findall(r"^(conv_(?:halo|tapunit)_\w+)\s+TM\d TN\d WM\d WN\d pre=(\w+)\s+(?:NI|U)=(\d+)", f.read(), re.M)
    got = [(u, p, int(n)) for u, p, n in lines]
    assert len(got) == 63 == len(set(got)) == len(fc.INSTANTIATIONS)
    assert set(got) == set(fc.INSTANTIATIONS)
    assert set(fc.STARRED) <= set(got)
    with open(os.path.join(REPO, "profiles", "f16_mode_resources.txt")) as f:
        star = re.findall(r"^(conv_halo_\w+)\s+.*pre=(\w+)\s+NI=(\d+)\s+KS=\d \*", f.read(), re.M)
    assert {(u, p, int(n)) for u, p, n in star} == set(fc.STARRED)


@pytest.fixture(scope="module")
def predictions():
    """{switch set name: {"table": ..., "before": ...}}: f16_cases.py --predict in one fresh CPU child per switch set (the library
    reads FUSG_HALO_MINWG / FUSG_NO_KSPLIT once per process)."""
    out = {}
    base = {k: v for k, v in os.environ.items() if k not in ("FUSG_HALO_MINWG", "FUSG_NO_KSPLIT", "FUSG_HALO_BN", "FUSG_NO_HALO",
                                                              "FUSG_NO_F16_TAPUNIT", "FUSG_NO_SMALL")}
    with tempfile.TemporaryDirectory() as td:
        for env in fc.SWITCH_SETS:
            path = os.path.join(td, "pred.json")
            cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(REPO, "tests", "f16_cases.py"), "--predict", path]
            p = subprocess.run(cmd, env=dict(base, **env), timeout=300, capture_output=True, text=True, cwd=REPO)
            assert p.returncode == 0, (env, p.returncode, p.stderr[-3000:])
            with open(path) as f:
                out[fc.switch_name(env)] = json.load(f)
    return out


def _insts(pred):
    return {tuple(v[1]) for v in pred.values() if v[1] is not None}


def test_table_reaches_every_instantiation(predictions):
    """The union over the four switch sets is all 63, and each instantiation is reached by a row with an operand-exact
    reference of its kind: a non-ELU row, or for the `elu` kind an ELU row (whose relu twin, same shape, is in the table).
    Before the table the GPU test reached 9 of the 45 halo instantiations (10 with its two extra rows), all of them 32 columns
    wide - the reason this test exists."""
    rows = {c.tag: c for c in fc.coverage_rows()}
    reached = {}
    for name, pred in predictions.items():
        assert set(pred["table"]) == set(rows)
        for tag, (ro, inst) in pred["table"].items():
            c = rows[tag]
            assert ro[0] == fc.predict_family(c), (name, tag, ro)
            if inst is not None:
                assert (tuple(inst)[1] == "elu") == (c.pre == "elu")
                reached.setdefault(tuple(inst), []).append((name, tag))
    assert set(reached) == set(fc.INSTANTIATIONS), sorted(set(fc.INSTANTIATIONS) - set(reached))
    assert len(reached) == 63
    tile = {c.tag: c for c in fc.tile_cases()}
    for c in tile.values():                                     # every row of the new table is a family 15 / 16 launch
        assert fc.predict_family(c) in fc.F16_FAMILIES, c.tag
        if c.pre == "elu":                                      # ... and every ELU row has its relu twin
            from dataclasses import replace
            twin = tile[c.tag.replace("_elu_", "_relu_")]
            assert replace(twin, tag=c.tag, pre="elu", seed=c.seed) == c, c.tag
    # the two instantiations whose MODE 3 build differs from its MODE 1 sibling in occupancy and epilogue:
    #   (conv_halo_128, elu, 10):   t16_k7_elu_n128_b3   under FUSG_HALO_MINWG=1
    #   (conv_halo_64, affine, 10): t16_k7_affine_n64_b1 under FUSG_HALO_MINWG=1 + FUSG_NO_KSPLIT=1
    assert ("FUSG_HALO_MINWG", "t16_k7_elu_n128_b3") in reached[fc.STARRED[0]]
    assert ("FUSG_HALO_MINWG+FUSG_NO_KSPLIT", "t16_k7_affine_n64_b1") in reached[fc.STARRED[1]]
    before = _insts(predictions["default"]["before"])
    halo_before = {i for i in before if i[0].startswith("conv_halo")}
    # (9 from the sweep's edge table and f16_cases.table_cases, as the restated column_tile / ksw rule counts them; the GPU module's
    # two EXTRA rows add (32k, affine, 6): 10 of 45, every one a 32-column unit)
    assert all(i[0] in ("conv_halo_32", "conv_halo_32k") for i in halo_before), sorted(halo_before)
    assert halo_before - {("conv_halo_32k", "affine", 6)} == {("conv_halo_32", "none", 6), ("conv_halo_32", "elu", 6), ("conv_halo_32", "affine", 6),
                           ("conv_halo_32k", "none", 6), ("conv_halo_32k", "elu", 6), ("conv_halo_32k", "none", 8),
                           ("conv_halo_32k", "elu", 8), ("conv_halo_32k", "affine", 8), ("conv_halo_32k", "none", 10)}


def test_instantiation_of_a_route_order():
    c = next(c for c in fc.tile_cases() if c.tag == "t16_k7_elu_n128_b3")
    assert fc.instantiation(c, [15, 128, 1, 0]) == ("conv_halo_128", "elu", 10)
    assert fc.instantiation(c, [15, 32, 1, 1]) == ("conv_halo_32k", "elu", 10)
    assert fc.instantiation(c, [1, 4, 1, 0]) is None
    s = next(c for c in fc.tile_cases() if c.tag == "t16_s2_k4_affine_n128_b3")
    assert fc.instantiation(s, [15, 64, 1, 0]) == ("conv_halo_64", "affine", 6)       # quadrant form: a 10 x 18 halo
    t = next(c for c in fc.tile_cases() if c.tag.startswith("t16_tap_c3_"))
    assert fc.instantiation(t, [16, 64, 1, 0])[2] == 4
    t = next(c for c in fc.tile_cases() if c.tag.startswith("t16_tap_c24_"))
    assert fc.instantiation(t, [16, 32, 1, 0])[2] == 8


@pytest.mark.parametrize("c", fc.tile_cases(), ids=lambda c: c.tag)
def test_tile_rows_discriminate_and_reject_mutations(c):
    """test_references_discriminate's rule on every row of the instantiation table (K <= 1568), and conv_sweep.mutations applied
    to the fp16-operand arithmetic - a tap moved, a 32-channel chunk dropped, the bias missing, one pixel off by 4 bars - all
    rejected by the comparator against reference_f16 at BAR_FP32."""
    cs.validate(c)
    assert c.K <= 1568 and c.mflop() <= 1300.0, (c.K, c.mflop())
    inp = cs.inputs(c)
    ref, den = cs.reference(c, inp)
    rf, rden = fc.operand_rounded(c, inp)
    e = cs.norm_err(rf, ref, den)
    print(f"{c.tag}: operand-rounded reference {e / cs.BAR_FP32:.1f} bars from the exact one")
    assert 10 * cs.BAR_FP32 < e <= fc.BAR_F16, (c.tag, e / cs.BAR_FP32)
    c2, inp2 = fc.rounded_operands_case(c, inp)
    same, _ = cs.reference(c2, inp2)
    assert torch.equal(same, rf)
    names = []
    for name, y in cs.mutations(c2, inp2):
        if name == "fp16_hi_only":                              # (rounding the rounded operands again: the identity)
            continue
        names.append(name)
        em = cs.norm_err(y, rf, rden)
        assert em > cs.BAR_FP32, (c.tag, name, em)
    assert {"k_chunk_dropped", "bias_missing", "one_pixel_off"} <= set(names) and (c.kh * c.kw == 1 or "tap_moved" in names), names


# ---- operand scales and the wrong readings of the mode --------------------------------------------------------------------
_SCALE = {c.tag: c for c in fc.scale_cases()}


def _scale_row(sx, sw):
    return _SCALE[f"f16_scale_x{sx:g}_w{sw:g}"]


def _bars_off(name, c):
    inp = cs.inputs(c)
    rf, rden = fc.operand_rounded(c, inp)
    return cs.norm_err(fc.restatement(name, c, inp), rf, rden) / cs.BAR_FP32


def test_scale_table_where_eleven_bits_hold():
    """The mode stages activations unscaled: below 2^-14 they are fp16 subnormals with an absolute 2^-25 rounding error, so the
    operand-rounding bound BAR_F16 (11 significant bits per operand) holds for sx >= 1e-5 - the few draws under 2^-14 are then
    carried by the rest of the sum - and not at sx = 1e-6, at any weight scale (the weights carry their own scale s_n)."""
    assert len(fc.scale_cases()) == len(fc.SCALES_X) * len(fc.SCALES_W) + 1
    for c in fc.scale_cases():
        cs.validate(c)
        inp = cs.inputs(c)
        ref, den = cs.reference(c, inp)
        e = cs.norm_err(fc.operand_rounded(c, inp)[0], ref, den)
        print(f"{c.tag}: {e / fc.BAR_F16:.3f} of BAR_F16")
        if c.sx >= 1e-5:
            assert e <= fc.BAR_F16, (c.tag, e / fc.BAR_F16)
        else:
            assert e > fc.BAR_F16, (c.tag, e / fc.BAR_F16)
        assert float(cs.pre_input(c, inp).abs().max()) < 2.0 ** 15          # none of them trips the range guard
    assert float(cs.inputs(fc.OVER_RANGE)["x0"].abs().max()) >= 2.0 ** 15


def test_wrong_restatements_fail_their_named_rows():
    """(a) weights as plain w.half(), without s_n: fails the sw = 1e-6 rows (and cannot be seen at sw >= 1: those rows cannot
    stand in); (b) staged fp16 subnormals flushed to zero: fails sx = 1e-2 and below (not sx >= 1); (c) activations truncated,
    (d) the lo term included: fail every row."""
    for sx in (1e-2, 1.0, 1e2):
        assert _bars_off("w_unscaled", _scale_row(sx, 1e-6)) > 1000.0
        for sw in (1.0, 1e3):
            assert _bars_off("w_unscaled", _scale_row(sx, sw)) < 0.1        # (s_n is not a power of two: a last-bit difference)
    assert _bars_off("w_unscaled", _SCALE["f16_scale_stem_x0.01_w1e-06"]) > 1000.0
    for sw in fc.SCALES_W:
        assert _bars_off("x_flushed", _scale_row(1e-2, sw)) > 10.0
        assert _bars_off("x_flushed", _scale_row(1e-4, sw)) > 1000.0
        for sx in (1.0, 1e2, 4e3):
            assert _bars_off("x_flushed", _scale_row(sx, sw)) == 0.0
    for c in fc.scale_cases():
        if c.sx >= 1e-4:
            assert _bars_off("x_truncated", c) > 10.0, c.tag
            assert _bars_off("lo_included", c) > 10.0, c.tag
    for c in fc.tile_cases()[::7]:
        assert _bars_off("x_truncated", c) > 10.0 and _bars_off("lo_included", c) > 10.0, c.tag


def test_fused_block_predicates_say_under_f16_what_they_say_under_bf16():
    """entry_nin_ok, respair_ok, bottleneck_ok, hg_head_ok fuse in f16x3 (bottleneck: f32 too) only, so a network under "f16"
    keeps the launches it keeps under "bf16"; up2_phases_ok does not read the precision.  (f16_cases.fused_block_predicates asks
    with the keyword and through the process-wide switch, and checks that the two agree.)"""
    with ops.status_scope(torch.zeros(4, dtype=torch.int32)):
        got = fc.fused_block_predicates("cpu")
    assert got["f16"] == got["bf16"] == (False, False, False, False, True), got
    # bottleneck_ok and up2_phases_ok read shapes only, and these shapes qualify where the precision allows it.  The other three
    # say no to any CPU tensor (ops.is_nhwc), so their False here shows the precision check only together with the GPU twin of
    # this test, where the same shapes give True under f16x3.
    assert got["f16x3"] == (False, False, True, False, True), got
