"""CPU: the statistics sweep's own machinery (tests/stats_sweep.py) - coverage of the case table by the restated router, the
restated eligibility rule against hand-written negatives, the order-independence of `combine`, the derived bars against an
fp32 emulation of the epilogue's and of the streaming kernel's arithmetic, and the synthetic inputs of the finaliser tests."""
from dataclasses import replace

import pytest
import torch
import torch.nn.functional as F

import conv_sweep as cs
import stats_sweep as ss

L = cs.L


def test_every_family_and_precision_has_a_case():
    want = {(cs.GEN_F32, "f32"), (cs.GEN_F16X3, "f16x3"), (cs.GEN_F16X3, "bf16"), (cs.HALO, "f16x3"), (cs.HALO_S2D, "f16x3"),
            (cs.HALO_F32, "f32"), (cs.HALO_BF16, "bf16"), (cs.TAPUNIT, "f16x3"), (cs.TAPUNIT_F32, "f32"),
            (cs.TAPUNIT_BF16, "bf16"), (ss.HALO_F16, "f16"), (ss.TAPUNIT_F16, "f16")}
    seen, variants, tiles = set(), {}, set()
    for sc in ss.stat_cases():
        assert ss.qualifies(sc.case, ksplit=1), sc.tag
        cs.validate(sc.case)
        for prec in sc.precs:
            fam = ss.predict_stats_family(sc.case, prec, sc.tile)
            assert fam in ss.STAT_FAMILIES and fam not in ss.NO_STAT_FAMILIES, (sc.tag, prec, fam)
            seen.add((fam, prec))
            variants.setdefault(fam, set()).add(sc.variant)
            if sc.case.sx != 1.0:
                variants[fam].add("small" if sc.case.sx < 1 else "large")
            if sc.tile:
                assert fam in (cs.GEN_F32, cs.GEN_F16X3), (sc.tag, prec, fam)      # an explicit tile is a generic launch
                tiles.add((sc.tile, prec))
    assert want <= seen, want - seen
    assert {(t, p) for t in (1, 2, 3, 4, 5) for p in ("f32", "f16x3")} <= tiles, tiles
    for fam in ss.STAT_FAMILIES:                                    # every data variant on at least one row per family
        assert {"plain", "bias50", "zero_ch", "small", "large"} <= variants[fam], (fam, variants[fam])
    # both epilogues of the halo body, at every precision; an out slice and a single image per family group
    ks = {(ss.halo_takes_ksplit(sc.case, p), p) for sc in ss.stat_cases() for p in sc.precs}
    assert {(k, p) for k in (True, False) for p in ss.PRECISIONS_F16} <= ks
    for fams in ((cs.GEN_F32, cs.GEN_F16X3), (cs.HALO, cs.HALO_F32, cs.HALO_BF16, ss.HALO_F16),
                 (cs.TAPUNIT, cs.TAPUNIT_F32, cs.TAPUNIT_BF16, ss.TAPUNIT_F16)):
        rows = [sc for sc in ss.stat_cases() if ss.predict_stats_family(sc.case, sc.precs[-1], sc.tile) in fams]
        assert any(sc.case.out == "slice" and sc.case.out_c_off % 4 == 0 for sc in rows), fams
        assert any(sc.case.B == 1 for sc in rows), fams


def test_qualifies_against_hand_written_negatives():
    ok = cs.Case("ok", 2, 12, 0, 36, 3, 3, 8, 12, pad=1, ksplit=1)
    assert ss.qualifies(ok)
    assert ss.qualifies(replace(ok, out="slice", out_c_off=8))
    assert ss.qualifies(replace(ok, pm=L.PAD_REPLICATE, qwin=(0, 0, 8, 12)))            # a window at the origin
    no = [replace(ok, act=L.ACT_RELU), replace(ok, act=L.ACT_TANH), replace(ok, res=1), replace(ok, res=2),
          replace(ok, cout=38), replace(ok, W=11), replace(ok, out="misaligned"), replace(ok, out="nchw"),
          replace(ok, out="slice", out_c_off=2), replace(ok, pm=L.PAD_REPLICATE, H=9, qwin=(1, 0, 8, 12)),
          replace(ok, pm=L.PAD_REPLICATE, W=13, qwin=(0, 1, 8, 12))]
    for c in no:
        assert not ss.qualifies(c), c
    assert not ss.qualifies(ok, store=L.STORE_D2S) and not ss.qualifies(ok, store=L.STORE_S2D)
    assert not ss.qualifies(ok, nphase=4) and not ss.qualifies(ok, tiles=True)
    big_k = cs.Case("k576", 1, 64, 0, 32, 3, 3, 8, 16, pad=1)
    for prec in cs.PRECISIONS:
        assert ss.planned_ksplit(big_k, prec, 0) > 1
        assert not ss.qualifies(big_k, ksplit=0, prec=prec) and ss.qualifies(big_k, ksplit=1, prec=prec)
        assert not ss.qualifies(ok, ksplit=2, prec=prec)
    got = sorted(n for n, c, kw in ss.negative_cases()
                 if not ss.qualifies(c, ksplit=c.ksplit, store=kw.get("store", L.STORE_NORMAL), tiles=bool(kw.get("tiles"))))
    assert got == sorted(n for n, _, _ in ss.negative_cases()) and len(got) == 10
    for n, c, kw in ss.negative_cases():                     # each fails ONE condition: the twin without it qualifies
        cs.validate(c)


@pytest.mark.parametrize("geometry", ["rows", "halo"])
def test_combine_is_exact_and_order_independent(geometry):
    g = torch.Generator().manual_seed(3)
    y = torch.randn(3, 8, 16, 32, generator=g, dtype=torch.float64) * 3 + torch.arange(8, dtype=torch.float64).view(1, 8, 1, 1) * 40
    y[:, 1] = -7.25
    slots = ss.host_slots(y, geometry)
    assert slots.shape == (3, 16, 8, 2)
    got, ref = ss.combine(slots), ss.direct(y)
    for k in ("mean", "var", "ln_mean", "ln_var"):
        ok = ref[k] != 0                                      # (the constant channel's variance: checked below)
        assert float(((got[k] - ref[k]).abs()[ok] / ref[k].abs()[ok]).max()) <= 1e-12, k
    assert float(got["var"][:, 1].abs().max()) == 0.0
    perm = torch.randperm(16, generator=g)
    again = ss.combine(slots[:, perm])
    for k in ("mean", "var", "ln_mean", "ln_var"):
        assert float((again[k] - got[k]).abs().max()) <= 1e-12 * float(got[k].abs().max())
    e = ss.stat_errs(got, ref)
    assert not ss.over_bars(e, 1e-6), e
    if geometry == "halo":                                   # the two geometries hold different pixels per slot
        assert not torch.equal(slots, ss.host_slots(y, "rows"))


@pytest.mark.parametrize("sc", ss.stat_cases(), ids=lambda sc: sc.tag)
def test_emulated_slots_stay_under_a_quarter_of_the_bars(sc):
    """The epilogue's fp32 slot arithmetic, emulated on the case's float64 reference output (rounded to fp32, as the kernel's
    values are), against the float64 statistics of those values.  The constant channel comes out exactly."""
    c = sc.case
    y = cs.reference(c, ss.stat_inputs(sc))[0]
    y32 = cs.window(c, y).float()
    ref = ss.direct(y32)
    for geometry in ("rows",) + (("halo",) if y32.shape[2] % 8 == 0 and y32.shape[3] % 16 == 0 else ()):
        got = ss.combine(ss.emulate_slots(y32, geometry))
        e = ss.stat_errs(got, ref)
        assert not ss.over_bars(e, 0.25), (sc.tag, geometry, e)
        if sc.variant == "zero_ch":
            assert float(got["var"][:, ss.ZERO_CH].abs().max()) == 0.0
            assert float(ref["var"][:, ss.ZERO_CH].abs().max()) == 0.0
        if sc.variant == "bias50":
            assert float((ref["mean"].abs() / ref["var"].sqrt()).min()) > 20.0


def test_comparator_rejects_subtly_wrong_statistics():
    """One slot's M2 dropped, a mean off by 8 ulp, statistics indexed by a padded channel pitch: all over the bars."""
    g = torch.Generator().manual_seed(5)
    y = (torch.randn(2, 36, 8, 16, generator=g) * 2 + 30).float()
    ref = ss.direct(y)
    slots = ss.emulate_slots(y, "halo")
    assert not ss.over_bars(ss.stat_errs(ss.combine(slots), ref), 0.25)
    bad = slots.clone()
    bad[0, 2, 5, 1] = 0
    assert "var" in ss.over_bars(ss.stat_errs(ss.combine(bad), ref))
    bad = slots.clone()
    bad[1, :, 7, 0] *= 1 + 8 * 2.0 ** -23
    assert "mean" in ss.over_bars(ss.stat_errs(ss.combine(bad), ref))
    bad = slots.clone()
    bad[:, :, 1:] = slots[:, :, :-1]
    assert ss.over_bars(ss.stat_errs(ss.combine(bad), ref))
    bad = slots.clone()                                       # a constant channel whose variance is not exactly 0
    y2 = y.clone()
    y2[:, 3] = 1.5
    s2 = ss.emulate_slots(y2, "halo")
    assert not ss.over_bars(ss.stat_errs(ss.combine(s2), ss.direct(y2)))
    s2[0, 0, 3, 1] = 1e-30
    assert "var" in ss.over_bars(ss.stat_errs(ss.combine(s2), ss.direct(y2)))


@pytest.mark.parametrize("shape", ss.FINAL_SHAPES, ids=lambda s: "b%d_n%d_c%d" % s)
def test_synthetic_slots_reproduce_instance_norm(shape):
    B, n, C = shape
    slots, y = ss.synthetic_slots(B, n, C)
    assert slots.dtype == torch.float32 and slots.shape == (B, n, C, 2) and y.shape == (B, C, n, 32)
    assert bool(torch.isfinite(slots).all()) and float(slots[..., 1].min()) >= 0.0
    # y's slots ARE the fp32 slots, to float64's own cancellation at mean = 1000 std - five orders under the 2^-22 they serve
    exact = ss.host_slots(y, "rows")
    d = (exact - slots.double()).abs()
    assert float((d[..., 0] / (slots[..., 0].double().abs() + (slots[..., 1].double() / 32).sqrt())).max()) <= 1e-12
    assert float((d[..., 1] / (slots[..., 1].double() + 1e-300))[slots[..., 1] > 0].max()) <= 1e-9
    got = ss.combine(slots)
    sc, sh, _ = ss.in_scale_shift(got["mean"], got["var"])
    ref = F.instance_norm(y, eps=ss.EPS)
    out = y * sc[:, :, None, None] + sh[:, :, None, None]
    # |y| rstd reaches 1000 std / std: the products cancel to O(1) values
    assert float((out - ref).abs().max()) <= 1e-9, float((out - ref).abs().max())
    assert float(got["var"][:, ss.CONST_CH].abs().max()) == 0.0
    g = torch.Generator().manual_seed(C)
    gamma, beta = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    sc, sh, _ = ss.ln_scale_shift(got["ln_mean"], got["ln_var"], gamma, beta)
    a = y.reshape(B, -1)
    mean, std = a.mean(1).view(B, 1, 1, 1), a.std(1).view(B, 1, 1, 1)
    ref = (y - mean) / (std + ss.EPS) * gamma.view(1, C, 1, 1) + beta.view(1, C, 1, 1)
    out = y * sc[:, :, None, None] + sh[:, :, None, None]
    assert float((out - ref).abs().max()) <= 1e-9 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("cc", ss.chan_cases(), ids=lambda cc: cc.tag)
def test_emulated_chan_stats_stay_under_a_quarter_of_the_bar(cc):
    """The streaming kernel's per-lane fp32 accumulation order, emulated, for every nchunk the GPU test uses."""
    x = ss.chan_input(cc)
    for n in ss.chan_nchunks(cc.hw):
        e = ss.chan_errs(ss.chan_combine(ss.emulate_chan_stats(x, n), x), x)
        if cc.C * cc.hw == 1:
            e = {k: v for k, v in e.items() if not k.startswith("ln_")}
        assert all(v <= 0.25 * ss.BAR_CHAN for v in e.values()), (cc.tag, n, e)


def test_chan_stats_emulation_is_the_plain_sum_in_exact_cases():
    x = torch.arange(2 * 8 * 3 * 5, dtype=torch.float32).reshape(2, 8, 3, 5) % 17      # small integers: fp32 sums are exact
    for n in (1, 2, 7, 15, 18):
        p = ss.emulate_chan_stats(x, n)
        v = (x - x[:, :, :1, :1]).reshape(2, 8, -1).double()
        assert torch.equal(p[..., 0].sum(1).double(), v.sum(2)) and torch.equal(p[..., 1].sum(1).double(), (v * v).sum(2))
        got = ss.chan_combine(p, x)
        ref = ss.direct(x)
        assert float((got["mean"] - ref["mean"]).abs().max()) <= 1e-12 and float((got["var"] - ref["var"]).abs().max()) <= 1e-10
        assert float((got["ln_var"] - ref["ln_var"]).abs().max()) <= 1e-10


@pytest.mark.parametrize("shape", ss.WRAPPER_SHAPES, ids=lambda s: "c%d_hw%d" % s)
def test_one_chunk_is_a_fair_reference_on_centred_inputs(shape):
    """The emulated one-chunk run and the emulated run at the wrappers' chunk count, on the centred input: each within half of
    BAR_WRAPPER of float64's rstd (so within the bar of each other); the chain-length criterion holds for every shape."""
    from future_urban_scene_generation_amd import ops
    C, hw = shape
    assert ss.chan_chain_length(C, hw) <= 768 and ops._nchunk(2, C, hw) > 1
    x = ss.chan_input(ss.ChanCase(C, hw, 2, "centred"))
    ref = ss.direct(x)
    r64 = 1.0 / torch.sqrt(ref["var"] + ss.EPS)
    for n in (1, ops._nchunk(2, C, hw)):
        got = ss.chan_combine(ss.emulate_chan_stats(x, n), x)
        r = 1.0 / torch.sqrt(got["var"] + ss.EPS)
        assert float(((r - r64).abs() / r64).max()) <= 0.5 * ss.BAR_WRAPPER, (n, float(((r - r64).abs() / r64).max()))
        assert float(((got["mean"] - ref["mean"]).abs() / ref["mean"].abs()).max()) <= 0.5 * ss.BAR_WRAPPER      # (shift)
