"""GPU: the discriminator layer on the device - LeakyReLU(0.2) in every conv family's epilogue and in the elementwise kernels,
the count-excluding average pool, the mask multiply and the GAN-term sums against their host twins, EdgeConnect's Discriminator
and Warp&Learn's D_NLayersMulti against the float64 restatement (tests/critic_ref.py, proven against the reference's stored
results by tests/test_critic_cpu.py), the scalar objectives at derived bars, `evaluate` against its separately called pieces
and a recorded pass of the discriminator."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_sweep as cs
import critic_cases as cc
import critic_ref as cr
from conftest import GOLD, record

pytestmark = pytest.mark.gpu

from future_urban_scene_generation_amd import _lib as L          # noqa: E402
from future_urban_scene_generation_amd import ops, pack           # noqa: E402
from future_urban_scene_generation_amd.synth import synth_inputs, synth_state_dict  # noqa: E402

DEV = "cuda:0"
CANARY = 12332318.0
U = 2.0 ** -23
PRECS = ("f16x3", "f32")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def _same(a, b):
    """Bit-equal, a NaN matching any NaN (its sign and payload are nobody's promise)."""
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(np.nan_to_num(a, nan=0.0)), _bits(np.nan_to_num(b, nan=0.0)))


def gold(case):
    return np.load(os.path.join(GOLD, f"critic_{case}.npz"))


# ---- LeakyReLU in the conv epilogues -------------------------------------------------------------------------------------
# one or two rows of conv_sweep's edge table per family it names; every one without an activation, a residual or a special
# destination of its own, so the only change is act = ACT_LEAKY02
LEAKY_TAGS = ("gen_c12_3x3", "gen_5x5_reflect", "gen_k2304", "halo_3x3_planner", "small_hw64_8x8", "small_k3_s2_odd", "pw_c8_4",
              "pw_c6_128_elu", "halo_2x2", "halo_3x3_ks1", "s2d_k3_even", "s2d_k4_reflect", "tap_c3_7x7_s2", "tap_c4_1x7_rep")
SPLIT_K_TAGS = ("gen_k2304", "halo_3x3_planner")
_EDGE = {c.tag: c for c in cs.EDGE}


def _leaky_case(tag):
    c = _EDGE[tag]
    assert c.act == L.ACT_NONE and c.res == 0 and c.out == "nhwc" and c.qwin is None and not c.per_sample, c
    return c


def _launch_leaky(c, inp, prec):
    plan = cs.make_plan(c, inp["w"], inp["b"])
    x0 = ops.as_nhwc(inp["x0"].contiguous().to(DEV), cpad=c.cin_pad)
    y = ops.conv(plan, x0, None, pre_op=cs.PRE[c.pre], act=L.ACT_LEAKY02, precision=prec, ksplit=c.ksplit)
    fam = ops.last_conv_kernel()
    return y.cpu().double(), fam, plan


@pytest.mark.parametrize("tag", LEAKY_TAGS)
def test_leaky_epilogue_in_every_conv_family(tag):
    """conv_sweep's float64 reference without an activation, LeakyReLU(0.2) applied in float64, judged by conv_sweep's
    comparator at the bar of the family that ran - which must be the family the edge table records for the row."""
    c = _leaky_case(tag)
    assert c.c1 == 0 and not c.pre.startswith("affine")
    inp = cs.inputs(c)
    ref, den = cs.reference(c, inp)
    ref = F.leaky_relu(ref, 0.2)
    for prec in PRECS:
        y, fam, plan = _launch_leaky(c, inp, prec)
        assert fam == c.expect[cs.PRECISIONS.index(prec)], (tag, prec, fam)
        err = cs.norm_err(y, ref, den)
        record(f"leaky_err_over_bar_{prec}", err / cs.bar(fam))
        assert err <= cs.bar(fam), (tag, prec, fam, err)
        assert not ops.range_exceeded(torch.device(DEV))
        if tag in SPLIT_K_TAGS:                   # the K-split reduce applies the activation, not the partial launches
            ho, wo = c.full_hw()
            assert cs.plan_ksplit(c.B * ho * wo, plan.cout_pad, plan.k_pad, prec == "f16x3")[1] > 1, tag


@pytest.mark.parametrize("tag", ("gen_c12_3x3", "pw_c8_4", "halo_2x2"))
def test_leaky_epilogue_keeps_a_nan(tag):
    """v > 0 ? v : 0.2 v: a NaN input element comes out as NaN wherever the float64 reference has one, nowhere else."""
    c = _leaky_case(tag)
    inp = cs.inputs(c)
    inp["x0"][0, 0, c.H // 2, c.W // 2] = float("nan")
    ref, den = cs.reference(c, inp)
    ref = F.leaky_relu(ref, 0.2)
    y, fam, _ = _launch_leaky(c, inp, "f32")
    nan = torch.isnan(ref)
    assert bool(nan.any()) and not bool(nan.all())
    assert torch.equal(torch.isnan(y), nan), (tag, fam)
    ok = ~nan
    assert float(((y - ref).abs() / den)[ok].max()) <= cs.bar(fam)
    ops.range_exceeded(torch.device(DEV))


def test_leaky_in_the_row_split_head():
    """pack_conv_rowsplit + fusg_hshift_sum: the horizontal gather-sum applies the activation."""
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 32, 16, 24, generator=g)
    w = torch.randn(3, 32, 7, 7, generator=g) / (32 * 49) ** 0.5
    b = torch.randn(3, generator=g)
    xp = F.pad(x.double(), (3, 3, 3, 3), mode="reflect")
    ref = F.leaky_relu(F.conv2d(xp, w.double(), b.double()), 0.2)
    den = F.conv2d(xp.abs(), w.double().abs()) + b.double().abs().view(1, -1, 1, 1)
    plan = pack.pack_conv_rowsplit(w, b, pad=3, pad_mode=L.PAD_REFLECT).to(torch.device(DEV))
    for prec in PRECS:
        with ops.precision(prec):
            y = ops.conv_rowsplit(plan, ops.as_nhwc(x.to(DEV)), act=L.ACT_LEAKY02)
        assert bool((ref < 0).any()) and cs.norm_err(y, ref, den) <= cs.BAR_FP32, prec
    assert not ops.range_exceeded(torch.device(DEV))


def test_affine_act_leaky_is_torch_bit_for_bit_on_a_pitched_slice():
    g = torch.Generator().manual_seed(5)
    buf = torch.full((2, 9, 11, 24), float("nan"))
    buf[..., 8:16] = torch.randn(2, 9, 11, 8, generator=g)
    buf[0, 0, 0, 8] = float("nan")
    x = buf.to(DEV).permute(0, 3, 1, 2)[:, 8:16]
    scale, shift = torch.randn(2, 8, generator=g).to(DEV), torch.randn(2, 8, generator=g).to(DEV)
    y = ops.affine_act(x, scale, shift, L.ACT_LEAKY02)
    # fmaf in the kernel: the product is not rounded before the sum, so the yardstick is the float64 product rounded once
    aff = (x.double() * scale.double()[:, :, None, None] + shift.double()[:, :, None, None]).float()
    want = F.leaky_relu(aff, 0.2)
    assert bool(torch.isnan(y[0, 0, 0, 0])) and int(torch.isnan(y).sum()) == 1

    def bits(t):                                  # (a NaN's payload is nobody's promise)
        return _bits(torch.nan_to_num(t, nan=0.0).cpu().numpy())
    assert np.array_equal(bits(y), bits(want))
    plain = ops.affine_act(x, None, None, L.ACT_LEAKY02)
    assert bool(torch.isnan(plain[0, 0, 0, 0])) and np.array_equal(bits(plain), bits(F.leaky_relu(x, 0.2)))


# ---- pool, mask multiply, GAN terms against the host twins -----------------------------------------------------------------
def _pitched(t, pitch, off, fill):
    """`t` [B, C, H, W] as channels off .. off + C of an NHWC buffer of `pitch` channels filled with `fill`: (view, buffer)."""
    b, c, h, w = t.shape
    buf = torch.full((b, h, w, pitch), fill, device=DEV)
    view = buf.permute(0, 3, 1, 2)[:, off:off + c]
    view.copy_(t.to(DEV))
    return view, buf


@pytest.mark.parametrize("shape", cc.POOL_SHAPES)
def test_avgpool3s2_equals_its_host_twin_inside_canaries(shape):
    x = cc.pool_input(shape)
    want = ops.avgpool3s2_host(x.numpy())
    got = ops.avgpool3s2(x.to(DEV))
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    b, c, h, w = shape
    src, _ = _pitched(x, 16, 4, float("nan"))
    dst, buf = _pitched(torch.zeros(want.shape), 16, 8, CANARY)
    L.check(L.lib().fusg_avgpool3s2_f32(C.byref(ops.desc(src)), C.byref(ops.desc(dst)), ops.stream_ptr()), "avgpool3s2")
    assert np.array_equal(_bits(dst.cpu().numpy()), _bits(want))
    whole = buf.cpu()
    assert bool((whole[..., :8] == CANARY).all()) and bool((whole[..., 8 + c:] == CANARY).all())


def test_mask_mul_equals_the_float32_product_inside_canaries():
    g = torch.Generator().manual_seed(9)
    x, m = torch.randn(2, 3, 7, 9, generator=g), (torch.rand(2, 1, 7, 9, generator=g) < 0.5).float() * 0.75
    want = (x * m).numpy()
    assert np.array_equal(_bits(ops.mask_mul(x.to(DEV), m.to(DEV)).cpu().numpy()), _bits(want))
    src, _ = _pitched(x, 8, 4, float("nan"))
    dst, buf = _pitched(torch.zeros(x.shape), 12, 4, CANARY)
    ops.mask_mul(src, m.to(DEV), out=dst)
    assert np.array_equal(_bits(dst.cpu().numpy()), _bits(want))
    whole = buf.cpu()
    assert bool((whole[..., :4] == CANARY).all()) and bool((whole[..., 7:] == CANARY).all())


def test_gan_terms_equal_the_host_twin_and_rows_do_not_depend_on_the_batch():
    for name, (pred, label, mask) in cc.gan_term_cases(ops.gan_terms_chunk).items():
        want = ops.gan_terms_host(pred.numpy(), label, None if mask is None else mask.numpy())
        pd = pred.to(DEV)
        if name == "pitched_slice":               # the same strided view on the device
            pd = pred._base.to(DEV).permute(0, 3, 1, 2)[:, 4:9]
            assert pd.stride() == pred.stride()
        md = None if mask is None else mask.to(DEV)
        got = ops.gan_terms(pd, label, md).cpu().numpy()
        assert _same(got, want), name
        alone = ops.gan_terms(pd[1:2], label, None if md is None else md[1:2]).cpu().numpy()
        assert _same(alone, got[1:2]), name


# ---- the networks -------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(case):
    """The float64 restatement's maps of inputs 'a' and 'b', computed once per case."""
    if case not in _REF:
        sd = cc.state_dict(case)
        xa, xb = cc.inputs(case)
        if cc.CASES[case][0] == "dis":
            _REF[case] = (cr.discriminator(sd, xa), cr.discriminator(sd, xb))
        else:
            _REF[case] = (cr.nlayers_multi(sd, xa), cr.nlayers_multi(sd, xb))
    return _REF[case]


_NETS = {}


def _net(case):
    key = cc.net_name(case)
    if key not in _NETS:
        from future_urban_scene_generation_amd.edgeconnect.networks import Discriminator
        from future_urban_scene_generation_amd.warp_learn.models import D_NLayersMulti
        net, c = cc.CASES[case][:2]
        m = D_NLayersMulti(c) if net == "icn" else Discriminator(c, use_sigmoid=True)
        m.load_state_dict(cc.state_dict(case))
        _NETS[key] = m.to(DEV).eval()
    return _NETS[key]


def _check_map(g, name, dev_map, ref64, bar=1e-4):
    """max |device - float64| / max |float64| over the whole map, and the same through the fixture's corner and channel sums."""
    d = dev_map.cpu().double()
    top = float(ref64.abs().max())
    err = float((d - ref64).abs().max()) / top
    assert err <= bar, (name, err)
    e_ref = float(g[name + "_E"])
    assert float(np.abs(d[:, :, :2, :2].numpy() - g[name + "_corner"]).max()) <= (bar + e_ref) * top, name
    hw = ref64.shape[2] * ref64.shape[3]
    assert float(np.abs(d.sum((2, 3)).numpy() - g[name + "_chsum"]).max()) <= bar * top * hw, name
    return err, e_ref


def _conv_families(monkeypatch):
    fams = []
    real = ops.conv

    def conv(*a, **k):
        out = real(*a, **k)
        fams.append(ops.last_conv_kernel())
        return out
    monkeypatch.setattr(ops, "conv", conv)
    return fams


@pytest.mark.parametrize("case", cc.DIS_CASES)
def test_discriminator_maps_and_scalars(case, monkeypatch):
    """Observed on MI355X (conftest.record keeps the figures): every map within 2.0e-6 of the float64 restatement relative
    to the map's maximum, 0.5 to 3.7 x the reference's own float32 error E_ref, under f16x3 and f32 alike (bar 1e-4); the
    scalars within 2 % of their Lipschitz bounds; each scalar equal to the host twin's on the device's own values."""
    from future_urban_scene_generation_amd.edgeconnect.loss import AdversarialScore, feature_matching
    g = gold(case)
    (oa64, fa64), (ob64, fb64) = _reference(case)
    d = _net(case)
    xa, xb = (t.to(DEV) for t in cc.inputs(case))
    h = cc.CASES[case][3]
    for prec in PRECS:
        fams = _conv_families(monkeypatch) if prec == PRECS[0] else fams
        del fams[:]
        with ops.precision(prec):
            oa, fa = d(xa)
            ob, fb = d(xb)
        assert len(fams) == 10
        for name, m, r in zip(cc.DIS_MAPS, fa, fa64):
            err, e_ref = _check_map(g, name, m, r)
            record(f"{name}_err_{prec}", err)
            print(f"{case} {prec} {name}: err {err:.2e} = {err / e_ref:.1f} x E_ref")
        top = float(fa64[4].abs().max())
        assert float((fa[4].cpu().double() - torch.from_numpy(g["conv5_a64"])).abs().max()) <= 1e-4 * top
        assert float((fb[4].cpu().double() - torch.from_numpy(g["conv5_b64"])).abs().max()) <= 1e-4 * float(fb64[4].abs().max())
        assert float((oa.cpu().double() - oa64).abs().max()) <= 1e-4 * top          # sigmoid is 1/4-Lipschitz
        # scalars: within L delta of the float64 fixture, delta = 1e-4 max |logit|, L the term's Lipschitz constant
        delta = 1e-4 * top
        for kind in cc.ADV_TYPES:
            score = AdversarialScore(kind)
            o_dev, o64 = (fa[4], fa64[4]) if kind == "hinge" else (oa, oa64)
            host_terms = {lab: ops.gan_terms_host(o_dev.cpu().numpy(), lab) for lab in (0.0, 1.0)}
            for is_real, is_disc in cc.ADV_CALLS:
                key = f"adv_{kind}_{int(is_real)}{int(is_disc)}"
                got = score(o_dev, is_real, is_disc)
                assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
                t = 1.0 if is_real else 0.0
                lip = 2 * (float((o64 - t).abs().max()) + delta) if kind == "lsgan" else 1.0
                diff = abs(float(got) - float(g[key + "_64"]))
                record(f"{key}_over_bound_{prec}", diff / (lip * delta))
                assert diff <= lip * delta, (key, prec, diff, lip * delta)
                # the reduction alone: the same formula on the host twin's sums of the device's own values
                ht = host_terms[t]
                n = ht[:, 0].sum()
                if kind == "hinge":
                    v = ht[:, 4 if is_real else 3].sum() / n if is_disc else -(ht[:, 1].sum() / n)
                else:
                    v = ht[:, 5 if kind == "nsgan" else 2].sum() / n
                assert abs(float(got) - v) <= U * abs(v), (key, prec)
        fm = feature_matching(fb, fa)
        bound = sum(1e-4 * max(float(ra.abs().max()), float(rb.abs().max())) for ra, rb in zip(fa64, fb64))
        diff = abs(float(fm) - float(g["fm_64"]))
        record(f"fm_over_bound_{prec}", diff / bound)
        assert fm.dtype == torch.float32 and diff <= bound, (prec, diff, bound)
        host_fm = sum(ops.abs_diff_rows_host(a.cpu().numpy(), b.cpu().numpy()).sum() / a.numel() for a, b in zip(fb, fa))
        assert abs(float(fm) - host_fm) <= U * host_fm
    assert not ops.range_exceeded(torch.device(DEV))


@pytest.mark.parametrize("case", [c for c in cc.DIS_CASES if cc.CASES[c][3] >= 64])
def test_discriminator_stride2_convs_run_the_halo_quadrant_form(case, monkeypatch):
    """conv2 and conv3 on the halo kernel's stride-2 (parity-quadrant) form: HALO_S2D under f16x3, the same kernel's exact-fp32
    mode (HALO_F32) under f32.  Discriminator keeps K whole for them (on few images the planner would split K, and a split
    launch takes the generic gather); at 64 x 64 conv3's 8 x 8 outputs are half a patch narrower than the kernel's 8 x 16
    pixels, and the layer runs on a copy widened by zero columns (Discriminator._stride2)."""
    d = _net(case)
    xa, _ = (t.to(DEV) for t in cc.inputs(case))
    fams = _conv_families(monkeypatch)
    for prec in PRECS:
        del fams[:]
        with ops.precision(prec):
            d(xa)
        want = cs.HALO_S2D if prec == "f16x3" else cs.HALO_F32
        print(f"{case} {prec}: conv families {fams}")
        assert fams[1] == want and fams[2] == want, (case, prec, fams)


@pytest.mark.parametrize("case", cc.ICN_CASES)
def test_nlayers_multi_maps_and_gan_loss(case):
    """Observed on MI355X: every map, the InstanceNorm'd ones included, within 1.2e-6 of the float64 restatement relative to
    the map's maximum, 0.5 to 1.3 x E_ref, under both precisions (bars 1e-4 and max(1e-4, 16 E_ref))."""
    from future_urban_scene_generation_amd.warp_learn.models import GANLoss
    g = gold(case)
    ma64, mb64 = _reference(case)
    d = _net(case)
    xa, _ = (t.to(DEV) for t in cc.inputs(case))
    mask = cc.mask(case)
    loss = GANLoss()
    for prec in PRECS:
        with ops.precision(prec):
            maps = d.features(xa)
            preds = d(xa)
        assert len(preds) == 2 and all(torch.equal(p, m[-1]) for p, m in zip(preds, maps))
        for s in range(2):
            for name, m, r in zip(cc.ICN_MAPS, maps[s], ma64[s]):
                full = f"s{s}_{name}"
                bar = max(1e-4, 16 * float(g[full + "_E"])) if name.startswith("norm") else 1e-4
                err, e_ref = _check_map(g, full, m, r, bar)
                record(f"{full}_err_{prec}", err)
                print(f"{case} {prec} {full}: err {err:.2e} = {err / e_ref:.1f} x E_ref")
            assert float((preds[s].cpu().double() - torch.from_numpy(g[f"s{s}_logits_a64"])).abs().max()) \
                <= 1e-4 * float(ma64[s][-1].abs().max())
        for nm, real in (("real", True), ("fake", False)):
            t = 1.0 if real else 0.0
            bound = 0.0
            for s in range(2):
                delta = 1e-4 * float(ma64[s][-1].abs().max())
                bound += 2 * (float((ma64[s][-1] - t).abs().max()) + delta) * delta
            for mtag, mk in (("", None), ("_mask", mask)):
                got = loss(preds, real, mask=None if mk is None else mk.to(DEV))
                assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
                want = float(g[f"gan_{nm}{mtag}_64"])
                record(f"gan_{nm}{mtag}_over_bound_{prec}", abs(float(got) - want) / bound)
                assert abs(float(got) - want) <= bound, (nm, mtag, prec)
                host = 0.0
                for p in preds:
                    ht = ops.gan_terms_host(p.cpu().numpy(), t, None if mk is None else mk.numpy())
                    host += ht[:, 2].sum() / ht[:, 0].sum()
                assert abs(float(got) - host) <= U * host
    # do_smooth draws torch.rand(1) per scale from the CPU generator, as the reference does
    torch.manual_seed(3)
    smooth = loss(preds, True, do_smooth=True)
    torch.manual_seed(3)
    want = 0.0
    for p in preds:
        lab = float(torch.tensor(1.0) + (torch.rand(1) - 0.5) / 2.0)
        ht = ops.gan_terms_host(p.cpu().numpy(), lab)
        want += ht[:, 2].sum() / ht[:, 0].sum()
    assert abs(float(smooth) - want) <= U * want
    assert not ops.range_exceeded(torch.device(DEV))


# ---- evaluate -----------------------------------------------------------------------------------------------------------
def _count_d2h(monkeypatch):
    calls = {"d2h": 0}
    real = ops.d2h
    monkeypatch.setattr(ops, "d2h", lambda t: (calls.__setitem__("d2h", calls["d2h"] + 1), real(t))[1])
    return calls


def _eval_inputs():
    i = synth_inputs("edge", 2, 64)
    return {k: v.to(DEV) for k, v in i.items()}


def test_edge_model_evaluate_equals_its_pieces(monkeypatch):
    from conftest import load_schema
    from future_urban_scene_generation_amd.edgeconnect.loss import feature_matching
    from future_urban_scene_generation_amd.edgeconnect.models import EdgeModel
    m = EdgeModel(None, discriminator=True)
    m.generator.load_state_dict(synth_state_dict("edge", load_schema("edge")))
    m.discriminator.load_state_dict(synth_state_dict("edge_dis", cc.schema("Discriminator2")))
    m = m.to(DEV).eval()
    i = _eval_inputs()
    calls = _count_d2h(monkeypatch)
    outputs, (names, logs) = m.evaluate(i["gray"], i["edge"], i["mask"])
    assert calls["d2h"] == 0
    assert names == ("l_d1", "l_g1", "l_fm") and logs.dtype == torch.float64 and tuple(logs.shape) == (3,) and logs.is_cuda
    out2 = m(i["gray"], i["edge"], i["mask"])
    assert torch.equal(outputs, out2)
    adv = m.adversarial_loss
    real, real_feat = m.discriminator(torch.cat((i["gray"], i["edge"]), 1))
    fake, fake_feat = m.discriminator(torch.cat((i["gray"], ops.to_nchw(out2)), 1))
    want = torch.stack([((adv(real, True, True) + adv(fake, False, True)) / 2).double(), adv(fake, True, False).double(),
                        (feature_matching(fake_feat, real_feat) * 10).double()])
    assert bool(torch.isfinite(logs).all()) and np.array_equal(_bits(logs.cpu().numpy()), _bits(want.cpu().numpy()))


def test_inpainting_model_evaluate_equals_its_pieces(monkeypatch):
    from conftest import load_schema
    from future_urban_scene_generation_amd.edgeconnect.loss import VGG19, PerceptualLoss, StyleLoss
    from future_urban_scene_generation_amd.edgeconnect.models import InpaintingModel
    m = InpaintingModel(None, discriminator=True)
    m.generator.load_state_dict(synth_state_dict("inpaint", load_schema("inpaint")))
    m.discriminator.load_state_dict(synth_state_dict("inpaint_dis", cc.schema("Discriminator3")))
    m = m.to(DEV).eval()
    vgg = VGG19().to(DEV)
    i = _eval_inputs()
    calls = _count_d2h(monkeypatch)
    outputs, (names, logs) = m.evaluate(i["img"], i["edge"], i["mask"], vgg=vgg)
    _, (_, no_vgg) = m.evaluate(i["img"], i["edge"], i["mask"])
    assert calls["d2h"] == 0
    assert names == ("l_d2", "l_g2", "l_l1", "l_per", "l_sty") and logs.dtype == torch.float64 and tuple(logs.shape) == (5,)
    assert bool(torch.isnan(no_vgg[3:]).all()) and np.array_equal(_bits(no_vgg[:3].cpu().numpy()), _bits(logs[:3].cpu().numpy()))
    out2 = ops.to_nchw(m(i["img"], i["edge"], i["mask"]))
    adv = m.adversarial_loss
    real, _ = m.discriminator(i["img"])
    fake, _ = m.discriminator(out2)
    per, sty = PerceptualLoss().to(DEV), StyleLoss().to(DEV)
    l1 = (ops.abs_diff_rows(out2, i["img"]).sum() / out2.numel()).float()
    want = torch.stack([((adv(real, True, True) + adv(fake, False, True)) / 2).double(), (adv(fake, True, False) * 0.01).double(),
                        (l1 * 1 / i["mask"].double().mean().float()).double(), (per(out2, i["img"]) * 1).double(),
                        (sty(out2 * i["mask"], i["img"] * i["mask"]) * 1).double()])
    assert bool(torch.isfinite(logs).all()) and np.array_equal(_bits(logs.cpu().numpy()), _bits(want.cpu().numpy()))


def test_recorded_discriminator_pass_replays_bit_identically():
    case = "dis3_b2_32x48"
    d = _net(case)
    xa, xb = (t.to(DEV) for t in cc.inputs(case))
    eager = [[t.cpu().numpy() for t in [o] + f] for o, f in (d(xa), d(xb))]
    torch.cuda.synchronize()
    lib = L.lib()
    pool = torch.cuda.MemPool()
    rec = ops.PlanRecorder()
    try:
        with torch.cuda.use_mem_pool(pool, device=torch.device(DEV)):
            bx = xa.clone()
            L.check(lib.fusg_plan_begin(rec.handle), "plan_begin")
            ops.RECORDER = rec
            try:
                out, feats = d(bx)
            finally:
                ops.RECORDER = None
                L.check(lib.fusg_plan_end(rec.handle), "plan_end")
        torch.cuda.synchronize()
        for x, want in ((xb, eager[1]), (xa, eager[0])):
            bx.copy_(x)
            L.check(lib.fusg_plan_run(rec.handle), "plan_run")
            torch.cuda.synchronize()
            for t, w in zip([out] + feats, want):
                assert np.array_equal(_bits(t.cpu().numpy()), _bits(w))
    finally:
        torch.cuda.synchronize()
        lib.fusg_plan_destroy(rec.handle)
