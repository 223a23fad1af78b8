"""CPU: the elementwise sweep's own machinery (tests/eltwise_sweep.py) - its references against the torch / oracle forms of
the same ops, the coverage of every route and listed edge by the case lists (through the restated routers), the accepted
parameters of fusg_hshift_sum against a brute-force walk of the indices its two kernels form, the recorded transcendental
bar against a fresh measurement, and per op a list of plausible wrong variants that the cases must tell from the reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eltwise_sweep as es
import oracle
from emu import emulate_conv, assemble_normal
from future_urban_scene_generation_amd import pack


def small(cases):
    return [c for c in cases if not c.p.get("big")]


def nhwc(view: torch.Tensor) -> np.ndarray:
    return view.permute(0, 2, 3, 1).numpy()


# ---- the references agree with the existing forms ---------------------------------------------------------------------------
def test_pool_and_upsample_references_match_torch():
    for c in small(es.pool_cases()):
        x = es.pool_inputs(c)["x"][0]
        assert es.same_bits(es.ref_maxpool2(x.numpy()), F.max_pool2d(x.contiguous(), 2, stride=2).numpy()), c
    for c in small(es.upsample_cases()):
        d = es.upsample_inputs(c)
        low, up1 = d["low"][0].contiguous(), d["up1"][0].contiguous()
        want = up1 + F.interpolate(low, scale_factor=2, mode="nearest")
        assert es.same_bits(es.ref_upsample2_add(low.numpy(), up1.numpy()), want.numpy()), c


def test_s2d_d2s_references_match_the_oracle():
    for c in es.s2d_cases():
        x = es.s2d_inputs(c)["x"][0].contiguous()
        if c.op == "s2d":
            assert es.same_bits(es.ref_s2d(x.numpy()), oracle.space_to_depth(x).contiguous().numpy()), c
        else:
            assert es.same_bits(es.ref_d2s(x.numpy()), oracle.depth_to_space(x).contiguous().numpy()), c
            assert es.same_bits(es.ref_s2d(es.ref_d2s(x.numpy())), x.numpy()), c


def test_u8_and_argmax_references_match_the_oracle():
    for c in es.u8_cases():
        x = es.u8_input(c).contiguous()
        assert np.array_equal(es.ref_to_image_u8(x.numpy()), oracle.to_image_u8(x)), c
    for c in es.argmax_cases():
        x = es.argmax_input(c).contiguous()
        assert np.array_equal(es.ref_argmax_hw(x.numpy()), oracle.heatmap_argmax(x)), c
    for c in es.merge_cases():                    # trajectory_inference.py:126-129 on float32 tensors, truncated by astype
        o, img, m = (t.contiguous() for t in es.merge_inputs(c))
        want = np.clip(((o * m + img * (1 - m)) * 255).numpy(), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
        assert np.array_equal(es.ref_merge_u8(o.numpy(), img.numpy(), m.numpy()), want), c


def test_ec_inputs_and_copy_references():
    for c in es.ec_cases():
        img, e, m = (t.contiguous() for t in es.ec_inputs_of(c))
        merged = img * (1 - m) + m                # edgeconnect/models.py:130-133, 236-238
        want = torch.cat([merged, e * (1 - m), m, torch.zeros_like(m)], 1) if c.mode == 0 else torch.cat([merged, e], 1)
        assert es.same_bits(es.ref_ec_inputs(img.numpy(), e.numpy(), m.numpy(), c.mode), want.numpy()), c
    for c in es.copy_cases():
        if c.dst != "nhwc":
            continue
        src = es.copy_inputs(c)
        buf = es.ref_copy4d_buffer(src.numpy(), c.pitch, c.c_off, c.fill)
        f = buf.view(np.float32)
        assert es.same_bits(f[..., c.c_off:c.c_off + c.C], nhwc(src)), c
        end = max(c.C, c.fill)
        assert np.all(buf[..., c.c_off + c.C:c.c_off + end] == 0) and np.all(buf[..., :c.c_off] == es.CANARY), c
        assert np.all(buf[..., c.c_off + end:] == es.CANARY) and c.c_off + end < c.pitch, c


@pytest.mark.parametrize("pm", [es.PAD_ZERO, es.PAD_REFLECT])
def test_hshift_reference_composes_with_the_rowsplit_packing_into_the_conv(pm):
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(2, 8, 9, 10, generator=g), torch.randn(3, 8, 7, 7, generator=g) * 0.1, torch.randn(3, generator=g)
    plan = pack.pack_conv_rowsplit(w, b, pad=3, pad_mode=pm)
    t = assemble_normal(plan, emulate_conv(plan, x))                                    # [B, 21, H, W]
    got = es.ref_hshift_sum(nhwc(t), b.numpy(), 7, 3, pm, 3)
    ref = F.conv2d(F.pad(x, (3,) * 4, mode="reflect"), w, b) if pm else F.conv2d(x, w, b, padding=3)
    torch.testing.assert_close(torch.from_numpy(got), ref, rtol=1e-4, atol=1e-4)


def test_affine_reference_matches_torch_float64():
    acts = {es.NONE: lambda v: v, es.RELU: torch.relu, es.TANH: torch.tanh, es.SIGMOID: torch.sigmoid,
            es.TANH01: lambda v: (torch.tanh(v) + 1) / 2}
    for c in small(es.affine_cases()):
        x, sc, sh, res = es.affine_logical(es.affine_inputs(c), c)
        assert not any(np.isnan(a).any() for a in (x, sc, sh, res) if a is not None), c
        v = torch.from_numpy(x).double()
        if sc is not None:
            v = v * torch.from_numpy(sc).double()[:, :, None, None] + torch.from_numpy(sh).double()[:, :, None, None]
        v = acts[c.act](v)
        if res is not None:
            v = v + torch.from_numpy(res).double()
        ref, _ = es.ref_affine_act(x, sc, sh, c.act, res)
        np.testing.assert_allclose(ref, v.numpy(), rtol=1e-14, atol=1e-15)


# ---- every route and every listed edge has a case ---------------------------------------------------------------------------
def test_capped_launches_are_crossed_and_the_small_cases_are_not():
    for cases, count in ((es.affine_cases(), lambda c: c.B * c.H * c.W * c.C // 4),
                         (es.pool_cases(), lambda c: c.B * c.Ho * c.Wo * c.C // 4),
                         (es.upsample_cases(), lambda c: c.B * c.H * c.W * c.C // 4)):
        big = [c for c in cases if c.big]
        assert len(big) == 1 and es.over_cap(count(big[0])), big
        assert not any(es.over_cap(count(c)) for c in small(cases))


def test_affine_cases_cover_every_form():
    cs = small(es.affine_cases())
    for ch in (4, 12, 64):
        mine = [c for c in cs if c.C == ch]
        assert {(c.act, c.res) for c in mine} == {(a, r) for a in es.ACTS for r in (False, True)}
        assert {c.scale for c in mine} == {"null", "tight", "wide"} and {c.dst_off for c in mine} == {0, 4}
    for act in es.ACTS:                           # every activation meets every scale form and both destinations
        assert {c.scale for c in cs if c.act == act} == {"null", "tight", "wide"}, act
        assert {c.dst_off for c in cs if c.act == act} == {0, 4}, act
    d = es.affine_inputs(cs[1])
    assert d["x"][0].stride(3) == cs[1].C + 4 and d["res"][0].stride(3) == cs[1].C + 8 and d["res"][0].storage_offset() == 4


def test_copy_cases_cover_both_routes_and_the_transpose_edges():
    cs = es.copy_cases()
    routes = {}
    for c in cs:
        routes.setdefault(es.copy_route_of(c), []).append(c)
    assert set(routes) == {"transpose", "generic"}
    tr = routes["transpose"]
    assert {c.C for c in tr} == {1, 3, 5, 32} and all(c.C == 33 or c.src != "nchw" or c.dst != "nhwc" for c in routes["generic"])
    assert {(c.H, c.W) for c in tr} == {(5, 7), (16, 16), (1, 257), (12, 25)}
    assert any(c.H * c.W > 256 and c.H * c.W % 256 for c in tr) and any(c.H * c.W == 256 for c in tr)
    for ch in (1, 3, 5, 32):                      # no fill, fill to the next multiple of 4, fill to 32; the pitch beyond all
        assert {c.fill for c in tr if c.C == ch} == {0, (ch + 3) // 4 * 4, 32}
    assert all(c.pitch > c.c_off + max(c.C, c.fill) for c in cs if c.dst == "nhwc")
    assert {c.c_off for c in tr} == {0, 4}
    assert {c.src for c in routes["generic"]} == {"nchw", "batch_sliced", "nhwc_slice"}
    assert not es.copy_inputs([c for c in cs if c.src == "batch_sliced"][0]).is_contiguous()


def test_hshift_cases_cover_both_routes_and_every_edge():
    cs = es.hshift_cases()
    by = {}
    for c in cs:
        by.setdefault(es.hshift_route_of(c), []).append(c)
    assert set(by) == {"lds", "direct"}
    lds, direct = by["lds"], by["direct"]
    assert {c.pitch for c in lds} >= {4, 8, 24, 32} and all(c.pitch <= 32 for c in lds)
    assert any(c.pitch > 32 for c in direct) and any(c.pitch <= 32 and c.W <= 2 * c.pad for c in direct)
    assert any(c.pitch <= 32 and c.W > 2 * c.pad and c.kw - 1 > 2 * c.pad and c.W > 256 for c in direct)     # the lopsided window
    assert any(c.kw != 2 * c.pad + 1 for c in lds)
    for pm in (es.PAD_ZERO, es.PAD_REFLECT):
        mine = [c for c in lds if c.pm == pm]
        assert any(c.W == 2 * c.pad + 1 for c in mine) and any(c.W == 256 for c in mine)
        assert any(c.W == 257 for c in mine) and any(c.W > 512 for c in mine)                               # one and two seams
        assert any(c.W > 256 and 0 < c.W - 256 < c.pad for c in mine)                                       # a last segment narrower than pad
        assert any(c.pad == 0 for c in mine)
    assert all(es.hshift_accepts(c.kw, c.pad, c.pm, c.W) for c in cs)
    assert not any(es.hshift_accepts(kw, pad, pm, w) for kw, pad, pm, w, _, _ in es.hshift_rejects())


def _hshift_indices_ok(kw, pad, pm, w, route):
    """Walk the indices the kernel of `route` forms for a row of width w: the direct kernel's row offsets must lie in
    [0, w); the LDS kernel's tile index in [0, 256 + 2*pad) and on a pixel that the staging loop loaded (0 <= gx < w)."""
    for x in range(w):
        x0 = x // 256 * 256
        for kx in range(kw):
            xx = x + kx - pad
            if pm == es.PAD_REFLECT:
                xx = -xx if xx < 0 else (2 * w - 2 - xx if xx >= w else xx)
            elif not 0 <= xx < w:
                continue
            if route == "direct":
                if not 0 <= xx < w:
                    return False
            else:
                ti = xx - x0 + pad
                if not (0 <= ti < 256 + 2 * pad and 0 <= xx < w):
                    return False
    return True


def test_hshift_accepts_is_what_the_kernels_can_index():
    """Everything accepted is in bounds on the route it takes; everything that the tightened checks turn away (beyond
    the old ones: kw <= 15, 0 <= pad < W) either leaves the row or is a window without its own pixel; and a window with
    kw - 1 > 2*pad would leave the LDS tile on a long row, which is why it is routed to the direct kernel."""
    widths = (1, 2, 3, 5, 8, 14, 15, 20, 255, 256, 257, 262, 300, 513)
    left_tile = False
    for kw in range(1, 16):
        for pad in range(0, 17):
            for pm in (es.PAD_ZERO, es.PAD_REFLECT):
                for w in widths:
                    if pad >= w:
                        assert not es.hshift_accepts(kw, pad, pm, w)
                        continue
                    if es.hshift_accepts(kw, pad, pm, w):
                        for pitch in (8, 36):
                            assert _hshift_indices_ok(kw, pad, pm, w, es.hshift_route(pitch, pad, w, True, kw)), (kw, pad, pm, w)
                        if kw - 1 > 2 * pad and w > 2 * pad:
                            left_tile |= not _hshift_indices_ok(kw, pad, pm, w, "lds")
                    else:
                        assert kw - 1 - pad < 0 or not _hshift_indices_ok(kw, pad, pm, w, "direct"), (kw, pad, pm, w)
    assert left_tile
    assert es.hshift_accepts(7, 3, es.PAD_REFLECT, 4) and not es.hshift_accepts(7, 3, es.PAD_REFLECT, 3)
    assert es.hshift_accepts(9, 1, es.PAD_ZERO, 7) and not es.hshift_accepts(9, 1, es.PAD_REFLECT, 7)
    assert es.hshift_route(16, 1, 300, True, 7) == "direct" and es.hshift_route(16, 3, 300, True, 7) == "lds"


def test_argmax_pool_u8_and_ec_edges():
    for c in es.argmax_cases():
        x = es.argmax_input(c)
        hw, ref = c.H * c.W, es.ref_argmax_hw(x.numpy())
        flat = x.reshape(c.B, len(es.ARGMAX_KINDS), hw).numpy()
        assert not np.isnan(flat).any()
        assert (ref[:, 3] == hw - 1).all() and (ref[:, 4] == 0).all() and (ref[:, 5] == 0).all(), c
        if hw > 256:
            assert all(flat[b, 1, ref[b, 1]] == flat[b, 1, ref[b, 1] + 256] for b in range(c.B)), c
        if hw > 2:
            assert all(flat[b, 2, ref[b, 2]] == flat[b, 2, ref[b, 2] + 1] for b in range(c.B)), c
    assert {(c.H, c.W) for c in es.argmax_cases()} == {(1, 1), (1, 7), (5, 51), (16, 16), (1, 257), (64, 64)}
    assert any(np.isnan(es.pool_inputs(c)["x"][0].numpy()).any() for c in es.pool_cases() if c.kind == "nan")
    assert all(np.isneginf(es.ref_maxpool2(es.pool_inputs(c)["x"][0].numpy())).any() for c in es.pool_cases() if c.kind == "inf")
    for c in es.u8_cases():
        x = es.u8_input(c).reshape(-1).numpy().astype(np.float64)
        v = (x + 1) / 2 * 255                    # around every threshold k: values on both sides within two ulp
        for k in range(1, 256):
            near = v[np.abs(v - k) < 1e-4]
            assert (near < k).any() and (near >= k).any(), (c, k)
        assert (x > 1).any() and (x < -1).any() and np.signbit(x[x == 0]).any()
    assert {(c.mode, c.mask, c.pitch) for c in es.ec_cases()} == {(mo, ma, p) for mo in (0, 1) for ma in ("binary", "fractional") for p in (4, 8)}
    assert any(not t.is_contiguous() for c in es.ec_cases() if c.lay == "strided" for t in es.ec_inputs_of(c))
    for c in es.merge_cases():
        o, img, m = (t.numpy() for t in es.merge_inputs(c))
        assert ((m > 0) & (m < 1)).any() and (o < 0).any() and (o > 1).any() and (img < 0).any() and (img > 1).any()


def test_recorded_activation_bars_are_four_times_a_fresh_measurement():
    """The bars are 4x the error torch's float32 shows against float64 on the cases' own inputs.  Another host libm may move
    the measurement a little: the record has to hold to within a factor of two, and the bars are exactly four times the record."""
    a, h = es.measure_act_error()
    assert es.ACT_BAR_AFFINE == 4 * es.ACT_ERR_AFFINE and es.ACT_BAR_HSHIFT == 4 * es.ACT_ERR_HSHIFT
    assert es.ACT_ERR_AFFINE / 2 <= a <= es.ACT_ERR_AFFINE * 2, a
    assert es.ACT_ERR_HSHIFT / 2 <= h <= es.ACT_ERR_HSHIFT * 2, h


# ---- mutants: every plausible wrong variant differs from the reference on some case ----------------------------------------
def killed(cases, ref, mutant) -> bool:
    return any(not es.same_bits(ref(c), mutant(c)) for c in cases)


def test_affine_mutants():
    cs = small(es.affine_cases())

    def run(c, **kw):
        ref, _ = es.ref_affine_act(*es.affine_logical(es.affine_inputs(c), c, **kw)[:3], c.act, None)
        return ref.astype(np.float32)
    assert killed(cs, run, lambda c: run(c, pitch_is_c=True))
    assert killed(cs, run, lambda c: run(c, ignore_bstride=True))
    # and per activation and per channel count, so that no single case carries the pitch
    for act in es.ACTS:
        assert killed([c for c in cs if c.act == act], run, lambda c: run(c, pitch_is_c=True)), act
    for ch in (4, 12, 64):
        assert killed([c for c in cs if c.C == ch], run, lambda c: run(c, ignore_bstride=True)), ch


def test_layout_mutants():
    s2d = [c for c in es.s2d_cases() if c.op == "s2d"]
    d2s = [c for c in es.s2d_cases() if c.op == "d2s"]
    x = lambda c: es.s2d_inputs(c)["x"][0].numpy()                       # noqa: E731
    for cases, fn in ((s2d, es.ref_s2d), (d2s, es.ref_d2s)):
        for c in cases:                                                  # (each case kills both: the data is random)
            assert killed([c], lambda c: fn(x(c)), lambda c: fn(x(c), swap_ij=True))
            assert killed([c], lambda c: fn(x(c)), lambda c: fn(x(c), crd=True))
    up = small(es.upsample_cases())
    lo = lambda c: [v[0].numpy() for v in es.upsample_inputs(c).values()]  # noqa: E731
    assert killed(up, lambda c: es.ref_upsample2_add(*lo(c)), lambda c: es.ref_upsample2_add(*lo(c), wrong_row=True))
    pool = small(es.pool_cases())
    px = lambda c: es.pool_inputs(c)["x"][0].numpy()                     # noqa: E731
    assert killed(pool, lambda c: es.ref_maxpool2(px(c)), lambda c: es.ref_maxpool2(px(c), drop_nan=True))
    assert not killed([c for c in pool if c.kind != "nan"], lambda c: es.ref_maxpool2(px(c)), lambda c: es.ref_maxpool2(px(c), drop_nan=True))
    cp = [c for c in es.copy_cases() if c.dst == "nhwc"]
    buf = lambda c, **kw: es.ref_copy4d_buffer(es.copy_inputs(c).numpy(), c.pitch, c.c_off, c.fill, **kw)    # noqa: E731
    for route in ("transpose", "generic"):
        assert killed([c for c in cp if es.copy_route_of(c) == route], buf, lambda c: buf(c, fill_to_pitch=True)), route


def test_hshift_mutants():
    cs = es.hshift_cases()

    def run(c, mutant=None):
        (tv, _), bias = es.hshift_inputs(c)
        return es.ref_hshift_sum(nhwc(tv), bias, c.kw, c.pad, c.pm, c.cout, mutant)
    for route in ("lds", "direct"):
        mine = [c for c in cs if es.hshift_route_of(c) == route and c.pad > 0]
        assert killed([c for c in mine if c.pm == es.PAD_REFLECT], run, lambda c: run(c, "reflect")), route
    lds = [c for c in cs if es.hshift_route_of(c) == "lds" and c.pad > 0]
    for pm in (es.PAD_ZERO, es.PAD_REFLECT):
        for w in (257, 300, 513):
            assert killed([c for c in lds if c.pm == pm and c.W == w], run, lambda c: run(c, "seam")), (pm, w)
    assert not killed([c for c in cs if c.W <= 256], run, lambda c: run(c, "seam"))


def test_argmax_and_u8_mutants():
    am = es.argmax_cases()
    ax = lambda c: es.argmax_input(c).numpy()                            # noqa: E731
    for lay in ("nchw", "nhwc"):
        mine = [c for c in am if c.lay == lay and c.H * c.W > 1]
        for c in mine:
            assert killed([c], lambda c: es.ref_argmax_hw(ax(c)), lambda c: es.ref_argmax_hw(ax(c), last=True)), c
    ux = lambda c: es.u8_input(c).numpy()                                # noqa: E731
    for c in es.u8_cases():
        assert killed([c], lambda c: es.ref_to_image_u8(ux(c)), lambda c: es.ref_to_image_u8(ux(c), nearest=True)), c
    mx = lambda c: [t.numpy() for t in es.merge_inputs(c)]               # noqa: E731
    for c in es.merge_cases():
        assert killed([c], lambda c: es.ref_merge_u8(*mx(c)), lambda c: es.ref_merge_u8(*mx(c), fused=True)), c
