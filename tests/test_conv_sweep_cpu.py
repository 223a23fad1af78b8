"""CPU: the routing sweep's own machinery (tests/conv_sweep.py) - its cases are reproducible and legal, the edge table's recorded
families are what the restated router predicts, the library's router (fusg_conv2d_route, a dry run) agrees with that
restatement, and the one comparator is tight enough to reject subtly wrong results."""
import ctypes as C
import os
from collections import Counter
from contextlib import contextmanager

import pytest
import torch

import conv_sweep as cs
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import ops


def test_random_draw_is_deterministic():
    a, b = cs.random_cases(), cs.random_cases()
    assert a == b and len(a) >= 200
    assert cs.random_cases(seed=7) != a
    assert len({c.tag for c in cs.all_cases()}) == len(cs.all_cases())


@pytest.mark.parametrize("c", cs.all_cases(), ids=lambda c: c.tag)
def test_case_is_valid_for_torch(c):
    cs.validate(c)
    inp = cs.inputs(c)
    ref, den = cs.reference(c, inp)
    ho, wo = c.full_hw()
    assert tuple(ref.shape) == (c.B, c.cout, ho, wo)
    assert torch.isfinite(ref).all() and (den > 0).all()
    assert c.mflop() <= 60.0, c.mflop()
    # the comparator passes the reference's own float32 rounding, far below the bar
    assert cs.norm_err(ref.float(), ref, den) <= cs.BAR_FP32 / 8


def test_edge_table_records_what_the_router_picks():
    """Each edge row's (f32, f16x3, bf16) families equal the restated router's, and the table reaches all eleven families."""
    seen = Counter()
    for c in cs.edge_cases():
        assert c.expect is not None, c.tag
        pred = tuple(cs.predict_family(c, p) for p in cs.PRECISIONS)
        assert pred == c.expect, (c.tag, pred, c.expect)
        seen.update(pred)
    assert set(seen) == set(cs.FAMILIES), sorted(seen)


def test_every_off_switch_leads_elsewhere():
    for c in cs.all_cases():
        for p in cs.PRECISIONS:
            fam = cs.predict_family(c, p)
            sw = cs.off_switch(fam, c)
            if sw is None:
                continue
            env, ks = sw
            assert cs.predict_family(c, p, env=env, ksplit=ks) != fam, (c.tag, p, fam)


PER_CALL = ("FUSG_NO_SMALL", "FUSG_NO_POINTWISE", "FUSG_NO_F32_HALO", "FUSG_NO_BF16_TAPUNIT", "FUSG_SMALL_KSPLIT")


@contextmanager
def _env(env):
    """Exactly the per-call switches of `env` set (the library and ops.conv read them per call)."""
    old = {k: os.environ.pop(k, None) for k in PER_CALL}
    os.environ.update(env or {})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _nhwc(b, c, h, w, cpad=4):
    """A CPU tensor laid out like ops.as_nhwc's: channels padded to a multiple of cpad, logical [b, c, h, w]."""
    cp = (c + cpad - 1) // cpad * cpad
    full = torch.zeros(b, h, w, cp).permute(0, 3, 1, 2)
    return full if cp == c else full[:, :c]


def _route(c, plan, prec, env=None, ksplit=None):
    """The library's family for the case's ops.conv launch (tests/test_gpu_conv_sweep.py, _launch), on CPU tensors: the
    descriptor ops.conv builds, planned by fusg_conv2d_plan, routed by fusg_conv2d_route."""
    ho, wo = c.full_hw()
    x0 = _nhwc(c.B, c.c0, c.H, c.W, c.cin_pad)
    x1 = _nhwc(c.B, c.c1, c.H, c.W, c.cin_pad) if c.c1 else None
    kw = dict(pre_op=cs.PRE[c.pre], act=c.act, precision=prec, ksplit=c.ksplit if ksplit is None else ksplit)
    if c.pre.startswith("affine"):
        ctot = plan.c0k + plan.c1k
        shape = (c.B, ctot) if c.per_sample else (ctot,)
        kw.update(pre=(torch.zeros(shape), torch.zeros(shape)), pre_bstride=ctot if c.per_sample else 0)
    for i in range(c.res):
        kw["res%d" % i] = _nhwc(c.B, c.cout, ho, wo)
    if c.out == "nchw":
        kw["nchw_out"] = True
    elif c.out == "slice":
        kw.update(out=ops.nhwc_empty(c.B, c.out_c_off + c.cout + 4, ho, wo, "cpu"), out_c_off=c.out_c_off)
    elif c.out == "misaligned":
        kw["out"] = torch.zeros(c.B * ho * wo * c.cout + 1)[1:].view(c.B, ho, wo, c.cout).permute(0, 3, 1, 2)
    if c.qwin:
        kw.update(out=ops.nhwc_empty(c.B, c.cout, ho, wo, "cpu"), q_window=c.qwin)
    lib = L.lib()
    with _env(env), ops.status_scope(torch.zeros(4, dtype=torch.int32)):
        d, _ = ops._conv_desc(plan, x0, x1, **kw)
        lib.fusg_conv2d_plan(C.byref(d))
        return lib.fusg_conv2d_route(C.byref(d))


def test_library_router_matches_restatement():
    """For every case and precision of the sweep, fusg_conv2d_route picks the family predict_family restates - and again with
    the off-switch of that family set (the next family in the router's order)."""
    seen = Counter()
    for c in cs.all_cases():
        plan = cs.make_plan(c, torch.zeros(c.cout, c.cin, c.kh, c.kw), torch.zeros(c.cout))
        for p in cs.PRECISIONS:
            fam = cs.predict_family(c, p)
            assert _route(c, plan, p) == fam, (c.tag, p)
            seen[fam] += 1
            sw = cs.off_switch(fam, c)
            if sw is not None:
                env, ks = sw
                assert _route(c, plan, p, env, ks) == cs.predict_family(c, p, env=env, ksplit=ks), (c.tag, p, env, ks)
    assert set(seen) == set(cs.FAMILIES), sorted(seen)


@pytest.mark.parametrize("c", cs.all_cases(), ids=lambda c: c.tag)
def test_comparator_rejects_mutations(c):
    """On every case of the sweep the comparator must reject: one tap moved, one 32-channel chunk of K dropped, the bias
    missing, one output off by 4x the bar, and (K <= 2304) operands rounded to fp16's 11 significant bits.  A mutation that
    gets through means the bar is too loose for that case.  (A tap is moved only where that changes the result at all: on a
    1 x 1 image with replicate padding every tap reads the same pixel.)"""
    inp = cs.inputs(c)
    ref, den = cs.reference(c, inp)
    names = []
    for name, mut in cs.mutations(c, inp):
        names.append(name)
        e = cs.norm_err(mut, ref, den)
        assert e > cs.BAR_FP32, (c.tag, name, e)
    assert ("fp16_hi_only" in names) == (c.K <= 2304)
    assert "k_chunk_dropped" in names and "bias_missing" in names and "one_pixel_off" in names


def test_bf16_bar_is_what_two_bf16_roundings_can_reach():
    """The bf16 families' bar is the worst case of one product of two operands rounded to bf16 (8 significant bits, ties to
    even): 2^-7 + 2^-16.  The bf16-operand emulation of the sweep's own cases stays within it and (few-term sums, where one
    product dominates) exceeds 2^-8 - a bar of 2^-8 would fail a correct kernel."""
    worst = 0.0
    for c in cs.all_cases():
        rb = cs.reference_bf16(c, cs.inputs(c))
        if rb is None:
            continue
        ref, den = cs.reference(c, cs.inputs(c))
        e = cs.norm_err(rb[0], ref, den)
        assert e <= cs.BAR_BF16, (c.tag, e)
        worst = max(worst, e)
    assert 2.0 ** -8 < worst <= cs.BAR_BF16, worst
    x = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -20], dtype=torch.float32)     # just above a tie: rounds up by ~2^-8 relative
    assert float(x.bfloat16().double() / x.double() - 1) > 2.0 ** -8 * 0.99
