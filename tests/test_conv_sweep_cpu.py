"""CPU: the routing sweep's own machinery (tests/conv_sweep.py) - its cases are reproducible and legal, the edge table's recorded
families are what the restated router predicts, and the one comparator is tight enough to reject subtly wrong results."""
from collections import Counter

import pytest
import torch

import conv_sweep as cs


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
