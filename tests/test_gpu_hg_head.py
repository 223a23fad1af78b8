"""fusg_hg_head on the MI355X: the 1x1 head that ends a stack of the hourglass - y = relu(fc(y_in)), score = score32(y),
x' = x + join(cat[y, score]) - as one launch, against the three fusg_conv2d launches it replaces, bit for bit, in both forms
(with the join, and the last stack's, which stops after score): on 16 x 16 (the smallest map the hourglass produces), 16 x 48
and 32 x 16 (non-square both ways, several 64-pixel tiles), on views with a padded channel pitch and a batch stride; the zero
padding of the score map, range status and NaN propagation; the predicate; then HourglassNet with ops.HG_HEAD on against off,
eager and as a recorded pass.

Weights are seeded and packed as the network packs them: fold_bn_after_conv for fc, the score filter zero-padded to 32 output
channels, the join with c_split = (256, 12) and cin_pad = 32.

Summation order.  A 1x1 launch has one summation order on the halo kernel (no K split over the waves), so every unfused launch
only has to report the halo family.  At B = 2 the router gives these small grids generic split-K launches (another order), so
the unfused launches are issued with ksplit = 1, which keeps them on the halo kernel, and the network is also run under a
routing batch of 32 (ops.route_batch), the benchmark's: there both heads fuse."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import load_schema                                            # noqa: E402
from future_urban_scene_generation_amd import _lib as L                    # noqa: E402
from future_urban_scene_generation_amd import ops, pack                    # noqa: E402
from future_urban_scene_generation_amd.stacked_hourglass.models import HourglassNet   # noqa: E402
from future_urban_scene_generation_amd.synth import synth_inputs, synth_state_dict   # noqa: E402

DEV = "cuda:0"
HALO, HG_HEAD = 2, 14                        # ops.last_conv_kernel() families
C, NC = 256, 12
SHAPES = ((16, 16), (16, 48), (32, 16))
_CACHE = {}


def _plans(fc_gain=1.0):
    """(fc 256 -> 256 with its BatchNorm folded, score32, score 256 -> 12, join 268 -> 256) with seeded weights, packed once."""
    key = ("plans", fc_gain)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(2024)
        rn = lambda *s: torch.randn(*s, generator=g)                        # noqa: E731
        w_fc, b_fc = rn(C, C, 1, 1) / C ** 0.5 * fc_gain, rn(C) * 0.1
        scale, shift = 1.0 + 0.1 * rn(C), 0.1 * rn(C)
        w_s, b_s = rn(NC, C, 1, 1) / C ** 0.5, rn(NC) * 0.1
        w_j, b_j = rn(C, C + NC, 1, 1) / (C + NC) ** 0.5, rn(C) * 0.1
        wf, bf = pack.fold_bn_after_conv(w_fc, b_fc, scale, shift)
        ws32, bs32 = torch.zeros(32, C, 1, 1), torch.zeros(32)
        ws32[:NC], bs32[:NC] = w_s, b_s
        _CACHE[key] = (pack.pack_conv(wf, bf), pack.pack_conv(ws32, bs32), pack.pack_conv(w_s, b_s),
                       pack.pack_conv(w_j, b_j, c_split=(C, NC), cin_pad=32))
    return _CACHE[key]


def _inputs(h, w, seed=0):
    g = torch.Generator().manual_seed(500 + 10 * h + w + seed)
    return torch.randn(2, C, h, w, generator=g), torch.randn(2, C, h, w, generator=g)


def _dev(t, strided):
    """NHWC-physical on the device; strided: a view with channel pitch 264, at a batch offset inside a larger buffer."""
    if not strided:
        return ops.as_nhwc(t.to(DEV))
    b, c, h, w = t.shape
    buf = torch.full((b + 1, h, w, c + 8), 3.0e4, device=DEV)               # (values the kernels must not read)
    v = buf[1:, :, :, :c].permute(0, 3, 1, 2)
    v.copy_(t)
    assert ops.is_nhwc(v) and v.stride(3) == c + 8
    return v


def _unfused(plans, y_in, x, join):
    fc, s32, s12, jn = plans
    ops.range_exceeded(DEV)

    def conv(plan, *src, **kw):
        out = ops.conv(plan, *src, ksplit=1, **kw)
        assert ops.last_conv_kernel() == HALO, ops.last_conv_kernel()
        return out

    y = conv(fc, y_in, act=L.ACT_RELU)
    if not join:
        return (conv(s12, y), None), ops.range_exceeded(DEV)
    s = torch.full((y.shape[0], y.shape[2], y.shape[3], 32), float("nan"), device=DEV).permute(0, 3, 1, 2)
    conv(s32, y, out=s)
    return (s, conv(jn, y, s[:, :NC], res0=x)), ops.range_exceeded(DEV)


def _fused(plans, y_in, x, join):
    fc, s32, s12, jn = plans
    ops.range_exceeded(DEV)
    out = ops.hg_head(fc, s32 if join else s12, y_in, jn if join else None, x if join else None)
    assert ops.last_conv_kernel() == HG_HEAD
    return out, ops.range_exceeded(DEV)


def _both(plans, yc, xc, join, strided=False):
    y_in, x = _dev(yc, strided), _dev(xc, strided)
    return _fused(plans, y_in, x, join), _unfused(plans, y_in, x, join)


def _check_equal(got, want, join, hw):
    names = ("score", "x'") if join else ("score",)
    for name, a, b in zip(names, got, want):
        assert tuple(a.shape) == (2, {"score": 32 if join else NC, "x'": C}[name]) + hw
        ndiff = int((a != b).sum())
        print(f"{name}: {ndiff} of {a.numel()} elements differ, max |diff| {float((a - b).abs().max()):.3e}")
        assert torch.equal(a, b), name


@pytest.mark.parametrize("strided", (False, True), ids=("dense", "padded_pitch"))
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("join", (True, False), ids=("join", "last"))
def test_one_launch_writes_the_bytes_of_the_unfused_launches(join, hw, strided):
    (got, hit), (want, hit_ref) = _both(_plans(), *_inputs(*hw), join, strided)
    assert not hit and not hit_ref
    _check_equal(got, want, join, hw)


def test_score_padding_channels_are_written_as_exact_zeros():
    """The launch itself writes channels 12 .. 31 on every call (a recorded pass replays addresses, not a memset): into a score
    tensor pre-filled with NaN, through the descriptor."""
    fc, s32, _, jn = _plans()
    y_in, x = (_dev(t, False) for t in _inputs(16, 48, seed=2))
    s = torch.full((2, 16, 48, 32), float("nan"), device=DEV).permute(0, 3, 1, 2)
    out = ops.nhwc_empty(2, C, 16, 48, DEV)
    d = L.HgHeadDesc()
    d.y_in, d.x, d.score, d.dst = ops.desc(y_in), ops.desc(x), ops.desc(s), ops.desc(out)
    for key, plan in (("fc", fc), ("score", s32), ("join", jn)):
        dev = plan.to(DEV).dev
        setattr(d, "wfrag_" + key, dev["wfrag"].data_ptr())
        setattr(d, "bias_" + key, dev["bias"].data_ptr())
        setattr(d, "wscale_" + key, dev["wscale"].data_ptr())
    d.status, d.join = ops.status_word(DEV).data_ptr(), 1
    import ctypes
    L.check(L.lib().fusg_hg_head(ctypes.byref(d), ops.stream_ptr()), "hg_head")
    assert not torch.isnan(s).any()
    assert torch.equal(s[:, NC:], torch.zeros_like(s[:, NC:])) and not torch.signbit(s[:, NC:]).any()
    assert float(s[:, :NC].abs().max()) > 0
    want, want_x = ops.hg_head(fc, s32, y_in, jn, x)
    assert torch.equal(s, want) and torch.equal(out, want_x)


@pytest.mark.parametrize("join", (True, False), ids=("join", "last"))
def test_range_status_is_raised_iff_the_unfused_path_raises_it(join):
    """Once by an input of 7e4, once by a large fc weight: then it is the intermediate y, which never reaches memory, that trips."""
    yc, xc = _inputs(16, 48, seed=3)
    (_, hit_small), (_, ref_small) = _both(_plans(), yc, xc, join)
    y_big = yc.clone()
    y_big[1, 7, 9, 20] = 7e4
    (_, hit_in), (_, ref_in) = _both(_plans(), y_big, xc, join)
    (_, hit_y), (_, ref_y) = _both(_plans(fc_gain=3.0e4), yc, xc, join)
    print(f"status plain / 7e4 input / large fc: fused {hit_small} / {hit_in} / {hit_y}, unfused {ref_small} / {ref_in} / {ref_y}")
    assert hit_small == ref_small and hit_in == ref_in and hit_y == ref_y
    assert not hit_small and hit_in and hit_y


@pytest.mark.parametrize("join", (True, False), ids=("join", "last"))
def test_a_nan_input_reaches_the_same_outputs(join):
    yc, xc = _inputs(16, 48, seed=4)
    yc[0, 2, 7, 15] = float("nan")
    (got, hit), (want, hit_ref) = _both(_plans(), yc, xc, join)
    assert hit == hit_ref
    for name, a, b in zip(("score", "x'"), got, want):
        if a is None:
            continue
        assert torch.equal(torch.isnan(a), torch.isnan(b)), name
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), name


def test_the_head_is_fused_only_where_the_predicate_holds():
    """ops.hg_head_ok asks the router.  Under the benchmark's routing batch the three launches on 64 x 64 are halo launches; at
    B = 2 without one the router gives the 32-column score launch (and everything on 16 x 16) a generic split-K launch, and an
    8 x 8 map goes to the small-image kernel: those stay unfused.  So do f32 and the switch off."""
    fc, s32, s12, jn = _plans()
    y64, y16, y8 = (ops.nhwc_empty(2, C, n, n, DEV) for n in (64, 16, 8))
    with ops.route_batch(32):
        assert ops.hg_head_ok(fc, s32, y64, jn, y64) and ops.hg_head_ok(fc, s12, y64)
        assert not ops.hg_head_ok(fc, s32, y64, jn, y64, precision="f32") and not ops.hg_head_ok(fc, s12, y64, precision="f32")
        assert not ops.hg_head_ok(fc, s32, y8, jn, y8) and not ops.hg_head_ok(fc, s12, y8)
        assert not ops.hg_head_ok(fc, s12, y64, jn, y64)                                         # the join reads a 32-channel score
        old = ops.HG_HEAD
        try:
            ops.HG_HEAD = False
            assert not ops.hg_head_ok(fc, s32, y64, jn, y64) and not ops.hg_head_ok(fc, s12, y64)
        finally:
            ops.HG_HEAD = old
    assert not ops.hg_head_ok(fc, s32, y64, jn, y64) and not ops.hg_head_ok(fc, s12, y16)
    assert not ops.hg_head_ok(fc, s32, y8, jn, y8) and not ops.hg_head_ok(fc, s12, y8)


def _hourglass():
    if "hg" not in _CACHE:
        hg = HourglassNet(2, 1, NC)
        hg.load_state_dict(synth_state_dict("hg", load_schema("hg"), 0))
        _CACHE["hg"] = hg.to(DEV).eval()
    return _CACHE["hg"]


@pytest.mark.parametrize("res,rb", ((64, 0), (256, 0), (256, 32)), ids=("64", "256", "256_routed_as_32"))
def test_hourglass_with_the_fused_heads_returns_the_unfused_bytes(res, rb):
    """HourglassNet at B = 2, ops.HG_HEAD on against off: both heat-maps, and the family of the last conv launch (the last
    stack's head) is the new one only where the predicate holds - at B = 2 nowhere (the router's small-grid launches), under the
    benchmark's routing batch on the 64 x 64 maps of the network's own 256 x 256 input for both heads."""
    hg = _hourglass()
    x = synth_inputs("hg", 2, res, 0)["x"].to(DEV)
    P = hg._ensure(x)
    y = ops.nhwc_empty(2, C, res // 4, res // 4, DEV)
    old = ops.HG_HEAD
    try:
        outs, fams, oks = {}, {}, {}
        for on in (False, True):
            ops.HG_HEAD = on
            with ops.route_batch(rb), torch.no_grad():
                oks[on] = (ops.hg_head_ok(P["fc"][0], P["score32"][0], y, P["join"][0], y), ops.hg_head_ok(P["fc"][1], P["score"][1], y))
                outs[on] = [t.clone() for t in hg(x)["heatmaps"]]
            fams[on] = ops.last_conv_kernel()
    finally:
        ops.HG_HEAD = old
    print(f"res {res} routing batch {rb}: predicate {oks[True]}, last conv family off / on {fams[False]} / {fams[True]}")
    assert oks[False] == (False, False) and oks[True] == ((True, True) if rb == 32 else (False, False))
    assert fams[False] != HG_HEAD and fams[True] == (HG_HEAD if oks[True][1] else fams[False]), (fams, oks)
    assert len(outs[True]) == 2 == len(outs[False])
    for i, (a, b) in enumerate(zip(outs[True], outs[False])):
        assert a.shape == (2, NC, res // 4, res // 4) == b.shape and torch.equal(a, b), i


def test_recorded_pass_with_the_fused_heads_replays_the_eager_bytes():
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline
    assert ops.HG_HEAD
    pipe = VehiclePipeline(DEV, state_dicts={"hg": _hourglass().state_dict()}, route_batch=32)
    b0, b1 = ({"hg_x": synth_inputs("hg", 2, 256, s)["x"].to(DEV)} for s in (0, 1))

    def fn(batch, vehicle_seeds=None):
        return {"hm%d" % i: h for i, h in enumerate(pipe.hg(batch["hg_x"])["heatmaps"])}

    with torch.no_grad():
        cp = pipe.compile(b0, fn=fn)
        for batch in (b0, b1):
            with ops.route_batch(32):
                want = {k: v.clone() for k, v in fn(batch).items()}
            assert ops.last_conv_kernel() == HG_HEAD
            got = cp.run(batch)
            assert set(got) == set(want) == {"hm0", "hm1"}
            for k in want:
                assert torch.equal(got[k], want[k]), k
