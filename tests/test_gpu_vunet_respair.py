"""fusg_vunet_respair on the MI355X: two 32-channel Residuals and their two skip NiNs (entry form: plus the few-channel NiN in
front) as one launch, against the five (four) fusg_conv2d launches it replaces - bit for bit - on one 8 x 16 patch (every
border and corner in one workgroup) and on 3 x 3 patches (interior, every edge kind, batch strides); zero padding of the
intermediates, range status and NaN propagation; then the VUnet's shape encoder with ops.VU_RESPAIR on against off, eager
and as a recorded pass.

Summation order.  The router gives a 32-column 3x3 halo launch of at most 1024 patches the K split over the waves (four
partial sums over the taps w, w + 4, w + 8, added in wave order); larger grids - the benchmark's - sum the taps in order.
The fused launch follows whichever the unfused launches get (tap_order 0).  Every shape here is a small grid, so the
in-order form (tap_order 1) is compared with launches that are given the list of all patches (`tiles`), which keeps the
halo kernel off the K split."""
from argparse import Namespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import load_schema                                            # noqa: E402
from future_urban_scene_generation_amd import _lib as L                    # noqa: E402
from future_urban_scene_generation_amd import ops, pack                    # noqa: E402
from future_urban_scene_generation_amd.synth import synth_inputs, synth_state_dict   # noqa: E402
from future_urban_scene_generation_amd.vunet.models import Vunet_fix_res   # noqa: E402

DEV = "cuda:0"
HALO, POINTWISE, RESPAIR = 2, 7, 12          # ops.last_conv_kernel() families
SHAPES = ((8, 16), (24, 48))
_CACHE = {}


def _plans(zero_3x3=False):
    """(nin_in 3 -> 32, res_a, res_b 32 -> 32 k3, nin_b, nin_c 32 -> 32 k1) with seeded weights, packed once."""
    key = ("plans", zero_3x3)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(4242)
        w_in = torch.randn(32, 3, 1, 1, generator=g) / 3 ** 0.5
        w3 = [torch.zeros(32, 32, 3, 3) if zero_3x3 else torch.randn(32, 32, 3, 3, generator=g) / (3.0 * 32 ** 0.5) for _ in range(2)]
        w1 = [torch.randn(32, 32, 1, 1, generator=g) / 32 ** 0.5 for _ in range(2)]
        b = [torch.randn(32, generator=g) * 0.1 for _ in range(5)]
        _CACHE[key] = (pack.pack_conv(w_in, b[0]), pack.pack_conv(w3[0], b[1], pad=1), pack.pack_conv(w3[1], b[2], pad=1),
                       pack.pack_conv(w1[0], b[3]), pack.pack_conv(w1[1], b[4]))
    return _CACHE[key]


def _input(entry, h, w, seed=0):
    g = torch.Generator().manual_seed(1000 + 10 * h + w + seed + (1 if entry else 0))
    return torch.randn(2, 3 if entry else 32, h, w, generator=g)


def _unfused(plans, x, entry, in_order):
    """(s1, kb, kc), range status, of the block as its fusg_conv2d launches; each launch must run on the family whose
    summation order the fused kernel follows."""
    nin_in, res_a, res_b, nin_b, nin_c = plans
    _, _, h, w = x.shape
    tiles = torch.arange((h // 8) * (w // 16), dtype=torch.int32, device=x.device) if in_order else None
    ops.range_exceeded(DEV)

    def conv(plan, src, fam, **kw):
        out = ops.conv(plan, src, pre_op=L.PRE_ELU, ksplit=1, **kw)
        assert ops.last_conv_kernel() == fam, (ops.last_conv_kernel(), fam)
        return out

    x0 = conv(nin_in, x, POINTWISE) if entry else x
    s0 = conv(res_a, x0, HALO, res0=x0, tiles=tiles)
    s1 = conv(res_b, s0, HALO, res0=s0, tiles=tiles)
    kb = conv(nin_b, s0, HALO)
    kc = conv(nin_c, s1, HALO)
    return (s1, kb, kc), ops.range_exceeded(DEV)


def _fused(plans, x, entry, in_order):
    nin_in, res_a, res_b, nin_b, nin_c = plans
    ops.range_exceeded(DEV)
    out = ops.respair(res_a, res_b, nin_b, nin_c, x, nin_in=nin_in if entry else None, tap_order=1 if in_order else 0)
    assert ops.last_conv_kernel() == RESPAIR
    return out, ops.range_exceeded(DEV)


def _both(plans, xc, entry, in_order):
    x = ops.as_nhwc(xc.to(DEV))
    return _fused(plans, x, entry, in_order), _unfused(plans, x, entry, in_order)


@pytest.mark.parametrize("in_order", (False, True), ids=("as_routed", "taps_in_order"))
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("entry", (True, False), ids=("entry", "plain"))
def test_one_launch_writes_the_bytes_of_the_unfused_launches(entry, hw, in_order):
    (got, hit), (want, hit_ref) = _both(_plans(), _input(entry, *hw), entry, in_order)
    assert not hit and not hit_ref
    for name, a, b in zip(("s1", "kb", "kc"), got, want):
        assert tuple(a.shape) == (2, 32) + hw
        ndiff = int((a != b).sum())
        print(f"{name}: {ndiff} of {a.numel()} elements differ, max |diff| {float((a - b).abs().max()):.3e}")
        assert torch.equal(a, b), name


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_intermediates_outside_the_image_are_zero_padding(hw):
    """Zero 3x3 weights, non-zero NiN bias: x0 = NiN(elu(u)) + b and s0 = bA + x0 inside the image, and nothing else."""
    (got, hit), (want, hit_ref) = _both(_plans(zero_3x3=True), _input(True, *hw, seed=5), True, False)
    assert not hit and not hit_ref
    for name, a, b in zip(("s1", "kb", "kc"), got, want):
        assert torch.equal(a, b), name


def test_intermediates_outside_the_image_do_not_reach_the_taps():
    """The same with live 3x3 weights and a large NiN bias: an x0 or s0 computed as NiN(0) + bias outside the image would
    reach every border pixel through the taps."""
    g = torch.Generator().manual_seed(77)
    base = _plans()
    nin_in = pack.pack_conv(torch.randn(32, 3, 1, 1, generator=g), torch.full((32,), 3.0))
    (got, hit), (want, hit_ref) = _both((nin_in,) + base[1:], _input(True, 8, 16, seed=9), True, False)
    assert not hit and not hit_ref
    for name, a, b in zip(("s1", "kb", "kc"), got, want):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("entry", (True, False), ids=("entry", "plain"))
def test_range_status_is_raised_iff_the_unfused_path_raises_it(entry):
    x = _input(entry, 24, 48, seed=3)
    (_, hit_small), (_, ref_small) = _both(_plans(), x, entry, False)
    x[1, 1, 9, 20] = 7e4
    (_, hit), (_, hit_ref) = _both(_plans(), x, entry, False)
    print(f"status without / with the 7e4 input: fused {hit_small} / {hit}, unfused {ref_small} / {hit_ref}")
    assert hit_small == ref_small and hit == hit_ref
    assert not hit_small


@pytest.mark.parametrize("entry", (True, False), ids=("entry", "plain"))
def test_a_nan_input_reaches_the_same_outputs(entry):
    x = _input(entry, 24, 48, seed=4)
    x[0, 2, 7, 15] = float("nan")                          # a patch corner: its 5 x 5 neighbourhood spans four patches
    (got, _), (want, _) = _both(_plans(), x, entry, False)
    for name, a, b in zip(("s1", "kb", "kc"), got, want):
        assert torch.equal(torch.isnan(a), torch.isnan(b)), name
        assert int(torch.isnan(a).sum()) > 0, name
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), name


def _vunet():
    if "vunet" not in _CACHE:
        vu = Vunet_fix_res(Namespace(up_mode="subpixel", w_norm=True, drop_prob=0.2, vunet_256=True))
        vu.load_state_dict(synth_state_dict("vunet", load_schema("vunet"), 0))
        _CACHE["vunet"] = vu.to(DEV).eval()
    return _CACHE["vunet"]


def test_the_block_is_fused_only_where_the_unfused_launches_run_on_the_halo_kernel():
    """ops.respair_ok asks the router: at B = 2 a 3x3 launch on 64 x 64 is a generic split-K launch (another summation order),
    so that level stays unfused; 128 x 128 is a halo launch."""
    nin_in, res_a, res_b, nin_b, nin_c = _plans()
    for h, want in ((64, False), (128, True)):
        x = ops.nhwc_empty(2, 32, h, h, DEV)
        assert ops.respair_ok(res_a, res_b, nin_b, nin_c, x) == want, h
        u = ops.as_nhwc(torch.zeros(2, 3, h, h, device=DEV))
        assert ops.respair_ok(res_a, res_b, nin_b, nin_c, u, nin_in=nin_in) == want, h
    x = ops.nhwc_empty(2, 32, 128, 128, DEV)
    assert not ops.respair_ok(res_a, res_b, nin_b, nin_c, x, precision="f32")
    assert not ops.respair_ok(res_a, res_b, nin_b, nin_c, ops.nhwc_empty(2, 32, 124, 128, DEV))


@pytest.mark.parametrize("res", (256, 64))
def test_shape_encoder_with_the_fused_blocks_returns_the_unfused_bytes(res):
    """forward_dec_up at B = 2, ops.VU_RESPAIR on against off: x and all 14 skips.  256 x 256, the network's own input: both
    32-channel levels (256 x 256 and 128 x 128) run fused.  64 x 64, the smallest input the six down-samplings allow: fusg_conv2d
    gives such small grids generic split-K launches, whose summation order is not the halo kernel's, so nothing is fused there
    (ops.respair_ok) and the switch changes nothing."""
    vu = _vunet()
    y = synth_inputs("vunet", 2, res, 0)["y_tilde"].to(DEV)
    old = ops.VU_RESPAIR
    try:
        outs, fams = {}, {}
        for on in (False, True):
            ops.VU_RESPAIR = on
            xs, skips = vu.forward_dec_up(y)
            outs[on] = [t.clone() for t in list(xs) + list(skips)]
            vu._init_block_skips("shape_encoder_1", "shape_skip_1", ops.as_nhwc(y))
            fams[on] = [ops.last_conv_kernel()]
            vu._down_block_skips("shape_encoder_1_a", "shape_skip_1_a", ops.nhwc_empty(2, 32, res, res, DEV, zero=True))
            fams[on].append(ops.last_conv_kernel())
    finally:
        ops.VU_RESPAIR = old
    assert fams[False] == [HALO, HALO], fams
    assert fams[True] == ([RESPAIR, RESPAIR] if res == 256 else [HALO, HALO]), fams
    assert len(outs[True]) == 15 == len(outs[False])
    for i, (a, b) in enumerate(zip(outs[True], outs[False])):
        assert a.shape == b.shape and torch.equal(a, b), i


def test_recorded_pass_with_the_fused_blocks_replays_the_eager_bytes():
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline
    assert ops.VU_RESPAIR
    pipe = VehiclePipeline(DEV, state_dicts={"vunet": _vunet().state_dict()})
    assert pipe.vunet.vunet_256
    i0, i1 = synth_inputs("vunet", 2, 256, 0), synth_inputs("vunet", 2, 256, 1)
    b0, b1 = ({"vu_y": i["y_tilde"].to(DEV), "vu_x": i["x"].to(DEV)} for i in (i0, i1))
    cp = pipe.compile(b0, vehicle_seeds=[7, 8], fn=pipe._vunet_forward)
    for batch, seeds in ((b0, [7, 8]), (b1, [9, 10])):
        want = {k: v.clone() for k, v in pipe.vunet_forward(batch, vehicle_seeds=seeds).items()}
        got = cp.run(batch, vehicle_seeds=seeds)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k
