"""fusg_conv2d_entry_nin on the MI355X: the VUnet's few-channel entry NiN computed inside the halo staging of the 128-channel 3x3
Residual that is its only reader, against the two fusg_conv2d launches it replaces - bit for bit (every check is torch.equal) - on
one 8 x 16 patch (every border and corner in one workgroup) and on 3 x 3 patches (interior, every edge kind, batch strides), from
6 channels (pixel pitch 8) and from 3 (pitch 4); zero padding of x0, range status and NaN propagation; then the appearance
encoder with ops.VU_ENTRY_NIN on against off, eager and as a recorded pass.

Summation order.  The router gives a 128-column 3x3 halo launch of fewer than 256 patches the 32-column tile with the K split over
the waves (four partial sums over the taps w, w + 4, w + 8, added in wave order) - every small shape here; from 512 patches on (the
benchmark's grids) the 128-column tile sums the taps in order: 128 x 128 at B = 4 is the smallest such grid (B = 3, 384 patches,
gets the 64-column tile split over two waves, a form the network never launches and that therefore stays two launches).  The fused
launch follows whichever form the Residual's own launch gets; ops.entry_nin_form reports it from the same routing decision."""
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
HALO, POINTWISE, ENTRY = 2, 7, 13            # ops.last_conv_kernel() families
M_SPLIT, K_SPLIT = 1, 2                      # ops.entry_nin_form()
SHAPES = ((8, 16), (24, 48))
C = 128
_CACHE = {}


def _plans(cin, zero_nin=False):
    """(nin cin -> 128 k1, res 128 -> 128 k3) with seeded weights, packed once.  zero_nin: zero NiN weights and a bias of 3."""
    key = ("plans", cin, zero_nin)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1313 + cin)
        w_in = torch.zeros(C, cin, 1, 1) if zero_nin else torch.randn(C, cin, 1, 1, generator=g) / cin ** 0.5
        b_in = torch.full((C,), 3.0) if zero_nin else torch.randn(C, generator=g) * 0.1
        w3 = torch.randn(C, C, 3, 3, generator=g) / (3.0 * C ** 0.5)
        _CACHE[key] = (pack.pack_conv(w_in, b_in), pack.pack_conv(w3, torch.randn(C, generator=g) * 0.1, pad=1))
    return _CACHE[key]


def _input(cin, b, h, w, seed=0):
    g = torch.Generator().manual_seed(2000 + 100 * cin + 10 * h + w + seed + b)
    return torch.randn(b, cin, h, w, generator=g)


def _both(plans, uc, form):
    """(fused output, its status), (the two launches' output, their status); each arm must run on the intended kernels."""
    nin, res = plans
    u = ops.as_nhwc(uc.to(DEV))
    assert u.stride(1) == 1 and u.stride(3) == (8 if uc.shape[1] > 4 else 4)
    assert ops.entry_nin_form(nin, res, u, ksplit=1) == form
    ops.range_exceeded(DEV)
    got = ops.entry_nin(nin, res, u, ksplit=1)
    assert ops.last_conv_kernel() == ENTRY
    hit = ops.range_exceeded(DEV)
    x0 = ops.conv(nin, u, pre_op=L.PRE_ELU, ksplit=1)
    assert ops.last_conv_kernel() == POINTWISE
    want = ops.conv(res, x0, pre_op=L.PRE_ELU, res0=x0, ksplit=1)
    assert ops.last_conv_kernel() == HALO
    return (got, hit), (want, ops.range_exceeded(DEV))


def _same(a, b):
    assert a.shape == b.shape
    print(f"{int((a != b).sum())} of {a.numel()} elements differ, max |diff| {float((a - b).abs().max()):.3e}")
    assert torch.equal(a, b)


@pytest.mark.parametrize("b", (1, 3))
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cin", (6, 3))
def test_k_split_form_writes_the_bytes_of_the_two_launches(cin, hw, b):
    (got, hit), (want, hit_ref) = _both(_plans(cin), _input(cin, b, *hw), K_SPLIT)
    assert not hit and not hit_ref
    assert tuple(got.shape) == (b, C) + hw
    _same(got, want)


@pytest.mark.parametrize("cin", (6, 3))
def test_m_split_form_writes_the_bytes_of_the_two_launches(cin):
    """128 x 128: 128 patches per image.  B = 4 is the first grid the router gives the 128-column tile; B = 3 gets the 64-column
    tile over two waves, which is not built in the entry form."""
    nin, res = _plans(cin)
    u3 = ops.as_nhwc(torch.zeros(3, cin, 128, 128, device=DEV))
    assert ops.entry_nin_form(nin, res, u3, ksplit=1) == 0 and not ops.entry_nin_ok(nin, res, u3)
    (got, hit), (want, hit_ref) = _both((nin, res), _input(cin, 4, 128, 128), M_SPLIT)
    assert not hit and not hit_ref
    _same(got, want)


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_pixels_outside_the_image_are_staged_as_zero(hw):
    """Zero NiN weights and a bias of 3: x0 is 3 everywhere inside the image.  An x0 staged as NiN(0) + bias outside the image
    would reach every border output through the taps."""
    (got, hit), (want, hit_ref) = _both(_plans(6, zero_nin=True), _input(6, 1, *hw, seed=5), K_SPLIT)
    assert not hit and not hit_ref
    _same(got, want)
    assert float((got[:, :, 0, :] - got[:, :, hw[0] // 2, :]).abs().max()) > 0      # the border does differ from the interior


def test_range_status_is_raised_in_both_arms():
    u = _input(6, 1, 24, 48, seed=3)
    (_, hit_small), (_, ref_small) = _both(_plans(6), u, K_SPLIT)
    u[0, 1, 9, 20] = 1e6                                   # elu(u) = u: |x0| = |w| 1e6 >= 2^15 in nearly every channel of that pixel
    (got, hit), (want, hit_ref) = _both(_plans(6), u, K_SPLIT)
    print(f"status without / with the 1e6 input: fused {hit_small} / {hit}, two launches {ref_small} / {hit_ref}")
    assert not hit_small and not ref_small
    assert hit and hit_ref
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))


def test_a_nan_input_reaches_the_same_outputs():
    u = _input(6, 3, 24, 48, seed=4)
    u[1, 2, 7, 15] = float("nan")                          # a patch corner: its 3 x 3 neighbourhood spans four patches
    (got, _), (want, _) = _both(_plans(6), u, K_SPLIT)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert int(torch.isnan(got).sum()) > 0
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))


def test_the_pair_is_fused_only_where_the_predicate_allows():
    nin, res = _plans(6)
    u = ops.as_nhwc(torch.zeros(4, 6, 128, 128, device=DEV))
    assert ops.entry_nin_ok(nin, res, u)
    assert not ops.entry_nin_ok(nin, res, u, precision="f32") and not ops.entry_nin_ok(nin, res, u, precision="bf16")
    assert not ops.entry_nin_ok(nin, res, ops.as_nhwc(torch.zeros(4, 6, 124, 128, device=DEV)))       # no 8 x 16 patches
    nin32 = pack.pack_conv(torch.zeros(32, 6, 1, 1), torch.zeros(32))
    res32 = pack.pack_conv(torch.zeros(32, 32, 3, 3), torch.zeros(32), pad=1)
    assert not ops.entry_nin_ok(nin32, res32, u)                                                        # 128 channels is what is built
    old = ops.VU_ENTRY_NIN
    try:
        ops.VU_ENTRY_NIN = False
        assert not ops.entry_nin_ok(nin, res, u)
    finally:
        ops.VU_ENTRY_NIN = old


def _vunet():
    if "vunet" not in _CACHE:
        vu = Vunet_fix_res(Namespace(up_mode="subpixel", w_norm=True, drop_prob=0.2, vunet_256=True))
        vu.load_state_dict(synth_state_dict("vunet", load_schema("vunet"), 0))
        _CACHE["vunet"] = vu.to(DEV).eval()
    return _CACHE["vunet"]


def test_appearance_encoder_with_the_fused_entry_returns_the_unfused_bytes():
    """forward_enc_up at B = 1, 256 x 256 (512 patches: the M-split form), ops.VU_ENTRY_NIN on against off: every returned tensor,
    and the InitBlock's own outputs."""
    vu = _vunet()
    x = synth_inputs("vunet", 1, 256, 0)["x"].to(DEV)
    old = ops.VU_ENTRY_NIN
    try:
        outs, fams = {}, {}
        for on in (False, True):
            ops.VU_ENTRY_NIN = on
            o, s = vu.forward_enc_up(x)
            outs[on] = [t.clone() for t in list(o) + list(s)]
            u = ops.as_nhwc(x)
            xb, sl = vu._init_block("app_encoder_1", u)
            outs[on] += [xb.clone()] + [t.clone() for t in sl]
            nin, res = vu._plans["app_encoder_1.nin.layers.1"], vu._plans["app_encoder_1.residual_0.layers.2"]
            fams[on] = ops.entry_nin_ok(nin, res, u), ops.entry_nin_form(nin, res, u)
    finally:
        ops.VU_ENTRY_NIN = old
    assert fams[False] == (False, M_SPLIT) and fams[True] == (True, M_SPLIT), fams
    assert len(outs[True]) == 7 == len(outs[False])
    for i, (a, b) in enumerate(zip(outs[True], outs[False])):
        assert a.shape == b.shape and torch.equal(a, b), i


def test_recorded_pass_with_the_fused_entry_replays_the_eager_bytes():
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline
    assert ops.VU_ENTRY_NIN
    pipe = VehiclePipeline(DEV, state_dicts={"vunet": _vunet().state_dict()})
    assert pipe.vunet.vunet_256
    i0, i1 = synth_inputs("vunet", 1, 256, 0), synth_inputs("vunet", 1, 256, 1)
    b0, b1 = ({"vu_y": i["y_tilde"].to(DEV), "vu_x": i["x"].to(DEV)} for i in (i0, i1))
    cp = pipe.compile(b0, vehicle_seeds=[7], fn=pipe._vunet_forward)
    for batch, seeds in ((b0, [7]), (b1, [9])):
        want = {k: v.clone() for k, v in pipe.vunet_forward(batch, vehicle_seeds=seeds).items()}
        got = cp.run(batch, vehicle_seeds=seeds)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k
