"""VUnet UpSample modes 'nearest' and 'conv2d_t' on the MI355X: the one-launch dense-equivalent form (pack.py) against the
float64 torch op with the conv sweep's comparator and bar, the tap-sparse halo instantiations against the dense launch
(byte for byte), their routing, the two reference fixtures, a recorded pass, and a guard on UpSample('subpixel').  Under the
single-pass modes ("bf16", "f16") the router runs the dense kernel on the tap-sparse weights: those launches are held to the
operand-rounded reference of the dense-equivalent weights."""
import ctypes as C
import json
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import conv_sweep as cs                                                    # noqa: E402
from conftest import load_golden, record                                   # noqa: E402
from future_urban_scene_generation_amd import _lib as L                    # noqa: E402
from future_urban_scene_generation_amd import ops, pack                    # noqa: E402
from future_urban_scene_generation_amd.synth import synth_inputs, synth_state_dict   # noqa: E402
from future_urban_scene_generation_amd.vunet.layers import UpSample        # noqa: E402
from future_urban_scene_generation_amd.vunet.models import Vunet_fix_res   # noqa: E402

DEV = "cuda:0"
TOL_VU = 2e-5            # tests/test_gpu_nets.py's bar on raw VUnet outputs (vunet_b2_r128.npz), relative to the largest magnitude
MODES = ("nearest", "conv2d_t")
PRECS = ("f16x3", "f32")
# (c_in, c_out, H, W): the smallest grid the halo kernel takes; 4 c_out = 128 columns = all four phases; off the halo route
SHAPES = {"halo_128": (128, 128, 8, 16), "four_phase": (64, 32, 16, 16), "generic": (32, 32, 5, 7)}
HALO_FAMILY = {"f16x3": cs.HALO, "f32": cs.HALO_F32}
GENERIC_FAMILY = {"f16x3": cs.GEN_F16X3, "f32": cs.GEN_F32}
SINGLE_PASS = {"bf16": (cs.HALO_BF16, cs.BAR_BF16), "f16": (L.CONV_HALO_F16, (1 + 2.0 ** -11) ** 2 - 1)}   # family, operand-rounding bound
_CACHE = {}


def _layer_all(mode, shape):
    """(plan, x [2, c_in, H, W], float64 reference, comparator's denominator, weight, bias) of one layer, computed once."""
    key = (mode, shape)
    if key not in _CACHE:
        cin, cout, h, w = SHAPES[shape]
        g = torch.Generator().manual_seed(100 + 7 * MODES.index(mode) + list(SHAPES).index(shape))
        x = torch.randn(2, cin, h, w, generator=g)
        wt = torch.randn((cout, cin, 3, 3) if mode == "nearest" else (cin, cout, 3, 3), generator=g) / (3.0 * cin ** 0.5)
        b = torch.randn(cout, generator=g) * 0.1
        if mode == "nearest":
            plan = pack.pack_conv_up2_nearest_d2s(wt, b)
            op = lambda xx, ww, bb: F.conv2d(F.interpolate(xx, scale_factor=2, mode="nearest"), ww, bb, padding=1)   # noqa: E731
        else:
            plan = pack.pack_conv_transpose_k3s2p1op1_d2s(wt, b)
            op = lambda xx, ww, bb: F.conv_transpose2d(xx, ww, bb, stride=2, padding=1, output_padding=1)            # noqa: E731
        ref = op(x.double(), wt.double(), b.double())
        den = op(x.double().abs(), wt.double().abs(), b.double().abs())
        _CACHE[key] = (plan, x, ref, den, wt, b)
    return _CACHE[key]


def _layer(mode, shape):
    return _layer_all(mode, shape)[:4]


def _launch(plan, x, prec, tap_sparse=None):
    tap_sparse = plan.tap_sparse if tap_sparse is None else tap_sparse      # (the pattern itself: ops.TAP_SPARSE_LAUNCH is off by default)
    out = ops.conv(plan, ops.as_nhwc(x.to(DEV)), store=L.STORE_D2S, precision=prec, ksplit=1, tap_sparse=tap_sparse)
    return out, ops.last_conv_kernel()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", MODES)
def test_layer_against_float64(mode, shape, prec):
    plan, x, ref, den = _layer(mode, shape)
    assert plan.tap_sparse == {"nearest": 1, "conv2d_t": 2}[mode]
    got, fam = _launch(plan, x, prec)
    assert not ops.range_exceeded(DEV)
    assert fam == (GENERIC_FAMILY if shape == "generic" else HALO_FAMILY)[prec]
    err = cs.norm_err(got, ref, den)
    record(f"{mode}_{shape}_{prec}_norm_err", err)
    print(f"{mode} {shape} {prec}: family {fam} norm_err {err:.3e} (bar {cs.bar(fam):.3e})")
    assert tuple(got.shape) == tuple(ref.shape) and err <= cs.bar(fam)


@pytest.mark.parametrize("prec", list(SINGLE_PASS))
@pytest.mark.parametrize("shape", ["halo_128", "four_phase"])
@pytest.mark.parametrize("mode", MODES)
def test_layer_single_pass_against_the_operand_rounded_reference(mode, shape, prec):
    """Under "bf16" / "f16" the halo shapes take family 5 / 15: the DENSE kernel, with a DepthToSpace store, on the tap-sparse
    weights.  Held to that arithmetic - activations and the dense-equivalent weights rounded as the mode rounds them, exact
    products and sums - at BAR_FP32, and to the float64 torch op at the mode's operand-rounding bound; the launch with the
    pattern set is the launch with pattern 0, bit for bit."""
    plan, x, ref, den, wt, b = _layer_all(mode, shape)
    wd = (pack.up2_nearest_dense_weight if mode == "nearest" else pack.transpose_k3s2p1op1_dense_weight)(wt.float())
    if prec == "bf16":
        xr, wr = x.bfloat16().double(), wd.bfloat16().double()
    else:
        xr, wr = x.half().double(), pack.f16_mode_weights(wd.reshape(1, wd.shape[0], -1)).reshape(wd.shape).double()
    b4 = b.repeat(4).double()
    own = cs.d2s(F.conv2d(xr, wr, b4, padding=1))
    own_den = cs.d2s(F.conv2d(xr.abs(), wr.abs(), b4.abs(), padding=1))
    family, bound = SINGLE_PASS[prec]
    got, fam = _launch(plan, x, prec)
    dense, fd = _launch(plan, x, prec, tap_sparse=0)
    assert not ops.range_exceeded(DEV)
    assert fam == fd == family, (fam, fd)
    assert torch.equal(got, dense)
    e_own, e_exact = cs.norm_err(got, own, own_den), cs.norm_err(got, ref, den)
    record(f"{mode}_{shape}_{prec}_operands_err", e_own)
    record(f"{mode}_{shape}_{prec}_norm_err", e_exact)
    print(f"{mode} {shape} {prec}: family {fam}, {e_own:.3e} from its own arithmetic (bar {cs.BAR_FP32:.3e}), {e_exact:.3e} from float64")
    assert tuple(got.shape) == tuple(ref.shape) and e_own <= cs.BAR_FP32 and e_exact <= bound
    assert cs.norm_err(own, ref, den) > 10 * cs.BAR_FP32       # (and that reference does tell the mode from f16x3)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", ["halo_128", "four_phase"])
@pytest.mark.parametrize("mode", MODES)
def test_sparse_launch_equals_dense_launch_bytes(mode, shape, prec):
    """The skipped products are exact zeros: pattern set == pattern 0 on the same packed weights, bit for bit.  Also on an
    input that raises the split's range status (where callers redo the launch in exact fp32: the f32 rows)."""
    plan, x, _, _ = _layer(mode, shape)
    big = x.clone()
    big[1, 3, 2, 5] = 7e4                                              # outside the fp16 split's range
    for tag, xin in (("finite", x), ("range", big)):
        dense, fd = _launch(plan, xin, prec, tap_sparse=0)
        hit_d = ops.range_exceeded(DEV)
        sparse, fs = _launch(plan, xin, prec)
        hit_s = ops.range_exceeded(DEV)
        assert fd == fs == HALO_FAMILY[prec]
        assert hit_d == hit_s == (tag == "range" and prec == "f16x3"), (tag, hit_d, hit_s)
        if tag == "range" and prec == "f16x3":
            continue                                                   # (the result of a flagged launch is discarded)
        assert torch.isfinite(dense).all() and torch.equal(dense, sparse), (tag, float((dense - sparse).abs().max()))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mode", MODES)
def test_router_reports_the_family(mode, prec):
    for shape in SHAPES:
        plan, x, _, _ = _layer(mode, shape)
        d, _ = ops._conv_desc(plan, ops.as_nhwc(x.to(DEV)), store=L.STORE_D2S, precision=prec, ksplit=1,
                              tap_sparse=plan.tap_sparse)
        L.lib().fusg_conv2d_plan(C.byref(d))
        assert d.tap_sparse == plan.tap_sparse != 0
        assert L.lib().fusg_conv2d_route(C.byref(d)) == (GENERIC_FAMILY if shape == "generic" else HALO_FAMILY)[prec], shape


CONFIG = {"nearest": dict(up_mode="nearest", w_norm=False, drop_prob=0.0, vunet_256=False),
          "conv2d_t": dict(up_mode="conv2d_t", w_norm=True, drop_prob=0.0, vunet_256=False)}


def _net(mode):
    key = ("net", mode)
    if key not in _CACHE:
        g = load_golden(f"vunet_up_{mode}_b2_r128")
        schema = {k: (tuple(s), "float32") for k, s in json.loads(str(g["schema"]))}
        vu = Vunet_fix_res(Namespace(**CONFIG[mode]))
        vu.load_state_dict(synth_state_dict("vunet", schema, int(g["seed"])))
        _CACHE[key] = (vu.to(DEV).eval(), g)
    return _CACHE[key]


def _rel(got, ref, what):
    got, ref = got.detach().to("cpu").double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    r = float((got - ref).abs().max() / (ref.abs().max() + 1e-12))
    record(what, r)
    return r


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mode", MODES)
def test_network_forward_matches_the_reference_fixture(mode, prec):
    vu, g = _net(mode)
    i = synth_inputs("vunet", 2, 128, int(g["seed"]))
    old = ops.TAP_SPARSE_LAUNCH
    try:
        with ops.precision(prec):
            ops.TAP_SPARSE_LAUNCH = False
            torch.manual_seed(int(g["fwd_seed"]))
            xt_dense = vu(i["y_tilde"].to(DEV), i["x"].to(DEV))[0].clone()
            ops.TAP_SPARSE_LAUNCH = True                              # the tap-skipping launches: the same bytes
            torch.manual_seed(int(g["fwd_seed"]))
            xt, mu_app, mu_shape = vu(i["y_tilde"].to(DEV), i["x"].to(DEV))
    finally:
        ops.TAP_SPARSE_LAUNCH = old
    assert torch.equal(xt, xt_dense)
    errs = {"x_tilde": _rel(xt, g["x_tilde"], f"{mode}_{prec}_x_tilde"),
            "mu_app0": _rel(mu_app[0], g["mu_app0"], f"{mode}_{prec}_mu_app0"), "mu_app1": _rel(mu_app[1], g["mu_app1"], f"{mode}_{prec}_mu_app1"),
            "mu_shape0": _rel(mu_shape[0], g["mu_shape0"], f"{mode}_{prec}_mu_shape0"),
            "mu_shape1": _rel(mu_shape[1], g["mu_shape1"], f"{mode}_{prec}_mu_shape1")}
    print(mode, prec, errs)
    assert tuple(xt.shape) == (2, 3, 128, 128) and max(errs.values()) < TOL_VU, errs


def test_recorded_pass_of_a_nearest_vunet_replays_the_eager_bytes():
    """A VehiclePipeline given a 'nearest' checkpoint builds that VUnet (the mode arrives with the weights); its recorded
    Vunet_fix_res.forward pass replays to the bytes of the eager one."""
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline
    vu, g = _net("nearest")
    pipe = VehiclePipeline(DEV, state_dicts={"vunet": vu.state_dict()})
    assert pipe.vunet.up_mode == "nearest" and not pipe.vunet.w_norm and not pipe.vunet.vunet_256
    i0, i1 = synth_inputs("vunet", 2, 128, 0), synth_inputs("vunet", 2, 128, 1)
    b0, b1 = ({"vu_y": i["y_tilde"].to(DEV), "vu_x": i["x"].to(DEV)} for i in (i0, i1))
    cp = pipe.compile(b0, vehicle_seeds=[7, 8], fn=pipe._vunet_forward)
    for batch, seeds in ((b0, [7, 8]), (b1, [9, 10])):
        want = {k: v.clone() for k, v in pipe.vunet_forward(batch, vehicle_seeds=seeds).items()}
        got = cp.run(batch, vehicle_seeds=seeds)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k
    # and the pipeline's network is the fixture's: same weights, same forward
    pipe.vunet.set_vehicle_seeds(None)
    torch.manual_seed(int(g["fwd_seed"]))
    xt = pipe.vunet(i0["y_tilde"].to(DEV), i0["x"].to(DEV))[0]
    assert _rel(xt, g["x_tilde"], "pipeline_nearest_x_tilde") < TOL_VU


@pytest.mark.parametrize("prec", PRECS)
def test_subpixel_upsample_is_the_plain_d2s_launch(prec):
    """Regression guard: UpSample('subpixel') through the network's `_upsample` == pack_conv + STORE_D2S called directly."""
    vu = Vunet_fix_res(Namespace(up_mode="subpixel", w_norm=False, drop_prob=0.0, vunet_256=False)).to(DEV).eval()
    up = vu.app_decoder_1_e
    assert isinstance(up, UpSample) and up.mode == "subpixel"
    x = ops.as_nhwc(torch.randn(2, 128, 8, 16, generator=torch.Generator().manual_seed(3)).to(DEV))
    vu._ensure(x)
    with ops.precision(prec):
        got = vu._upsample("app_decoder_1_e", x)
        plan = pack.pack_conv(up.depth4x.conv.weight, up.depth4x.conv.bias, stride=1, pad=1)
        assert plan.tap_sparse == 0
        want = ops.conv(plan, x, store=L.STORE_D2S)
    assert tuple(got.shape) == (2, 128, 16, 32) and torch.equal(got, want)
