"""GPU: batch-invariant routing (ops.route_batch / fusg_set_route_batch).  With a routing batch set, what a launch computes for
one image does not depend on the images it shares the launch with: row i of a B = 9 launch equals the B = 1 launch of image i,
bit for bit - for single conv layers of every kernel family, the streamed and fused norm statistics, the fused hourglass
Bottleneck, the VUnet's fused Residual pair and entry NiN, the four networks, and the frame drivers of the pipeline.  Every
comparison is torch.equal: an image passes through the same instructions in the same order."""
import os
import sys
from argparse import Namespace

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import batch_invariant_layers as bl                                        # noqa: E402
from conftest import synth_sd                                              # noqa: E402
from future_urban_scene_generation_amd import _lib as L                    # noqa: E402
from future_urban_scene_generation_amd import ops, pack                    # noqa: E402
from future_urban_scene_generation_amd import pipeline as pl               # noqa: E402
from future_urban_scene_generation_amd.synth import schema_of, synth_inputs, synth_state_dict   # noqa: E402

DEV = "cuda:0"
B = 9
ROWS = (0, 4, 8)
_CACHE = {}


@pytest.fixture(autouse=True)
def _clean_state():
    """Every test starts and ends with the mode off, in f16x3, with the range status clear."""
    ops.set_route_batch(0)
    ops.set_precision("f16x3")
    ops.range_exceeded(DEV)
    yield
    ops.set_route_batch(0)
    ops.set_precision("f16x3")


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not torch.equal(a, b):
        d = a.float() - b.float()
        print(f"{what}: {int((a != b).sum())} of {a.numel()} elements differ, max |diff| {float(d.abs().max()):.3e}")
    assert torch.equal(a, b), what


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _rows_equal(fn, xc, routes, rows=ROWS):
    """fn(NHWC device tensor) -> tensor or tuple of tensors with a leading batch axis.  Under every routing batch of `routes`,
    row i of the launch of all of xc equals the launch of image i alone."""
    x = ops.as_nhwc(xc.to(DEV))
    for R in routes:
        with ops.route_batch(R):
            full = fn(x)
            full = full if isinstance(full, (tuple, list)) else (full,)
            for i in rows:
                one = fn(ops.as_nhwc(xc[i:i + 1].to(DEV)))
                one = one if isinstance(one, (tuple, list)) else (one,)
                for k, (f, o) in enumerate(zip(full, one)):
                    _same(f[i:i + 1], o, f"R={R} row {i} output {k}")
    return x


def test_route_batch_api_exists():
    """Fails on a library or ops module without the feature."""
    with ops.route_batch(8):
        assert ops.ROUTE_BATCH == 8 and L.lib().fusg_route_batch() == 8
    assert ops.ROUTE_BATCH == 0 and L.lib().fusg_route_batch() == 0


# ------------------------------------------------------------------------------------------------ single conv layers
@pytest.mark.parametrize("prec", bl.PRECISIONS)
@pytest.mark.parametrize("name", list(bl.LAYERS))
def test_conv_layer_rows_do_not_depend_on_the_batch(name, prec):
    s = bl.LAYERS[name]
    plan = bl.plan_of(name)
    xc = _randn((B, s["cin"]) + s["hw"], 7 + len(name))
    conv = lambda x: ops.conv(plan, x, precision=prec)                      # noqa: E731
    today = conv(ops.as_nhwc(xc.to(DEV)))
    fam_today = ops.last_conv_kernel()
    assert fam_today == bl.route_order(name, B, prec, DEV)[0]
    x = _rows_equal(conv, xc, (1, 32))
    with ops.route_batch(B):                                                # R == n: today's launch at that n
        _same(conv(x), today, "route_batch(9) against the mode off")
        assert ops.last_conv_kernel() == fam_today
    _same(conv(x), today, "mode off again")
    assert not ops.range_exceeded(DEV)
    for R in (1, 32):                                                       # the launches ran on the family the dry run names
        with ops.route_batch(R):
            want = bl.route_order(name, 1, prec, DEV)[0]                    # (the same for every n: test_batch_invariant_cpu.py)
            conv(x)
            assert ops.last_conv_kernel() == want, (R, ops.last_conv_kernel(), want)


# ------------------------------------------------------------------------------------------------ norm statistics
@pytest.mark.parametrize("hw", ((32, 32), (96, 96)), ids=("32x32", "96x96"))
def test_streamed_statistics_rows(hw):
    """instnorm_stats / layernorm_stats at [B, 64, h, w].  At 96 x 96 the number of partial sums per image differs between B = 1
    and B = 9 with the mode off (144 against 113); at 32 x 32 it is 16 for both."""
    n_off = [ops._nchunk(b, 64, hw[0] * hw[1]) for b in (1, B)]
    assert (n_off[0] != n_off[1]) == (hw == (96, 96)), n_off
    xc = _randn((B, 64) + hw, 21) * 1.5 + 0.3
    gamma, beta = (_randn((64,), 22) * 0.2 + 1.0).to(DEV), (_randn((64,), 23) * 0.1).to(DEV)
    x = _rows_equal(lambda t: ops.instnorm_stats(t), xc, (1, 32))
    _rows_equal(lambda t: ops.layernorm_stats(t, gamma, beta), xc, (1, 32))
    today = ops.instnorm_stats(x), ops.layernorm_stats(x, gamma, beta)
    with ops.route_batch(B):
        got = ops.instnorm_stats(x), ops.layernorm_stats(x, gamma, beta)
    for a, b in zip(today, got):
        for u, v in zip(a, b):
            _same(u, v, "route_batch(9) against the mode off")


def test_fused_statistics_rows():
    """conv_in (InstanceNorm statistics out of the conv epilogue) and conv_ln: 64 -> 64 k3 p1 at 32 x 32.  With R = 32 the launch
    keeps K whole and the statistics are fused at B = 1 too; with R = 1 it is a split-K launch and they are streamed."""
    g = torch.Generator().manual_seed(31)
    plan = pack.pack_conv(torch.randn(64, 64, 3, 3, generator=g) / 24.0, torch.randn(64, generator=g) * 0.1, pad=1)
    xc = _randn((B, 64, 32, 32), 32)
    gamma, beta = (_randn((64,), 33) * 0.2 + 1.0).to(DEV), (_randn((64,), 34) * 0.1).to(DEV)

    def conv_in(t):
        out, (sc, sh) = ops.conv_in(plan, t)
        return out, sc, sh

    def conv_ln(t):
        out, (sc, sh) = ops.conv_ln(plan, t, gamma, beta)
        return out, sc, sh

    x = _rows_equal(conv_in, xc, (1, 32))
    _rows_equal(conv_ln, xc, (1, 32))
    fused = {}
    for R in (1, 32):
        with ops.route_batch(R):
            fused[R] = [ops.conv(plan, t, want_stats=True)[1] is not None for t in (x, ops.as_nhwc(xc[:1].to(DEV)))]
    assert fused == {1: [False, False], 32: [True, True]}, fused
    today = conv_in(x)
    with ops.route_batch(B):
        for a, b in zip(today, conv_in(x)):
            _same(a, b, "route_batch(9) against the mode off")


# ------------------------------------------------------------------------------------------------ fused blocks
def _hourglass():
    if "hg" not in _CACHE:
        from future_urban_scene_generation_amd.stacked_hourglass.models import HourglassNet
        hg = HourglassNet(2, 1, 12)
        hg.load_state_dict(synth_sd("hg"))
        _CACHE["hg"] = hg.to(DEV).eval()
    return _CACHE["hg"]


def test_hourglass_bottleneck_rows(monkeypatch):
    """One Bottleneck, 128 planes at 16 x 16, B in {1, 8, 9}.  With the mode off the block is three launches up to B = 8 and one
    fused launch from 9; under route_batch(8) it is three launches for all, under route_batch(32) the fused one."""
    for k in ("FUSG_NO_BNECK", "FUSG_BNECK_MAXHW", "FUSG_NO_SMALL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(ops, "BNECK_MINHW", None)
    hg = _hourglass()
    P = hg._ensure(torch.zeros(1, 3, 64, 64, device=DEV))
    p = P["hg"][0][0][0][0]
    assert p["c1"].cout == 128 and p["c1"].c0k == 256
    xc = _randn((B, 256, 16, 16), 41)
    xs = {b: ops.as_nhwc(xc[:b].to(DEV)) for b in (1, 8, 9)}
    assert [ops.bottleneck_ok(p, xs[b]) for b in (1, 8, 9)] == [False, False, True]
    for R, fused in ((8, False), (32, True)):
        with ops.route_batch(R):
            assert [ops.bottleneck_ok(p, xs[b]) for b in (1, 8, 9)] == [fused] * 3
            outs = {b: hg._bottleneck(p, xs[b]) for b in (1, 8, 9)}
            assert (ops.last_conv_kernel() == 6) == fused
            for i in range(B):
                one = hg._bottleneck(p, ops.as_nhwc(xc[i:i + 1].to(DEV)))
                _same(outs[9][i:i + 1], one, f"R={R} B=9 row {i}")
                if i < 8:
                    _same(outs[8][i:i + 1], one, f"R={R} B=8 row {i}")
            _same(outs[1], outs[9][:1], f"R={R} B=1")
    assert not ops.range_exceeded(DEV)


def _respair_plans():
    if "respair" not in _CACHE:
        g = torch.Generator().manual_seed(51)
        k3 = lambda: pack.pack_conv(torch.randn(32, 32, 3, 3, generator=g) / 17.0, torch.randn(32, generator=g) * 0.1, pad=1)    # noqa: E731
        k1 = lambda: pack.pack_conv(torch.randn(32, 32, 1, 1, generator=g) / 5.7, torch.randn(32, generator=g) * 0.1)          # noqa: E731
        _CACHE["respair"] = (k3(), k3(), k1(), k1())
    return _CACHE["respair"]


def test_vunet_respair_rows():
    """fusg_vunet_respair at 32 x 64 (16 patches per image), tap_order 0: the K split over the waves up to 1024 patches of the
    ROUTING batch - R = 1 and 32 split like tap_order 2, R = 128 (2048 patches) sums the taps in order like tap_order 1."""
    plans = _respair_plans()
    xc = _randn((B, 32, 32, 64), 52)
    x = _rows_equal(lambda t: ops.respair(*plans, t), xc, (1, 32, 128), rows=range(B))
    assert ops.last_conv_kernel() == 12
    in_order, split = ops.respair(*plans, x, tap_order=1), ops.respair(*plans, x, tap_order=2)
    assert not torch.equal(in_order[0], split[0])                           # the two orders do differ in their bits
    for R, want in ((1, split), (32, split), (128, in_order), (0, split), (B, split)):
        with ops.route_batch(R):
            for a, b in zip(ops.respair(*plans, x), want):
                _same(a, b, f"R={R} against the explicit tap order")
    assert not ops.range_exceeded(DEV)


def _entry_plans():
    if "entry" not in _CACHE:
        g = torch.Generator().manual_seed(61)
        nin = pack.pack_conv(torch.randn(128, 6, 1, 1, generator=g) / 6 ** 0.5, torch.randn(128, generator=g) * 0.1)
        res = pack.pack_conv(torch.randn(128, 128, 3, 3, generator=g) / (3.0 * 128 ** 0.5), torch.randn(128, generator=g) * 0.1, pad=1)
        _CACHE["entry"] = (nin, res)
    return _CACHE["entry"]


def test_entry_nin_rows():
    """The entry NiN + Residual pair as the VUnet issues it (fused where entry_nin_form allows, else two launches), at the
    smallest shape whose form differs between B = 1 and B = 9 with the mode off."""
    nin, res = _entry_plans()
    form = lambda b, h, w: ops.entry_nin_form(nin, res, ops.as_nhwc(torch.zeros(b, 6, h, w, device=DEV)))    # noqa: E731
    shapes = sorted(((h, w) for h in range(8, 136, 8) for w in range(16, 144, 16)), key=lambda s: (s[0] * s[1], s[0]))
    hw = next(s for s in shapes if form(1, *s) != form(B, *s))
    print("entry NiN: smallest shape whose form differs", hw, form(1, *hw), form(B, *hw))
    assert form(1, *hw) != form(B, *hw)
    ran = []

    def pair(u):
        if ops.entry_nin_ok(nin, res, u):
            out = ops.entry_nin(nin, res, u)
        else:
            x0 = ops.conv(nin, u, pre_op=L.PRE_ELU)
            out = ops.conv(res, x0, pre_op=L.PRE_ELU, res0=x0)
        ran.append(ops.last_conv_kernel())
        return out

    xc = _randn((B, 6) + hw, 62)
    for R in (1, 32):
        with ops.route_batch(R):
            assert form(1, *hw) == form(B, *hw)
        del ran[:]
        _rows_equal(pair, xc, (R,))
        assert len(set(ran)) == 1, (R, ran)                                 # one kernel family for the batch and for each image
    assert not ops.range_exceeded(DEV)


# ------------------------------------------------------------------------------------------------ whole networks
def _net(name):
    if name in _CACHE:
        return _CACHE[name]
    if name == "hg":
        return _hourglass()
    if name == "icn":
        from future_urban_scene_generation_amd.warp_learn.models import G_Resnet
        net = G_Resnet(21)
        net.load_state_dict(synth_sd("icn"))
    elif name == "vunet":
        from future_urban_scene_generation_amd.vunet.models import Vunet_fix_res
        net = Vunet_fix_res(Namespace(up_mode="subpixel", w_norm=True, drop_prob=0.2, vunet_256=False))
        net.load_state_dict(synth_state_dict("vunet", schema_of(net.state_dict()), 0))
    else:
        from future_urban_scene_generation_amd.edgeconnect.models import EdgeModel, InpaintingModel
        em, im = EdgeModel(None), InpaintingModel(None)
        em.generator.load_state_dict(synth_sd("edge"))
        im.generator.load_state_dict(synth_sd("inpaint"))
        _CACHE[name] = (em.to(DEV).eval(), im.to(DEV).eval())
        return _CACHE[name]
    _CACHE[name] = net.to(DEV).eval()
    return _CACHE[name]


def _network_rows(run, n_rows=B):
    """run(lo, hi) -> dict of tensors for the images [lo, hi).  Under route_batch(8) every row of the pass of all images equals
    that image's own pass."""
    with ops.route_batch(8):
        full = run(0, n_rows)
        for i in range(n_rows):
            one = run(i, i + 1)
            for k in full:
                _same(full[k][i:i + 1], one[k], f"{k} row {i}")
    assert not ops.range_exceeded(DEV)
    return full


@pytest.mark.parametrize("prec", ("f16x3", "f32"))
def test_hourglass_rows(prec):
    hg = _hourglass()
    x = synth_inputs("hg", B, 64, seed=3)["x"].to(DEV)

    def run(lo, hi):
        hm = hg(x[lo:hi].contiguous())["heatmaps"]
        return {"hm0": hm[0], "hm1": hm[1], "kp_idx": ops.argmax_hw(hm[-1])}

    with ops.precision(prec):
        full = _network_rows(run)
        assert full["kp_idx"].dtype == torch.int32 and tuple(full["kp_idx"].shape) == (B, 12)


def test_icn_rows():
    icn = _net("icn")
    x = synth_inputs("icn", B, 64, seed=3)["x"].to(DEV)
    _network_rows(lambda lo, hi: {"y": icn(x[lo:hi].contiguous())})


def test_vunet_forward_rows():
    """Vunet_fix_res.forward at 128 x 128 with a seed per vehicle: the noise of a row is its own, so are its bits."""
    vu = _net("vunet")
    i = synth_inputs("vunet", B, 128, seed=3)
    x, y = i["x"].to(DEV), i["y_tilde"].to(DEV)

    def run(lo, hi):
        vu.set_vehicle_seeds([900 + v for v in range(lo, hi)])
        xt, mu_app, mu_shape = vu(y[lo:hi].contiguous(), x[lo:hi].contiguous())
        out = {"x_tilde": xt}
        out.update({f"mu_app_{k}": t for k, t in enumerate(mu_app)})
        out.update({f"mu_shape_{k}": t for k, t in enumerate(mu_shape)})
        return out

    try:
        _network_rows(run)
    finally:
        vu.set_vehicle_seeds(None)


def test_edgeconnect_rows():
    em, im = _net("edgeconnect")
    i = {k: v.to(DEV) for k, v in synth_inputs("edge", B, 64, seed=3).items()}

    def run(lo, hi):
        s = {k: v[lo:hi].contiguous() for k, v in i.items()}
        e = em(s["gray"], s["edge"], s["mask"])
        return {"edges": e, "inpainted": im(s["img"], e, s["mask"])}

    _network_rows(run)


# ------------------------------------------------------------------------------------------------ the pipeline
def test_pipeline_batched_frames_equal_per_frame_passes():
    """VehiclePipeline(route_batch=8): three scenes of 1 / 2 / 3 vehicles with seeds.  The crops of run_frames_batched - replayed
    (six rows padded to eight) and eager unpadded - equal run_frame's per scene (batches of 1, 2 and 3), byte for byte; the recorded
    plan is kept under a key that names the routing batch, and nothing is left set behind the calls."""
    sds = {n: synth_sd(n) for n in ("hg", "icn", "vunet")}
    pipe = pl.VehiclePipeline(DEV, state_dicts=sds, route_batch=8)
    scenes = []
    for V, seed, base in ((1, 11, 31), (2, 17, 11), (3, 49, 51)):
        sc = pl.synth_frame(V, (360, 640), DEV, seed=seed)
        sc["vehicle_seeds"] = [base + v for v in range(V)]
        scenes.append(sc)
    keys = ("icn_u8", "vunet_u8", "kp_idx")
    per_frame = [pipe.run_frame(sc) for sc in scenes]
    assert ops.ROUTE_BATCH == 0 and L.lib().fusg_route_batch() == 0
    replayed = pipe.run_frames_batched(scenes, replay=True)
    eager = pipe.run_frames_batched(scenes)
    again = pipe.run_frames_batched(scenes, replay=True)
    assert ops.ROUTE_BATCH == 0 and L.lib().fusg_route_batch() == 0
    for f, sc in enumerate(scenes):
        for k in keys:
            _same(replayed[f][k], per_frame[f][k], f"replay, scene {f}, {k}")
            _same(eager[f][k], per_frame[f][k], f"eager, scene {f}, {k}")
            _same(again[f][k], per_frame[f][k], f"second replay, scene {f}, {k}")
        for a, b in zip(replayed[f]["state"]["appearance"], per_frame[f]["state"]["appearance"]):
            _same(a, b, f"replay, scene {f}, appearance")
    batch_keys = [k for k in pipe._frame_plans if k[0] == "frame_batch"]
    assert batch_keys == [("frame_batch", 8, ops.PRECISION, ("route_batch", 8))], batch_keys
    # the same pipeline under another routing batch records another plan: a replay never mixes routings
    pipe.route_batch = 2
    pipe.run_frames_batched(scenes, replay=True)
    assert ("frame_batch", 8, ops.PRECISION, ("route_batch", 2)) in pipe._frame_plans
    assert ("frame_batch", 8, ops.PRECISION, ("route_batch", 8)) in pipe._frame_plans


def test_recorded_pass_keeps_its_routing():
    """A pass recorded under a routing batch replays under it whatever is set later (fusg.h: a recorded launch is re-issued
    under the value it was recorded with)."""
    sds = {n: synth_sd(n) for n in ("hg", "icn", "vunet")}
    pipe = pl.VehiclePipeline(DEV, state_dicts=sds)
    batch = pl.synth_batch(2, 256, DEV, seed=5)
    seeds = [5, 6]
    with ops.route_batch(32):
        want = {k: v.clone() for k, v in pipe.run(batch, seeds).items()}
        cp = pipe.compile(batch, seeds)
    assert cp.route_batch == 32 and ops.ROUTE_BATCH == 0
    got = cp.run(batch, seeds)                                              # replayed with the mode off
    for k in ("kp_idx", "icn_u8", "vunet_u8"):
        _same(got[k], want[k], k)
