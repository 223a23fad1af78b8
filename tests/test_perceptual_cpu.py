"""CPU: the feature-distance layer (csrc/perceptual.h) without a device - the exports, the host twins of fusg_gram_f32 and
fusg_abs_diff_rows_f32 against numpy float64 with derived bounds, the edgeconnect.loss drop-in's schema and argument checks,
install(losses=True), the fixtures against the float64 restatement, and the argument checks that precede every launch."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import perceptual_cases as pc
import perceptual_ref as pr
from conftest import GOLD, REPO, load_golden
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import ops

NEW_EXPORTS = ("fusg_gram_f32", "fusg_gram_scratch_bytes", "fusg_gram_chunk_pixels", "fusg_gram_f32_host", "fusg_abs_diff_rows_f32",
               "fusg_abs_diff_rows_scratch_bytes", "fusg_abs_diff_rows_f32_host")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def test_exports_declared_bound_and_built(lib):
    hdr = open(os.path.join(REPO, "include", "fusg.h")).read()
    for name in NEW_EXPORTS:
        assert name + "(" in hdr, name
        assert name in L.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.fusg_version() == 118


def test_chunk_rule(lib):
    """A function of (C, H W) only: a multiple of the 32-pixel staged block, at least 128, about 64 workgroups per image."""
    assert ops.gram_chunk(128, 1) == ops.gram_chunk(128, 128) == 128
    assert ops.gram_chunk(128, 16384) == 768                      # relu2_2 at 256^2: 3 tile pairs -> 22 chunks
    assert ops.gram_chunk(256, 4096) == 608 and ops.gram_chunk(512, 1024) == 512 and ops.gram_chunk(512, 256) == 128
    assert ops.gram_chunk(512, 379) == 192 and ops.gram_chunk(3, 10000) == 160
    assert ops.gram_chunk(1, 1 << 24) == (1 << 24) // 64
    for c, hw in ((0, 4), (1025, 4), (4, 0), (4, (1 << 24) + 1)):
        with pytest.raises(ValueError):
            ops.gram_chunk(c, hw)
    # scratch: fp32 [B][chunks][tile pairs][64][64]
    assert lib.fusg_gram_scratch_bytes(2, 128, 128, 128) == 2 * 22 * 3 * 4096 * 4
    assert lib.fusg_gram_scratch_bytes(1, 3, 1, 1) == 4096 * 4
    assert lib.fusg_gram_scratch_bytes(1, 1025, 4, 4) == -1 and lib.fusg_gram_scratch_bytes(1 << 16, 4, 4, 4) == -1
    assert lib.fusg_gram_scratch_bytes(1, 4, 1 << 13, 1 << 12) == -1
    assert lib.fusg_abs_diff_rows_scratch_bytes(3, 1, 1, 70001) == 3 * 18 * 8
    assert lib.fusg_abs_diff_rows_scratch_bytes(1, 4, 512, 520) == 256 * 8
    assert lib.fusg_abs_diff_rows_scratch_bytes(1, 1 << 11, 1 << 10, 1 << 10) == -1


@pytest.mark.parametrize("c,hw", pc.GRAM_CASES, ids=pc.GRAM_IDS)
def test_gram_host_twin_against_float64(lib, c, hw):
    """Per entry |G - G64| <= (gamma_n + 2u) S / (H W C): one fp32 fmaf chain of at most n = chunk pixels per chunk (gamma_n),
    the float64 chunk sum and division (2^-53 terms) and one rounding to fp32 (u), with u to spare; u = 2^-24, S = sum_p |x_i
    x_j|.  Derived, not measured.  Exactly symmetric; a row's bits are those of the row alone (B = 1) and of its copy in the
    same batch; the NaN padding channels of the pitched case are not read."""
    buf = pc.gram_buffer(c, hw)
    x = pc.view(buf, c)
    _, _, h, w = pc.gram_shape(c, hw)
    n = min(ops.gram_chunk(c, h * w), h * w)
    if hw in ("Kc+1", "3Kc-5", "big_hw"):
        assert h * w > ops.gram_chunk(c, h * w), "meant to be a multi-chunk case"
    g = ops.gram_host(x)
    assert g.shape == (3, c, c) and g.dtype == np.float32 and np.isfinite(g).all()
    g64, s = pc.gram_ref64(x)
    ratio = float((np.abs(g.astype(np.float64) - g64) / np.maximum(pc.gram_bound(s, n), 1e-300)).max())
    print(f"c={c} hw={h * w} chunk={ops.gram_chunk(c, h * w)}: max |G - G64| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert np.array_equal(g, g.transpose(0, 2, 1))
    assert np.array_equal(g[2], g[0])
    assert np.array_equal(ops.gram_host(x[1:2])[0], g[1])


def test_gram_host_takes_a_plain_array(lib):
    """A standard-contiguous [B, C, H, W] array is converted (channel stride 1 is the kernel's layout): same bits."""
    buf = pc.gram_buffer(20, "7x9")
    x = pc.view(buf, 20)
    assert np.array_equal(ops.gram_host(np.ascontiguousarray(x)), ops.gram_host(x))


@pytest.mark.parametrize("case", pc.ABS_CASES)
def test_abs_diff_rows_host_against_float64(lib, case):
    """Relative difference <= 1e-12: every |a - b| is exact in float64 and n <= 2^24 additions lose at most n 2^-53 = 1.9e-9
    in the worst case, ~sqrt(n) 2^-53 for a fixed-order tree - 1e-12 has room for the largest case here (1.06e6 elements)."""
    a, b = pc.abs_pair(case)
    got = ops.abs_diff_rows_host(a, b)
    want = pc.abs_ref64(a, b)
    assert got.shape == (a.shape[0],) and got.dtype == np.float64
    if case == "identical":
        assert (got == 0.0).all()
        return
    rel = float(np.abs(got / want - 1.0).max())
    print(case, "max relative difference", rel)
    assert rel <= 1e-12
    if case in ("pitched_nan", "groups"):
        assert got[2] == got[0]
        assert ops.abs_diff_rows_host(a[1:2], b[1:2])[0] == got[1]


# ---- module and drop-in
@pytest.fixture(scope="module")
def schema():
    with open(os.path.join(GOLD, "perceptual_schema.json")) as f:
        return json.load(f)


def test_state_dict_schema_is_the_references(schema):
    from future_urban_scene_generation_amd.edgeconnect import loss
    for name in ("VGG19", "PerceptualLoss", "StyleLoss"):
        sd = getattr(loss, name)().state_dict()
        assert [[k, list(v.shape)] for k, v in sd.items()] == schema[name], name
    assert len(schema["VGG19"]) == 32 and schema["VGG19"][0][0] == "relu1_1.0.weight" and schema["VGG19"][-1][0] == "relu5_4.34.bias"
    assert loss.PerceptualLoss().weights == [1.0] * 5 and loss.PerceptualLoss(weights=[1, 2, 3, 4, 5]).weights == [1, 2, 3, 4, 5]
    assert len(loss.FEATURE_DISTANCE_COLUMNS) == 9 and loss.FEATURE_DISTANCE_COLUMNS == pr.COLUMNS
    assert loss.USED_TAPS == tuple(n for n, _, _ in pr.tap_layers() if n in pr.PERCEPTUAL_TAPS + pr.STYLE_TAPS)
    with pytest.raises(NotImplementedError):
        loss.AdversarialLoss()
    with pytest.raises(NotImplementedError):
        loss.AdversarialLoss("hinge")


def test_load_torchvision_round_trips():
    """Default weights: the `features` part of synth_state_dict("vgg", vgg19_schema(10), seed).  A torchvision state dict
    (features.N.*, classifier.* ignored) lands under the reference's names; a missing or mis-shaped entry is refused."""
    from future_urban_scene_generation_amd.cad_classifier import vgg19_schema
    from future_urban_scene_generation_amd.edgeconnect.loss import TAPS, VGG19
    from future_urban_scene_generation_amd.synth import synth_state_dict
    feats = {k: v for k, v in vgg19_schema(10).items() if k.startswith("features.")}
    sd0 = synth_state_dict("vgg", feats, 0)
    vgg = VGG19()
    own = vgg.state_dict()
    for name, idx, _, _, _ in TAPS:
        assert torch.equal(own[f"{name}.{idx}.weight"], sd0[f"features.{idx}.weight"])
        assert torch.equal(own[f"{name}.{idx}.bias"], sd0[f"features.{idx}.bias"])
    assert not vgg.training and not any(p.requires_grad for p in vgg.parameters())
    sd3 = dict(synth_state_dict("vgg", feats, 3))
    sd3["classifier.0.weight"] = torch.zeros(2, 2)                # ignored
    gen = vgg.generation
    vgg.load_torchvision(sd3)
    assert vgg.generation > gen                                   # packed weights are rebuilt
    back = {f"features.{k.split('.', 1)[1]}": v for k, v in vgg.state_dict().items()}
    assert set(back) == set(feats) and all(torch.equal(back[k], sd3[k]) for k in feats)
    with pytest.raises(KeyError, match="features.0.bias"):
        vgg.load_torchvision({k: v for k, v in sd3.items() if k != "features.0.bias"})
    with pytest.raises(ValueError, match="features.2.weight"):
        vgg.load_torchvision(dict(sd3, **{"features.2.weight": torch.zeros(64, 3, 3, 3)}))


@pytest.mark.parametrize("shape", [(1, 3, 24, 32), (1, 3, 32, 8), (1, 4, 32, 32), (3, 32, 32), (1, 3, 0, 32)])
def test_bad_input_shapes_raise_value_error(shape):
    from future_urban_scene_generation_amd.edgeconnect.loss import VGG19
    vgg = VGG19()
    with pytest.raises(ValueError, match="multiples of 16"):
        vgg(torch.zeros(shape))
    with pytest.raises(ValueError, match="multiples of 16"):
        vgg.taps(torch.zeros(shape))


def test_install_losses_is_opt_in(tmp_path):
    """`from edgeconnect.loss import PerceptualLoss`: the reference's own file by default - through install() and through the
    dropin/ shim -, install(losses=True) / FUSG_DROPIN_LOSSES=1 select the forward-only device classes."""
    ref = tmp_path / "reference" / "edgeconnect"
    ref.mkdir(parents=True)
    (ref / "__init__.py").write_text("")
    (ref / "loss.py").write_text("class PerceptualLoss:\n    pass\n\nclass StyleLoss:\n    pass\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, str(tmp_path / "reference")]))
    env.pop("FUSG_DROPIN_LOSSES", None)
    code = ("import sys, future_urban_scene_generation_amd as f; f.install(); print('A', 'edgeconnect.loss' in sys.modules); "
            "import edgeconnect.loss as m0; print('A2', m0.PerceptualLoss.__module__); del sys.modules['edgeconnect.loss']; "
            "f.install(losses=True); import edgeconnect.loss as m; from edgeconnect.loss import PerceptualLoss, StyleLoss, VGG19; "
            "print('B', m.__name__, PerceptualLoss.__module__, StyleLoss.__module__)")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "A False" in r.stdout and "A2 edgeconnect.loss" in r.stdout
    mod = "future_urban_scene_generation_amd.edgeconnect.loss"
    assert f"B {mod} {mod} {mod}" in r.stdout
    code = "import edgeconnect.loss as m; from edgeconnect.loss import StyleLoss; print('RESULT', m.FUSG_DROPIN, StyleLoss.__module__)"
    base = dict(env, PYTHONPATH=os.pathsep.join([os.path.join(REPO, "dropin"), REPO, str(tmp_path / "reference")]))
    r = subprocess.run([sys.executable, "-c", code], env=base, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "RESULT False edgeconnect.loss" in r.stdout
    r = subprocess.run([sys.executable, "-c", code], env=dict(base, FUSG_DROPIN_LOSSES="1"), capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"RESULT True {mod}" in r.stdout


# ---- fixtures
@pytest.mark.parametrize("case", pc.SMALL_FIXTURES)
def test_restatement_reproduces_the_fixture(case):
    """The float64 restatement the GPU tests use (tests/perceptual_ref.py) on the recreated inputs gives the fixture's table,
    and its taps are the reference VGG19's: the stored corners and per-channel sums (float32 module against float64: 1e-5 of
    the tap's largest activation, 100x the reference's float32 error on these 10-to-16-layer stacks)."""
    from future_urban_scene_generation_amd.cad_classifier import vgg19_schema
    from future_urban_scene_generation_amd.synth import synth_state_dict
    g = load_golden(f"perceptual_{case}")
    sd = synth_state_dict("vgg", {k: v for k, v in vgg19_schema(10).items() if k.startswith("features.")}, int(g["weight_seed"]))
    assert json.loads(str(g["columns"])) == list(pr.COLUMNS)
    for kind in pc.PAIRS:
        x, y = pc.image_pair(case, kind)
        assert np.array_equal(x[:, :, :4, :4].numpy(), g[f"{kind}_x_corner"]) and np.array_equal(y[:, :, :4, :4].numpy(), g[f"{kind}_y_corner"])
        for t, want in ((x, float(g[f"{kind}_x_sum"])), (y, float(g[f"{kind}_y_sum"]))):
            assert abs(float(t.double().sum()) - want) <= 1e-12 * want  # (a float64 sum whose order may depend on the thread count)
        if kind == "lsb":
            d = torch.round((y - x) * 255.0)
            assert set(d.unique().tolist()) <= {-1.0, 0.0, 1.0} and 0.25 < float((d != 0).float().mean()) < 0.35
    x, y = pc.image_pair(case, "noise")
    t = pr.table(sd, x, y).numpy()
    assert np.abs(t / g["noise_table64"] - 1.0).max() <= 1e-12
    taps = pr.taps(sd, x)
    for n in pr.PERCEPTUAL_TAPS + pr.STYLE_TAPS:
        top = float(taps[n].max())
        assert np.abs(taps[n][:, :, :2, :2].numpy() - g[f"tap_{n}_corner"]).max() <= 1e-5 * top, n
        hw = taps[n].shape[2] * taps[n].shape[3]
        assert np.abs(taps[n].sum((2, 3)).numpy() - g[f"tap_{n}_chsum"]).max() <= 1e-5 * top * hw, n


def test_fixture_scalars_are_the_tables_means():
    """The reference's two float32 scalars are the column-mean sums of the float64 table up to the stored E_ref, and E_ref is
    of float32 size: at most 1e-4 (observed 2e-9 .. 1.6e-5; the 'lsb' pairs' small differences of Gram entries are the top)."""
    for case in pc.FIXTURES:
        g = load_golden(f"perceptual_{case}")
        b = pc.FIXTURES[case][0]
        for kind in pc.PAIRS:
            t = g[f"{kind}_table64"]
            assert t.shape == (b, 9) and t.dtype == np.float64 and (t > 0).all()
            for name, cols in (("perceptual", slice(0, 5)), ("style", slice(5, 9))):
                want = t[:, cols].sum(1).mean()
                e = abs(float(g[f"{kind}_{name}_ref"]) - want) / want
                assert g[f"{kind}_{name}_ref"].dtype == np.float32
                assert abs(e - float(g[f"{kind}_E_{name}"])) <= 1e-12 and e <= 1e-4, (case, kind, name, e)


# ---- refused arguments, through the ABI, without a device
def _aligned(nbytes=4096):
    raw = np.zeros(nbytes + 16, dtype=np.uint8)
    return raw, raw.ctypes.data + (-raw.ctypes.data) % 16


@pytest.mark.parametrize("what,shape,dtype,nchw", [
    ("not f32", (1, 4, 4, 4), L.U8, False), ("C = 1025", (1, 4, 4, 1025), L.F32, False), ("H W > 2^24", (1, 4097, 4096, 1), L.F32, False),
    ("channel stride", (1, 4, 4, 8), L.F32, True)])
def test_gram_refuses_bad_arguments_before_any_launch(lib, what, shape, dtype, nchw):
    """FUSG_ERR_INVALID with a message from the host twin AND from the launching entry point: its checks come first, so no
    device is touched (this test runs without one)."""
    buf = np.zeros(shape, dtype=np.uint8 if dtype == L.U8 else np.float32)          # [B, H, W, C]
    x = np.ascontiguousarray(buf.transpose(0, 3, 1, 2)) if nchw else buf.transpose(0, 3, 1, 2)
    d = ops._np_desc(x, dtype)
    out = np.zeros((1, 8, 8), dtype=np.float32)
    raw, scratch = _aligned()
    assert lib.fusg_gram_f32_host(C.byref(d), out.ctypes.data) == -1, what
    assert b"gram_f32_host" in lib.fusg_last_error()
    assert lib.fusg_gram_f32(C.byref(d), out.ctypes.data, scratch, None) == -1, what
    assert b"gram_f32" in lib.fusg_last_error()


def test_abs_diff_rows_refuses_bad_arguments_before_any_launch(lib):
    a, b = np.zeros((2, 3, 4, 5), dtype=np.float32), np.zeros((2, 3, 4, 6), dtype=np.float32)
    out = np.zeros(2, dtype=np.float64)
    raw, scratch = _aligned()
    for da, db, what in ((ops._np_desc(a, L.F32), ops._np_desc(b, L.F32), "shapes differ"),
                         (ops._np_desc(a, L.U8), ops._np_desc(a, L.U8), "not f32")):
        assert lib.fusg_abs_diff_rows_f32_host(C.byref(da), C.byref(db), out.ctypes.data) == -1, what
        assert b"abs_diff_rows_f32_host" in lib.fusg_last_error()
        assert lib.fusg_abs_diff_rows_f32(C.byref(da), C.byref(db), out.ctypes.data, scratch, None) == -1, what
        assert b"abs_diff_rows_f32" in lib.fusg_last_error()
    with pytest.raises(ValueError):
        ops.abs_diff_rows_host(a, b)
    with pytest.raises(ValueError):
        ops.gram_host(np.zeros((2, 3, 4), dtype=np.float32))
    # a misaligned or missing scratch is refused too
    d = ops._np_desc(a, L.F32)
    assert lib.fusg_abs_diff_rows_f32(C.byref(d), C.byref(d), out.ctypes.data, scratch + 4, None) == -1
    assert lib.fusg_gram_f32(C.byref(d), out.ctypes.data, None, None) == -1


def test_no_rows_succeed_and_launch_nothing(lib):
    x = np.zeros((0, 4, 8, 8), dtype=np.float32).transpose(0, 3, 1, 2)
    d = ops._np_desc(x, L.F32)
    assert lib.fusg_gram_f32(C.byref(d), None, None, None) == 0 and lib.fusg_gram_f32_host(C.byref(d), None) == 0
    assert lib.fusg_abs_diff_rows_f32(C.byref(d), C.byref(d), None, None, None) == 0
    assert ops.gram_host(x).shape == (0, 8, 8) and ops.abs_diff_rows_host(x, x).shape == (0,)


def test_pipeline_compare_methods_take_features_keyword_only():
    import inspect
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline
    for fn in (VehiclePipeline.compare_outputs, VehiclePipeline.compare_precisions):
        p = inspect.signature(fn).parameters["features"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
