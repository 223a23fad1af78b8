"""CPU: the per-image metrics (csrc/metrics.h) without a device - the exports, the host twin of fusg_image_metrics_u8 against
oracle.ssim and numpy, the edge counts, the drop-in PSNR / EdgeAccuracy on CPU tensors, install(metrics=True), and the
argument checks that precede every launch."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_metrics_cases as mc
from conftest import REPO
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import ops

NEW_EXPORTS = ("fusg_image_metrics_u8", "fusg_image_metrics_scratch_bytes", "fusg_image_metrics_host", "fusg_edge_counts",
               "fusg_edge_counts_host", "fusg_sq_diff_sum_f32")
COL = {n: i for i, n in enumerate(("ssim", "mse", "psnr", "max_abs", "n_diff", "sse"))}


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
    assert ops.IMAGE_METRIC_COLUMNS == tuple(COL)


@pytest.mark.parametrize("case", mc.CASES)
def test_host_twin_ssim_is_the_oracles(lib, case):
    """Per row and for the batch within 1e-9 of oracle.ssim: float64 rounding through the variance cancellation (a factor of at
    most 65025 / 58 on 1e-16) with room to spare.  float32 window sums would miss `flat` by 1.4e-5."""
    import oracle
    a, b = mc.pair(case)
    t = mc.host_table(case)
    assert t.shape == (a.shape[0], 6) and t.dtype == np.float64
    err = np.abs(t[:, COL["ssim"]] - mc.oracle_rows(case))
    print(case, "per-row |ssim - oracle| max", err.max())
    assert err.max() <= 1e-9
    assert abs(t[:, COL["ssim"]].mean() - oracle.ssim(a.copy(), b.copy())) <= 1e-9
    if case == "flat":
        assert abs(t[0, COL["ssim"]] - 0.99952068) < 1e-8
    if case == "identical":
        assert (t[:, COL["ssim"]] == 1.0).all()


@pytest.mark.parametrize("case", mc.CASES)
def test_host_twin_integer_columns_are_exact(lib, case):
    a, b = mc.pair(case)
    t = mc.host_table(case)
    mx, nd, sse = mc.numpy_integers(a, b)
    assert np.array_equal(t[:, COL["max_abs"]], mx.astype(np.float64))
    assert np.array_equal(t[:, COL["n_diff"]], nd.astype(np.float64))
    assert np.array_equal(t[:, COL["sse"]], sse.astype(np.float64))
    n = a.shape[1] * a.shape[2] * a.shape[3]
    mse = sse.astype(np.float64) / n
    assert np.array_equal(t[:, COL["mse"]], mse)
    for r in range(a.shape[0]):
        if sse[r] == 0:
            assert t[r, COL["psnr"]] == math.inf
        else:                                                     # (two libm log10 of one argument: a few ulp at most)
            assert abs(t[r, COL["psnr"]] - 10.0 * math.log10(255.0 ** 2 / mse[r])) <= 1e-12 * 100
    if case == "far":
        assert (mx == 255).all() and (sse == 255 ** 2 * n).all() and (t[:, COL["psnr"]] == 0.0).all()
    if case == "border":
        assert (nd == 9 * 3).all()                                # four corners + one pixel in each of rows 0..4, 3 channels


def _edge_maps():
    rng = np.random.default_rng(77)
    x = rng.random((4, 1, 19, 23)).astype(np.float32)
    y = rng.random((4, 1, 19, 23)).astype(np.float32)
    x[1], y[1] = x[1] * 0.4, y[1] * 0.4                           # a row with everything below the threshold
    x[2, 0, :4], y[2, 0, 2:6] = 0.5, 0.5                          # values equal to the threshold: not counted (strict >)
    x[3, 0, 0, 0] = np.nan                                        # a NaN is not above anything
    return x, y


def _edge_numpy(x, y, t):
    t = np.float32(t)
    bx, by = x > t, y > t
    return np.stack([bx.reshape(len(x), -1).sum(1), by.reshape(len(x), -1).sum(1), (bx & by).reshape(len(x), -1).sum(1)], axis=1)


def test_edge_counts_host_equals_numpy(lib):
    x, y = _edge_maps()
    for t in (0.5, 0.25, 2.0):
        got = ops.edge_counts_host(x, y, t)
        assert got.dtype == np.int64 and np.array_equal(got, _edge_numpy(x, y, t)), t
    got = ops.edge_counts_host(x, y, 0.5)
    assert got[1].tolist() == [0, 0, 0]
    assert got[2, 0] == (x[2, 0, 4:] > 0.5).sum()
    # strided views (a channel slice of a wider tensor) read the right elements
    wide = np.zeros((4, 3, 19, 23), dtype=np.float32)
    wide[:, 1:2] = x
    assert np.array_equal(ops.edge_counts_host(wide[:, 1:2], y, 0.5), got)


def test_dropin_edge_accuracy_on_cpu_tensors(lib):
    from future_urban_scene_generation_amd.edgeconnect.metrics import EdgeAccuracy
    x, y = _edge_maps()
    acc = EdgeAccuracy()                                          # the reference's default threshold
    assert acc.threshold == 0.5
    p, r = acc(torch.from_numpy(x[:3]), torch.from_numpy(y[:3]))
    rel, sel, tp = (float(v) for v in _edge_numpy(x[:3], y[:3], 0.5).sum(axis=0))
    assert p.dim() == 0 and r.dim() == 0
    assert abs(float(p) - tp / (sel + 1e-8)) <= 2.0 ** -23 and abs(float(r) - tp / (rel + 1e-8)) <= 2.0 ** -23
    # nothing relevant, nothing selected: (1, 1)
    p, r = EdgeAccuracy(0.5)(torch.from_numpy(x[1:2]), torch.from_numpy(y[1:2]))
    assert int(p) == 1 and int(r) == 1
    # nothing selected but something relevant: precision 0 / 1e-8 = 0, recall 0
    p, r = EdgeAccuracy(threshold=0.5)(torch.from_numpy(x[:1]), torch.zeros(1, 1, 19, 23))
    assert float(p) == 0.0 and float(r) == 0.0


def test_dropin_psnr_on_cpu_tensors(lib):
    from future_urban_scene_generation_amd.edgeconnect.metrics import PSNR
    a, b = mc.pair("ragged")
    ta, tb = torch.from_numpy(a.copy()), torch.from_numpy(b.copy())
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    want = 20.0 * math.log10(255.0) - 10.0 * math.log10(mse)
    got = PSNR(255.)(ta, tb)
    assert got.dim() == 0 and abs(float(got) - want) <= 2.0 ** -23 * want
    # uint8 in another layout (not a [B, H, W, C <= 4] batch): the same number by the plain float64 sum
    got = PSNR(255.)(ta.permute(0, 3, 1, 2).contiguous(), tb.permute(0, 3, 1, 2).contiguous())
    assert abs(float(got) - want) <= 2.0 ** -23 * want
    assert int(PSNR(255.)(ta, ta.clone())) == 0                   # mse == 0 -> 0
    rng = np.random.default_rng(5)
    fa, fb = rng.random((2, 1, 32, 32)).astype(np.float32), rng.random((2, 1, 32, 32)).astype(np.float32)
    want = 20.0 * math.log10(1.0) - 10.0 * math.log10(((fa.astype(np.float64) - fb.astype(np.float64)) ** 2).mean())
    got = PSNR(1.)(torch.from_numpy(fa), torch.from_numpy(fb))
    assert abs(float(got) - want) <= 2.0 ** -23 * abs(want)
    assert int(PSNR(1.)(torch.from_numpy(fa), torch.from_numpy(fa.copy()))) == 0
    assert set(PSNR(255.).state_dict()) == {"base10", "max_val"}  # the reference's buffers


def test_install_metrics_is_opt_in(tmp_path):
    """`from edgeconnect.metrics import PSNR, EdgeAccuracy`: the reference's own file by default - through install() and
    through the dropin/ shim -, install(metrics=True) / FUSG_DROPIN_METRICS=1 select the device-counting classes."""
    ref = tmp_path / "reference" / "edgeconnect"
    ref.mkdir(parents=True)
    (ref / "__init__.py").write_text("")
    (ref / "metrics.py").write_text("class PSNR:\n    pass\n\nclass EdgeAccuracy:\n    pass\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, str(tmp_path / "reference")]))
    env.pop("FUSG_DROPIN_METRICS", None)
    code = ("import sys, future_urban_scene_generation_amd as f; f.install(); print('A', 'edgeconnect.metrics' in sys.modules); "
            "import edgeconnect.metrics as m0; print('A2', m0.PSNR.__module__); del sys.modules['edgeconnect.metrics']; "
            "f.install(metrics=True); import edgeconnect.metrics as m; from edgeconnect.metrics import PSNR, EdgeAccuracy; "
            "print('B', m.__name__, PSNR.__module__, EdgeAccuracy(0.5).threshold)")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "A False" in r.stdout and "A2 edgeconnect.metrics" in r.stdout
    assert "B future_urban_scene_generation_amd.edgeconnect.metrics future_urban_scene_generation_amd.edgeconnect.metrics 0.5" in r.stdout
    code = "import edgeconnect.metrics as m; from edgeconnect.metrics import PSNR; print('RESULT', m.FUSG_DROPIN, PSNR.__module__)"
    base = dict(env, PYTHONPATH=os.pathsep.join([os.path.join(REPO, "dropin"), REPO, str(tmp_path / "reference")]))
    r = subprocess.run([sys.executable, "-c", code], env=base, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "RESULT False edgeconnect.metrics" in r.stdout
    r = subprocess.run([sys.executable, "-c", code], env=dict(base, FUSG_DROPIN_METRICS="1"), capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "RESULT True future_urban_scene_generation_amd.edgeconnect.metrics" in r.stdout


def _pair_descs(shape_a, shape_b=None, dtype=L.U8):
    a = np.zeros(shape_a, dtype=np.uint8)
    b = np.zeros(shape_a if shape_b is None else shape_b, dtype=np.uint8)
    return a, b, ops._np_desc(a.transpose(0, 3, 1, 2), dtype), ops._np_desc(b.transpose(0, 3, 1, 2), dtype)


@pytest.mark.parametrize("what,shape_a,shape_b,dtype", [
    ("H = 10", (1, 10, 16, 3), None, L.U8), ("W = 10", (1, 16, 10, 3), None, L.U8), ("C = 5", (1, 16, 16, 5), None, L.U8),
    ("shapes differ", (2, 16, 16, 3), (2, 16, 17, 3), L.U8), ("batches differ", (2, 16, 16, 3), (1, 16, 16, 3), L.U8),
    ("not uint8", (1, 16, 16, 3), None, L.F32)])
def test_bad_arguments_are_refused_before_any_launch(lib, what, shape_a, shape_b, dtype):
    """FUSG_ERR_INVALID with a message from the host twin AND from the launching entry point: its checks come first, so no
    device is touched (this test runs without one)."""
    a, b, da, db = _pair_descs(shape_a, shape_b, dtype)
    out = np.zeros((2, 6), dtype=np.float64)
    raw = np.zeros(4096 + 16, dtype=np.uint8)
    scratch = raw.ctypes.data + (-raw.ctypes.data) % 16
    assert lib.fusg_image_metrics_host(C.byref(da), C.byref(db), out.ctypes.data) == -1, what
    assert b"image_metrics_host" in lib.fusg_last_error()
    assert lib.fusg_image_metrics_u8(C.byref(da), C.byref(db), out.ctypes.data, scratch, None) == -1, what
    assert b"image_metrics_u8" in lib.fusg_last_error()
    if dtype == L.U8 and shape_b is None:
        assert lib.fusg_image_metrics_scratch_bytes(*[shape_a[i] for i in (0, 1, 2, 3)]) == -1


def test_no_rows_succeed_and_launch_nothing(lib):
    a, b, da, db = _pair_descs((0, 16, 16, 3))
    assert lib.fusg_image_metrics_host(C.byref(da), C.byref(db), None) == 0
    assert lib.fusg_image_metrics_u8(C.byref(da), C.byref(db), None, None, None) == 0     # (a launch would need a device)
    assert ops.image_metrics_host(a, b).shape == (0, 6)
    x = np.zeros((0, 1, 8, 8), dtype=np.float32)
    assert lib.fusg_edge_counts(C.byref(ops._np_desc(x, L.F32)), C.byref(ops._np_desc(x, L.F32)), 0.5, None, None) == 0
    assert ops.edge_counts_host(x, x).shape == (0, 3)
    # edge counts: mismatched shapes and a non-float tensor are refused
    x1, x2 = np.zeros((1, 1, 8, 8), dtype=np.float32), np.zeros((1, 1, 8, 9), dtype=np.float32)
    out = np.zeros((1, 3), dtype=np.int64)
    assert lib.fusg_edge_counts_host(C.byref(ops._np_desc(x1, L.F32)), C.byref(ops._np_desc(x2, L.F32)), 0.5, out.ctypes.data) == -1
    assert lib.fusg_edge_counts(C.byref(ops._np_desc(x1, L.U8)), C.byref(ops._np_desc(x1, L.U8)), 0.5, out.ctypes.data, None) == -1
    assert lib.fusg_sq_diff_sum_f32(None, None, 4, None, None) == -1


def test_scratch_size(lib):
    # 16 x 16 tiles of valid positions: 256^2 -> 246^2 positions -> 16 x 16 tiles; 24 bytes per (row, tile)
    assert lib.fusg_image_metrics_scratch_bytes(64, 256, 256, 3) == 64 * 256 * 24
    assert lib.fusg_image_metrics_scratch_bytes(3, 43, 37, 3) == 3 * 6 * 24
    assert lib.fusg_image_metrics_scratch_bytes(1, 11, 11, 1) == 32              # one tile, rounded up to 16 bytes
    assert lib.fusg_image_metrics_scratch_bytes(-1, 16, 16, 3) == -1


def test_pipeline_methods_refuse_bad_arguments_without_a_device():
    """`compare_precisions` checks its arguments before any launch (it needs no device to say no)."""
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline
    pipe = VehiclePipeline.__new__(VehiclePipeline)               # no networks: the checks come before anything uses them
    with pytest.raises(ValueError, match="vehicle_seeds"):
        pipe.compare_precisions({}, None)
    with pytest.raises(ValueError, match="precision"):
        pipe.compare_precisions({}, [1], precision="fp8")
    with pytest.raises(ValueError, match="precision"):
        pipe.compare_precisions({}, [1], against="nope")
