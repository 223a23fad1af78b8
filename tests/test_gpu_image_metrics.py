"""GPU: the per-image metrics kernels (csrc/metrics.hip) against their host twin and the oracle, row independence, a recorded
pass, the edge counts, the drop-in PSNR / EdgeAccuracy on device tensors and VehiclePipeline.compare_outputs /
compare_precisions.

The host twin was built to walk the kernel's order of sums (tiles, positions of a tile, the halving trees: csrc/metrics.h), so
its `ssim` is bit-equal to the kernel's on every case here (observed on an MI355X; recorded through conftest.record); the tests
assert the 1e-12 bound the two are held to and print what they saw."""
import math

import numpy as np
import pytest
import torch

import image_metrics_cases as mc
from conftest import record
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COL = {n: i for i, n in enumerate(ops.IMAGE_METRIC_COLUMNS)}


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)                  # (a writable, contiguous copy: the cases are read-only)


def _table(a, b):
    return ops.image_metrics_u8(_dev(a), _dev(b)).cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


@pytest.mark.parametrize("case", mc.CASES)
def test_kernel_equals_host_twin_and_oracle(case):
    a, b = mc.pair(case)
    got, want = _table(a, b), mc.host_table(case)
    assert got.shape == want.shape == (a.shape[0], 6)
    for c in ("max_abs", "n_diff", "sse", "mse"):                 # exact integers (and their quotient)
        assert np.array_equal(got[:, COL[c]], want[:, COL[c]]), c
    mx, nd, sse = mc.numpy_integers(a, b)
    assert np.array_equal(got[:, COL["max_abs"]], mx) and np.array_equal(got[:, COL["n_diff"]], nd) and np.array_equal(got[:, COL["sse"]], sse)
    d_twin = np.abs(got[:, COL["ssim"]] - want[:, COL["ssim"]]).max()
    d_oracle = np.abs(got[:, COL["ssim"]] - mc.oracle_rows(case)).max()
    print(case, "ssim: |kernel - twin|", d_twin, "bit-equal", np.array_equal(_bits(got[:, COL["ssim"]]), _bits(want[:, COL["ssim"]])),
          "|kernel - oracle|", d_oracle)
    record(f"{case}_ssim_vs_twin", d_twin)
    record(f"{case}_ssim_vs_oracle", d_oracle)
    assert d_twin <= 1e-12
    assert d_oracle <= 1e-9
    fin = np.isfinite(want[:, COL["psnr"]])
    assert np.array_equal(np.isposinf(got[:, COL["psnr"]]), ~fin)
    assert np.all(np.abs(got[fin, COL["psnr"]] - want[fin, COL["psnr"]]) <= 1e-12 * 100)      # (device / host log10: ulps)


def test_a_row_does_not_depend_on_its_batch_or_position():
    a, b = mc.pair("ragged")
    full = _table(a, b)
    assert np.array_equal(_bits(full), _bits(_table(a, b)))                                # two runs
    for r in range(a.shape[0]):
        assert np.array_equal(_bits(_table(a[r:r + 1], b[r:r + 1])[0]), _bits(full[r])), r   # alone
    perm = [2, 0, 1]
    assert np.array_equal(_bits(_table(a[perm], b[perm])), _bits(full[perm]))              # in another position
    # the pipeline's layout: channel pitch 4, logical C = 3 (a strided view) - the same bits
    pa = torch.zeros(a.shape[:3] + (4,), dtype=torch.uint8, device=DEV)
    pb = torch.full(a.shape[:3] + (4,), 9, dtype=torch.uint8, device=DEV)
    pa[..., :3], pb[..., :3] = _dev(a), _dev(b)
    assert np.array_equal(_bits(ops.image_metrics_u8(pa[..., :3], pb[..., :3]).cpu().numpy()), _bits(full))


def test_bad_shapes_raise_and_no_rows_give_an_empty_table():
    a = torch.zeros((1, 10, 16, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.FusgError, match="image_metrics_u8"):
        ops.image_metrics_u8(a, a)
    with pytest.raises(ValueError):
        ops.image_metrics_u8(a.float(), a.float())
    e = torch.zeros((0, 16, 16, 3), dtype=torch.uint8, device=DEV)
    assert tuple(ops.image_metrics_u8(e, e).shape) == (0, 6)


def test_recorded_pass_replays_the_metric_on_refreshed_inputs():
    """The launches go through plan_dispatch: recorded between fusg_plan_begin / _end (ops.PlanRecorder), they replay with
    fusg_plan_run on whatever the input buffers hold by then, into the recording's table."""
    lib = L.lib()
    a0, b0 = mc.pair("ragged")
    a1, b1 = mc.pair("border")
    a1, b1 = np.ascontiguousarray(a1[:, :37, :37]), np.ascontiguousarray(b1[:, :37, :37])   # two rows of another content
    buf_a, buf_b = _dev(a0[:2, :37]), _dev(b0[:2, :37])
    ex, ey = _edge_maps()
    buf_x, buf_y = _dev(ex), _dev(ey)                             # (every buffer a recorded launch points at lives until the destroy)
    rec = ops.PlanRecorder()
    try:
        L.check(lib.fusg_plan_begin(rec.handle), "plan_begin")
        ops.RECORDER = rec
        try:
            table = ops.image_metrics_u8(buf_a, buf_b)
            counts = ops.edge_counts(buf_x, buf_y, 0.5)
        finally:
            ops.RECORDER = None
            L.check(lib.fusg_plan_end(rec.handle), "plan_end")
        assert lib.fusg_plan_size(rec.handle) == 2
        first = table.cpu().numpy().copy()
        assert np.abs(first[:, 0] - ops.image_metrics_host(a0[:2, :37], b0[:2, :37])[:, 0]).max() <= 1e-12
        buf_a.copy_(_dev(a1))
        buf_b.copy_(_dev(b1))
        buf_x.copy_(_dev(ey))
        table.zero_()
        counts.zero_()
        L.check(lib.fusg_plan_run(rec.handle), "plan_run")
        torch.cuda.synchronize()
        want = ops.image_metrics_host(a1, b1)
        got = table.cpu().numpy()
        assert np.array_equal(got[:, 3:], want[:, 3:]) and np.abs(got[:, 0] - want[:, 0]).max() <= 1e-12
        assert not np.array_equal(got, first)
        assert np.array_equal(counts.cpu().numpy(), ops.edge_counts_host(ey, ey, 0.5))
    finally:
        torch.cuda.synchronize()
        lib.fusg_plan_destroy(rec.handle)


def _edge_maps():
    rng = np.random.default_rng(78)
    x = rng.random((3, 1, 67, 129)).astype(np.float32)            # 8643 elements per row: not a multiple of the workgroup
    y = rng.random((3, 1, 67, 129)).astype(np.float32)
    x[1], y[1] = x[1] * 0.4, y[1] * 0.4
    x[2, 0, :4], y[2, 0, 2:6] = 0.5, 0.5
    return x, y


def test_edge_counts_equal_the_host_twin():
    x, y = _edge_maps()
    for t in (0.5, 0.25):
        got = ops.edge_counts(_dev(x), _dev(y), t)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), ops.edge_counts_host(x, y, t))
    wide = torch.zeros((3, 3, 67, 129), dtype=torch.float32, device=DEV)
    wide[:, 1:2] = _dev(x)
    assert np.array_equal(ops.edge_counts(wide[:, 1:2], _dev(y)).cpu().numpy(), ops.edge_counts_host(x, y))
    assert tuple(ops.edge_counts(_dev(x[:0]), _dev(y[:0])).shape) == (0, 3)


@pytest.mark.parametrize("n", [1, 2048, 300001, 1300003])        # one workgroup / several / more elements than the grid's cap covers at once
def test_sq_diff_sum_is_the_float64_sum(n):
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    want = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum())
    got = [float(ops.sq_diff_sum(_dev(a), _dev(b)).cpu()) for _ in range(2)]
    assert got[0] == got[1]                                       # a fixed order
    assert abs(got[0] - want) <= 1e-12 * want                     # float64 sums of n <= 2^21 terms in two orders


def test_dropin_classes_on_device_equal_the_cpu_results():
    from future_urban_scene_generation_amd.edgeconnect.metrics import PSNR, EdgeAccuracy
    x, y = _edge_maps()
    for sl in (slice(0, 3), slice(1, 2)):                         # the general case; nothing relevant, nothing selected -> (1, 1)
        cp, cr = EdgeAccuracy(0.5)(torch.from_numpy(x[sl]), torch.from_numpy(y[sl]))
        gp, gr = EdgeAccuracy(0.5)(_dev(x[sl]), _dev(y[sl]))
        assert float(gp) == float(cp) and float(gr) == float(cr)
    assert int(gp) == 1 and int(gr) == 1
    a, b = mc.pair("ragged")
    ta, tb = torch.from_numpy(a.copy()), torch.from_numpy(b.copy())
    cpu = float(PSNR(255.)(ta, tb))
    assert float(PSNR(255.)(ta.to(DEV), tb.to(DEV))) == cpu                               # exact integers both ways
    assert float(PSNR(255.)(ta.permute(0, 3, 1, 2).contiguous().to(DEV), tb.permute(0, 3, 1, 2).contiguous().to(DEV))) == cpu
    assert int(PSNR(255.)(ta.to(DEV), ta.clone().to(DEV))) == 0
    fa, fb = torch.from_numpy(x), torch.from_numpy(y)
    cpu = float(PSNR(1.)(fa, fb))
    assert abs(float(PSNR(1.)(fa.to(DEV), fb.to(DEV))) - cpu) <= 2.0 ** -23 * abs(cpu)    # float32 of two float64 sums
    want = -10.0 * math.log10(((x.astype(np.float64) - y.astype(np.float64)) ** 2).mean())
    assert abs(cpu - want) <= 2.0 ** -23 * abs(want)


# ---- the pipeline layer ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe_batch():
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline, synth_batch
    return VehiclePipeline(DEV), synth_batch(2, 128, DEV)


def _counted(monkeypatch, pipe):
    """Count ops.d2h calls and keep what compare_outputs was handed."""
    seen = {"d2h": 0, "in_compare": 0, "args": None}
    real_d2h, real_cmp = ops.d2h, pipe.compare_outputs
    inside = [False]

    def d2h(t):
        seen["d2h"] += 1
        seen["in_compare"] += inside[0]
        return real_d2h(t)

    def compare_outputs(a, b):
        seen["args"] = (a, b)
        inside[0] = True
        try:
            return real_cmp(a, b)
        finally:
            inside[0] = False

    monkeypatch.setattr(ops, "d2h", d2h)
    monkeypatch.setattr(pipe, "compare_outputs", compare_outputs)
    return seen


def test_compare_precisions_of_one_precision_with_itself(pipe_batch, monkeypatch):
    pipe, batch = pipe_batch
    seen = _counted(monkeypatch, pipe)
    before = ops.PRECISION
    rep = pipe.compare_precisions(batch, [7, 8], precision="f16x3", against="f16x3")
    assert ops.PRECISION == before
    assert seen["d2h"] == 1 and seen["in_compare"] == 1
    for k in ("icn_u8", "vunet_u8"):
        assert rep[k]["ssim"].shape == (2,) and (rep[k]["ssim"] == 1.0).all() and (rep[k]["n_diff"] == 0).all()
        assert (rep[k]["max_abs"] == 0).all() and np.isposinf(rep[k]["psnr"]).all()
        assert rep["worst"][k]["ssim"] == 1.0 and rep["worst"][k]["max_abs"] == 0
    assert rep["kp_equal"].tolist() == [12, 12]
    assert "inpaint_u8" not in rep


def test_compare_precisions_bf16_reports_what_the_oracle_measures(pipe_batch, monkeypatch):
    """A consistency check, not a quality bar: the reported per-row SSIM of bf16 against f16x3 is oracle.ssim of the two
    crops, and `worst` names the true minimum."""
    import oracle
    pipe, batch = pipe_batch
    seen = _counted(monkeypatch, pipe)
    before = ops.PRECISION
    rep = pipe.compare_precisions(batch, [7, 8], "bf16")
    assert ops.PRECISION == before
    assert seen["d2h"] == 1 and seen["in_compare"] == 1
    out, ref = seen["args"]
    for k in ("icn_u8", "vunet_u8"):
        a, b = out[k].cpu().numpy(), ref[k].cpu().numpy()
        want = np.array([oracle.ssim(a[r], b[r]) for r in range(2)])
        print(k, "ssim bf16 vs f16x3", rep[k]["ssim"], "max_abs", rep[k]["max_abs"], "n_diff", rep[k]["n_diff"])
        record(f"{k}_ssim_bf16_vs_f16x3", rep[k]["ssim"].min(), worst=min)
        record(f"{k}_max_abs_bf16_vs_f16x3", rep[k]["max_abs"].max())
        assert np.abs(rep[k]["ssim"] - want).max() <= 1e-9
        mx, nd, _ = mc.numpy_integers(a, b)
        assert np.array_equal(rep[k]["max_abs"], mx) and np.array_equal(rep[k]["n_diff"], nd)
        w = rep["worst"][k]
        assert w["row"] == int(np.argmin(rep[k]["ssim"])) and w["ssim"] == rep[k]["ssim"].min() and w["max_abs"] == mx.max()
    assert rep["kp_equal"].tolist() == (out["kp_idx"] == ref["kp_idx"]).sum(dim=1).tolist()


def test_compare_precisions_refuses_before_any_launch(pipe_batch):
    pipe, batch = pipe_batch
    torch.cuda.synchronize()
    before, prec = ops.last_conv_kernel(), ops.PRECISION
    with pytest.raises(ValueError, match="vehicle_seeds"):
        pipe.compare_precisions(batch, None)
    with pytest.raises(ValueError, match="precision"):
        pipe.compare_precisions(batch, [7, 8], precision="fp8")
    assert ops.last_conv_kernel() == before and ops.PRECISION == prec


def test_compare_outputs_of_hand_made_dicts(pipe_batch):
    pipe, _ = pipe_batch
    a, b = mc.pair("product")
    a, b = np.ascontiguousarray(a[:, :128, :128]), np.ascontiguousarray(b[:, :128, :128])
    kp = torch.arange(24, dtype=torch.int32, device=DEV).reshape(2, 12)
    kp2 = kp.clone()
    kp2[1, :5] += 1
    rep = pipe.compare_outputs({"icn_u8": _dev(a), "vunet_u8": _dev(a), "kp_idx": kp, "extra": 1},
                               {"icn_u8": _dev(b), "vunet_u8": _dev(a), "kp_idx": kp2})
    want = ops.image_metrics_host(a, b)
    assert np.abs(rep["icn_u8"]["ssim"] - want[:, 0]).max() <= 1e-12 and np.array_equal(rep["icn_u8"]["n_diff"], want[:, 4].astype(np.int64))
    assert np.abs(rep["icn_u8"]["psnr"] - want[:, 2]).max() <= 1e-10
    assert (rep["vunet_u8"]["ssim"] == 1.0).all() and rep["kp_equal"].tolist() == [12, 7]
    assert rep["worst"]["icn_u8"]["row"] == int(np.argmin(want[:, 0])) and rep["worst"]["icn_u8"]["max_abs"] == 1
    assert set(rep) == {"icn_u8", "vunet_u8", "kp_equal", "worst"}
