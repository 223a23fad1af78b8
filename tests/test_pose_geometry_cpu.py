"""CPU: fusg_pose_geometry_host (csrc/pose_geometry.h, the code the device kernel runs) against the numpy chain the frame
driver runs between the pose fit and the render - select_and_flip, rotations, extrinsics_from_poses, plane_corners_batch,
visibility_inputs_batch, project_keypoints_batch, render_jobs (tests/pose_geometry_cases.py builds the cases and asserts the
precondition under which truncated integers can be compared exactly).  Integer outputs are equal; float outputs are within
8 x the largest difference measured over these cases (profiles/pose_geometry_parity.json, "host_vs_numpy"), the float32 pose
within 1 float32 ulp."""
import numpy as np
import pytest

import pose_geometry_cases as pc
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import render as R

# 8 x the measured maximum absolute difference per output (profiles/pose_geometry_parity.json: "host_vs_numpy" -> "bar_abs";
# tools/pose_geometry_parity.py measures it).  Everything but the moved keypoints came out equal bit for bit - the header takes
# numpy's operations in numpy's order and numpy's float64 cos / sin / arccos are libm's -, so their bar is 0: equality.
BAR_ABS = {"pose": 0.0, "extrinsic": 0.0, "kp3d": 8 * 2.220446049250313e-16, "job.R": 0.0, "job.tr": 0.0, "job.E": 0.0, "job.fx": 0.0,
           "job.fy": 0.0, "job.cx": 0.0, "job.cy": 0.0}
CASES = pc.cases()


@pytest.fixture(scope="module")
def results():
    """(reference, host twin) per case, computed once."""
    return {name: (pc.reference(c), pc.host(c)) for name, c in CASES.items()}


def _compare(name, ref, got):
    rows = ref["valid"]
    for k in pc.INT_KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k][rows], ref[k]), (name, k)
    for k in pc.JOB_INT:
        assert np.array_equal(got["jobs"][k][rows], ref["jobs"][k]), (name, "jobs." + k)
    fg, fr = pc.float_outputs(got, rows), pc.float_outputs(ref)
    assert pc.ulp32(fg["pose"], fr["pose"]) <= 1, (name, "pose ulp")
    for k in fg:
        ad, rel = pc.diffs(fg[k], fr[k])
        print(f"{name}: {k}: max abs {ad:.3g} rel {rel:.3g} (bar {BAR_ABS[k]:.3g})")
        assert ad <= BAR_ABS[k], (name, k, ad)


@pytest.mark.parametrize("name", ["ordinary", "later", "v1"])
def test_matches_numpy_chain(results, name):
    ref, got = results[name]
    assert len(ref["valid"]) == len(CASES[name]["cad_idx"]) == {"ordinary": 5, "later": 3, "v1": 1}[name]
    assert (got["status"] == 0).all()
    if name == "later":
        assert (CASES[name]["steps"][:, 0] != 0).all() and np.abs(CASES[name]["steps"][:, 1:]).sum(1).all()
        assert not np.array_equal(got["kp3d"], pc.bank().kp3d[CASES[name]["cad_idx"]])
    _compare(name, ref, got)


def test_tied_errors_first_wins(results):
    c = CASES["tied"]
    ref, got = results["tied"]
    _compare("tied", ref, got)
    # vehicle 0: starts 1 and 3 tie for the minimum; vehicle 1: all four tie
    for v, first in ((0, 1), (1, 0)):
        want = (c["raw"][1][v, first] * np.sign(c["raw"][1][v, first, 2])).astype(np.float32)
        assert np.array_equal(got["pose"][v, 4:7], want), v
        assert not np.array_equal(c["raw"][1][v, first], c["raw"][1][v, 3])


def test_nan_error_wins(results):
    c = CASES["nan_error"]
    ref, got = results["nan_error"]
    _compare("nan_error", ref, got)
    assert np.isnan(got["pose"][:, 0]).all()
    for v, idx in ((0, 2), (1, 1)):                         # start 2; of two NaNs (1 and 2) the first
        assert np.array_equal(np.abs(got["pose"][v, 4:7]), np.abs(c["raw"][1][v, idx])), v


def test_sign_flip_branches(results):
    c = CASES["flip"]
    ref, got = results["flip"]
    assert [pc.branch_of(c, v) for v in range(4)] == ["general", "pi", "pi", "zero"]
    assert (c["raw"][1][:3, 0, 2] < 0).all() and c["raw"][1][3, 0, 2] > 0
    assert not c["raw"][0][2, 0].any() and not c["raw"][0][3, 0].any()          # zero rvecs: the identity branch of rodrigues
    _compare("flip", ref, got)
    assert (got["pose"][:3, 6] > 0).all()                                        # flipped in front of the camera
    assert np.allclose(np.linalg.norm(got["pose"][1:3, 1:4], axis=1), np.pi, atol=1e-6)
    assert not got["pose"][3, 1:4].any()


def test_tz_zero_gives_sign_zero(results):
    c = CASES["tz_zero"]
    ref, got = results["tz_zero"]
    assert c["raw"][1][0, 1, 2] == 0 and int(np.argmin(c["raw"][2][0])) == 1
    _compare("tz_zero", ref, got)
    assert not got["pose"][0, 4:7].any() and got["pose"][1, 4:7].all()


def test_cad_idx_out_of_range(results):
    c = CASES["bad_cad"]
    ref, got = results["bad_cad"]
    assert c["cad_idx"].tolist() == [1, len(pc.bank()), -1] and ref["valid"].tolist() == [0]
    assert got["status"].tolist() == [0, 1, 1]
    for k in pc.JOB_INT:
        assert not got["jobs"][k][1:].any(), k                                   # an empty job: nt == 0 (and nv == 0)
    assert not got["kp3d"][1:].any()
    _compare("bad_cad", ref, got)
    # the pose does not depend on the bank: the flagged vehicles' equals the chain's on the same fit
    from future_urban_scene_generation_amd.utils.pnp_utils import select_and_flip
    for v in (1, 2):
        e, r, t = select_and_flip(*(a[v] for a in c["raw"]))
        assert np.array_equal(got["pose"][v], np.concatenate([[e], r.ravel(), t.ravel()]).astype(np.float32)), v


def test_no_vehicles(results):
    ref, got = results["v0"]
    for k in pc.INT_KEYS + ("pose", "extrinsic", "kp3d", "status"):
        assert got[k].shape[0] == 0, k
    assert got["jobs"].shape == (0,)
    _compare("v0", ref, got)


def test_refused_arguments():
    lib = L.lib()
    assert "fusg_pose_geometry" in L.EXPORTS and "fusg_pose_geometry_host" in L.EXPORTS and lib.fusg_version() == 118
    assert R.JOB_DTYPE.itemsize == lib.fusg_sizeof_render_job()
    c = CASES["v1"]
    b = pc.bank()
    rv, tv, er = (np.ascontiguousarray(a) for a in c["raw"])
    kp, cad = np.ascontiguousarray(c["kp_xy"]), c["cad_idx"]
    pose, steps = np.zeros((1, 7), np.float32), np.zeros((1, 4))
    tabs = [np.ascontiguousarray(b.kp3d), b.v_off.astype(np.int32), b.t_off.astype(np.int32)]
    K = np.ascontiguousarray(c["K"].reshape(9))
    outs = [np.zeros(n, dt) for dt, n in ((np.float32, 7), (np.float64, 12), (np.float64, 36), (np.uint8, 240), (np.int32, 112),
                                          (np.int32, 7), (np.int32, 7), (np.int32, 80), (np.int32, 5), (np.int32, 1))]
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731

    def call(ins=(rv, tv, er, None, kp, None), cad_=cad, tabs_=tabs, n_cad=len(b), K_=K, hw=(pc.H, pc.W), V=1, outs_=outs, fn=None):
        fn = fn or lib.fusg_pose_geometry_host
        return fn(*(p(a) for a in ins), p(cad_), *(p(a) for a in tabs_), n_cad, p(K_), hw[0], hw[1], V, *(p(a) for a in outs_))

    assert call() == 0
    bad = [dict(ins=(None, tv, er, None, kp, None)), dict(ins=(rv, tv, er, None, None, None)),           # a first frame lacks a part
           dict(ins=(rv, tv, er, pose, kp, None)), dict(ins=(rv, tv, er, None, kp, steps)),              # both forms at once
           dict(ins=(None, None, None, pose, None, None)), dict(ins=(None, None, None, None, None, steps)),
           dict(ins=(None,) * 6), dict(cad_=None), dict(tabs_=[None] + tabs[1:]), dict(tabs_=tabs[:2] + [None]),
           dict(n_cad=0), dict(K_=None), dict(hw=(0, pc.W)), dict(hw=(pc.H, -1)), dict(V=-1)]
    bad += [dict(outs_=outs[:i] + [None] + outs[i + 1:]) for i in range(len(outs))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"pose_geometry_host" in lib.fusg_last_error(), kw
    assert call(ins=(None, None, None, pose, None, steps)) == 0
    # the device entry point refuses the same arguments on the host, before any launch (no GPU is touched)
    dev = lambda *a: lib.fusg_pose_geometry(*a, None)       # noqa: E731
    for kw in (bad[0], bad[2], bad[7], bad[10], bad[11], bad[-1]):
        assert call(fn=dev, **kw) == -1, kw
        assert b"pose_geometry" in lib.fusg_last_error()
    assert call(fn=dev, V=0) == 0                            # V = 0: nothing is launched
    assert call(V=0, ins=(None,) * 6) == 0
