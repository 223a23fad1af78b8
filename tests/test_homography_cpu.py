"""CPU: the homography solver of csrc/homography.h through its host twins (fusg_find_homography_host,
fusg_plane_homographies_host) against planes_utils.find_homography / warp_jobs_frame - the code the device kernel runs, so
that tests/test_gpu_homography.py only has to show the device equal to the twin."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO, record
from homography_cases import (FIXTURE_SOURCES, FIXTURE_STATUS, P, apply_h, frame_fixture, pixel_metric, solver_cases,
                              tables_from_jobs, warp_u8)
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd.warp_learn import planes_utils as pu
from oracle import cv_host

# 10 x the worst value observed (1.94e-8 px, profiles/homography_parity.json: a hexagon fit, whose Levenberg-Marquardt loop
# ends on steps accepted or rejected by the rounding of the cost; the 4-point fits agree to 2e-11 px).  The warp quantises
# coordinates to 1/32 px.
BAR_PX = 2e-7
assert BAR_PX < 1e-6


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def test_exports_and_host_validation(lib):
    for name in ("fusg_plane_homographies", "fusg_plane_homographies_host", "fusg_find_homography_host"):
        assert name in L.EXPORTS and hasattr(lib, name)
    buf = (L.C.c_int32 * 64)()
    f = lib.fusg_plane_homographies
    assert f(None, buf, buf, buf, buf, 1, 5, 0, 1, buf, buf, None, None, None) == -1        # null input
    assert f(buf, buf, buf, buf, buf, 1, 9, 0, 1, buf, buf, None, None, None) == -1         # more than 8 planes
    assert f(buf, buf, buf, buf, buf, -1, 5, 0, 1, buf, buf, None, None, None) == -1        # negative vehicle count
    assert f(buf, buf, buf, buf, buf, 1, 5, 0, 0, buf, buf, None, None, None) == -1         # the symmetric pair is one plane
    assert f(buf, buf, buf, buf, buf, 1, 5, 0, 5, buf, buf, None, None, None) == -1         # ... or out of range
    assert b"symmetric" in lib.fusg_last_error()
    assert f(buf, buf, buf, buf, buf, 0, 5, 0, 1, buf, buf, None, None, None) == 0          # no vehicle: nothing launched


def test_host_twin_matches_find_homography(lib):
    """Every seeded problem: twin and numpy map the point set and the corners of a 720 x 1280 frame to the same place."""
    seen = {}
    for name, s, d in solver_cases():
        for a, b in ((s, d), (d, s)):                                          # H12 and H21, as warp_jobs fits them
            ref, got = pu.find_homography(a, b), pu.find_homography_host(a, b)
            assert ref is not None and got is not None, name
            m = pixel_metric(ref, got, a)
            seen[name] = max(seen.get(name, 0.0), m)
            record("homography_twin_vs_numpy_px", m)
    worst = max(seen.values())
    print("worst px:", worst, seen)
    with open(os.path.join(REPO, "profiles", "homography_parity.json"), "w") as f:
        json.dump({"metric": "max distance in px between H_numpy x and H_twin x over the points and the corners of a 720 x 1280 frame",
                   "worst_px": worst, "bar_px": BAR_PX, "cases": seen}, f, indent=1, sort_keys=True)
        f.write("\n")
    assert worst <= BAR_PX, seen


def test_lm_rejects_a_step_on_the_hexagons(monkeypatch):
    """The 6-point cases are not exactly projective, and planes_utils' own loop rejects at least one step on each of them: a
    rejected step leaves the parameters alone, so the next system has the same off-diagonal entries (only lambda moved)."""
    systems = []
    solve = np.linalg.solve
    monkeypatch.setattr(np.linalg, "solve", lambda A, b: (systems.append(A.copy()), solve(A, b))[1])
    off = ~np.eye(8, dtype=bool)
    hexagons = [(n, s, d) for n, s, d in solver_cases() if len(s) == 6]
    assert len(hexagons) >= 3
    for name, s, d in hexagons:
        systems.clear()
        H = pu.find_homography(s, d)
        r = np.abs(apply_h(H, s) - d).max()
        assert 1e-3 < r < 2.0, (name, r)                                        # a real residual remains
        assert any(np.array_equal(a[off], b[off]) for a, b in zip(systems, systems[1:])), name


def test_invalid_fits_match_numpy(lib):
    sq = np.int32([[0, 0], [10, 0], [10, 10], [0, 10]])
    bad = [("collinear source", np.int32([[0, 0], [5, 5], [10, 10], [15, 15]]), sq),
           ("collinear destination", sq, np.int32([[0, 0], [5, 5], [10, 10], [15, 15]])),
           ("zero deviation in x", np.int32([[3, 0], [3, 4], [3, 9], [3, 12]]), sq),
           ("repeated point: zero deviation", np.int32([[7, 7]] * 4), sq),
           ("three points", sq[:3], sq[:3])]
    for name, s, d in bad:
        assert pu.find_homography(s, d) is None, name
        assert pu.find_homography_host(s, d) is None, name
    assert pu.find_homography_host(sq, sq[:3]) is None                          # unequal lengths
    H = pu.find_homography_host(sq, sq * 3 + 2)
    assert H is not None and np.abs(H - np.float64([[3, 0, 2], [0, 3, 2], [0, 0, 1]])).max() < 1e-12


def _host_tables(fx):
    return pu.plane_homographies_host(fx["src_kp"], fx["dst_kp"], fx["src_vis"], fx["dst_vis"])


def test_gating_and_slot_table(lib):
    """The table of (vehicle, slot) rows against the jobs of warp_jobs_frame, on visibilities that take every branch of the
    gate (homography_cases.frame_fixture), and against the table written down by hand."""
    fx = frame_fixture()
    V = len(fx["src_kp"])
    jobs = pu.warp_jobs_frame(fx["src_kp"], fx["dst_kp"], fx["src_vis"], fx["dst_vis"])
    ref_index, ref_minv = tables_from_jobs(jobs, V)
    minv, index, H, status = _host_tables(fx)
    assert np.array_equal(index, ref_index) and ref_minv.shape == minv.shape
    src = np.where(index[:, 0] >= 0, index[:, 0] - np.arange(V * P) // P * P, -1).reshape(V, P)
    assert np.array_equal(src, FIXTURE_SOURCES) and np.array_equal(status, FIXTURE_STATUS)
    assert np.array_equal(index[:, 1], np.arange(V * P))
    none = index[:, 0] < 0
    assert not minv[none].any() and not H.reshape(V * P, -1)[none].any()
    for v, jb in enumerate(jobs):                                              # the matrices of the winning jobs
        for i, j, H12, H21 in jb:
            if index[v * P + j, 0] != v * P + i:
                continue
            # (hexagons of 30 px radius with whole-pixel corners: the refinement's own rounding noise is ~1e-6 px here; the
            # solver's parity bar is set on test_host_twin_matches_find_homography's problems, the bytes of this fixture in
            # test_fixture_is_free_of_rounding_ties - this only says "the same job's matrices", at 1/30 of the warp's 1/32 px)
            assert pixel_metric(H12, H[v, j, 0], fx["src_kp"][v][i], fx["hw"]) <= 1e-3
            assert pixel_metric(H21, H[v, j, 1], fx["dst_kp"][v][j], fx["hw"]) <= 1e-3
            assert np.abs(H[v, j, 0] @ minv[v * P + j].reshape(3, 3) - np.eye(3)).max() < 1e-9
    # every vehicle alone gives its own rows (no state leaks between vehicles); no vehicle gives empty tables
    for v in range(V):
        one = pu.plane_homographies_host([fx["src_kp"][v]], [fx["dst_kp"][v]], fx["src_vis"][v:v + 1], fx["dst_vis"][v:v + 1])
        assert np.array_equal(one[0], minv[v * P:(v + 1) * P]) and np.array_equal(one[2][0], H[v])
    empty = pu.plane_homographies_host([], [], np.zeros((0, P), np.uint8), np.zeros((0, P), np.uint8))
    assert empty[0].shape == (0, 9) and empty[1].shape == (0, 2)


def test_swapped_plane_lands_when_its_partner_is_not_a_source(lib):
    """left -> right with the right plane hidden in the source: the swapped plane is the only job of slot 1; and the mirror."""
    fx = frame_fixture()
    for sv, dv, want in (([1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [-1, 0, -1, -1, -1]), ([0, 1, 0, 0, 0], [1, 0, 0, 0, 0], [1, -1, -1, -1, -1]),
                         ([0, 0, 1, 1, 1], [1, 1, 0, 0, 0], [-1] * 5), ([0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [-1] * 5)):
        sv, dv = np.uint8([sv]), np.uint8([dv])
        _, index, _, _ = pu.plane_homographies_host(fx["src_kp"][:1], fx["dst_kp"][:1], sv, dv)
        ref, _ = tables_from_jobs(pu.warp_jobs_frame(fx["src_kp"][:1], fx["dst_kp"][:1], sv, dv), 1)
        assert np.array_equal(index, ref) and index[:, 0].tolist() == want


def test_fixture_is_free_of_rounding_ties(lib):
    """The frame the GPU warp test uses: warpPerspective (oracle.cv_host's restatement) gives identical bytes with the twin's
    inverse matrices and with numpy's, so the byte equality asserted on the GPU does not hang on a rounding tie."""
    fx = frame_fixture()
    V = len(fx["src_kp"])
    ref_index, ref_minv = tables_from_jobs(pu.warp_jobs_frame(fx["src_kp"], fx["dst_kp"], fx["src_vis"], fx["dst_vis"]), V)
    minv, index, _, _ = _host_tables(fx)
    flat = fx["planes"].reshape((V * P,) + fx["planes"].shape[2:])
    jobs = 0
    for r in range(V * P):
        if index[r, 0] < 0:
            continue
        a, b = warp_u8(flat[index[r, 0]], ref_minv[r], cv_host), warp_u8(flat[index[r, 0]], minv[r], cv_host)
        assert np.array_equal(a, b), r
        assert a.any()                                                          # the job does put pixels into the frame
        jobs += 1
    assert jobs == 6


def test_frame_test_scene_is_free_of_rounding_ties(lib, monkeypatch):
    """The scene tests/test_gpu_homography.py runs through run_frame / run_later_frame (synth_frame seed 41, 2 vehicles, and
    its later pose): for every job the two inverse matrices address the same source cell with the same 1/32-px weights at
    every destination pixel whose source lies in the frame."""
    from future_urban_scene_generation_amd import pipeline as pl
    monkeypatch.setattr(pu, "fill_planes", lambda frame, polys: torch.zeros(1))      # the planes' pixels are not needed here
    hw = (360, 640)
    first = pl.synth_frame(2, hw, "cpu", seed=41)
    g = np.random.default_rng(9)
    later = dict(first)
    later["dst_kp"] = [[np.int32(p + np.array([-7, 5]) + g.integers(-2, 3, p.shape)) for p in veh] for veh in first["dst_kp"]]
    for sc in (first, later):
        ref_index, ref_minv = tables_from_jobs(pu.warp_jobs_frame(sc["src_kp"], sc["dst_kp"], sc["src_vis"], sc["dst_vis"]), 2)
        minv, index, _, _ = pu.plane_homographies_host(sc["src_kp"], sc["dst_kp"], sc["src_vis"], sc["dst_vis"])
        assert np.array_equal(index, ref_index) and (index[:, 0] >= 0).sum() >= 4
        for r in np.nonzero(index[:, 0] >= 0)[0]:
            a = cv_host.perspective_coords(ref_minv[r].reshape(3, 3), hw[1], hw[0])
            b = cv_host.perspective_coords(minv[r].reshape(3, 3), hw[1], hw[0])
            inside = (a[0] >= -1) & (a[0] < hw[1]) & (a[1] >= -1) & (a[1] < hw[0])
            assert all(np.array_equal(x[inside], y[inside]) for x, y in zip(a, b)), r
