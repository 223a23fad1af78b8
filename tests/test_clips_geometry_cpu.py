"""CPU: fusg_pose_geometry_clips_host (csrc/pose_geometry.h `clips_row`: the later-frame branch of fusg_pose_geometry for rows of
several clips, each with its own pose table, CAD indices, source corner points and camera) against fusg_pose_geometry_host run
clip by clip on the repeated rows - equal with np.array_equal, dtypes included: it is the same per-vehicle code -, the arguments it
refuses, and the pure-Python validation of `run_later_clips_batched_geometry` (`pipeline.later_clips_geometry_batch_rows`)."""
import ctypes as C

import numpy as np
import pytest

import pose_geometry_cases as pc
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import pipeline as P
from future_urban_scene_generation_amd import render as R

LATER = pc.cases()["later"]                                  # the later-frame case: 3 vehicles with pose, steps, cad_idx and K
K2 = LATER["K"].copy()                                        # a second camera: focals scaled by a few per cent, centers shifted
K2[0, 0] *= 1.03
K2[1, 1] *= 0.98
K2[0, 2] += 4.0
K2[1, 2] -= 3.0
OUT_KEYS = ("pose", "extrinsic", "kp3d", "jobs", "vis_pts", "vis_nv", "nearer", "tex_pts", "tex_nv", "status")
PER = {"pose": (np.float32, 7), "extrinsic": (np.float64, 12), "kp3d": (np.float64, 36), "jobs": (np.uint8, 240), "vis_pts": (np.int32, 112),
       "vis_nv": (np.int32, 7), "nearer": (np.int32, 7), "tex_pts": (np.int32, 80), "tex_nv": (np.int32, 5), "status": (np.int32, 1),
       "src_pts_rows": (np.int32, 80)}


def make_clips(shapes, seed=0):
    """Clips of (F, V) from the later-frame case: vehicle v of clip c is the case's vehicle (c + v) % 3, frame f scales its step's
    translation by (1 + 0.07 f) - the angles stay the case's, on which the device's cos / sin are known to give the host's bits
    (tests/test_gpu_pose_geometry.py) -; odd clips use the second camera; random source corner points."""
    g = np.random.default_rng(seed)
    clips = []
    for c, (F, V) in enumerate(shapes):
        idx = [(c + v) % 3 for v in range(V)]
        far = lambda f: np.array([1.0, 1 + 0.07 * f, 1 + 0.07 * f, 1 + 0.07 * f])          # noqa: E731
        steps = np.concatenate([LATER["steps"][idx] * far(f) for f in range(F)]) if F * V else np.zeros((0, 4))
        clips.append({"pose": LATER["pose"][idx].reshape(V, 7), "cad_idx": LATER["cad_idx"][idx].reshape(V),
                      "src_pts": g.integers(-50, 1300, (V, 5, 8, 2)).astype(np.int32), "K": K2 if c % 2 else LATER["K"], "steps": steps,
                      "F": F})
    return clips


def per_clip(clips):
    """fusg_pose_geometry_host per clip with that clip's K on the repeated rows, concatenated in row order."""
    parts, pts = [], []
    for cl in clips:
        F, V = cl["F"], len(cl["cad_idx"])
        if F * V:
            parts.append(R.pose_geometry_host(pc.bank(), np.tile(cl["cad_idx"], F), cl["K"], (pc.H, pc.W), pose=np.tile(cl["pose"], (F, 1)),
                                              steps=cl["steps"]))
            pts.append(np.tile(cl["src_pts"], (F, 1, 1, 1)))
    out = {k: np.concatenate([p[k] for p in parts]) for k in OUT_KEYS}
    out["src_pts_rows"] = np.concatenate(pts)
    return out


def same(got, want):
    for k in OUT_KEYS + ("src_pts_rows",):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k


@pytest.mark.parametrize("shapes", [[(2, 2), (1, 3), (3, 1), (0, 2), (2, 0)], [(64, 1)], [(1, 1)] * 64, [(0, 3), (2, 0), (4, 3)]],
                         ids=["ragged", "one_clip_64_rows", "64_clips_of_one_row", "empty_clips_first"])
def test_host_twin_equals_per_clip_host(shapes):
    clips = make_clips(shapes)
    got = R.pose_geometry_clips_host(pc.bank(), (pc.H, pc.W), clips)
    want = per_clip(clips)
    assert got["pose"].shape[0] == sum(f * v for f, v in shapes)
    same(got, want)
    assert (got["status"] == 0).all() and got["jobs"]["nt"].all()
    if len(shapes) > 1 and len({id(cl["K"]) for cl in clips if cl["F"] * len(cl["cad_idx"])}) > 1:
        assert len({float(x) for x in got["jobs"]["fx"]}) == 2           # both cameras are in use


def test_bad_cad_index_is_flagged_per_row():
    clips = make_clips([(2, 2), (1, 1)])
    clips[0]["cad_idx"] = np.array([1, len(pc.bank())], np.int64)
    got = R.pose_geometry_clips_host(pc.bank(), (pc.H, pc.W), clips)
    assert got["status"].tolist() == [0, 1, 0, 1, 0]
    same(got, per_clip(clips))


def _raw_call(fn, clips, guard=1, **over):
    """The entry point `fn` on host arrays with `guard` extra rows (filled with 0x5A) behind each output; over: arguments replaced.
    Returns (rc, outputs as uint8 arrays, J)."""
    b = pc.bank()
    n = len(clips)
    keep = {"pose": [np.ascontiguousarray(cl["pose"], np.float32) for cl in clips],
            "cad": [np.ascontiguousarray(cl["cad_idx"], np.int64) for cl in clips],
            "pts": [np.ascontiguousarray(cl["src_pts"], np.int32) for cl in clips]}
    first = [0]
    for cl in clips:
        first.append(first[-1] + cl["steps"].shape[0])
    J = over.get("J", first[-1])
    tab = lambda arrs: (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])     # noqa: E731
    a = {"poses": tab(keep["pose"]), "cads": tab(keep["cad"]), "pts": tab(keep["pts"]),
         "vehicles": (C.c_int32 * max(n, 1))(*[len(x) for x in keep["cad"]]), "row_first": (C.c_int32 * (n + 1))(*first), "n_clips": n,
         "steps": np.ascontiguousarray(np.concatenate([cl["steps"] for cl in clips])),
         "cams": np.ascontiguousarray(np.concatenate([np.asarray(cl["K"], np.float64).reshape(9) for cl in clips])),
         "kp3d": np.ascontiguousarray(b.kp3d, dtype=np.float32), "v_off": b.v_off.astype(np.int32), "t_off": b.t_off.astype(np.int32),
         "n_cad": len(b), "H": pc.H, "W": pc.W, "J": J}
    a.update(over)
    rows = max(first[-1], 0) + guard
    outs = {k: np.full(rows * per * np.dtype(dt).itemsize, 0x5A, np.uint8) for k, (dt, per) in PER.items()}
    p = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x)           # noqa: E731
    names = OUT_KEYS + ("src_pts_rows",)
    out_ptrs = [None if over.get("null_out") == k else outs[k].ctypes.data for k in names]
    rc = fn(a["poses"], a["cads"], a["pts"], a["vehicles"], a["row_first"], a["n_clips"], p(a["steps"]), p(a["cams"]), p(a["kp3d"]),
            p(a["v_off"]), p(a["t_off"]), a["n_cad"], a["H"], a["W"], a["J"], *out_ptrs)
    return rc, outs, first[-1]


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def test_refused_arguments_write_nothing():
    lib = L.lib()
    assert lib.fusg_version() == 118 and L.MAX_FRAMES == 64
    for name in ("fusg_pose_geometry_clips", "fusg_pose_geometry_clips_host"):
        assert name in L.EXPORTS and hasattr(lib, name), name
    clips = make_clips([(2, 2), (1, 3)])                          # 7 rows: offsets 0, 4, 7
    host = lib.fusg_pose_geometry_clips_host
    rc, outs, J = _raw_call(host, clips)
    assert rc == 0 and J == 7
    for k, (dt, per) in PER.items():                              # the guard row behind each output is untouched
        nb = per * np.dtype(dt).itemsize
        assert (outs[k][J * nb:] == 0x5A).all() and not (outs[k][:J * nb] == 0x5A).all(), k
    null_first = (C.c_void_p * 2)(None, 1)
    bad = [dict(poses=null_first), dict(cads=null_first), dict(pts=null_first),          # a null table entry of a clip that owns rows
           dict(poses=None), dict(vehicles=None), dict(row_first=None),
           dict(row_first=_i32(0, 5, 4)), dict(row_first=_i32(1, 4, 7)),                 # not monotone; not from 0
           dict(row_first=_i32(0, 4, 6)), dict(row_first=_i32(0, 4, 8)),                 # do not end at J
           dict(row_first=_i32(0, 3, 7)), dict(row_first=_i32(0, 4, 6), J=6),            # no multiple of V_c (clip 0; clip 1)
           dict(vehicles=_i32(0, 3)), dict(vehicles=_i32(2, -1)),                        # rows for a clip without vehicles
           dict(n_clips=0), dict(n_clips=65), dict(J=-1), dict(J=1 << 20),
           dict(steps=None), dict(cams=None), dict(kp3d=None), dict(v_off=None), dict(t_off=None), dict(n_cad=0), dict(H=0), dict(W=-2)]
    bad += [dict(null_out=k) for k in OUT_KEYS + ("src_pts_rows",)]
    dev = lambda *a: lib.fusg_pose_geometry_clips(*a, None)       # noqa: E731  (refused on the host, before any launch)
    for kw in bad:
        for fn, what in ((host, b"pose_geometry_clips_host"), (dev, b"pose_geometry_clips")):
            rc, outs, _ = _raw_call(fn, clips, **kw)
            assert rc == -1, kw
            assert what in lib.fusg_last_error(), kw
            for k in outs:
                assert (outs[k] == 0x5A).all(), (kw, k)
    # J == 0: nothing to do, on either entry point (no GPU is touched), null device pointers included
    empty = make_clips([(0, 2), (3, 0)])
    for fn in (host, dev):
        rc, outs, J = _raw_call(fn, empty, steps=None, cams=None)
        assert rc == 0 and J == 0 and all((o == 0x5A).all() for o in outs.values())
    # a clip without rows may pass null tables
    rc, _, _ = _raw_call(host, make_clips([(0, 2), (1, 1)]), poses=(C.c_void_p * 2)(None, np.ascontiguousarray(LATER["pose"][1:2]).ctypes.data))
    assert rc == 0


# ---- the pure-Python validation of the driver
class _T:
    def __init__(self, shape):
        self.shape = shape


def _clip(F, veh, n_first=None, seeds=True, inpaint=False, hw=(360, 640), geometry=True):
    n_first = (max(veh) + 1 if veh else 1) if n_first is None else n_first
    scs = []
    for f in range(F):
        sc = {"frame": _T(hw + (3,)), "steps": [(0.0, np.zeros(3))] * n_first}
        if seeds:
            sc["vehicle_seeds"] = [100 * f + v for v in range(n_first)]
        if inpaint:
            sc["inpaint"] = {"boxes": np.zeros((n_first, 4), np.int32), "det_masks": None}
        scs.append(sc)
    return scs, {"geometry": {"vehicles": list(veh)} if geometry else None}


def test_validation_helper():
    f = P.later_clips_geometry_batch_rows
    clips = [_clip(2, [0, 2]), _clip(1, [1, 2, 3]), _clip(3, [0]), _clip(0, [0, 1]), _clip(2, [])]
    veh, seeds, has = f(clips, True, True, False)
    assert veh == [2, 3, 1, 2, 0] and has is False
    want = P.clip_batch_seeds([[[sc["vehicle_seeds"][v] for v in st["geometry"]["vehicles"]] for sc in scs] for scs, st in clips], veh)
    assert seeds == want and len(seeds) == 10 and seeds[:4] == [0, 2, 100, 102]
    assert f([_clip(2, [0, 1], seeds=False)], True, True)[1] is None
    assert f(clips, True, True, True)[2] is False                 # the networks are there, no scene carries 'inpaint'
    assert f([_clip(2, [0, 1], inpaint=True), _clip(1, [], inpaint=False)], True, True, True)[2] is True
    assert f([_clip(2, [0, 1], inpaint=True)], True, True, False)[2] is False     # no inpainting networks: the key is ignored

    def refused(cl, msg, dp=True, dh=True, inpaint=False):
        with pytest.raises(ValueError, match=msg):
            f(cl, dp, dh, inpaint)

    refused(clips, "device_pose=True and device_homography=True", dp=False)
    refused(clips, "device_pose=True and device_homography=True", dh=False)
    c = _clip(2, [0, 1])
    c[0][1]["masks"] = object()
    refused([_clip(1, [0]), c], "clip 1 scene 1 is not a geometry-mode scene")
    c = _clip(2, [0, 1])
    del c[0][0]["steps"]
    refused([c], "clip 0 scene 0 is not a geometry-mode scene")
    refused([_clip(2, [0, 3], n_first=3)], "'steps' entries")
    c = _clip(2, [0, 3])
    c[0][1]["vehicle_seeds"] = [1, 2, 3]
    refused([c], "3 'vehicle_seeds' entries")
    c = _clip(2, [0, 1])
    del c[0][1]["vehicle_seeds"]
    refused([_clip(1, [0]), c], r"vehicle_seeds.*\[\(1, 1\)\]")
    c = _clip(2, [0, 1], inpaint=True)
    del c[0][0]["inpaint"]
    refused([c, _clip(1, [0], inpaint=True)], r"inpaint.*\[\(0, 0\)\]", inpaint=True)
    refused([_clip(1, [0]), _clip(1, [0], hw=(720, 1280))], "one size")
    refused([_clip(1, [0]), _clip(1, [0], geometry=False)], r"mixes geometry-mode clips and given-geometry clips \(given-geometry: \[1\]\)")
    # a clip without vehicles decides nothing about seeds or 'inpaint'
    assert f([_clip(1, [0]), _clip(2, [], seeds=False)], True, True)[1] == [0]
