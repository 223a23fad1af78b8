#!/usr/bin/env python
"""tests/golden/trajectories_to_meters.npz from the reference's own `utils.gps_utils.trajectories_to_meters` and
`utils.bounding_box.BoundingBox`: a few small tracker tables, an inverse homography, both box scales the reference is run with
(1.0 and 1.2), and what the reference makes of them - the metres of every track and the box (x0, y0, x1, y1) and lower-edge
midpoint of every row.  Runs only where a reference checkout exists (FUSG_REFERENCE, as for gen_golden.py); `cv2` is a stub of
our own with the one call needed, convertPointsToHomogeneous.  Only the data file is kept."""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FUSG_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

cv2 = types.ModuleType("cv2")
cv2.convertPointsToHomogeneous = lambda p: np.concatenate([np.asarray(p, np.float64), np.ones((len(p), 1))], axis=1)[:, None, :]
sys.modules["cv2"] = cv2

from utils.bounding_box import BoundingBox                           # noqa: E402  (reference)
from utils.gps_utils import trajectories_to_meters                   # noqa: E402  (reference)

SHAPE, IMG_SCALE, SCALES = (640, 360), 0.5, (1.0, 1.2)


def tracks():
    """[n, 6] = (frame, id, x, y, w, h) in the tracker's pixels (twice the image's: img_scale 0.5), fractions included."""
    rng = np.random.default_rng(225)
    out = []
    for i, (x, y, vx, vy, n) in enumerate(((100.0, 200.0, 22.5, 6.25, 6), (900.0, 420.0, -31.0, -9.5, 6), (1180.0, 640.0, 14.0, 11.0, 4),
                                           (-9.0, 30.0, 17.0, 3.0, 5), (400.0, 300.0, 0.0, 12.0, 3))):
        f = np.arange(n, dtype=np.float64)
        w, h = 90.0 + 7.0 * f + rng.integers(0, 5, n), 61.0 + 3.0 * f + rng.integers(0, 5, n)
        out.append(np.stack([10 + 2 * f, np.full(n, 7.0 + i), x + vx * f + rng.random(n), y + vy * f + rng.random(n), w, h], axis=1))
    out.append(np.stack([np.arange(3.0), np.full(3, 20.0), np.full(3, 333.0), np.full(3, 222.0), np.full(3, 80.0), np.full(3, 50.0)], axis=1))   # stands
    return out


def main():
    inv_h = np.asarray([[2.1e-6, -4.0e-7, 42.49], [3.0e-7, 2.9e-6, -90.67], [1.0e-6, 2.0e-6, 1.0]])
    tr = tracks()
    data = {"rows": np.concatenate(tr), "offsets": np.cumsum([0] + [len(t) for t in tr]), "inv_homography": inv_h,
            "shape": np.asarray(SHAPE), "img_scale": np.asarray(IMG_SCALE), "scales": np.asarray(SCALES)}
    for k, scale in enumerate(SCALES):
        with np.errstate(all="ignore"):
            data[f"meters_{k}"] = np.concatenate([trajectories_to_meters(t, inv_h, scale, SHAPE, IMG_SCALE) for t in tr])
        bb = [BoundingBox(*r[2:6] * IMG_SCALE, bounds=(0, SHAPE[0] - 1, 0, SHAPE[1] - 1), scale=scale) for t in tr for r in t]
        data[f"boxes_{k}"] = np.asarray([b.xyxy for b in bb], dtype=np.int64)
        data[f"mid_bottom_{k}"] = np.asarray([b.mid_bottom for b in bb], dtype=np.int64)
    path = os.path.join(REPO, "tests", "golden", "trajectories_to_meters.npz")
    np.savez(path, **data)
    print(path, {k: v.shape for k, v in data.items()})


if __name__ == "__main__":
    main()
