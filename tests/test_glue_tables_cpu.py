"""The host halves of the frame glue that need neither the library nor a GPU: the ONE job table behind the three
`warp_planes_*_batch` forms (checked against index tables written out by hand) and the refusals of the several-frame paste
wrappers, which raise before anything is launched."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from future_urban_scene_generation_amd.warp_learn import planes_utils as pu   # noqa: E402

P = 5


def _H(k):
    return np.array([[1 + 0.1 * k, 0.02 * k, 3.0 * k], [0.01 * k, 1 - 0.05 * k, -2.0 * k], [1e-4 * k, 0.0, 1.0]])


H = [_H(k) for k in range(8)]
# five rows of (source plane i, destination slot j, H12, H21): row 0 writes slot 0 twice (the later job wins and keeps the slot's
# place in the order), row 1 has no job
ROWS = [[(0, 0, H[1], None), (1, 0, H[2], None), (3, 3, H[3], None)],
        [],
        [(2, 4, H[4], None)],
        [(4, 1, H[5], None)],
        [(0, 1, H[6], None), (1, 0, H[7], None)]]
KEPT = [H[2], H[3], H[4], H[5], H[6], H[7]]


def test_stack_starts_of_the_three_forms():
    # two clips of (F, V) = (2, 2) and (1, 1): rows f0v0 f0v1 f1v0 f1v1 | f0v0; clip 1's planes start at image 4 * P
    assert pu._stack_starts([(2, 2), (1, 1)], [0, 4, 5], P) == [0, 5, 0, 5, 20]
    assert pu._stack_starts([(2, 2)], [0], P) == [0, 5, 0, 5]                 # a clip's tail: F = 2 frames of V = 2
    assert pu._stack_starts([(1, 3)], [0], P) == [0, 5, 10]                   # a frame's V = 3 vehicles
    assert pu._stack_starts([(2, 0), (1, 2)], [0, 0, 2], P) == [0, 5]         # a clip without vehicles has no rows


@pytest.mark.parametrize("form, rows, src_first, index", [
    ("clips", 5, [0, 5, 0, 5, 20], [[1, 0], [3, 3], [2, 14], [9, 16], [20, 21], [21, 20]]),
    ("frames", 4, [0, 5, 0, 5], [[1, 0], [3, 3], [2, 14], [9, 16]]),
    ("one frame", 3, [0, 5, 10], [[1, 0], [3, 3], [12, 14]]),
])
def test_job_table_against_tables_written_by_hand(form, rows, src_first, index):
    minv, idx = pu._job_table_host(ROWS[:rows], P, src_first)
    assert idx.dtype == np.int32 and idx.tolist() == index
    kept = KEPT[:len(index)]
    assert minv.dtype == np.float64 and minv.shape == (len(index), 9)
    assert np.array_equal(minv, np.linalg.inv(np.stack(kept)).reshape(-1, 9))
    for m, h in zip(minv, kept):
        np.testing.assert_allclose(m.reshape(3, 3) @ h, np.eye(3), atol=1e-12)


def test_job_table_without_jobs():
    minv, idx = pu._job_table_host([[], []], P, [0, 5])
    assert minv.shape == (0, 9) and idx.shape == (0, 2) and idx.dtype == np.int32


def _paste_args(N=4, H_=6, W=10, R=4):
    z = lambda *sh: torch.zeros(sh, dtype=torch.uint8)                            # noqa: E731
    return dict(net_images=z(N, R, R, 3), geom=torch.zeros((N, 8), dtype=torch.int32), masks=z(N, H_, W))


def test_the_paste_wrappers_refuse_before_any_launch():
    z = lambda *sh: torch.zeros(sh, dtype=torch.uint8)                            # noqa: E731
    bases, a = [z(6, 10, 3), z(6, 10, 3)], _paste_args()
    box = z(4, 4, 4, 3)
    with pytest.raises(ValueError, match="paste_back_frames_device: at least one frame"):
        pu.paste_back_frames_device([], **a)
    with pytest.raises(ValueError, match=r"paste_back_frames_device: every base image is uint8 \(6, 10, 3\) on cpu"):
        pu.paste_back_frames_device([bases[0], bases[1].float()], **a)
    with pytest.raises(ValueError, match=r"paste_back_frames_device: every base image is uint8"):
        pu.paste_back_frames_device([bases[0], z(7, 10, 3)], **a)
    with pytest.raises(ValueError, match=r"paste_back_frames_device: 4 masks, 4 crops, geom \(4, 8\) for 3 frames"):
        pu.paste_back_frames_device(bases + bases[:1], **a)
    with pytest.raises(ValueError, match=r"paste_back_frames_device: 4 masks, 3 crops"):
        pu.paste_back_frames_device(bases, **dict(a, net_images=a["net_images"][:3]))
    with pytest.raises(ValueError, match=r"paste_back_frames_device: 4 masks, 4 crops, geom \(4, 8\) for 2 frames"):
        pu.paste_back_frames_device(bases, **dict(a, geom=a["geom"].long()))
    for bad in (dict(box_images=box), dict(box_geom=a["geom"]), dict(box_images=box[:3], box_geom=a["geom"]),
                dict(box_images=box, box_geom=a["geom"].long()), dict(box_images=box, box_geom=a["geom"][:, :4])):
        with pytest.raises(ValueError, match=r"paste_back_frames_device: box_images \[F \* V, h, w, 3\] come with box_geom int32 \[F \* V, 8\]"):
            pu.paste_back_frames_device(bases, **a, **bad)
        with pytest.raises(ValueError, match=r"paste_back_ragged_device: box_images \[rows, h, w, 3\] come with box_geom int32 \[rows, 8\]"):
            pu.paste_back_ragged_device(bases, [0, 1, 4], **a, **bad)
    with pytest.raises(ValueError, match=r"paste_back_ragged_device: 0 frames \(1\.\.64 per launch\)"):
        pu.paste_back_ragged_device([], [0], **a)
    with pytest.raises(ValueError, match=r"paste_back_ragged_device: 65 frames"):
        pu.paste_back_ragged_device(bases[:1] * 65, list(range(66)), **a)
    with pytest.raises(ValueError, match=r"paste_back_ragged_device: 2 row offsets for 2 frames \(one more than frames\)"):
        pu.paste_back_ragged_device(bases, [0, 4], **a)
    with pytest.raises(ValueError, match=r"paste_back_ragged_device: every base image is uint8 \(6, 10, 3\) on cpu"):
        pu.paste_back_ragged_device([bases[0], bases[1].float()], [0, 1, 4], **a)
    with pytest.raises(ValueError, match=r"paste_back_ragged_device: masks \(4, 7, 10\), 4 crops, geom \(4, 8\) for frames of \(6, 10\)"):
        pu.paste_back_ragged_device(bases, [0, 1, 4], **dict(a, masks=z(4, 7, 10)))
    with pytest.raises(ValueError, match=r"paste_back_ragged_device: masks \(4, 6, 10\), 3 crops"):
        pu.paste_back_ragged_device(bases, [0, 1, 4], **dict(a, net_images=a["net_images"][:3]))
