"""The background estimator's definition restated in numpy, and the small cases its kernel is checked on (numpy only: imported by
the CPU and the GPU test file).

Definition (csrc/background.h): frame t covers pixel (x, y) if one of its boxes has x0 - margin <= x <= x1 + margin and y0 - margin
<= y <= y1 + margin, both ends inclusive, a box with x1 < x0 or y1 < y0 covering nothing; n = the frames that do not cover the
pixel; the samples are those n frames if n >= min_valid, else all T; bg = per channel the sample of rank (m - 1) // 2 in ascending
order; count = n."""
import functools

import numpy as np


def coverage(boxes, T, H, W, margin, exclusive=False):
    """bool [T, H, W].  exclusive=True is the WRONG rule (half-open box ends) the tests show the cases can tell apart."""
    cov = np.zeros((T, H, W), dtype=bool)
    if boxes is None:
        return cov
    end = 0 if exclusive else 1
    for t in range(T):
        for x0, y0, x1, y1 in np.asarray(boxes[t], dtype=np.int64).reshape(-1, 4).tolist():
            if x1 < x0 or y1 < y0:
                continue
            xa, xb = max(x0 - margin, 0), min(x1 + margin + end, W)
            ya, yb = max(y0 - margin, 0), min(y1 + margin + end, H)
            if xb > xa and yb > ya:
                cov[t, ya:yb, xa:xb] = True
    return cov


def reference(frames, boxes=None, margin=0, min_valid=1, upper=False, exclusive=False):
    """(bg uint8 [H, W, 3], count uint8 [H, W]).  upper=True is the WRONG rank m // 2."""
    fr = np.stack([np.asarray(f) for f in frames]).astype(np.int16)            # [T, H, W, 3]
    T, H, W, _ = fr.shape
    free = ~coverage(boxes, T, H, W, margin, exclusive)
    n = free.sum(axis=0)
    use = free | (n < min_valid)[None]                                          # the fallback: all T
    m = use.sum(axis=0)
    vals = np.where(use[..., None], fr, 256)                                    # the samples that are not selected sort last
    srt = np.sort(vals, axis=0)
    rank = (m // 2) if upper else ((m - 1) // 2)
    bg = np.take_along_axis(srt, np.broadcast_to(rank[None, :, :, None], (1, H, W, 3)), axis=0)[0]
    assert bg.max() <= 255
    return bg.astype(np.uint8), n.astype(np.uint8)


def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (2 ** 32))


def _frames(rng, T, H, W, lo=0, hi=256):
    return [rng.integers(lo, hi, (H, W, 3), dtype=np.int64).astype(np.uint8) for _ in range(T)]


def _random_boxes(rng, T, H, W, most=3):
    """Up to `most` boxes per frame, some reaching outside the frame."""
    out = []
    for _ in range(T):
        nb = int(rng.integers(0, most + 1))
        x0 = rng.integers(-3, W + 2, nb)
        y0 = rng.integers(-3, H + 2, nb)
        out.append(np.stack([x0, y0, x0 + rng.integers(0, max(W // 2, 2), nb), y0 + rng.integers(0, max(H // 2, 2), nb)], axis=1).astype(np.int64))
    return out


def _case(name, frames, boxes=None, margin=0, min_valid=1):
    return {"name": name, "frames": frames, "boxes": boxes, "margin": margin, "min_valid": min_valid}


def _region(T, frames_covered, box):
    """Per-frame box lists: `box` in the listed frames, nothing elsewhere."""
    return [np.asarray([box], dtype=np.int64) if t in frames_covered else np.zeros((0, 4), dtype=np.int64) for t in range(T)]


def _build():
    cases = []
    # every T at which the kernel changes its bucket or fills one, on a frame smaller than a wave with 3 W not a multiple of 4
    for T in (1, 2, 3, 8, 9, 16, 17, 32, 33, 63, 64):
        name = f"t{T}_5x7"
        r = _rng(name)
        cases.append(_case(name, _frames(r, T, 5, 7), _random_boxes(r, T, 5, 7), margin=1, min_valid=1))
    for T in (1, 64):
        name = f"t{T}_1x1"
        r = _rng(name)
        cases.append(_case(name, _frames(r, T, 1, 1)))
    cases.append(_case("t2_1x1_box", _frames(_rng("t2_1x1_box"), 2, 1, 1), _region(2, {0}, [0, 0, 0, 0])))
    # more than one workgroup, rows that straddle workgroups (3 * 130 = 390 bytes a row)
    for T, mv in ((3, 1), (9, 2), (17, 17), (33, 4), (64, 8)):
        name = f"t{T}_33x130"
        r = _rng(name)
        cases.append(_case(name, _frames(r, T, 33, 130), _random_boxes(r, T, 33, 130, most=4), margin=2, min_valid=mv))
    r = _rng("t16_64x257")                                                       # 3 * 64 * 257 is a multiple of 4, 3 * 257 is not
    cases.append(_case("t16_64x257", _frames(r, 16, 64, 257), _random_boxes(r, 16, 64, 257, most=6), margin=3, min_valid=2))
    r = _rng("t5_3x3_no_boxes")                                                  # 27 bytes: the last dword is partial
    cases.append(_case("t5_3x3_no_boxes", _frames(r, 5, 3, 3)))
    # values
    cases.append(_case("all_equal", [np.full((5, 7, 3), 77, dtype=np.uint8) for _ in range(9)], _random_boxes(_rng("all_equal"), 9, 5, 7)))
    r = _rng("extremes")
    cases.append(_case("extremes", [(r.integers(0, 2, (5, 7, 3)) * 255).astype(np.uint8) for _ in range(8)], _random_boxes(r, 8, 5, 7)))
    r = _rng("ties")
    cases.append(_case("ties", _frames(r, 17, 33, 130, lo=10, hi=13), _random_boxes(r, 17, 33, 130), margin=1, min_valid=3))
    # a pixel whose three channels take their median from three different frames: (20 of frame 1, 21 of frame 2, 22 of frame 0)
    tri = [np.broadcast_to(np.asarray(v, dtype=np.uint8), (5, 7, 3)).copy() for v in ((10, 31, 22), (20, 11, 32), (30, 21, 12))]
    cases.append(_case("channels_differ", tri))
    # boxes
    H, W = 33, 130
    r = _rng("borders")
    touch = [[0, 0, 0, H - 1], [W - 1, 0, W - 1, H - 1], [0, 0, W - 1, 0], [0, H - 1, W - 1, H - 1], [40, 10, 60, 20]]
    cases.append(_case("borders", _frames(r, 8, H, W), [np.asarray([touch[t % 5], touch[(t + 2) % 5]], dtype=np.int64) for t in range(8)]))
    r = _rng("outside")
    out_boxes = [[-10, -10, 3, 3], [W - 2, H - 2, W + 50, H + 50], [W, 0, W + 5, H], [-100, -100, -1, -1], [0, H, W - 1, H + 3],
                 [-2 ** 31, 5, 4, 6], [100, -7, 2 ** 31 - 1, 2]]
    cases.append(_case("outside", _frames(r, 7, H, W), [np.asarray([out_boxes[t], out_boxes[(t + 3) % 7]], dtype=np.int64) for t in range(7)]))
    r = _rng("outside_margin")                                                   # boxes wholly outside that the margin brings in
    cases.append(_case("outside_margin", _frames(r, 7, H, W),
                       [np.asarray([out_boxes[t], out_boxes[(t + 3) % 7]], dtype=np.int64) for t in range(7)], margin=2))
    r = _rng("margin_past_frame")                                                # the margin reaches past the frame: frames 0 and 3 see nothing
    cases.append(_case("margin_past_frame", _frames(r, 5, H, W), _region(5, {0, 3}, [60, 15, 61, 16]), margin=32767))
    r = _rng("empty_and_full")                                                   # empty boxes (a margin must not revive them); 0 boxes next to 64
    eb = []
    for t in range(9):
        if t % 3 == 0:
            eb.append(np.zeros((0, 4), dtype=np.int64))
        elif t % 3 == 1:
            eb.append(np.asarray([[50, 10, 49, 20], [50, 10, 60, 9], [5, 5, 4, 4]], dtype=np.int64))
        else:
            x0 = r.integers(-5, W, 64)
            y0 = r.integers(-5, H, 64)
            eb.append(np.stack([x0, y0, x0 + r.integers(-1, 6, 64), y0 + r.integers(-1, 4, 64)], axis=1).astype(np.int64))
    cases.append(_case("empty_and_full", _frames(r, 9, H, W), eb, margin=2, min_valid=2))
    # how many frames see a pixel: never (fallback), once (n = 1), n even, n odd
    r = _rng("fallback_and_one")
    fb = [np.asarray([[10, 5, 30, 12]] + ([[70, 20, 90, 28]] if t != 4 else []), dtype=np.int64) for t in range(9)]
    cases.append(_case("fallback_and_one", _frames(r, 9, H, W), fb))
    r = _rng("n_even_odd")
    eo = [np.asarray(([[10, 5, 30, 12]] if t < 3 else []) + ([[70, 20, 90, 28]] if t < 4 else []), dtype=np.int64).reshape(-1, 4) for t in range(9)]
    cases.append(_case("n_even_odd", _frames(r, 9, H, W), eo))
    # min_valid at 1, n, n + 1 and T around a region with n = 5 of T = 8
    for mv in (1, 5, 6, 8):
        name = f"min_valid_{mv}_n5_t8"
        cases.append(_case(name, _frames(_rng("min_valid_n5_t8"), 8, H, W), _region(8, {1, 2, 6}, [20, 8, 99, 25]), min_valid=mv))
    return cases


CASES = _build()
CASE_NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The reference's (bg, count) of a case: computed once, read-only."""
    c = BY_NAME[name]
    bg, count = reference(c["frames"], c["boxes"], c["margin"], c["min_valid"])
    bg.setflags(write=False)
    count.setflags(write=False)
    return bg, count
