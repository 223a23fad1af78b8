"""The cases of the foreground-box tests and a pure-numpy restatement of the definition at the head of csrc/foreground_boxes.h.
CPU-importable: nothing here touches the library or a device.

A case is one call: 'frames' and 'backgrounds' (lists of uint8 [H, W, 3]; a background may be the same array for every frame),
'params' (thr, cell, min_count, open_r, close_r, min_area, min_w, min_h, max_boxes, roi) and, where the answer is known without
any code, 'want' = the boxes of frame 0 and 'want_stats' = its (n_kept, n_examined, flags).  Output tables start as `CANARY`.

reference(): erosion and dilation take the whole square window at once (the kernel's passes are separable: the restatement is
not); a component is "dilate by the cross, AND with what is left, until nothing changes" from the first cell left in raster order;
a box is the extent of the P pixels themselves under the component's cells, not of any per-cell record."""
import functools

import numpy as np

CANARY = -0x5A5A5A5B
OVERFLOW, TRUNCATED = 1, 2
MAX_COMPONENTS = 256
DEFAULTS = dict(thr=24, cell=4, min_count=8, open_r=0, close_r=0, min_area=1, min_w=1, min_h=1, max_boxes=8, roi=None)
WRONG = ("eight", "gt", "cellbox", "close0")


# ---------------------------------------------------------------------------------------------------------------- the definition
def _window(a, r, outside, op):
    if r == 0 or a.size == 0:
        return a.copy()
    h, w = a.shape
    p = np.pad(a, r, constant_values=outside)
    out = p[r:r + h, r:r + w].copy()
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = op(out, p[dy:dy + h, dx:dx + w])
    return out


def erode(a, r, outside):
    return _window(a, r, bool(outside), np.logical_and)


def dilate(a, r):
    return _window(a, r, False, np.logical_or)


def propagate(seed, mask, eight=False):
    cur = seed & mask
    while True:
        g = cur.copy()
        g[1:] |= cur[:-1]
        g[:-1] |= cur[1:]
        g[:, 1:] |= cur[:, :-1]
        g[:, :-1] |= cur[:, 1:]
        if eight:
            g[1:, 1:] |= cur[:-1, :-1]
            g[1:, :-1] |= cur[:-1, 1:]
            g[:-1, 1:] |= cur[1:, :-1]
            g[:-1, :-1] |= cur[1:, 1:]
        g &= mask
        if np.array_equal(g, cur):
            return cur
        cur = g


def pixels(frame, background, thr, roi):
    """P: bool [H, W]."""
    H, W = frame.shape[:2]
    P = np.abs(frame.astype(np.int64) - background.astype(np.int64)).max(axis=2) > thr
    x0, y0, x1, y1 = (0, 0, W, H) if roi is None else roi
    inside = np.zeros((H, W), dtype=bool)
    inside[y0:y1, x0:x1] = True
    return P & inside


def grid(P, cell):
    """-> (cnt int64 [gh, gw], P padded with False to [gh cell, gw cell])."""
    H, W = P.shape
    gh, gw = -(-H // cell), -(-W // cell)
    pad = np.zeros((gh * cell, gw * cell), dtype=bool)
    pad[:H, :W] = P
    return pad.reshape(gh, cell, gw, cell).sum(axis=(1, 3)), pad


def g2_of(cnt, p, wrong=None):
    G0 = cnt > p["min_count"] if wrong == "gt" else cnt >= p["min_count"]
    G1 = dilate(erode(G0, p["open_r"], 0), p["open_r"])
    return erode(dilate(G1, p["close_r"]), p["close_r"], 0 if wrong == "close0" else 1)


def components(G2, eight=False):
    """The components of G2 as bool planes, in the raster order of their first cell, and whether more than MAX_COMPONENTS exist."""
    left, out = G2.copy(), []
    while left.any() and len(out) < MAX_COMPONENTS:
        seed = np.zeros_like(left)
        seed.flat[int(np.argmax(left))] = True
        comp = propagate(seed, left, eight)
        left &= ~comp
        out.append(comp)
    return out, bool(left.any())


def frame_reference(frame, background, p, wrong=None):
    """-> (boxes int32 [K, 4], box_stats int32 [K, 2], stats int32 [4]).  wrong: None, or one of `WRONG`: 'eight' (8-connected
    components), 'gt' (cnt > min_count), 'cellbox' (boxes snapped to the cells), 'close0' (the closing's erosion, outside = 0)."""
    H, W = frame.shape[:2]
    cell, K = p["cell"], p["max_boxes"]
    P = pixels(frame, background, p["thr"], p["roi"])
    cnt, pad = grid(P, cell)
    comps, more = components(g2_of(cnt, p, wrong), wrong == "eight")
    boxes, box_stats = np.zeros((K, 4), dtype=np.int32), np.zeros((K, 2), dtype=np.int32)
    n_kept = 0
    for comp in comps:
        area = int(cnt[comp].sum())
        if area < p["min_area"]:
            continue
        under = pad & np.repeat(np.repeat(comp, cell, axis=0), cell, axis=1)
        if wrong == "cellbox":
            under = np.repeat(np.repeat(comp & (cnt > 0), cell, axis=0), cell, axis=1)
            under[H:] = False
            under[:, W:] = False
        ys, xs = np.nonzero(under)
        box = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1)
        if box[2] - box[0] < p["min_w"] or box[3] - box[1] < p["min_h"]:
            continue
        if n_kept < K:
            boxes[n_kept] = box
            box_stats[n_kept] = (area, int(comp.sum()))
        n_kept += 1
    flags = (OVERFLOW if n_kept > K else 0) | (TRUNCATED if more else 0)
    return boxes, box_stats, np.asarray([n_kept, len(comps), int(P.sum()), flags], dtype=np.int32)


def reference(c, wrong=None):
    r = [frame_reference(f, g, c["params"], wrong) for f, g in zip(c["frames"], c["backgrounds"])]
    return tuple(np.stack([x[i] for x in r]) for i in range(3))


# ---------------------------------------------------------------------------------------------------------------- the cases
def _background(H, W, seed):
    return np.random.default_rng(seed).integers(10, 100, (H, W, 3)).astype(np.uint8)


def _frame(bg, P, seed, by=60):
    """bg + 0..4 of noise (never over thr = 24), and + `by` on one channel at the pixels of P."""
    rng = np.random.default_rng(seed + 1000)
    fr = bg.astype(np.int64) + rng.integers(0, 5, bg.shape)
    ch = rng.integers(0, 3, P.shape)
    for c in range(3):
        fr[..., c] += by * (P & (ch == c))
    return fr.astype(np.uint8)


def _cells(H, W, cell, G):
    """The pixels of the cells of G (bool [gh, gw]), cut at the frame."""
    return np.repeat(np.repeat(np.asarray(G, dtype=bool), cell, axis=0), cell, axis=1)[:H, :W]


def _grid_of(gh, gw, rects):
    G = np.zeros((gh, gw), dtype=bool)
    for i0, j0, i1, j1 in rects:
        G[i0:i1, j0:j1] = True
    return G


def _case(name, H, W, P, seed=0, want=None, want_stats=None, frames=None, **params):
    p = dict(DEFAULTS, **params)
    bg = _background(H, W, seed)
    if frames is None:
        frames = [_frame(bg, P, seed)]
    return dict(name=name, frames=frames, backgrounds=[bg] * len(frames), params=p,
                want=None if want is None else np.asarray(want, dtype=np.int32).reshape(-1, 4), want_stats=want_stats)


def _blobs(H, W, cell, seed, density=0.45, drop=0.1):
    """Coarse random blobs of 2 x 2 cells with single pixels dropped: partial cells on both axes when H, W are no multiples."""
    rng = np.random.default_rng(seed)
    gh, gw = -(-H // cell), -(-W // cell)
    coarse = rng.random((gh // 2 + 1, gw // 2 + 1)) < density
    G = np.repeat(np.repeat(coarse, 2, axis=0), 2, axis=1)[:gh, :gw]
    return _cells(H, W, cell, G) & (rng.random((H, W)) >= drop)


def _spiral(n):
    """A one-cell-wide square spiral on an n x n grid (n odd), walls and corridor alternating."""
    G = np.zeros((n, n), dtype=bool)
    i, j, di, dj = 0, 0, 0, 1
    G[0, 0] = True
    run = n - 1
    for leg in range(n):
        for _ in range(run):
            i, j = i + di, j + dj
            G[i, j] = True
        di, dj = dj, -di
        if leg >= 2 and leg % 2 == 0:
            run -= 2
        if run <= 0:
            break
    return G


def _comb(gh, gw):
    """A spine along the bottom row with a one-cell-wide tooth of full height in every other column."""
    G = np.zeros((gh, gw), dtype=bool)
    G[gh - 1] = True
    G[:, ::2] = True
    return G


def _build():
    cases = []
    add = cases.append
    # word seams of the grid with partial edge cells on both axes
    for H, W in ((37, 70), (37, 133), (21, 260)):
        P = _blobs(H, W, 4, H * W)
        add(_case(f"seam_{H}x{W}", H, W, P, seed=W, max_boxes=64))
        add(_case(f"seam_{H}x{W}_open1_close1", H, W, P, seed=W, open_r=1, close_r=1, max_boxes=64))
    # 18 x 22: the last cell of both axes is 2 pixels; the only P pixels are its four
    P = np.zeros((18, 22), dtype=bool)
    P[16:, 20:] = True
    add(_case("partial_last_cell_only", 18, 22, P, min_count=4, want=[[20, 16, 22, 18]], want_stats=(1, 1, 0)))
    # cnt = min_count - 1 beside cnt = min_count
    P = np.zeros((12, 24), dtype=bool)
    P[4:6, 4:8] = True
    P[4:6, 16:20] = True
    P[5, 7] = False
    add(_case("count_edge", 12, 24, P, want=[[16, 4, 20, 6]], want_stats=(1, 1, 0)))
    # a difference of exactly thr is not over it
    bg = _background(12, 24, 5)
    fr = bg.copy()
    fr[4:8, 4:8, 1] += 24
    fr[4:8, 16:20, 2] += 25
    c = _case("thr_exact", 12, 24, None, seed=5, frames=[fr], want=[[16, 4, 20, 8]], want_stats=(1, 1, 0))
    add(c)
    # an roi that cuts through cells
    P = np.zeros((32, 32), dtype=bool)
    P[4:28, 4:28] = True
    add(_case("roi_cuts_cells", 32, 32, P, roi=(10, 6, 23, 21), min_count=1, want=[[10, 6, 23, 21]], want_stats=(1, 1, 0)))
    add(_case("roi_empty", 32, 32, P, roi=(10, 6, 10, 21), min_count=1, want=[], want_stats=(0, 0, 0)))
    add(_case("empty_frame", 30, 45, np.zeros((30, 45), dtype=bool), want=[], want_stats=(0, 0, 0)))
    add(_case("all_foreground", 30, 45, np.ones((30, 45), dtype=bool), roi=(3, 2, 41, 29), min_count=1, want=[[3, 2, 41, 29]],
              want_stats=(1, 1, 0)))
    # two blobs that touch only diagonally stay two
    G = _grid_of(8, 8, [(1, 1, 3, 3), (3, 3, 5, 5)])
    add(_case("diagonal_touch", 32, 32, _cells(32, 32, 4, G), want=[[4, 4, 12, 12], [12, 12, 20, 20]], want_stats=(2, 2, 0)))
    # floods that need many sweeps, both ways
    add(_case("spiral", 60, 60, _cells(60, 60, 4, _spiral(15)), want=[[0, 0, 60, 60]], want_stats=(1, 1, 0)))
    add(_case("spiral_flipped", 60, 60, _cells(60, 60, 4, _spiral(15)[::-1, ::-1]), want=[[0, 0, 60, 60]], want_stats=(1, 1, 0)))
    add(_case("comb", 60, 140, _cells(60, 140, 4, _comb(15, 35)), want=[[0, 0, 140, 60]], want_stats=(1, 1, 0)))
    add(_case("comb_upside_down", 60, 140, _cells(60, 140, 4, _comb(15, 35)[::-1]), want=[[0, 0, 140, 60]], want_stats=(1, 1, 0)))
    # the closing joins across 2 close_r cells and not across 2 close_r + 1
    G = _grid_of(7, 25, [(2, 1, 5, 4), (2, 6, 5, 9), (2, 14, 5, 17), (2, 20, 5, 23)])
    add(_case("close_joins_gap2_not_gap3", 28, 100, _cells(28, 100, 4, G), close_r=1,
              want=[[4, 8, 36, 20], [56, 8, 68, 20], [80, 8, 92, 20]], want_stats=(3, 3, 0)))
    # the closing at the frame edge: outside = 1, the corner blob is not eaten back
    G = _grid_of(6, 6, [(0, 0, 3, 3)])
    add(_case("close_at_edge", 24, 24, _cells(24, 24, 4, G), close_r=1, want=[[0, 0, 12, 12]], want_stats=(1, 1, 0)))
    # a one-cell speck goes with open_r = 1, the 3 x 3 blob stays
    G = _grid_of(8, 12, [(1, 1, 2, 2), (3, 5, 6, 8)])
    add(_case("speck_opened", 32, 48, _cells(32, 48, 4, G), open_r=1, want=[[20, 12, 32, 24]], want_stats=(1, 1, 0)))
    # a blob that fills only a part of its cells: the box is tight
    P = np.zeros((24, 28), dtype=bool)
    P[5:18, 6:21] = True
    add(_case("tight_box", 24, 28, P, min_count=1, want=[[6, 5, 21, 18]], want_stats=(1, 1, 0)))
    # a component that is too small and comes first; too narrow; too low
    G = _grid_of(10, 16, [(0, 12, 1, 13), (2, 2, 6, 6), (2, 9, 9, 10), (8, 1, 9, 7)])
    add(_case("small_first_then_kept", 40, 64, _cells(40, 64, 4, G), min_area=40, min_w=6, min_h=6, want=[[8, 8, 24, 24]],
              want_stats=(1, 4, 0)))
    # four kept, room for two
    G = _grid_of(8, 16, [(1, 1, 3, 3), (1, 5, 3, 7), (5, 1, 7, 3), (5, 9, 7, 11)])
    add(_case("overflow_k2", 32, 64, _cells(32, 64, 4, G), max_boxes=2, want=[[4, 4, 12, 12], [20, 4, 28, 12]], want_stats=(4, 4, OVERFLOW)))
    # 24 x 24 cells as a checkerboard: 288 isolated components, 256 examined
    G = (np.add.outer(np.arange(24), np.arange(24)) % 2) == 0
    add(_case("checkerboard_288", 96, 96, _cells(96, 96, 4, G), min_count=16, max_boxes=64, want_stats=(256, 256, OVERFLOW | TRUNCATED)))
    # three frames against one background
    bg = _background(37, 70, 9)
    frames = [_frame(bg, _blobs(37, 70, 4, 90 + f, density=0.3), 90 + f) for f in range(3)]
    add(_case("three_frames_one_background", 37, 70, None, seed=9, frames=frames, close_r=1, min_area=20, max_boxes=16))
    add(_case("cell8", 50, 150, _blobs(50, 150, 8, 8, density=0.3), seed=8, cell=8, min_count=16, close_r=1, max_boxes=32))
    add(_case("cell16", 70, 200, _blobs(70, 200, 16, 16, density=0.3), seed=16, cell=16, min_count=100, close_r=1, max_boxes=32))
    return cases


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
CASE_NAMES = [c["name"] for c in CASES]
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def expected(name):
    return reference(BY_NAME[name])


def roi_of(c):
    H, W = c["frames"][0].shape[:2]
    return (0, 0, W, H) if c["params"]["roi"] is None else tuple(c["params"]["roi"])
