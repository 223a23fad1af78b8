"""The cases of the foreground-mask tests and a pure-numpy restatement of the definition at the head of csrc/foreground.h.
CPU-importable: nothing here touches the library or a device.

A case is one launch: 'frames' and 'backgrounds' (lists of uint8 [H, W, 3]), 'boxes' and 'cores' (int64 [n, 4], half-open, frame
coordinates), 'frame_rows' (None for one frame), 'params' (thr, open_r, close_r, grow, fallback), and optionally 'max_box' (the
bound of the launch), 'offs' + 'buf_len' (mask offsets other than the running sum) and 'raw' (a box leaves the frame: the ops
wrappers refuse such a table, so the tests hand it to the library themselves).  The mask buffer of every case starts as `CANARY`
bytes: what a refused box or a gap leaves behind is part of the expected result.

reference(): the flood is "dilate by the cross, AND with the mask, until nothing changes"; erosion and dilation take the whole
square window at once (the kernel's passes are separable: the restatement is not)."""
import functools

import numpy as np

CANARY = 0xA5
DEFAULTS = dict(thr=24, open_r=1, close_r=3, grow=0, fallback=True)
FALLBACK, BORDER, REFUSED = 1, 2, 4


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


def border_of(h, w):
    b = np.zeros((h, w), dtype=bool)
    if h and w:
        b[0] = b[-1] = True
        b[:, 0] = b[:, -1] = True
    return b


def box_f0(frame, background, box, thr, wrong=None):
    x0, y0, x1, y1 = (int(v) for v in box)
    d = np.abs(frame[y0:y1, x0:x1].astype(np.int64) - background[y0:y1, x0:x1].astype(np.int64))
    v = d.sum(axis=2) if wrong == "sum" else d.max(axis=2)
    return v >= thr if wrong == "ge" else v > thr


def core_mask(box, core):
    x0, y0, x1, y1 = (int(v) for v in box)
    h, w = y1 - y0, x1 - x0
    cx0, cx1 = (min(max(int(core[i]) - x0, 0), w) for i in (0, 2))
    cy0, cy1 = (min(max(int(core[i]) - y0, 0), h) for i in (1, 3))
    m = np.zeros((h, w), dtype=bool)
    m[cy0:cy1, cx0:cx1] = True
    return m


def box_reference(frame, background, box, core, thr, open_r, close_r, grow, fallback, wrong=None):
    """-> (M bool [h, w], [n_F0, n_seed, n_mask, flags]).  wrong: None, or one of the four mistakes the table must tell apart:
    'eight' (8-connected floods), 'close0' (the closing's erosion with outside = 0), 'sum' (channel sum), 'ge' (>= thr)."""
    F0 = box_f0(frame, background, box, thr, wrong)
    h, w = F0.shape
    F1 = dilate(erode(F0, open_r, 0), open_r)
    F2 = erode(dilate(F1, close_r), close_r, 0 if wrong == "close0" else 1)
    cm = core_mask(box, core)
    seed = F2 & cm
    flags = 0
    if seed.any():
        R = propagate(seed, F2, wrong == "eight")
        M = ~propagate(~R & border_of(h, w), ~R, wrong == "eight")
    elif fallback:
        M, flags = cm, FALLBACK
    else:
        M = np.zeros((h, w), dtype=bool)
    M = dilate(M, grow)
    if (M & border_of(h, w)).any():
        flags |= BORDER
    return M, [int(F0.sum()), int(seed.sum()), int(M.sum()), flags]


def max_box_of(c):
    if c.get("max_box") is not None:
        return tuple(c["max_box"])
    b = c["boxes"]
    return (int((b[:, 3] - b[:, 1]).max()), int((b[:, 2] - b[:, 0]).max())) if len(b) else (0, 0)


def offsets_of(c):
    if c.get("offs") is not None:
        return np.asarray(c["offs"], dtype=np.int64)
    b = c["boxes"]
    hw = (b[:, 3] - b[:, 1]) * (b[:, 2] - b[:, 0])
    return np.concatenate([[0], np.cumsum(hw)[:-1]]).astype(np.int64) if len(b) else np.zeros(0, np.int64)


def buf_len_of(c):
    if c.get("buf_len") is not None:
        return int(c["buf_len"])
    b = c["boxes"]
    return int(((b[:, 3] - b[:, 1]) * (b[:, 2] - b[:, 0])).sum())


def accepted(c, b):
    H, W = c["frames"][0].shape[:2]
    x0, y0, x1, y1 = (int(v) for v in c["boxes"][b])
    if x0 < 0 or y0 < 0 or x1 < x0 or y1 < y0 or x1 > W or y1 > H:
        return False
    mh, mw = max_box_of(c)
    if y1 - y0 > mh or x1 - x0 > mw:
        return False
    off = int(offsets_of(c)[b])
    return 0 <= off <= buf_len_of(c) and (y1 - y0) * (x1 - x0) <= buf_len_of(c) - off


def box_frame(c, b):
    """The frame whose rows hold box b (a frame without boxes holds none)."""
    rows = c["frame_rows"] if c["frame_rows"] is not None else [0, len(c["boxes"])]
    return next(f for f in range(len(rows) - 1) if rows[f] <= b < rows[f + 1])


def reference(c, wrong=None):
    """-> (mask buffer uint8 [buf_len] that started as CANARY bytes, stats int32 [n, 4])."""
    buf = np.full(buf_len_of(c), CANARY, dtype=np.uint8)
    n = len(c["boxes"])
    stats = np.zeros((n, 4), dtype=np.int32)
    offs = offsets_of(c)
    for b in range(n):
        if not accepted(c, b):
            stats[b] = (0, 0, 0, REFUSED)
            continue
        f = box_frame(c, b)
        M, st = box_reference(c["frames"][f], c["backgrounds"][f], c["boxes"][b], c["cores"][b], wrong=wrong, **c["params"])
        buf[offs[b]:offs[b] + M.size] = np.where(M, 255, 0).astype(np.uint8).reshape(-1)
        stats[b] = st
    return buf, stats


# ---------------------------------------------------------------------------------------------------------------------- the table
def scene(H, W, fg, seed=0, delta=100):
    """(frame, background): a background of 10..100 per channel, the frame = background + noise of at most 6 levels, plus `delta`
    on one channel wherever `fg` is set - so F0 at thr 24 is exactly `fg`."""
    r = np.random.default_rng(seed)
    bg = r.integers(10, 101, (H, W, 3)).astype(np.int64)
    fr = bg + r.integers(-6, 7, (H, W, 3))
    fr[..., seed % 3] += np.where(fg, delta, 0)
    return fr.astype(np.uint8), bg.astype(np.uint8)


def blocks(H, W, seed, cell=3, density=0.6):
    r = np.random.default_rng(seed)
    coarse = r.random((H // cell + 1, W // cell + 1)) < density
    fine = np.kron(coarse, np.ones((cell, cell), dtype=bool))[:H, :W]
    return fine ^ (r.random((H, W)) < 0.03)                                      # salt and pepper on top


CASES = []


def add(name, frames, backgrounds, boxes, cores, frame_rows=None, **kw):
    params = dict(DEFAULTS)
    extra = {k: kw.pop(k) for k in ("max_box", "offs", "buf_len", "raw") if k in kw}
    params.update(kw)
    single = isinstance(frames, np.ndarray) and frames.ndim == 3
    CASES.append(dict(name=name, frames=[frames] if single else list(frames), backgrounds=[backgrounds] if single else list(backgrounds),
                      boxes=np.asarray(boxes, dtype=np.int64).reshape(-1, 4), cores=np.asarray(cores, dtype=np.int64).reshape(-1, 4),
                      frame_rows=frame_rows, params=params, **extra))


def _seams(name, **kw):
    """widths 1, 31, 32, 33, 63, 64, 65, 130 against heights 1, 2, 70: word seams and single rows"""
    fr, bg = scene(80, 140, blocks(80, 140, 7), seed=7)
    boxes, cores = [], []
    for i, w in enumerate((1, 31, 32, 33, 63, 64, 65, 130)):
        for j, h in enumerate((1, 2, 70)):
            x0, y0 = (3 * i + j) % (141 - w), (5 * j + i) % (81 - h)
            boxes.append([x0, y0, x0 + w, y0 + h])
            cores.append([x0 + w // 4, y0 + h // 4, x0 + w - w // 4, y0 + h - h // 4])
    add(name, fr, bg, boxes, cores, **kw)


_seams("seams_default")
_seams("seams_open0_close1", open_r=0, close_r=1)
_seams("seams_open0_close0_grow2", open_r=0, close_r=0, grow=2)

# d == thr against d == thr + 1, and a channel sum over thr under a channel maximum that is not
bg = np.full((4, 8, 3), 50, dtype=np.uint8)
fr = bg.copy()
fr[1, 1] = (74, 50, 50)          # d = 24 = thr: out
fr[1, 3] = (50, 25, 50)          # d = 25: in
fr[1, 5] = (60, 60, 60)          # sum 30, max 10: out
fr[2, 6] = (50, 50, 26)          # d = 24 downwards: out
fr[3, 0] = (50, 50, 24)          # d = 26: in
add("thr_edge", fr, bg, [[0, 0, 8, 4]], [[0, 0, 8, 4]], open_r=0, close_r=0, fallback=False)
bg = np.zeros((3, 5, 3), dtype=np.uint8)
fr = bg.copy()
fr[1, 2] = (255, 0, 0)
fr[1, 4] = (254, 254, 254)
add("thr_254", fr, bg, [[0, 0, 5, 3]], [[0, 0, 5, 3]], thr=254, open_r=0, close_r=0, fallback=False)
add("thr_0", fr, bg, [[0, 0, 5, 3]], [[0, 0, 5, 3]], thr=0, open_r=0, close_r=0, fallback=False)

# specks of 1, 3 x 3 and 5 x 5 beside a body, the core the whole box: only the opening can remove them
fg = np.zeros((40, 60), dtype=bool)
fg[10:30, 5:35] = True
fg[3, 50] = fg[20, 45] = fg[38, 58] = True
fg[5:8, 40:43] = True
fg[30:35, 50:55] = True
fr, bg = scene(40, 60, fg, seed=1)
for r_ in (0, 1, 3):
    add(f"specks_open{r_}", fr, bg, [[0, 0, 60, 40]], [[0, 0, 60, 40]], open_r=r_, close_r=0)

# a body cut by the box edge: the closing must not eat it back from there
fg = np.zeros((50, 70), dtype=bool)
fg[8:50, 0:40] = True
fg[20:26, 10:18] = False                                                         # a window
fr, bg = scene(50, 70, fg, seed=2)
for r_ in (3, 7):
    add(f"edge_close{r_}", fr, bg, [[5, 4, 60, 45]], [[10, 15, 30, 40]], close_r=r_)
    add(f"edge_close{r_}_full_frame", fr, bg, [[0, 0, 70, 50]], [[10, 15, 30, 40]], close_r=r_)

# holes: enclosed, open to the border, closed only diagonally - three boxes of one frame
fg = np.zeros((30, 90), dtype=bool)
for x in (2, 32, 62):
    fg[5:22, x + 3:x + 23] = True
    fg[8:19, x + 6:x + 20] = False                                               # 3-thick rings
fg[8:19, 32 + 20:32 + 30] = False                                                # the second opens to its box's right border
fg[0:30, 62:90] = False
fg[5, 66:84] = fg[20, 66:84] = fg[5:21, 66] = fg[5:21, 83] = True                # the third: a 1-thick outline ..
fg[5, 66] = False                                                                # .. without a corner: the gap is diagonal
fr, bg = scene(30, 90, fg, seed=3)
add("holes", fr, bg, [[0, 0, 30, 30], [30, 0, 57, 30], [60, 0, 90, 30]], [[0, 0, 30, 30], [30, 0, 60, 30], [60, 0, 90, 30]],
    open_r=0, close_r=0)

# a second component that touches the seeded one only diagonally, and one apart from it inside the box but outside the core
fg = np.zeros((30, 40), dtype=bool)
fg[5:11, 5:11] = True
fg[11:16, 11:16] = True
fg[20:27, 25:36] = True
fr, bg = scene(30, 40, fg, seed=4)
add("diag_component", fr, bg, [[0, 0, 40, 30]], [[6, 6, 9, 9]], open_r=0, close_r=0)
fg = np.zeros((60, 100), dtype=bool)
fg[15:45, 10:55] = True
fg[10:30, 75:95] = True
fr, bg = scene(60, 100, fg, seed=5)
add("outside_core", fr, bg, [[2, 3, 99, 58]], [[20, 20, 45, 40]])

# a 65 x 65 comb: a serpentine corridor that a flood needs tens of sweeps to walk, along the rows and along the columns
fg = np.zeros((65, 65), dtype=bool)
fg[0::2] = True
for i in range(1, 65, 2):
    fg[i, 64 if (i // 2) % 2 == 0 else 0] = True
for name, pat in (("comb_rows", fg), ("comb_cols", fg.T.copy())):
    full = np.zeros((70, 72), dtype=bool)
    full[3:68, 4:69] = pat
    fr, bg = scene(70, 72, full, seed=6)
    add(name, fr, bg, [[4, 3, 69, 68]], [[4, 3, 6, 5]], open_r=0, close_r=0)

# cores partly and wholly outside their box; an empty seed with the fallback on and off
fg = np.zeros((40, 60), dtype=bool)
fg[10:30, 10:40] = True
fr, bg = scene(40, 60, fg, seed=8)
B = [8, 6, 50, 36]
add("core_partly_outside", fr, bg, [B, B, B], [[0, 0, 14, 14], [35, 25, 70, 50], [-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1]])
add("core_outside_fallback", fr, bg, [B, B, B], [[0, 0, 8, 6], [50, 36, 60, 40], [30, 20, 20, 10]])
add("empty_seed_fallback", fr, bg, [B, B], [[42, 8, 48, 20], [41, 31, 60, 40]])
add("empty_seed_no_fallback", fr, bg, [B, B], [[42, 8, 48, 20], [41, 31, 60, 40]], fallback=False)

# grow against the box edge
for g_ in (0, 4, 15):
    add(f"grow{g_}", fr, bg, [[8, 6, 50, 36], [12, 12, 45, 28]], [[20, 15, 30, 25], [20, 15, 30, 25]], grow=g_)

# boxes in the four frame corners, and two that overlap
fg = np.zeros((50, 70), dtype=bool)
fg[0:12, 0:15] = fg[0:10, 58:70] = fg[40:50, 0:9] = fg[37:50, 55:70] = True
fg[18:32, 25:45] = True
fr, bg = scene(50, 70, fg, seed=9)
add("corners_and_overlap", fr, bg, [[0, 0, 20, 16], [50, 0, 70, 14], [0, 34, 14, 50], [48, 30, 70, 50], [20, 14, 44, 36], [28, 16, 50, 34]],
    [[2, 2, 8, 8], [62, 2, 68, 6], [1, 42, 6, 48], [60, 40, 68, 48], [28, 20, 40, 30], [30, 20, 42, 30]], close_r=2)

# 64 boxes over three frames, ragged, the middle frame without boxes; every frame with a background of its own
r_ = np.random.default_rng(64)
frs, bgs = zip(*[scene(60, 90, blocks(60, 90, 20 + f, cell=5, density=0.45), seed=20 + f) for f in range(3)])
boxes, cores = [], []
for b in range(64):
    w, h = int(r_.integers(1, 51)), int(r_.integers(1, 41))
    x0, y0 = int(r_.integers(0, 91 - w)), int(r_.integers(0, 61 - h))
    boxes.append([x0, y0, x0 + w, y0 + h])
    cores.append([x0 + w // 3, y0 + h // 3, x0 + w - w // 3, y0 + h - h // 3])
add("ragged64", frs, bgs, boxes, cores, frame_rows=[0, 40, 40, 64], close_r=2)
add("ragged64_grow3_max_box_frame", frs, bgs, boxes, cores, frame_rows=[0, 40, 40, 64], close_r=2, grow=3, max_box=(60, 90))

add("v0", fr, bg, np.zeros((0, 4)), np.zeros((0, 4)))

# one 600 x 1000 box in a 640 x 1024 frame: the planes cannot be in LDS.  A body with a window, a neighbour, specks.
fg = np.zeros((640, 1024), dtype=bool)
fg[200:420, 300:720] = True
fg[260:330, 400:560] = False
fg[100:160, 800:900] = True
fg[np.random.default_rng(11).integers(0, 640, 300), np.random.default_rng(12).integers(0, 1024, 300)] ^= True
fr, bg = scene(640, 1024, fg, seed=10)
add("big_scratch", fr, bg, [[12, 20, 1012, 620]], [[350, 220, 680, 400]])

# a box whose mask would leave the buffer (flagged, its bytes untouched), offsets with gaps, one negative
fg = np.zeros((40, 60), dtype=bool)
fg[10:30, 10:40] = True
fr, bg = scene(40, 60, fg, seed=8)
add("leaves_buffer", fr, bg, [[8, 6, 28, 26], [8, 6, 29, 26], [20, 10, 40, 30], [0, 0, 5, 5], [10, 10, 10, 30]],
    [[10, 10, 20, 20], [10, 10, 20, 20], [22, 12, 30, 20], [0, 0, 5, 5], [10, 10, 20, 20]], offs=[10, 600, 500, -1, 900], buf_len=1000)
# boxes that leave the frame or exceed the bound: refused on the device, the others of the launch unharmed
add("refused", fr, bg, [[8, 6, 50, 36], [40, 10, 61, 30], [-1, 5, 20, 20], [5, 30, 20, 41], [30, 5, 20, 20], [5, 5, 20, 4],
                        [2, 2, 45, 20], [2, 2, 20, 33], [10, 8, 40, 38], [2 ** 31 - 1, 0, -2 ** 31, 5]],
    [[20, 15, 30, 25]] * 10, max_box=(30, 42), raw=True, offs=[0, 1260, 1260, 1260, 1260, 1260, 1260, 1260, 1300, 2200], buf_len=2264)



def raw_args(c, frame_ptrs, bg_ptrs, boxes_ptr, cores_ptr, offs_ptr, mask_ptr, stats_ptr):
    """The arguments of fusg_foreground_masks_host (and, followed by scratch and stream, of fusg_foreground_masks_u8) for a case,
    given the addresses of its tables: for the cases the ops wrappers refuse.  frame_rows is kept alive by the returned list."""
    import ctypes as C
    F, n = len(c["frames"]), len(c["boxes"])
    H, W = c["frames"][0].shape[:2]
    rows = (C.c_int32 * (F + 1))(*(c["frame_rows"] if c["frame_rows"] is not None else [0, n]))
    p, (mh, mw) = c["params"], max_box_of(c)
    return [(C.c_void_p * F)(*frame_ptrs), (C.c_void_p * F)(*bg_ptrs), rows, F, H, W, boxes_ptr, cores_ptr, offs_ptr, n, p["thr"], p["open_r"],
            p["close_r"], p["grow"], int(p["fallback"]), mh, mw, mask_ptr, buf_len_of(c), stats_ptr]


BY_NAME = {c["name"]: c for c in CASES}
CASE_NAMES = [c["name"] for c in CASES]
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def expected(name):
    buf, stats = reference(BY_NAME[name])
    buf.setflags(write=False)
    stats.setflags(write=False)
    return buf, stats
