"""Pure-numpy restatement of EdgeConnect's input construction (the definition heading csrc/inpaint_inputs.h:
create_inpaint_inputs_shape, utils/inpaint_utils.py:35-58) and the fixtures the inpaint-input tests share.  No SciPy, no
OpenCV, no scikit-image: the resize is oracle.cv_host.resize_linear_u8, the hysteresis a plain stack flood fill, and every
float64 step is written as separate numpy operations (one rounding each), in the summation order the definition states."""
import math

import numpy as np

from oracle import cv_host

R = 256
EPS = 2.220446049250313e-16
LOW_T, HIGH_T = 25.5, 51.0
ELLIPSE_TABLE = [(4, 4), (1, 7), (1, 7), (0, 7), (0, 7), (0, 7), (1, 7), (1, 7)]     # inclusive column spans, 53 taps


def ellipse_rows(ksize: int = 8):
    """cv2.getStructuringElement(MORPH_ELLIPSE, (8, 8)) from its rule: the inclusive column span of every row."""
    r = c = ksize // 2
    rows = []
    for i in range(ksize):
        dy = i - r
        dx = round(c * math.sqrt((r * r - dy * dy) / (r * r)))               # Python's round: half to even
        rows.append((max(c - dx, 0), min(c + dx + 1, ksize) - 1))
    return rows


def dilate(mask: np.ndarray) -> np.ndarray:
    """cv2.dilate of a box-sized mask with the ellipse, anchor (4, 4); taps outside the box are ignored."""
    h, w = mask.shape
    out = np.zeros_like(mask)
    for i, (j0, j1) in enumerate(ellipse_rows()):
        for j in range(j0, j1 + 1):
            dy, dx = i - 4, j - 4                                            # dst(y, x) takes src(y + dy, x + dx)
            ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
            yd, xd = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
            if ys.start < ys.stop and xs.start < xs.stop:
                out[ys, xs] = np.maximum(out[ys, xs], mask[yd, xd])
    return out


def gauss_table(sigma: float):
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return phi[radius:].copy(), radius


def gauss_axis(a: np.ndarray, w: np.ndarray, axis: int) -> np.ndarray:
    """t = x[l] w[0]; for d = radius .. 1: t += (x[l - d] + x[l + d]) w[d], zeros outside."""
    r = len(w) - 1
    a = np.moveaxis(a, axis, 0)
    p = np.concatenate([np.zeros((r,) + a.shape[1:]), a, np.zeros((r,) + a.shape[1:])], axis=0)
    n = a.shape[0]
    t = p[r:r + n] * w[0]
    for d in range(r, 0, -1):
        t = t + (p[r - d:r - d + n] + p[r + d:r + d + n]) * w[d]
    return np.moveaxis(t, 0, axis)


def sobel(s: np.ndarray, axis: int) -> np.ndarray:
    """ndimage.sobel(mode='reflect'): [-1, 0, 1] along `axis`, then [1, 2, 1] across it; the edge sample is repeated."""
    s = np.moveaxis(s, axis, 0)
    p = np.pad(s, ((1, 1), (0, 0)), mode="edge")
    d = p[2:] - p[:-2]
    q = np.pad(d, ((0, 0), (1, 1)), mode="edge")
    out = q[:, 1:-1] * 2.0 + (q[:, :-2] + q[:, 2:])
    return np.moveaxis(out, 0, axis)


def erode3(valid: np.ndarray) -> np.ndarray:
    p = np.pad(valid, 1, mode="constant", constant_values=False)
    out = np.ones_like(valid)
    for dy in range(3):
        for dx in range(3):
            out &= p[dy:dy + valid.shape[0], dx:dx + valid.shape[1]]
    return out


SECTORS = (  # (same sign?, |gi| >= |gj| ?, plus side (c1, c2), minus side (c1, c2)) as (di, dj) offsets, in evaluation order
    (True, True, ((1, 0), (1, 1)), ((-1, 0), (-1, -1))),
    (True, False, ((0, 1), (1, 1)), ((0, -1), (-1, -1))),
    (False, False, ((0, 1), (-1, 1)), ((0, -1), (1, -1))),
    (False, True, ((-1, 0), (-1, 1)), ((1, 0), (1, -1))),
)


def nms(gi, gj, mag, er):
    """-> (local maxima, the sector that decided each candidate pixel: 1..4, 0 elsewhere)."""
    ai, aj = np.abs(gi), np.abs(gj)
    same = ((gi >= 0) & (gj >= 0)) | ((gi <= 0) & (gj <= 0))
    opp = ((gi <= 0) & (gj >= 0)) | ((gi >= 0) & (gj <= 0))
    cand = er & (mag > 0)
    pm = np.pad(mag, 1, mode="constant")
    at = lambda o: pm[1 + o[0]:1 + o[0] + R, 1 + o[1]:1 + o[1] + R]      # noqa: E731  (candidates never sit on the border)
    lm = np.zeros_like(cand)
    sector = np.zeros(cand.shape, dtype=np.int8)
    for n, (sm, i_big, plus, minus) in enumerate(SECTORS, 1):
        pts = cand & (same if sm else opp) & ((ai >= aj) if i_big else (ai <= aj))
        with np.errstate(divide="ignore", invalid="ignore"):
            w = (aj / ai) if i_big else (ai / aj)
            ok = (at(plus[1]) * w + at(plus[0]) * (1.0 - w) <= mag) & (at(minus[1]) * w + at(minus[0]) * (1.0 - w) <= mag)
        lm[pts] = ok[pts]
        sector[pts] = n
    return lm, sector


def hysteresis(low: np.ndarray, high: np.ndarray) -> np.ndarray:
    kept = np.zeros_like(low)
    stack = [(int(y), int(x)) for y, x in zip(*np.nonzero(high & low))]
    for y, x in stack:
        kept[y, x] = True
    while stack:
        y, x = stack.pop()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                yy, xx = y + dy, x + dx
                if 0 <= yy < low.shape[0] and 0 <= xx < low.shape[1] and low[yy, xx] and not kept[yy, xx]:
                    kept[yy, xx] = True
                    stack.append((yy, xx))
    return kept


def canny(gray: np.ndarray, valid: np.ndarray, sigma: float = 2.0):
    """-> (edge map, diagnostics)."""
    w, _ = gauss_table(sigma)
    m = np.where(valid, gray.astype(np.float64), 0.0)
    f = valid.astype(np.float64)
    gm = gauss_axis(gauss_axis(m, w, 0), w, 1)
    gf = gauss_axis(gauss_axis(f, w, 0), w, 1)
    s = gm / (gf + EPS)
    gi, gj = sobel(s, 0), sobel(s, 1)
    mag = np.sqrt(gi * gi + gj * gj)
    er = erode3(valid)
    lm, sector = nms(gi, gj, mag, er)
    low, high = lm & (mag >= LOW_T), lm & (mag >= HIGH_T)
    kept = hysteresis(low, high)
    return kept, dict(valid=valid, s=s, mag=mag, sector=sector, lm=lm, low=low, high=high, kept=kept)


def reference(frame: np.ndarray, det_masks: np.ndarray, boxes, sigma: float = 2.0):
    """frame uint8 [H, W, 3], det_masks uint8 [V, 1, H, W], boxes [V, 4] -> ({'img', 'gray', 'edge', 'mask'} float32, [diagnostics])."""
    V = det_masks.shape[0]
    out = {"img": np.zeros((V, 3, R, R), np.float32), "gray": np.zeros((V, 1, R, R), np.float32),
           "edge": np.zeros((V, 1, R, R), np.float32), "mask": np.zeros((V, 1, R, R), np.float32)}
    diags = []
    for v, (x0, y0, x1, y1) in enumerate(np.asarray(boxes).reshape(-1, 4).tolist()):
        if x1 <= x0 or y1 <= y0:
            diags.append(None)
            continue
        img = frame[y0:y1, x0:x1].copy()
        m = dilate(det_masks[v, 0, y0:y1, x0:x1])
        img[m == 255] = 255
        img = cv_host.resize_linear_u8(img, (R, R))
        m = cv_host.resize_linear_u8(m[:, :, None], (R, R))[:, :, 0]
        c = img.astype(np.int64)
        gray = ((3735 * c[..., 0] + 19235 * c[..., 1] + 9798 * c[..., 2] + 16384) >> 15).astype(np.uint8)
        hole = m > 0
        edge, d = canny(gray, ~hole, sigma)
        out["img"][v] = (img.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)
        out["gray"][v, 0] = gray.astype(np.float32) / np.float32(255)
        out["mask"][v, 0] = hole.astype(np.float32)
        out["edge"][v, 0] = edge.astype(np.float32)
        diags.append(d)
    return out, diags


def geodesic_reach(kept: np.ndarray, seeds: np.ndarray) -> int:
    """The largest 8-connected step count from the seed pixels to a kept pixel reached through kept pixels."""
    dist = np.full(kept.shape, -1, dtype=np.int64)
    front = [(int(y), int(x)) for y, x in zip(*np.nonzero(seeds & kept))]
    for y, x in front:
        dist[y, x] = 0
    far = 0
    while front:
        nxt = []
        for y, x in front:
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < kept.shape[0] and 0 <= xx < kept.shape[1] and kept[yy, xx] and dist[yy, xx] < 0:
                        dist[yy, xx] = dist[y, x] + 1
                        far = max(far, int(dist[yy, xx]))
                        nxt.append((yy, xx))
        front = nxt
    return far


def count_rejected_components(low: np.ndarray, kept: np.ndarray) -> int:
    """The number of 8-connected low components without a kept pixel."""
    left = low & ~kept
    n = 0
    while left.any():
        y, x = (int(a[0]) for a in np.nonzero(left))
        seed = np.zeros_like(left)
        seed[y, x] = True
        left &= ~hysteresis(left, seed)
        n += 1
    return n


# ---------------------------------------------------------------------------------------------- fixtures
def _texture(H: int, W: int, seed: int) -> np.ndarray:
    """Smooth plus texture: a low-frequency colour field, blocks of random contrast (edges at every scale the boxes are
    resized by) and a little noise."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W, 3))
    for c in range(3):
        img[..., c] = 110 + 50 * np.sin(xx / (17.0 + 5 * c) + c) * np.cos(yy / (23.0 - 3 * c))
    for _ in range(max(40, H * W // 120)):
        bw, bh = int(g.integers(4, max(8, W // 8))), int(g.integers(4, max(8, H // 6)))
        x0, y0 = int(g.integers(-bw // 2, W)), int(g.integers(-bh // 2, H))
        img[max(y0, 0):y0 + bh, max(x0, 0):x0 + bw] += g.uniform(-110, 110, 3)
    img += g.uniform(-4, 4, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def _blob(H, W, box, seed, touch="left", value=255) -> np.ndarray:
    """A frame-sized mask with an elliptical blob inside `box` that runs into the box border on the `touch` side."""
    x0, y0, x1, y1 = box
    bw, bh = x1 - x0, y1 - y0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cx = x0 + (0.2 * bw if touch == "left" else 0.55 * bw)
    cy = y0 + (0.85 * bh if touch == "bottom" else 0.5 * bh)
    m = (((xx - cx) / (0.3 * bw)) ** 2 + ((yy - cy) / (0.28 * bh)) ** 2 <= 1.0).astype(np.uint8) * value
    return m


def _serpentine(size: int = R):
    """A weak step edge (Canny magnitude between the two thresholds) along two interleaved Archimedean spirals that wind
    from the middle of the image to its border, and one strong spot on the outer end of one of them."""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    dy, dx = yy - (size / 2 - 0.5), xx - (size / 2 - 0.5)
    r, th = np.hypot(dy, dx), np.arctan2(dy, dx)
    pitch = 30.0
    ph = ((r - pitch * th / (2 * np.pi)) / pitch) % 1.0                      # 0..1 across one turn: stripes of half a pitch
    d = np.where(ph < 0.5, 0.25 - np.abs(ph - 0.25), np.abs(ph - 0.75) - 0.25) * pitch   # signed distance to the stripe border, px
    sy, sx = size / 2 - 0.5, size / 2 - 0.5 + 3.5 * pitch                    # on the stripe border of the outermost full turn
    step = 26.0 + 60.0 * np.exp(-((yy - sy) ** 2 + (xx - sx) ** 2) / (2 * 2.5 ** 2))   # locally a strong step
    img = 100.0 + step * np.clip(0.5 + d, 0.0, 1.0) * (r > 14)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def fixtures():
    """Two frames (96 x 160 and 300 x 420) with V = 6 vehicles each -> list of dicts 'name', 'frame', 'det_masks', 'boxes',
    'nondegenerate' (per vehicle: Canny has something to find), 'serpentine' (vehicle index or None)."""
    out = []
    # ---- 96 x 160
    H, W = 96, 160
    frame = _texture(H, W, 1)
    boxes = [(21, 30, 74, 67),       # odd-sized 53 x 37, a blob running into the left border
             (0, 0, 61, 45),         # clipped at the left and the top frame border
             (100, 50, 105, 57),     # 5 x 7: smaller than the structuring element
             (70, 10, 150, 70),      # no hole at all: Canny over the whole image
             (10, 60, 60, 90),       # everything is hole
             (30, 20, 30, 50)]       # zero extent
    det = np.zeros((6, 1, H, W), np.uint8)
    det[0, 0] = _blob(H, W, boxes[0], 0, "left")
    det[1, 0] = _blob(H, W, boxes[1], 1, "bottom")
    det[2, 0, 52:55, 101:103] = 255
    det[4, 0] = 255
    det[5, 0] = 255
    out.append(dict(name="96x160", frame=frame, det_masks=det, boxes=np.asarray(boxes, np.int64),
                    nondegenerate=[True, True, False, True, False, False], serpentine=None))
    # ---- 300 x 420
    H, W = 300, 420
    frame = _texture(H, W, 2)
    boxes = [(80, 20, 80 + R, 20 + R),   # the serpentine, exactly 256 x 256 (resize = copy), no hole
             (60, 150, 360, 270),        # 300 x 120: wider than 256, lower than 256
             (300, 5, 400, 295),         # 100 x 290: the other way round
             (333, 211, 420, 300),       # 87 x 89, clipped at the right and the bottom frame border
             (5, 5, 420, 300),           # larger than 256 both ways, no hole
             (10, 200, 70, 290)]         # everything is hole
    frame[20:20 + R, 80:80 + R] = _serpentine()[:, :, None]
    det = np.zeros((6, 1, H, W), np.uint8)
    det[1, 0] = _blob(H, W, boxes[1], 2, "left")
    det[1, 0, 160:200, 250:300] = 128                                        # non-zero but not 255: a hole that is not whitened
    det[2, 0] = _blob(H, W, boxes[2], 3, "bottom")
    det[3, 0] = _blob(H, W, boxes[3], 4, "left")
    det[5, 0] = 255
    out.append(dict(name="300x420", frame=frame, det_masks=det, boxes=np.asarray(boxes, np.int64),
                    nondegenerate=[True, True, True, True, True, False], serpentine=0))
    return out
