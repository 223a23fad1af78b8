"""The input cases the image-metric tests share (CPU: host twin against the oracle; GPU: kernel against the host twin): pairs
(a, b) of uint8 [B, H, W, C] arrays from fixed numpy seeds, and the expensive references (oracle.ssim per row, the host
twin's table), computed once per process and handed out as read-only arrays."""
import numpy as np

CASES = ("ragged", "one_window", "flat", "border", "identical", "far", "product")
SHAPES = {"ragged": (3, 43, 37, 3), "one_window": (2, 11, 11, 1), "flat": (1, 64, 64, 3), "border": (2, 40, 40, 3),
          "identical": (2, 32, 48, 3), "far": (2, 32, 32, 3), "product": (2, 256, 256, 3)}


def _texture(rng, shape):
    """Block-constant texture (8 x 8 blocks) plus noise."""
    B, H, W, C = shape
    blocks = rng.integers(0, 256, size=(B, (H + 7) // 8, (W + 7) // 8, C))
    base = np.repeat(np.repeat(blocks, 8, axis=1), 8, axis=2)[:, :H, :W]
    return np.clip(base + rng.integers(-12, 13, size=shape), 0, 255).astype(np.uint8)


def _plus_minus_one(rng, a):
    """b = a +- 1 on 30 % of the values."""
    step = np.where(rng.random(a.shape) < 0.3, rng.choice(np.array([-1, 1]), size=a.shape), 0)
    return np.clip(a.astype(np.int64) + step, 0, 255).astype(np.uint8)


def build(name):
    shape = SHAPES[name]
    rng = np.random.default_rng(1000 + CASES.index(name))
    if name in ("ragged", "one_window", "product"):
        a = _texture(rng, shape)
        return a, _plus_minus_one(rng, a)
    if name == "flat":
        a = np.full(shape, 250, dtype=np.uint8)
        b = a.copy()
        b[0, ::7, ::5, :] = 249
        return a, b
    if name == "border":
        a = rng.integers(0, 256, size=shape).astype(np.uint8)
        b = a.copy()
        H, W = shape[1:3]
        for r in range(shape[0]):
            for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)) + tuple((y, 7 + 5 * y + r) for y in range(5)):
                b[r, y, x] = a[r, y, x] ^ 0x55                    # every channel differs (by 1 .. 255)
        return a, b
    if name == "identical":
        a = rng.integers(0, 256, size=shape).astype(np.uint8)
        return a, a.copy()
    if name == "far":
        return np.zeros(shape, dtype=np.uint8), np.full(shape, 255, dtype=np.uint8)
    raise KeyError(name)


_CACHE = {}


def _frozen(x):
    x.setflags(write=False)
    return x


def pair(name):
    if ("pair", name) not in _CACHE:
        a, b = build(name)
        _CACHE["pair", name] = (_frozen(a), _frozen(b))
    return _CACHE["pair", name]


def oracle_rows(name):
    """oracle.ssim of every row, float64 [B]."""
    if ("oracle", name) not in _CACHE:
        import oracle
        a, b = pair(name)
        _CACHE["oracle", name] = _frozen(np.array([oracle.ssim(a[r].copy(), b[r].copy()) for r in range(a.shape[0])], dtype=np.float64))
    return _CACHE["oracle", name]


def host_table(name):
    """The host twin's float64 [B, 6] table."""
    if ("host", name) not in _CACHE:
        from future_urban_scene_generation_amd import ops
        a, b = pair(name)
        _CACHE["host", name] = _frozen(ops.image_metrics_host(a, b))
    return _CACHE["host", name]


def numpy_integers(a, b):
    """max_abs, n_diff, sse per row by numpy, int64 [B] each."""
    d = np.abs(a.astype(np.int64) - b.astype(np.int64)).reshape(a.shape[0], -1)
    return d.max(axis=1), (d != 0).sum(axis=1), (d * d).sum(axis=1)
