"""Sweep of the elementwise, layout and row-split sum kernels (csrc/elementwise.hip) - a helper module of the tests, not a
conftest.  Plain numpy / torch on the CPU, importable without a GPU.

References.  Every op is restated from its formula in include/fusg.h, on logical [B, C, H, W] numpy arrays:
  maxpool2, upsample2_add, copy4d (as the whole physical destination buffer), add4d, space/depth_to_space2 (DCR), ec_inputs,
  to_image_u8, merge_u8      numpy float32, op by op in the documented order (numpy rounds every op to fp32: no contraction)
  argmax_hw                  integers
  hshift_sum                 the fp32 emulation acc = bias; for kx ascending: if valid: acc += t[...]
  affine_act                 float64
and judged by (tests/test_gpu_eltwise_sweep.py)
  same_bits                  every op but affine_act and the transcendental activations (any NaN equals any NaN)
  affine_act NONE / RELU     |got - ref64| <= 1 fp32 ulp.  Without a residual that is the ulp of the reference: one fmaf
                             rounding (1/2 ulp) against a reference rounded twice (fp64, then the comparison).  With a residual
                             the kernel rounds twice, v = fl(fma) and fl(v + res), each by half an ulp of its own result, so the
                             ulp is taken at max(|act(x*scale + shift)|, |ref|): 1/2 ulp(v) + 1/2 ulp(out) <= that ulp.
  TANH / SIGMOID / TANH01    absolute error against float64 under a bar that is four times what torch's own float32 evaluation
                             of the same formula shows on the same case inputs (device libm is specified to a few ulp where
                             the host's is about one).  Measured by measure_act_error() on the CPU:
                                 affine_act   2.91e-07 (the whole formula: the fp32 argument and the residual add round too)
                                                                          -> ACT_BAR_AFFINE = 1.16e-06
                                 hshift_sum   8.85e-08 (the activation alone, of the exact sums)
                                                                          -> ACT_BAR_HSHIFT = 3.54e-07
                             (tests/test_eltwise_sweep_cpu.py re-measures and holds the record to within a factor of two).
                             Observed on the MI355X: 2.91e-07 and 8.85e-08, the host's own figures (the worst elements are
                             those where the fp32 argument is furthest off); affine_act NONE / RELU at most 0.998 ulp.

`embed` places a logical tensor inside a wider buffer.  A destination's surroundings hold CANARY, a fixed bit pattern, and
`outside_unchanged` compares everything outside the view as integers after the launch.  A source's surroundings hold NaN, so a
stray read poisons the result (+3e38 for maxpool2: it wins every window it strays into, and leaves NaN to the cases that
plant one).

`hshift_route`, `copy_route` and `hshift_accepts` restate the host's routing and the accepted parameters of fusg_hshift_sum."""
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

NONE, RELU, TANH, SIGMOID, TANH01 = 0, 1, 2, 3, 4           # FUSG_ACT_* (include/fusg.h)
ACTS = (NONE, RELU, TANH, SIGMOID, TANH01)
EXACT_ACTS = (NONE, RELU)
PAD_ZERO, PAD_REFLECT = 0, 1

CANARY = 0x4B3C2D1E             # destination surroundings, as int32 (the float 12332318.0)
CANARY_U8 = 0xA5
NAN = float("nan")
HUGE = 3e38

GRID_CAP = 16384 * 256          # threads of a capped launch (affine_act, maxpool2, upsample2_add): more work takes the stride

ACT_ERR_AFFINE = 2.91e-07       # measured: torch float32 against float64 on the transcendental cases (measure_act_error)
ACT_ERR_HSHIFT = 8.85e-08
ACT_BAR_AFFINE = 4 * ACT_ERR_AFFINE
ACT_BAR_HSHIFT = 4 * ACT_ERR_HSHIFT


def rng(tag: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(tag.encode()))


def randn(g, *shape) -> np.ndarray:
    return g.standard_normal(shape, dtype=np.float32)


def f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- embedding ---------------------------------------------------------------------------------------------------------------
def _fill(buf: torch.Tensor, fill) -> torch.Tensor:
    if isinstance(fill, int) and buf.dtype == torch.float32:
        buf.view(torch.int32).fill_(fill)
    else:
        buf.fill_(fill)
    return buf


def embed(view_shape, pitch, c_off=0, fill=NAN, dtype=torch.float32):
    """(view, buf): a logical [B, C, H, W] view at channel offset c_off of a fresh NHWC buffer [B, H, W, pitch] that holds
    `fill` (a float, or an int taken as a bit pattern) everywhere."""
    b, c, h, w = view_shape
    assert c_off + c <= pitch, (view_shape, pitch, c_off)
    buf = _fill(torch.empty((b, h, w, pitch), dtype=dtype), fill)
    return buf.permute(0, 3, 1, 2)[:, c_off:c_off + c], buf


def embed_nchw(view_shape, margin=64, fill=CANARY, dtype=torch.float32):
    """(view, buf): a contiguous NCHW view with `margin` elements of `fill` before and after it in a flat buffer."""
    n = int(np.prod(view_shape))
    buf = _fill(torch.empty(n + 2 * margin, dtype=dtype), fill)
    return buf[margin:margin + n].view(*view_shape), buf


def put(view: torch.Tensor, a) -> torch.Tensor:
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


def rebase(view: torch.Tensor, other_buf: torch.Tensor) -> torch.Tensor:
    """The same view (sizes, strides, offset) on another buffer of the same layout, e.g. the copy on the device."""
    return other_buf.as_strided(view.shape, view.stride(), view.storage_offset())


def _ints(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def outside_unchanged(view: torch.Tensor, before: torch.Tensor, after: torch.Tensor) -> bool:
    """Is every element of `after` that lies outside the view bit-equal to `before` (both whole buffers, on the CPU)?"""
    expect = before.clone()
    rebase(view, expect).copy_(rebase(view, after))
    return bool(torch.equal(_ints(expect), _ints(after)))


def same_bits(got, ref) -> bool:
    """Bit equality of two arrays of one dtype; for floats any NaN equals any NaN (the payload is not part of the contract)."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    if got.dtype != np.float32:
        return bool(np.array_equal(got, ref))
    gn, rn = np.isnan(got), np.isnan(ref)
    return bool(np.array_equal(gn, rn) and np.array_equal(got.view(np.int32)[~gn], ref.view(np.int32)[~rn]))


def ulp32(a) -> np.ndarray:
    """The fp32 ulp at |a| (float64 in, float64 out)."""
    return np.spacing(np.abs(np.asarray(a, np.float64)).astype(np.float32)).astype(np.float64)


# ---- references --------------------------------------------------------------------------------------------------------------
def act64(v, act: int) -> np.ndarray:
    v = np.asarray(v, np.float64)
    if act == RELU:
        return np.maximum(v, 0.0)
    if act == TANH:
        return np.tanh(v)
    if act == SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    if act == TANH01:
        return (np.tanh(v) + 1.0) / 2.0
    return v


def act_torch32(v: torch.Tensor, act: int) -> torch.Tensor:
    """The activation as torch evaluates it in float32 (the yardstick of the transcendental bar, never a reference)."""
    if act == RELU:
        return torch.relu(v)
    if act == TANH:
        return torch.tanh(v)
    if act == SIGMOID:
        return torch.sigmoid(v)
    if act == TANH01:
        return (torch.tanh(v) + 1.0) / 2.0
    return v


def ref_affine_act(x, scale, shift, act, res):
    """(ref, pre) in float64: ref = act(x*scale[b,c] + shift[b,c]) + res, pre = the activated term alone.  scale/shift are
    [B, C] or None (identity), res [B, C, H, W] or None."""
    v = np.asarray(x, np.float64)
    if scale is not None:
        v = v * np.asarray(scale, np.float64)[:, :, None, None] + np.asarray(shift, np.float64)[:, :, None, None]
    pre = act64(v, act)
    return (pre if res is None else pre + np.asarray(res, np.float64)), pre


def ref_maxpool2(x, drop_nan=False):
    x = f32(x)
    a, b, c, d = x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]
    mx = np.fmax if drop_nan else np.maximum                 # np.maximum hands a NaN on, np.fmax drops it (the mutant)
    return mx(mx(a, b), mx(c, d))


def ref_upsample2_add(low, up1, wrong_row=False):
    low, up1 = f32(low), f32(up1)
    b, c, h, w = up1.shape
    if not wrong_row:
        return up1 + low.repeat(2, axis=2).repeat(2, axis=3)
    # the mutant: the low-resolution row pitch taken as W instead of W >> 1 (indices past the image wrap)
    flat = low.transpose(0, 2, 3, 1).reshape(b, -1, c)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    idx = ((y >> 1) * w + (x >> 1)) % flat.shape[1]
    return up1 + flat[:, idx].transpose(0, 3, 1, 2)


def ref_copy4d_buffer(src, pitch, c_off, fill, fill_to_pitch=False):
    """The whole destination buffer [B, H, W, pitch] as int32 after fusg_copy4d into a CANARY-filled buffer: the source's
    channels at c_off, zeros in [C, fill) behind them, everything else untouched."""
    src = f32(src)
    b, c, h, w = src.shape
    buf = np.full((b, h, w, pitch), CANARY, np.int32)
    fbuf = buf.view(np.float32)
    fbuf[..., c_off:c_off + c] = src.transpose(0, 2, 3, 1)
    end = pitch - c_off if fill_to_pitch else fill
    if end > c:
        fbuf[..., c_off + c:c_off + end] = 0.0
    return buf


def ref_add4d(a, b):
    return f32(a) + f32(b)


def ref_s2d(x, swap_ij=False, crd=False):
    """dst[b, (2i+j)*C + c, h, w] = x[b, c, 2h+i, 2w+j]   (DCR; CRD would be c*4 + 2i + j)"""
    x = f32(x)
    b, c, h, w = x.shape
    out = np.empty((b, 4 * c, h // 2, w // 2), np.float32)
    for i in range(2):
        for j in range(2):
            blk = x[:, :, j::2, i::2] if swap_ij else x[:, :, i::2, j::2]
            if crd:
                out[:, 2 * i + j::4] = blk
            else:
                out[:, (2 * i + j) * c:(2 * i + j + 1) * c] = blk
    return out


def ref_d2s(x, swap_ij=False, crd=False):
    """dst[b, c, 2h+i, 2w+j] = x[b, (2i+j)*C + c, h, w],  C = x.c / 4"""
    x = f32(x)
    b, c4, h, w = x.shape
    c = c4 // 4
    out = np.empty((b, c, 2 * h, 2 * w), np.float32)
    for i in range(2):
        for j in range(2):
            blk = x[:, 2 * i + j::4] if crd else x[:, (2 * i + j) * c:(2 * i + j + 1) * c]
            if swap_ij:
                out[:, :, j::2, i::2] = blk
            else:
                out[:, :, i::2, j::2] = blk
    return out


def ref_ec_inputs(images, edges, masks, mode):
    """[B, 4, H, W]: mode 0 cat(img*(1-m)+m, edge*(1-m), m, 0); mode 1 cat(img*(1-m)+m (3 channels), edge)."""
    img, e, m = f32(images), f32(edges), f32(masks)
    one = np.float32(1.0)
    if mode == 0:
        return np.concatenate([img * (one - m) + m, e * (one - m), m, np.zeros_like(m)], axis=1)
    return np.concatenate([img * (one - m) + m, e], axis=1)


def ref_to_image_u8(x, nearest=False):
    """uint8 [B, H, W, C] = trunc(clip((x+1)/2*255, 0, 255)) in float32."""
    with np.errstate(over="ignore"):                         # (3e38 overflows to +inf, which clips to 255 like on the device)
        v = (f32(x) + np.float32(1.0)) / np.float32(2.0) * np.float32(255.0)
    v = np.clip(v, np.float32(0.0), np.float32(255.0))
    if nearest:
        v = np.rint(v)
    return v.astype(np.uint8).transpose(0, 2, 3, 1)


def ref_merge_u8(out, img, mask, fused=False):
    """uint8 [B, H, W, C] = trunc(clip((out*m + img*(1-m))*255, 0, 255)) in float32, every op rounded."""
    o, im, m = f32(out), f32(img), f32(mask)
    t = im * (np.float32(1.0) - m)
    if fused:        # the mutant: out*m + t as one fma (the exact product fits a double; one rounding to fp32 after the add)
        s = (o.astype(np.float64) * m.astype(np.float64) + t.astype(np.float64)).astype(np.float32)
    else:
        s = o * m + t
    v = np.clip(s * np.float32(255.0), np.float32(0.0), np.float32(255.0))
    return v.astype(np.uint8).transpose(0, 2, 3, 1)


def ref_argmax_hw(x, last=False):
    """int32 [B, C]: row-major first-occurrence argmax over H*W (no NaN: unspecified, include/fusg.h)."""
    x = f32(x)
    b, c, h, w = x.shape
    flat = x.reshape(b, c, -1)
    if last:
        return (h * w - 1 - flat[:, :, ::-1].argmax(axis=2)).astype(np.int32)
    return flat.argmax(axis=2).astype(np.int32)


def ref_hshift_sum(t, bias, kw, pad, pad_mode, cout, mutant=None):
    """The pre-activation sums [B, cout, H, W] in float32, tap by tap as the kernels add them:
        acc = bias[co]; for kx ascending: xx = pad_x(x + kx - pad); if valid: acc += t[b, y, xx, co*kw + kx]
    t is [B, H, W, >= cout*kw].  NONE / RELU of it are exact; the other activations are judged from it in float64."""
    t, bias = f32(t), f32(bias)
    b, h, w, _ = t.shape
    acc = np.empty((b, cout, h, w), np.float32)
    acc[:] = bias.reshape(1, cout, 1, 1)
    x = np.arange(w)
    for kx in range(kw):
        xx = x + kx - pad
        if pad_mode == PAD_REFLECT:
            hi = 2 * w - (1 if mutant == "reflect" else 2) - xx
            xx = np.where(xx < 0, -xx, np.where(xx >= w, hi, xx))
        ok = (xx >= 0) & (xx < w)
        if mutant == "seam":                                   # a tap in the neighbouring 256-pixel segment is lost
            ok &= (xx // 256) == (x // 256)
        for co in range(cout):
            acc[:, co][:, :, ok] += t[:, :, xx[ok], co * kw + kx]
    return acc


# ---- routing and the accepted parameters, restated ----------------------------------------------------------------------------
def hshift_accepts(kw, pad, pad_mode, w) -> bool:
    """fusg_hshift_sum's contract (include/fusg.h): the window holds its own pixel (kw-1-pad >= 0), pad < W, and under reflect
    padding the right overshoot kw-1-pad < W, so that 2W-2-xx >= 0 like -xx <= pad < W on the left."""
    reach = kw - 1 - pad
    return 1 <= kw <= 15 and 0 <= pad < w and reach >= 0 and (pad_mode == PAD_ZERO or reach < w)


def hshift_route(pitch, pad, w, aligned=True, kw=None) -> str:
    """"lds" or "direct" (hshift_sum_impl).  The LDS tile is a segment's 256 pixels +- pad: it needs a pitch of at most 32
    floats, W > 2*pad, and a window reaching no further right than pad (kw-1 <= 2*pad; kw defaults to 2*pad+1)."""
    kw = 2 * pad + 1 if kw is None else kw
    return "lds" if (pitch % 4 == 0 and pitch <= 32 and pad <= 16 and kw - 1 - pad <= pad and w > 2 * pad and aligned) else "direct"


def copy_route(src_nchw_contiguous, dst_nhwc, c, fill, pitch) -> str:
    """"transpose" (nchw_to_nhwc_kernel, the LDS transpose behind ops.as_nhwc) or "generic" (copy4d_impl)."""
    return "transpose" if (src_nchw_contiguous and dst_nhwc and c <= 32 and fill <= 32 and fill <= pitch) else "generic"


def over_cap(float4s: int) -> bool:
    return float4s > GRID_CAP


# ---- cases -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    tag: str
    p: dict = field(hash=False, compare=False)

    def __getattr__(self, k):
        try:
            return self.p[k]
        except KeyError:
            raise AttributeError(k)

    def __repr__(self):
        return self.tag


def case(tag, **p) -> Case:
    return Case(tag, p)


def source(tag, a, pitch, c_off=0, fill=NAN):
    """A logical float32 array as an NHWC slice (view, buf) whose surroundings hold `fill`."""
    v, buf = embed(a.shape, pitch, c_off, fill)
    put(v, f32(a))
    return v, buf


# affine_act ....................................................................................................................
def affine_cases():
    out = []
    for c in (4, 12, 64):
        for act in ACTS:
            for res in (False, True):
                # the three scale forms and the two destinations rotate through the cross product (each occurs per C)
                k = len(out)
                sform = ("null", "tight", "wide")[k % 3]
                out.append(case(f"affine-c{c}-act{act}-res{int(res)}-{sform}-{'slice' if k // 2 % 2 else 'tight'}", B=2, C=c, H=3, W=5,
                                act=act, res=res, scale=sform, dst_off=4 if k // 2 % 2 else 0, big=False))
    out.append(case("affine-over-cap", B=1, C=64, H=514, W=512, act=RELU, res=False, scale="tight", dst_off=0, big=True))
    return out


def affine_inputs(c: Case):
    """x (pitch C+4; tight for the large case), scale/shift flat with their row stride, residual (pitch C+8), as CPU tensors."""
    g = rng(c.tag)
    shape = (c.B, c.C, c.H, c.W)
    d = {"x": source(c.tag, randn(g, *shape) * 2, c.C if c.big else c.C + 4)}
    d["bstride"] = {"null": 0, "tight": c.C, "wide": c.C + 8}[c.scale]
    if c.scale != "null":
        for name, a in (("scale", randn(g, c.B, c.C) + 1.5), ("shift", randn(g, c.B, c.C))):
            flat = torch.full((c.B, d["bstride"]), NAN)
            flat[:, :c.C] = torch.from_numpy(f32(a))
            d[name] = flat
    if c.res:
        d["res"] = source(c.tag, randn(g, *shape), c.C + 8, 4)
    return d


def affine_logical(d, c: Case, pitch_is_c=False, ignore_bstride=False):
    """The operands the kernel must read (x, scale, shift, res as numpy; absent: None) - or, for the two mutants, what a
    kernel reads that takes C for the pixel pitch of x, or C for the row stride of scale/shift."""
    xv, xbuf = d["x"]
    if pitch_is_c:
        x = xbuf.flatten()[xv.storage_offset():][:c.B * c.H * c.W * c.C].view(c.B, c.H, c.W, c.C).permute(0, 3, 1, 2).numpy()
    else:
        x = xv.numpy()
    sc = sh = None
    if c.scale != "null":
        if ignore_bstride:
            sc, sh = (d[k].flatten()[:c.B * c.C].view(c.B, c.C).numpy() for k in ("scale", "shift"))
        else:
            sc, sh = d["scale"][:, :c.C].numpy(), d["shift"][:, :c.C].numpy()
    return x, sc, sh, (d["res"][0].numpy() if c.res else None)


# maxpool2 / upsample2_add ........................................................................................................
def pool_cases():
    out = [case(f"pool-c{c}-{kind}-off{off}", C=c, B=2, Ho=3, Wo=5, kind=kind, dst_off=off, big=False)
           for c in (4, 20) for kind, off in (("plain", 0), ("inf", 4), ("nan", 0), ("nan", 4))]
    out.append(case("pool-over-cap", C=4, B=1, Ho=2050, Wo=2048, kind="plain", dst_off=0, big=True))
    return out


def pool_inputs(c: Case):
    g = rng(c.tag)
    x = randn(g, c.B, c.C, 2 * c.Ho, 2 * c.Wo)
    if c.kind in ("inf", "nan"):
        x[:, :, 0:2, 0:2] = -np.inf                            # a window of -inf alone, and -inf beside finite values
        x[:, :, 2, 5] = -np.inf
    if c.kind == "nan":
        for k, (y, xx) in enumerate(((0, 2), (1, 5), (2, 6), (3, 9), (4, 0), (5, 1))):     # every position of a window
            x[k % c.B, k % c.C, y, xx] = np.nan
    return {"x": source(c.tag, x, c.C if c.big else c.C + 4, 0, HUGE)}


def upsample_cases():
    out = [case(f"up-c{c}-{kind}-off{off}", C=c, B=2, H=6, W=10, kind=kind, dst_off=off, big=False)
           for c in (4, 20) for kind, off in (("plain", 0), ("inf", 4))]
    out.append(case("up-over-cap", C=4, B=1, H=2050, W=2048, kind="plain", dst_off=0, big=True))
    return out


def upsample_inputs(c: Case):
    g = rng(c.tag)
    low, up1 = randn(g, c.B, c.C, c.H // 2, c.W // 2), randn(g, c.B, c.C, c.H, c.W)
    if c.kind == "inf":
        low[:, :, 0, 0] = -np.inf
        up1[:, :, 2, 3] = -np.inf
    return {"low": source(c.tag, low, c.C if c.big else c.C + 4), "up1": source(c.tag, up1, c.C if c.big else c.C + 8, 4 * (not c.big))}


# copy4d / add4d ................................................................................................................
def copy_cases():
    out = []
    for c in (1, 3, 5, 32, 33):
        for h, w in ((5, 7), (16, 16), (1, 257), (12, 25)):
            for fill in (0, (c + 3) // 4 * 4, 32):
                cd = max(c, fill)
                off = 4 * ((len(out) // 3) % 2)
                out.append(case(f"copy-c{c}-{h}x{w}-fill{fill}-off{off}", B=2, C=c, H=h, W=w, fill=fill, c_off=off,
                                pitch=off + (cd + 3) // 4 * 4 + 4, src="nchw", dst="nhwc"))
    out.append(case("copy-batch-sliced-src", B=2, C=3, H=5, W=7, fill=4, c_off=0, pitch=8, src="batch_sliced", dst="nhwc"))
    out.append(case("copy-nhwc-slice-to-nchw", B=2, C=5, H=12, W=25, fill=0, c_off=0, pitch=0, src="nhwc_slice", dst="nchw"))
    return out


def copy_inputs(c: Case):
    """The source view on the CPU: contiguous NCHW, every other image of a contiguous NCHW batch, or an NHWC slice."""
    a = randn(rng(c.tag), c.B, c.C, c.H, c.W)
    if c.src == "nchw":
        return torch.from_numpy(a)
    if c.src == "batch_sliced":
        big = torch.full((2 * c.B, c.C, c.H, c.W), NAN)
        big[::2] = torch.from_numpy(a)
        return big[::2]
    return source(c.tag, a, c.C + 7, 4)[0]


def copy_route_of(c: Case) -> str:
    return copy_route(c.src == "nchw", c.dst == "nhwc", c.C, c.fill, c.pitch)


# s2d / d2s .....................................................................................................................
def s2d_cases():
    return [case(f"{op}-c{c}-off{off}", op=op, B=2, C=c, H=4, W=6, dst_off=off)
            for op in ("s2d", "d2s") for c in (4, 12, 32) for off in (0, 4)]


def s2d_inputs(c: Case):
    """s2d: x [B, C, 2H, 2W] -> [B, 4C, H, W];  d2s: x [B, 4C, H, W] -> [B, C, 2H, 2W].  Source pitch > its channels."""
    shape = (c.B, c.C, 2 * c.H, 2 * c.W) if c.op == "s2d" else (c.B, 4 * c.C, c.H, c.W)
    return {"x": source(c.tag, randn(rng(c.tag), *shape), shape[1] + 8, 4)}


# ec_inputs .....................................................................................................................
def ec_cases():
    return [case(f"ec-mode{mode}-{mask}-pitch{pitch}-{lay}", mode=mode, mask=mask, pitch=pitch, lay=lay, B=2, H=5, W=7)
            for mode in (0, 1) for mask in ("binary", "fractional") for pitch, lay in ((4, "nchw"), (8, "strided"))]


def ec_inputs_of(c: Case):
    """images [B,1|3,H,W], edges, masks [B,1,H,W] as CPU views: contiguous NCHW, or (strided) channel slices of NHWC buffers
    for the images and every other column of a wider map for the edges and masks."""
    g = rng(c.tag)
    ci = 1 if c.mode == 0 else 3
    img, e = g.random((c.B, ci, c.H, c.W), dtype=np.float32), g.random((c.B, 1, c.H, c.W), dtype=np.float32)
    m = g.random((c.B, 1, c.H, c.W), dtype=np.float32)
    if c.mask == "binary":
        m = (m > 0.5).astype(np.float32)
    if c.lay == "nchw":
        return tuple(torch.from_numpy(a) for a in (img, e, m))
    views = [source(c.tag, img, ci + 2, 1)[0]]
    for a in (e, m):
        wide = torch.full((c.B, 1, c.H, 2 * c.W), NAN)
        wide[..., ::2] = torch.from_numpy(a)
        views.append(wide[..., ::2])
    return tuple(views)


# hshift_sum ....................................................................................................................
HSHIFT_CONFIGS = ((3, 7, 3, 24), (1, 7, 3, 8), (2, 15, 7, 32), (1, 1, 0, 4), (4, 9, 4, 36))       # cout, kw, pad, pitch
# beyond kw = 2*pad + 1 (what the packers pass): windows that reach further right than left go the direct way, at a W whose
# tile they would leave; windows the kernels cannot index are turned away (hshift_rejects)
HSHIFT_LOPSIDED = ((2, 7, 1, 16), (1, 4, 0, 4), (2, 6, 3, 12))


def hshift_cases():
    out = []
    for cout, kw, pad, pitch in HSHIFT_CONFIGS:
        for w in sorted({2 * pad, 2 * pad + 1, 20, 256, 257, 256 + pad - 1, 300, 513}):
            for pm in (PAD_ZERO, PAD_REFLECT):
                if hshift_accepts(kw, pad, pm, w):
                    out.append(case(f"hshift-co{cout}-kw{kw}-pad{pad}-p{pitch}-w{w}-pm{pm}", cout=cout, kw=kw, pad=pad,
                                    pitch=pitch, B=2, H=2, W=w, pm=pm))
    for cout, kw, pad, pitch in HSHIFT_LOPSIDED:
        for w in (20, 300):
            for pm in (PAD_ZERO, PAD_REFLECT):
                assert hshift_accepts(kw, pad, pm, w)
                out.append(case(f"hshift-lopsided-co{cout}-kw{kw}-pad{pad}-p{pitch}-w{w}-pm{pm}", cout=cout, kw=kw, pad=pad,
                                pitch=pitch, B=2, H=2, W=w, pm=pm))
    return out


def hshift_rejects():
    """(kw, pad, pad_mode, W, cout, pitch) the ABI must turn away: hshift_accepts is False for each."""
    return [(3, 3, PAD_ZERO, 20, 1, 4), (3, 3, PAD_REFLECT, 20, 1, 4),         # the window ends left of its own pixel
            (9, 1, PAD_REFLECT, 7, 1, 12), (15, 0, PAD_REFLECT, 14, 1, 16),    # the reflected overshoot leaves the row
            (7, 3, PAD_ZERO, 3, 1, 8), (16, 8, PAD_ZERO, 300, 1, 16), (0, 0, PAD_ZERO, 20, 1, 4)]     # pad >= W, kw > 15, kw < 1


def hshift_route_of(c: Case) -> str:
    return hshift_route(c.pitch, c.pad, c.W, True, c.kw)


def hshift_inputs(c: Case):
    """t as (view, buf): [B, cout*kw, H, W] inside an NHWC buffer of the case's pitch (NaN behind the channels), and the bias."""
    g = rng(c.tag)
    return source(c.tag, randn(g, c.B, c.cout * c.kw, c.H, c.W), c.pitch), f32(randn(g, c.cout))


# argmax_hw .....................................................................................................................
ARGMAX_KINDS = ("random", "tie_stride", "tie_neighbours", "last", "constant", "neg_inf")     # one channel each


def argmax_cases():
    return [case(f"argmax-{h}x{w}-{lay}", H=h, W=w, lay=lay, B=2)
            for h, w in ((1, 1), (1, 7), (5, 51), (16, 16), (1, 257), (64, 64)) for lay in ("nchw", "nhwc")]


def argmax_input(c: Case):
    """[B, 6, H, W]: a channel per ARGMAX_KINDS.  Values are small integers below the planted maxima, so ties abound."""
    g = rng(c.tag)
    hw = c.H * c.W
    x = g.integers(-5, 5, (c.B, len(ARGMAX_KINDS), hw)).astype(np.float32)
    for b in range(c.B):
        if hw > 256:                           # one thread's stride class: i and i + 256
            i = (37 + 100 * b) % (hw - 256)
            x[b, 1, [i, i + 256]] = 9.0
        else:                                  # (no such pair at this size: the first and the last pixel)
            x[b, 1, [0, hw - 1]] = 9.0
        j = (hw // 2 + b) % hw                 # neighbouring threads
        x[b, 2, [j, min(j + 1, hw - 1)]] = 9.0
        x[b, 3, hw - 1] = 9.0
        x[b, 4] = 2.5
        x[b, 5] = -np.inf
    x = x.reshape(c.B, -1, c.H, c.W)
    return torch.from_numpy(x) if c.lay == "nchw" else source(c.tag, x, 12, 2)[0]


# to_image_u8 / merge_u8 ..........................................................................................................
def _neighbours(v: np.ndarray) -> np.ndarray:
    """v and its +-1 and +-2 ulp neighbours (float32)."""
    out = [v]
    for direction in (np.float32(-np.inf), np.float32(np.inf)):
        a = v
        for _ in range(2):
            a = np.nextafter(a, direction)
            out.append(a)
    return np.concatenate(out)


def u8_cases():
    return [case(f"to_image-c{c}-{lay}", C=c, lay=lay, B=2, H=h, W=w) for c, h, w in ((1, 24, 28), (3, 14, 16)) for lay in ("nchw", "nhwc")]


def u8_input(c: Case):
    """Every truncation threshold k = 1..255 to the ulp (the fp32 nearest 2k/255 - 1 and its +-1, +-2 ulp neighbours), +-1,
    values beyond, -0.0, the infinities; the rest uniform in [-1.1, 1.1]."""
    k = np.arange(1, 256, dtype=np.float64)
    probes = np.concatenate([_neighbours((2 * k / 255 - 1).astype(np.float32)),
                             np.array([1, -1, 1.5, -1.5, 3e38, -3e38, -0.0, 0.0, np.inf, -np.inf], np.float32)])
    n = c.B * c.C * c.H * c.W
    assert probes.size <= n
    x = rng(c.tag).uniform(-1.1, 1.1, n).astype(np.float32)
    x[:probes.size] = probes
    x = x.reshape(c.B, c.C, c.H, c.W)
    return torch.from_numpy(x) if c.lay == "nchw" else source(c.tag, x, c.C + 3, 1)[0]


def merge_cases():
    return [case(f"merge-c{c}-{lay}", C=c, lay=lay, B=2, H=24, W=28) for c in (1, 3) for lay in ("nchw", "nhwc")]


def merge_inputs(c: Case):
    """out at k/255 +- ulp, the image equal to it or a neighbour (so that out*m + img*(1-m) lands on the threshold k/255 and the
    last bit of every rounding decides the byte), fractional masks; a block below 0 and above 1; a block of binary masks."""
    g = rng(c.tag)
    n = c.B * c.H * c.W
    k = g.integers(1, 256, (n, c.C)).astype(np.float64)
    o = (k / 255).astype(np.float32)
    step = g.integers(-1, 2, (n, c.C))
    o = np.where(step < 0, np.nextafter(o, np.float32(-1)), np.where(step > 0, np.nextafter(o, np.float32(2)), o))
    img = np.where(g.integers(0, 2, (n, c.C)) > 0, o, np.nextafter(o, np.float32(2)))
    m = g.random((n, 1), dtype=np.float32)
    q = n // 8
    o[:q] = g.uniform(-0.5, 1.5, (q, c.C)).astype(np.float32)                  # below 0 and above 1: clipped before the cast
    img[:q] = g.uniform(-0.5, 1.5, (q, c.C)).astype(np.float32)
    m[q:2 * q] = (m[q:2 * q] > 0.5).astype(np.float32)

    def lay(a, ch):
        a = f32(a.reshape(c.B, c.H, c.W, ch).transpose(0, 3, 1, 2))
        return torch.from_numpy(a) if c.lay == "nchw" else source(c.tag, a, ch + 5, 2)[0]
    return lay(o, c.C), lay(img, c.C), lay(m, 1)


# ---- the transcendental bar -----------------------------------------------------------------------------------------------------
def measure_act_error():
    """(affine, hshift): the largest absolute error of torch's float32 evaluation against float64 over the inputs of every
    small case with TANH / SIGMOID / TANH01 - the whole affine_act formula for the one, the activation of the emulated fp32
    sums for the other."""
    worst_a = worst_h = 0.0
    for c in affine_cases():
        if c.act in EXACT_ACTS or c.big:
            continue
        x, sc, sh, res = affine_logical(affine_inputs(c), c)
        ref, _ = ref_affine_act(x, sc, sh, c.act, res)
        v = torch.from_numpy(x)
        if sc is not None:
            v = v * torch.from_numpy(sc)[:, :, None, None] + torch.from_numpy(sh)[:, :, None, None]
        v = act_torch32(v, c.act)
        if res is not None:
            v = v + torch.from_numpy(res)
        worst_a = max(worst_a, float(np.abs(v.numpy().astype(np.float64) - ref).max()))
    for c in hshift_cases():
        (tv, _), bias = hshift_inputs(c)
        acc = ref_hshift_sum(tv.permute(0, 2, 3, 1).numpy(), bias, c.kw, c.pad, c.pm, c.cout)
        for act in (TANH, SIGMOID, TANH01):
            got = act_torch32(torch.from_numpy(acc), act).numpy().astype(np.float64)
            worst_h = max(worst_h, float(np.abs(got - act64(acc, act)).max()))
    return worst_a, worst_h
