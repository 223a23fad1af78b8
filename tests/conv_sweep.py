"""Routing sweep of fusg_conv2d - a helper module of the tests, not a conftest.  Plain torch on the CPU, importable without
a GPU.

The dispatcher of csrc/conv_igemm.hip (plan_impl, small_cfg, conv2d_impl) sends every launch to one of eleven kernel families
(include/fusg.h, FUSG_CONV_*; ops.last_conv_kernel()).  This module describes launches (`Case`), draws them from the space the
router admits (`edge_cases`: both sides of every eligibility condition, each row with the family it must land on per
precision; `random_cases`: a seeded draw), computes their float64 reference (`reference`) and judges a result with ONE
comparator (`norm_err` against `bar`):

    err = |got - ref| / (conv(|x'|, |w|) + |bias| + |res0| + |res1|)        elementwise, float64, x' = input after the pre-op

(the normalisation of test_gpu_ops.test_f16x3_scale_sweep).  `predict_family` restates the router's order and predicates, so
that the recorded expectations of the edge table are checked against it on the CPU and the GPU tests can name the family an
off-switch leads to."""
import math
import os
import sys
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from future_urban_scene_generation_amd import _lib as L       # noqa: E402
from future_urban_scene_generation_amd import pack            # noqa: E402

GEN_F32, GEN_F16X3, HALO, HALO_S2D, TAPUNIT, HALO_BF16 = 0, 1, 2, 3, 4, 5
POINTWISE, SMALL, HALO_F32, TAPUNIT_F32, TAPUNIT_BF16 = 7, 8, 9, 10, 11
FAMILIES = (GEN_F32, GEN_F16X3, HALO, HALO_S2D, TAPUNIT, HALO_BF16, POINTWISE, SMALL, HALO_F32, TAPUNIT_F32, TAPUNIT_BF16)
PRECISIONS = ("f32", "f16x3", "bf16")

# Bars of the comparator, by the family that RAN.  Exact-fp32 and split-fp16 families: 2^-18 (observed worst ~2.2e-6 at
# extreme operand scales, ~1e-7 at unit scale).  Single-pass bf16 families: bf16 keeps 8 significant bits, so rounding to
# nearest errs by up to 2^-8 per operand and a product of two rounded operands by (1 + 2^-8)^2 - 1 = 2^-7 + 2^-16 - the bound a
# correct kernel meets when one or two products dominate a sum (K = 4 and K = 72 layers: 4.2e-3 and 4.3e-3 > 2^-8, reproduced
# exactly by the bf16-operand emulation).  What the bf16 kernels compute beyond their operand rounding is pinned separately:
# against `reference_bf16` at BAR_FP32.
BAR_FP32 = 2.0 ** -18
BAR_BF16 = (1 + 2.0 ** -8) ** 2 - 1


def bar(family: int) -> float:
    return BAR_BF16 if family in (HALO_BF16, TAPUNIT_BF16) else BAR_FP32


PRE = {"none": L.PRE_NONE, "relu": L.PRE_RELU, "elu": L.PRE_ELU, "affine_relu": L.PRE_AFFINE_RELU, "affine": L.PRE_AFFINE}


@dataclass(frozen=True)
class Case:
    """One fusg_conv2d launch through ops.conv.  `pad_w` None: = pad.  `out`: "nhwc" (allocated by ops.conv), "slice"
    (channels out_c_off .. of a wider NHWC buffer), "nchw" (nchw_out), "misaligned" (an NHWC buffer 4 bytes off 16-byte
    alignment: no 16-byte epilogue).  `qwin` = (oy, ox, h, w): ops.conv(q_window=...).  `ksplit` 0: the planner's choice; 1:
    K whole (what the halo / tap-unit families need on grids too small for the planner to keep K whole).  `cin_pad` 32:
    pack_conv(cin_pad=32), the few-channel layers made halo-eligible.  `expect`: (f32, f16x3, bf16) families of an edge row."""
    tag: str
    B: int
    c0: int
    c1: int
    cout: int
    kh: int
    kw: int
    H: int
    W: int
    stride: int = 1
    pad: int = 0
    pad_w: Optional[int] = None
    dil: int = 1
    pm: int = L.PAD_ZERO
    ups: int = 0
    pre: str = "none"
    per_sample: bool = False
    act: int = L.ACT_NONE
    res: int = 0
    out: str = "nhwc"
    out_c_off: int = 0
    qwin: Optional[Tuple[int, int, int, int]] = None
    ksplit: int = 0
    cin_pad: int = 4
    sx: float = 1.0
    sw: float = 1.0
    seed: int = 0
    expect: Optional[Tuple[int, int, int]] = None

    @property
    def pw(self) -> int:
        return self.pad if self.pad_w is None else self.pad_w

    @property
    def cin(self) -> int:
        return self.c0 + self.c1

    @property
    def K(self) -> int:
        return self.cin * self.kh * self.kw

    def full_hw(self) -> Tuple[int, int]:
        hv, wv = self.H << self.ups, self.W << self.ups
        return ((hv + 2 * self.pad - self.dil * (self.kh - 1) - 1) // self.stride + 1,
                (wv + 2 * self.pw - self.dil * (self.kw - 1) - 1) // self.stride + 1)

    def q_hw(self) -> Tuple[int, int]:
        """The launch's output grid (the window's, for a q_window launch)."""
        return (self.qwin[2], self.qwin[3]) if self.qwin else self.full_hw()

    def mflop(self) -> float:
        ho, wo = self.full_hw()
        return 2.0 * self.B * ho * wo * self.cout * self.K / 1e6


def validate(c: Case) -> None:
    """Raise AssertionError unless the case is a legal launch of ops.conv AND a legal torch operation."""
    assert c.B >= 1 and c.c0 >= 1 and c.c1 >= 0 and c.cout >= 1 and c.kh >= 1 and c.kw >= 1, c
    assert c.stride in (1, 2) and c.dil >= 1 and c.ups in (0, 1) and c.pm in (L.PAD_ZERO, L.PAD_REFLECT, L.PAD_REPLICATE), c
    ho, wo = c.full_hw()
    assert ho >= 1 and wo >= 1, c
    hv, wv = c.H << c.ups, c.W << c.ups
    if c.pm == L.PAD_REFLECT:
        assert c.pad < hv and c.pw < wv, c                      # torch's reflect pad must be smaller than the size
    if c.pm != L.PAD_ZERO:
        assert c.pad <= hv - 1 and c.pw <= wv - 1, c            # (conv2d_impl's q-window check)
    if c.qwin:
        oy, ox, h, w = c.qwin
        assert c.pm == L.PAD_REPLICATE and 0 <= oy and oy + h <= ho and 0 <= ox and ox + w <= wo and h >= 1 and w >= 1, c
        assert c.out == "nhwc", c
    if c.out == "slice":
        assert c.out_c_off > 0, c
    assert c.pre in PRE and (not c.per_sample or c.pre.startswith("affine")), c
    assert 0 <= c.res <= 2 and c.act in (L.ACT_NONE, L.ACT_RELU, L.ACT_TANH, L.ACT_SIGMOID), c


# ---- packing, inputs, float64 reference ------------------------------------------------------------------------------------
def make_plan(c: Case, w: torch.Tensor, b: torch.Tensor) -> pack.ConvPlan:
    """pack.pack_conv, with a horizontal padding of its own when pad_w differs from pad (the K table then holds dx = kx dil -
    pad_w, as pack_conv_rowsplit does for its heads)."""
    split = (c.c0, c.c1) if c.c1 else None
    if c.pad_w is None:
        return pack.pack_conv(w, b, c_split=split, stride=c.stride, pad=c.pad, dil=c.dil, pad_mode=c.pm, upsample=c.ups,
                              cin_pad=c.cin_pad)
    taps = [(ky, kx, ky * c.dil - c.pad, kx * c.dil - c.pad_w) for ky in range(c.kh) for kx in range(c.kw)]
    panel, tab, c0k, c1k, k_pad, cout_pad = pack._pack_panel(w.float(), taps, split or (c.c0,), c.cin_pad)
    bb = torch.zeros(cout_pad)
    bb[:c.cout] = b
    return pack.ConvPlan(wpack=panel[None].contiguous(), bias=bb, ktab=tab[None].contiguous(), cout=c.cout, cout_pad=cout_pad,
                         k_pad=k_pad, c_split=split or (c.c0,), c0k=c0k, c1k=c1k, kh=c.kh, kw=c.kw, stride=c.stride, pad=c.pad,
                         dil=c.dil, pad_mode=c.pm, upsample=c.ups, nphase=1, flops_per_pixel=2.0 * c.cout * c.K, pad_w=c.pad_w)


# ---- the keywords of a case's ops.conv launch: ONE copy, for the GPU launch and for the router's dry run on CPU tensors ----
SENTINEL = 1234.5        # what every output buffer of the tests' own holds before the launch
GUARD = 64               # fp32 elements on each side of a "misaligned" output (a padded column, a pixel's channels past the end)


def launch_kwargs(c: Case, B: int, device, prec: str, pre=None, pre_bstride: int = 0, res=(), ksplit: Optional[int] = None,
                  tile: int = L.TILE_AUTO):
    """(kw, guard) of ops.conv(plan, x0, x1, **kw) for the case at batch B: `pre` the (scale, shift) of an affine pre-op in the K
    layout, `res` the residuals.  Output buffers of its own are filled with SENTINEL.  `guard` is None except for a "misaligned"
    output: then the flat buffer the output lies in, GUARD + 1 sentinels before it (an odd count: the output starts 4 bytes off
    16-byte alignment) and GUARD after it - `guard_elements` takes them back out after the launch."""
    from future_urban_scene_generation_amd import ops
    ho, wo = c.full_hw()
    kw = dict(pre_op=PRE[c.pre], act=c.act, precision=prec, ksplit=c.ksplit if ksplit is None else ksplit, tile=tile)
    if pre is not None:
        kw.update(pre=pre, pre_bstride=pre_bstride)
    for i, r in enumerate(res):
        kw["res%d" % i] = r
    out = guard = None
    if c.out == "nchw":
        kw["nchw_out"] = True
    elif c.out == "slice":
        out = ops.nhwc_empty(B, c.out_c_off + c.cout + 4, ho, wo, device)
        kw.update(out=out, out_c_off=c.out_c_off)
    elif c.out == "misaligned":
        n = B * ho * wo * c.cout
        guard = torch.empty(GUARD + 1 + n + GUARD, device=device)
        out = guard[GUARD + 1:GUARD + 1 + n].view(B, ho, wo, c.cout).permute(0, 3, 1, 2)
        assert out.data_ptr() % 16 != 0
        kw["out"] = out
    if c.qwin:
        out = ops.nhwc_empty(B, c.cout, ho, wo, device)
        kw.update(out=out, q_window=c.qwin)
    if guard is not None:
        guard.fill_(SENTINEL)
    elif out is not None:
        out.fill_(SENTINEL)
    return kw, guard


def guard_elements(guard: torch.Tensor) -> torch.Tensor:
    """The elements before and after the misaligned output inside `guard` (launch_kwargs), float64 on the CPU."""
    g = guard.cpu().double()
    return torch.cat([g[:GUARD + 1], g[-GUARD:]])


def d2s(t: torch.Tensor) -> torch.Tensor:
    """DepthToSpace(2), DCR order, of an NCHW-logical tensor: out[b, c, 2h + i, 2w + j] = in[b, (2i + j) C + c, h, w]."""
    b, c4, h, w = t.shape
    return t.reshape(b, 2, 2, c4 // 4, h, w).permute(0, 3, 4, 1, 5, 2).reshape(b, c4 // 4, 2 * h, 2 * w)


def s2d(t: torch.Tensor) -> torch.Tensor:
    """SpaceToDepth(2), the inverse of d2s."""
    b, c, h, w = t.shape
    return t.reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(b, 4 * c, h // 2, w // 2)


def inputs(c: Case) -> dict:
    """Seeded CPU float32 operands of the case: x0, x1, w, b, the pre-op's (scale, shift) per logical channel ([cin] or
    [B, cin]) and the residuals (output-shaped)."""
    g = torch.Generator().manual_seed(1000 + c.seed)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc     # noqa: E731
    ho, wo = c.full_hw()
    d = {"x0": r(c.B, c.c0, c.H, c.W, sc=c.sx),
         "x1": r(c.B, c.c1, c.H, c.W, sc=c.sx) if c.c1 else None,
         "w": r(c.cout, c.cin, c.kh, c.kw, sc=c.sw / math.sqrt(c.K)),
         "b": r(c.cout, sc=c.sx * c.sw)}
    if c.pre.startswith("affine"):
        shape = (c.B, c.cin) if c.per_sample else (c.cin,)
        d["scale"], d["shift"] = r(*shape), r(*shape, sc=c.sx)
    d["res"] = [r(c.B, c.cout, ho, wo, sc=c.sx * c.sw) for _ in range(c.res)]
    return d


def pre_input(c: Case, inp: dict, dtype=torch.float64) -> torch.Tensor:
    """x' = the pre-op applied to the concatenated sources, before upsample and padding (padding is zero AFTER the pre-op)."""
    x = torch.cat([inp["x0"], inp["x1"]], 1) if c.c1 else inp["x0"]
    x = x.to(dtype)
    if c.pre.startswith("affine"):
        sc, sh = inp["scale"].to(dtype), inp["shift"].to(dtype)
        view = (c.B, c.cin, 1, 1) if c.per_sample else (1, c.cin, 1, 1)
        x = x * sc.view(view) + sh.view(view)
    if c.pre in ("relu", "affine_relu"):
        x = F.relu(x)
    elif c.pre == "elu":
        x = F.elu(x)
    return x


def _padded(c: Case, x: torch.Tensor) -> torch.Tensor:
    if c.ups:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    p = (c.pw, c.pw, c.pad, c.pad)
    if c.pm == L.PAD_ZERO:
        return F.pad(x, p)
    return F.pad(x, p, mode="reflect" if c.pm == L.PAD_REFLECT else "replicate")


_ACT = {L.ACT_NONE: lambda v: v, L.ACT_RELU: F.relu, L.ACT_TANH: torch.tanh, L.ACT_SIGMOID: torch.sigmoid}


def reference(c: Case, inp: dict, w: Optional[torch.Tensor] = None, xp: Optional[torch.Tensor] = None):
    """(ref, den): the float64 result [B, cout, Ho, Wo] of the whole launch (pre-op, upsample, padding, conv, bias, activation,
    residuals) and the comparator's denominator.  `w` / `xp` replace the weights / the pre-processed input (mutations)."""
    w = (inp["w"] if w is None else w).to(torch.float64)
    xq = _padded(c, pre_input(c, inp) if xp is None else xp)
    b = inp["b"].to(torch.float64)
    y = F.conv2d(xq, w, b, stride=c.stride, dilation=c.dil)
    den = F.conv2d(xq.abs(), w.abs(), None, stride=c.stride, dilation=c.dil) + b.abs().view(1, -1, 1, 1)
    y = _ACT[c.act](y)
    if c.act == L.ACT_SIGMOID:
        den = den + y.abs() / 16     # sigmoid's offset: its fp32 result carries a few roundings of its own (2^-22 |y|)
    for rr in inp["res"]:
        y = y + rr.to(torch.float64)
        den = den + rr.to(torch.float64).abs()
    return y, den + 1e-300


def reference_bf16(c: Case, inp: dict):
    """(ref, den) of the single-pass bf16 kernels' own arithmetic: x' (formed in fp32, as the staging does) and the weights
    rounded to bf16 (ties to even), exact products and sums.  None for ELU, whose device exp differs from torch's by ~1e-7 -
    enough to flip an operand's bf16 rounding."""
    if c.pre == "elu":
        return None
    xr = pre_input(c, inp).float().bfloat16().double()
    return reference(c, inp, w=inp["w"].bfloat16().double(), xp=xr)


def window(c: Case, t: torch.Tensor) -> torch.Tensor:
    if not c.qwin:
        return t
    oy, ox, h, w = c.qwin
    return t[:, :, oy:oy + h, ox:ox + w]


def norm_err(got: torch.Tensor, ref: torch.Tensor, den: torch.Tensor) -> float:
    """The comparator: max |got - ref| / den in float64 (NaN / inf count as infinitely wrong)."""
    e = (got.detach().to("cpu", torch.float64) - ref).abs() / den
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, math.inf))
    return float(e.max()) if e.numel() else 0.0


# ---- mutations the comparator must reject (tests/test_conv_sweep_cpu.py) --------------------------------------------------
def round_sig_bits(t: torch.Tensor, bits: int) -> torch.Tensor:
    """float64 -> nearest value with `bits` significant bits (the exponent range unbounded: fp16's mantissa, not its range)."""
    m, e = torch.frexp(t)
    return torch.ldexp(torch.round(m * 2.0 ** bits), e - bits)


def mutations(c: Case, inp: dict):
    """(name, float64 result) of subtly wrong computations of the case: one tap moved, one 32-channel chunk of K dropped, the
    bias missing, one output off by 4x the bar, operands with 11 significant bits (when K <= 2304)."""
    w = inp["w"].to(torch.float64)
    ref, den = reference(c, inp)
    ntaps = c.kh * c.kw

    def first_visible(ws):                                      # the first weight mutation that changes the result at all
        for wm in ws:                                           # (taps that only ever read padding cannot be told apart)
            y = reference(c, inp, w=wm)[0]
            if bool((y != ref).any()):
                return y
        return None

    def swapped(t, j):
        wf = w.reshape(c.cout, c.cin, ntaps).clone()
        wf[:, :, [t, j]] = wf[:, :, [j, t]]
        return wf.reshape(w.shape)

    if ntaps > 1:
        # a wrong tap decode: tap t's weights applied at another tap's offset.  Non-square kernels first: the last tap decoded
        # transposed ((t // kh, t % kh) instead of (t // kw, t % kw)) when that lands elsewhere in the grid; then the centre
        # tap exchanged with each other tap
        t = ntaps - 1
        dst = (t // c.kh, t % c.kh)
        pairs = [(t, dst[0] * c.kw + dst[1])] if c.kh != c.kw and dst[0] < c.kh and dst[1] < c.kw else []
        ctr = (c.kh // 2) * c.kw + c.kw // 2
        pairs += [(ctr, j) for j in range(ntaps) if j != ctr]
        y = first_visible(swapped(a, b) for a, b in pairs if a != b)
        if y is not None:
            yield "tap_moved", y
    lo = 32 if c.cin > 32 else 0                                # K order (tap, channel): chunk 1 of a tap, or chunk 0

    def dropped(tap):
        wd = w.clone()
        wd[:, lo:lo + 32, tap // c.kw, tap % c.kw] = 0
        return wd
    ctr = (c.kh // 2) * c.kw + c.kw // 2
    y = first_visible(dropped(tp) for tp in [ctr] + [j for j in range(ntaps) if j != ctr])
    if y is not None:
        yield "k_chunk_dropped", y
    nob = dict(inp, b=torch.zeros_like(inp["b"]))
    yield "bias_missing", reference(c, nob)[0] + 0 * ref
    off = ref.clone()
    idx = tuple(int(v) // 2 for v in ref.shape)
    off[idx] += 4 * BAR_FP32 * den[idx]
    yield "one_pixel_off", off
    if c.K <= 2304:
        xr = round_sig_bits(pre_input(c, inp), 11)
        yield "fp16_hi_only", reference(c, inp, w=round_sig_bits(w, 11), xp=xr)[0]


# ---- the router, restated -------------------------------------------------------------------------------------------------
_TILES = {1: (128, 128), 2: (128, 64), 3: (128, 32), 4: (64, 64), 5: (64, 128)}


def _cdiv(a, b):
    return -(-a // b)


def plan_ksplit(M: int, cout_pad: int, k_pad: int, prec_f16x3: bool, tile: int = 0, ksplit: int = 0) -> Tuple[int, int]:
    """plan_impl's (tile, ksplit) for a launch that does not take the small-image kernel.  (ops.conv plans with the caller's
    precision code: bf16 is not F16X3 there, so it keeps the 128-row tiles.)"""
    if tile == 0:
        bn = 128 if cout_pad >= 128 and cout_pad % 128 == 0 else (64 if cout_pad % 64 == 0 else 32)
        bm = 128
        tiles = _cdiv(M, 128) * (cout_pad // bn)
        if tiles < 256 and bn == 128:
            bn = 64
            tiles = _cdiv(M, 128) * (cout_pad // bn)
        if tiles < 256 and bn == 64:
            bm = 64
        tile = {(128, 128): 1, (128, 64): 2, (128, 32): 3, (64, 64): 4, (64, 128): 4}[(bm, bn)]
        if prec_f16x3 and bm == 128 and bn >= 64:
            tile = 5 if bn == 128 else 4
    bm, bn = _TILES[tile]
    tiles = _cdiv(M, bm) * (cout_pad // bn)
    nk = k_pad // 32
    if ksplit <= 0:
        ks = 1
        if tiles < 192 and nk >= 8:
            ks = min(_cdiv(512, tiles), nk // 4, 32)
            ks = max(ks, 1)
        ksplit = ks
    return tile, max(ksplit, 1)


def wfrag_order(plan: pack.ConvPlan) -> Optional[int]:
    """ConvPlan.to's fusg_conv_desc.wfrag_order, or None when the plan has no fragment-order weights."""
    taps, ctot = plan.kh * plan.kw, plan.c0k + plan.c1k
    has_frag = plan.c0k % 32 == 0 and plan.c1k % 32 == 0 and ctot > 0 and plan.k_pad == taps * ctot
    if not has_frag and not plan.tapunit_ok():
        return None
    return 1 if plan.s2d_ok() else (2 if plan.tapunit_ok() else 0)


def small_ksplit(c: Case, plan: pack.ConvPlan, env: dict, ksplit_req: int) -> Optional[int]:
    """small_cfg: the K ranges of the small-image kernel, or None when the launch does not take it (split-fp16 only)."""
    order = wfrag_order(plan)
    if env.get("FUSG_NO_SMALL") or order not in (0, 1):
        return None
    kh, kw, s = c.kh, c.kw, c.stride
    if not (1 <= kh <= 3 and 1 <= kw <= 3) or c.dil != 1 or c.pm not in (L.PAD_ZERO, L.PAD_REPLICATE) or c.ups or s not in (1, 2):
        return None
    ntaps = kh * kw
    if plan.c0k <= 0 or plan.c0k % 32 or plan.k_pad % ntaps:
        return None
    ctot = plan.k_pad // ntaps
    if (ctot - plan.c0k) % 32:
        return None
    Ho, Wo = c.q_hw()
    hw = Ho * Wo
    part = bool(c.qwin and (c.qwin[0] or c.qwin[1])) or (Ho, Wo) != c.full_hw()
    win = part and c.pm == L.PAD_REPLICATE
    if part and not win:
        return None
    if not win and hw > 64:
        return None
    if hw < 32 and 32 % hw == 0 and not win:
        nimg, RIN, WIN = 32 // hw, (Ho - 1) * s + kh, (Wo - 1) * s + kw
    else:
        nimg = 1
        if Wo >= 32:
            if not (Ho == 1 or Wo % 32 == 0):
                return None
            RIN, WIN = kh, 31 * s + kw
        else:
            if 32 % Wo:
                return None
            RIN, WIN = (32 // Wo - 1) * s + kh, (Wo - 1) * s + kw
    npix = nimg * RIN * WIN
    if npix > 192:
        return None
    nch32 = ctot // 32
    nchw = min((112 * 1024) // (npix * 128), 72 // ntaps)
    if nchw < 1 or (ksplit_req == 1 and nchw < nch32):
        return None
    nchw = min(nchw, nch32)
    ks = _cdiv(nch32, nchw)
    nchw = _cdiv(nch32, ks)
    ks = _cdiv(nch32, nchw)
    if ks > 1 and not env.get("FUSG_SMALL_KSPLIT"):
        return None
    return ks


def vec_epi(c: Case) -> bool:
    return c.cout % 4 == 0 and c.out_c_off % 4 == 0 and c.out in ("nhwc", "slice")


def predict_family(c: Case, prec: str, env: Optional[dict] = None, ksplit: Optional[int] = None, tile: int = 0) -> int:
    """The family conv2d_impl picks for this case at `prec` ("f32" / "f16x3" / "bf16") with the per-call switches of `env`
    set (FUSG_NO_SMALL, FUSG_NO_POINTWISE, FUSG_NO_F32_HALO, FUSG_NO_BF16_TAPUNIT, FUSG_SMALL_KSPLIT) and the process-wide
    ones at their defaults.  `ksplit` / `tile`: the caller's choices (default: the case's ksplit, the automatic tile)."""
    env = env or {}
    g = torch.Generator().manual_seed(0)
    plan = make_plan(c, torch.randn(c.cout, c.cin, c.kh, c.kw, generator=g), torch.zeros(c.cout))
    ks_req = c.ksplit if ksplit is None else ksplit
    f16 = prec in ("f16x3", "bf16")
    order = wfrag_order(plan)
    if f16:
        if small_ksplit(c, plan, env, ks_req) is not None:
            return SMALL
    Ho, Wo = c.q_hw()
    M = c.B * Ho * Wo
    _, ks = plan_ksplit(M, plan.cout_pad, plan.k_pad, prec == "f16x3", tile, ks_req)
    no_f32_halo = bool(env.get("FUSG_NO_F32_HALO"))
    taps = c.kh * c.kw
    has1 = c.c1 > 0
    if (not env.get("FUSG_NO_POINTWISE") and c.kh == 1 and c.kw == 1 and c.stride == 1 and not c.ups and not has1 and
            4 <= plan.c0k <= 8 and ks <= 1 and vec_epi(c) and c.pre in ("none", "relu", "elu") and not c.qwin and
            c.pad == 0 and c.pw == 0 and 256 % (plan.cout_pad // 4) == 0):
        return POINTWISE
    tap_geom = (not c.ups and ks <= 1 and not has1 and 4 <= plan.c0k <= 24 and c.dil == 1 and Ho % 8 == 0 and Wo % 16 == 0
                and plan.k_pad >= taps * plan.c0k and not c.qwin)
    HH, HW = 7 * c.stride + c.kh, 15 * c.stride + c.kw
    if order == 2 and prec == "f32" and not no_f32_halo:
        if tap_geom and taps * (plan.c0k // 4) <= 320 and HH * HW * plan.c0k * 4 <= 80 * 1024 and HH * HW * (plan.c0k // 4) <= 2048:
            return TAPUNIT_F32
    if order == 2 and f16:
        unit = 8 if plan.c0k % 8 == 0 else 4
        RP = _cdiv(HW * plan.c0k, 128) * 128
        if tap_geom and taps * (plan.c0k // unit) <= 160 and 4 * HH * RP <= 80 * 1024 and HH * HW * (plan.c0k // 4) <= 2048:
            return TAPUNIT_BF16 if prec == "bf16" and not env.get("FUSG_NO_BF16_TAPUNIT") else TAPUNIT
    s2d_form = order == 1 and c.stride == 2 and c.H % 2 == 0 and c.W % 2 == 0 and c.pm != L.PAD_REPLICATE
    f32_halo = prec == "f32" and not no_f32_halo and order in (0, 1)
    halo = ((f16 or f32_halo) and order is not None and ks <= 1 and ((c.stride == 1 and order == 0) or (s2d_form and not c.ups))
            and plan.c0k % 32 == 0 and plan.c0k > 0 and plan.c1k % 32 == 0 and Ho % 8 == 0 and Wo % 16 == 0 and not c.qwin)
    if halo:
        hh, hw_ = (10, 18) if s2d_form else (8 + (c.kh - 1) * c.dil, 16 + (c.kw - 1) * c.dil)
        if hh * hw_ <= 320:
            if f32_halo:
                return HALO_F32
            if prec == "bf16":
                return HALO_BF16
            return HALO_S2D if s2d_form else HALO
    return GEN_F32 if prec == "f32" else GEN_F16X3


def off_switch(family: int, c: Case):
    """(env, ksplit) that turns the family off for this launch - the next family in the router's order runs on the same
    data - or None (the generic gathers are the end of the line)."""
    if family == SMALL:
        return {"FUSG_NO_SMALL": "1"}, None
    if family == POINTWISE:
        return {"FUSG_NO_POINTWISE": "1"}, None
    if family in (HALO_F32, TAPUNIT_F32):
        return {"FUSG_NO_F32_HALO": "1"}, None
    if family == TAPUNIT_BF16:
        return {"FUSG_NO_BF16_TAPUNIT": "1"}, None
    if family in (HALO, HALO_S2D, HALO_BF16, TAPUNIT):
        return ({}, 2) if c.K > 32 else None                     # (two K ranges need two 32-wide K steps)
    return None


# ---- the edge table --------------------------------------------------------------------------------------------------
def _e(tag, B, c0, c1, cout, kh, kw, H, W, expect, **kw_):
    return Case(tag=tag, B=B, c0=c0, c1=c1, cout=cout, kh=kh, kw=kw, H=H, W=W, expect=expect, **kw_)


G, G3 = GEN_F32, GEN_F16X3
EDGE = [
    # -- small-image kernel: Ho*Wo 64 vs 65, Wo 16 vs 32 ("wide" runs), whole images per workgroup hw in {1, 2, 4, 8, 16}
    _e("small_hw64_8x8", 2, 32, 0, 32, 3, 3, 8, 8, (G, SMALL, SMALL), pad=1),
    _e("small_hw65_5x13", 2, 32, 0, 32, 3, 3, 5, 13, (G, G3, G3), pad=1),
    _e("small_wo16_2x16", 2, 32, 0, 32, 3, 3, 2, 16, (G, SMALL, SMALL), pad=1),
    _e("small_wo32_wide_2x32", 2, 32, 0, 32, 3, 3, 2, 32, (G, SMALL, SMALL), pad=1),
    _e("small_wo64_wide_1x64", 1, 32, 0, 64, 1, 3, 1, 64, (G, SMALL, SMALL), pad=0, pad_w=1),
    _e("small_wo24_no_32", 1, 32, 0, 32, 1, 1, 2, 24, (G, G3, G3)),
    _e("small_hw1", 3, 64, 0, 32, 1, 1, 1, 1, (G, SMALL, SMALL)),
    _e("small_hw1_k3_npix288_no", 3, 64, 0, 32, 3, 3, 1, 1, (G, G3, G3), pad=1),
    _e("small_hw2", 5, 32, 0, 32, 3, 3, 1, 2, (G, SMALL, SMALL), pad=1),
    _e("small_hw4", 3, 32, 0, 64, 3, 3, 2, 2, (G, SMALL, SMALL), pad=1),
    _e("small_hw8", 3, 32, 32, 32, 3, 3, 2, 4, (G, SMALL, SMALL), pad=1),
    _e("small_hw16", 3, 32, 0, 40, 3, 3, 4, 4, (G, SMALL, SMALL), pad=1),
    _e("small_hw3_no", 3, 32, 0, 32, 3, 3, 1, 3, (G, G3, G3), pad=1),
    # -- small-image kernel: every kh x kw it admits (the tap decode), stride 2, replicate, pad_w != pad
    _e("small_k2x2_9x9", 2, 32, 0, 32, 2, 2, 9, 9, (G, SMALL, SMALL)),
    _e("small_k3x2", 2, 32, 0, 32, 3, 2, 8, 7, (G, SMALL, SMALL), pad=1),
    _e("small_k2x3", 2, 32, 0, 32, 2, 3, 4, 4, (G, SMALL, SMALL), pad=0, pad_w=1),
    _e("small_k1x2", 1, 32, 0, 32, 1, 2, 4, 5, (G, SMALL, SMALL)),
    _e("small_k2x1", 1, 32, 0, 32, 2, 1, 5, 4, (G, SMALL, SMALL)),
    _e("small_k1x3", 2, 64, 0, 32, 1, 3, 4, 4, (G, SMALL, SMALL), pad_w=1),
    _e("small_k3x1_elu", 2, 32, 0, 32, 3, 1, 8, 4, (G, SMALL, SMALL), pad=1, pad_w=0, pre="elu"),
    _e("small_k3x2_s2", 2, 32, 0, 32, 3, 2, 8, 6, (G, SMALL, SMALL), stride=2, pad=1),
    _e("small_k2x2_s2_rep", 2, 32, 32, 32, 2, 2, 7, 7, (G, SMALL, SMALL), stride=2, pm=L.PAD_REPLICATE, pad=1),
    _e("small_k3_s2_s2d_rep", 2, 32, 0, 32, 3, 3, 8, 8, (G, SMALL, SMALL), stride=2, pad=1, pm=L.PAD_REPLICATE),
    _e("small_k3_s2_odd", 1, 32, 0, 32, 3, 3, 7, 7, (G, SMALL, SMALL), stride=2, pad=1),
    _e("small_k2x2_affine_ps", 3, 32, 32, 32, 2, 2, 3, 3, (G, SMALL, SMALL), pre="affine_relu", per_sample=True),
    _e("small_k3_reflect_no", 2, 32, 0, 32, 3, 3, 4, 4, (G, G3, G3), pad=1, pm=L.PAD_REFLECT),
    _e("small_k3_dil2_no", 2, 32, 0, 32, 3, 3, 6, 6, (G, G3, G3), pad=2, dil=2),
    _e("small_k4_no", 2, 32, 0, 32, 4, 4, 5, 5, (G, G3, G3), pad=1),
    _e("small_c1_20_no", 2, 32, 20, 32, 3, 3, 4, 4, (G, G3, G3), pad=1),
    _e("small_ksplit_k2x2", 4, 512, 512, 64, 2, 2, 3, 3, (G, G3, G3)),
    _e("small_act_tanh_res2", 3, 64, 0, 32, 3, 3, 4, 4, (G, SMALL, SMALL), pad=1, act=L.ACT_TANH, res=2),
    _e("small_misaligned", 2, 32, 0, 12, 2, 2, 5, 5, (G, SMALL, SMALL), out="misaligned"),
    _e("small_nchw_sigmoid", 2, 32, 0, 40, 3, 3, 4, 4, (G, SMALL, SMALL), pad=1, out="nchw", act=L.ACT_SIGMOID),
    _e("small_slice_off2", 2, 32, 0, 32, 3, 2, 4, 3, (G, SMALL, SMALL), pad=1, out="slice", out_c_off=2),
    _e("small_cout1", 3, 32, 0, 1, 3, 3, 2, 2, (G, SMALL, SMALL), pad=1),
    _e("small_cout3", 2, 32, 0, 3, 2, 2, 5, 5, (G, SMALL, SMALL)),
    # -- q_window launches with replicate padding (ring windows: the small kernel takes a window of any size)
    _e("qwin_row_rep", 2, 32, 0, 32, 3, 3, 16, 40, (G, SMALL, SMALL), pad=1, pm=L.PAD_REPLICATE, qwin=(15, 0, 1, 40)),
    _e("qwin_col_rep", 2, 32, 0, 32, 3, 3, 40, 16, (G, SMALL, SMALL), pad=1, pm=L.PAD_REPLICATE, qwin=(0, 15, 40, 1)),
    _e("qwin_corner_k2x2", 1, 32, 0, 32, 2, 2, 12, 12, (G, SMALL, SMALL), pad=1, pm=L.PAD_REPLICATE, qwin=(11, 11, 2, 2)),
    _e("qwin_inner_c20", 1, 20, 0, 32, 3, 3, 12, 20, (G, G3, G3), pad=1, pm=L.PAD_REPLICATE, qwin=(2, 3, 5, 7)),
    # -- pointwise few-channel kernel: c0k 4..8, cout_pad | 1024 with 256 % (cout_pad / 4) == 0, cout % 4, pre-ops
    _e("pw_c6_128_elu", 2, 6, 0, 128, 1, 1, 9, 11, (POINTWISE, POINTWISE, POINTWISE), pre="elu"),
    _e("pw_c3_32_relu", 1, 3, 0, 32, 1, 1, 5, 7, (POINTWISE, POINTWISE, POINTWISE), pre="relu"),
    _e("pw_c8_12_res", 3, 8, 0, 12, 1, 1, 6, 6, (POINTWISE, POINTWISE, POINTWISE), res=1, act=L.ACT_TANH),
    _e("pw_c8_4", 2, 8, 0, 4, 1, 1, 7, 5, (POINTWISE, POINTWISE, POINTWISE)),
    _e("pw_c9_no", 2, 9, 0, 32, 1, 1, 7, 5, (G, G3, G3)),
    _e("pw_cout3_no", 2, 8, 0, 3, 1, 1, 7, 5, (G, G3, G3)),
    _e("pw_cout96_no", 2, 8, 0, 96, 1, 1, 7, 5, (G, G3, G3)),
    _e("pw_affine_no", 2, 8, 0, 32, 1, 1, 8, 16, (TAPUNIT_F32, TAPUNIT, TAPUNIT_BF16), pre="affine"),
    _e("pw_slice_off4", 2, 4, 0, 32, 1, 1, 7, 5, (POINTWISE, POINTWISE, POINTWISE), out="slice", out_c_off=4),
    _e("pw_slice_off2_no", 2, 4, 0, 32, 1, 1, 7, 5, (G, G3, G3), out="slice", out_c_off=2),
    _e("pw_nchw_no", 2, 4, 0, 32, 1, 1, 8, 16, (TAPUNIT_F32, TAPUNIT, TAPUNIT_BF16), out="nchw"),
    # -- tap-unit stems: c0k 24 vs 28, nunits 160 vs 168, qh % 8 / qw % 16, stride 2, every precision
    _e("tap_c3_7x7_s2", 1, 3, 0, 64, 7, 7, 32, 64, (TAPUNIT_F32, TAPUNIT, TAPUNIT_BF16), stride=2, pad=3),
    _e("tap_c24_3x3", 1, 24, 0, 32, 3, 3, 8, 16, (TAPUNIT_F32, TAPUNIT, TAPUNIT_BF16), pad=1, pre="elu"),
    _e("tap_c28_3x3_no", 1, 28, 0, 32, 3, 3, 8, 16, (G, G3, G3), pad=1, ksplit=1),
    _e("tap_c20_4x8_n160", 1, 20, 0, 32, 4, 8, 11, 23, (TAPUNIT_F32, TAPUNIT, TAPUNIT_BF16), ksplit=1),
    _e("tap_c24_7x8_n168_no", 1, 24, 0, 32, 7, 8, 14, 23, (G, G3, G3), ksplit=1),
    _e("tap_c12_7x7_reflect", 1, 12, 0, 40, 7, 7, 8, 16, (TAPUNIT_F32, TAPUNIT, TAPUNIT_BF16), pad=3, pm=L.PAD_REFLECT,
       ksplit=1, act=L.ACT_RELU),
    _e("tap_c4_3x3_qw17_no", 1, 4, 0, 32, 3, 3, 8, 17, (G, G3, G3), pad=1),
    _e("tap_c8_5x5_qh9_no", 1, 8, 0, 32, 5, 5, 9, 16, (G, G3, G3), pad=2, ksplit=1),
    _e("tap_c4_1x7_rep", 2, 4, 0, 32, 1, 7, 8, 16, (TAPUNIT_F32, TAPUNIT, TAPUNIT_BF16), pad=0, pad_w=3, pm=L.PAD_REPLICATE),
    _e("tap_c4_planner_split", 1, 16, 0, 32, 7, 7, 8, 16, (G, G3, G3), pad=3),
    _e("tap_c8_affine_ps_nchw", 2, 8, 0, 64, 3, 3, 16, 16, (TAPUNIT_F32, TAPUNIT, TAPUNIT_BF16), pad=1, pre="affine",
       per_sample=True, out="nchw"),
    # -- halo kernel: dense (1 x 1 .. 7 x 7, non-square), qh % 8 / qw % 16, dil (k-1) at the halo_fits limit, two sources,
    #    padding modes, upsample, pad_w != pad; parity-quadrant stride 2 on even / odd sizes
    _e("halo_1x1_8x16", 1, 64, 0, 32, 1, 1, 8, 16, (HALO_F32, HALO, HALO_BF16)),
    _e("halo_1x1_9x16_no", 1, 64, 0, 32, 1, 1, 9, 16, (G, G3, G3)),
    _e("halo_1x1_8x24_no", 1, 64, 0, 32, 1, 1, 8, 24, (G, G3, G3)),
    _e("halo_1x3_rep", 2, 32, 0, 32, 1, 3, 8, 16, (HALO_F32, HALO, HALO_BF16), pad=0, pad_w=1, pm=L.PAD_REPLICATE),
    _e("halo_3x1_reflect", 1, 32, 0, 40, 3, 1, 8, 32, (HALO_F32, HALO, HALO_BF16), pad=1, pad_w=0, pm=L.PAD_REFLECT),
    _e("halo_2x2", 1, 32, 0, 32, 2, 2, 9, 17, (HALO_F32, HALO, HALO_BF16)),
    _e("halo_1x3_ups_reflect", 1, 32, 0, 32, 1, 3, 4, 8, (HALO_F32, HALO, HALO_BF16), pad=0, pad_w=1, ups=1, pm=L.PAD_REFLECT),
    _e("small_k2x2_ups_no", 1, 32, 0, 32, 2, 2, 3, 3, (G, G3, G3), ups=1),
    _e("halo_3x2_zero", 1, 32, 0, 32, 3, 2, 8, 17, (HALO_F32, HALO, HALO_BF16), pad=1, pad_w=0),
    _e("halo_1x7", 1, 32, 0, 32, 1, 7, 8, 16, (HALO_F32, HALO, HALO_BF16), pad=0, pad_w=3),
    _e("halo_7x1_elu", 1, 32, 0, 32, 7, 1, 8, 16, (HALO_F32, HALO, HALO_BF16), pad=3, pad_w=0, pre="elu"),
    _e("halo_3x3_ks1", 1, 32, 0, 64, 3, 3, 8, 16, (HALO_F32, HALO, HALO_BF16), pad=1, ksplit=1),
    _e("halo_3x3_planner", 1, 32, 0, 64, 3, 3, 8, 16, (G, G3, G3), pad=1),
    _e("halo_5x5_ks1", 1, 32, 0, 32, 5, 5, 8, 16, (HALO_F32, HALO, HALO_BF16), pad=2, ksplit=1, pm=L.PAD_REFLECT),
    _e("halo_7x7_ks1", 1, 32, 0, 32, 7, 7, 8, 16, (HALO_F32, HALO, HALO_BF16), pad=3, ksplit=1),
    _e("halo_dil3_fits", 1, 32, 0, 32, 3, 3, 8, 16, (HALO_F32, HALO, HALO_BF16), pad=3, dil=3, ksplit=1, pm=L.PAD_REFLECT),
    _e("halo_dil4_no", 1, 32, 0, 32, 3, 3, 8, 16, (G, G3, G3), pad=4, dil=4, ksplit=1, pm=L.PAD_REFLECT),
    _e("halo_2x2_dil4", 1, 32, 0, 32, 2, 2, 12, 20, (HALO_F32, HALO, HALO_BF16), dil=4),
    _e("halo_two_src", 2, 32, 32, 32, 1, 1, 8, 16, (HALO_F32, HALO, HALO_BF16), pre="elu", res=1),
    _e("halo_two_src_c1_20_no", 2, 32, 20, 32, 1, 1, 8, 16, (G, G3, G3)),
    _e("halo_c20_cinpad32", 1, 20, 0, 32, 1, 3, 8, 16, (HALO_F32, HALO, HALO_BF16), pad_w=1, cin_pad=32),
    _e("halo_affine_ps_slice", 2, 64, 0, 32, 1, 1, 8, 16, (HALO_F32, HALO, HALO_BF16), pre="affine_relu", per_sample=True,
       out="slice", out_c_off=4),
    _e("halo_misaligned_cout3", 1, 32, 0, 3, 1, 3, 8, 16, (HALO_F32, HALO, HALO_BF16), pad_w=1, out="misaligned"),
    _e("halo_nchw_sigmoid_cout1", 1, 64, 0, 1, 1, 1, 8, 32, (HALO_F32, HALO, HALO_BF16), out="nchw", act=L.ACT_SIGMOID),
    _e("halo_cout128_ks1", 1, 32, 0, 128, 3, 3, 8, 16, (HALO_F32, HALO, HALO_BF16), pad=1, ksplit=1, res=2),
    _e("halo_cout12_odd_batch", 3, 32, 0, 12, 1, 3, 8, 16, (HALO_F32, HALO, HALO_BF16), pad_w=1, act=L.ACT_TANH),
    _e("s2d_k3_even", 1, 32, 0, 32, 3, 3, 16, 32, (HALO_F32, HALO_S2D, HALO_BF16), stride=2, pad=1, ksplit=1),
    _e("s2d_k4_reflect", 1, 32, 0, 32, 4, 4, 16, 32, (HALO_F32, HALO_S2D, HALO_BF16), stride=2, pad=1, ksplit=1,
       pm=L.PAD_REFLECT),
    _e("s2d_k3_odd_no", 1, 32, 0, 32, 3, 3, 17, 31, (G, G3, G3), stride=2, pad=1, ksplit=1),
    _e("s2d_k3_replicate", 1, 32, 0, 32, 3, 3, 16, 32, (G, G3, G3), stride=2, pad=1, ksplit=1, pm=L.PAD_REPLICATE),
    _e("s2_k2_no_quadrants", 1, 32, 0, 32, 2, 2, 16, 32, (G, G3, G3), stride=2),
    # -- generic gathers: what no fast kernel takes
    _e("gen_c12_3x3", 3, 12, 0, 40, 3, 3, 17, 9, (G, G3, G3), pad=1),
    _e("gen_c12_s2", 2, 12, 0, 40, 3, 3, 8, 12, (G, G3, G3), stride=2, pad=1),
    _e("gen_5x5_reflect", 1, 24, 0, 16, 5, 5, 12, 12, (G, G3, G3), pad=2, pm=L.PAD_REFLECT),
    _e("gen_ups_c1_odd", 1, 12, 4, 32, 3, 3, 5, 7, (G, G3, G3), pad=1, ups=1),
    _e("gen_dil2_rep", 2, 36, 0, 12, 3, 3, 9, 9, (G, G3, G3), pad=2, dil=2, pm=L.PAD_REPLICATE),
    _e("gen_affine_misaligned", 2, 36, 0, 7, 3, 3, 9, 9, (G, G3, G3), pad=1, pre="affine", out="misaligned"),
    _e("gen_k2304", 1, 256, 0, 32, 3, 3, 7, 9, (G, G3, G3), pad=1),
    _e("gen_scale_small", 2, 40, 0, 32, 3, 3, 11, 11, (G, G3, G3), pad=1, sx=1e-3, sw=2e-3),
    _e("gen_scale_large", 2, 40, 0, 32, 3, 3, 11, 11, (G, G3, G3), pad=1, sx=1e2, sw=1e1, pre="relu"),
    _e("gen_1x7_split", 1, 40, 0, 32, 1, 7, 9, 20, (G, G3, G3), pad_w=3),
]


# ---- the random draw ---------------------------------------------------------------------------------------------------
_KS = [(1, 1), (3, 3), (3, 3), (2, 2), (1, 3), (3, 1), (3, 2), (2, 3), (5, 5), (1, 7), (7, 1), (4, 4), (7, 7)]


def _draw(rng: np.random.RandomState, i: int) -> Optional[Case]:
    ch = lambda seq: seq[rng.randint(len(seq))]                 # noqa: E731
    kh, kw = ch(_KS)
    fewc = rng.rand() < 0.25
    c0 = ch([3, 4, 6, 8, 12, 16, 20, 24]) if fewc else ch([28, 32, 32, 36, 64, 64, 96, 128, 256])
    c1 = 0 if fewc or rng.rand() < 0.7 else ch([20, 32, 64])
    cout = ch([1, 3, 4, 12, 32, 40, 64, 96, 128])
    stride = 2 if rng.rand() < 0.25 else 1
    dil = 2 if stride == 1 and rng.rand() < 0.15 else 1
    ups = 1 if stride == 1 and rng.rand() < 0.1 else 0
    pm = ch([L.PAD_ZERO, L.PAD_ZERO, L.PAD_REFLECT, L.PAD_REPLICATE])
    pad = rng.randint(0, (dil * (kh - 1)) // 2 + 2)
    pw = pad if rng.rand() < 0.8 else rng.randint(0, (dil * (kw - 1)) // 2 + 2)
    # output grid: aligned to the halo / tap-unit patches, small-image sizes, or anything
    r = rng.rand()
    if r < 0.35:
        Ho, Wo = ch([8, 16]), ch([16, 32])
    elif r < 0.7:
        Ho, Wo = ch([(1, 1), (1, 2), (2, 2), (2, 4), (4, 4), (2, 16), (4, 8), (8, 8), (1, 32), (1, 64), (2, 32), (3, 3), (5, 13)])
    else:
        Ho, Wo = rng.randint(1, 20), rng.randint(1, 24)
    ek_h, ek_w = dil * (kh - 1) + 1, dil * (kw - 1) + 1
    H = (Ho - 1) * stride + ek_h - 2 * pad
    W = (Wo - 1) * stride + ek_w - 2 * pw
    if ups:
        H, W = (H + 1) // 2, (W + 1) // 2
    if H < 1 or W < 1:
        return None
    B = ch([1, 1, 2, 3, 4, 5])
    pre = ch(["none", "none", "relu", "elu", "affine", "affine_relu"])
    per_sample = pre.startswith("affine") and rng.rand() < 0.5
    act = ch([L.ACT_NONE, L.ACT_NONE, L.ACT_NONE, L.ACT_RELU, L.ACT_TANH, L.ACT_SIGMOID])
    res = ch([0, 0, 0, 1, 2])
    out = ch(["nhwc", "nhwc", "nhwc", "nhwc", "slice", "nchw", "misaligned"])
    off = ch([4, 8, 2, 1]) if out == "slice" else 0
    ksplit = 1 if rng.rand() < 0.3 else 0
    cin_pad = 32 if fewc and rng.rand() < 0.3 else 4
    # (operand scales away from 1 only without tanh / sigmoid: those saturate, or their own rounding hides the contraction's)
    sx, sw = (1.0, 1.0) if rng.rand() < 0.8 or act in (L.ACT_TANH, L.ACT_SIGMOID) else (ch([1e-2, 1e2]), ch([2e-3, 1e1]))
    c = Case(tag=f"rand{i:03d}", B=B, c0=c0, c1=c1, cout=cout, kh=kh, kw=kw, H=H, W=W, stride=stride, pad=pad,
             pad_w=None if pw == pad else pw, dil=dil, pm=pm, ups=ups, pre=pre, per_sample=per_sample, act=act, res=res,
             out=out, out_c_off=off, ksplit=ksplit, cin_pad=cin_pad, sx=sx, sw=sw, seed=i)
    try:
        validate(c)
    except AssertionError:
        return None
    if c.full_hw() != (Ho, Wo) or c.mflop() > 24.0 or c.K > 4608:
        return None
    if pad >= ek_h or pw >= ek_w:                               # (outputs that read nothing but padding: no operand matters)
        return None
    if act == L.ACT_SIGMOID and c.K > 576:                      # (sigmoid' <= 1/4 hides a quarter of an error from the bar)
        return None
    return c


def random_cases(n: int = 240, seed: int = 20261016):
    """A seeded, reproducible draw of `n` cases from the space the router admits (each at most ~24 MFLOP of reference)."""
    rng = np.random.RandomState(seed)
    out, i = [], 0
    while len(out) < n:
        c = _draw(rng, i)
        i += 1
        if c is not None:
            out.append(replace(c, tag=f"rand{len(out):03d}"))
    return out


def edge_cases():
    return list(EDGE)


def all_cases():
    return edge_cases() + random_cases()
