"""The single-pass fp16 precision mode ("f16", include/fusg.h FUSG_PREC_F16) - a helper module of its tests, not a conftest.
Plain torch on the CPU, importable without a GPU.

The mode's arithmetic on a launch that takes the halo or the tap-unit kernel (families 15 / 16):

    a' = RTN_fp16(pre_op(a))        w' = RTN_fp16(w s_n)        acc(fp32) += a' w'        out = act(fmaf(acc, 1 / s_n, bias)) (+ residuals)

`reference_f16` is that arithmetic with exact products and sums, in float64: what the kernels compute up to their fp32
accumulation order, so they are held to it at conv_sweep.BAR_FP32.  `f16_family` maps the family a case takes under bf16 to the
one it takes under f16; `MASK_SHAPES` are the staging shapes of the GPU test (their references must tell the mode from f16x3:
tests/test_f16_mode_cpu.py).

`INSTANTIATIONS` names the 63 MODE 3 kernel instantiations, `instantiation` the one a launch takes (from the library's
fusg_conv2d_route_order), `tile_cases` the table that reaches each of them under `SWITCH_SETS`; `scale_cases` are the operand
scales (fp16 subnormal activations) and `restatement` four wrong readings of the mode that the references must reject."""
from typing import Optional

import torch

import conv_sweep as cs
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import pack

HALO_F16, TAPUNIT_F16 = L.CONV_HALO_F16, L.CONV_TAPUNIT_F16
F16_FAMILIES = (HALO_F16, TAPUNIT_F16)

# ELU rows (no operand-exact reference: the device exp differs from torch's by ~1e-7, enough to flip an operand's rounding) are
# judged against the exact reference at the operand-rounding bound, built as conv_sweep.BAR_BF16 is: fp16 keeps 11 significant
# bits, rounding to nearest errs by up to 2^-11 per operand and a product of two rounded operands by (1 + 2^-11)^2 - 1.
BAR_F16 = (1 + 2.0 ** -11) ** 2 - 1


def f16_family(bf16_family: int) -> int:
    """The family a launch takes under "f16", given the one it takes under "bf16": 5 -> 15, 11 -> 16, others unchanged."""
    return {cs.HALO_BF16: HALO_F16, cs.TAPUNIT_BF16: TAPUNIT_F16}.get(bf16_family, bf16_family)


def predict_family(c: cs.Case, env: Optional[dict] = None, ksplit: Optional[int] = None, tile: int = 0) -> int:
    """conv_sweep.predict_family for "f16": the bf16 route's family, mapped.  FUSG_NO_F16_TAPUNIT stands where
    FUSG_NO_BF16_TAPUNIT stands under bf16."""
    env = dict(env or {})
    if env.pop("FUSG_NO_F16_TAPUNIT", None):
        env["FUSG_NO_BF16_TAPUNIT"] = "1"
    return f16_family(cs.predict_family(c, "bf16", env=env, ksplit=ksplit, tile=tile))


def f16_weights(w: torch.Tensor) -> torch.Tensor:
    """[cout, cin, kh, kw] -> pack.f16_mode_weights of the layer, in the same shape, float64.  (The scale s_n depends on the
    channel's largest |w| alone, so the packed panel's K order and zero padding do not matter.)"""
    return pack.f16_mode_weights(w.float().reshape(1, w.shape[0], -1)).reshape(w.shape).double()


def reference_f16(c: cs.Case, inp: dict):
    """(ref, den) of the single-pass fp16 kernels' own arithmetic, float64: x' (formed in fp32, as the staging does) rounded to
    fp16 (ties to even), the weights pack.f16_mode_weights, exact products and sums.  None for ELU, as reference_bf16."""
    return None if c.pre == "elu" else operand_rounded(c, inp)


def operand_rounded(c: cs.Case, inp: dict):
    """reference_f16 without its ELU exclusion (torch's ELU then stands for the device's): what the CPU test uses to show
    that every shape of the GPU table tells the mode's operand rounding from f16x3."""
    xr = cs.pre_input(c, inp).float().half().double()
    return cs.reference(c, inp, w=f16_weights(inp["w"]), xp=xr)


# ---- the explicit staging shapes of tests/test_gpu_f16_mode.py: masks and tails ------------------------------------------
def _m(tag, B, c0, c1, cout, kh, kw, H, W, **kw_):
    return cs.Case(tag=tag, B=B, c0=c0, c1=c1, cout=cout, kh=kh, kw=kw, H=H, W=W, ksplit=1, **kw_)


MASK_SHAPES = [
    _m("f16_one_patch", 1, 32, 0, 32, 3, 3, 8, 16, pad=1),
    _m("f16_ragged_2x13x21", 2, 32, 0, 32, 3, 3, 13, 21, pad=1),
    _m("f16_two_src_cout48", 2, 64, 32, 48, 3, 3, 9, 17, pad=1),
]
# the six shapes of test_gpu_ops.test_bf16_halo_conv: (cin, cout, k, stride, pad, dil, pad_mode, h, w, pre), batch 2 - the 5 x 5 one
# from 32 channels instead of 128: over K = 3200 the operand roundings average down to 9.5 bars, under the 10 the CPU test asks
HALO_SHAPES = [(128, 128, 3, 1, 1, 1, L.PAD_ZERO, 32, 32, "elu"), (256, 256, 3, 1, 2, 2, L.PAD_REFLECT, 16, 16, "affine_relu"),
               (64, 32, 3, 1, 1, 1, L.PAD_ZERO, 32, 64, "none"), (32, 64, 5, 1, 2, 1, L.PAD_REFLECT, 16, 32, "none"),
               (64, 128, 4, 2, 1, 1, L.PAD_REFLECT, 32, 64, "relu"), (128, 256, 1, 1, 0, 1, L.PAD_ZERO, 16, 16, "none")]
# the three of test_gpu_ops.test_bf16_tapunit_stems: (cin, cout, stride, pad_mode, h, w, pre), 7 x 7, pad 3, batch 2
STEM_SHAPES = [(21, 64, 1, L.PAD_REFLECT, 32, 32, "none"), (3, 64, 2, L.PAD_ZERO, 64, 64, "none"), (4, 64, 1, L.PAD_REFLECT, 16, 32, "elu")]


# staging shapes that DO land on the halo kernel: several patches with zero padding on every side of the image, and two sources
# into 48 outputs (cout_pad 64: the padded columns' stores must be masked) - beside the ragged ones above, which take the
# generic gather and must therefore equal f16x3
EXTRA = [cs.Case(tag="f16_patches_2x16x32", B=2, c0=32, c1=0, cout=32, kh=3, kw=3, H=16, W=32, pad=1, ksplit=1, seed=61),
         cs.Case(tag="f16_two_src_cout48_8x16", B=2, c0=64, c1=32, cout=48, kh=3, kw=3, H=8, W=16, pad=1, ksplit=1, seed=62,
                 pre="affine_relu", per_sample=True, res=1)]


def table_cases():
    """The GPU table: the explicit masks and tails, the six halo shapes and the three stems, as sweep cases."""
    out = list(MASK_SHAPES)
    for i, (cin, cout, k, s, p, d, pm, h, w, pre) in enumerate(HALO_SHAPES):
        out.append(cs.Case(tag=f"f16_halo{i}_{cin}_{cout}_k{k}s{s}d{d}", B=2, c0=cin, c1=0, cout=cout, kh=k, kw=k, H=h, W=w,
                           stride=s, pad=p, dil=d, pm=pm, pre=pre, ksplit=1, seed=40 + i))
    for i, (cin, cout, s, pm, h, w, pre) in enumerate(STEM_SHAPES):
        out.append(cs.Case(tag=f"f16_stem{i}_c{cin}_s{s}", B=2, c0=cin, c1=0, cout=cout, kh=7, kw=7, H=h, W=w, stride=s, pad=3,
                           pm=pm, pre=pre, ksplit=1, seed=50 + i))
    return out


# ---- the 63 MODE 3 kernel instantiations and the table that reaches each of them ------------------------------------------
# (unit, pre kind, NI staged items per thread | U channels per K unit): the rows of profiles/f16_mode_resources.txt
PRE_KINDS = ("none", "elu", "affine")
HALO_UNITS = ("conv_halo_128", "conv_halo_64", "conv_halo_32", "conv_halo_64k", "conv_halo_32k")
TAP_UNITS = ("conv_tapunit_128", "conv_tapunit_64", "conv_tapunit_32")
INSTANTIATIONS = tuple([(u, p, ni) for u in HALO_UNITS for p in PRE_KINDS for ni in (6, 8, 10)] +
                       [(u, p, un) for u in TAP_UNITS for p in PRE_KINDS for un in (4, 8)])
# the two whose MODE 3 build takes another occupancy and epilogue than its MODE 1 sibling (* in the profile)
STARRED = (("conv_halo_128", "elu", 10), ("conv_halo_64", "affine", 10))
_PRE_KIND = {"none": "none", "relu": "none", "elu": "elu", "affine": "affine", "affine_relu": "affine"}

# The process-wide environments the table runs under (csrc/api.hip reads these once per process: one fresh child process per
# non-empty set).  On grids of a few patches the default narrows every halo launch to a 32-column unit; FUSG_HALO_MINWG=1 keeps
# the widest unit that divides cout_pad, FUSG_NO_KSPLIT=1 takes the M-split units where the K split over the waves would run.
SWITCH_SETS = ({}, {"FUSG_HALO_MINWG": "1"}, {"FUSG_HALO_MINWG": "1", "FUSG_NO_KSPLIT": "1"}, {"FUSG_NO_KSPLIT": "1"})


def switch_name(env: dict) -> str:
    return "+".join(sorted(env)) or "default"


def instantiation(c: cs.Case, route_order):
    """(unit, pre kind, NI | U) of the launch whose fusg_conv2d_route_order is `route_order` = [family, bn, ksplit, ksw], or None
    when the family is neither 15 nor 16.  Halo: the unit is bn, `k` appended when the K runs over the waves (ksw == 1); NI as
    launch_halo_fn buckets it, ceil(HH HW 8 / 256) -> 6 / 8 / 10, the halo 10 x 18 in quadrant form (stride 2) and otherwise
    (8 + (kh - 1) dil) x (16 + (kw - 1) dil).  Tap-unit: U = 8 when the padded channel count c0k divides by 8, else 4."""
    fam, bn, _, ksw = (int(v) for v in route_order)
    kind = _PRE_KIND[c.pre]
    if fam == HALO_F16:
        hh, hw = (10, 18) if c.stride == 2 else (8 + (c.kh - 1) * c.dil, 16 + (c.kw - 1) * c.dil)
        ni = -(-hh * hw * 8 // 256)
        return ("conv_halo_%d%s" % (bn, "k" if ksw == 1 else ""), kind, 6 if ni <= 6 else (8 if ni <= 8 else 10))
    if fam == TAPUNIT_F16:
        c0k = -(-c.c0 // c.cin_pad) * c.cin_pad
        return ("conv_tapunit_%d" % bn, kind, 8 if c0k % 8 == 0 else 4)
    return None


def _t(tag, B, c0, c1, cout, k, H, W, **kw_):
    return cs.Case(tag="t16_" + tag, B=B, c0=c0, c1=c1, cout=cout, kh=k, kw=k, H=H, W=W, ksplit=1, **kw_)


_PADS = (L.PAD_ZERO, L.PAD_REFLECT, L.PAD_REPLICATE)
_ACTS = (L.ACT_NONE, L.ACT_RELU, L.ACT_TANH)
# (name, k, dil, pad, (c0, c1) choices): K <= 1568 keeps 5 x 5 and 7 x 7 at one 32-channel chunk; 3 x 3 turns the chunk loop over
_KERNELS = (("k3", 3, 1, 1, ((64, 0), (32, 32))), ("k5", 5, 1, 2, ((32, 0),)), ("k7", 7, 1, 3, ((32, 0),)),
            ("k3d3", 3, 3, 3, ((32, 32), (64, 0))))


def tile_cases():
    """The instantiation table: the smallest launches that between them, under SWITCH_SETS, take each of the 63 MODE 3
    instantiations - one 8 x 16 patch at B = 1, or 16 x 32 at B = 3 (patch-in-image and image-in-batch indices, an odd batch, the
    reciprocal divisions), one chunk of 32 input channels or two, K <= 1568 (tests/test_f16_mode_cpu.py: the operand-rounded
    reference of every row must lie > 10 bars from the exact one).  Every ELU row (no operand-exact reference) has a twin with
    pre="relu" on the same shape."""
    rows, seed = [], [200]

    def add(tag, *a, **kw_):
        seed[0] += 1
        rows.append(_t(tag, *a, seed=seed[0], **kw_))

    # ---- halo, k x k: NI 6 / 8 / 10 x pre kind x cout_pad 128 / 64 - under the four switch sets each row takes 32k, then its
    # widest unit (128, 64k), then that unit's M-split sibling (128, 64), then 32
    n = 0
    for ki, (name, k, dil, pad, chans) in enumerate(_KERNELS):
        for ci, cout in enumerate((128, 64)):
            big = (ki + ci) % 2 == 0
            B, H, W = (3, 16, 32) if big else (1, 8, 16)
            c0, c1 = chans[ci % len(chans)]
            for pre in ("elu", "relu", "affine", "affine_relu"):
                if pre == "affine" and ci == 0 or pre == "affine_relu" and ci == 1:
                    continue
                # (the relu row is the ELU row's twin: everything but the pre-op is shared)
                v = n if pre not in ("elu", "relu") else 100 + ki * 2 + ci
                out = ("nhwc", "nchw", "slice")[v % 3]
                add(f"{name}_{pre}_n{cout}_b{B}", B, c0, c1, cout, k, H, W, pad=pad, dil=dil, pm=_PADS[(v + ki) % 3], pre=pre,
                    per_sample=pre.startswith("affine") and v % 2 == 0, res=v % 3 if out != "nchw" else (v // 3) % 3,
                    act=_ACTS[(v // 2) % 3], out=out, out_c_off=8 if out == "slice" else 0)
                n += 1
    # ---- halo, 1 x 1 (NI 6; the router caps it at the 64-column unit and never splits its K over the waves) and the quadrant
    # form (stride 2: NI 6, never K-split): the M-split units 64 and 32 at NI 6
    for pre, ps in (("none", False), ("elu", False), ("relu", False), ("affine_relu", True)):
        add(f"k1_{pre}_n64_b3", 3, 64, 0, 64, 1, 16, 32, pre=pre, per_sample=ps, res=1 if pre == "none" else 0)
    add("k1_two_src_n128_b1", 1, 32, 32, 128, 1, 8, 16, pre="affine", act=L.ACT_RELU)
    add("s2_k3_none_n64_b1", 1, 32, 0, 64, 3, 16, 32, stride=2, pad=1, res=2)
    add("s2_k4_affine_n128_b3", 3, 32, 0, 128, 4, 32, 64, stride=2, pad=1, pm=L.PAD_REFLECT, pre="affine_relu", per_sample=True)
    add("s2_k3_elu_n64_b1", 1, 64, 0, 64, 3, 16, 32, stride=2, pad=1, pre="elu")
    add("s2_k3_relu_n64_b1", 1, 64, 0, 64, 3, 16, 32, stride=2, pad=1, pre="relu")
    # ---- halo, the narrow and the masked column counts: 32, 48 (cout_pad 64: padded columns masked), 12, 3 into a misaligned
    # buffer (the scalar epilogue: K split by default, M split under FUSG_NO_KSPLIT)
    add("k3_none_n32_b3", 3, 64, 0, 32, 3, 16, 32, pad=1, res=1, out="slice", out_c_off=4)
    add("k3_two_src_n48_b3", 3, 32, 32, 48, 3, 16, 32, pad=1, pre="affine_relu", per_sample=True, res=2, pm=L.PAD_REFLECT)
    add("k5_none_n48_b1", 1, 32, 0, 48, 5, 8, 16, pad=2, out="nchw", act=L.ACT_TANH)
    add("k3_none_n12_b2", 2, 32, 0, 12, 3, 8, 16, pad=1, act=L.ACT_TANH, pm=L.PAD_REPLICATE)
    add("k3_none_n3_misaligned", 1, 32, 0, 3, 3, 8, 16, pad=1, out="misaligned")
    add("k7_relu_n3_misaligned_b3", 3, 32, 0, 3, 7, 16, 32, pad=3, pre="relu", out="misaligned", res=1)
    add("k1_none_n3_misaligned", 1, 64, 0, 3, 1, 8, 16, out="misaligned")
    # ---- tap-unit stems: U 4 (c0 3, 4, 12) / 8 (c0 8, 24) x pre kind x units 128 / 64 / 32.  The 128 unit needs cout_pad % 128
    # == 0 and more than 4 K steps (taps c0k > 64: a 3 x 3 from 4 channels stays on the 64 unit)
    n = 0
    for ui, c0s in enumerate(((3, 4, 12), (8, 24))):
        for ci, cout in enumerate((128, 64, 32)):
            k = (3, 5, 7)[(ui + ci) % 3]
            c0 = c0s[ci % len(c0s)]
            if cout == 128 and k * k * (-(-c0 // 4) * 4) <= 64:
                k = 7
            big = (ui + ci) % 2 == 1
            B, H, W = (3, 16, 32) if big else (1, 8, 16)
            for pre in ("elu", "relu", "affine_relu" if ci % 2 else "affine"):
                v = n if pre.startswith("affine") else 100 + ui * 3 + ci
                out = ("nhwc", "slice", "nchw")[v % 3]
                add(f"tap_c{c0}_k{k}_{pre}_n{cout}_b{B}", B, c0, 0, cout, k, H, W, pad=k // 2, pm=_PADS[v % 3], pre=pre,
                    per_sample=pre.startswith("affine") and v % 2 == 1, res=(v // 2) % 3, act=_ACTS[v % 3], out=out,
                    out_c_off=4 if out == "slice" else 0)
                n += 1
    add("tap_c3_k7_s2_none_n64_b2", 2, 3, 0, 64, 7, 32, 32, stride=2, pad=3)
    add("tap_c12_k3_none_n40_b1", 1, 12, 0, 40, 3, 8, 16, pad=1, pm=L.PAD_REFLECT, out="misaligned")
    tags = [c.tag for c in rows]
    assert len(set(tags)) == len(tags), sorted(t for t in tags if tags.count(t) > 1)
    return rows


# ---- operand scales: the mode stages activations UNSCALED (weights carry the per-channel scale s_n), so small activations are
# fp16 subnormals - 11 significant bits hold for staged |a| >= 2^-14, an absolute 2^-25 below
SCALES_X = (1e-6, 1e-5, 1e-4, 1e-2, 1.0, 1e2, 4e3)
SCALES_W = (1e-6, 1.0, 1e3)


def scale_cases():
    """sx x sw on the 32 -> 32 3 x 3 one-patch layer, and one stem."""
    rows = [cs.Case(tag=f"f16_scale_x{sx:g}_w{sw:g}", B=1, c0=32, c1=0, cout=32, kh=3, kw=3, H=8, W=16, pad=1, ksplit=1, sx=sx,
                    sw=sw, seed=300 + 3 * i + j) for i, sx in enumerate(SCALES_X) for j, sw in enumerate(SCALES_W)]
    rows.append(cs.Case(tag="f16_scale_stem_x0.01_w1e-06", B=1, c0=3, c1=0, cout=64, kh=7, kw=7, H=8, W=16, pad=3, ksplit=1,
                        pm=L.PAD_REFLECT, sx=1e-2, sw=1e-6, seed=330))
    return rows


# one row past the range guard: a staged |a| >= 2^15 (sx 2e4: the largest of 4096 normal draws is > 3 sigma)
OVER_RANGE = cs.Case(tag="f16_scale_over_range", B=1, c0=32, c1=0, cout=32, kh=3, kw=3, H=8, W=16, pad=1, ksplit=1, sx=2e4, seed=331)


# ---- wrong restatements of the mode: each must fail the rows named for it (tests/test_f16_mode_cpu.py) ---------------------
def _half_toward_zero(x32: torch.Tensor) -> torch.Tensor:
    """fp32 -> fp16 truncated (round toward zero), as float64."""
    h = x32.half()
    over = h.double().abs() > x32.double().abs()
    bits = h.view(torch.int16).to(torch.int32) & 0xFFFF
    mag = torch.where(over, (bits & 0x7FFF) - 1, bits & 0x7FFF)
    v = (bits & 0x8000) | mag
    return ((v + 0x8000) % 0x10000 - 0x8000).to(torch.int16).view(torch.float16).double()


def restatement(name: str, c: cs.Case, inp: dict) -> torch.Tensor:
    """The float64 result of a subtly wrong reading of the mode's arithmetic:
    "w_unscaled"  weights as plain w.half(), without the per-channel scale s_n;
    "x_flushed"   staged activations with fp16 subnormals flushed to zero;
    "x_truncated" staged activations truncated, not rounded to nearest even;
    "lo_included" the second product of the split too (x = hi + lo): f16x3's activations."""
    x32 = cs.pre_input(c, inp).float()
    xr, w = x32.half().double(), f16_weights(inp["w"])
    if name == "w_unscaled":
        w = inp["w"].half().double()
    elif name == "x_flushed":
        xr = torch.where(xr.abs() < 2.0 ** -14, torch.zeros_like(xr), xr)
    elif name == "x_truncated":
        xr = _half_toward_zero(x32)
    elif name == "lo_included":
        xr = xr + (x32.double() - xr).float().half().double()
    else:
        raise ValueError(name)
    return cs.reference(c, inp, w=w, xp=xr)[0]


def rounded_operands_case(c: cs.Case, inp: dict):
    """(case, inputs) whose EXACT arithmetic is the mode's: the pre-op applied and rounded to fp16, the weights
    f16_mode_weights - so that conv_sweep.mutations mutates the fp16-operand arithmetic.  cs.reference of the pair equals
    operand_rounded(c, inp)."""
    from dataclasses import replace
    xr = cs.pre_input(c, inp).float().half().double()
    c2 = replace(c, c0=c.cin, c1=0, pre="none", per_sample=False)
    inp2 = dict(inp, x0=xr, x1=None, w=f16_weights(inp["w"]))
    return c2, inp2


# ---- the library's router as a dry run on CPU tensors -----------------------------------------------------------------------
def cpu_route_order(c: cs.Case, prec: str = "f16"):
    """fusg_conv2d_route_order = [family, bn / tile, ksplit, ksw] of the ops.conv launch of the case, from the descriptor
    ops._conv_desc builds on CPU tensors (no GPU).  The process-wide switches are those of THIS process."""
    import ctypes as C
    from future_urban_scene_generation_amd import ops
    ho, wo = c.full_hw()

    def nhwc(b, ch, h, w, cpad=4):
        cp = (ch + cpad - 1) // cpad * cpad
        full = torch.zeros(b, h, w, cp).permute(0, 3, 1, 2)
        return full if cp == ch else full[:, :ch]
    plan = cs.make_plan(c, torch.zeros(c.cout, c.cin, c.kh, c.kw), torch.zeros(c.cout))
    x0 = nhwc(c.B, c.c0, c.H, c.W, c.cin_pad)
    x1 = nhwc(c.B, c.c1, c.H, c.W, c.cin_pad) if c.c1 else None
    pre, bstride = None, 0
    if c.pre.startswith("affine"):
        ctot = plan.c0k + plan.c1k
        shape = (c.B, ctot) if c.per_sample else (ctot,)
        pre, bstride = (torch.zeros(shape), torch.zeros(shape)), ctot if c.per_sample else 0
    # the keywords of the GPU launch (test_gpu_conv_sweep._launch builds its own from the same function)
    kw, _ = cs.launch_kwargs(c, c.B, "cpu", prec, pre=pre, pre_bstride=bstride, res=[nhwc(c.B, c.cout, ho, wo) for _ in range(c.res)])
    lib = L.lib()
    with ops.status_scope(torch.zeros(4, dtype=torch.int32)):
        d, _ = ops._conv_desc(plan, x0, x1, **kw)
        lib.fusg_conv2d_plan(C.byref(d))
        out = (C.c_int32 * 4)()
        rc = lib.fusg_conv2d_route_order(C.byref(d), C.byref(out))
    assert rc == 0, (c.tag, rc)
    return [int(v) for v in out]


def fused_block_predicates(device):
    """{precision: (entry_nin_ok, respair_ok, bottleneck_ok, hg_head_ok, up2_phases_ok)} for f16x3, bf16 and f16, on one block of
    each kind at 2 x 64 x 64 under the benchmark's routing batch (at B = 2 without one the router splits the K of these launches,
    and the predicates that ask it would say no whatever the precision).  Asked with the keyword and through the process-wide
    switch; the two must agree."""
    from future_urban_scene_generation_amd import ops
    g = torch.Generator().manual_seed(3)
    pc = lambda co, ci, k, **kw: pack.pack_conv(torch.randn(co, ci, k, k, generator=g) * 0.1, torch.zeros(co), **kw)   # noqa: E731
    nin, res = pc(128, 6, 1), pc(128, 128, 3, pad=1)
    u = ops.nhwc_empty(2, 8, 64, 64, device)[:, :6]
    ra, rb, nb, nc = pc(32, 32, 3, pad=1), pc(32, 32, 3, pad=1), pc(32, 32, 1), pc(32, 32, 1)
    x32 = ops.nhwc_empty(2, 32, 64, 64, device)
    bp = {"c1": pc(128, 256, 1), "c2": pc(128, 128, 3, pad=1), "c3": pc(256, 128, 1)}
    x256 = ops.nhwc_empty(2, 256, 64, 64, device)
    fcp, sc32 = pc(256, 256, 1), pc(32, 256, 1)
    jn = pack.pack_conv(torch.zeros(256, 288, 1, 1), torch.zeros(256), c_split=(256, 32))

    def ask(**kw):
        with ops.route_batch(32):
            return (ops.entry_nin_ok(nin, res, u, **kw), ops.respair_ok(ra, rb, nb, nc, x32, **kw), ops.bottleneck_ok(bp, x256, **kw),
                    ops.hg_head_ok(fcp, sc32, x256, jn, x256, **kw), ops.up2_phases_ok(x32, **kw))
    got = {prec: ask(precision=prec) for prec in ("f16x3", "bf16", "f16")}
    prev = ops.PRECISION
    try:
        for prec in got:
            ops.set_precision(prec)
            assert ask() == got[prec], (prec, ask(), got[prec])
    finally:
        ops.set_precision(prev)
    return got


def coverage_rows():
    """Every row the GPU test launches under "f16" with the table's checks: the instantiation table and the earlier one."""
    return tile_cases() + table_cases() + EXTRA


def predicted(rows=None):
    """{tag: [route_order, instantiation or None]} of this process's dry run (its FUSG_HALO_MINWG / FUSG_NO_KSPLIT)."""
    out = {}
    for c in (coverage_rows() if rows is None else rows):
        ro = cpu_route_order(c)
        inst = instantiation(c, ro)
        out[c.tag] = [ro, None if inst is None else list(inst)]
    return out


if __name__ == "__main__":                                     # the CPU child of the coverage test: f16_cases.py --predict OUT.json
    import json
    import sys
    if len(sys.argv) == 3 and sys.argv[1] == "--predict":
        with open(sys.argv[2], "w") as f:                       # "before": the rows test_f16_sweep ran before the table existed
            json.dump({"table": predicted(), "before": predicted(cs.edge_cases() + table_cases() + EXTRA)}, f)
    else:
        sys.exit("usage: f16_cases.py --predict OUT.json")
