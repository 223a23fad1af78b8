"""The single-pass fp16 precision mode ("f16", include/fusg.h FUSG_PREC_F16) - a helper module of its tests, not a conftest.
Plain torch on the CPU, importable without a GPU.

The mode's arithmetic on a launch that takes the halo or the tap-unit kernel (families 15 / 16):

    a' = RTN_fp16(pre_op(a))        w' = RTN_fp16(w s_n)        acc(fp32) += a' w'        out = act(fmaf(acc, 1 / s_n, bias)) (+ residuals)

`reference_f16` is that arithmetic with exact products and sums, in float64: what the kernels compute up to their fp32
accumulation order, so they are held to it at conv_sweep.BAR_FP32.  `f16_family` maps the family a case takes under bf16 to the
one it takes under f16; `MASK_SHAPES` are the staging shapes of the GPU test (their references must tell the mode from f16x3:
tests/test_f16_mode_cpu.py)."""
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
