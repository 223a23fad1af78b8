"""Sweep of the norm statistics behind every InstanceNorm / LayerNorm - a helper module of the tests, not a conftest.  Plain
torch / numpy on the CPU, importable without a GPU.  Builds on tests/conv_sweep.py (Case, inputs, make_plan, reference,
predict_family).

Two paths give a norm its (scale, shift):
  fused      fusg_conv2d with stats_out: per 32-pixel slot the mean and the centred M2 of every output channel, written by the
             conv epilogue (csrc/conv_kernel.h: epilogue_rows), combined in fp64 by fusg_in/ln_finalize_slots;
  streaming  fusg_chan_stats (pivot-shifted sums per chunk) + fusg_in/ln_finalize.

The slot order is kernel-defined (include/fusg.h), so only order-independent quantities are compared: `combine(slots)` in
float64 against the float64 statistics of the launch's OWN output (the output itself is pinned by the conv sweep), under

    err_mean = |mean - mean64| / mean|y|                              bar 2^-20
    err_var  = |var  - var64 | / (var64 + max|y| sqrt(var64))         bar 2^-18 (conv_sweep.BAR_FP32)

per (b, c) and for the whole-sample LayerNorm moments; a denominator of 0 (a constant channel) means exact equality.  The bars
are derived, not measured: a slot is 32 fp32 values summed in two passes (tree mean, then centred squares), i.e. a handful of
roundings of 2^-24 each relative to mean|y| (mean) and to max|y| sqrt(var) (variance); `emulate_slots` is that arithmetic in
numpy fp32, and tests/test_stats_sweep_cpu.py shows it stays under a quarter of each bar on every case."""
import math
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import torch

import conv_sweep as cs
from conv_sweep import Case, inputs, make_plan, reference, predict_family      # noqa: F401  (the sweep's own helpers)

L = cs.L

BAR_MEAN = 2.0 ** -20
BAR_VAR = cs.BAR_FP32
BAR_FINAL = 2.0 ** -22          # finalisers: float64 on both sides until one rounding to fp32 (2^-24), a few of them in shift
BAR_CHAN = 2.0 ** -18           # streaming path, both forms (against the pivot-shifted denominators)
BAR_WRAPPER = 2.0 ** -20        # the wrappers' nchunk against the direct ABI at nchunk = 1
EPS = float(np.float32(1e-5))   # the C ABI takes eps as a float

HALO_F16, TAPUNIT_F16 = L.CONV_HALO_F16, L.CONV_TAPUNIT_F16      # the single-pass fp16 mode ("f16": tests/f16_cases.py)
STAT_FAMILIES = (cs.GEN_F32, cs.GEN_F16X3, cs.HALO, cs.HALO_S2D, cs.HALO_F32, cs.HALO_BF16, cs.TAPUNIT, cs.TAPUNIT_F32,
                 cs.TAPUNIT_BF16, HALO_F16, TAPUNIT_F16)
# "f16" is carried explicitly by the rows that run it (conv_sweep.PRECISIONS indexes the edge table's `expect` triplets)
PRECISIONS_F16 = cs.PRECISIONS + ("f16",)
NO_STAT_FAMILIES = (cs.POINTWISE, cs.SMALL)       # the router keeps a launch with stats_out off these
# a launch with statistics routes as one with these two families switched off
STATS_ENV = {"FUSG_NO_SMALL": "1", "FUSG_NO_POINTWISE": "1"}


# ---- which launches may write statistics -----------------------------------------------------------------------------------
def planned_ksplit(c: Case, prec: str, ksplit: int) -> int:
    """fusg_conv2d_plan's K split for the case launched with `ksplit` (0: the planner's choice)."""
    g = torch.Generator().manual_seed(0)
    plan = make_plan(c, torch.randn(c.cout, c.cin, c.kh, c.kw, generator=g), torch.zeros(c.cout))
    if prec != "f32":
        ks = cs.small_ksplit(c, plan, {}, ksplit)
        if ks is not None:
            return ks
    ho, wo = c.q_hw()
    return cs.plan_ksplit(c.B * ho * wo, plan.cout_pad, plan.k_pad, prec == "f16x3", 0, ksplit)[1]


def qualifies(c: Case, *, ksplit: int = 1, prec: str = "f32", store: int = L.STORE_NORMAL, nphase: int = 1,
              tiles: bool = False) -> bool:
    """The rule of csrc/conv_igemm.hip (conv2d's `if (d->stats_out)` block and the tile-list / q-origin checks) and
    include/fusg.h (stats_out), restated: act NONE, no residual, NORMAL store, one phase, ksplit <= 1, qh*qw % 32 == 0, a
    channel-contiguous 16-byte aligned destination with cout % 4 == 0 and out_c_off % 4 == 0, no tile list, no q origin."""
    qh, qw = c.q_hw()
    if c.act != L.ACT_NONE or c.res != 0 or store != L.STORE_NORMAL or nphase != 1:
        return False
    if (planned_ksplit(c, prec, ksplit) if ksplit != 1 else 1) > 1:
        return False
    if (qh * qw) % 32 != 0:
        return False
    if c.out not in ("nhwc", "slice") or c.cout % 4 != 0 or c.out_c_off % 4 != 0:
        return False
    if tiles or (c.qwin is not None and (c.qwin[0] != 0 or c.qwin[1] != 0)):
        return False
    return True


def predict_stats_family(c: Case, prec: str, tile: int = 0) -> int:
    """The family of the case launched with statistics and ksplit = 1.  ("f16" routes as "bf16" does, onto its own families.)"""
    if prec == "f16":
        fam = predict_family(c, "bf16", env=STATS_ENV, ksplit=1, tile=tile)
        return {cs.HALO_BF16: HALO_F16, cs.TAPUNIT_BF16: TAPUNIT_F16}.get(fam, fam)
    return predict_family(c, prec, env=STATS_ENV, ksplit=1, tile=tile)


# ---- the cases -------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class StatCase:
    """One launch with statistics: a conv_sweep.Case (run with ksplit = 1), a data variant ("plain"; "bias50": bias 50x the
    output's standard deviation, so mean >> std; "zero_ch": output channel 1 has all-zero weights, a constant channel), an
    explicit tile of the generic gathers (0: automatic) and the precisions it runs at."""
    case: Case
    variant: str = "plain"
    tile: int = 0
    precs: Tuple[str, ...] = cs.PRECISIONS

    @property
    def tag(self) -> str:
        return self.case.tag + ("" if self.variant == "plain" else "+" + self.variant) + (f"+tile{self.tile}" if self.tile else "")


ZERO_CH = 1


def stat_inputs(sc: StatCase) -> dict:
    """conv_sweep.inputs of the case with the data variant applied."""
    inp = inputs(sc.case)
    if sc.variant == "bias50":
        y0 = reference(sc.case, dict(inp, b=torch.zeros_like(inp["b"])))[0]
        std = float(y0.std())
        k = torch.arange(sc.case.cout, dtype=torch.float32)
        inp["b"] = (50.0 * std * (1.0 + 0.25 * torch.cos(k)) * (1 - 2 * (k % 2))).float()     # both signs, 37 .. 63 std
    elif sc.variant == "zero_ch":
        w = inp["w"].clone()
        w[ZERO_CH] = 0
        inp["w"] = w
    else:
        assert sc.variant == "plain", sc.variant
    return inp


def _c(tag, B, c0, cout, kh, kw, H, W, **kw_):
    return Case(tag=tag, B=B, c0=c0, c1=0, cout=cout, kh=kh, kw=kw, H=H, W=W, ksplit=1, **kw_)


_GEN_TILES = {4: (L.TILE_128x32,), 36: (L.TILE_128x32, L.TILE_64x64, L.TILE_128x64), 64: (L.TILE_64x64, L.TILE_128x64),
              160: (L.TILE_128x32,), 128: (L.TILE_128x128, L.TILE_64x128)}


def _added():
    rows = []
    # generic gathers: B = 3, output 8 x 12 -> M = 288 = 2 * 128 + 32: a partial last M tile, and a 128-row tile that spans two
    # images.  c0 = 12 keeps the halo / tap-unit kernels off (3 x 3, 12 channels: wfrag_order None).  Every tile explicitly,
    # f32 and f16x3 (cout 128 is there for the two 128-column tiles, which need cout_pad % 128 == 0).
    for cout, tiles in _GEN_TILES.items():
        g = _c(f"st_gen_c{cout}", 3, 12, cout, 3, 3, 8, 12, pad=1)
        rows.append(StatCase(g, precs=("f32", "f16x3")))
        for t in tiles:
            rows.append(StatCase(g, tile=t, precs=("f32", "f16x3")))
    g = _c("st_gen_c36", 3, 12, 36, 3, 3, 8, 12, pad=1)
    rows += [StatCase(g, "bias50", precs=("f32", "f16x3")), StatCase(g, "zero_ch", precs=("f32", "f16x3")),
             StatCase(replace(g, tag="st_gen_small", sx=1e-3, sw=1e-3), precs=("f32", "f16x3")),
             StatCase(replace(g, tag="st_gen_large", sx=1e3, sw=1e3), precs=("f32", "f16x3")),
             StatCase(replace(g, tag="st_gen_b1", B=1), precs=("f32", "f16x3")),
             StatCase(replace(g, tag="st_gen_slice8", out="slice", out_c_off=8), precs=("f32", "f16x3"))]
    n_generic = len(rows)
    # halo kernels.  The launcher's rule for the in-workgroup K split (csrc/conv_igemm.hip, conv2d's halo branch):
    #     r->bn  = column_tile(cout_pad, ntaps == 1 ? 64 : 128, mt, halo_minwg)   // halved while mt * cout_pad / bn < 512
    #     r->ksw = !s2d && !d->tile_list && !no_ksplit && mt * (cout_pad / r->bn) <= 1024 &&
    #              ((r->bn == 32 && ntaps >= 4) || (r->bn == 64 && ntaps >= 2));
    # On these grids (mt <= 8 patches) the column tile is always 32, so a stride-1 layer with >= 4 taps (3 x 3: 9) takes the
    # K-split epilogue (`statk`) and one with fewer (1 x 1, 1 x 3) or in parity-quadrant form (s2d) the plain one (`statfn`).
    for cout in (32, 48, 128):
        rows.append(StatCase(_c(f"st_halo_k3_8x16_c{cout}", 1, 32, cout, 3, 3, 8, 16, pad=1)))               # ksw: 9 taps
        rows.append(StatCase(_c(f"st_halo_k1_16x32_c{cout}", 2, 64, cout, 1, 1, 16, 32)))                     # plain: 1 tap
    rows += [StatCase(_c("st_halo_k3_16x32_b2", 2, 32, 48, 3, 3, 16, 32, pad=1, pm=L.PAD_REFLECT)),        # ksw
             StatCase(_c("st_halo_1x3_8x16", 1, 32, 32, 1, 3, 8, 16, pad=0, pad_w=1)),                       # plain: 3 taps
             StatCase(_c("st_s2d_k3_row", 2, 32, 48, 3, 3, 16, 64, stride=2, pad=1)),                       # quadrants: plain
             StatCase(_c("st_s2d_k4_reflect", 1, 32, 32, 4, 4, 16, 32, stride=2, pad=1, pm=L.PAD_REFLECT))]
    h = _c("st_halo_k3_8x16_c48", 1, 32, 48, 3, 3, 8, 16, pad=1)
    p = _c("st_halo_k1_16x32_c48", 2, 64, 48, 1, 1, 16, 32)
    s = _c("st_s2d_k3_row", 2, 32, 48, 3, 3, 16, 64, stride=2, pad=1)
    for base in (h, p, s):
        rows += [StatCase(base, "bias50"), StatCase(base, "zero_ch")]
    rows += [StatCase(replace(h, tag="st_halo_k3_small", sx=1e-3, sw=1e-3)), StatCase(replace(h, tag="st_halo_k3_large", sx=1e3, sw=1e3)),
             StatCase(replace(p, tag="st_halo_k1_small", sx=1e-3, sw=1e-3)), StatCase(replace(p, tag="st_halo_k1_large", sx=1e3, sw=1e3)),
             StatCase(replace(s, tag="st_s2d_k3_small", sx=1e-3, sw=1e-3)), StatCase(replace(s, tag="st_s2d_k3_large", sx=1e3, sw=1e3)),
             StatCase(replace(h, tag="st_halo_k3_slice4", out="slice", out_c_off=4))]
    # tap-unit stems: the 7 x 7 and 3 x 3 few-channel layers of the edge table, at 8 x 16 and 16 x 16 (column tiles 32, 64, 128)
    t7 = _c("st_tap_c3_7x7_8x16", 1, 3, 64, 7, 7, 8, 16, pad=3, pm=L.PAD_REFLECT)
    t3 = _c("st_tap_c24_3x3_16x16", 2, 24, 32, 3, 3, 16, 16, pad=1)
    rows += [StatCase(t7), StatCase(t3), StatCase(_c("st_tap_c3_7x7_16x16_c128", 1, 3, 128, 7, 7, 16, 16, pad=3)),
             StatCase(_c("st_tap_c8_3x3_8x16_c36", 3, 8, 36, 3, 3, 8, 16, pad=1)),
             StatCase(t7, "bias50"), StatCase(t7, "zero_ch"), StatCase(t3, "bias50"), StatCase(t3, "zero_ch"),
             StatCase(replace(t7, tag="st_tap_7x7_small", sx=1e-3, sw=1e-3)), StatCase(replace(t7, tag="st_tap_7x7_large", sx=1e3, sw=1e3)),
             StatCase(replace(t3, tag="st_tap_3x3_slice4", out="slice", out_c_off=4))]
    # the halo and tap-unit rows run under the single-pass fp16 mode too (families 15 / 16: `epilogue_vec16` per half with
    # `stath` on the tile that leaves in two halves, the K-split `statk`)
    rows[n_generic:] = [replace(r, precs=PRECISIONS_F16) for r in rows[n_generic:]]
    return rows


def stat_cases():
    """Every row of the conv sweep's edge table that qualifies (launched with ksplit = 1) and the added rows."""
    rows = [StatCase(replace(c, ksplit=1)) for c in cs.edge_cases() if qualifies(c, ksplit=1)]
    rows += _added()
    tags = [r.tag for r in rows]
    assert len(set(tags)) == len(tags), sorted(t for t in tags if tags.count(t) > 1)
    return rows


def halo_takes_ksplit(c: Case, prec: str) -> Optional[bool]:
    """Does the launch (a halo family, default switches, grids of < 512 workgroups: column tile 32) take the in-workgroup
    K-split epilogue?  None: not a halo family."""
    fam = predict_stats_family(c, prec)
    if fam not in (cs.HALO, cs.HALO_S2D, cs.HALO_F32, cs.HALO_BF16, HALO_F16):
        return None
    s2d = c.stride == 2
    return (not s2d) and c.kh * c.kw >= 4


# launches that must NOT write statistics, one per condition of the rule: (tag, case, extra launch keywords)
def negative_cases():
    g = _c("neg", 2, 12, 36, 3, 3, 8, 12, pad=1)
    h = _c("neg_halo", 1, 32, 32, 3, 3, 16, 32, pad=1)
    return [
        ("act", replace(g, tag="neg_act", act=L.ACT_RELU), {}),
        ("residual", replace(g, tag="neg_res", res=1), {}),
        ("cout%4", replace(g, tag="neg_cout38", cout=38), {}),
        ("qh*qw%32", replace(g, tag="neg_hw88", W=11), {}),
        ("planner_ksplit", replace(_c("neg_ksplit", 1, 64, 32, 3, 3, 8, 16, pad=1), ksplit=0), {}),      # K = 576: split 4
        ("misaligned", replace(g, tag="neg_misaligned", out="misaligned"), {}),
        ("nchw_out", replace(g, tag="neg_nchw", out="nchw"), {}),
        ("d2s_store", replace(g, tag="neg_d2s", cout=64), {"store": L.STORE_D2S}),
        ("q_origin", replace(g, tag="neg_qwin", pm=L.PAD_REPLICATE, H=9, qwin=(1, 0, 8, 12)), {}),
        ("tiles", h, {"tiles": True}),
    ]


# ---- float64 statistics, slots, combine, comparator ------------------------------------------------------------------------
def direct(y: torch.Tensor) -> dict:
    """Float64 statistics of y [B, C, H, W]: per (b, c) mean / biased var / mean|y| / max|y|; per b the LayerNorm moments (mean,
    unbiased var, mean|y|, max|y|)."""
    y = y.to(torch.float64)
    B, C = y.shape[:2]
    f = y.reshape(B, C, -1)
    a = y.reshape(B, -1)
    return {"mean": f.mean(2), "var": f.var(2, unbiased=False), "absmean": f.abs().mean(2), "absmax": f.abs().amax(2),
            "ln_mean": a.mean(1), "ln_var": a.var(1, unbiased=True) if a.shape[1] > 1 else torch.zeros(B, dtype=torch.float64),
            "ln_absmean": a.abs().mean(1), "ln_absmax": a.abs().amax(1)}


def combine(slots: torch.Tensor) -> dict:
    """slots [B, n, C, 2] = (mean, centred M2) of 32 values each -> float64 per (b, c) mean, M2, biased var, and the
    whole-sample mean and unbiased variance (std = sqrt) the LayerNorm uses.  Order-independent."""
    s = slots.to(torch.float64)
    B, n, C, _ = s.shape
    ms, m2s = s[..., 0], s[..., 1]
    mean = ms.mean(1)
    m2 = m2s.sum(1) + 32.0 * ((ms - mean[:, None]) ** 2).sum(1)
    ln_mean = ms.reshape(B, -1).mean(1)
    ln_m2 = m2s.reshape(B, -1).sum(1) + 32.0 * ((ms.reshape(B, -1) - ln_mean[:, None]) ** 2).sum(1)
    return {"mean": mean, "m2": m2, "var": m2 / (32.0 * n), "ln_mean": ln_mean, "ln_var": ln_m2 / (32.0 * n * C - 1.0)}


def _groups(y: torch.Tensor, geometry: str) -> torch.Tensor:
    """y [B, C, H, W] -> [B, n, C, 32]: the 32-pixel slots, "rows" (row-major runs of 32 pixels: the generic gathers) or
    "halo" (the four 2 x 16 row pairs of every 8 x 16 patch: the halo and tap-unit kernels)."""
    B, C, H, W = y.shape
    if geometry == "rows":
        assert (H * W) % 32 == 0
        return y.reshape(B, C, H * W // 32, 32).permute(0, 2, 1, 3)
    assert geometry == "halo" and H % 8 == 0 and W % 16 == 0
    t = y.reshape(B, C, H // 8, 4, 2, W // 16, 16).permute(0, 2, 5, 3, 1, 4, 6)          # [B, py, px, pair, C, 2, 16]
    return t.reshape(B, (H // 8) * (W // 16) * 4, C, 32)


def host_slots(y: torch.Tensor, geometry: str = "rows") -> torch.Tensor:
    """Exact (float64) slots of y."""
    g = _groups(y.to(torch.float64), geometry)
    mean = g.mean(3)
    return torch.stack([mean, ((g - mean[..., None]) ** 2).sum(3)], 3)


def emulate_slots(y32: torch.Tensor, geometry: str = "rows") -> torch.Tensor:
    """The epilogue's slot arithmetic in numpy fp32: a pairwise-tree sum of the 32 values times 1/32, then the tree sum of the
    squared fp32 differences from that mean.  Returns float32 slots [B, n, C, 2]."""
    g = _groups(y32.to(torch.float32), geometry).contiguous().numpy().astype(np.float32)

    def tree(a):
        while a.shape[-1] > 1:
            a = (a[..., ::2] + a[..., 1::2]).astype(np.float32)
        return a[..., 0]
    mean = (tree(g) * np.float32(1.0 / 32.0)).astype(np.float32)
    dv = (g - mean[..., None]).astype(np.float32)
    m2 = tree((dv * dv).astype(np.float32))
    return torch.from_numpy(np.stack([mean, m2], -1))


def _rel(diff: torch.Tensor, den: torch.Tensor) -> float:
    """max diff / den; where den == 0 the difference must be exactly 0 (else infinitely wrong); NaN counts as infinite."""
    diff, den = diff.to(torch.float64).abs(), den.to(torch.float64)
    e = torch.where(den > 0, diff / torch.where(den > 0, den, torch.ones_like(den)),
                    torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, math.inf)))
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, math.inf))
    return float(e.max()) if e.numel() else 0.0


def stat_errs(got: dict, ref: dict) -> dict:
    """The comparator: `got` = combine(slots), `ref` = direct(output).  Errors against BAR_MEAN (mean, ln_mean) and BAR_VAR
    (var, ln_var)."""
    return {"mean": _rel(got["mean"] - ref["mean"], ref["absmean"]),
            "var": _rel(got["var"] - ref["var"], ref["var"] + ref["absmax"] * ref["var"].sqrt()),
            "ln_mean": _rel(got["ln_mean"] - ref["ln_mean"], ref["ln_absmean"]),
            "ln_var": _rel(got["ln_var"] - ref["ln_var"], ref["ln_var"] + ref["ln_absmax"] * ref["ln_var"].sqrt())}


def over_bars(e: dict, frac: float = 1.0):
    """The entries of stat_errs' result above `frac` of their bars."""
    bars = {"mean": BAR_MEAN, "ln_mean": BAR_MEAN, "var": BAR_VAR, "ln_var": BAR_VAR}
    return {k: v for k, v in e.items() if not v <= frac * bars[k]}


# ---- finalisers on the host (float64) --------------------------------------------------------------------------------------
def in_scale_shift(mean: torch.Tensor, var: torch.Tensor, eps: float = EPS):
    """InstanceNorm2d: y * scale + shift = (y - mean) / sqrt(var + eps).  Returns (scale, shift, shift's denominator)."""
    rstd = 1.0 / torch.sqrt(var + eps)
    return rstd, -mean * rstd, mean.abs() * rstd


def ln_scale_shift(ln_mean: torch.Tensor, ln_var: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = EPS):
    """The ICN's LayerNorm: (y - mean) / (std + eps) * gamma + beta with the unbiased whole-sample std.  [B, C] each."""
    g, bt = gamma.to(torch.float64)[None], beta.to(torch.float64)[None]
    sc = g / (ln_var.sqrt() + eps)[:, None]
    return sc, bt - ln_mean[:, None] * sc, ln_mean.abs()[:, None] * sc.abs() + bt.abs()


def final_errs(scale, shift, ref) -> Tuple[float, float]:
    """(scale error relative to |scale|, shift error relative to |mean| rstd + |beta|) of device results against
    in_scale_shift / ln_scale_shift's float64 (scale, shift, den)."""
    rs, rh, den = ref
    return (_rel(scale.detach().cpu().double() - rs, rs.abs()), _rel(shift.detach().cpu().double() - rh, den))


FINAL_SHAPES = [(B, n, C) for B in (1, 3) for n in (1, 3, 12, 16, 17, 36) for C in (4, 16, 20, 36, 256)]
CONST_CH = 1


def synthetic_slots(B: int, nslots: int, C: int, seed: int = 0):
    """(slots float32 [B, nslots, C, 2], y float64 [B, C, nslots, 32]) with y's exact slot statistics EQUAL to the fp32 slots:
    y is drawn in float64, its slots are rounded to fp32, and each slot of y is then moved and rescaled onto the rounded values.
    Channels differ in offset (0 .. 1000 std: mean >> std) and scale; channel 1 is constant."""
    g = torch.Generator().manual_seed(7000 + seed + 131 * B + 17 * nslots + C)
    y = torch.randn(B, C, nslots, 32, generator=g, dtype=torch.float64)
    k = torch.arange(C, dtype=torch.float64).view(1, C, 1, 1)
    y = (y * torch.pow(10.0, (k % 7) - 3) + torch.pow(10.0, (k % 7) - 3) * torch.tensor([0.0, 3.0, 50.0, 1000.0])[(k.long() % 4)])
    y[:, CONST_CH] = 0.75
    mean = y.mean(3, keepdim=True)
    m2 = ((y - mean) ** 2).sum(3, keepdim=True)
    mean32, m232 = mean.float().double(), m2.float().double()
    ratio = torch.where(m2 > 0, torch.sqrt(m232 / torch.where(m2 > 0, m2, torch.ones_like(m2))), torch.zeros_like(m2))
    y = mean32 + (y - mean) * ratio
    slots = torch.stack([mean32[..., 0], m232[..., 0]], 3).permute(0, 2, 1, 3).contiguous().float()      # [B, n, C, 2]
    return slots, y


# ---- the streaming path ----------------------------------------------------------------------------------------------------
CHAN_C = (4, 12, 64, 256, 260, 320)          # 260: a second channel block holding a single quad
CHAN_HW = {1: (1, 1), 2: (1, 2), 31: (1, 31), 33 * 17: (33, 17), 4096: (64, 64)}


def chan_nchunks(hw: int):
    return sorted({n for n in (1, 2, 7, hw, hw + 3, 4096) if 1 <= n <= 4096})


@dataclass(frozen=True)
class ChanCase:
    """One input of fusg_chan_stats: [B, C, h, w]; kind "plain", "outlier" (pixel 0 of every channel 1000 std away: the pivot),
    "cpad32" (channel pitch padded to a multiple of 32), "slice" (channels 8 .. 8 + C of a buffer of C + 16), "centred"
    (pixel 0 of every channel is the channel's mean: the pivot shift then cancels nothing)."""
    C: int
    hw: int
    B: int = 2
    kind: str = "plain"

    @property
    def tag(self) -> str:
        return f"c{self.C}_hw{self.hw}_b{self.B}_{self.kind}"


def chan_cases():
    rows = [ChanCase(C, hw) for C in CHAN_C for hw in CHAN_HW]
    rows += [ChanCase(64, 33 * 17, 3, "outlier"), ChanCase(12, 4096, 2, "outlier"), ChanCase(20, 33 * 17, 2, "cpad32"),
             ChanCase(36, 33 * 17, 2, "slice"), ChanCase(4, 1, 1), ChanCase(260, 31, 1)]
    return rows


# The wrappers' chunk count against the direct ABI at nchunk = 1, at BAR_WRAPPER = 2^-20 on (scale, shift).  One chunk is the
# LEAST accurate way to run the kernel: a result is a chain of L + pl - 1 fp32 additions (L = ceil(HW / pl) pixels per lane, then
# lane 0 adds the pl lanes in order), a random walk of about u sqrt((L + pl) / 3), u = 2^-24, on each sum; var = E[v^2] - E[v]^2
# then amplifies it by 1 + d^2, d = |pivot - mean| / std, and rstd takes half.  With a pivot drawn like any pixel (d up to
# ~2.5 over a few hundred channels: 1 + d^2 ~ 7) the one-chunk run ALONE is 4e-7 .. 4e-6 from float64 at HW = 561 .. 4096
# (emulate_chan_stats shows the same figures on the CPU), i.e. at or over the bar it is supposed to serve as the reference
# for, while the wrappers' nchunk stays within 4e-7.  So the comparison is made where one chunk is a fair reference: "centred"
# inputs (d = 0) with L + pl <= 768, where the model gives u sqrt(768 / 3) / 2 = 4.8e-7 = half the bar.  The plain inputs'
# figures are recorded beside it.
WRAPPER_SHAPES = ((12, 33 * 17), (64, 33 * 17), (260, 33 * 17), (12, 4096), (64, 4096))


def chan_chain_length(C: int, hw: int) -> int:
    """The longest chain L + pl of fp32 additions behind one partial sum at nchunk = 1."""
    worst = 0
    for cg0 in range(0, C // 4, 64):
        nq = min(64, C // 4 - cg0)
        pl = 1 << ((256 // nq).bit_length() - 1)
        worst = max(worst, -(-hw // pl) + pl)
    return worst


def chan_input(cc: ChanCase) -> torch.Tensor:
    """float32 [B, C, h, w]: mean 5 std 2 (the pivot shift at work), per-channel factors 1/4 .. 4."""
    h, w = CHAN_HW[cc.hw]
    g = torch.Generator().manual_seed(9000 + 7 * cc.C + cc.hw + cc.B)
    k = torch.arange(cc.C, dtype=torch.float32).view(1, cc.C, 1, 1)
    x = (torch.randn(cc.B, cc.C, h, w, generator=g) * 2 + 5) * torch.pow(2.0, (k % 5) - 2)
    if cc.kind == "outlier":
        x[:, :, 0, 0] += 1000.0 * 2 * torch.pow(2.0, (k[0, :, 0, 0] % 5) - 2)
    if cc.kind == "centred":
        x[:, :, 0, 0] = x.double().mean((2, 3)).float()
    return x.float()


def emulate_chan_stats(x: torch.Tensor, nchunk: int) -> torch.Tensor:
    """chan_stats_kernel (csrc/norm.hip) in numpy fp32, in its accumulation order: per channel block of <= 64 quads, pl = the
    largest power of two with nq * pl <= 256 pixel lanes; lane j sums v = x - pivot and v * v over pixels p0 + j, p0 + j + pl,
    ... of its chunk, lane 0 then adds lanes 1 .. pl - 1 in order.  x [B, C, h, w] -> partial float32 [B, nchunk, C, 2]."""
    B, C, h, w = x.shape
    HW = h * w
    xs = x.permute(0, 2, 3, 1).reshape(B, HW, C).numpy().astype(np.float32)
    v = (xs - xs[:, :1]).astype(np.float32)
    per = -(-HW // nchunk)
    out = np.zeros((B, nchunk, C, 2), np.float32)
    C4 = C // 4
    for cg0 in range(0, C4, 64):
        nq = min(64, C4 - cg0)
        pl = 1 << ((256 // nq).bit_length() - 1)
        steps = -(-per // pl)
        ch = slice(cg0 * 4, (cg0 + nq) * 4)
        buf = np.zeros((B, nchunk * per, nq * 4), np.float32)          # pixels past HW add +0: as good as skipped
        n_in = min(HW, nchunk * per)
        buf[:, :n_in] = v[:, :n_in, ch]
        buf = buf.reshape(B, nchunk, per, nq * 4)
        lanes = np.zeros((B, nchunk, steps * pl, nq * 4), np.float32)
        lanes[:, :, :per] = buf
        lanes = lanes.reshape(B, nchunk, steps, pl, nq * 4)
        s1 = np.zeros((B, nchunk, pl, nq * 4), np.float32)
        s2 = np.zeros_like(s1)
        for s in range(steps):
            t = lanes[:, :, s]
            s1 = (s1 + t).astype(np.float32)
            s2 = (s2 + (t * t).astype(np.float32)).astype(np.float32)
        a1, a2 = s1[:, :, 0], s2[:, :, 0]
        for j in range(1, pl):
            a1 = (a1 + s1[:, :, j]).astype(np.float32)
            a2 = (a2 + s2[:, :, j]).astype(np.float32)
        out[:, :, ch, 0], out[:, :, ch, 1] = a1, a2
    return torch.from_numpy(out)


def chan_combine(partial: torch.Tensor, x: torch.Tensor) -> dict:
    """What fusg_in_finalize / fusg_ln_finalize compute from the partial sums, in float64: per (b, c) mean and biased var, the
    whole-sample mean and unbiased var."""
    B, C, h, w = x.shape
    n = float(h * w)
    p = partial.to(torch.float64)
    piv = x[:, :, 0, 0].to(torch.float64)
    s1, s2 = p[..., 0].sum(1), p[..., 1].sum(1)
    ms = s1 / n
    var = (s2 / n - ms * ms).clamp_min(0.0)
    mean = piv + ms
    ln_mean = mean.mean(1)
    m2c = (s2 - s1 * s1 / n).clamp_min(0.0)
    ln_m2 = (m2c + n * (mean - ln_mean[:, None]) ** 2).sum(1)
    return {"mean": mean, "var": var, "ln_mean": ln_mean, "ln_var": ln_m2 / max(n * C - 1.0, 1.0)}


def chan_errs(got: dict, x: torch.Tensor) -> dict:
    """The streaming comparator, on the quantities the algorithm accumulates: v = x - x[b, 0, 0, c].  mean against
    mean|v| + |pivot| 2^-4, var against var + max|v| sqrt(mean v^2); the whole-sample moments against the same forms taken
    over the sample.  All four against BAR_CHAN."""
    x = x.to(torch.float64)
    B, C = x.shape[:2]
    ref = direct(x)
    piv = x[:, :, :1, :1]
    v = (x - piv).reshape(B, C, -1)
    piv = piv.reshape(B, C)
    dm = v.abs().mean(2) + piv.abs() / 16
    dv = ref["var"] + v.abs().amax(2) * (v * v).mean(2).sqrt()
    va = v.reshape(B, -1)
    return {"mean": _rel(got["mean"] - ref["mean"], dm), "var": _rel(got["var"] - ref["var"], dv),
            "ln_mean": _rel(got["ln_mean"] - ref["ln_mean"], dm.mean(1)),
            "ln_var": _rel(got["ln_var"] - ref["ln_var"], ref["ln_var"] + va.abs().amax(1) * (va * va).mean(1).sqrt())}
