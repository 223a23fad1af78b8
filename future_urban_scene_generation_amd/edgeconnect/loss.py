"""Drop-in for the reference's ``edgeconnect.loss``, forward only: ``VGG19`` (the sixteen ReLU taps of VGG-19 configuration
E), ``PerceptualLoss(weights)`` (L1 distance of the activations at relu1_1, 2_1, 3_1, 4_1, 5_1) and ``StyleLoss()`` (L1
distance of the Gram matrices of relu2_2, 3_4, 4_4, 5_2), with the reference's constructor arguments, ``state_dict`` keys and
call signatures.  ``AdversarialLoss`` belongs to training and raises on construction; ``AdversarialScore`` computes its values
forward only, and ``feature_matching`` the discriminator feature-matching sum.

``VGG19`` holds the ``features`` weights of a torchvision ``vgg19`` under the reference's names (``relu1_1.0.weight`` ...
``relu5_4.34.bias``); ``load_torchvision(sd)`` takes a torchvision state dict (``features.N.*``).  Nothing is downloaded:
until weights are loaded the module holds the deterministic synthetic ones of ``synth_state_dict("vgg", ...)``, and parity
with torchvision's own module stays unpinned like the CAD classifier's.

Execution: the CAD classifier's convolutions (3 x 3 + fused ReLU, the tap-unit stem, ``ops.maxpool2``), the Gram matrix by
``ops.gram`` (exact-fp32 matrix instruction, contraction over pixels) and every L1 sum by ``ops.abs_diff_rows`` (float64, per
row).  ``feature_distances`` is the per-row form both losses are means of; it never synchronises with the host.  Under
``precision="bf16"`` and ``precision="f16"`` the convolutions run f16x3, as ``VGG19Classifier.forward`` does: a measure must not be noisier than what
it measures.  No autograd: inputs are detached.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional, Sequence

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops, pack
from ..cad_classifier import CFG_E, vgg19_schema
from ..nn_base import ConvP, FusedNet, entry_point
from ..synth import synth_state_dict

FUSG_DROPIN = True


def _tap_table():
    """[(tap name, torchvision features index of its conv, cin, cout, pooled before it)] in network order."""
    out, idx, cin, block, k, pooled = [], 0, 3, 1, 1, False
    for v in CFG_E:
        if v == "M":
            idx, block, k, pooled = idx + 1, block + 1, 1, True
            continue
        out.append((f"relu{block}_{k}", idx, cin, v, pooled))
        idx, cin, k, pooled = idx + 2, v, k + 1, False
    return out


TAPS = tuple(_tap_table())
TAP_NAMES = tuple(t[0] for t in TAPS)
PERCEPTUAL_TAPS = ("relu1_1", "relu2_1", "relu3_1", "relu4_1", "relu5_1")
STYLE_TAPS = ("relu2_2", "relu3_4", "relu4_4", "relu5_2")
USED_TAPS = tuple(n for n in TAP_NAMES if n in PERCEPTUAL_TAPS + STYLE_TAPS)
LAST_USED = "relu5_2"
FEATURE_DISTANCE_COLUMNS = tuple(f"perceptual_{n}" for n in PERCEPTUAL_TAPS) + tuple(f"style_{n}" for n in STYLE_TAPS)
MAX_ROWS = 64                                                  # rows per VGG pass of feature_distances


def vgg19_features_schema() -> "OrderedDict[str, tuple]":
    """The ``features.N.*`` part of the CAD classifier's schema: the keys of a torchvision vgg19's convolutions."""
    return OrderedDict((k, v) for k, v in vgg19_schema(10).items() if k.startswith("features."))


class VGG19(FusedNet):
    def __init__(self, seed: int = 0):
        super().__init__()
        for name, idx, cin, cout, _ in TAPS:
            self.add_module(name, nn.ModuleDict({str(idx): ConvP(cin, cout, 3)}))
        self.load_torchvision(synth_state_dict("vgg", vgg19_features_schema(), seed))
        for p in self.parameters():
            p.requires_grad = False
        self.eval()

    def load_torchvision(self, sd) -> None:
        """Load the ``features.N.{weight, bias}`` entries of a torchvision ``vgg19`` state dict (``classifier.*`` and anything
        else is ignored; a missing or mis-shaped entry is an error)."""
        own = OrderedDict()
        for name, idx, cin, cout, _ in TAPS:
            for leaf, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
                key = f"features.{idx}.{leaf}"
                if key not in sd:
                    raise KeyError(f"VGG19.load_torchvision: {key} is missing")
                if tuple(sd[key].shape) != shape:
                    raise ValueError(f"VGG19.load_torchvision: {key} is {tuple(sd[key].shape)}, expected {shape}")
                own[f"{name}.{idx}.{leaf}"] = sd[key].detach().to(torch.float32)
        self.load_state_dict(own)

    def _build_plans(self, device) -> dict:
        P = {}
        for name, idx, _, _, _ in TAPS:
            m = getattr(self, name)[str(idx)]
            P[name] = pack.pack_conv(m.weight, m.bias, pad=1).to(device)
        return P

    def train(self, mode: bool = True):
        """Forward-only: the module stays in eval mode whatever its parent is switched to."""
        return super().train(False)

    @staticmethod
    def _check_input(x: torch.Tensor) -> None:
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] < 16 or x.shape[3] < 16 or x.shape[2] % 16 or x.shape[3] % 16:
            raise ValueError(f"VGG19 expects [B, 3, H, W] with H and W multiples of 16 (at least 16), got {tuple(x.shape)}")
        if not x.is_floating_point():
            raise ValueError(f"VGG19 expects a float tensor, got {x.dtype}")

    def _run(self, x: torch.Tensor, last: str, keep: Sequence[str]) -> "OrderedDict[str, torch.Tensor]":
        """The taps in `keep` up to `last`, NHWC-physical, convolutions at the current precision (bf16, f16 -> f16x3)."""
        if ops.PRECISION in ("bf16", "f16"):
            with ops.precision("f16x3"):
                return self._run(x, last, keep)
        P = self._ensure(x)
        t = ops.as_nhwc(x.detach().to(torch.float32))
        out = OrderedDict()
        for name, _, _, _, pooled in TAPS:
            if pooled:
                t = ops.maxpool2(t)
            t = ops.conv(P[name], t, act=L.ACT_RELU)
            if name in keep:
                out[name] = t
            if name == last:
                break
        return out

    @entry_point
    def forward(self, x: torch.Tensor) -> dict:
        """The reference's dict of sixteen activations, each a contiguous [B, C, h, w] tensor."""
        self._check_input(x)
        return {k: ops.to_nchw(v) for k, v in self._run(x, TAP_NAMES[-1], TAP_NAMES).items()}

    @entry_point
    def taps(self, x: torch.Tensor) -> dict:
        """The internal form: stops after relu5_2 and keeps the nine taps the two distances read, in the NHWC-physical
        layout `ops.gram` takes (logical shape [B, C, h, w])."""
        self._check_input(x)
        return self._run(x, LAST_USED, USED_TAPS)


def _as_input(t: torch.Tensor, what: str) -> torch.Tensor:
    """float [B, 3, H, W] as it is; uint8 [B, H, W, 3] as / 255."""
    t = t.detach()
    if t.dtype == torch.uint8:
        if t.dim() != 4 or t.shape[3] != 3:
            raise ValueError(f"{what}: a uint8 input must be [B, H, W, 3], got {tuple(t.shape)}")
        return t.permute(0, 3, 1, 2).to(torch.float32) / 255.0
    return t.to(torch.float32)


def _stack_rows(parts):
    """NHWC-physical tensors of one shape but the batch, joined along the batch (still NHWC-physical)."""
    if len(parts) == 1:
        return parts[0]
    return torch.cat([p.permute(0, 2, 3, 1) for p in parts], 0).permute(0, 3, 1, 2)


def feature_sums(vgg: VGG19, x: torch.Tensor, y: torch.Tensor):
    """The launches of `feature_distances`: (sums, counts, word) with sums float64 [9, B] on the device - per column the per-row
    sum of |f(x) - f(y)| resp. |G(x) - G(y)|, each row of the table written by its own `ops.abs_diff_rows` -, counts the nine
    element counts the sums are divided by, and word the range-status word the convolutions reported to.  x, y: float32
    [B, 3, H, W] of one shape.  Everything here is a library launch, so a pass recorded with `ops.PlanRecorder` replays on
    whatever x and y hold by then (at most `MAX_ROWS` stacked rows: larger batches are joined by torch)."""
    B, _, H, W = x.shape
    if ops.RECORDER is not None and 2 * B > MAX_ROWS:
        raise ValueError(f"feature_sums: a recorded pass holds at most {MAX_ROWS // 2} pairs, got {B}")
    buf = torch.empty((2 * B, H, W, 4), device=x.device, dtype=torch.float32)
    full = buf.permute(0, 3, 1, 2)
    ops.copy4d(x, full[:B], 4)                                 # NCHW or NHWC in, NHWC pitch 4 out, the padding channel zero
    ops.copy4d(y, full[B:], 4)
    rows = full[:, :3]
    word = ops.new_status_word(x.device)
    sums = torch.empty((len(FEATURE_DISTANCE_COLUMNS), B), dtype=torch.float64, device=x.device)
    if ops.RECORDER is not None:
        ops.RECORDER.keep += [buf, word, sums]
    with ops.status_scope(word), ops.defer_range_check():
        groups = [vgg.taps(rows[i:i + MAX_ROWS]) for i in range(0, 2 * B, MAX_ROWS)]
    taps = {n: _stack_rows([g[n] for g in groups]) for n in USED_TAPS}
    counts = []
    for i, n in enumerate(PERCEPTUAL_TAPS):
        t = taps[n]
        ops.abs_diff_rows(t[:B], t[B:], out=sums[i])
        counts.append(t[0].numel())
    for i, n in enumerate(STYLE_TAPS):
        g = ops.gram(taps[n])
        ops.abs_diff_rows(g[:B], g[B:], out=sums[len(PERCEPTUAL_TAPS) + i])
        counts.append(g[0].numel())
    return sums, counts, word


def feature_distances(vgg: VGG19, x: torch.Tensor, y: torch.Tensor, weights: Optional[Sequence[float]] = None) -> torch.Tensor:
    """float64 [B, 9] on the device, columns `FEATURE_DISTANCE_COLUMNS`: per row the five means |f(x) - f(y)| over the
    perceptual taps (multiplied by `weights[i]` when given, else unweighted), then the four means |G(x) - G(y)| over the Gram
    matrices of the style taps.  The mean of a column over the rows is the reference's batch-wide L1Loss of that tap.
    x, y: float [B, 3, H, W] as the reference feeds them (not normalised), or uint8 [B, H, W, 3] taken as / 255.

    One VGG pass over the 2B stacked rows (groups of at most `MAX_ROWS`), one `ops.gram` per style tap, nine
    `ops.abs_diff_rows`, the division on the device: no host synchronisation.  The range guard of the split-fp16 convolutions
    therefore cannot redo the pass; a pass that met an operand outside the split's range comes back as NaN in every entry
    (run it again under `ops.precision("f32")`)."""
    ops._require_gpu(x, "x")
    ops._require_gpu(y, "y")
    with torch.cuda.device(x.device):
        x, y = _as_input(x, "feature_distances"), _as_input(y.to(x.device), "feature_distances")
        if x.shape != y.shape:
            raise ValueError(f"feature_distances: shapes {tuple(x.shape)} and {tuple(y.shape)} differ")
        if weights is not None and len(weights) != len(PERCEPTUAL_TAPS):
            raise ValueError(f"feature_distances: {len(PERCEPTUAL_TAPS)} weights expected, got {len(weights)}")
        VGG19._check_input(x)
        if x.shape[0] == 0:
            return torch.zeros((0, len(FEATURE_DISTANCE_COLUMNS)), dtype=torch.float64, device=x.device)
        sums, counts, word = feature_sums(vgg, x, y)
        scale = [(1.0 if weights is None or i >= len(PERCEPTUAL_TAPS) else float(weights[i])) / float(n) for i, n in enumerate(counts)]
        out = (sums * ops.h2d(scale, x.device, torch.float64)[:, None]).t()
        return torch.where(word[0] != 0, torch.full_like(out, float("nan")), out)


class _FeatureLoss(nn.Module):
    def __init__(self):
        super().__init__()
        self.add_module("vgg", VGG19())

    def _mean(self, x, y, cols, weights=None) -> torch.Tensor:
        table = feature_distances(self.vgg, x, y, weights)
        return table[:, cols].sum(1).mean().to(torch.float32)


class PerceptualLoss(_FeatureLoss):
    """sum_i weights[i] * L1Loss(relu{i}_1(x), relu{i}_1(y)) as a 0-d float32 device tensor."""

    def __init__(self, weights=[1.0, 1.0, 1.0, 1.0, 1.0]):
        super().__init__()
        self.weights = weights

    def __call__(self, x, y):
        return self._mean(x, y, slice(0, len(PERCEPTUAL_TAPS)), self.weights)


class StyleLoss(_FeatureLoss):
    """sum over relu2_2, 3_4, 4_4, 5_2 of L1Loss(gram(x), gram(y)) as a 0-d float32 device tensor."""

    def compute_gram(self, x):
        return ops.gram(x)

    def __call__(self, x, y):
        return self._mean(x, y, slice(len(PERCEPTUAL_TAPS), len(FEATURE_DISTANCE_COLUMNS)))


class AdversarialLoss(nn.Module):
    """Training only: this library is forward-only evaluation.  The VALUES of the reference's objective are
    `AdversarialScore`."""

    def __init__(self, type="nsgan", target_real_label=1.0, target_fake_label=0.0):
        raise NotImplementedError("AdversarialLoss belongs to training (discriminators, backward passes), which this "
                                  "forward-only library does not provide; AdversarialScore computes the same values forward only")


class AdversarialScore(nn.Module):
    """The reference ``AdversarialLoss``'s values (loss.py:6-42), forward only: ``type`` 'nsgan' (BCELoss), 'lsgan' (MSELoss) or
    'hinge', called as ``score(outputs, is_real, is_disc=None)``; a 0-d float32 device tensor computed from the float64 columns of
    ``ops.gan_terms`` without a host synchronisation.  'nsgan' expects probabilities (a discriminator built with
    ``use_sigmoid=True``): for values outside [0, 1] nn.BCELoss raises, this returns NaN."""

    def __init__(self, type="nsgan", target_real_label=1.0, target_fake_label=0.0):
        super().__init__()
        if type not in ("nsgan", "lsgan", "hinge"):
            raise ValueError(f"AdversarialScore: type must be 'nsgan', 'lsgan' or 'hinge', got {type!r}")
        self.type = type
        self.register_buffer("real_label", torch.tensor(target_real_label))
        self.register_buffer("fake_label", torch.tensor(target_fake_label))
        self._labels = (float(torch.tensor(target_fake_label, dtype=torch.float32)), float(torch.tensor(target_real_label, dtype=torch.float32)))

    def value64(self, outputs: torch.Tensor, is_real, is_disc=None) -> torch.Tensor:
        """The value as a 0-d float64 device tensor (what `__call__` rounds to float32)."""
        t = ops.gan_terms(outputs.detach(), self._labels[1 if is_real else 0])
        n = t[:, 0].sum()
        if self.type == "hinge":
            if is_disc:
                return t[:, 4 if is_real else 3].sum() / n     # relu(1 - x) for real, relu(1 + x) for fake
            return -(t[:, 1].sum() / n)
        return t[:, 5 if self.type == "nsgan" else 2].sum() / n

    def __call__(self, outputs, is_real, is_disc=None):
        return self.value64(outputs, is_real, is_disc).to(torch.float32)


def feature_matching64(feats_a: Sequence[torch.Tensor], feats_b: Sequence[torch.Tensor]) -> torch.Tensor:
    """sum_i L1Loss(a_i, b_i) as a 0-d float64 device tensor: one `ops.abs_diff_rows` per pair, no host synchronisation."""
    if len(feats_a) != len(feats_b) or not len(feats_a):
        raise ValueError(f"feature_matching: {len(feats_a)} and {len(feats_b)} feature maps")
    total = None
    for a, b in zip(feats_a, feats_b):
        v = ops.abs_diff_rows(a.detach(), b.detach()).sum() / float(a.numel())
        total = v if total is None else total + v
    return total


def feature_matching(feats_a: Sequence[torch.Tensor], feats_b: Sequence[torch.Tensor]) -> torch.Tensor:
    """EdgeConnect's feature-matching term before its weight (models.py:115-117): sum_i L1Loss(a_i, b_i) over two lists of
    discriminator feature maps, a 0-d float32 device tensor."""
    return feature_matching64(feats_a, feats_b).to(torch.float32)
