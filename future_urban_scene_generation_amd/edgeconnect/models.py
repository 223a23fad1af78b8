"""Drop-in for the inference half of the reference's ``edgeconnect.models`` on MI355X.

``EdgeModel(config)`` / ``InpaintingModel(config)`` keep the reference's construction, ``load()``
(checkpoint dict ``{'iteration', 'generator'}`` at ``<PATH>/<name>_gen.pth``, models.py:17-30) and
``forward(images, edges, masks)`` (models.py:130-135, 236-240).  The training half (optimisers,
``process``/``backward``) is out of scope - which also
removes the reference's import-time dependency on torchvision's pretrained VGG19.
The mask compositing + channel concat in front of the generator is one libfusg kernel.

``EdgeModel(config, discriminator=True)`` / ``InpaintingModel(config, discriminator=True)`` add the reference's
``discriminator`` (``<PATH>/<name>_dis.pth = {'discriminator': state_dict}`` in ``load`` / ``save``) and ``evaluate(images,
edges, masks)``: the forward pass plus the terms the reference's ``process`` logs (models.py:99-126, 196-232) as one float64
device vector - forward only, no ``.item()``, no host synchronisation.  The default builds the generator-only module.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .. import ops
from .networks import Discriminator, EdgeGenerator, InpaintGenerator

# the reference's DEFAULT_CONFIG (edgeconnect/config.py:31-60), the entries `evaluate` reads
EVAL_DEFAULTS = {"GAN_LOSS": "nsgan", "L1_LOSS_WEIGHT": 1, "FM_LOSS_WEIGHT": 10, "STYLE_LOSS_WEIGHT": 1, "CONTENT_LOSS_WEIGHT": 1,
                 "INPAINT_ADV_LOSS_WEIGHT": 0.01}


class BaseModel(nn.Module):
    def __init__(self, name, config):
        super().__init__()
        self.name = name
        self.config = config
        self.iteration = 0
        path = getattr(config, "PATH", ".") if config is not None else "."
        self.gen_weights_path = os.path.join(path, name + "_gen.pth")
        self.dis_weights_path = os.path.join(path, name + "_dis.pth")

    def _cfg(self, name):
        """config.<name>, else the reference's default."""
        v = getattr(self.config, name, None) if self.config is not None else None
        return EVAL_DEFAULTS[name] if v is None else v

    def _add_discriminator(self, in_channels: int) -> None:
        from .loss import AdversarialScore
        gan = self._cfg("GAN_LOSS")
        self.add_module("discriminator", Discriminator(in_channels=in_channels, use_sigmoid=gan != "hinge"))
        self.add_module("adversarial_loss", AdversarialScore(type=gan))

    def load(self):
        """Reads `<PATH>/<name>_gen.pth` = {'iteration': int, 'generator': state_dict} when it exists (the
        reference's checkpoint contract, edgeconnect/models.py:25-30); a missing file leaves the initial weights.  With a
        discriminator also `<PATH>/<name>_dis.pth` = {'discriminator': state_dict} (models.py:32-35)."""
        if os.path.exists(self.gen_weights_path):
            ckpt = torch.load(self.gen_weights_path, map_location="cpu", weights_only=True)
            self.generator.load_state_dict(ckpt["generator"])
            self.iteration = ckpt["iteration"]
        if hasattr(self, "discriminator") and os.path.exists(self.dis_weights_path):
            ckpt = torch.load(self.dis_weights_path, map_location="cpu", weights_only=True)
            self.discriminator.load_state_dict(ckpt["discriminator"])

    def save(self):
        """Writes the same files `load` reads (edgeconnect/models.py:38-52)."""
        torch.save({"iteration": self.iteration, "generator": self.generator.state_dict()}, self.gen_weights_path)
        if hasattr(self, "discriminator"):
            torch.save({"discriminator": self.discriminator.state_dict()}, self.dis_weights_path)

    def _need_discriminator(self):
        if not hasattr(self, "discriminator"):
            raise RuntimeError(f"{self.name}.evaluate needs the discriminator: construct {self.name}(config, discriminator=True)")

    @staticmethod
    def _logs(values, word: torch.Tensor) -> torch.Tensor:
        """The float64 device vector of the logged terms; NaN throughout when a split-fp16 launch met an operand outside its
        range (evaluate cannot redo the pass without reading the word back: run it under ops.precision("f32"))."""
        out = torch.stack([v.to(torch.float64) for v in values])
        return torch.where(word[0] != 0, torch.full_like(out, float("nan")), out)

    def process(self, *a, **k):
        raise NotImplementedError("training is out of scope of the MI355X inference path")

    backward = process


def _channel_cat(parts, device) -> torch.Tensor:
    """torch.cat(parts, dim=1) of [B, c_i, H, W] float32 tensors as channel slices of ONE zero-filled NHWC buffer of pitch 4
    (each slice written by ops.copy4d): the discriminator's input, its padding channels zero."""
    b, _, h, w = parts[0].shape
    c = sum(p.shape[1] for p in parts)
    full = ops.nhwc_empty(b, (c + 3) // 4 * 4, h, w, device, zero=True)
    o = 0
    for p in parts:
        ops.copy4d(p.detach().to(torch.float32), full[:, o:o + p.shape[1]], 0)
        o += p.shape[1]
    x = full[:, :c]
    x._fusg_zero_pad = True
    if ops.RECORDER is not None:
        ops.RECORDER.keep.append(full)
    return x


class EdgeModel(BaseModel):
    LOG_NAMES = ("l_d1", "l_g1", "l_fm")

    def __init__(self, config, discriminator: bool = False):
        super().__init__("EdgeModel", config)
        self.add_module("generator", EdgeGenerator(use_spectral_norm=True))
        if discriminator:
            self._add_discriminator(2)

    def forward(self, images, edges, masks):
        return self.generator.run_model(images, edges, masks, 0)   # cat(img*(1-m)+m, edge*(1-m), m) -> generator

    def evaluate(self, images, edges, masks):
        """(outputs, (names, values)): the forward pass and the terms `process` logs (reference models.py:99-126) - l_d1 the
        discriminator objective, l_g1 the generator's adversarial term, l_fm the weighted feature-matching sum - as a float64
        device vector in the order of `names`.  Each term is the reference's float32 formula on `AdversarialScore` /
        `feature_matching` values.  No host synchronisation."""
        from .loss import feature_matching
        self._need_discriminator()
        adv = self.adversarial_loss
        with torch.cuda.device(images.device):
            word = ops.new_status_word(images.device)
            with ops.status_scope(word), ops.defer_range_check():
                outputs = self(images, edges, masks)
                dis_real, real_feat = self.discriminator(_channel_cat((images, edges), images.device))
                dis_fake, fake_feat = self.discriminator(_channel_cat((images, outputs), images.device))
            l_d1 = (adv(dis_real, True, True) + adv(dis_fake, False, True)) / 2
            l_g1 = adv(dis_fake, True, False)
            l_fm = feature_matching(fake_feat, real_feat) * self._cfg("FM_LOSS_WEIGHT")
            return outputs, (self.LOG_NAMES, self._logs((l_d1, l_g1, l_fm), word))


class InpaintingModel(BaseModel):
    LOG_NAMES = ("l_d2", "l_g2", "l_l1", "l_per", "l_sty")

    def __init__(self, config, discriminator: bool = False):
        super().__init__("InpaintingModel", config)
        self.add_module("generator", InpaintGenerator())
        if discriminator:
            self._add_discriminator(3)

    def forward(self, images, edges, masks):
        return self.generator.run_model(images, edges, masks, 1)   # cat(img*(1-m)+m, edge) -> generator

    def evaluate(self, images, edges, masks, vgg=None):
        """(outputs, (names, values)): the forward pass and the terms `process` logs (reference models.py:196-232) - l_d2, l_g2
        (weighted), l_l1 (weighted, over the mean of the masks), l_per, l_sty - as a float64 device vector in the order of
        `names`.  vgg: a loaded `edgeconnect.loss.VGG19`; without one l_per and l_sty are NaN.  No host synchronisation."""
        from .loss import FEATURE_DISTANCE_COLUMNS, PERCEPTUAL_TAPS, feature_distances
        self._need_discriminator()
        adv = self.adversarial_loss
        with torch.cuda.device(images.device):
            word = ops.new_status_word(images.device)
            with ops.status_scope(word), ops.defer_range_check():
                outputs = self(images, edges, masks)
                dis_real, _ = self.discriminator(_channel_cat((images,), images.device))
                dis_fake, _ = self.discriminator(_channel_cat((outputs,), images.device))
            l_d2 = (adv(dis_real, True, True) + adv(dis_fake, False, True)) / 2
            l_g2 = adv(dis_fake, True, False) * self._cfg("INPAINT_ADV_LOSS_WEIGHT")
            images32, masks32 = images.detach().to(torch.float32), masks.detach().to(torch.float32)
            l1 = (ops.abs_diff_rows(outputs, images32).sum() / float(outputs.numel())).to(torch.float32)
            mt = ops.gan_terms(masks32)
            l_l1 = l1 * self._cfg("L1_LOSS_WEIGHT") / (mt[:, 1].sum() / mt[:, 0].sum()).to(torch.float32)
            nan = torch.full((), float("nan"), dtype=torch.float32, device=images.device)
            l_per = l_sty = nan
            if vgg is not None:
                np_ = len(PERCEPTUAL_TAPS)
                per = feature_distances(vgg, outputs, images32, [1.0] * np_)
                sty = feature_distances(vgg, ops.mask_mul(outputs, masks32), ops.mask_mul(images32, masks32))
                l_per = per[:, :np_].sum(1).mean().to(torch.float32) * self._cfg("CONTENT_LOSS_WEIGHT")
                l_sty = sty[:, np_:len(FEATURE_DISTANCE_COLUMNS)].sum(1).mean().to(torch.float32) * self._cfg("STYLE_LOSS_WEIGHT")
            return outputs, (self.LOG_NAMES, self._logs((l_d2, l_g2, l_l1, l_per, l_sty), word))
