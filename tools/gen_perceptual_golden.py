#!/usr/bin/env python3
"""Generate tests/golden/perceptual_<case>.npz and tests/golden/perceptual_schema.json from the REFERENCE's edgeconnect.loss
(CPU, build container only: needs the reference checkout, FUSG_REFERENCE or /root/reference).

torchvision is absent from the build container, and the reference's VGG19 only takes `models.vgg19(pretrained=True).features`
from it: `torchvision.models.vgg19` is stubbed with a plain nn.Sequential of configuration E (conv 3 x 3, ReLU(inplace),
MaxPool2d(2, 2) at torchvision's indices) holding the synthetic `features.*` weights of synth_state_dict("vgg", ...).  Then
the reference's own PerceptualLoss(), StyleLoss() and VGG19() run on the seeded image pairs of tests/perceptual_cases.py.

Inputs are recreated from seeds, not stored (a corner and the sum of each catch a drift); outputs are results only.  Per case
and pair kind ('noise', 'lsb'):
  <kind>_perceptual_ref, <kind>_style_ref   the reference's two float32 scalars
  <kind>_table64                            the float64 [B, 9] per-row table of the restatement tests/perceptual_ref.py
  <kind>_E_perceptual, <kind>_E_style       |reference scalar - column-mean sum of the table| / the latter: the reference's
                                            own float32 error against float64, the yardstick of the device tests
and for the two small cases, of the reference VGG19()'s nine used taps on the 'noise' x: tap_<name>_corner (float32
[B, C, 2, 2], the top-left activations) and tap_<name>_chsum (float64 [B, C], every activation summed per channel) - the
whole tensors would put a file past the 1 MiB this repository allows (relu1_1 of one 64 x 64 row alone is 1 MiB).

Usage:  python -B tools/gen_perceptual_golden.py
"""
import json
import os
import sys
import types
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FUSG_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np                                # noqa: E402
import torch                                      # noqa: E402
import torch.nn as nn                             # noqa: E402

warnings.filterwarnings("ignore")

import perceptual_cases as pc                     # noqa: E402
import perceptual_ref as pr                       # noqa: E402

from future_urban_scene_generation_amd.cad_classifier import vgg19_schema  # noqa: E402
from future_urban_scene_generation_amd.synth import synth_state_dict  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
USED = tuple(n for n, _, _ in pr.tap_layers() if n in pr.PERCEPTUAL_TAPS + pr.STYLE_TAPS)


def features_sd():
    schema = {k: v for k, v in vgg19_schema(10).items() if k.startswith("features.")}
    return synth_state_dict("vgg", schema, pc.WEIGHT_SEED)


def stub_torchvision(sd):
    """`import torchvision.models as models; models.vgg19(pretrained=True).features` -> configuration E with `sd` loaded."""
    def vgg19(pretrained=False, **kw):
        layers, cin = [], 3
        for v in pr.CFG_E:
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        net = nn.Module()
        net.features = nn.Sequential(*layers)
        net.load_state_dict(sd)
        return net

    tv, models = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
    models.vgg19, tv.models = vgg19, models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models


def main():
    torch.set_grad_enabled(False)
    sd = features_sd()
    stub_torchvision(sd)
    from edgeconnect import loss as ref_loss      # (reference)
    assert ref_loss.__file__.startswith(REF), ref_loss.__file__
    perceptual, style, vgg = ref_loss.PerceptualLoss(), ref_loss.StyleLoss(), ref_loss.VGG19()
    schema = {name: [[k, list(v.shape)] for k, v in mod.state_dict().items()]
              for name, mod in (("VGG19", vgg), ("PerceptualLoss", perceptual), ("StyleLoss", style))}
    with open(os.path.join(GOLD, "perceptual_schema.json"), "w") as f:
        json.dump(schema, f, indent=0)
    for case in pc.FIXTURES:
        arrs = dict(weight_seed=np.array(pc.WEIGHT_SEED), columns=np.array(json.dumps(list(pr.COLUMNS))))
        for kind in pc.PAIRS:
            x, y = pc.image_pair(case, kind)
            p_ref, s_ref = perceptual(x, y), style(x, y)
            t64 = pr.table(sd, x, y)
            p64, s64 = float(t64[:, :5].sum(1).mean()), float(t64[:, 5:].sum(1).mean())
            e_p, e_s = abs(float(p_ref.double()) - p64) / p64, abs(float(s_ref.double()) - s64) / s64
            arrs.update({f"{kind}_perceptual_ref": p_ref, f"{kind}_style_ref": s_ref, f"{kind}_table64": t64,
                         f"{kind}_E_perceptual": np.array(e_p), f"{kind}_E_style": np.array(e_s),
                         f"{kind}_x_corner": x[:, :, :4, :4], f"{kind}_y_corner": y[:, :, :4, :4],
                         f"{kind}_x_sum": x.double().sum(), f"{kind}_y_sum": y.double().sum()})
            print(f"{case} {kind}: perceptual {float(p_ref):.6f} (E_ref {e_p:.2e})  style {float(s_ref):.3e} (E_ref {e_s:.2e})")
            if case in pc.SMALL_FIXTURES and kind == "noise":
                taps = vgg(x)
                for n in USED:
                    t = taps[n]
                    arrs[f"tap_{n}_corner"] = t[:, :, :2, :2].clone()
                    arrs[f"tap_{n}_chsum"] = t.double().sum((2, 3))
                    print(f"   {n}: {tuple(t.shape)} positive {float((t > 0).float().mean()):.2f} max {float(t.max()):.2f}")
        path = os.path.join(GOLD, f"perceptual_{case}.npz")
        np.savez(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
        print(f"wrote perceptual_{case}.npz  {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
