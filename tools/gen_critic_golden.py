#!/usr/bin/env python3
"""Generate tests/golden/critic_<case>.npz and tests/golden/critic_schema.json from the REFERENCE's edgeconnect.networks.
Discriminator, edgeconnect.loss.AdversarialLoss and warp_learn.models.D_NLayersMulti / GANLoss (CPU, build container only:
needs the reference checkout, FUSG_REFERENCE or /root/reference).

cv2 and torchvision are absent from the build container and only imported at module top by the reference files used here:
both are stubbed as tools/gen_golden.py stubs them.  The reference modules load the synthetic weights of
synth_state_dict('edge_dis' | 'inpaint_dis' | 'icn_dis', ...) and are put in eval mode - in train mode spectral norm runs a power
iteration on every forward and the logits are no function of the state dict.

Inputs are recreated from seeds (tests/critic_cases.py), not stored: a corner and the sum of each catch a drift.  The weights
are recreated too, but for spectral norm's u / v vectors (critic_sn_uv.npz): their float32 power iteration is not bit-stable
across thread counts.  Per case, for
input 'a', per returned map <m> (conv1 .. conv5; s<i>_stem, s<i>_norm1, s<i>_norm2, s<i>_logits):
  <m>_corner   float32 [:, :, :2, :2] of the reference's map          <m>_chsum   float64 [B, C] sums of the restatement's map
  <m>_E        the reference's own max |float32 - float64| / max |float64| on that map (E_ref)
the 1-channel logit maps whole, for 'a' and 'b', as <m>_{a,b}32 (reference) and <m>_{a,b}64 (restatement), and the scalars as
<name>_ref (reference, float32) and <name>_64 (restatement): adv_<type>_<is_real><is_disc> on 'a', fm (feature matching between
'a' and 'b'), gan_{real,fake}[_mask] on 'a'.  max |logit| <= 8 is asserted.

Usage:  python -B tools/gen_critic_golden.py
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

cv2 = types.ModuleType("cv2")
cv2.FILLED = -1
sys.modules["cv2"] = cv2
tv, tvt, tvm = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.models")
tvt.ToTensor = tvt.Normalize = object
tv.transforms, tv.models = tvt, tvm
sys.modules["torchvision"], sys.modules["torchvision.transforms"], sys.modules["torchvision.models"] = tv, tvt, tvm

import numpy as np                                # noqa: E402
import torch                                      # noqa: E402

warnings.filterwarnings("ignore")

from edgeconnect.networks import Discriminator                      # noqa: E402  (reference)
from edgeconnect.loss import AdversarialLoss                        # noqa: E402  (reference)
from warp_learn.models import D_NLayersMulti, GANLoss               # noqa: E402  (reference)

from future_urban_scene_generation_amd.synth import schema_of      # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")


def e_ref(f32, f64):
    return float((f32.double() - f64).abs().max() / f64.abs().max())


def put_map(arrs, name, f32, f64):
    arrs[f"{name}_corner"] = f32[:, :, :2, :2].clone()
    arrs[f"{name}_chsum"] = f64.sum((2, 3))
    arrs[f"{name}_E"] = np.array(e_ref(f32, f64))


def main():
    torch.set_grad_enabled(False)
    mods = {"Discriminator2": Discriminator(2), "Discriminator3": Discriminator(3),
            "Discriminator3_plain": Discriminator(3, use_spectral_norm=False), "D_NLayersMulti3": D_NLayersMulti(3)}
    with open(os.path.join(GOLD, "critic_schema.json"), "w") as f:
        json.dump({n: [[k, list(v.shape)] for k, v in m.state_dict().items()] for n, m in mods.items()}, f, indent=0)
    import critic_cases as cc                     # (reads the schema just written)
    import critic_ref as cr
    uv = {}                                       # spectral norm's vectors as generated on this machine (critic_cases.state_dict)
    for case in ("dis2_b2_32x32", "dis3_b2_32x32"):
        for k, v in cc.state_dict(case, stored_uv=False).items():
            if k.endswith(("weight_u", "weight_v")) and not k.startswith("features."):
                uv[f"{cc.net_name(case)}/{k}"] = v.numpy()
    np.savez(cc.SN_VECTORS, **uv)
    for case, (net, c, b, h, w) in cc.CASES.items():
        sd = cc.state_dict(case)
        xa, xb = cc.inputs(case)
        mask = cc.mask(case)
        arrs = dict(weight_seed=np.array(cc.WEIGHT_SEED), a_corner=xa[:, :, :4, :4], b_corner=xb[:, :, :4, :4],
                    a_sum=xa.double().sum(), b_sum=xb.double().sum(), mask_sum=mask.double().sum())
        if net == "dis":
            ref = Discriminator(c, use_sigmoid=True)
            ref.load_state_dict(sd)
            ref.eval()
            (oa, fa), (ob, fb) = ref(xa), ref(xb)
            (oa64, fa64), (ob64, fb64) = cr.discriminator(sd, xa), cr.discriminator(sd, xb)
            for name, m32, m64 in zip(cc.DIS_MAPS, fa, fa64):
                put_map(arrs, name, m32, m64)
            logits = [(fa[4], fa64[4]), (fb[4], fb64[4])]
            for tag, (l32, l64) in zip("ab", logits):
                arrs[f"conv5_{tag}32"], arrs[f"conv5_{tag}64"] = l32.clone(), l64
            for kind in cc.ADV_TYPES:
                adv = AdversarialLoss(type=kind)
                o32, o64 = (fa[4], fa64[4]) if kind == "hinge" else (oa, oa64)
                for is_real, is_disc in cc.ADV_CALLS:
                    key = f"adv_{kind}_{int(is_real)}{int(is_disc)}"
                    arrs[key + "_ref"] = adv(o32, is_real, is_disc)
                    arrs[key + "_64"] = cr.adversarial(kind, o64, is_real, is_disc)
            arrs["fm_ref"] = sum(torch.nn.L1Loss()(x, y) for x, y in zip(fb, fa))
            arrs["fm_64"] = cr.feature_matching(fb64, fa64)
            worst = max(float(l.abs().max()) for l, _ in logits)
        else:
            ref = D_NLayersMulti(c)
            ref.load_state_dict(sd)
            ref.eval()
            pa, pb = ref(xa), ref(xb)
            ma64, mb64 = cr.nlayers_multi(sd, xa), cr.nlayers_multi(sd, xb)
            down = xa
            for s in range(ref.num_D):                  # the reference's intermediate maps: its Sequential, slot by slot
                y, maps = down, []
                for slot, layer in enumerate(getattr(ref, "model_%d" % s)):
                    y = layer(y)
                    if isinstance(layer, torch.nn.LeakyReLU) or slot == 8:
                        maps.append(y.clone())
                assert torch.equal(maps[-1], pa[s])
                for name, m32, m64 in zip(cc.ICN_MAPS, maps, ma64[s]):
                    put_map(arrs, f"s{s}_{name}", m32, m64)
                down = ref.down(down)
            for tag, p32, m64 in (("a", pa, ma64), ("b", pb, mb64)):
                for s in range(ref.num_D):
                    arrs[f"s{s}_logits_{tag}32"], arrs[f"s{s}_logits_{tag}64"] = p32[s].clone(), m64[s][-1]
            gl = GANLoss()
            for nm, real in (("real", True), ("fake", False)):
                for mtag, mk in (("", None), ("_mask", mask)):
                    arrs[f"gan_{nm}{mtag}_ref"] = gl(pa, real, mask=mk)
                    arrs[f"gan_{nm}{mtag}_64"] = cr.gan_loss([m[-1] for m in ma64], 1.0 if real else 0.0, mk)
            worst = max(float(p.abs().max()) for p in pa + pb)
        assert worst <= cc.MAX_LOGIT, (case, worst)
        path = os.path.join(GOLD, f"critic_{case}.npz")
        np.savez(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
        es = {k[:-2]: float(v) for k, v in arrs.items() if k.endswith("_E")}
        print(f"{case}: max |logit| {worst:.3f}  E_ref {max(es.values()):.2e}  wrote {os.path.getsize(path) / 1e3:.1f} kB")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
