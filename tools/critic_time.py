#!/usr/bin/env python3
"""What the discriminators and the GAN terms cost on the device (GPU box) -> profiles/critic_time.json.  Recorded only: no
bar is attached to these times, the nets are on no product pass.

Timing: medians of 9 after a warm-up, HIP events around `--inner` back-to-back calls, per call, synthetic weights:
  discriminator   edgeconnect.networks.Discriminator(3).forward on `--batch` 256 x 256 images (and on one), with conv2 / conv3
                  on the halo kernel's stride-2 form (K kept whole) and, for comparison, with the planner's K split
  nlayers_multi   warp_learn.models.D_NLayersMulti(3).forward on the same images
  adversarial     AdversarialScore('nsgan') on the discriminator's output (one ops.gan_terms)
  gan_loss        GANLoss on the two logit maps, with a mask
  feature_matching  over the five feature maps of two passes
  gan_terms_1m    ops.gan_terms alone on [batch, 16, 256, 256] (16 Mi elements at batch 16) with its rate in GB/s
  evaluate_edge / evaluate_inpaint   EdgeModel / InpaintingModel(None, discriminator=True).evaluate at `--batch` images
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch  # noqa: E402

import critic_cases as cc  # noqa: E402

from future_urban_scene_generation_amd import ops  # noqa: E402
from future_urban_scene_generation_amd.edgeconnect import loss  # noqa: E402
from future_urban_scene_generation_amd.edgeconnect.models import EdgeModel, InpaintingModel  # noqa: E402
from future_urban_scene_generation_amd.edgeconnect.networks import Discriminator  # noqa: E402
from future_urban_scene_generation_amd.synth import synth_inputs, synth_state_dict  # noqa: E402
from future_urban_scene_generation_amd.warp_learn.models import D_NLayersMulti, GANLoss  # noqa: E402


def timed(fn, reps, inner):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return {"ms": statistics.median(out), "min_max": [min(out), max(out)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("-o", "--out", default=os.path.join(REPO, "profiles", "critic_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("critic_time: needs a HIP device (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    B, R = args.batch, args.res
    dis = Discriminator(3)
    dis.load_state_dict(synth_state_dict("inpaint_dis", cc.schema("Discriminator3")))
    dis = dis.to(dev).eval()
    icn = D_NLayersMulti(3)
    icn.load_state_dict(synth_state_dict("icn_dis", cc.schema("D_NLayersMulti3")))
    icn = icn.to(dev).eval()
    i = {k: v.to(dev) for k, v in synth_inputs("edge", B, R).items()}
    x, x1 = i["img"], i["img"][:1].contiguous()
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "res": R, "reps": args.reps, "inner": args.inner, "precision": ops.PRECISION}
    T = lambda fn: timed(fn, args.reps, args.inner)               # noqa: E731
    with torch.no_grad(), ops.defer_range_check():
        for _ in range(2):
            out, feats = dis(x)
            preds = icn(x)
        res["discriminator"] = T(lambda: dis(x))
        res["discriminator_b1"] = T(lambda: dis(x1))
        whole = Discriminator.__dict__["_whole_k"]
        try:
            Discriminator._whole_k = staticmethod(lambda t: 0)
            dis(x1)
            res["discriminator_planner_ksplit"] = T(lambda: dis(x))
            res["discriminator_b1_planner_ksplit"] = T(lambda: dis(x1))
        finally:
            Discriminator._whole_k = whole
        res["nlayers_multi"] = T(lambda: icn(x))
        score, gl = loss.AdversarialScore("nsgan"), GANLoss()
        res["adversarial"] = T(lambda: score(out, True, True))
        res["gan_loss"] = T(lambda: gl(preds, True, mask=i["mask"]))
        _, feats2 = dis(x.flip(0))
        res["feature_matching"] = T(lambda: loss.feature_matching(feats, feats2))
        big = torch.rand((B, 16, R, R), device=dev)
        r = T(lambda: ops.gan_terms(big))
        r["gbytes_per_s"] = big.numel() * 4 / r["ms"] / 1e6
        res["gan_terms_1m"] = r
        em, im = EdgeModel(None, discriminator=True).to(dev).eval(), InpaintingModel(None, discriminator=True).to(dev).eval()
        vgg = loss.VGG19().to(dev)
        em.evaluate(i["gray"], i["edge"], i["mask"])
        im.evaluate(i["img"], i["edge"], i["mask"], vgg=vgg)
        res["evaluate_edge"] = T(lambda: em.evaluate(i["gray"], i["edge"], i["mask"]))
        res["evaluate_inpaint"] = T(lambda: im.evaluate(i["img"], i["edge"], i["mask"], vgg=vgg))
    print(json.dumps(res, indent=1, sort_keys=True))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
