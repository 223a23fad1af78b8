#!/usr/bin/env python3
"""Generate tests/golden/vunet_up_{nearest,conv2d_t}_b2_r128.npz from the REFERENCE's Vunet_fix_res (CPU, build
container only: needs the reference checkout, FUSG_REFERENCE or /root/reference).

The two UpSample modes the shipped configuration does not use:
  nearest   Namespace(w_norm=False, drop_prob=0.0, up_mode='nearest', vunet_256=False)   (the reference's own self-check)
  conv2d_t  Namespace(w_norm=True,  drop_prob=0.0, up_mode='conv2d_t', vunet_256=False)
Like tests/golden/manifest.json's cases, weights and inputs are recreated from seeds (synth_state_dict over the state_dict
schema stored in the fixture, synth_inputs), not stored: each file holds the ordered state_dict keys with shapes, the
seeds, a corner and the sum of each input (so a test can tell that it recreated the same tensors) and the outputs of
`forward(y_tilde, x)` under torch.manual_seed(fwd_seed) - the Sampler noise comes from the CPU default generator.
The inputs are not stored because the manifest's convention is to recreate them from the seed (synth_inputs is bit-stable:
the existing VUnet goldens rely on it); the corner and sum catch a drift.  Storing them as well (1.2 MB, 1.08 MB
compressed) would also put each file past the 1 MiB this repository allows a newly committed file.

Usage:  python -B tools/gen_vunet_upmodes_golden.py
"""
import json
import os
import sys
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FUSG_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, REPO)

import numpy as np                                # noqa: E402
import torch                                      # noqa: E402

warnings.filterwarnings("ignore")
from argparse import Namespace                    # noqa: E402

from vunet.models import Vunet_fix_res            # noqa: E402  (reference)

from future_urban_scene_generation_amd.synth import schema_of, synth_inputs, synth_state_dict  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
SEED, FWD_SEED, B, R = 0, 999, 2, 128
CASES = {"vunet_up_nearest_b2_r128": dict(up_mode="nearest", w_norm=False, drop_prob=0.0, vunet_256=False),
         "vunet_up_conv2d_t_b2_r128": dict(up_mode="conv2d_t", w_norm=True, drop_prob=0.0, vunet_256=False)}


def main():
    torch.set_grad_enabled(False)
    for tag, cfg in CASES.items():
        net = Vunet_fix_res(Namespace(**cfg))
        schema = schema_of(net.state_dict())
        net.load_state_dict(synth_state_dict("vunet", schema, SEED))
        net.eval()
        i = synth_inputs("vunet", B, R, SEED)
        assert tuple(i["y_tilde"].shape) == (B, 3, R, R) and tuple(i["x"].shape) == (B, 6, R, R)
        torch.manual_seed(FWD_SEED)
        x_tilde, mu_app, mu_shape = net(i["y_tilde"], i["x"])
        arrs = dict(config=np.array(json.dumps(cfg)), schema=np.array(json.dumps([[k, list(s)] for k, (s, _) in schema.items()])),
                    seed=np.array(SEED), fwd_seed=np.array(FWD_SEED),
                    y_tilde_corner=i["y_tilde"][:, :, :8, :8], x_corner=i["x"][:, :, :8, :8],
                    y_tilde_sum=i["y_tilde"].double().sum(), x_sum=i["x"].double().sum(),
                    x_tilde=x_tilde, mu_app0=mu_app[0], mu_app1=mu_app[1], mu_shape0=mu_shape[0], mu_shape1=mu_shape[1])
        path = os.path.join(GOLD, tag + ".npz")
        np.savez(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
        print(f"wrote {tag}.npz  {os.path.getsize(path) / 1e6:.2f} MB  x_tilde {tuple(x_tilde.shape)} "
              f"|x_tilde| max {float(x_tilde.abs().max()):.3f}  finite {bool(torch.isfinite(x_tilde).all())}")


if __name__ == "__main__":
    main()
