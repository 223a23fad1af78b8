"""The conv layers of the batch-invariant routing tests (test_batch_invariant_cpu.py, test_gpu_batch_invariant.py): bare
shapes, their packed plans, and the descriptor ops.conv would hand to the library for a launch of n images."""
import ctypes as C

import torch

from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import ops, pack

# name -> layer.  The first two are the ones whose route changes most with the batch (routing batch).
LAYERS = {
    "c256_k3_16x16": dict(cin=256, cout=256, k=3, pad=1, hw=(16, 16)),               # hourglass / ICN bottleneck scale
    "c32_k3_64x128": dict(cin=32, cout=32, k=3, pad=1, hw=(64, 128)),                # VUnet shape encoder
    "c128_k1_32x32": dict(cin=128, cout=128, k=1, pad=0, hw=(32, 32)),               # hourglass 1x1
    "c64_c32_k3_128x128": dict(cin=64, cout=32, k=3, pad=1, hw=(128, 128)),
    "stem_k7_reflect_64x64": dict(cin=3, cout=64, k=7, pad=3, hw=(64, 64), pad_mode=L.PAD_REFLECT),
    "s2_k4_quadrant_64x64": dict(cin=64, cout=128, k=4, pad=1, hw=(64, 64), stride=2),
    "small_c256_k3_8x8": dict(cin=256, cout=256, k=3, pad=1, hw=(8, 8)),             # <= 64 pixels: the small-image kernel
    "small_c512_k3_4x4": dict(cin=512, cout=512, k=3, pad=1, hw=(4, 4)),             # several images per workgroup
}
PRECISIONS = ("f16x3", "f32", "bf16")
BATCHES = (1, 2, 8, 9, 32, 64)

_PLANS = {}


def weights(name):
    """Seeded weights and bias of the layer (fan-in scaled: outputs stay O(1))."""
    s = LAYERS[name]
    g = torch.Generator().manual_seed(1000 + sorted(LAYERS).index(name))
    w = torch.randn(s["cout"], s["cin"], s["k"], s["k"], generator=g) / (s["cin"] * s["k"] * s["k"]) ** 0.5
    return w, torch.randn(s["cout"], generator=g) * 0.1


def plan_of(name):
    if name not in _PLANS:
        s = LAYERS[name]
        w, b = weights(name)
        _PLANS[name] = pack.pack_conv(w, b, stride=s.get("stride", 1), pad=s["pad"], pad_mode=s.get("pad_mode", L.PAD_ZERO))
    return _PLANS[name]


def planned_desc(name, n, prec, device="cpu"):
    """(descriptor of the layer's ops.conv launch at n images after fusg_conv2d_plan, workspace bytes): no launch, so CPU
    tensors do.  (A plan lives on one device at a time: the GPU tests pass theirs.)"""
    s = LAYERS[name]
    with ops.status_scope(torch.zeros(4, dtype=torch.int32, device=device)):
        d, _ = ops._conv_desc(plan_of(name), ops.nhwc_empty(n, s["cin"], *s["hw"], device), precision=prec)
    return d, int(L.lib().fusg_conv2d_plan(C.byref(d)))


def route_order(name, n, prec, device="cpu"):
    """(family, tile, ksplit, ksw) of the launch (fusg_conv2d_route_order)."""
    d, _ = planned_desc(name, n, prec, device)
    out = (C.c_int32 * 4)()
    rc = L.lib().fusg_conv2d_route_order(C.byref(d), C.byref(out))
    assert rc == 0, (name, n, prec, rc, L.lib().fusg_last_error())
    return tuple(out)
