"""A float64 restatement of EdgeConnect's PerceptualLoss / StyleLoss in plain torch.nn.functional on the CPU: VGG-19
configuration E's ReLU taps from a torchvision-style `features.N.*` state dict, the Gram matrix f f^T / (h w ch), and the
per-row table whose column means are the losses' terms.  What the fixtures (tools/gen_perceptual_golden.py) and the GPU tests
measure the device against."""
import torch
import torch.nn.functional as F

CFG_E = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M")
PERCEPTUAL_TAPS = ("relu1_1", "relu2_1", "relu3_1", "relu4_1", "relu5_1")
STYLE_TAPS = ("relu2_2", "relu3_4", "relu4_4", "relu5_2")
COLUMNS = tuple(f"perceptual_{n}" for n in PERCEPTUAL_TAPS) + tuple(f"style_{n}" for n in STYLE_TAPS)


def tap_layers():
    """[(tap name, features index of its conv, pooled before it)] in network order."""
    out, idx, block, k, pooled = [], 0, 1, 1, False
    for v in CFG_E:
        if v == "M":
            idx, block, k, pooled = idx + 1, block + 1, 1, True
            continue
        out.append((f"relu{block}_{k}", idx, pooled))
        idx, k, pooled = idx + 2, k + 1, False
    return out


def taps(sd, x, last="relu5_2", dtype=torch.float64):
    """{tap name: [B, C, h, w] in `dtype`} up to `last` for x [B, 3, H, W]."""
    t, out = x.to(dtype), {}
    for name, idx, pooled in tap_layers():
        if pooled:
            t = F.max_pool2d(t, 2, 2)
        t = F.relu(F.conv2d(t, sd[f"features.{idx}.weight"].to(dtype), sd[f"features.{idx}.bias"].to(dtype), padding=1))
        out[name] = t
        if name == last:
            break
    return out


def gram(f):
    b, ch, h, w = f.shape
    f = f.reshape(b, ch, h * w)
    return f.bmm(f.transpose(1, 2)) / (h * w * ch)


def table(sd, x, y):
    """float64 [B, 9] (COLUMNS): per row the mean |f(x) - f(y)| of the five perceptual taps, then the mean |G(x) - G(y)| of
    the four style taps' Gram matrices."""
    fx, fy = taps(sd, x), taps(sd, y)
    cols = [(fx[n] - fy[n]).abs().flatten(1).mean(1) for n in PERCEPTUAL_TAPS]
    cols += [(gram(fx[n]) - gram(fy[n])).abs().flatten(1).mean(1) for n in STYLE_TAPS]
    return torch.stack(cols, 1)
