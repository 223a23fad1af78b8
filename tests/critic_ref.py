"""float64 restatement (torch on the CPU) of EdgeConnect's Discriminator / AdversarialLoss and Warp&Learn's D_NLayersMulti /
GANLoss, from a float32 state dict: the yardstick of the discriminator tests.  tests/test_critic_cpu.py proves it against the
reference's float32 results stored in tests/golden/critic_<case>.npz.
"""
import torch
import torch.nn.functional as F


def _w(sd, prefix):
    """(weight, bias) in float64; a spectral-normed conv folds as eval mode does: weight_orig / (u . (W v))."""
    if prefix + ".weight_orig" in sd:
        w = sd[prefix + ".weight_orig"].double()
        u, v = sd[prefix + ".weight_u"].double(), sd[prefix + ".weight_v"].double()
        w = w / torch.dot(u, torch.mv(w.reshape(w.shape[0], -1), v))
    else:
        w = sd[prefix + ".weight"].double()
    b = sd.get(prefix + ".bias")
    return w, (b.double() if b is not None else None)


def discriminator(sd, x, use_sigmoid=True):
    """(outputs, [conv1 ... conv5]) in float64: conv1 - conv4 after LeakyReLU(0.2), conv5 raw."""
    y, feats = x.double(), []
    for i, stride in enumerate((2, 2, 2, 1, 1), 1):
        w, b = _w(sd, f"conv{i}.0")
        y = F.conv2d(y, w, b, stride=stride, padding=1)
        if i < 5:
            y = F.leaky_relu(y, 0.2)
        feats.append(y)
    return (torch.sigmoid(y) if use_sigmoid else y), feats


def nlayers_multi(sd, x, n_layers=2, num_D=2):
    """Per scale [stem, normed layers ..., logits] in float64."""
    down, out = x.double(), []
    idx = [0] + [2 + 3 * i for i in range(n_layers)] + [2 + 3 * n_layers]
    for s in range(num_D):
        y, maps = down, []
        for j, k in enumerate(idx):
            w, b = _w(sd, f"model_{s}.{k}")
            y = F.conv2d(y, w, b, stride=2 if j < n_layers else 1, padding=1)
            if 0 < j < len(idx) - 1:
                y = F.instance_norm(y, eps=1e-5)
            if j < len(idx) - 1:
                y = F.leaky_relu(y, 0.2)
            maps.append(y)
        out.append(maps)
        if s != num_D - 1:
            down = F.avg_pool2d(down, 3, stride=2, padding=1, count_include_pad=False)
    return out


def adversarial(kind, outputs, is_real, is_disc, real_label=1.0, fake_label=0.0):
    o = outputs.double()
    if kind == "hinge":
        if is_disc:
            return F.relu(1 + (-o if is_real else o)).mean()
        return (-o).mean()
    t = torch.full_like(o, real_label if is_real else fake_label)
    if kind == "nsgan":
        return -(t * torch.log(o).clamp(min=-100) + (1 - t) * torch.log(1 - o).clamp(min=-100)).mean()
    return ((o - t) ** 2).mean()


def gan_loss(predictions, label, mask=None):
    """sum over the scales of mean((p m - label m)^2); the mask is sampled in float32 as the reference samples it."""
    total = 0.0
    for p in predictions:
        p = p.double()
        t = torch.full_like(p, float(label))
        if mask is not None:
            m = F.interpolate(mask.float(), size=p.shape[2:]).double()
            p, t = p * m, t * m
        total = total + ((p - t) ** 2).mean()
    return total


def feature_matching(feats_a, feats_b):
    return sum((a.double() - b.double()).abs().mean() for a, b in zip(feats_a, feats_b))
