"""Drop-in for the network half of the reference's ``warp_learn.models`` on MI355X.

Public surface kept (warp_learn/models.py:190-208): ``G_Resnet(input_nc, output_nc=3, num_downs=2,
n_res=3, ngf=64, norm='inst', nl_layer='relu')`` with ``forward(image)`` and ``decode(content)``,
and the reference's ``state_dict`` schema (``enc_content.model.{i}.conv.*``,
``...model.{j}.model.{0,1}.conv.*``, ``dec.model.{k}.norm.{gamma,beta}``).

Execution (NHWC, libfusg): every convolution reads its input through the fused reflect-pad
address mapping; ``InstanceNorm -> ReLU -> conv`` chains never materialise the normalised tensor
(a streaming statistics pass produces per-(b,c) scale/shift which the consumer conv applies while
staging its tile); the decoder's ``nearest-upsample -> 5x5 conv`` reads the low-resolution tensor
directly (upsample folded into the gather), its custom LayerNorm (unbiased std, eps on std)
becomes the next conv's per-(b,c) affine prologue, and ``x + IN(conv(.))`` is one elementwise pass.

``D_NLayersMulti(input_nc, ndf=64, n_layers=2, num_D=2)`` and ``GANLoss(target_real_label=1.0, target_fake_label=0.0)``
(warp_learn/models.py:211-320) are provided forward only: the multi-scale PatchGAN critic with the reference's schema
(``model_{i}.{0,2,5,8}.{weight,bias}`` at the defaults) and the sum over scales of its MSE objective.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops, pack
from ..nn_base import ConvP, FusedNet, dev_vec, entry_point


class LayerNorm(nn.Module):
    """Parameter holder of the ICN's custom LayerNorm (gamma, beta); reference models.py:15-35."""

    def __init__(self, num_features: int, eps: float = 1e-5, affine: bool = True):
        super().__init__()
        self.num_features, self.eps, self.affine = num_features, eps, affine
        if affine:
            self.gamma = nn.Parameter(torch.Tensor(num_features).uniform_())
            self.beta = nn.Parameter(torch.zeros(num_features))


class Conv2dBlock(nn.Module):
    """Parameter holder: [norm.{gamma,beta}], conv.{weight,bias} (reference models.py:38-90)."""

    def __init__(self, input_dim, output_dim, kernel_size, stride, padding=0, norm="none", activation="relu",
                 pad_type="zero"):
        super().__init__()
        if norm not in ("inst", "ln", "none") or activation not in ("relu", "tanh", "none") \
                or pad_type not in ("reflect", "zero"):
            raise NotImplementedError(f"Conv2dBlock(norm={norm}, activation={activation}, pad_type={pad_type})")
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding
        self.norm_type, self.act_type, self.pad_type = norm, activation, pad_type
        if norm == "ln":
            self.norm = LayerNorm(output_dim)
        self.conv = ConvP(input_dim, output_dim, kernel_size)


class ResBlock(nn.Module):
    def __init__(self, dim, norm="inst", activation="relu", pad_type="zero"):
        super().__init__()
        self.model = nn.Sequential(Conv2dBlock(dim, dim, 3, 1, 1, norm=norm, activation=activation, pad_type=pad_type),
                                   Conv2dBlock(dim, dim, 3, 1, 1, norm=norm, activation="none", pad_type=pad_type))


class ResBlocks(nn.Module):
    def __init__(self, num_blocks, dim, norm="inst", activation="relu", pad_type="zero"):
        super().__init__()
        self.model = nn.Sequential(*[ResBlock(dim, norm=norm, activation=activation, pad_type=pad_type)
                                     for _ in range(num_blocks)])


class ContentEncoder(nn.Module):
    def __init__(self, n_downsample, n_res, input_dim, dim, norm, activ, pad_type="zero"):
        super().__init__()
        layers = [Conv2dBlock(input_dim, dim, 7, 1, 3, norm=norm, activation=activ, pad_type="reflect")]
        for _ in range(n_downsample):
            layers.append(Conv2dBlock(dim, 2 * dim, 4, 2, 1, norm=norm, activation=activ, pad_type="reflect"))
            dim *= 2
        layers.append(ResBlocks(n_res, dim, norm=norm, activation=activ, pad_type=pad_type))
        self.model = nn.Sequential(*layers)
        self.output_dim = dim


class Decoder(nn.Module):
    def __init__(self, n_upsample, n_res, dim, output_dim, norm="batch", activ="relu", pad_type="zero"):
        super().__init__()
        layers = [ResBlocks(n_res, dim, norm, activ, pad_type=pad_type)]
        for _ in range(n_upsample):
            layers += [nn.Identity(),                                   # slot of the parameter-free Upsample
                       Conv2dBlock(dim, dim // 2, 5, 1, 2, norm="ln", activation=activ, pad_type="reflect")]
            dim //= 2
        layers.append(Conv2dBlock(dim, output_dim, 7, 1, 3, norm="none", activation="tanh", pad_type="reflect"))
        self.model = nn.Sequential(*layers)


class G_Resnet(FusedNet):
    def __init__(self, input_nc, output_nc=3, num_downs=2, n_res=3, ngf=64, norm="inst", nl_layer="relu"):
        super().__init__()
        if norm != "inst" or nl_layer != "relu":
            raise NotImplementedError("G_Resnet: only norm='inst', nl_layer='relu' (the reference's configuration)")
        self.input_nc, self.output_nc, self.num_downs, self.n_res = input_nc, output_nc, num_downs, n_res
        self.enc_content = ContentEncoder(num_downs, n_res, input_nc, ngf, norm, nl_layer, pad_type="reflect")
        self.dec = Decoder(num_downs, n_res, self.enc_content.output_dim, output_nc, norm=norm, activ=nl_layer,
                           pad_type="reflect")

    # ------------------------------------------------------------------ packing
    @staticmethod
    def _pack_block(blk: Conv2dBlock, device, upsample: int = 0):
        return pack.pack_conv(blk.conv.weight, blk.conv.bias, stride=blk.stride, pad=blk.padding,
                              pad_mode=L.PAD_REFLECT if blk.pad_type == "reflect" else L.PAD_ZERO,
                              upsample=upsample).to(device)

    def _pack_head(self, blk: Conv2dBlock, device):
        """7x7 -> output_nc head: row-split form when output_nc*7 fits one 32-wide N tile."""
        if blk.conv.cout * blk.kernel_size <= 32 and blk.pad_type == "reflect":
            return pack.pack_conv_rowsplit(blk.conv.weight, blk.conv.bias, pad=blk.padding, pad_mode=L.PAD_REFLECT).to(device)
        return self._pack_block(blk, device)

    def _pack_res(self, rbs: ResBlocks, device) -> List[tuple]:
        return [(self._pack_block(rb.model[0], device), self._pack_block(rb.model[1], device)) for rb in rbs.model]

    def _build_plans(self, device) -> dict:
        enc, dec = self.enc_content.model, self.dec.model
        nd = self.num_downs
        # 7x7 stem on 21 channels: K-channels padded to 24 - the tap-unit kernel stages the whole 14x22x24 halo once
        # and walks K in 8-channel units (74 MFMA k-steps; padding the channels to 32 for the halo kernel took 98)
        stem = enc[0]
        P = {"stem": pack.pack_conv(stem.conv.weight, stem.conv.bias, stride=1, pad=stem.padding, pad_mode=L.PAD_REFLECT,
                                    cin_pad=4).to(device),
             "down": [self._pack_block(enc[1 + i], device) for i in range(nd)],
             "enc_res": self._pack_res(enc[1 + nd], device),
             "dec_res": self._pack_res(dec[0], device),
             "up": [], "up_phases": [], "up_ring": [], "up_edge": [], "ln": [],
             "head": self._pack_head(dec[1 + 2 * nd], device)}
        for i in range(nd):
            blk = dec[2 + 2 * i]
            P["up"].append(self._pack_block(blk, device, upsample=1))
            # 5x5 reflect-padded conv after a 2x nearest upsample: also packed as the four 3x3 phase convolutions of
            # the low-res input (pack.up2_phase_weights: 2.8x fewer MACs), stacked into one launch whose DepthToSpace
            # store interleaves the phases; ops.conv_up2 picks the route per input
            ok = blk.kernel_size == 5 and blk.padding == 2 and blk.stride == 1 and blk.pad_type == "reflect"
            ok = ok and blk.conv.weight.shape[0] % 4 == 0
            P["up_phases"].append(pack.pack_conv_up2_d2s(blk.conv.weight, blk.conv.bias).to(device) if ok else None)
            # ... and, on request only (FUSG_UP2_RING9: measured no faster than the four 25-tap windows, ops.conv_up2), the
            # outermost ring of output pixels as twelve border-specific 3x3 launches (pack.pack_conv_up2_ring)
            P["up_ring"].append({k: v.to(device) for k, v in pack.pack_conv_up2_ring(blk.conv.weight, blk.conv.bias).items()}
                                if ok and ops._env_set("FUSG_UP2_RING9") else None)
            # ... and the border ring as an additive correction of the phase form: the frame taps in fp32 (pack.pack_conv_up2_edge;
            # None where the kernel does not take the channel counts)
            ed = pack.pack_conv_up2_edge(blk.conv.weight) if ok else None
            P["up_edge"].append(ed.to(device) if ed is not None else None)
            P["ln"].append((dev_vec(blk.norm.gamma, device), dev_vec(blk.norm.beta, device), blk.norm.eps))
        return P

    # ------------------------------------------------------------------ execution
    @staticmethod
    def _resblocks(plans, y: torch.Tensor) -> torch.Tensor:
        for pa, pb in plans:
            a, sa = ops.conv_in(pa, y)                      # InstanceNorm statistics come out of the conv epilogue
            b, sb = ops.conv_in(pb, a, pre_op=L.PRE_AFFINE_RELU, pre=sa, pre_bstride=a.shape[1])
            y = ops.affine_act(b, sb[0], sb[1], L.ACT_NONE, res=y)
        return y

    def _encode(self, P, x: torch.Tensor) -> torch.Tensor:
        c, st = ops.conv_in(P["stem"], ops.as_nhwc(x, cpad=P["stem"].c0k))
        for p in P["down"]:
            c, st = ops.conv_in(p, c, pre_op=L.PRE_AFFINE_RELU, pre=st, pre_bstride=c.shape[1])
        y = ops.affine_act(c, st[0], st[1], L.ACT_RELU)
        return self._resblocks(P["enc_res"], y)

    def _decode(self, P, y: torch.Tensor) -> torch.Tensor:
        y = self._resblocks(P["dec_res"], y)
        pre_op, pre, bs = L.PRE_NONE, None, 0
        for p, ph, rg, ed, (gamma, beta, eps) in zip(P["up"], P["up_phases"], P["up_ring"], P["up_edge"], P["ln"]):
            if ph is not None and ops.up2_phases_ok(y):
                # (scale, shift) from the phase launch's epilogue plus the ring correction's sums on the edge route, else streamed
                y, pre = ops.conv_up2(p, ph, y, pre_op=pre_op, pre=pre, pre_bstride=bs, ring=rg, edge=ed, ln=(gamma, beta, eps))
            else:
                y, pre = ops.conv_ln(p, y, gamma, beta, eps, pre_op=pre_op, pre=pre, pre_bstride=bs)
            pre_op, bs = L.PRE_AFFINE_RELU, y.shape[1]
        if P["head"].rowsplit is not None:
            return ops.conv_rowsplit(P["head"], y, pre_op=pre_op, pre=pre, pre_bstride=bs, act=L.ACT_TANH)
        return ops.conv(P["head"], y, pre_op=pre_op, pre=pre, pre_bstride=bs, act=L.ACT_TANH, nchw_out=True)

    @entry_point
    def decode(self, content: torch.Tensor) -> torch.Tensor:
        P = self._ensure(content)
        return self._decode(P, ops.as_nhwc(content))

    @entry_point
    def forward(self, image: torch.Tensor) -> torch.Tensor:
        P = self._ensure(image)
        if image.dim() != 4 or image.shape[1] != self.input_nc or image.shape[2] % 4 or image.shape[3] % 4:
            raise ValueError(f"G_Resnet expects [B,{self.input_nc},H,W] with H,W multiples of 4, got {tuple(image.shape)}")
        return self._decode(P, self._encode(P, image))


class D_NLayersMulti(FusedNet):
    """The ICN's multi-scale PatchGAN critic (reference models.py:211-259), forward only.  Scale i > 0 has
    ``round(ndf / 2**i)`` base channels and sees the input after i count-excluding 3 x 3 stride-2 average pools.
    Per scale: the stride-2 stem with LeakyReLU(0.2) in its epilogue; per normed layer ``ops.conv_in`` (InstanceNorm statistics
    from the conv) and one ``ops.affine_act`` applying norm + LeakyReLU; the final 1-channel conv.  ``forward`` returns the
    reference's list of logit maps; ``features`` every map of every scale."""

    def __init__(self, input_nc, ndf=64, n_layers=2, num_D=2):
        super().__init__()
        self.input_nc, self.ndf, self.n_layers, self.num_D = input_nc, ndf, n_layers, num_D
        for i in range(num_D):
            self.add_module("model_%d" % i, nn.Sequential(*self.get_layers(input_nc, int(round(ndf / (2 ** i))), n_layers)))

    @staticmethod
    def get_layers(input_nc, ndf=64, n_layers=3):
        """Parameter holders in the reference's slots (conv, [norm], LeakyReLU): each ConvP carries its stride."""
        I = nn.Identity

        def cv(cin, cout, stride):
            m = ConvP(cin, cout, 4)
            m.stride = stride
            return m
        seq = [cv(input_nc, ndf, 2), I()]
        nf = 1
        for n in range(1, n_layers):
            prev, nf = nf, min(2 ** n, 8)
            seq += [cv(ndf * prev, ndf * nf, 2), I(), I()]
        prev, nf = nf, min(2 ** n_layers, 8)
        seq += [cv(ndf * prev, ndf * nf, 1), I(), I()]
        seq += [cv(ndf * nf, 1, 1)]
        return seq

    def _build_plans(self, device) -> dict:
        P = {}
        for i in range(self.num_D):
            P[i] = [pack.pack_conv(m.weight, m.bias, stride=m.stride, pad=1).to(device)
                    for m in getattr(self, "model_%d" % i) if isinstance(m, ConvP)]
        return P

    @staticmethod
    def _scale(plans, x: torch.Tensor) -> List[torch.Tensor]:
        y = ops.conv(plans[0], x, act=L.ACT_LEAKY02)
        maps = [y]
        for p in plans[1:-1]:
            c, st = ops.conv_in(p, y)
            y = ops.affine_act(c, st[0], st[1], L.ACT_LEAKY02)
            maps.append(y)
        maps.append(ops.conv(plans[-1], y))
        return maps

    def _run(self, x: torch.Tensor) -> List[List[torch.Tensor]]:
        P = self._ensure(x)
        if x.dim() != 4 or x.shape[1] != self.input_nc:
            raise ValueError(f"D_NLayersMulti expects [B,{self.input_nc},H,W], got {tuple(x.shape)}")
        h, w = x.shape[2:]
        for _ in range(self.num_D - 1):
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        if (h >> self.n_layers) < 3 or (w >> self.n_layers) < 3:
            raise ValueError(f"D_NLayersMulti: {tuple(x.shape)} leaves the last scale's logit map empty")
        down = ops.as_nhwc(x.detach())
        out = []
        for i in range(self.num_D):
            out.append(self._scale(P[i], down))
            if i != self.num_D - 1:
                down = ops.avgpool3s2(down)
        return out

    @entry_point
    def features(self, input: torch.Tensor) -> List[List[torch.Tensor]]:
        """Per scale: [stem, normed layers ..., logits], each after its LeakyReLU (the reference's is in place) but the logits."""
        return self._run(input)

    @entry_point
    def forward(self, input: torch.Tensor) -> List[torch.Tensor]:
        return [maps[-1] for maps in self._run(input)]


class GANLoss(nn.Module):
    """The reference's least-squares objective (models.py:262-320), forward only: the sum over the scales of
    ``MSELoss(prediction [* mask], label [* mask])`` as a 0-d float32 device tensor, from ``ops.gan_terms``' squared column (the
    mask is sampled inside the kernel as ``F.interpolate(mask, size=prediction.shape[2:])`` samples it).  ``do_smooth`` draws
    ``torch.rand(1)`` from the CPU generator exactly as the reference does.  No host synchronisation."""

    def __init__(self, target_real_label=1.0, target_fake_label=0.0):
        super().__init__()
        self.register_buffer("real_label", torch.tensor(target_real_label))
        self.register_buffer("fake_label", torch.tensor(target_fake_label))
        self._labels = (torch.tensor(target_fake_label).to(torch.float32), torch.tensor(target_real_label).to(torch.float32))

    def __call__(self, predictions, target_is_real: bool, do_smooth: bool = False, mask: Optional[torch.Tensor] = None):
        total = None
        for prediction in predictions:
            label = self._labels[1 if target_is_real else 0]
            if do_smooth:
                label = label + (torch.rand(1) - 0.5) / 2.0           # [-0.25, 0.25], float32 like the reference's tensor
            if mask is not None:
                mask = mask.detach().to(prediction.device, torch.float32)
            t = ops.gan_terms(prediction.detach(), float(label), mask)
            mse = t[:, 2].sum() / t[:, 0].sum()
            total = mse if total is None else total + mse
        return total.to(torch.float32)


def get_icn_inputs(planes, sketch_normal, sketch_mask, central_crop, icn_w: int, icn_h: int):
    """ICN input assembly (reference warp_learn/models.py:323-366): crop all inputs to the 1.1x square box around the
    sketch mask, resize to (icn_w, icn_h), convert to Lab, scale to [-1, 1] and stack [sketch(3), central crop(3),
    planes(5x3)] -> float32 [1, 21, icn_h, icn_w] + crop_info.  Runs on the device (one libfusg launch,
    planes_utils.get_icn_inputs); numpy or CUDA uint8 images are accepted.  OpenCV arithmetic, parity unpinned."""
    from .planes_utils import get_icn_inputs as _impl
    return _impl(planes, sketch_normal, sketch_mask, central_crop, icn_w, icn_h)
