"""The border ring of nn.Upsample(2) -> ReflectionPad2d(2) -> 5x5 as an additive correction of the phase form (pack.pack_conv_up2_edge,
pack.up2_edge_delta: what fusg_up2_edge_fix adds), in float64 against the definition: conv5x5(reflect-padded) - conv5x5(replicate-padded)."""
import pytest
import torch
import torch.nn.functional as F

from future_urban_scene_generation_amd import pack

SHAPES = [(2, 2), (3, 5), (8, 16)]
B, CIN, COUT = 2, 32, 16


def _definition(w5: torch.Tensor, fx: torch.Tensor) -> torch.Tensor:
    u = F.interpolate(fx, scale_factor=2, mode="nearest")
    return F.conv2d(F.pad(u, (2, 2, 2, 2), mode="reflect"), w5) - F.conv2d(F.pad(u, (2, 2, 2, 2), mode="replicate"), w5)


def _ring_mask(h: int, w: int) -> torch.Tensor:
    m = torch.zeros(2 * h, 2 * w, dtype=torch.bool)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    return m


def _case(h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    w5 = torch.randn(COUT, CIN, 5, 5, generator=g, dtype=torch.float32)           # fp32-representable: the pack holds fp32
    fx = torch.randn(B, CIN, h, w, generator=g, dtype=torch.float64)
    return w5, fx


@pytest.mark.parametrize("h,w", SHAPES)
def test_packed_edge_taps_reproduce_reflect_minus_replicate(h, w):
    w5, fx = _case(h, w)
    edge = pack.pack_conv_up2_edge(w5)
    assert edge.w.dtype == torch.float32 and tuple(edge.w.shape) == (4, 5, CIN // 16, COUT // 16, 64, 4)
    assert torch.equal(edge.taps(), pack.up2_edge_taps(w5))                        # the lane order is a permutation
    want = _definition(w5.double(), fx)
    got = pack.up2_edge_delta(edge.taps(), fx)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-12 * scale
    # the definition itself is exactly zero off the ring, and so is the correction
    ring = _ring_mask(h, w)
    assert float(want[:, :, ~ring].abs().max() if (~ring).any() else 0.0) == 0.0
    assert float(got[:, :, ~ring].abs().max() if (~ring).any() else 0.0) == 0.0


@pytest.mark.parametrize("h,w", SHAPES)
def test_each_frame_element_is_used_once(h, w):
    """With an all-ones centre-free probe: a filter that is 1 on exactly one frame tap position sums every frame element that
    tap reaches; summed over the 16 frame taps of the 5x5 (ring of the filter) and all output pixels, every non-zero element of
    D = reflect - replicate must be counted as often as the dense convolution counts it."""
    _, fx = _case(h, w, seed=1)
    fx = fx[:, :1]                                                                 # one channel is enough
    u = F.interpolate(fx, scale_factor=2, mode="nearest")
    D = F.pad(u, (2, 2, 2, 2), mode="reflect") - F.pad(u, (2, 2, 2, 2), mode="replicate")
    for ky in range(5):
        for kx in range(5):
            w5 = torch.zeros(1, 1, 5, 5, dtype=torch.float64)
            w5[0, 0, ky, kx] = 1.0
            got = pack.up2_edge_delta(pack.up2_edge_taps(w5), fx)
            # a one-hot filter shifts D: output (y, x) = D[y + ky, x + kx] (padded coordinates) - each element once, exactly
            want = D[:, :, ky:ky + 2 * h, kx:kx + 2 * w]
            assert torch.equal(got, want), (ky, kx)


@pytest.mark.parametrize("tap", [(0, 0), (0, 2), (4, 4), (2, 0)])
@pytest.mark.parametrize("h,w", SHAPES)
def test_one_hot_filters_isolate_corner_edge_and_column_taps(h, w, tap):
    w5, fx = _case(h, w, seed=2)
    hot = torch.zeros_like(w5)
    hot[:, :, tap[0], tap[1]] = w5[:, :, tap[0], tap[1]]
    edge = pack.pack_conv_up2_edge(hot)
    want = _definition(hot.double(), fx)
    got = pack.up2_edge_delta(edge.taps(), fx)
    assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)
    # which sides the tap feeds: (0, 0) top row and left column (the corner pixel from both), (0, 2) the top row only,
    # (4, 4) bottom row and right column, (2, 0) the left column only
    nz = (got.abs().sum(dim=(0, 1)) > 0)
    rows = {"top": bool(nz[0, 1:-1].any()), "bottom": bool(nz[-1, 1:-1].any())} if w > 1 else {}
    assert rows.get("top", False) == (tap[0] == 0) and rows.get("bottom", False) == (tap[0] == 4)
    if 2 * h > 2:
        assert bool(nz[1:-1, 0].any()) == (tap[1] == 0) and bool(nz[1:-1, -1].any()) == (tap[1] == 4)


def test_shapes_the_kernel_does_not_take_pack_to_none():
    assert pack.pack_conv_up2_edge(torch.randn(16, 24, 5, 5)) is None
    assert pack.pack_conv_up2_edge(torch.randn(12, 32, 5, 5)) is None
    assert pack.pack_conv_up2_edge(torch.randn(16, 32, 5, 5)) is not None
