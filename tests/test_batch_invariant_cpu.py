"""CPU: the routing batch (fusg_set_route_batch / ops.route_batch) in the library's host code and in ops' own decisions.
With R set, the tuple that fixes a conv launch's summation order - (family, tile, ksplit, ksw), fusg_conv2d_route_order - no
longer depends on the number of images in the launch; the workspace still does."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import REPO
from future_urban_scene_generation_amd import _lib as L
from future_urban_scene_generation_amd import ops, pack

import batch_invariant_layers as bl

NEW = ("fusg_set_route_batch", "fusg_route_batch", "fusg_conv2d_route_order")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


@pytest.fixture(autouse=True)
def _mode_off(lib):
    """Every test starts and ends with the mode off."""
    ops.set_route_batch(0)
    yield
    ops.set_route_batch(0)


def test_exports_and_version(lib):
    hdr = open(os.path.join(REPO, "include", "fusg.h")).read()
    declared = set(re.findall(r"\b(fusg_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.fusg_version() == 118 and "#define FUSG_VERSION 118" in hdr


def test_setter_validates_and_round_trips(lib):
    assert lib.fusg_route_batch() == 0
    prev = 0
    for n in (0, 1, 64, 1 << 20):
        assert lib.fusg_set_route_batch(n) == prev                  # returns the previous value
        assert lib.fusg_route_batch() == n
        prev = n
    for bad in (-1, (1 << 20) + 1):
        assert lib.fusg_set_route_batch(bad) == -1                  # FUSG_ERR_INVALID, nothing changed
        assert b"set_route_batch" in lib.fusg_last_error() and str(bad).encode() in lib.fusg_last_error()
        assert lib.fusg_route_batch() == prev
    assert lib.fusg_set_route_batch(0) == prev and lib.fusg_route_batch() == 0


def test_ops_entry_points(lib):
    assert ops.ROUTE_BATCH == 0
    assert ops.set_route_batch(8) == 0 and ops.ROUTE_BATCH == 8 and lib.fusg_route_batch() == 8
    with ops.route_batch(32):
        assert ops.ROUTE_BATCH == 32 and lib.fusg_route_batch() == 32
        with ops.route_batch(None):                                 # None: leaves what is in force
            assert ops.ROUTE_BATCH == 32 and lib.fusg_route_batch() == 32
        with ops.route_batch(0):
            assert ops.ROUTE_BATCH == 0 and lib.fusg_route_batch() == 0
        assert ops.ROUTE_BATCH == 32 and lib.fusg_route_batch() == 32
    assert ops.ROUTE_BATCH == 8 and lib.fusg_route_batch() == 8
    with pytest.raises(ValueError):
        ops.set_route_batch(-1)
    assert ops.ROUTE_BATCH == 8 and lib.fusg_route_batch() == 8
    assert ops.set_route_batch(0) == 8


def test_route_order_refuses_what_conv2d_refuses(lib):
    d = L.ConvDesc()
    out = (C.c_int32 * 4)()
    assert lib.fusg_conv2d_route_order(C.byref(d), C.byref(out)) == -1 and b"src0" in lib.fusg_last_error()
    assert lib.fusg_conv2d_route_order(C.byref(d), None) == -1


# (family, tile, ksplit, ksw) observed with the mode off - family: 0 / 1 generic fp32 / split-fp16 (tile = FUSG_TILE_*, 3 = 128x32,
# 4 = 64x64), 2 halo, 3 halo in parity-quadrant form (tile = column-tile width); ksw: halo K split over the waves:
#   c256_k3_16x16  f16x3   n = 1 (1, 4, 18, 0)   2 (1, 4, 16, 0)   8, 9 (1, 4, 4, 0)   32 (2, 32, 1, 1)   64 (2, 64, 1, 1)
#                  (hand-derived in the issue: ksplit 18 / 4 / halo at 1 / 9 / 32 - confirmed; the halo launches at 32 and 64 split K
#                  over the waves and differ in their column tile)
#   c32_k3_64x128  f16x3   n = 1, 2 (1, 3, 2, 0)   8, 9 (2, 32, 1, 1)   32, 64 (2, 32, 1, 0)              (as derived by hand)
#   c128_k1_32x32          n <= 9 (2, 32, 1, 0)   32, 64 (2, 64, 1, 0)
#   c64_c32_k3_128x128     n = 1 (1, 3, 4, 0)   2, 8 (2, 32, 1, 1)   >= 9 (2, 32, 1, 0)
#   s2_k4_quadrant_64x64   n = 1, 2 (1, 4, 8, 0)   8, 9 (3, 32, 1, 0)   32 (3, 64, 1, 0)   64 (3, 128, 1, 0)
#   small_c512_k3_4x4 f32  ksplit 32, 32, 32, 22, 8, 4 on the generic fp32 gather
#   the 7x7 stem (tap-unit kernel, column tile 64) and the small-image launches in f16x3 / bf16 are constant
# f32 / bf16 follow f16x3 with families 0 / 9 / 10 and 1 / 5 / 11.
EXPECT_OFF = {
    ("c256_k3_16x16", "f16x3"): {1: (1, 4, 18, 0), 9: (1, 4, 4, 0), 32: (2, 32, 1, 1)},
    ("c32_k3_64x128", "f16x3"): {1: (1, 3, 2, 0), 9: (2, 32, 1, 1), 32: (2, 32, 1, 0)},
}


def test_mode_off_table_discriminates(lib):
    """(a) With R = 0 the tuple changes with n on the layers that matter: the table exercises real route changes."""
    varying = set()
    for name in bl.LAYERS:
        for prec in bl.PRECISIONS:
            if len({bl.route_order(name, n, prec) for n in bl.BATCHES}) > 1:
                varying.add((name, prec))
    for name in ("c256_k3_16x16", "c32_k3_64x128"):
        for prec in bl.PRECISIONS:
            assert (name, prec) in varying, (name, prec)
    for (name, prec), want in EXPECT_OFF.items():
        for n, t in want.items():
            assert bl.route_order(name, n, prec) == t, (name, prec, n)


@pytest.mark.parametrize("R", (1, 8, 32))
def test_mode_on_order_is_constant(lib, R):
    """(b) With R set the tuple is the same for every n, and it is the R = 0 tuple at n = R."""
    for name in bl.LAYERS:
        for prec in bl.PRECISIONS:
            want = bl.route_order(name, R, prec)                    # mode off, n = R
            with ops.route_batch(R):
                for n in bl.BATCHES + (R,):
                    assert bl.route_order(name, n, prec) == want, (name, prec, R, n)
            assert bl.route_order(name, R, prec) == want


@pytest.mark.parametrize("R", (1, 8, 32))
def test_workspace_scales_with_real_batch(lib, R):
    """(c) fusg_conv2d_plan under R: the chosen ksplit is R's, the bytes are ksplit x the REAL M x cout_pad floats."""
    some = 0
    for name, s in bl.LAYERS.items():
        for prec in bl.PRECISIONS:
            d0, _ = bl.planned_desc(name, R, prec)                  # mode off at n = R: the ksplit R stands for
            with ops.route_batch(R):
                for n in bl.BATCHES:
                    d, nbytes = bl.planned_desc(name, n, prec)
                    assert (d.tile, d.ksplit) == (d0.tile, d0.ksplit), (name, prec, n)
                    want = d.ksplit * n * d.qh * d.qw * d.cout_pad * 4 if d.ksplit > 1 else 0
                    assert nbytes == want, (name, prec, n, nbytes, want)
                    some += nbytes > 0
    assert some > 0


def test_entry_nin_route_follows_routing_batch(lib):
    """fusg_conv2d_entry_nin_route on the descriptors ops.entry_nin builds: one form for every b under R, the mode-off form at
    b = R.  (16 x 32, four patches per image: K split over the waves up to 64 workgroups of the 32-column tile, no fused form
    once the router picks the 64-column tile.)"""
    g = torch.Generator().manual_seed(5)
    nin = pack.pack_conv(torch.randn(128, 6, 1, 1, generator=g), torch.zeros(128))
    res = pack.pack_conv(torch.randn(128, 128, 3, 3, generator=g) * 0.03, torch.zeros(128), pad=1)

    def form(b, hw):
        u = torch.zeros(b, hw[0], hw[1], 8).permute(0, 3, 1, 2)[:, :6]          # six channels at a pitch of eight
        with ops.status_scope(torch.zeros(4, dtype=torch.int32)):
            dr, dn = ops._entry_nin_descs(nin, res, u, ops.nhwc_empty(b, 128, hw[0], hw[1], "cpu"), "f16x3", ksplit=1)
        return int(lib.fusg_conv2d_entry_nin_route(C.byref(dr), C.byref(dn)))

    hw = (16, 32)
    off = {b: form(b, hw) for b in (1, 9, 64)}
    assert off == {1: 2, 9: 2, 64: 0}, off                          # the form depends on the grid with the mode off
    for R in (1, 64):
        with ops.route_batch(R):
            assert {form(b, hw) for b in (1, 9, 64)} == {off[R]}, (R, off)


def _bneck_plans():
    g = torch.Generator().manual_seed(3)
    mk = lambda co, ci, k: pack.pack_conv(torch.randn(co, ci, k, k, generator=g) * 0.05, torch.zeros(co), pad=k // 2)
    return {"c1": mk(128, 256, 1), "c2": mk(128, 128, 3), "c3": mk(256, 128, 1)}


def test_python_decisions(lib, monkeypatch):
    for k in ("FUSG_NO_BNECK", "FUSG_BNECK_MAXHW", "FUSG_NO_SMALL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(ops, "BNECK_MINHW", None)
    p = _bneck_plans()
    x = {b: torch.empty((b, 256, 16, 16), device="meta") for b in (1, 8, 9, 32)}
    # today's answers: at 16 x 16 the fused block from 9 images up (f16x3); _nchunk falls with the batch
    assert [ops.bottleneck_ok(p, x[b], "f16x3") for b in (1, 8, 9, 32)] == [False, False, True, True]
    today = [ops._nchunk(b, 64, 32 * 32) for b in (1, 8, 9, 32)]
    assert today == [16, 16, 16, 16] and [ops._nchunk(b, 64, 256 * 256) for b in (1, 8, 9, 32)] == [1024, 128, 113, 32]
    with ops.route_batch(8):
        assert [ops.bottleneck_ok(p, x[b], "f16x3") for b in (1, 8, 9, 32)] == [False] * 4
        assert [ops._nchunk(b, 64, 256 * 256) for b in (1, 8, 9, 32)] == [128] * 4
        assert [ops._nchunk(b, 64, 32 * 32) for b in (1, 8, 9, 32)] == [16] * 4
    with ops.route_batch(32):
        assert [ops.bottleneck_ok(p, x[b], "f16x3") for b in (1, 8, 9, 32)] == [True] * 4
        assert [ops._nchunk(b, 64, 256 * 256) for b in (1, 8, 9, 32)] == [32] * 4
    assert [ops.bottleneck_ok(p, x[b], "f16x3") for b in (1, 8, 9, 32)] == [False, False, True, True]
    assert [ops._nchunk(b, 64, 256 * 256) for b in (1, 8, 9, 32)] == [1024, 128, 113, 32]
