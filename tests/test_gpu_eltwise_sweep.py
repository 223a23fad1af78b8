"""GPU: every kernel of csrc/elementwise.hip over the case lists of tests/eltwise_sweep.py, through the C ABI (the wrappers of
ops.py allocate tight outputs and cannot express a pitch, a slice or a scale stride).  Bit equality with the float32
references; affine_act within one ulp of float64; the transcendental activations under the measured bars; and on every case
the destination's surroundings compared as integers after the launch (eltwise_sweep.outside_unchanged)."""
import ctypes as C

import numpy as np
import pytest
import torch

import eltwise_sweep as es

pytestmark = pytest.mark.gpu

from future_urban_scene_generation_amd import _lib as L          # noqa: E402
from future_urban_scene_generation_amd import ops                 # noqa: E402


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def up(view: torch.Tensor) -> torch.Tensor:
    """A CPU view on the device with its whole storage (surroundings included) and the same sizes, strides and offset."""
    flat = torch.empty(0, dtype=view.dtype).set_(view.untyped_storage())
    return flat.to(dev()).as_strided(view.shape, view.stride(), view.storage_offset())


def D(t: torch.Tensor):
    return C.byref(ops.desc(t))


def call(name: str, *args):
    L.check(getattr(L.lib(), name)(*args, ops.stream_ptr()), name)


def run_into(emb, launch) -> torch.Tensor:
    """Launch into the device copy of an embedded destination; the view's content on the CPU, once everything outside the
    view has been found unchanged."""
    view, buf = emb
    dbuf = buf.to(dev())
    launch(es.rebase(view, dbuf))
    after = dbuf.cpu()
    assert es.outside_unchanged(view, buf, after), "the launch wrote outside its destination view"
    return es.rebase(view, after)


def dst_slice(shape, off):
    """A canary-filled NHWC destination: tight at off == 0, else a slice at channel offset off of a buffer 8 channels wider."""
    return es.embed(shape, shape[1] + (8 if off else 0), off, es.CANARY)


IDS = dict(ids=repr)


# ---- affine_act ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", es.affine_cases(), **IDS)
def test_affine_act(c):
    from conftest import record
    d = es.affine_inputs(c)
    x = up(d["x"][0])
    sc, sh = (d[k].to(dev()) for k in ("scale", "shift")) if c.scale != "null" else (None, None)
    res = up(d["res"][0]) if c.res else None
    got = run_into(dst_slice((c.B, c.C, c.H, c.W), c.dst_off), lambda dst: call(
        "fusg_affine_act", D(x), sc.data_ptr() if sc is not None else None, sh.data_ptr() if sh is not None else None,
        d["bstride"], c.act, D(res) if c.res else None, D(dst))).numpy()
    xl, scl, shl, resl = es.affine_logical(d, c)
    ref, pre = es.ref_affine_act(xl, scl, shl, c.act, resl)
    assert not np.isnan(got).any()
    err = np.abs(got.astype(np.float64) - ref)
    if c.act in es.EXACT_ACTS:
        ulps = float((err / es.ulp32(np.maximum(np.abs(pre), np.abs(ref)))).max())
        record("ulp", ulps)
        print(f"{c}: {ulps:.3f} ulp")
        assert ulps <= 1.0, (c, ulps)
    else:
        record("abs_err", float(err.max()))
        print(f"{c}: abs err {err.max():.3e} (bar {es.ACT_BAR_AFFINE:.3e})")
        assert err.max() <= es.ACT_BAR_AFFINE, (c, float(err.max()))


# ---- maxpool2 / upsample2_add -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", es.pool_cases(), **IDS)
def test_maxpool2(c):
    xv = es.pool_inputs(c)["x"][0]
    x = up(xv)
    got = run_into(dst_slice((c.B, c.C, c.Ho, c.Wo), c.dst_off), lambda dst: call("fusg_maxpool2", D(x), D(dst))).numpy()
    ref = es.ref_maxpool2(xv.numpy())
    assert np.isnan(ref).any() == (c.kind == "nan")
    assert es.same_bits(got, ref), (c, int((got != ref).sum()))


@pytest.mark.parametrize("c", es.upsample_cases(), **IDS)
def test_upsample2_add(c):
    d = es.upsample_inputs(c)
    low, up1 = up(d["low"][0]), up(d["up1"][0])
    got = run_into(dst_slice((c.B, c.C, c.H, c.W), c.dst_off),
                   lambda dst: call("fusg_upsample2_add", D(low), D(up1), D(dst))).numpy()
    assert es.same_bits(got, es.ref_upsample2_add(d["low"][0].numpy(), d["up1"][0].numpy())), c


# ---- copy4d / add4d -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", es.copy_cases(), **IDS)
def test_copy4d(c):
    srcv = es.copy_inputs(c)
    src = up(srcv)
    if c.dst == "nhwc":
        view, buf = es.embed((c.B, max(c.C, c.fill), c.H, c.W), c.pitch, c.c_off, es.CANARY)
        dbuf = buf.to(dev())
        call("fusg_copy4d", D(src), D(es.rebase(view, dbuf)), c.fill)
        after = dbuf.cpu().numpy().view(np.int32)
        ref = es.ref_copy4d_buffer(srcv.numpy(), c.pitch, c.c_off, c.fill)
        assert np.array_equal(after, ref), (c, es.copy_route_of(c), int((after != ref).sum()))
    else:
        got = run_into(es.embed_nchw((c.B, c.C, c.H, c.W)), lambda dst: call("fusg_copy4d", D(src), D(dst), c.fill)).numpy()
        assert es.same_bits(got, srcv.numpy()), c


def test_add4d_mixed_layouts_into_a_slice():
    g = es.rng("add4d")
    a, b = es.randn(g, 2, 3, 5, 7), es.randn(g, 2, 3, 5, 7)
    da, db = up(es.source("a", a, 8, 1)[0]), up(torch.from_numpy(b))
    got = run_into(es.embed((2, 3, 5, 7), 8, 2, es.CANARY), lambda dst: call("fusg_add4d", D(da), D(db), D(dst))).numpy()
    assert es.same_bits(got, es.ref_add4d(a, b))


# ---- space_to_depth2 / depth_to_space2 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", es.s2d_cases(), **IDS)
def test_s2d_d2s(c):
    xv = es.s2d_inputs(c)["x"][0]
    x = up(xv)
    if c.op == "s2d":
        shape, fn, ref = (c.B, 4 * c.C, c.H, c.W), "fusg_space_to_depth2", es.ref_s2d(xv.numpy())
    else:
        shape, fn, ref = (c.B, c.C, 2 * c.H, 2 * c.W), "fusg_depth_to_space2", es.ref_d2s(xv.numpy())
    got = run_into(es.embed(shape, shape[1] + 8, c.dst_off, es.CANARY), lambda dst: call(fn, D(x), D(dst))).numpy()
    assert es.same_bits(got, ref), c


# ---- ec_inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", es.ec_cases(), **IDS)
def test_ec_inputs(c):
    views = es.ec_inputs_of(c)
    img, e, m = (up(v) for v in views)
    got = run_into(es.embed((c.B, 4, c.H, c.W), c.pitch, 0, es.CANARY),
                   lambda dst: call("fusg_ec_inputs", D(img), D(e), D(m), D(dst), c.mode)).numpy()
    assert es.same_bits(got, es.ref_ec_inputs(*(v.numpy() for v in views), c.mode)), c


# ---- hshift_sum ---------------------------------------------------------------------------------------------------------------
def _hshift_dsts(c):
    shape = (c.B, c.cout, c.H, c.W)
    cp = (c.cout + 3) // 4 * 4
    return (("nchw", es.embed_nchw(shape)), ("nhwc", es.embed(shape, cp, 0, es.CANARY)), ("slice", es.embed(shape, cp + 8, 3, es.CANARY)))


@pytest.mark.parametrize("c", es.hshift_cases(), **IDS)
def test_hshift_sum(c):
    from conftest import record
    (tv, _), bias = es.hshift_inputs(c)
    t, dbias = up(tv), torch.from_numpy(bias).to(dev())
    acc = es.ref_hshift_sum(tv.permute(0, 2, 3, 1).numpy(), bias, c.kw, c.pad, c.pm, c.cout)
    assert not np.isnan(acc).any()
    fails = []
    for act in es.ACTS:
        for kind, emb in _hshift_dsts(c):
            got = run_into(emb, lambda dst: call("fusg_hshift_sum", D(t), dbias.data_ptr(), c.kw, c.pad, c.pm, act, D(dst))).numpy()
            if act in es.EXACT_ACTS:
                ref = acc if act == es.NONE else np.maximum(acc, np.float32(0))
                if not es.same_bits(got, ref):
                    fails.append((act, kind, int((got != ref).sum())))
            else:
                err = float(np.abs(got.astype(np.float64) - es.act64(acc, act)).max())
                record("abs_err", err)
                if not err <= es.ACT_BAR_HSHIFT:
                    fails.append((act, kind, err))
    assert not fails, (c, es.hshift_route_of(c), fails)


@pytest.mark.parametrize("kw,pad,pm,w,cout,pitch", es.hshift_rejects())
def test_hshift_sum_turns_away_what_its_kernels_cannot_index(kw, pad, pm, w, cout, pitch):
    """The host's checks answer before any launch: an error status, and the destination as it was."""
    assert not es.hshift_accepts(kw, pad, pm, w)
    tv, _ = es.embed((1, max(1, cout * kw), 1, w), pitch, 0, 0.0)
    t, bias = up(tv), torch.zeros(4, device=dev())
    view, buf = es.embed_nchw((1, cout, 1, w))
    dbuf = buf.to(dev())
    with pytest.raises(L.FusgError):
        call("fusg_hshift_sum", D(t), bias.data_ptr(), kw, pad, pm, es.NONE, D(es.rebase(view, dbuf)))
    assert torch.equal(dbuf.cpu().view(torch.int32), buf.view(torch.int32))


# ---- argmax_hw ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", es.argmax_cases(), **IDS)
def test_argmax_hw(c):
    xv = es.argmax_input(c)
    x = up(xv)
    n, margin = c.B * xv.shape[1], 16
    idx = torch.full((n + 2 * margin,), es.CANARY, dtype=torch.int32)
    didx = idx.to(dev())
    call("fusg_argmax_hw", D(x), didx[margin:].data_ptr())
    after = didx.cpu().numpy()
    assert (after[:margin] == es.CANARY).all() and (after[margin + n:] == es.CANARY).all()
    got, ref = after[margin:margin + n].reshape(c.B, -1), es.ref_argmax_hw(xv.numpy())
    assert np.array_equal(got, ref), (c, dict(zip(es.ARGMAX_KINDS, zip(got.T.tolist(), ref.T.tolist()))))


# ---- to_image_u8 / merge_u8 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", es.u8_cases(), **IDS)
def test_to_image_u8(c):
    xv = es.u8_input(c)
    x = up(xv)
    got = run_into(es.embed((c.B, c.C, c.H, c.W), c.C + 1, 0, es.CANARY_U8, torch.uint8),
                   lambda dst: call("fusg_to_image_u8", D(x), D(dst))).permute(0, 2, 3, 1).numpy()
    ref = es.ref_to_image_u8(xv.numpy())
    assert np.array_equal(got, ref), (c, int((got != ref).sum()))


@pytest.mark.parametrize("c", es.merge_cases(), **IDS)
def test_merge_u8(c):
    views = es.merge_inputs(c)
    o, img, m = (up(v) for v in views)
    got = run_into(es.embed((c.B, c.C, c.H, c.W), c.C + 1, 0, es.CANARY_U8, torch.uint8),
                   lambda dst: call("fusg_merge_u8", D(o), D(img), D(m), D(dst))).permute(0, 2, 3, 1).numpy()
    ref = es.ref_merge_u8(*(v.numpy() for v in views))
    assert np.array_equal(got, ref), (c, int((got != ref).sum()))
