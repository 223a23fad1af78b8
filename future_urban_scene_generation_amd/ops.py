"""Thin Python wrappers over the libfusg C ABI (include/fusg.h).

PyTorch is used here only as plumbing: device allocations (caching allocator), the current HIP
stream, and host<->device copies.  All arithmetic on activations happens inside libfusg kernels.
Activations are torch tensors of *logical* NCHW shape whose memory is NHWC ("NHWC-physical":
channels contiguous, channel pitch a multiple of 4) so that callers can still `.cpu().numpy()`
them like any other tensor.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib as L
from .pack import ConvPlan

_DT = {torch.float32: L.F32, torch.uint8: L.U8, torch.int32: L.I32}

# Arithmetic of the conv contraction (include/fusg.h fusg_precision): "f32" = exact fp32 MFMA,
# "f16x3" = split-fp16 (fp32-class accuracy, 3 passes at the fp16 matrix rate).  Process-wide default,
# overridable per call; FUSG_PRECISION in the environment sets the initial value.
import contextlib as _contextlib
import os as _os
from types import SimpleNamespace as _SimpleNamespace
import numpy as _np


def _env_set(name: str) -> bool:
    """Development switch read from the environment (per call: tests and bench flip some of them at run time)."""
    return name in _os.environ


_PREC = {"f32": L.PREC_F32, "f16x3": L.PREC_F16X3,
         # BASELINE configs[4]: single-pass bf16 MFMA on the halo-kernel layers, f16x3 elsewhere (include/fusg.h)
         "bf16": L.PREC_BF16,
         # single-pass fp16 on the halo and tap-unit layers (f16x3's first product of three: 11 significant bits per operand, the
         # split's weight scales and range guard), f16x3 elsewhere (include/fusg.h)
         "f16": L.PREC_F16,
         # evidence paths (include/fusg.h): operands rounded to 8 / 16 significant bits on the exact-fp32 kernel
         "emu_bf16": L.PREC_EMU_BF16, "emu_bf16x2": L.PREC_EMU_BF16X2}
_EMU_BITS = {"emu_bf16": 8, "emu_bf16x2": 16}


def _round_sig_bits(w: torch.Tensor, bits: int) -> torch.Tensor:
    """fp32 -> nearest (ties to even) value with `bits` significant bits, as fp32."""
    drop = 24 - bits
    u = w.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + ((1 << (drop - 1)) - 1) + ((u >> drop) & 1)) & ~((1 << drop) - 1) & 0xFFFFFFFF
    u = torch.where(u >= (1 << 31), u - (1 << 32), u).to(torch.int32)
    return u.view(torch.float32)
PRECISION = _os.environ.get("FUSG_PRECISION", "f16x3")


def set_precision(name: str) -> None:
    global PRECISION
    if name not in _PREC:
        raise ValueError(f"precision must be one of {list(_PREC)}")
    PRECISION = name


class precision:
    """`with ops.precision("f32"):` - temporary override of the process-wide contraction arithmetic."""

    def __init__(self, name: str):
        if name not in _PREC:
            raise ValueError(f"precision must be one of {list(_PREC)}")
        self.name = name

    def __enter__(self):
        global PRECISION
        self.prev, PRECISION = PRECISION, self.name
        return self

    def __exit__(self, *exc):
        global PRECISION
        PRECISION = self.prev
        return False


# ---- routing batch: a row's bits independent of its batch ---------------------------------------------------
# Which kernel family a layer runs on, its tile and its K split - the order of its sums - depend on how many images share
# the launch.  With a routing batch R > 0 every such decision, in the library (include/fusg.h, fusg_set_route_batch) and
# here (`bottleneck_ok`, `_nchunk`, the memoised route questions), is made as if the launch held R images; sizes, grids and
# bounds keep describing the real launch.  0 (the default) decides by the real batch.  Process-wide like PRECISION;
# FUSG_ROUTE_BATCH=n in the environment sets the initial value (read once at import, applied when the library loads).
ROUTE_BATCH = L.ROUTE_BATCH_ENV


def set_route_batch(n: int) -> int:
    """Set the routing batch (0 = off, at most 2**20); returns the previous value.  Not to be changed while another thread
    issues launches."""
    global ROUTE_BATCH
    n = int(n)
    prev = L.lib().fusg_set_route_batch(n)
    if prev < 0:
        raise ValueError(f"route batch {n}: {L.lib().fusg_last_error().decode()}")
    ROUTE_BATCH = n
    return int(prev)


class route_batch:
    """`with ops.route_batch(8):` - temporary routing batch (None leaves the current one in force)."""

    def __init__(self, n: Optional[int]):
        self.n = n

    def __enter__(self):
        self.prev = None if self.n is None else set_route_batch(self.n)
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            set_route_batch(self.prev)
        return False


def _route_n(b: int) -> int:
    """The image count a routing decision sees for a launch of b images."""
    return ROUTE_BATCH if ROUTE_BATCH > 0 else int(b)


# ---- range guard of the split-fp16 contraction --------------------------------------------------------------
# An f16x3 launch that stages an operand with |x| >= 2^15 (or a non-finite one) cannot represent it and raises a
# device-side status word instead of clamping (include/fusg.h, fusg_precision).  The word is caller-owned: one int32
# per device, here.  The module entry points (nn_base.range_guarded) and VehiclePipeline.run read it after their
# launches and redo the call in exact fp32 when it is set, so a result computed from a saturated operand never
# reaches the caller.
# Single-threaded by contract, like the reference's callers (Threading): `_GUARD`, `_STATUS_SCOPE`,
# `PRECISION` and `RECORDER` are process-wide, not per-thread.
_STATUS = {}
_STATUS_SCOPE = []                       # innermost `status_scope` word; empty: the device's default word
_GUARD = {"depth": 0, "deferred": 0}


def range_guarded() -> bool:
    """Do launches of the current precision use the fp16 split (and hence its range status)?  f16x3 does everywhere;
    bf16 does on the layers that do not run on the halo kernel (and the hourglass keeps f16x3 under it); f16 does everywhere
    too - its single-pass launches keep the split's status word."""
    return PRECISION in ("f16x3", "bf16", "f16")


def halo_precision() -> bool:
    """Does the current precision route qualifying layers to the halo kernel?  (f32: its exact-fp32 mode, round 4.)"""
    return PRECISION in ("f16x3", "bf16", "f16") or (PRECISION == "f32" and not _env_set("FUSG_NO_F32_HALO"))


def new_status_word(device) -> torch.Tensor:
    return torch.zeros(4, dtype=torch.int32, device=torch.device(device))


def status_word(device) -> torch.Tensor:
    """The word the launches issued NOW report to: the innermost `status_scope`'s, else the device's default one
    (what the module entry points read)."""
    if _STATUS_SCOPE:
        return _STATUS_SCOPE[-1]
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    w = _STATUS.get(key)
    if w is None:
        w = _STATUS[key] = new_status_word(torch.device("cuda", key))
    return w


class status_scope:
    """Launches issued inside report their range status to `word` instead of the device's default word.  A
    VehiclePipeline owns one: passes issued with check="async" then cannot be cleared (or mistaken for its own) by a
    module entry point called between them and `finish()` - each reader only ever sees the launches it issued."""

    def __init__(self, word: torch.Tensor):
        self.word = word

    def __enter__(self):
        _STATUS_SCOPE.append(self.word)
        return self

    def __exit__(self, *exc):
        _STATUS_SCOPE.pop()
        return False


def range_exceeded(device, clear: bool = True, word: Optional[torch.Tensor] = None) -> bool:
    """Has any f16x3 launch reporting to `word` (default: the current scope's / the device's word) since the last
    clear seen an operand outside the split's range?  Synchronises the current stream (a 4-byte read)."""
    w = status_word(device) if word is None else word
    hit = bool(w[0].item())
    if hit and clear:
        w.zero_()
    return hit


class defer_range_check:
    """Inside this context the module entry points do not read the status word (no host synchronisation per
    network): the caller checks once, after all its launches (VehiclePipeline.run / finish)."""

    def __enter__(self):
        _GUARD["deferred"] += 1
        return self

    def __exit__(self, *exc):
        _GUARD["deferred"] -= 1
        return False


def _require_gpu(t: torch.Tensor, what: str = "input") -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device}: the MI355X-native modules run on a HIP device only "
                           "(there is no CPU fallback; the CPU oracle lives in oracle/ for tests)")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr() -> int:
    """Raw hipStream_t of torch's current stream on the current device (the fast C accessor when this torch has
    it: `torch.cuda.current_stream()` costs ~4 us of Python per call, and there are ~370 launches per pass)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


_NO_TENSOR = L.Tensor()

# ---- recorded passes (include/fusg.h, fusg_plan) -----------------------------------------------------------------
# While `RECORDER` is set, the calling thread is recording a pass into a fusg_plan (pipeline.CompiledPass): libfusg
# remembers every launch by itself; the Python side only has to route the two things that are not libfusg launches
# through the recorder - cross-stream dependencies and the host-to-device copies of per-pass host data.
RECORDER = None


class PlanRecorder:
    def __init__(self):
        self.handle = L.lib().fusg_plan_create()
        self.noise_slots = []                  # [(pinned host buffer, [shape, ...])] in draw order
        self.keep = []                         # tensors the recorded launches point into beyond the memory pool

    def dependency(self, waiter: int, signaller: int) -> None:
        L.check(L.lib().fusg_plan_add_dependency(self.handle, waiter, signaller), "plan_add_dependency")

    NSLOTS = 4                                 # ring depth of the pinned sources: the host may run this many passes ahead

    def h2d(self, dst: torch.Tensor, src_ring: torch.Tensor) -> None:
        """src_ring: pinned [NSLOTS, n] - slot 0 holds the data of the recording pass."""
        assert src_ring.is_pinned() and dst.is_cuda and src_ring.dim() == 2 and src_ring.shape[0] == self.NSLOTS
        nbytes = dst.numel() * dst.element_size()
        assert nbytes == src_ring.shape[1] * src_ring.element_size()
        L.check(L.lib().fusg_plan_add_h2d(self.handle, dst.data_ptr(), src_ring.data_ptr(), nbytes, self.NSLOTS,
                                          src_ring.stride(0) * src_ring.element_size(), stream_ptr()), "plan_add_h2d")


# ---- side streams ---------------------------------------------------------------------------------------------------
# Launches that depend on little else (the VUnet's shape encoder, its 1x1 skip projections, the conditioning of its
# autoregressive blocks) are issued on side streams so that they do not lengthen the chain of dependent launches on
# the main one - what bounds a pass at small batches.  Both directions of every hand-over are explicit
# (fork_to / join_from; through the plan recorder while a pass is being recorded), and a tensor that a side stream
# reads must be kept referenced by the caller until the join: the caching allocator only knows the stream a tensor was
# allocated on, and a recorded pass replays the addresses of the recording with no allocator in the loop.
# Fork each branch ONCE and join it once: every additional event hand-over between streams costs ~0.2 ms of latency
# on this stack (measured: the VUnet's 14 skip projections forked level by level onto a fifth stream made a B=1 replay
# 2.2 -> 4.1 ms and B=8 1223 -> 966 crops/s; GPU_MAX_HW_QUEUES made no difference) - DESIGN.md §9.
_SIDE = {}


def side_streams_enabled() -> bool:
    return _os.environ.get("FUSG_STREAMS", "1") != "0" and _os.environ.get("FUSG_VUNET_SPLIT", "1") != "0"


def side_stream(name: str, device) -> "torch.cuda.Stream":
    dev = torch.device(device)
    key = (name, dev.index if dev.index is not None else torch.cuda.current_device())
    st = _SIDE.get(key)
    if st is None:
        st = _SIDE[key] = torch.cuda.Stream(device=dev, priority=-1)
    return st


def fork_to(st: "torch.cuda.Stream") -> None:
    """`st` may not start anything issued from now on before what is queued on the current stream has finished."""
    cur = torch.cuda.current_stream(st.device)
    if RECORDER is None:
        st.wait_stream(cur)
    else:
        RECORDER.dependency(st.cuda_stream, cur.cuda_stream)


def join_from(st: "torch.cuda.Stream", tensors=()) -> None:
    """The current stream waits for `st`; `tensors` (allocated under `st`) will be used on the current stream."""
    cur = torch.cuda.current_stream(st.device)
    if RECORDER is None:
        cur.wait_stream(st)
    else:
        RECORDER.dependency(cur.cuda_stream, st.cuda_stream)
    for t in tensors:
        t.record_stream(cur)


def desc(t: Optional[torch.Tensor]) -> L.Tensor:
    """fusg_tensor for a 4-D torch tensor (or an absent tensor: a shared all-zero struct, never written to)."""
    if t is None:
        return _NO_TENSOR
    d = L.Tensor()
    assert t.dim() == 4, t.shape
    d.data = t.data_ptr()
    d.n, d.c, d.h, d.w = t.shape
    d.sn, d.sc, d.sh, d.sw = t.stride()
    d.dtype = _DT[t.dtype]
    return d


def h2d(a, device, dtype=None) -> torch.Tensor:
    """Small host data (a list, a numpy array, a CPU tensor) to the device WITHOUT synchronising the stream: staged in
    pinned memory (torch's caching host allocator holds the block until the copy has run) and copied asynchronously.
    `torch.tensor(..., device=...)` / `.to(device)` from pageable memory wait for everything queued on the stream - one
    such call per frame is enough to serialise `VehiclePipeline.run_frames`' host against its GPU."""
    if isinstance(a, _np.ndarray) and not a.flags.writeable:
        a = a.copy()                       # (a broadcast view: torch refuses to wrap read-only memory silently)
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(a)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous().pin_memory().to(device, non_blocking=True)


def d2h(t: torch.Tensor) -> _np.ndarray:
    """A device tensor to a host numpy array: a BLOCKING copy (the host waits for everything queued before it on the current
    stream).  The frame drivers' device-pose front stage makes exactly one of these per frame and routes it through here, so a
    test can count them."""
    return t.cpu().numpy()


def nhwc_empty(b: int, c: int, h: int, w: int, device, dtype=torch.float32, zero: bool = False) -> torch.Tensor:
    """Logical [b, c, h, w] view over a fresh NHWC buffer whose channel pitch is c rounded up to 4."""
    cp = (c + 3) // 4 * 4
    buf = (torch.zeros if zero else torch.empty)((b, h, w, cp), device=device, dtype=dtype)
    t = buf.permute(0, 3, 1, 2)
    t = t if cp == c else t[:, :c]
    if zero:
        t._fusg_zero_pad = True         # this very object: its padding channels hold zeros (see as_nhwc)
    return t


def pitch_view(t: torch.Tensor) -> torch.Tensor:
    """An NHWC-physical tensor widened to its whole channel pitch (a view: the padding channels hold whatever the buffer
    does), for the float4 elementwise kernels on a tensor whose channel count is no multiple of 4."""
    b, c, h, w = t.shape
    return t if c == t.stride(3) else t.as_strided((b, t.stride(3), h, w), t.stride(), t.storage_offset())


def is_nhwc(t: torch.Tensor) -> bool:
    if t.dim() != 4 or t.dtype != torch.float32 or not t.is_cuda:
        return False
    b, c, h, w = t.shape
    sn, sc, sh, sw = t.stride()
    if c > 1 and sc != 1:
        return False
    if sw < c or sw % 4:
        return False
    if h > 1 and sh != w * sw:
        return False
    if b > 1 and sn != h * w * sw:
        return False
    return t.data_ptr() % 16 == 0


def copy4d(src: torch.Tensor, dst: torch.Tensor, c_fill: int = 0) -> torch.Tensor:
    L.check(L.lib().fusg_copy4d(C.byref(desc(src)), C.byref(desc(dst)), int(c_fill), stream_ptr()), "copy4d")
    return dst


def as_nhwc(t: torch.Tensor, cpad: int = 4) -> torch.Tensor:
    """Return `t` itself if it already is NHWC-physical f32, else a converted copy (channel padding
    zero-filled).  Used at the module boundary for caller-provided NCHW tensors.  `cpad` > 4 forces a
    copy whose channel pitch is a multiple of cpad (zero-filled), for layers packed with cin_pad."""
    _require_gpu(t)
    if t.dtype != torch.float32:
        raise TypeError(f"expected float32, got {t.dtype}")
    if cpad == 4 and is_nhwc(t):
        return t
    b, c, h, w = t.shape
    cp = (c + cpad - 1) // cpad * cpad
    # a buffer of ours whose pixel pitch already is the layer's and whose padding channels are known to be zero (the
    # glue kernels' outputs, a recorded pass's inputs): read in place, e.g. the ICN stem on fusg_icn_inputs' 24-pitch rows
    if getattr(t, "_fusg_zero_pad", False) and is_nhwc(t) and t.stride(3) == cp:
        return t
    buf = torch.empty((b, h, w, cp), device=t.device, dtype=torch.float32)
    full = buf.permute(0, 3, 1, 2)
    copy4d(t, full, cp)
    out = full if cp == c else full[:, :c]
    out._fusg_zero_pad = True              # (this very object: its padding channels were zero-filled just now)
    return out


def to_nchw(t: torch.Tensor) -> torch.Tensor:
    """Standard-contiguous NCHW copy (module outputs handed back to the caller)."""
    out = torch.empty(t.shape, device=t.device, dtype=torch.float32)
    return copy4d(t, out, 0)


# ---------------------------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------------------------
_WS = {}


_COUNTERS = {}
N_COUNTERS = 4096


def _splitk_counters(device) -> torch.Tensor:
    """Zeroed arrival counters of the in-launch split-K combine (fusg_conv_desc.splitk_counters), one array per device
    and stream: launches on one stream run in order and each leaves its counters zero."""
    key = (str(device), stream_ptr())
    c = _COUNTERS.get(key)
    if c is None:
        c = _COUNTERS[key] = torch.zeros(N_COUNTERS, device=device, dtype=torch.int32)
    if RECORDER is not None:
        RECORDER.keep.append(c)
    return c


def _workspace(device, nbytes: int) -> torch.Tensor:
    """Stream-ordered split-K scratch, grown on demand (one per device and stream: branches of the crop pass
    run concurrently on their own streams)."""
    key = (str(device), stream_ptr())
    ws = _WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty((max(nbytes, 1 << 22) + 3) // 4, device=device, dtype=torch.float32)
        _WS[key] = ws
    if RECORDER is not None:
        # a recorded pass replays this address: it must outlive a later, larger eager pass that replaces _WS[key]
        # (the old block would go back to the caching allocator and be handed to someone else while the plan still
        # writes split-K partial sums into it)
        RECORDER.keep.append(ws)
    return ws


# Do launches of tap-sparse plans (ConvPlan.tap_sparse: VUnet UpSample 'nearest' / 'conv2d_t') hand their pattern to the library,
# i.e. run the halo kernel's tap-skipping instantiations?  Same bytes either way.  Off by default: the sparse launches have not
# been timed against the dense ones yet (tools/upmodes_time.py), and an unmeasured kernel does not become the
# default route.  FUSG_TAP_SPARSE=1 (read at import) or `ops.TAP_SPARSE_LAUNCH = True` turns them on; ops.conv(tap_sparse=...)
# decides per launch.
TAP_SPARSE_LAUNCH = _os.environ.get("FUSG_TAP_SPARSE", "0") == "1"


def _conv_desc(plan: ConvPlan, x0: torch.Tensor, x1: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None,
               out_c_off: int = 0, res0: Optional[torch.Tensor] = None, res1: Optional[torch.Tensor] = None,
               pre_op: int = L.PRE_NONE, pre: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, pre_bstride: int = 0,
               act: int = L.ACT_NONE, store: int = L.STORE_NORMAL, nchw_out: bool = False, tile: int = L.TILE_AUTO,
               ksplit: int = 0, precision: Optional[str] = None, want_stats: bool = False,
               out_stride: int = 1, out_off: Tuple[int, int] = (0, 0), tiles: Optional[torch.Tensor] = None,
               q_window: Optional[Tuple[int, int, int, int]] = None, q_size: Optional[Tuple[int, int]] = None,
               tap_sparse: Optional[int] = None):
    """The fusg_conv_desc of an ops.conv launch before planning -> (desc, out).  Takes CPU tensors too (no launch, no
    torch.cuda call when a `status_scope` is open): tests describe launches to fusg_conv2d_route this way."""
    plan.to(x0.device)
    if RECORDER is not None:
        RECORDER.keep.append(plan.dev)             # packed weights / tables the recorded launch points into
        if pre is not None:
            RECORDER.keep.append(pre)
    b, c0, h, w = x0.shape
    assert c0 == plan.c_split[0], (x0.shape, plan.c_split)
    if len(plan.c_split) > 1:
        assert x1 is not None and x1.shape[1] == plan.c_split[1] and x1.shape[0] == b and x1.shape[2:] == x0.shape[2:], \
            (x0.shape, None if x1 is None else x1.shape, plan.c_split)
    else:
        assert x1 is None
    qh, qw = plan.out_hw(h, w)
    if q_size is not None:
        assert out is not None and plan.nphase == 1 and plan.pad_mode == L.PAD_ZERO and q_window is None
        qh, qw = int(q_size[0]), int(q_size[1])
    if q_window is not None:
        assert out is not None and plan.nphase == 1 and store == L.STORE_NORMAL
        assert 0 <= q_window[0] and q_window[0] + q_window[2] <= qh and 0 <= q_window[1] and q_window[1] + q_window[3] <= qw
    if plan.nphase == 4:
        oc, oh, ow = plan.cout, 2 * qh, 2 * qw
    elif store == L.STORE_D2S:
        oc, oh, ow = plan.cout // 4, 2 * qh, 2 * qw
    elif store == L.STORE_S2D:
        oc, oh, ow = plan.cout * 4, qh // 2, qw // 2
    else:
        oc, oh, ow = plan.cout, qh, qw
    if out is None:
        out = torch.empty((b, oc, oh, ow), device=x0.device, dtype=torch.float32) if nchw_out \
            else nhwc_empty(b, oc, oh, ow, x0.device)
    d = L.ConvDesc()
    d.src0 = desc(x0)
    d.src1 = desc(x1)
    d.dst = desc(out)
    d.res0 = desc(res0)
    d.res1 = desc(res1)
    dev = plan.dev
    prec_name = precision or PRECISION
    if prec_name in _EMU_BITS:                # reduced-precision evidence path: weights rounded like the activations
        key = "wpack_r%d" % _EMU_BITS[prec_name]
        if key not in dev:
            dev[key] = _round_sig_bits(dev["wpack"], _EMU_BITS[prec_name])
        d.wpack = dev[key].data_ptr()
    else:
        d.wpack = dev["wpack"].data_ptr()
    d.bias = dev["bias"].data_ptr()
    d.ktab = dev["ktab"].data_ptr()
    if pre is not None:
        d.pre_scale = pre[0].data_ptr()
        d.pre_shift = pre[1].data_ptr()
        d.pre_bstride = int(pre_bstride)
    d.k_pad, d.c0k, d.cout, d.cout_pad = plan.k_pad, plan.c0k, plan.cout, plan.cout_pad
    d.stride, d.upsample, d.pad_mode = plan.stride, plan.upsample, plan.pad_mode
    d.pre_op, d.act, d.store_mode = int(pre_op), int(act), int(store)
    if q_window is not None:
        d.q_oy, d.q_ox, qh, qw = (int(v) for v in q_window)
    d.qh, d.qw, d.nphase = qh, qw, plan.nphase
    if plan.nphase == 4:
        d.out_sy = d.out_sx = 2
        for ph in range(4):
            d.out_oy[ph] = ph >> 1
            d.out_ox[ph] = ph & 1
    else:
        assert out_stride == 1 or (out is not None and store == L.STORE_NORMAL)
        d.out_sy = d.out_sx = int(out_stride)
        d.out_oy[0], d.out_ox[0] = int(out_off[0]), int(out_off[1])
    if tiles is not None:
        assert tiles.dtype == torch.int32 and tiles.is_contiguous() and tiles.device == x0.device
        d.tile_list, d.tile_count = tiles.data_ptr(), int(tiles.numel())
    d.dst_c_off = int(out_c_off)
    d.tap_sparse = int((plan.tap_sparse if TAP_SPARSE_LAUNCH else 0) if tap_sparse is None else tap_sparse)
    d.tile, d.ksplit = int(tile), int(ksplit)
    d.precision = _PREC[precision or PRECISION]
    d.wpack_h = dev["wpack_h"].data_ptr()
    d.wscale = dev["wscale"].data_ptr()
    d.status = status_word(x0.device).data_ptr()
    if plan.nphase == 1:                      # dense kh x kw tap grid: lets the library pick the halo-tiled kernel
        d.kh, d.kw, d.dil = plan.kh, plan.kw, plan.dil
        d.pad_h, d.pad_w = plan.pad, (plan.pad if plan.pad_w < 0 else plan.pad_w)
        if dev.get("wfrag") is not None:
            d.wfrag = dev["wfrag"].data_ptr()
            d.wfrag_order = dev["wfrag_order"]
            if prec_name == "bf16" and dev.get("wfrag_bf16") is not None:
                d.wfrag_bf16 = dev["wfrag_bf16"].data_ptr()
            if prec_name == "f32" and dev["wfrag_order"] in (0, 1, 2) and not _env_set("FUSG_NO_F32_HALO"):
                ff = plan.frag_f32_dev()                  # exact-fp32 halo kernel (built on first use)
                if ff is not None:
                    d.wfrag_f32 = ff.data_ptr()
                    if RECORDER is not None:
                        RECORDER.keep.append(ff)
    return d, out


def conv(plan: ConvPlan, x0: torch.Tensor, x1: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None,
         out_c_off: int = 0, res0: Optional[torch.Tensor] = None, res1: Optional[torch.Tensor] = None,
         pre_op: int = L.PRE_NONE, pre: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, pre_bstride: int = 0,
         act: int = L.ACT_NONE, store: int = L.STORE_NORMAL, nchw_out: bool = False, tile: int = L.TILE_AUTO,
         ksplit: int = 0, precision: Optional[str] = None, want_stats: bool = False,
         out_stride: int = 1, out_off: Tuple[int, int] = (0, 0), tiles: Optional[torch.Tensor] = None,
         q_window: Optional[Tuple[int, int, int, int]] = None, q_size: Optional[Tuple[int, int]] = None,
         stats_into: Optional[Tuple[torch.Tensor, int]] = None, tap_sparse: Optional[int] = None, stats_d2s: bool = False):
    """One fused convolution launch (fusg_conv2d).  Returns the output tensor (allocated NHWC-physical
    unless `out` is given or `nchw_out` asks for a standard-contiguous NCHW result).
    out_stride / out_off: write output pixel (qy, qx) at (qy*out_stride + out_off[0], qx*out_stride + out_off[1])
    of `out` (phase launches).  tiles: int32 device tensor of 8x16-pixel patch indices - compute only those
    (halo-kernel launches only).  q_window = (oy, ox, h, w): compute only that window of the output grid (into the
    same positions of `out`, which must be given).  q_size = (qh, qw): output grid of a launch whose padding is not
    symmetric (transposed-conv phases; zero padding only).  stats_into = (buffer [B, slots, cout, 2], first_slot): write
    this launch's fused statistics slots there (the launch must qualify).  tap_sparse: the fusg_conv_desc.tap_sparse pattern
    of this launch (0 runs a tap-sparse plan's weights dense: same bytes); None: the plan's if TAP_SPARSE_LAUNCH, else 0.
    stats_d2s: with want_stats, a DepthToSpace launch may fuse its statistics too - the slots are then per STACKED column
    ([B, slots, plan.cout = 4 C, 2]: the same multiset of values per image, which is all LayerNorm needs; conv_up2 asks for it)."""
    d, out = _conv_desc(plan, x0, x1, out=out, out_c_off=out_c_off, res0=res0, res1=res1, pre_op=pre_op, pre=pre,
                        pre_bstride=pre_bstride, act=act, store=store, nchw_out=nchw_out, tile=tile, ksplit=ksplit,
                        precision=precision, want_stats=want_stats, out_stride=out_stride, out_off=out_off, tiles=tiles,
                        q_window=q_window, q_size=q_size, tap_sparse=tap_sparse)
    b, qh, qw = x0.shape[0], d.qh, d.qw
    lib = L.lib()
    nbytes = lib.fusg_conv2d_plan(C.byref(d))
    ws = None
    if nbytes > 0:
        ws = _workspace(x0.device, nbytes)
        d.workspace = ws.data_ptr()
        # In-launch combine by the last-arriving workgroup (fusg_conv_desc.splitk_counters): correct and bit-identical,
        # but measured SLOWER than the separate reduce kernel on this chip (B=1 replay 2.6 -> 3.3 ms/pass, B=32 conv time
        # 26.4 -> 27.1 ms/step): every split workgroup pays an agent-scope release (an L2 write-back) that costs more
        # than the kernel boundary it saves - as cdna_hip_programming.md §5.6 predicts for seams of this size.  Opt-in.
        if _env_set("FUSG_SPLITK_IN_LAUNCH"):
            d.splitk_counters = _splitk_counters(x0.device).data_ptr()
            d.splitk_counters_len = N_COUNTERS
    stats = None
    if want_stats:
        # fused norm statistics when the launch qualifies (include/fusg.h, stats_out: no tile list, no window origin
        # either); else the caller falls back to the separate streaming pass
        # (a DepthToSpace store only moves the stores; its 16-byte epilogue needs cout/4 % 4 == 0)
        if (d.ksplit <= 1 and plan.nphase == 1 and (store == L.STORE_NORMAL or (stats_d2s and store == L.STORE_D2S and plan.cout % 16 == 0))
                and act == L.ACT_NONE and res0 is None
                and res1 is None and (qh * qw) % 32 == 0 and plan.cout % 4 == 0 and out_c_off % 4 == 0 and is_nhwc(out)
                and out.stride(3) % 4 == 0 and not _env_set("FUSG_NO_VEC_EPI") and q_window is None and tiles is None):
            stats = torch.empty((b, qh * qw // 32, plan.cout, 2), device=x0.device, dtype=torch.float32)
            d.stats_out = stats.data_ptr()
    if stats_into is not None:
        buf, first = stats_into
        assert store == L.STORE_NORMAL                # (slots of a DepthToSpace launch are per stacked column: want_stats + stats_d2s)
        assert buf.dtype == torch.float32 and buf.is_contiguous() and buf.shape[0] == b and buf.shape[2] == plan.cout
        assert (qh * qw) % 32 == 0 and first + qh * qw // 32 <= buf.shape[1]
        d.stats_out = buf.data_ptr() + first * plan.cout * 2 * 4
        d.stats_slots = int(buf.shape[1])
    L.check(lib.fusg_conv2d(C.byref(d), stream_ptr()), "conv2d")
    return (out, stats) if want_stats else out


def bottleneck_ok(p: dict, x: torch.Tensor, precision: Optional[str] = None) -> bool:
    """Can this hourglass Bottleneck (packed plans c1, c2, c3 + bn1 affine) run as ONE launch (fusg_hg_bottleneck)?
    planes 64 or 128, split-fp16 or (round 4) exact-fp32 arithmetic, channels of x a multiple of 32.  FUSG_NO_BNECK=1 keeps the
    three launches (FUSG_NO_BNECK_F32=1: only for f32); FUSG_BNECK_MAXHW=n fuses only levels of at most n x n pixels."""
    prec = precision or PRECISION
    if prec not in ("f16x3", "f32") or _env_set("FUSG_NO_BNECK") or (prec == "f32" and (_env_set("FUSG_NO_BNECK_F32") or _env_set("FUSG_NO_F32_HALO"))):
        return False
    c1, c2, c3 = p["c1"], p["c2"], p["c3"]
    if not (c1.cout in (64, 128) and c2.cout == c1.cout and c3.cout == 2 * c1.cout and c1.kh == 1 and c2.kh == 3 and c3.kh == 1
            and c1.c0k == x.shape[1] and x.shape[1] % 32 == 0 and c1.c1k == 0 and c2.pad == 1 and c2.stride == 1):
        return False
    lim = _os.environ.get("FUSG_BNECK_MAXHW")
    if lim is not None and max(x.shape[2], x.shape[3]) > int(lim):
        return False
    # Levels below a minimum size run as three launches (small-image kernel at 4 x 4 / 8 x 8, halo kernel at 16 x 16) instead of the
    # fused block, whose grid there is one workgroup per image walking 48 K-steps in series.  Measured (profiles/
    # r04_ab_experiments.txt [r04j], recorded-plan replay): with at most 8 images the three launches win - B = 8 1266 -> 1305
    # crops/s, B = 1 2.10 -> 2.03 ms per pass with levels < 32 unfused - from B = 16 up the fused block wins (B = 32: conv 23.5 ->
    # 23.8 ms).  FUSG_BNECK_MINHW=n overrides (0 = always fused).  (The fused block and the three launches sum in different
    # orders: the batch that decides is the routing batch when one is set.)
    minhw = BNECK_MINHW if BNECK_MINHW is not None else (32 if _route_n(x.shape[0]) <= 8 and prec == "f16x3" else 0)
    return max(x.shape[2], x.shape[3]) >= minhw or _env_set("FUSG_NO_SMALL")


BNECK_MINHW = int(_os.environ["FUSG_BNECK_MINHW"]) if "FUSG_BNECK_MINHW" in _os.environ else None


def bottleneck(p: dict, x: torch.Tensor, res: Optional[torch.Tensor] = None, precision: Optional[str] = None) -> torch.Tensor:
    """res + conv3(relu(conv2(relu(conv1(relu(bn1(x))))))) in one launch (fusg_hg_bottleneck; stacked_hourglass/
    models.py:22-42).  `p`: the packed Bottleneck (pre = bn1 scale / shift, c1 / c2 with bn2 / bn3 folded, c3);
    `res` defaults to x (no downsample conv).  precision "f32": the exact-fp32 form of the block (fp32 fragment copies)."""
    f32 = (precision or PRECISION) == "f32"
    res = x if res is None else res
    b, _, h, w = x.shape
    planes = p["c1"].cout
    out = nhwc_empty(b, 2 * planes, h, w, x.device)
    d = L.BneckDesc()
    d.x, d.res, d.dst = desc(x), desc(res), desc(out)
    d.pre_scale, d.pre_shift = p["pre"][0].data_ptr(), p["pre"][1].data_ptr()
    if RECORDER is not None:
        RECORDER.keep.append(p["pre"])
    for i, key in ((1, "c1"), (2, "c2"), (3, "c3")):
        plan = p[key].to(x.device)
        dev = plan.dev
        if RECORDER is not None:
            RECORDER.keep.append(dev)
        assert dev.get("wfrag") is not None and dev["wfrag_order"] == 0, key
        frag = plan.frag_f32_dev() if f32 else dev["wfrag"]
        assert frag is not None, key
        if RECORDER is not None:
            RECORDER.keep.append(frag)
        setattr(d, "w%dfrag" % i, frag.data_ptr())
        setattr(d, "bias%d" % i, dev["bias"].data_ptr())
        setattr(d, "wscale%d" % i, dev["wscale"].data_ptr())
    d.status = status_word(x.device).data_ptr()
    d.planes = planes
    d.exact_f32 = 1 if f32 else 0
    L.check(L.lib().fusg_hg_bottleneck(C.byref(d), stream_ptr()), "hg_bottleneck")
    return out


VU_RESPAIR = not _env_set("FUSG_NO_RESPAIR")      # the VUnet's 32-channel Residual pairs as one launch each (tests flip it)


def respair_ok(res_a: ConvPlan, res_b: ConvPlan, nin_b: ConvPlan, nin_c: ConvPlan, x: torch.Tensor,
               nin_in: Optional[ConvPlan] = None, precision: Optional[str] = None) -> bool:
    """Can two Residuals (3x3 plans res_a, res_b), the skip NiNs of their outputs (nin_b, nin_c) and, in the entry form, the
    few-channel NiN in front (nin_in, x = its input) run as ONE launch (fusg_vunet_respair)?  Split-fp16 only, 32 channels,
    k3 pad 1 stride 1 from a single source, and only where fusg_conv2d would run every launch of the block on the halo
    kernel (H % 8 == 0, W % 16 == 0, a grid large enough not to be split over K) and the entry NiN on the pointwise kernel:
    the fused launch then writes their bytes.  Anything else runs unfused; so does everything with VU_RESPAIR off
    (FUSG_NO_RESPAIR=1 at import)."""
    prec = precision or PRECISION
    if not VU_RESPAIR or prec != "f16x3" or not is_nhwc(x):
        return False
    for p in (res_a, res_b):
        if not (p.cout == 32 and p.cout_pad == 32 and p.c0k == 32 and p.c1k == 0 and p.kh == 3 and p.kw == 3 and p.pad == 1
                and p.pad_w < 0 and p.stride == 1 and p.dil == 1 and p.upsample == 0 and p.nphase == 1 and p.pad_mode == L.PAD_ZERO):
            return False
    for p in (nin_b, nin_c):
        if not (p.cout == 32 and p.cout_pad == 32 and p.c0k == 32 and p.c1k == 0 and p.kh == 1 and p.kw == 1 and p.pad == 0
                and p.stride == 1 and p.nphase == 1):
            return False
    b, c, h, w = x.shape
    if nin_in is not None:
        if not (nin_in.cout == 32 and nin_in.cout_pad == 32 and nin_in.c0k in (4, 8) and nin_in.c1k == 0 and nin_in.kh == 1
                and nin_in.kw == 1 and nin_in.pad == 0 and nin_in.stride == 1 and nin_in.nphase == 1 and c == nin_in.c_split[0]):
            return False
    elif c != 32:
        return False
    # The fused launch sums as the HALO kernel does.  The router is asked what each launch it replaces would run on: small
    # grids get a generic split-K launch (another order of summation), tiny images the small-image kernel - those stay unfused.
    # The answer depends on the shapes and on the switches the router reads per call: asked once per such key.
    key = (id(res_b), id(nin_b), id(nin_c), id(nin_in), b, c, h, w, x.stride(3), str(x.device), ROUTE_BATCH,
           _env_set("FUSG_NO_SMALL"), _env_set("FUSG_NO_POINTWISE"), _env_set("FUSG_SMALL_KSPLIT"))
    memo = res_a.__dict__.setdefault("_respair_routes", {})
    if key not in memo:
        t32 = x if nin_in is None else nhwc_empty(b, 32, h, w, x.device)   # stands in for x0 / s0 / s1 (no launch reads it)
        asks = [(res_a, t32, t32, 2), (res_b, t32, t32, 2), (nin_b, t32, None, 2), (nin_c, t32, None, 2)]
        if nin_in is not None:
            asks.append((nin_in, x, None, 7))
        ok = True
        for plan, src, res, family in asks:
            d, _ = _conv_desc(plan, src, pre_op=L.PRE_ELU, res0=res, out=t32, precision=prec)
            L.lib().fusg_conv2d_plan(C.byref(d))
            ok = ok and L.lib().fusg_conv2d_route(C.byref(d)) == family
        memo[key] = ok
    return memo[key]


def respair(res_a: ConvPlan, res_b: ConvPlan, nin_b: ConvPlan, nin_c: ConvPlan, x: torch.Tensor,
            nin_in: Optional[ConvPlan] = None, tap_order: int = 0):
    """(s1, kb, kc) of  x0 = nin_in(elu(x)) or x;  s0 = res_a(elu(x0)) + x0;  s1 = res_b(elu(s0)) + s0;  kb = nin_b(elu(s0));
    kc = nin_c(elu(s1))  in one launch (fusg_vunet_respair) - the bytes of the five (four) `conv` launches it replaces.
    tap_order: 0 = the summation order fusg_conv2d gives those launches at this grid size, 1 = taps in order (large grids),
    2 = K split over the waves (small grids)."""
    b, _, h, w = x.shape
    s1, kb, kc = (nhwc_empty(b, 32, h, w, x.device) for _ in range(3))
    d = L.RespairDesc()
    d.x, d.s1, d.kb, d.kc = desc(x), desc(s1), desc(kb), desc(kc)
    for key, plan in (("A", res_a), ("B", res_b), ("_b", nin_b), ("_c", nin_c)):
        dev = plan.to(x.device).dev
        if RECORDER is not None:
            RECORDER.keep.append(dev)
        assert dev.get("wfrag") is not None and dev["wfrag_order"] == 0, key
        setattr(d, "wfrag" + key, dev["wfrag"].data_ptr())
        setattr(d, "bias" + key, dev["bias"].data_ptr())
        setattr(d, "wscale" + key, dev["wscale"].data_ptr())
    if nin_in is not None:
        dev = nin_in.to(x.device).dev
        if RECORDER is not None:
            RECORDER.keep.append(dev)
        d.w_in, d.bias_in = dev["wpack"].data_ptr(), dev["bias"].data_ptr()
        d.entry, d.cin, d.kpad_in = 1, nin_in.c0k, nin_in.k_pad
    d.status = status_word(x.device).data_ptr()
    d.channels = 32
    d.tap_order = int(tap_order)
    L.check(L.lib().fusg_vunet_respair(C.byref(d), stream_ptr()), "vunet_respair")
    return s1, kb, kc


VU_ENTRY_NIN = not _env_set("FUSG_NO_ENTRY_NIN")  # the VUnet's 6 -> 128 entry NiN inside the Residual that reads it (tests flip it)


def _entry_nin_descs(nin: ConvPlan, res: ConvPlan, u: torch.Tensor, out: torch.Tensor, precision: Optional[str] = None,
                     ksplit: int = 0, plan: bool = True):
    """The two descriptors fusg_conv2d_entry_nin takes: the NiN's on u and the Residual's.  x0 = nin(elu(u)) is never
    materialised: `out`, which has its shape, stands in as the Residual's source (the library ignores src0 / res0 there)."""
    dn, _ = _conv_desc(nin, u, pre_op=L.PRE_ELU, out=out, precision=precision)
    dr, _ = _conv_desc(res, out, pre_op=L.PRE_ELU, out=out, precision=precision, ksplit=ksplit)
    for d in (dn, dr) if plan else ():
        L.lib().fusg_conv2d_plan(C.byref(d))
    return dr, dn


def entry_nin_form(nin: ConvPlan, res: ConvPlan, u: torch.Tensor, precision: Optional[str] = None, ksplit: int = 0) -> int:
    """Which form of the halo kernel would run  res(elu(x0)) + x0,  x0 = nin(elu(u)),  as ONE launch (fusg_conv2d_entry_nin_route):
    0 none - the pair stays two launches -, 1 the 128-column tile with the M split over the waves, 2 the 32-column tile with the K
    split over the waves.  Fuses only in f16x3 on NHWC tensors, where the NiN is a k1 launch from at most 8 channels that
    fusg_conv2d would put on the pointwise kernel and the Residual a single-source k3 s1 p1 zero-padded launch from the NiN's 128
    channels that it would put on the halo kernel in one of those two forms - the fused launch then writes their bytes.  f32, bf16
    and the range guard's fp32 redo keep the two launches.  ksplit: the Residual's, as ops.conv takes it (0: planned - small grids
    then get a generic split-K launch and stay unfused).  Asked once per shape and per the switches the router reads per call."""
    prec = precision or PRECISION
    if prec != "f16x3" or not is_nhwc(u):
        return 0
    if not (nin.kh == 1 and nin.kw == 1 and nin.nphase == 1 and nin.c1k == 0 and nin.c0k <= 8 and res.kh == 3 and res.kw == 3
            and res.nphase == 1 and res.c1k == 0 and res.c0k == nin.cout and res.cout == nin.cout and u.shape[1] == nin.c_split[0]):
        return 0
    b, c, h, w = u.shape
    key = (id(nin), b, c, h, w, u.stride(3), str(u.device), int(ksplit), ROUTE_BATCH,
           _env_set("FUSG_NO_SMALL"), _env_set("FUSG_NO_POINTWISE"), _env_set("FUSG_SMALL_KSPLIT"))
    memo = res.__dict__.setdefault("_entry_nin_routes", {})
    if key not in memo:
        # x0 / the output stand in as one 8 x 16 image whose descriptors are stretched to the real extents: the route reads
        # shapes only, and a real stand-in would be a 1 GB allocation at B = 32
        t = nhwc_empty(1, res.cout, 8, 16, u.device)
        dr, dn = _entry_nin_descs(nin, res, u, t, prec, ksplit=ksplit, plan=False)
        for tt in (dr.src0, dr.dst):
            tt.n, tt.h, tt.w, tt.sh, tt.sn = b, h, w, w * tt.sw, h * w * tt.sw
        dr.qh, dr.qw = res.out_hw(h, w)
        for d in (dn, dr):
            L.lib().fusg_conv2d_plan(C.byref(d))
        memo[key] = max(0, int(L.lib().fusg_conv2d_entry_nin_route(C.byref(dr), C.byref(dn))))
    return memo[key]


def entry_nin_ok(nin: ConvPlan, res: ConvPlan, u: torch.Tensor, precision: Optional[str] = None) -> bool:
    """Does `entry_nin` apply (see entry_nin_form)?  False with VU_ENTRY_NIN off (FUSG_NO_ENTRY_NIN=1 at import)."""
    return VU_ENTRY_NIN and entry_nin_form(nin, res, u, precision) != 0


def entry_nin(nin: ConvPlan, res: ConvPlan, u: torch.Tensor, out: Optional[torch.Tensor] = None, ksplit: int = 0) -> torch.Tensor:
    """res(elu(x0)) + x0  with  x0 = nin(elu(u))  in one halo launch (fusg_conv2d_entry_nin) - the bytes of the two `conv`
    launches it replaces; x0 is computed in the staging and never written.  Raises where entry_nin_form is 0."""
    b, _, h, w = u.shape
    if out is None:
        out = nhwc_empty(b, res.cout, h, w, u.device)
    dr, dn = _entry_nin_descs(nin, res, u, out, ksplit=ksplit)
    L.check(L.lib().fusg_conv2d_entry_nin(C.byref(dr), C.byref(dn), stream_ptr()), "conv2d_entry_nin")
    return out


HG_HEAD = not _env_set("FUSG_NO_HG_HEAD")         # the 1x1 head of an hourglass stack (fc, score, join) as one launch (tests flip it)


def _k1(p: ConvPlan, c0k: int, c1k: int) -> bool:
    return (p.kh == 1 and p.kw == 1 and p.pad == 0 and p.stride == 1 and p.dil == 1 and p.upsample == 0 and p.nphase == 1
            and p.c0k == c0k and p.c1k == c1k)


def hg_head_ok(fc: ConvPlan, score: ConvPlan, y_in: torch.Tensor, join: Optional[ConvPlan] = None,
               x: Optional[torch.Tensor] = None, precision: Optional[str] = None) -> bool:
    """Can  y = relu(fc(y_in));  s = score(y);  x' = x + join(cat[y, s])  (last stack: join None, stops after s) run as ONE launch
    (fusg_hg_head)?  Split-fp16 only, 256 channels, at most 32 classes - in the join form the score plan is the one zero-padded to
    32 output channels, its tensor the join's 32-channel source - and only where fusg_conv2d would run all three launches on the
    halo kernel: the fused launch then writes their bytes.  Small maps, which the small-image kernel takes, and everything else
    stay unfused; so does everything with HG_HEAD off (FUSG_NO_HG_HEAD=1 at import)."""
    prec = precision or PRECISION
    if not HG_HEAD or prec != "f16x3" or not is_nhwc(y_in) or y_in.shape[1] != 256:
        return False
    if not (_k1(fc, 256, 0) and fc.cout == 256 and _k1(score, 256, 0) and 1 <= score.cout <= 32 and score.cout_pad == 32):
        return False
    if join is not None:
        if not (_k1(join, 256, 32) and join.cout == 256 and score.cout == 32 and x is not None and is_nhwc(x)
                and x.shape == y_in.shape):
            return False
    b, c, h, w = y_in.shape
    # The fused launch sums as the HALO kernel does: the router is asked what each launch it replaces would run on (as respair_ok
    # does), once per shape and per the switches the router reads per call.
    key = (id(score), id(join), b, h, w, y_in.stride(3), None if x is None else x.stride(3), str(y_in.device), ROUTE_BATCH,
           _env_set("FUSG_NO_SMALL"), _env_set("FUSG_NO_POINTWISE"), _env_set("FUSG_SMALL_KSPLIT"))
    memo = fc.__dict__.setdefault("_hg_head_routes", {})
    if key not in memo:
        s = nhwc_empty(b, score.cout, h, w, y_in.device)         # stands in for score; y_in for y and the outputs (no launch)
        asks = [_conv_desc(fc, y_in, act=L.ACT_RELU, out=y_in, precision=prec)[0],
                _conv_desc(score, y_in, out=s, precision=prec)[0]]
        if join is not None:
            asks.append(_conv_desc(join, y_in, s[:, :join.c_split[1]], res0=x, out=y_in, precision=prec)[0])
        ok = True
        for d in asks:
            L.lib().fusg_conv2d_plan(C.byref(d))
            ok = ok and L.lib().fusg_conv2d_route(C.byref(d)) == 2
        memo[key] = ok
    return memo[key]


def hg_head(fc: ConvPlan, score: ConvPlan, y_in: torch.Tensor, join: Optional[ConvPlan] = None, x: Optional[torch.Tensor] = None):
    """(s, x') of  y = relu(fc(y_in));  s = score(y);  x' = x + join(cat[y, s])  in one launch (fusg_hg_head) - the bytes of the
    three `conv` launches it replaces; y is never written.  join None (the last stack): (s, None).  In the join form s has the
    score plan's 32 channels, those past the classes exact zeros.  Raises where hg_head_ok is false."""
    b, _, h, w = y_in.shape
    s = nhwc_empty(b, score.cout, h, w, y_in.device)
    out = None if join is None else nhwc_empty(b, join.cout, h, w, y_in.device)
    d = L.HgHeadDesc()
    d.y_in, d.x, d.score, d.dst = desc(y_in), desc(x if join is not None else None), desc(s), desc(out)
    for key, plan in (("fc", fc), ("score", score), ("join", join)):
        if plan is None:
            continue
        dev = plan.to(y_in.device).dev
        if RECORDER is not None:
            RECORDER.keep.append(dev)
        assert dev.get("wfrag") is not None and dev["wfrag_order"] == 0, key
        setattr(d, "wfrag_" + key, dev["wfrag"].data_ptr())
        setattr(d, "bias_" + key, dev["bias"].data_ptr())
        setattr(d, "wscale_" + key, dev["wscale"].data_ptr())
    d.status = status_word(y_in.device).data_ptr()
    d.join = 0 if join is None else 1
    L.check(L.lib().fusg_hg_head(C.byref(d), stream_ptr()), "hg_head")
    return s, out


def last_conv_kernel() -> int:
    """Kernel family of the last conv launch issued by this thread (fusg_last_conv_kernel): 0 generic fp32,
    1 generic split-fp16, 2 halo, 3 halo in parity-quadrant (stride-2) form, 4 tap-unit kernel (few-channel stems),
    5 halo in bf16 mode, 6 fused hourglass Bottleneck, 7 pointwise-from-few-channels streaming kernel, 8 small-image kernel,
    9 halo in exact fp32, 10 tap-unit in exact fp32, 11 tap-unit in bf16 mode, 12 fused VUnet Residual pair (respair),
    13 halo kernel with the entry NiN computed in its staging (entry_nin), 14 fused head of an hourglass stack (hg_head),
    15 halo in single-pass fp16 mode, 16 tap-unit in single-pass fp16 mode."""
    return int(L.lib().fusg_last_conv_kernel())


_BORDER_TILES = {}


def border_tiles(h: int, w: int, device) -> torch.Tensor:
    """Indices of the 8x16-pixel patches of an h x w image that touch its border (row-major patch grid)."""
    key = (h, w, str(device))
    t = _BORDER_TILES.get(key)
    if t is None:
        ny, nx = h // 8, w // 16
        idx = [y * nx + x for y in range(ny) for x in range(nx) if y in (0, ny - 1) or x in (0, nx - 1)]
        t = torch.tensor(idx, dtype=torch.int32, device=device)
        _BORDER_TILES[key] = t
    return t


def up2_phases_ok(x: torch.Tensor, precision: Optional[str] = None) -> bool:
    """Does `conv_up2` take the 4-phase route for this input?  (Any shape the reflect padding itself allows; the
    launches use the halo kernel where they qualify and the generic gather elsewhere.)"""
    b, c, h, w = x.shape
    return h >= 2 and w >= 2 and _os.environ.get("FUSG_NO_UP2_PHASES") is None


def up2_edge_ok(edge, phases, x: torch.Tensor, pre_op: int, ring) -> bool:
    """Does `conv_up2` correct the border ring additively (fusg_up2_edge_fix)?  The single DepthToSpace phase plan, the edge
    taps packed (pack.pack_conv_up2_edge: cin % 32, cout % 16), pre-op NONE or AFFINE_RELU.  FUSG_NO_UP2_EDGE=1, read per call,
    restores the four 25-tap windows."""
    return (edge is not None and isinstance(phases, ConvPlan) and ring is None and not _env_set("FUSG_NO_UP2_EDGE")
            and pre_op in (L.PRE_NONE, L.PRE_AFFINE_RELU) and x.shape[1] == edge.cin and is_nhwc(x))


def up2_edge_fix(edge, x: torch.Tensor, out: torch.Tensor, *, pre_op: int = L.PRE_NONE, pre=None, pre_bstride: int = 0,
                 want_delta: bool = False) -> Optional[torch.Tensor]:
    """out += conv5x5(reflect-padded - replicate-padded up2(f(x))) on the outermost ring, in place (fusg_up2_edge_fix); with
    want_delta returns [B, entries, 2] float64 = per workgroup (sum of the changes, sum of change * (2 old + change))."""
    b, c, h, w = x.shape
    lib = L.lib()
    delta, n = None, 0
    if want_delta:
        n = int(lib.fusg_up2_edge_entries(h, w))
        delta = torch.empty((b, n, 2), device=x.device, dtype=torch.float64)
    if RECORDER is not None:
        RECORDER.keep.append(edge.w)
        if pre is not None:
            RECORDER.keep.append(pre)
    L.check(lib.fusg_up2_edge_fix(C.byref(desc(x)), int(pre_op), pre[0].data_ptr() if pre is not None else None,
                                  pre[1].data_ptr() if pre is not None else None, int(pre_bstride), edge.w.data_ptr(),
                                  C.byref(desc(out)), delta.data_ptr() if delta is not None else None, n, stream_ptr()), "up2_edge_fix")
    return delta


def conv_up2(exact: ConvPlan, phases, x: torch.Tensor, *, pre_op: int = L.PRE_NONE, pre=None, pre_bstride: int = 0,
             precision: Optional[str] = None, ring: Optional[dict] = None, edge=None, ln=None):
    """nn.Upsample(2) -> ReflectionPad2d(2) -> 5x5 conv.  `exact` = the 25-tap plan with the upsample fused into its
    gather (pack_conv(..., upsample=1)); `phases` = pack_conv_up2_d2s (one launch) or pack_conv_up2_phases (four) of the same filter.  When the shapes qualify,
    four 3x3 phase launches on the low-res input (9 MACs per output instead of 25) write the interleaved output; the
    outermost ring of pixels, the only place where the phase form and the reflect-padded 25-tap form differ
    (pack.up2_phase_weights), is then rewritten: by four one-pixel-wide windows of the 25-tap form, or - with `ring`
    (pack.pack_conv_up2_ring) - by twelve small 3x3 launches whose weights are regrouped for the border (9 MACs there
    too).  Measured (round 3, same card): the twelve launches, eight of them 32 - 4000 output pixels small, cost as much as the
    four efficient 25-tap windows (conv 23.2 vs 23.3 - 23.7 ms per step, 1437 vs 1426 crops/s), so the networks do not
    pass `ring` unless FUSG_UP2_RING9 is set.
    `edge` (pack.pack_conv_up2_edge) where up2_edge_ok: the ring is not recomputed at all - the phase form is the convolution
    of the REPLICATE-padded image everywhere, and fusg_up2_edge_fix adds the convolution of (reflect - replicate), which lives
    on the ring and uses the 5 (corner: 9) taps on the padding frame only.
    `ln` = (gamma, beta, eps): also return the ICN LayerNorm's (scale, shift) of the result -> (out, (scale, shift)).  On the
    edge route they come from the phase launch's epilogue slots plus the two sums per workgroup of the ring correction
    (fusg_ln_finalize_slots_delta) where the launch qualifies for fused statistics; else from layernorm_stats."""
    def with_ln(o, ss=None):
        if ln is None:
            return o
        return o, (ss if ss is not None else layernorm_stats(o, ln[0], ln[1], ln[2]))

    if phases is None or not up2_phases_ok(x, precision):
        return with_ln(conv(exact, x, pre_op=pre_op, pre=pre, pre_bstride=pre_bstride, precision=precision))
    b, c, h, w = x.shape
    out = nhwc_empty(b, exact.cout, 2 * h, 2 * w, x.device)
    # split-K launches do not use the halo kernel: keep K whole where the phase launches qualify for it
    halo = (((precision or PRECISION) in ("f16x3", "bf16", "f16") or ((precision or PRECISION) == "f32" and not _env_set("FUSG_NO_F32_HALO")))
            and c % 32 == 0 and h % 8 == 0 and w % 16 == 0 and _os.environ.get("FUSG_NO_HALO") is None)
    if up2_edge_ok(edge, phases, x, pre_op, ring):
        r = conv(phases, x, out=out, store=L.STORE_D2S, pre_op=pre_op, pre=pre, pre_bstride=pre_bstride,
                 precision=precision, ksplit=1 if halo else 0, want_stats=ln is not None, stats_d2s=True)
        stats = r[1] if ln is not None else None
        if ln is None or stats is not None:
            delta = up2_edge_fix(edge, x, out, pre_op=pre_op, pre=pre, pre_bstride=pre_bstride, want_delta=stats is not None)
            if ln is None:
                return out
            nslots, cols = stats.shape[1], stats.shape[2]
            ss = torch.empty((2, b, exact.cout), device=x.device, dtype=torch.float32)
            L.check(L.lib().fusg_ln_finalize_slots_delta(stats.data_ptr(), b, nslots, cols, exact.cout, float(ln[2]), ln[0].data_ptr(),
                                                         ln[1].data_ptr(), delta.data_ptr(), delta.shape[1], ss[0].data_ptr(),
                                                         ss[1].data_ptr(), stream_ptr()), "ln_finalize_slots_delta")
            return out, (ss[0], ss[1])
        # the phase launch does not qualify for fused statistics (split K, qh*qw % 32): today's windows and streamed statistics
    elif isinstance(phases, ConvPlan):                             # all four phases in one launch, DepthToSpace store
        conv(phases, x, out=out, store=L.STORE_D2S, pre_op=pre_op, pre=pre, pre_bstride=pre_bstride,
             precision=precision, ksplit=1 if halo else 0)
    else:
        for ph, plan in enumerate(phases):
            conv(plan, x, out=out, out_stride=2, out_off=(ph >> 1, ph & 1), pre_op=pre_op, pre=pre,
                 pre_bstride=pre_bstride, precision=precision, ksplit=1 if halo else 0)
    if ring is not None:
        from .pack import up2_ring_launches
        for ry, rx, win, off in up2_ring_launches(h, w):
            if win[2] > 0 and win[3] > 0:
                conv(ring[(ry, rx)], x, out=out, q_window=win, out_stride=2, out_off=off, pre_op=pre_op, pre=pre,
                     pre_bstride=pre_bstride, precision=precision)
        return with_ln(out)
    # the outermost ring of output pixels, with the 25-tap form: four one-pixel-wide windows of the full convolution
    for win in ((0, 0, 1, 2 * w), (2 * h - 1, 0, 1, 2 * w), (0, 0, 2 * h, 1), (0, 2 * w - 1, 2 * h, 1)):
        conv(exact, x, out=out, q_window=win, pre_op=pre_op, pre=pre, pre_bstride=pre_bstride, precision=precision)
    return with_ln(out)


def conv_transpose_phases(phases, x: torch.Tensor, *, pre_op: int = L.PRE_NONE, pre=None, pre_bstride: int = 0,
                          act: int = L.ACT_NONE, want_stats: bool = False, precision: Optional[str] = None):
    """nn.ConvTranspose2d(k4, s2, p1) as four dense 2x2 stride-1 launches with strided stores
    (pack.pack_conv_transpose_k4s2p1_phases): each one qualifies for the halo kernel when the input does
    (split-fp16, channels % 32 == 0, H % 8 == 0, W % 16 == 0).  With want_stats the four launches write disjoint
    slot ranges of one statistics buffer: returns (out, stats [B, 4*h*w/32, cout, 2] or None)."""
    b, c, h, w = x.shape
    cout = phases[0].cout
    out = nhwc_empty(b, cout, 2 * h, 2 * w, x.device)
    n = h * w // 32
    fuse = (want_stats and act == L.ACT_NONE and (h * w) % 32 == 0 and cout % 4 == 0
            and _os.environ.get("FUSG_NO_VEC_EPI") is None)
    stats = torch.empty((b, 4 * n, cout, 2), device=x.device, dtype=torch.float32) if fuse else None
    for ph, plan in enumerate(phases):
        conv(plan, x, out=out, out_stride=2, out_off=(ph >> 1, ph & 1), q_size=(h, w), pre_op=pre_op, pre=pre,
             pre_bstride=pre_bstride, act=act, precision=precision, ksplit=1,
             stats_into=(stats, ph * n) if fuse else None)
    return (out, stats) if want_stats else out


def conv_rowsplit(plan: ConvPlan, x0: torch.Tensor, *, pre_op: int = L.PRE_NONE, pre=None, pre_bstride: int = 0,
                  act: int = L.ACT_NONE, nchw_out: bool = True) -> torch.Tensor:
    """Small-cout head (pack.pack_conv_rowsplit): kh x 1 implicit GEMM + horizontal gather-sum."""
    rs = plan.rowsplit
    t = conv(plan, x0, pre_op=pre_op, pre=pre, pre_bstride=pre_bstride)
    b, _, h, w = t.shape
    out = torch.empty((b, rs["cout"], h, w), device=x0.device, dtype=torch.float32) if nchw_out \
        else nhwc_empty(b, rs["cout"], h, w, x0.device)
    L.check(L.lib().fusg_hshift_sum(C.byref(desc(t)), plan.dev["rs_bias"].data_ptr(), rs["kw"], rs["pad"], plan.pad_mode,
                                    int(act), C.byref(desc(out)), stream_ptr()), "hshift_sum")
    return out


# ---------------------------------------------------------------------------------------------
# normalisation
# ---------------------------------------------------------------------------------------------
def _nchunk(b: int, c: int, hw: int) -> int:
    """Partial sums per image of the streamed statistics (their number fixes the order of the sums: by the routing batch)."""
    zg = (c // 4 + 63) // 64
    want = max(1, 1024 // max(1, _route_n(b) * zg))
    return int(max(1, min(want, max(1, hw // 64), 4096)))


def _chan_stats(x: torch.Tensor):
    b, c, h, w = x.shape
    n = _nchunk(b, c, h * w)
    partial = torch.empty((b, n, c, 2), device=x.device, dtype=torch.float32)
    L.check(L.lib().fusg_chan_stats(C.byref(desc(x)), partial.data_ptr(), n, stream_ptr()), "chan_stats")
    return partial, n


def instnorm_stats(x: torch.Tensor, eps: float = 1e-5) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scale, shift) [B, C] such that InstanceNorm2d(x) = x*scale + shift."""
    b, c = x.shape[:2]
    partial, n = _chan_stats(x)
    ss = torch.empty((2, b, c), device=x.device, dtype=torch.float32)
    L.check(L.lib().fusg_in_finalize(C.byref(desc(x)), partial.data_ptr(), n, float(eps), ss[0].data_ptr(),
                                     ss[1].data_ptr(), stream_ptr()), "in_finalize")
    return ss[0], ss[1]


def layernorm_stats(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5):
    """(scale, shift) [B, C] of the ICN's custom LayerNorm (warp_learn/models.py:26-35)."""
    b, c = x.shape[:2]
    partial, n = _chan_stats(x)
    ss = torch.empty((2, b, c), device=x.device, dtype=torch.float32)
    L.check(L.lib().fusg_ln_finalize(C.byref(desc(x)), partial.data_ptr(), n, float(eps), gamma.data_ptr(),
                                     beta.data_ptr(), ss[0].data_ptr(), ss[1].data_ptr(), stream_ptr()), "ln_finalize")
    return ss[0], ss[1]


def conv_in(plan: ConvPlan, x0: torch.Tensor, eps: float = 1e-5, **kw):
    """conv followed by InstanceNorm2d statistics: returns (raw conv output, (scale, shift)).  The statistics
    come out of the conv epilogue when the launch qualifies, else from the streaming pass."""
    if isinstance(plan, (list, tuple)):                               # transposed conv as four phase plans
        out, stats = conv_transpose_phases(plan, x0, want_stats=True, **kw)
    else:
        out, stats = conv(plan, x0, want_stats=True, **kw)
    if stats is None:
        return out, instnorm_stats(out, eps)
    b, nslots, c, _ = stats.shape
    ss = torch.empty((2, b, c), device=out.device, dtype=torch.float32)
    L.check(L.lib().fusg_in_finalize_slots(stats.data_ptr(), b, nslots, c, float(eps), ss[0].data_ptr(), ss[1].data_ptr(),
                                           stream_ptr()), "in_finalize_slots")
    return out, (ss[0], ss[1])


def conv_ln(plan: ConvPlan, x0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, **kw):
    """conv followed by the ICN's custom LayerNorm statistics (see layernorm_stats)."""
    out, stats = conv(plan, x0, want_stats=True, **kw)
    if stats is None:
        return out, layernorm_stats(out, gamma, beta, eps)
    b, nslots, c, _ = stats.shape
    ss = torch.empty((2, b, c), device=out.device, dtype=torch.float32)
    L.check(L.lib().fusg_ln_finalize_slots(stats.data_ptr(), b, nslots, c, float(eps), gamma.data_ptr(), beta.data_ptr(),
                                           ss[0].data_ptr(), ss[1].data_ptr(), stream_ptr()), "ln_finalize_slots")
    return out, (ss[0], ss[1])


def affine_act(x: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor], act: int = L.ACT_NONE,
               res: Optional[torch.Tensor] = None, bstride: Optional[int] = None) -> torch.Tensor:
    b, c, h, w = x.shape
    out = nhwc_empty(b, c, h, w, x.device)
    if bstride is None:
        bstride = c
    L.check(L.lib().fusg_affine_act(C.byref(desc(x)), scale.data_ptr() if scale is not None else None,
                                    shift.data_ptr() if shift is not None else None, int(bstride), int(act),
                                    C.byref(desc(res)) if res is not None else None, C.byref(desc(out)), stream_ptr()),
            "affine_act")
    return out


# ---------------------------------------------------------------------------------------------
# data movement / small ops
# ---------------------------------------------------------------------------------------------
def maxpool2(x: torch.Tensor) -> torch.Tensor:
    b, c, h, w = x.shape
    out = nhwc_empty(b, c, h // 2, w // 2, x.device)
    L.check(L.lib().fusg_maxpool2(C.byref(desc(x)), C.byref(desc(out)), stream_ptr()), "maxpool2")
    return out


def upsample2_add(low: torch.Tensor, up1: torch.Tensor) -> torch.Tensor:
    out = nhwc_empty(*up1.shape, up1.device)
    L.check(L.lib().fusg_upsample2_add(C.byref(desc(low)), C.byref(desc(up1)), C.byref(desc(out)), stream_ptr()),
            "upsample2_add")
    return out


def add4d(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if out is None:
        out = nhwc_empty(*a.shape, a.device)
    L.check(L.lib().fusg_add4d(C.byref(desc(a)), C.byref(desc(b)), C.byref(desc(out)), stream_ptr()), "add4d")
    return out


def space_to_depth2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    b, c, h, w = x.shape
    if out is None:
        out = nhwc_empty(b, 4 * c, h // 2, w // 2, x.device)
    L.check(L.lib().fusg_space_to_depth2(C.byref(desc(x)), C.byref(desc(out)), stream_ptr()), "space_to_depth2")
    return out


def depth_to_space2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    b, c, h, w = x.shape
    if out is None:
        out = nhwc_empty(b, c // 4, 2 * h, 2 * w, x.device)
    L.check(L.lib().fusg_depth_to_space2(C.byref(desc(x)), C.byref(desc(out)), stream_ptr()), "depth_to_space2")
    return out


def ec_inputs(images: torch.Tensor, edges: torch.Tensor, masks: torch.Tensor, mode: int) -> torch.Tensor:
    b, _, h, w = images.shape
    out = nhwc_empty(b, 4, h, w, images.device)
    L.check(L.lib().fusg_ec_inputs(C.byref(desc(images)), C.byref(desc(edges)), C.byref(desc(masks)), C.byref(desc(out)),
                                   int(mode), stream_ptr()), "ec_inputs")
    return out if mode == 1 else out[:, :3]


def argmax_hw(x: torch.Tensor) -> torch.Tensor:
    """int32 [B, C] row-major first-occurrence argmax over H*W."""
    _require_gpu(x)
    b, c = x.shape[:2]
    idx = torch.empty((b, c), device=x.device, dtype=torch.int32)
    L.check(L.lib().fusg_argmax_hw(C.byref(desc(x)), idx.data_ptr(), stream_ptr()), "argmax_hw")
    return idx


def to_image_u8(x: torch.Tensor) -> torch.Tensor:
    """uint8 [B, H, W, C] = trunc(clip((x+1)/2*255)) (to_image without the LAB branch)."""
    _require_gpu(x)
    b, c, h, w = x.shape
    out = torch.empty((b, h, w, c), device=x.device, dtype=torch.uint8)
    L.check(L.lib().fusg_to_image_u8(C.byref(desc(x)), C.byref(desc(out.permute(0, 3, 1, 2))), stream_ptr()), "to_image_u8")
    return out


def merge_u8(out_: torch.Tensor, img: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """uint8 [B, H, W, C] = trunc((out*m + img*(1-m))*255) (trajectory_inference.py:126-129)."""
    b, c, h, w = out_.shape
    dst = torch.empty((b, h, w, c), device=out_.device, dtype=torch.uint8)
    L.check(L.lib().fusg_merge_u8(C.byref(desc(out_)), C.byref(desc(img)), C.byref(desc(mask)),
                                  C.byref(desc(dst.permute(0, 3, 1, 2))), stream_ptr()), "merge_u8")
    return dst


# ---------------------------------------------------------------------------------------------
# EdgeConnect's inputs from a detector mask (csrc/inpaint_inputs.h: create_inpaint_inputs_shape, utils/inpaint_utils.py:35-58)
# ---------------------------------------------------------------------------------------------
INPAINT_KEYS = ("img", "gray", "edge", "mask")


def gauss_table(sigma: float = 2.0) -> Tuple[_np.ndarray, int]:
    """The one-sided Gaussian table Canny's smoothing takes, in numpy float64 exactly as SciPy builds its kernel (radius =
    int(4 sigma + 0.5), exp(-0.5 / sigma^2 * x^2) over -radius..radius divided by its sum): (w[0..radius], radius)."""
    sigma = float(sigma)
    if not sigma > 0.0:
        raise ValueError(f"inpaint_inputs: sigma must be positive, got {sigma}")
    radius = int(4.0 * sigma + 0.5)
    x = _np.arange(-radius, radius + 1)
    phi = _np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return _np.ascontiguousarray(phi[radius:], dtype=_np.float64), radius


def _inpaint_args(frame_shape, frame_dtype, det_shape, det_dtype, boxes, gauss_w, radius, max_box, u8) -> Tuple:
    """What both forms of `inpaint_inputs` check before anything is touched: -> (V, H, W, host boxes or None, table, radius,
    (max_box_h, max_box_w))."""
    if frame_dtype != u8 or len(frame_shape) != 3 or frame_shape[2] != 3:
        raise ValueError(f"inpaint_inputs: frame must be uint8 [H, W, 3], got {frame_dtype} {tuple(frame_shape)}")
    H, W = int(frame_shape[0]), int(frame_shape[1])
    if det_dtype != u8 or len(det_shape) != 4 or tuple(det_shape[1:]) != (1, H, W):
        raise ValueError(f"inpaint_inputs: det_masks must be uint8 [V, 1, {H}, {W}], got {det_dtype} {tuple(det_shape)}")
    V = int(det_shape[0])
    gauss_w = _np.ascontiguousarray(gauss_w, dtype=_np.float64).reshape(-1)
    if radius != gauss_w.shape[0] - 1 or not 0 <= radius <= 32:
        raise ValueError(f"inpaint_inputs: radius {radius} must be the table's length - 1 ({gauss_w.shape[0] - 1}) and at most 32")
    host = None
    if not torch.is_tensor(boxes) or not boxes.is_cuda:
        host = _np.ascontiguousarray(_np.asarray(boxes).reshape(-1, 4), dtype=_np.int64)
        if host.shape[0] != V:
            raise ValueError(f"inpaint_inputs: {host.shape[0]} boxes for {V} detector masks")
        bad = (host[:, 0] < 0) | (host[:, 1] < 0) | (host[:, 2] < host[:, 0]) | (host[:, 3] < host[:, 1]) | (host[:, 2] > W) | (host[:, 3] > H)
        if bad.any():
            v = int(_np.nonzero(bad)[0][0])
            raise ValueError(f"inpaint_inputs: box {v} = {host[v].tolist()} leaves the {W} x {H} frame (x0, y0, x1, y1, half-open)")
        if max_box is None:
            max_box = (int((host[:, 3] - host[:, 1]).max()), int((host[:, 2] - host[:, 0]).max())) if V else (0, 0)
        host = host.astype(_np.int32)
    elif tuple(boxes.shape) != (V, 4) or boxes.dtype != torch.int32:
        raise ValueError(f"inpaint_inputs: device boxes must be int32 [{V}, 4], got {boxes.dtype} {tuple(boxes.shape)}")
    if max_box is None:
        max_box = (H, W)                                          # device boxes nobody has looked at: the frame bounds them
    return V, H, W, host, gauss_w, int(radius), (int(max_box[0]), int(max_box[1]))


def inpaint_inputs(frame: torch.Tensor, det_masks: torch.Tensor, boxes, sigma: float = 2.0, out=None, max_box=None):
    """EdgeConnect's four inputs for V vehicles, built on the device (fusg_inpaint_inputs, five launches on the current
    stream): frame CUDA uint8 [H, W, 3]; det_masks CUDA uint8 [V, 1, H, W], the detector's masks in frame coordinates
    (non-zero = vehicle, read only inside the box); boxes [V, 4] = bbox_new_img (x0, y0, x1, y1, half-open) as a host array
    (checked here, uploaded without a synchronisation) or a device int32 tensor (then max_box = (h, w) bounds the box
    extents; default: the frame).  -> {'img' float32 [V, 3, 256, 256], 'gray', 'edge', 'mask' float32 [V, 1, 256, 256]};
    out: a dict of such buffers (any strides) to write into."""
    _require_gpu(frame, "frame")
    _require_gpu(det_masks, "det_masks")
    gw, radius = gauss_table(sigma)
    V, H, W, host, gw, radius, mb = _inpaint_args(frame.shape, frame.dtype, det_masks.shape, det_masks.dtype, boxes, gw, radius, max_box,
                                                  torch.uint8)
    dev, R = frame.device, 256
    with torch.cuda.device(dev):
        if out is None:
            out = {k: torch.empty((V, 3 if k == "img" else 1, R, R), dtype=torch.float32, device=dev) for k in INPAINT_KEYS}
        for k in INPAINT_KEYS:
            if tuple(out[k].shape) != (V, 3 if k == "img" else 1, R, R) or out[k].dtype != torch.float32 or out[k].device != dev:
                raise ValueError(f"inpaint_inputs: out['{k}'] must be float32 {(V, 3 if k == 'img' else 1, R, R)} on {dev}")
        if V == 0:
            return out
        bx = h2d(host, dev, torch.int32) if host is not None else boxes.contiguous()
        lib = L.lib()
        scratch = torch.empty((int(lib.fusg_inpaint_inputs_scratch_bytes(V, mb[0], mb[1])),), dtype=torch.uint8, device=dev)
        fr, dm = frame.contiguous(), det_masks.contiguous()
        L.check(lib.fusg_inpaint_inputs(C.byref(desc(fr[None].permute(0, 3, 1, 2))), C.byref(desc(dm)), bx.data_ptr(), gw.ctypes.data, radius,
                                        mb[0], mb[1], *(C.byref(desc(out[k])) for k in INPAINT_KEYS), scratch.data_ptr(), stream_ptr()),
                "inpaint_inputs")
    return out


def _np_desc(a: _np.ndarray, dtype: int) -> L.Tensor:
    """fusg_tensor over a 4-D numpy array, logical [n, c, h, w] (strides in elements)."""
    d = L.Tensor()
    d.data = a.ctypes.data
    d.n, d.c, d.h, d.w = a.shape
    d.sn, d.sc, d.sh, d.sw = (s // a.itemsize for s in a.strides)
    d.dtype = dtype
    return d


def inpaint_inputs_host(frame, det_masks, boxes, sigma: float = 2.0, gauss_w=None, radius=None, max_box=None):
    """`inpaint_inputs` on the CPU by the same code (fusg_inpaint_inputs_host; no GPU needed): numpy in (frame uint8
    [H, W, 3], det_masks uint8 [V, 1, H, W], boxes [V, 4]) and out.  gauss_w / radius: a table other than `gauss_table(sigma)`."""
    frame, det_masks = _np.asarray(frame), _np.asarray(det_masks)
    if gauss_w is None:
        gauss_w, r = gauss_table(sigma)
        radius = r if radius is None else radius
    elif radius is None:
        radius = len(gauss_w) - 1
    V, H, W, host, gw, radius, mb = _inpaint_args(frame.shape, frame.dtype, det_masks.shape, det_masks.dtype, _np.asarray(boxes), gauss_w,
                                                  radius, max_box, _np.uint8)
    R = 256
    out = {k: _np.zeros((V, 3 if k == "img" else 1, R, R), dtype=_np.float32) for k in INPAINT_KEYS}
    if V == 0:
        return out
    lib = L.lib()
    fr, dm = _np.ascontiguousarray(frame), _np.ascontiguousarray(det_masks)
    nbytes = int(lib.fusg_inpaint_inputs_scratch_bytes(V, mb[0], mb[1]))
    raw = _np.zeros(nbytes + 16, dtype=_np.uint8)
    off = (-raw.ctypes.data) % 16
    L.check(lib.fusg_inpaint_inputs_host(C.byref(_np_desc(fr[None].transpose(0, 3, 1, 2), L.U8)), C.byref(_np_desc(dm, L.U8)), host.ctypes.data,
                                         gw.ctypes.data, radius, mb[0], mb[1], *(C.byref(_np_desc(out[k], L.F32)) for k in INPAINT_KEYS),
                                         raw.ctypes.data + off), "inpaint_inputs_host")
    return out


# ---- the same from masks in BOX coordinates (fusg_inpaint_inputs_boxed): what a detector run on the box crop returns
def _is_packed_pair(box_masks) -> bool:
    """An already packed (buffer [n], offsets [V]) pair, as opposed to a sequence of per-vehicle pieces."""
    return isinstance(box_masks, tuple) and len(box_masks) == 2 and getattr(box_masks[0], "ndim", 0) == 1 \
        and getattr(box_masks[1], "ndim", 0) == 1


def box_mask_pieces(box_masks, what: str = "inpaint_inputs_boxed"):
    """A sequence of V per-vehicle masks [h_v, w_v] or [1, h_v, w_v] -> (the pieces as 2-D views, their (h, w), int64 offsets
    [V] into their concatenation, is_cuda).  All uint8 or all float32; all CUDA tensors or all host tensors / arrays."""
    pcs = []
    for v, m in enumerate(box_masks):
        m = m if torch.is_tensor(m) else _np.asarray(m)
        if m.ndim == 3 and m.shape[0] == 1:
            m = m[0]
        if m.ndim != 2:
            raise ValueError(f"{what}: box_masks[{v}] must be [h, w] or [1, h, w], got {tuple(m.shape)}")
        pcs.append(m)
    kinds = {(torch.is_tensor(m) and m.is_cuda, str(m.dtype).replace("torch.", "")) for m in pcs}
    if len(kinds) > 1 or (kinds and next(iter(kinds))[1] not in ("uint8", "float32")):
        raise ValueError(f"{what}: box_masks must be all uint8 or all float32, all on the device or all on the host, got {sorted(kinds)}")
    shapes = [(int(m.shape[0]), int(m.shape[1])) for m in pcs]
    offs = _np.zeros(len(pcs), dtype=_np.int64)
    if pcs:
        offs[1:] = _np.cumsum([h * w for h, w in shapes])[:-1]
    return pcs, shapes, offs, bool(kinds) and next(iter(kinds))[0]


def _boxed_check(shapes, offs, n_elems, host, what: str) -> None:
    """With host boxes, before any launch: every piece has its clipped box's shape, every packed mask lies in the buffer."""
    if host is None:
        return
    for v in range(host.shape[0]):
        bh, bw = int(host[v, 3] - host[v, 1]), int(host[v, 2] - host[v, 0])
        if shapes is not None and shapes[v] != (bh, bw):
            raise ValueError(f"{what}: box_masks[{v}] is {shapes[v][0]} x {shapes[v][1]}, its box {host[v].tolist()} is {bh} x {bw} (h x w)")
        if offs is not None and (offs[v] < 0 or offs[v] + bh * bw > n_elems):
            raise ValueError(f"{what}: the {bh} x {bw} mask of box {v} at offset {int(offs[v])} leaves the buffer of {n_elems} elements")


def _boxed_frame_args(frame_shape, frame_dtype, V, boxes, gauss_w, radius, max_box, u8):
    """`_inpaint_args` for V box-coordinate masks: the frame-form checks with a mask shape that passes."""
    H, W = (int(frame_shape[0]), int(frame_shape[1])) if len(frame_shape) == 3 else (0, 0)
    return _inpaint_args(frame_shape, frame_dtype, (V, 1, H, W), u8, boxes, gauss_w, radius, max_box, u8)


def inpaint_inputs_boxed(frame: torch.Tensor, box_masks, boxes, sigma: float = 2.0, out=None, max_box=None):
    """`inpaint_inputs` from the detector's masks in BOX coordinates (fusg_inpaint_inputs_boxed; trajectory_inference.py:113-119,
    :316-324: Mask R-CNN runs on the box crop): box_masks = a sequence of V tensors or arrays [h_v, w_v] or [1, h_v, w_v], h_v x
    w_v = vehicle v's box - all uint8 (non-zero = vehicle, a dilated 255 whitens) or all float32 (binarised m * 255 > 0), all
    CUDA (packed with one `torch.cat`) or all host (packed into one pinned buffer, one asynchronous copy, no synchronisation) -
    or an already packed pair (buffer [n] CUDA uint8 / float32, offsets int64 [V], device or host).  With host boxes a piece
    whose shape is not its box's raises ValueError before any launch; with device boxes a mask that would leave the buffer
    makes its vehicle a zero-extent box (zeros) and is never read.  boxes, sigma, out, max_box and the result: as `inpaint_inputs`."""
    what = "inpaint_inputs_boxed"
    _require_gpu(frame, "frame")
    dev, R = frame.device, 256
    gw, radius = gauss_table(sigma)
    if _is_packed_pair(box_masks):
        buf, offs = box_masks
        if not torch.is_tensor(buf) or not buf.is_cuda or buf.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"{what}: a packed buffer must be a CUDA uint8 or float32 tensor [n]")
        pcs, shapes, V = None, None, int(offs.shape[0])
        offs_host = None if (torch.is_tensor(offs) and offs.is_cuda) else _np.asarray(offs, dtype=_np.int64).reshape(-1)
    else:
        pcs, shapes, offs_host, on_dev = box_mask_pieces(box_masks, what)
        V = len(pcs)
    V, H, W, host, gw, radius, mb = _boxed_frame_args(frame.shape, frame.dtype, V, boxes, gw, radius, max_box, torch.uint8)
    n_elems = int(buf.numel()) if pcs is None else int(sum(h * w for h, w in shapes))
    _boxed_check(shapes, offs_host, n_elems, host, what)
    with torch.cuda.device(dev):
        if out is None:
            out = {k: torch.empty((V, 3 if k == "img" else 1, R, R), dtype=torch.float32, device=dev) for k in INPAINT_KEYS}
        for k in INPAINT_KEYS:
            if tuple(out[k].shape) != (V, 3 if k == "img" else 1, R, R) or out[k].dtype != torch.float32 or out[k].device != dev:
                raise ValueError(f"{what}: out['{k}'] must be float32 {(V, 3 if k == 'img' else 1, R, R)} on {dev}")
        if V == 0:
            return out
        if pcs is not None and on_dev:
            buf = torch.cat([m.reshape(-1) for m in pcs])
        elif pcs is not None:                                     # one pinned staging buffer, one copy
            stage = torch.empty((n_elems,), dtype=torch.uint8 if str(pcs[0].dtype).endswith("uint8") else torch.float32, pin_memory=True)
            view = stage.numpy()
            for m, o, (h, w) in zip(pcs, offs_host, shapes):
                view[o:o + h * w] = (m.numpy() if torch.is_tensor(m) else m).reshape(-1)
            buf = h2d(stage, dev)
        off_d = h2d(offs_host, dev, torch.int64) if offs_host is not None else offs.to(torch.int64).contiguous()
        bx = h2d(host, dev, torch.int32) if host is not None else boxes.contiguous()
        buf = buf.contiguous()
        lib = L.lib()
        scratch = torch.empty((int(lib.fusg_inpaint_inputs_scratch_bytes(V, mb[0], mb[1])),), dtype=torch.uint8, device=dev)
        fr = frame.contiguous()
        L.check(lib.fusg_inpaint_inputs_boxed(C.byref(desc(fr[None].permute(0, 3, 1, 2))), buf.data_ptr(), _DT[buf.dtype], n_elems,
                                              off_d.data_ptr(), bx.data_ptr(), gw.ctypes.data, radius, mb[0], mb[1],
                                              *(C.byref(desc(out[k])) for k in INPAINT_KEYS), scratch.data_ptr(), stream_ptr()), what)
    return out


def inpaint_inputs_boxed_host(frame, box_masks, boxes, sigma: float = 2.0, gauss_w=None, radius=None, max_box=None):
    """`inpaint_inputs_boxed` on the CPU by the same code (fusg_inpaint_inputs_boxed_host; no GPU needed): numpy in (pieces or
    a packed (buffer, offsets) pair) and out.  It sees the offsets: a mask that would leave the buffer is refused (the library's
    FUSG_ERR_INVALID), a piece of the wrong shape raises ValueError."""
    what = "inpaint_inputs_boxed_host"
    frame = _np.asarray(frame)
    if gauss_w is None:
        gauss_w, r = gauss_table(sigma)
        radius = r if radius is None else radius
    elif radius is None:
        radius = len(gauss_w) - 1
    if _is_packed_pair(box_masks):
        buf, offs = _np.ascontiguousarray(box_masks[0]), _np.ascontiguousarray(box_masks[1], dtype=_np.int64)
        if buf.dtype not in (_np.uint8, _np.float32):
            raise ValueError(f"{what}: a packed buffer must be uint8 or float32 [n], got {buf.dtype}")
        shapes = None
    else:
        pcs, shapes, offs, on_dev = box_mask_pieces(box_masks, what)
        if on_dev:
            raise ValueError(f"{what}: box_masks must be host arrays")
        pcs = [m.numpy() if torch.is_tensor(m) else m for m in pcs]
        buf = _np.concatenate([m.reshape(-1) for m in pcs]) if pcs else _np.zeros(0, _np.uint8)
    V = int(offs.shape[0])
    V, H, W, host, gw, radius, mb = _boxed_frame_args(frame.shape, frame.dtype, V, _np.asarray(boxes), gauss_w, radius, max_box, _np.uint8)
    _boxed_check(shapes, None, int(buf.size), host, what)
    R = 256
    out = {k: _np.zeros((V, 3 if k == "img" else 1, R, R), dtype=_np.float32) for k in INPAINT_KEYS}
    if V == 0:
        return out
    lib = L.lib()
    fr = _np.ascontiguousarray(frame)
    nbytes = int(lib.fusg_inpaint_inputs_scratch_bytes(V, mb[0], mb[1]))
    raw = _np.zeros(nbytes + 16, dtype=_np.uint8)
    off = (-raw.ctypes.data) % 16
    L.check(lib.fusg_inpaint_inputs_boxed_host(C.byref(_np_desc(fr[None].transpose(0, 3, 1, 2), L.U8)), buf.ctypes.data,
                                               L.U8 if buf.dtype == _np.uint8 else L.F32, int(buf.size), offs.ctypes.data, host.ctypes.data,
                                               gw.ctypes.data, radius, mb[0], mb[1], *(C.byref(_np_desc(out[k], L.F32)) for k in INPAINT_KEYS),
                                               raw.ctypes.data + off), what)
    return out


# ---------------------------------------------------------------------------------------------
# per-image quality metrics (csrc/metrics.h): SSIM / PSNR / difference counts of uint8 crops, EdgeAccuracy's counts
# ---------------------------------------------------------------------------------------------
IMAGE_METRIC_COLUMNS = ("ssim", "mse", "psnr", "max_abs", "n_diff", "sse")


def _image_pair(a, b, u8, what: str) -> None:
    if a.dtype != u8 or b.dtype != u8 or len(a.shape) != 4 or len(b.shape) != 4:
        raise ValueError(f"{what}: a and b must be uint8 [B, H, W, C], got {a.dtype} {tuple(a.shape)} and {b.dtype} {tuple(b.shape)}")


def image_metrics_u8(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The float64 [B, 6] table (`IMAGE_METRIC_COLUMNS`) of two CUDA uint8 [B, H, W, C] batches of any strides, on the device:
    two launches on the current stream, no host synchronisation (fusg_image_metrics_u8; SSIM as the test oracle defines it)."""
    _require_gpu(a, "a")
    _require_gpu(b, "b")
    _image_pair(a, b, torch.uint8, "image_metrics_u8")
    B, H, W, Cn = a.shape
    with torch.cuda.device(a.device):
        out = torch.empty((B, len(IMAGE_METRIC_COLUMNS)), dtype=torch.float64, device=a.device)
        lib = L.lib()
        nbytes = int(lib.fusg_image_metrics_scratch_bytes(B, H, W, Cn))
        scratch = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=a.device)
        L.check(lib.fusg_image_metrics_u8(C.byref(desc(a.permute(0, 3, 1, 2))), C.byref(desc(b.permute(0, 3, 1, 2))), out.data_ptr(),
                                          scratch.data_ptr(), stream_ptr()), "image_metrics_u8")
        if RECORDER is not None:
            RECORDER.keep.append(scratch)
    return out


def image_metrics_host(a, b) -> _np.ndarray:
    """`image_metrics_u8` on the CPU by the same code in the same order of sums (fusg_image_metrics_host; no GPU needed):
    numpy uint8 [B, H, W, C] in, float64 [B, 6] out."""
    a, b = _np.asarray(a), _np.asarray(b)
    _image_pair(a, b, _np.uint8, "image_metrics_host")
    out = _np.zeros((a.shape[0], len(IMAGE_METRIC_COLUMNS)), dtype=_np.float64)
    L.check(L.lib().fusg_image_metrics_host(C.byref(_np_desc(a.transpose(0, 3, 1, 2), L.U8)), C.byref(_np_desc(b.transpose(0, 3, 1, 2), L.U8)),
                                            out.ctypes.data), "image_metrics_host")
    return out


def _edge_pair(x, y, f32, what: str) -> None:
    if x.dtype != f32 or y.dtype != f32 or len(x.shape) != 4 or len(y.shape) != 4:
        raise ValueError(f"{what}: x and y must be float32 [B, 1, H, W], got {x.dtype} {tuple(x.shape)} and {y.dtype} {tuple(y.shape)}")


def edge_counts(x: torch.Tensor, y: torch.Tensor, threshold: float = 0.5) -> torch.Tensor:
    """int64 [B, 3] on the device = per row #(x > threshold), #(y > threshold), #(both) of two CUDA float32 [B, 1, H, W] edge
    maps (labels, outputs): the counts behind EdgeAccuracy, exact, one launch, no host synchronisation."""
    _require_gpu(x, "x")
    _require_gpu(y, "y")
    _edge_pair(x, y, torch.float32, "edge_counts")
    with torch.cuda.device(x.device):
        out = torch.empty((x.shape[0], 3), dtype=torch.int64, device=x.device)
        L.check(L.lib().fusg_edge_counts(C.byref(desc(x)), C.byref(desc(y)), float(threshold), out.data_ptr(), stream_ptr()), "edge_counts")
    return out


def edge_counts_host(x, y, threshold: float = 0.5) -> _np.ndarray:
    """`edge_counts` on the CPU (fusg_edge_counts_host): numpy float32 [B, 1, H, W] in, int64 [B, 3] out."""
    x, y = _np.asarray(x), _np.asarray(y)
    _edge_pair(x, y, _np.float32, "edge_counts_host")
    out = _np.zeros((x.shape[0], 3), dtype=_np.int64)
    L.check(L.lib().fusg_edge_counts_host(C.byref(_np_desc(x, L.F32)), C.byref(_np_desc(y, L.F32)), float(threshold), out.ctypes.data),
            "edge_counts_host")
    return out


def sq_diff_sum(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """0-d float64 device tensor = sum((a - b)^2) of two CUDA float tensors of one shape, added in float64 in a fixed order
    (fusg_sq_diff_sum_f32: two launches, no host synchronisation)."""
    _require_gpu(a, "a")
    _require_gpu(b, "b")
    if a.shape != b.shape:
        raise ValueError(f"sq_diff_sum: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    a, b = a.to(torch.float32).contiguous(), b.to(torch.float32).contiguous()
    with torch.cuda.device(a.device):
        out = torch.empty((257,), dtype=torch.float64, device=a.device)
        L.check(L.lib().fusg_sq_diff_sum_f32(a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), stream_ptr()), "sq_diff_sum")
    return out[0]


# ---- feature-space distances (csrc/perceptual.hip; edgeconnect/loss.py) ----------------------------------------------------
def gram_chunk(c: int, hw: int) -> int:
    """Pixels per chunk of `gram` for a C-channel activation of H W = hw pixels (fusg_gram_chunk_pixels): inside a chunk an
    entry is one fp32 fmaf chain, so this is the n of the entry's error bound.  A function of (C, H W) only."""
    k = int(L.lib().fusg_gram_chunk_pixels(int(c), int(hw)))
    if k < 0:
        raise ValueError(f"gram_chunk: C = {c} must be in 1..1024 and H W = {hw} in 1..2^24")
    return k


def _scratch(device, nbytes: int) -> torch.Tensor:
    """Scratch of one call from the caching allocator (kept alive by a recording pass, which replays its address)."""
    s = torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device=device)
    if RECORDER is not None:
        RECORDER.keep.append(s)
    return s


def gram(x: torch.Tensor) -> torch.Tensor:
    """float32 [B, C, C] on the device: out[b] = x[b] x[b]^T / (H W C) over the pixels of a CUDA float32 [B, C, H, W]
    activation in the NHWC-physical layout (channel stride 1; anything else is converted by `as_nhwc`) - StyleLoss.compute_gram.
    Exact-fp32 matrix instruction, exactly symmetric, two launches, no atomics, no host synchronisation (fusg_gram_f32)."""
    _require_gpu(x, "x")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"gram: x must be float32 [B, C, H, W], got {x.dtype} {tuple(x.shape)}")
    B, Cn, H, W = x.shape
    with torch.cuda.device(x.device):
        if Cn > 1 and x.stride(1) != 1:
            x = as_nhwc(x)
        lib = L.lib()
        nbytes = int(lib.fusg_gram_scratch_bytes(B, Cn, H, W))
        if nbytes < 0:
            raise ValueError(f"gram: {tuple(x.shape)}: C must be in 1..1024, H W in 1..2^24, B < 65536")
        out = torch.empty((B, Cn, Cn), dtype=torch.float32, device=x.device)
        L.check(lib.fusg_gram_f32(C.byref(desc(x)), out.data_ptr(), _scratch(x.device, nbytes).data_ptr(), stream_ptr()), "gram")
    return out


def gram_host(x) -> _np.ndarray:
    """`gram` on the CPU in the same order of sums (fusg_gram_f32_host; no GPU needed): numpy float32 [B, C, H, W] in - any
    strides with channel stride 1, a plain array is converted - float32 [B, C, C] out."""
    x = _np.asarray(x)
    if x.ndim != 4 or x.dtype != _np.float32:
        raise ValueError(f"gram_host: x must be float32 [B, C, H, W], got {x.dtype} {x.shape}")
    if x.shape[1] > 1 and x.strides[1] != x.itemsize:
        x = _np.ascontiguousarray(x.transpose(0, 2, 3, 1)).transpose(0, 3, 1, 2)
    out = _np.zeros((x.shape[0], x.shape[1], x.shape[1]), dtype=_np.float32)
    L.check(L.lib().fusg_gram_f32_host(C.byref(_np_desc(x, L.F32)), out.ctypes.data), "gram_host")
    return out


def _as4d(t):
    """[B, ...] as [B, C, H, W] for the row-wise kernels: [B, n] -> [B, n, 1, 1], [B, m, n] -> [B, 1, m, n] (views)."""
    if len(t.shape) == 4:
        return t
    if len(t.shape) == 3:
        return t[:, None]
    if len(t.shape) == 2:
        return t[:, :, None, None]
    raise ValueError(f"expected a [B, ...] tensor of 2 to 4 dimensions, got {tuple(t.shape)}")


def abs_diff_rows(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 [B] on the device: out[r] = sum |a[r] - b[r]| in float64 of two CUDA float32 tensors of one shape [B, ...] and
    any strides (2 to 4 dimensions; only logical elements are read).  Two launches, a fixed order of sums, no atomics, no host
    synchronisation (fusg_abs_diff_rows_f32).  out: a contiguous float64 [B] to write to (a row of a table)."""
    _require_gpu(a, "a")
    _require_gpu(b, "b")
    if a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f"abs_diff_rows: a and b must be float32 of one shape, got {a.dtype} {tuple(a.shape)} and {b.dtype} {tuple(b.shape)}")
    a, b = _as4d(a), _as4d(b)
    with torch.cuda.device(a.device):
        lib = L.lib()
        nbytes = int(lib.fusg_abs_diff_rows_scratch_bytes(*a.shape))
        if nbytes < 0:
            raise ValueError(f"abs_diff_rows: {tuple(a.shape)}: a row must hold 1..2^31 - 1 elements, B < 65536")
        if out is None:
            out = torch.empty((a.shape[0],), dtype=torch.float64, device=a.device)
        elif out.dtype != torch.float64 or tuple(out.shape) != (a.shape[0],) or not out.is_contiguous() or out.device != a.device:
            raise ValueError(f"abs_diff_rows: out must be a contiguous float64 [{a.shape[0]}] on {a.device}")
        L.check(lib.fusg_abs_diff_rows_f32(C.byref(desc(a)), C.byref(desc(b)), out.data_ptr(), _scratch(a.device, nbytes).data_ptr(),
                                           stream_ptr()), "abs_diff_rows")
    return out


def abs_diff_rows_host(a, b) -> _np.ndarray:
    """`abs_diff_rows` on the CPU in the same order of sums (fusg_abs_diff_rows_f32_host): numpy float32 in, float64 [B] out."""
    a, b = _np.asarray(a), _np.asarray(b)
    if a.shape != b.shape or a.dtype != _np.float32 or b.dtype != _np.float32:
        raise ValueError(f"abs_diff_rows_host: a and b must be float32 of one shape, got {a.dtype} {a.shape} and {b.dtype} {b.shape}")
    a, b = _as4d(a), _as4d(b)
    out = _np.zeros((a.shape[0],), dtype=_np.float64)
    L.check(L.lib().fusg_abs_diff_rows_f32_host(C.byref(_np_desc(a, L.F32)), C.byref(_np_desc(b, L.F32)), out.ctypes.data),
            "abs_diff_rows_host")
    return out


# ---- discriminator glue and GAN terms (csrc/gan_terms.hip, elementwise.hip; edgeconnect/networks.py, warp_learn/models.py) -----
GAN_TERM_COLUMNS = ("n", "sum", "sq", "relu_plus", "relu_minus", "bce")


def avgpool3s2(x: torch.Tensor) -> torch.Tensor:
    """nn.AvgPool2d(3, stride=2, padding=1, count_include_pad=False) of an NHWC-physical float32 [B, C, H, W] (anything else is
    converted by `as_nhwc`): [B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1], NHWC-physical (fusg_avgpool3s2_f32)."""
    _require_gpu(x, "x")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"avgpool3s2: x must be float32 [B, C, H, W], got {x.dtype} {tuple(x.shape)}")
    with torch.cuda.device(x.device):
        if not is_nhwc(x):
            x = as_nhwc(x)
        b, c, h, w = x.shape
        # (padding channels are not written: zero them when there are any, for a consumer conv that reads whole quads)
        out = nhwc_empty(b, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1, x.device, zero=c % 4 != 0)
        L.check(L.lib().fusg_avgpool3s2_f32(C.byref(desc(x)), C.byref(desc(out)), stream_ptr()), "avgpool3s2")
    return out


def _np_nhwc(x: _np.ndarray) -> _np.ndarray:
    """A float32 [B, C, H, W] numpy array as a logical view over a dense NHWC copy."""
    return _np.array(x.transpose(0, 2, 3, 1), order="C", copy=True).transpose(0, 3, 1, 2)


def avgpool3s2_host(x) -> _np.ndarray:
    """`avgpool3s2` on the CPU in the same order of sums (fusg_avgpool3s2_f32_host): numpy float32 [B, C, H, W] in and out."""
    x = _np.asarray(x)
    if x.ndim != 4 or x.dtype != _np.float32:
        raise ValueError(f"avgpool3s2_host: x must be float32 [B, C, H, W], got {x.dtype} {x.shape}")
    x = _np_nhwc(x)
    b, c, h, w = x.shape
    out = _np.zeros((b, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=_np.float32).transpose(0, 3, 1, 2)
    L.check(L.lib().fusg_avgpool3s2_f32_host(C.byref(_np_desc(x, L.F32)), C.byref(_np_desc(out, L.F32))), "avgpool3s2_host")
    return out


def mask_mul(x: torch.Tensor, m: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B, C, H, W] * m [B, 1, H, W], float32 through any strides (fusg_mask_mul_f32); out: an NHWC-physical tensor unless given."""
    _require_gpu(x, "x")
    _require_gpu(m, "m")
    if (x.dim() != 4 or m.dim() != 4 or x.dtype != torch.float32 or m.dtype != torch.float32 or m.shape[1] != 1
            or (m.shape[0],) + tuple(m.shape[2:]) != (x.shape[0],) + tuple(x.shape[2:])):
        raise ValueError(f"mask_mul: x must be float32 [B, C, H, W] and m float32 [B, 1, H, W], got {tuple(x.shape)} and {tuple(m.shape)}")
    with torch.cuda.device(x.device):
        if out is None:
            out = nhwc_empty(*x.shape, x.device)
        L.check(L.lib().fusg_mask_mul_f32(C.byref(desc(x)), C.byref(desc(m)), C.byref(desc(out)), stream_ptr()), "mask_mul")
    return out


def gan_terms_chunk(n: int) -> int:
    """Elements per (row, chunk) workgroup of `gan_terms` for a row of n elements: a function of n only."""
    return int(L.lib().fusg_gan_terms_chunk(int(n)))


def gan_terms(pred: torch.Tensor, label: float = 1.0, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 [B, 6] on the device, columns `GAN_TERM_COLUMNS`: per row of a CUDA float32 [B, C, H, W] `pred` (any strides)
    n, sum x, sum (m x - m label)^2, sum relu(1 + x), sum relu(1 - x) and the BCE sum against `label` with nn.BCELoss's clamp
    at -100.  The BCE column is NaN for a row with an x outside [0, 1]: pick the columns that mean something for `pred`.
    mask: float32 [B, 1, Hm, Wm], sampled as `F.interpolate(mask, size=(H, W))` samples (nearest), used in the squared column
    only.  Two launches, a fixed order of float64 sums, no atomics, no host synchronisation (fusg_gan_terms_rows_f32)."""
    _require_gpu(pred, "pred")
    if pred.dim() != 4 or pred.dtype != torch.float32:
        raise ValueError(f"gan_terms: pred must be float32 [B, C, H, W], got {pred.dtype} {tuple(pred.shape)}")
    if mask is not None:
        _require_gpu(mask, "mask")
        if mask.dim() != 4 or mask.dtype != torch.float32 or mask.shape[0] != pred.shape[0] or mask.shape[1] != 1:
            raise ValueError(f"gan_terms: mask must be float32 [{pred.shape[0]}, 1, Hm, Wm], got {mask.dtype} {tuple(mask.shape)}")
    nc = len(GAN_TERM_COLUMNS)
    with torch.cuda.device(pred.device):
        lib = L.lib()
        nbytes = int(lib.fusg_gan_terms_scratch_bytes(*pred.shape))
        if nbytes < 0:
            raise ValueError(f"gan_terms: {tuple(pred.shape)}: a row must hold 1..2^31 - 1 elements, B < 65536")
        if out is None:
            out = torch.empty((pred.shape[0], nc), dtype=torch.float64, device=pred.device)
        elif out.dtype != torch.float64 or tuple(out.shape) != (pred.shape[0], nc) or not out.is_contiguous() or out.device != pred.device:
            raise ValueError(f"gan_terms: out must be a contiguous float64 [{pred.shape[0]}, {nc}] on {pred.device}")
        L.check(lib.fusg_gan_terms_rows_f32(C.byref(desc(pred)), C.byref(desc(mask)) if mask is not None else None, float(label),
                                            out.data_ptr(), _scratch(pred.device, nbytes).data_ptr(), stream_ptr()), "gan_terms")
    return out


def gan_terms_host(pred, label: float = 1.0, mask=None) -> _np.ndarray:
    """`gan_terms` on the CPU in the same order of sums (fusg_gan_terms_rows_f32_host): numpy float32 in (any strides), float64
    [B, 6] out."""
    pred = _np.asarray(pred)
    if pred.ndim != 4 or pred.dtype != _np.float32:
        raise ValueError(f"gan_terms_host: pred must be float32 [B, C, H, W], got {pred.dtype} {pred.shape}")
    md = None
    if mask is not None:
        mask = _np.asarray(mask)
        if mask.ndim != 4 or mask.dtype != _np.float32 or mask.shape[0] != pred.shape[0] or mask.shape[1] != 1:
            raise ValueError(f"gan_terms_host: mask must be float32 [{pred.shape[0]}, 1, Hm, Wm], got {mask.dtype} {mask.shape}")
        md = C.byref(_np_desc(mask, L.F32))
    out = _np.zeros((pred.shape[0], len(GAN_TERM_COLUMNS)), dtype=_np.float64)
    L.check(L.lib().fusg_gan_terms_rows_f32_host(C.byref(_np_desc(pred, L.F32)), md, float(label), out.ctypes.data), "gan_terms_host")
    return out


# ---------------------------------------------------------------------------------------------
# background frame (csrc/background.h): the per-pixel lower median of the frames in which no tracker box covers the pixel
# ---------------------------------------------------------------------------------------------
BACKGROUND_MAX_FRAMES = 64
BACKGROUND_MAX_BOXES = 64           # per frame
BACKGROUND_MAX_DIM = 32767          # H, W and the margin (csrc/workgroup.h: wg::MAX_DIM)


# Every function of the video front end comes as a pair: the device form takes CUDA tensors, its `_host` twin numpy arrays and
# runs the kernel's code on the CPU.  A pair has ONE private body; what differs is asked of the side it runs on, _DEV or _HOST.
@_contextlib.contextmanager
def _device_side(ref: torch.Tensor, name: str):
    """What only the device form does: the GPU check, the device's scope around the allocations and the launch, and `up` - a host
    table to the device without a synchronisation (a tensor stays as it is) - whose results a pass that is being recorded keeps."""
    _require_gpu(ref, name)
    held = []

    def up(t):
        held.append(t if torch.is_tensor(t) else h2d(t, ref.device))
        return held[-1]
    with torch.cuda.device(ref.device):
        yield up
    if RECORDER is not None:
        RECORDER.keep.extend(held)


@_contextlib.contextmanager
def _host_side(ref, name: str):
    yield lambda t: t


def _as_np(x):
    return [_np.asarray(v) for v in x] if isinstance(x, (list, tuple)) else _np.asarray(x)


_DEV = _SimpleNamespace(
    tag="", noun="tensor", stream=True, side=_device_side, arrays=lambda x: x, is_array=torch.is_tensor,
    u8=torch.uint8, i32=torch.int32, i64=torch.int64,
    empty=lambda shape, dtype, ref: torch.empty(shape, dtype=dtype, device=ref.device),
    zeros=lambda shape, dtype, ref: torch.zeros(shape, dtype=dtype, device=ref.device),
    ptr=lambda a: a.data_ptr(), dense=lambda a: a.is_contiguous(), contiguous=lambda a: a.contiguous(), cat=torch.cat,
    near=lambda a, ref: a.device == ref.device, at=lambda ref: f" on {ref.device}")
_HOST = _SimpleNamespace(
    tag="_host", noun="array", stream=False, side=_host_side, arrays=_as_np, is_array=lambda a: isinstance(a, _np.ndarray),
    u8=_np.uint8, i32=_np.int32, i64=_np.int64,
    empty=lambda shape, dtype, ref: _np.zeros(shape, dtype=dtype), zeros=lambda shape, dtype, ref: _np.zeros(shape, dtype=dtype),
    ptr=lambda a: a.ctypes.data, dense=lambda a: a.flags.c_contiguous, contiguous=_np.ascontiguousarray, cat=_np.concatenate,
    near=lambda a, ref: True, at=lambda ref: "")


def _call(wh, what: str, entry: str, *args) -> None:
    """The library's entry of this side: `entry` with the current stream appended, or its `_host` twin (fusg_x_u8 -> fusg_x_host)."""
    if wh.stream:
        return L.check(getattr(L.lib(), entry)(*args, stream_ptr()), what)
    L.check(getattr(L.lib(), (entry[:-3] if entry.endswith("_u8") else entry) + "_host")(*args), what)


def _fits(wh, a, dtype, shape, ref) -> bool:
    """A dense array of this side, of this type and shape (None: any one-dimensional), where `ref` is."""
    return wh.is_array(a) and a.dtype == dtype and (len(a.shape) == 1 if shape is None else tuple(a.shape) == tuple(shape)) \
        and wh.dense(a) and wh.near(a, ref)


def _ptrs(wh, arrays):
    return (C.c_void_p * len(arrays))(*[wh.ptr(a) for a in arrays])


def _int_rows4(table, what: str, name: str, row: str) -> _np.ndarray:
    """An integer [n, 4] host table as int64 [n, 4], every entry inside int32: the caller casts after its own checks."""
    b = _np.asarray(table)
    if b.size and (b.dtype.kind not in "iu" or b.size % 4 or (b.ndim > 1 and b.shape[-1] != 4)):
        raise ValueError(f"{what}: {name} must be an integer [n, 4] array, got {b.dtype} {b.shape}")
    b = b.reshape(-1, 4).astype(_np.int64)
    if b.size and (b.min() < -2 ** 31 or b.max() > 2 ** 31 - 1):
        raise ValueError(f"{what}: {row} does not fit int32")
    return b


def _background_frames(frames, u8, what: str):
    """The T frames as a list, checked: uint8 [H, W, 3], dense, one shape, T, H and W inside the limits."""
    if not isinstance(frames, (list, tuple)):
        if not hasattr(frames, "shape") or len(frames.shape) != 4:
            raise ValueError(f"{what}: frames must be a sequence of uint8 [H, W, 3] images or one [T, H, W, 3] stack")
        frames = [frames[t] for t in range(frames.shape[0])]
    T = len(frames)
    if not 1 <= T <= BACKGROUND_MAX_FRAMES:
        raise ValueError(f"{what}: {T} frames (1..{BACKGROUND_MAX_FRAMES})")
    for t, f in enumerate(frames):
        if not hasattr(f, "shape") or f.dtype != u8 or len(f.shape) != 3 or f.shape[2] != 3:
            raise ValueError(f"{what}: frame {t} must be uint8 [H, W, 3], got {getattr(f, 'dtype', type(f))} {tuple(getattr(f, 'shape', ()))}")
        if tuple(f.shape) != tuple(frames[0].shape):
            raise ValueError(f"{what}: frame {t} is {tuple(f.shape)}, frame 0 is {tuple(frames[0].shape)}")
        if not (f.is_contiguous() if isinstance(f, torch.Tensor) else f.flags.c_contiguous):
            raise ValueError(f"{what}: frame {t} is not contiguous")
    H, W = int(frames[0].shape[0]), int(frames[0].shape[1])
    if not (1 <= H <= BACKGROUND_MAX_DIM and 1 <= W <= BACKGROUND_MAX_DIM):
        raise ValueError(f"{what}: frames of {H} x {W} (H and W in 1..{BACKGROUND_MAX_DIM})")
    return list(frames), T, H, W


def _background_args(T: int, boxes, margin, min_valid, what: str):
    """(flat int32 [N, 4] boxes, int32 [T + 1] offsets, margin, min_valid), checked against the limits."""
    margin, min_valid = int(margin), int(min_valid)
    if not 0 <= margin <= BACKGROUND_MAX_DIM:
        raise ValueError(f"{what}: margin = {margin} (0..{BACKGROUND_MAX_DIM})")
    if not 1 <= min_valid <= T:
        raise ValueError(f"{what}: min_valid = {min_valid} (1..T = {T})")
    offs = _np.zeros((T + 1,), dtype=_np.int32)
    if boxes is None:
        return _np.zeros((0, 4), dtype=_np.int32), offs, margin, min_valid
    if len(boxes) != T:
        raise ValueError(f"{what}: {len(boxes)} box lists for {T} frames")
    rows = []
    for t, b in enumerate(boxes):
        b = _int_rows4(b, what, f"the boxes of frame {t}", f"a box of frame {t}")
        if b.shape[0] > BACKGROUND_MAX_BOXES:
            raise ValueError(f"{what}: frame {t} has {b.shape[0]} boxes (at most {BACKGROUND_MAX_BOXES})")
        rows.append(b.astype(_np.int32))
        offs[t + 1] = offs[t] + b.shape[0]
    return _np.ascontiguousarray(_np.concatenate(rows, axis=0)), offs, margin, min_valid


def background_median(frames, boxes=None, margin: int = 0, min_valid: int = 1, out=None):
    """(bg uint8 [H, W, 3], count uint8 [H, W]) on the device: per pixel and channel the lower median (rank (m - 1) // 2, always a
    value that occurred) over the frames in which no box, grown by `margin` on every side, covers the pixel; `count` is the
    number of those frames, and a pixel with count < min_valid took all T frames instead.  frames: a sequence of T <= 64 CUDA
    uint8 [H, W, 3] tensors (separate allocations are fine) or one [T, H, W, 3] tensor; boxes: None or T host int arrays
    [nb_t, 4] of (x0, y0, x1, y1), both ends inclusive, at most 64 per frame.  out: an optional (bg, count) pair to write into.
    One launch on the current stream, no atomics, no host synchronisation (fusg_background_median_u8)."""
    return _background_median(_DEV, frames, boxes, margin, min_valid, out)


def background_median_host(frames, boxes=None, margin: int = 0, min_valid: int = 1):
    """`background_median` on the CPU by the same code (fusg_background_median_host; no GPU needed): numpy uint8 frames in,
    (bg, count) numpy arrays out."""
    return _background_median(_HOST, frames, boxes, margin, min_valid, None)


def _one_place(wh, arrays, what: str) -> None:
    for a in arrays:
        if not wh.near(a, arrays[0]):
            raise ValueError(f"{what}: a frame or background is on {a.device}, frame 0 on {arrays[0].device}")


def _background_median(wh, frames, boxes, margin, min_valid, out):
    what = "background_median" + wh.tag
    frames, T, H, W = _background_frames(wh.arrays(frames), wh.u8, what)
    for t, f in enumerate(frames):
        if not wh.near(f, frames[0]):
            raise ValueError(f"{what}: frame {t} is on {f.device}, frame 0 on {frames[0].device}")
    flat, offs, margin, min_valid = _background_args(T, boxes, margin, min_valid, what)
    shapes = {"bg": (H, W, 3), "count": (H, W)}
    for (name, shape), o in zip(shapes.items(), out or ()):
        if not _fits(wh, o, wh.u8, shape, frames[0]):
            raise ValueError(f"{what}: out's {name} must be a contiguous uint8 {shape} {wh.noun}{wh.at(frames[0])}")
    with wh.side(frames[0], "frames") as up:
        bg, count = out if out is not None else [wh.empty(s, wh.u8, frames[0]) for s in shapes.values()]
        _call(wh, what, "fusg_background_median_u8", _ptrs(wh, frames), T, H, W, wh.ptr(up(flat)) if flat.shape[0] else None,
              offs.ctypes.data, margin, min_valid, wh.ptr(bg), wh.ptr(count))
    return bg, count


# ---------------------------------------------------------------------------------------------
# vehicle masks from the estimated background (csrc/foreground.h) and the erase that uses them
# ---------------------------------------------------------------------------------------------
FOREGROUND_LIMITS = {"thr": 254, "open_r": 3, "close_r": 7, "grow": 15}
FOREGROUND_STATS = ("n_f0", "n_seed", "n_mask", "flags")
FOREGROUND_FALLBACK, FOREGROUND_BORDER, FOREGROUND_REFUSED = 1, 2, 4


def _box_table(boxes, n, H, W, what: str, name: str, inside: bool) -> _np.ndarray:
    """An integer [n, 4] host table as int32; inside: every row a half-open rectangle of the W x H frame, as `_inpaint_args` asks."""
    b = _int_rows4(boxes, what, name, f"a row of {name}")
    if n is not None and b.shape[0] != n:
        raise ValueError(f"{what}: {b.shape[0]} {name} for {n} boxes")
    if inside:
        bad = (b[:, 0] < 0) | (b[:, 1] < 0) | (b[:, 2] < b[:, 0]) | (b[:, 3] < b[:, 1]) | (b[:, 2] > W) | (b[:, 3] > H)
        if bad.any():
            v = int(_np.nonzero(bad)[0][0])
            raise ValueError(f"{what}: box {v} = {b[v].tolist()} leaves the {W} x {H} frame (x0, y0, x1, y1, half-open)")
    return _np.ascontiguousarray(b.astype(_np.int32))


def _frames_and_backgrounds(frames, backgrounds, u8, what: str, name: str = "backgrounds"):
    """One frame or up to 64, and one background for all of them or one each -> (frames, backgrounds, T, H, W), checked as
    `_background_frames` checks the frames."""
    if hasattr(frames, "shape") and len(frames.shape) == 3:
        frames = [frames]
    frames, T, H, W = _background_frames(frames, u8, what)
    if hasattr(backgrounds, "shape") and len(backgrounds.shape) == 3:
        backgrounds = [backgrounds] * T
    if hasattr(backgrounds, "shape") and len(backgrounds.shape) != 4:
        raise ValueError(f"{what}: {name} must be uint8 [H, W, 3], or one per frame")
    bgs = [backgrounds[f] for f in range(len(backgrounds))]
    if len(bgs) != T:
        raise ValueError(f"{what}: {len(bgs)} backgrounds for {T} frames")
    for f, g in enumerate(bgs):
        if not hasattr(g, "shape") or g.dtype != u8 or tuple(g.shape) != (H, W, 3):
            raise ValueError(f"{what}: background {f} must be uint8 {(H, W, 3)}, got {getattr(g, 'dtype', type(g))} {tuple(getattr(g, 'shape', ()))}")
        if not (g.is_contiguous() if isinstance(g, torch.Tensor) else g.flags.c_contiguous):
            raise ValueError(f"{what}: background {f} is not contiguous")
    return frames, bgs, T, H, W


def _foreground_args(frames, background, boxes, cores, thr, open_r, close_r, grow, fallback, frame_rows, max_box, offs, u8, what):
    """What both forms of `foreground_masks` check before anything is touched -> (frames, backgrounds, H, W, boxes int32 [n, 4],
    cores int32 [n, 4], offsets int64 [n], the bytes the masks take, frame_rows int32 [F + 1], the five parameters, max_box)."""
    frames, bgs, F, H, W = _frames_and_backgrounds(frames, background, u8, what, "background")
    par = []
    for name, v in (("thr", thr), ("open_r", open_r), ("close_r", close_r), ("grow", grow)):
        if int(v) != v or not 0 <= int(v) <= FOREGROUND_LIMITS[name]:
            raise ValueError(f"{what}: {name} = {v} (0..{FOREGROUND_LIMITS[name]})")
        par.append(int(v))
    par.append(1 if fallback else 0)
    bx = _box_table(boxes, None, H, W, what, "boxes", True)
    n = bx.shape[0]
    cr = _box_table(cores, n, H, W, what, "cores", False)
    if frame_rows is None:
        if F != 1:
            raise ValueError(f"{what}: {F} frames need frame_rows (int [{F + 1}], from 0 to the number of boxes)")
        rows = _np.asarray([0, n], dtype=_np.int32)
    else:
        rows = _np.asarray(frame_rows, dtype=_np.int64).reshape(-1)
        if rows.shape[0] != F + 1 or rows[0] != 0 or rows[-1] != n or (_np.diff(rows) < 0).any():
            raise ValueError(f"{what}: frame_rows = {rows.tolist()} must be {F + 1} non-decreasing offsets from 0 to the {n} boxes")
        rows = rows.astype(_np.int32)
    hw = (bx[:, 3] - bx[:, 1]).astype(_np.int64) * (bx[:, 2] - bx[:, 0]).astype(_np.int64)
    if offs is None:
        offs = _np.zeros(n, dtype=_np.int64)
        offs[1:] = _np.cumsum(hw)[:-1]
    else:
        offs = _np.ascontiguousarray(_np.asarray(offs, dtype=_np.int64).reshape(-1))
        if offs.shape[0] != n:
            raise ValueError(f"{what}: {offs.shape[0]} offsets for {n} boxes")
    if max_box is None:
        max_box = (int((bx[:, 3] - bx[:, 1]).max()), int((bx[:, 2] - bx[:, 0]).max())) if n else (0, 0)
    mb = (int(max_box[0]), int(max_box[1]))
    if not (0 <= mb[0] <= BACKGROUND_MAX_DIM and 0 <= mb[1] <= BACKGROUND_MAX_DIM):
        raise ValueError(f"{what}: max_box = {mb} (0..{BACKGROUND_MAX_DIM})")
    return frames, bgs, H, W, bx, cr, offs, int(hw.sum()), _np.ascontiguousarray(rows), par, mb


def foreground_masks(frames, background, boxes, cores, thr: int = 24, open_r: int = 1, close_r: int = 3, grow: int = 0,
                     fallback: bool = True, frame_rows=None, max_box=None, out=None):
    """Every box's vehicle mask from the background, on the device (fusg_foreground_masks_u8, one launch on the current stream, one
    workgroup per box, nothing read back; csrc/foreground.h states the definition): inside the box, max_c |frame - background| >
    thr, opened by the (2 open_r + 1)^2 square, closed by the (2 close_r + 1)^2 square without eating back from the box edge, the
    part 4-connected to the core kept, its enclosed holes filled, grown by `grow`; an empty seed gives the core rectangle
    (fallback) or nothing.  The defaults 24 / 1 / 3 are untried on real video.
    frames: one CUDA uint8 [H, W, 3] frame, or a sequence / stack of up to 64 with frame_rows (int [F + 1]: boxes [frame_rows[f],
    frame_rows[f + 1]) read frame f); background: one [H, W, 3] for all frames or one per frame; boxes, cores: host int [n, 4]
    (x0, y0, x1, y1) half-open, frame coordinates - the boxes checked as `inpaint_inputs` checks them, the cores free (clipped to
    their box); both uploaded without a synchronisation.  max_box = (h, w): the bound the launch is sized for (default: the largest
    box; a box that exceeds it is refused and flagged).  out = (buffer CUDA uint8 [m], host int64 offsets [n]) to write into
    (default: a fresh buffer, the offsets the running sum of h w).
    -> ((buffer uint8 [m], offsets int64 [n]) on the device - what `inpaint_inputs_boxed` takes as box_masks -, stats int32 [n, 4]
    on the device: `FOREGROUND_STATS`, flags = 1 fallback taken | 2 touches the box border | 4 refused, bytes not written)."""
    return _foreground_masks(_DEV, frames, background, boxes, cores, thr, open_r, close_r, grow, fallback, frame_rows, max_box, out)


def foreground_masks_host(frames, background, boxes, cores, thr: int = 24, open_r: int = 1, close_r: int = 3, grow: int = 0,
                          fallback: bool = True, frame_rows=None, max_box=None, out=None):
    """`foreground_masks` on the CPU by the same code (fusg_foreground_masks_host; no GPU needed): numpy uint8 images in,
    ((buffer uint8 [m], offsets int64 [n]), stats int32 [n, 4]) numpy arrays out."""
    return _foreground_masks(_HOST, frames, background, boxes, cores, thr, open_r, close_r, grow, fallback, frame_rows, max_box, out)


def _foreground_masks(wh, frames, background, boxes, cores, thr, open_r, close_r, grow, fallback, frame_rows, max_box, out):
    what = "foreground_masks" + wh.tag
    frames, bgs, H, W, bx, cr, offs, nbytes, rows, par, mb = _foreground_args(
        wh.arrays(frames), wh.arrays(background), boxes, cores, thr, open_r, close_r, grow, fallback, frame_rows, max_box,
        None if out is None else out[1], wh.u8, what)
    ref = frames[0]
    _one_place(wh, frames + bgs, what)
    if out is not None and not _fits(wh, out[0], wh.u8, None, ref):
        raise ValueError(f"{what}: out's buffer must be a contiguous uint8 [m] {wh.noun}{wh.at(ref)}")
    n = bx.shape[0]
    with wh.side(ref, "frames") as up:
        buf = wh.empty((nbytes,), wh.u8, ref) if out is None else out[0]
        stats = wh.empty((n, 4), wh.i32, ref)
        if n == 0:
            return (buf, wh.empty((0,), wh.i64, ref)), stats
        tab, offs = up(_np.concatenate([bx, cr])), up(offs)       # one copy for both tables
        scratch = ()
        if wh.stream:                                             # the planes of boxes that do not fit LDS
            sb = int(L.lib().fusg_foreground_masks_scratch_bytes(n, mb[0], mb[1]))
            scratch = (up(torch.empty((sb,), dtype=torch.uint8, device=ref.device)).data_ptr() if sb > 0 else None,)
        _call(wh, what, "fusg_foreground_masks_u8", _ptrs(wh, frames), _ptrs(wh, bgs), rows.ctypes.data, len(frames), H, W,
              wh.ptr(tab[:n]), wh.ptr(tab[n:]), wh.ptr(offs), n, *par, mb[0], mb[1], wh.ptr(buf) if buf.shape[0] else None,
              int(buf.shape[0]), wh.ptr(stats), *scratch)
    return (buf, offs), stats


def _erase_args(frame, background, box_masks, boxes, u8, what):
    """Shared by both forms of `erase_to_background`: -> (H, W, boxes int32 [n, 4], buffer, offsets)."""
    for name, a in (("frame", frame), ("background", background)):
        if not hasattr(a, "shape") or a.dtype != u8 or len(a.shape) != 3 or a.shape[2] != 3:
            raise ValueError(f"{what}: {name} must be uint8 [H, W, 3], got {getattr(a, 'dtype', type(a))} {tuple(getattr(a, 'shape', ()))}")
        if not (a.is_contiguous() if isinstance(a, torch.Tensor) else a.flags.c_contiguous):
            raise ValueError(f"{what}: {name} is not contiguous")
    if tuple(background.shape) != tuple(frame.shape):
        raise ValueError(f"{what}: background is {tuple(background.shape)}, the frame {tuple(frame.shape)}")
    H, W = int(frame.shape[0]), int(frame.shape[1])
    if not (1 <= H <= BACKGROUND_MAX_DIM and 1 <= W <= BACKGROUND_MAX_DIM):
        raise ValueError(f"{what}: frames of {H} x {W} (H and W in 1..{BACKGROUND_MAX_DIM})")
    if not _is_packed_pair(box_masks) or box_masks[0].dtype != u8:
        raise ValueError(f"{what}: box_masks must be a packed (uint8 buffer [m], int64 offsets [n]) pair, as `foreground_masks` returns it")
    bx = _box_table(boxes, int(box_masks[1].shape[0]), H, W, what, "boxes", True)
    return H, W, bx, box_masks[0], box_masks[1]


def erase_to_background(frame: torch.Tensor, background: torch.Tensor, box_masks, boxes, out=None) -> torch.Tensor:
    """The frame with the masked pixels of every box replaced by the background (fusg_erase_boxes_u8, two launches on the current
    stream): a compositing base that keeps the rest of the traffic.  frame, background CUDA uint8 [H, W, 3]; box_masks = the
    packed (buffer, offsets) pair of `foreground_masks` (offsets on the device or host); boxes host int [n, 4].  -> uint8 [H, W,
    3] (out: a buffer to write into, not overlapping the inputs)."""
    return _erase_to_background(_DEV, frame, background, box_masks, boxes, out)


def erase_to_background_host(frame, background, box_masks, boxes) -> _np.ndarray:
    """`erase_to_background` on the CPU by the same code (fusg_erase_boxes_host): numpy in and out."""
    if isinstance(box_masks, tuple) and len(box_masks) == 2:
        box_masks = (_np.ascontiguousarray(box_masks[0]), _np.ascontiguousarray(box_masks[1], dtype=_np.int64))
    return _erase_to_background(_HOST, frame, background, box_masks, boxes, None)


def _erase_to_background(wh, frame, background, box_masks, boxes, out):
    what = "erase_to_background" + wh.tag
    frame, background = wh.arrays(frame), wh.arrays(background)
    H, W, bx, buf, offs = _erase_args(frame, background, box_masks, boxes, wh.u8, what)
    if not _fits(wh, buf, wh.u8, None, frame) or not wh.near(background, frame):
        raise ValueError(f"{what}: the frame, the background and the mask buffer must be contiguous tensors on one device")
    if out is not None and not _fits(wh, out, wh.u8, (H, W, 3), frame):
        raise ValueError(f"{what}: out must be a contiguous uint8 {(H, W, 3)} {wh.noun}{wh.at(frame)}")
    n = bx.shape[0]
    with wh.side(frame, "frame") as up:
        dst = wh.empty((H, W, 3), wh.u8, frame) if out is None else out
        offs = up(offs.to(torch.int64).contiguous() if torch.is_tensor(offs) and offs.is_cuda else _np.asarray(offs, dtype=_np.int64))
        _call(wh, what, "fusg_erase_boxes_u8", wh.ptr(frame), wh.ptr(background), H, W, wh.ptr(buf) if buf.shape[0] else None,
              int(buf.shape[0]), wh.ptr(offs) if n else None, wh.ptr(up(bx)) if n else None, n, wh.ptr(dst))
    return dst


# ---------------------------------------------------------------------------------------------
# vehicle boxes from the estimated background, on a cell grid (csrc/foreground_boxes.h)
# ---------------------------------------------------------------------------------------------
FOREGROUND_BOXES_MAX = 64           # K: boxes per frame, the background median's limit
FOREGROUND_BOXES_COMPONENTS = 256   # components examined per frame
FOREGROUND_BOXES_STATS = ("n_kept", "n_examined", "n_p", "flags")
FOREGROUND_BOXES_OVERFLOW, FOREGROUND_BOXES_TRUNCATED = 1, 2


def _foreground_boxes_args(frames, backgrounds, thr, cell, min_count, open_r, close_r, min_area, min_w, min_h, max_boxes, roi, u8, what):
    """What both forms of `foreground_boxes` check themselves - the images and that every parameter is an integer; the ranges are
    the library's to refuse -> (frames, backgrounds, T, H, W, the eleven int32 parameters with K in place, roi int32 [4])."""
    frames, bgs, T, H, W = _frames_and_backgrounds(frames, backgrounds, u8, what)
    par = []
    for name, v in (("thr", thr), ("cell", cell), ("min_count", min_count), ("open_r", open_r), ("close_r", close_r),
                    ("min_area", min_area), ("min_w", min_w), ("min_h", min_h), ("max_boxes", max_boxes)):
        if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
            raise ValueError(f"{what}: {name} = {v} must be an integer")
        par.append(int(v))
    r = _np.asarray((0, 0, W, H) if roi is None else roi)
    if r.dtype.kind not in "iu" or r.shape != (4,) or r.min() < -2 ** 31 or r.max() >= 2 ** 31:
        raise ValueError(f"{what}: roi must be four integers (x0, y0, x1, y1), half-open, got {roi}")
    return frames, bgs, T, H, W, par, _np.ascontiguousarray(r.astype(_np.int32))


def foreground_boxes(frames, backgrounds, thr: int = 24, cell: int = 8, min_count: int = 16, open_r: int = 0, close_r: int = 1,
                     min_area: int = 400, min_w: int = 12, min_h: int = 12, max_boxes: int = 64, roi=None, out=None):
    """Vehicle boxes of every frame from the background, on the device (fusg_foreground_boxes_u8: two launches on the current
    stream, nothing read back; csrc/foreground_boxes.h states the definition): a pixel counts when max_c |frame - background| >
    thr inside roi; a cell x cell cell (4, 8 or 16) is on with >= min_count such pixels; the cell grid is opened by the
    (2 open_r + 1)^2 square and closed by the (2 close_r + 1)^2 one without eating back from the frame edge; each 4-connected
    component, in the raster order of its first cell (the first 256 are looked at), is kept when it has >= min_area such pixels
    and its pixel-tight box is >= min_w wide and >= min_h high.  The defaults are tried on synthetic scenes only.
    frames: one CUDA uint8 [H, W, 3] frame, or a sequence / stack of up to 64; backgrounds: one [H, W, 3] for all frames or one
    per frame; roi = (x0, y0, x1, y1) half-open, default the frame; out = (boxes, box_stats, stats) to write into.
    -> (boxes int32 [T, K, 4] half-open (x0, y0, x1, y1), box_stats int32 [T, K, 2] = (area, n_cells), stats int32 [T, 4] =
    `FOREGROUND_BOXES_STATS`, flags 1 = more than K = max_boxes were kept, 2 = more than 256 components) on the device; the rows
    from min(n_kept, K) on are zeros."""
    return _foreground_boxes(_DEV, frames, backgrounds, thr, cell, min_count, open_r, close_r, min_area, min_w, min_h, max_boxes, roi, out)


def foreground_boxes_host(frames, backgrounds, thr: int = 24, cell: int = 8, min_count: int = 16, open_r: int = 0, close_r: int = 1,
                          min_area: int = 400, min_w: int = 12, min_h: int = 12, max_boxes: int = 64, roi=None, out=None):
    """`foreground_boxes` on the CPU by the same code (fusg_foreground_boxes_host; no GPU needed): numpy uint8 images in, (boxes,
    box_stats, stats) int32 numpy arrays out."""
    return _foreground_boxes(_HOST, frames, backgrounds, thr, cell, min_count, open_r, close_r, min_area, min_w, min_h, max_boxes, roi, out)


def _foreground_boxes(wh, frames, backgrounds, thr, cell, min_count, open_r, close_r, min_area, min_w, min_h, max_boxes, roi, out):
    what = "foreground_boxes" + wh.tag
    frames, bgs, T, H, W, par, r = _foreground_boxes_args(wh.arrays(frames), wh.arrays(backgrounds), thr, cell, min_count, open_r, close_r,
                                                          min_area, min_w, min_h, max_boxes, roi, wh.u8, what)
    ref = frames[0]
    _one_place(wh, frames + bgs, what)
    K = par[-1]
    if not 1 <= K <= FOREGROUND_BOXES_MAX:
        raise ValueError(f"{what}: max_boxes = {K} (1..{FOREGROUND_BOXES_MAX})")
    shapes = ((T, K, 4), (T, K, 2), (T, 4))
    if out is not None and not all(_fits(wh, o, wh.i32, s, ref) for o, s in zip(out, shapes)):
        raise ValueError(f"{what}: out must be contiguous int32 {wh.noun}s of {shapes}{wh.at(ref)}")
    with wh.side(ref, "frames") as up:
        scratch = ()
        if wh.stream:                                             # the cell pass's records
            sb = int(L.lib().fusg_foreground_boxes_scratch_bytes(T, H, W, par[1]))
            if sb < 0:
                raise ValueError(f"{what}: cell = {par[1]} (4, 8 or 16)")
            scratch = (up(torch.empty((sb // 4,), dtype=torch.int32, device=ref.device)).data_ptr(),)
        boxes, box_stats, stats = out if out is not None else [wh.empty(s, wh.i32, ref) for s in shapes]
        _call(wh, what, "fusg_foreground_boxes_u8", _ptrs(wh, frames), _ptrs(wh, bgs), T, H, W, *par[:8], r.ctypes.data, K,
              wh.ptr(boxes), wh.ptr(box_stats), wh.ptr(stats), *scratch)
    return boxes, box_stats, stats


# ---------------------------------------------------------------------------------------------
# the boxes of successive frames linked into trajectories (csrc/track_boxes.h)
# ---------------------------------------------------------------------------------------------
LINK_BOXES_STATS = ("n_tracks", "n_live", "n_linked", "flags")
LINK_BOXES_BAD_BOX, LINK_BOXES_TRACKS_FULL, LINK_BOXES_LIVE_FULL, LINK_BOXES_ORDER, LINK_BOXES_BAD_STATE = 1, 2, 4, 8, 16
LINK_BOXES_LIVE_MAX = 128           # live tracks per video
LINK_BOXES_MAX_VIDEOS = 64          # videos (workgroups) per call
LINK_BOXES_STATE_WORDS = 8 + 128 * 13


def _link_boxes_args(boxes, stats, iou, max_gap, predict, max_tracks, t0, wh, what):
    """What both forms of `link_boxes` check themselves - the tables' shapes and types and that every parameter is an integer;
    the ranges are the library's to refuse -> (boxes and stats as ONE table each, one video?, S, K, first int32 [S + 1], t0 int32
    [S], the five int32 parameters)."""
    is_t, i32 = wh.is_array, wh.i32
    one = is_t(boxes)
    bl, sl = ([boxes], [stats]) if one else (list(boxes), list(stats))
    S = len(bl)
    if S < 1 or len(sl) != S:
        raise ValueError(f"{what}: {S} box tables and {len(sl)} stats tables (one pair per video, at least one)")
    K = None
    for s, (b, st) in enumerate(zip(bl, sl)):
        if not is_t(b) or not is_t(st) or b.dtype != i32 or st.dtype != i32 or len(b.shape) != 3 or b.shape[2] != 4 \
                or tuple(st.shape) != (b.shape[0], 4):
            raise ValueError(f"{what}: video {s} must be int32 boxes [T, K, 4] and int32 stats [T, 4] (ops.foreground_boxes' tables), got "
                             f"{getattr(b, 'dtype', type(b))} {tuple(getattr(b, 'shape', ()))} and {getattr(st, 'dtype', type(st))} "
                             f"{tuple(getattr(st, 'shape', ()))}")
        K = int(b.shape[1]) if K is None else K
        if int(b.shape[1]) != K:
            raise ValueError(f"{what}: video {s} has K = {int(b.shape[1])} boxes per frame, video 0 has {K}")
    first = _np.zeros((S + 1,), dtype=_np.int64)
    first[1:] = _np.cumsum([int(b.shape[0]) for b in bl])
    if first[-1] >= 2 ** 31:
        raise ValueError(f"{what}: {int(first[-1])} frames in all")
    par = []
    if not isinstance(iou, (tuple, list)) or len(iou) != 2:
        raise ValueError(f"{what}: iou must be a pair of integers (numerator, denominator), got {iou}")
    for name, v in (("iou[0]", iou[0]), ("iou[1]", iou[1]), ("max_gap", max_gap), ("predict", predict), ("max_tracks", max_tracks)):
        if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
            raise ValueError(f"{what}: {name} = {v} must be an integer")
        par.append(int(v))
    t0a = _np.asarray([t0] * S if _np.ndim(t0) == 0 else t0)
    if t0a.dtype.kind not in "iu" or t0a.shape != (S,) or t0a.min() < -2 ** 31 or t0a.max() >= 2 ** 31:
        raise ValueError(f"{what}: t0 must be an integer, or one per video, got {t0}")
    cat = lambda x: wh.contiguous(x[0] if len(x) == 1 else wh.cat(x))  # noqa: E731
    return cat(bl), cat(sl), one, S, K, _np.ascontiguousarray(first.astype(_np.int32)), _np.ascontiguousarray(t0a.astype(_np.int32)), par


def _link_boxes_split(ids, tracks, stats, state, one, first):
    """`link_boxes`' tables in the caller's form: one video without the leading axis, several with ids as one view per video."""
    if one:
        return ids, tracks[0], stats[0], state[0]
    return [ids[first[s]:first[s + 1]] for s in range(len(first) - 1)], tracks, stats, state


def link_boxes(boxes, stats, iou=(3, 10), max_gap: int = 2, predict: int = 1, max_tracks: int = 1024, state=None, t0=0, out=None):
    """The boxes of successive frames linked into trajectories, on the device (fusg_link_boxes: one launch on the current stream,
    one workgroup per video, nothing read back; csrc/track_boxes.h states the definition): a track is live while it was seen
    within the last max_gap + 1 frames; its expected box is its last one, with predict = 1 moved on by its centre's velocity; in a
    frame the pairs (live track, box) whose intersection over union is at least iou = (numerator, denominator) are matched best
    first, ties to the smaller track id and then the smaller box index; a matched box takes its track's id, the others found new
    tracks.  The defaults are tried on synthetic scenes only.
    boxes, stats: `foreground_boxes`' int32 [T, K, 4] and [T, 4] of ONE video's successive frames, or a list of such pairs' halves
    for several videos (ragged, the same K, at most 64).  t0: the frame index of the first frame (one for all or one per video).
    state: None to start the videos, or the state an earlier call returned to go on after its last frame (then pass that call's
    tracks in out too: the rows of tracks that have died are not written again).  out = (ids [frames, K], tracks [S, max_tracks,
    4], stats [S, 4]) to write into.
    -> (ids int32 [T, K], -1 where there is no box or none could be given; tracks int32 [max_tracks, 4] = (first_t, last_t, hits,
    0); stats int32 [4] = `LINK_BOXES_STATS`, flags `LINK_BOXES_*`; state int32 [`LINK_BOXES_STATE_WORDS`]) on the device - for a
    list, ids is a list of views and the others gain a leading axis S."""
    return _link_boxes(_DEV, boxes, stats, iou, max_gap, predict, max_tracks, state, t0, out)


def link_boxes_host(boxes, stats, iou=(3, 10), max_gap: int = 2, predict: int = 1, max_tracks: int = 1024, state=None, t0=0, out=None):
    """`link_boxes` on the CPU by the same code (fusg_link_boxes_host; no GPU needed): int32 numpy tables in and out.  A state that
    is passed in is updated in place."""
    return _link_boxes(_HOST, boxes, stats, iou, max_gap, predict, max_tracks, state, t0, out)


def _link_boxes(wh, boxes, stats, iou, max_gap, predict, max_tracks, state, t0, out):
    what = "link_boxes" + wh.tag
    b, st, one, S, K, first, t0a, par = _link_boxes_args(wh.arrays(boxes), wh.arrays(stats), iou, max_gap, predict, max_tracks, t0, wh, what)
    if not wh.near(st, b):
        raise ValueError(f"{what}: stats is on {st.device}, boxes on {b.device}")
    N, F = par[4], int(first[-1])
    if not 1 <= N <= 2 ** 20:
        raise ValueError(f"{what}: max_tracks = {N} (1..{2 ** 20})")
    shapes = ((F, K), (S, N, 4), (S, 4))
    if out is not None and not all(_fits(wh, o, wh.i32, s, b) for o, s in zip(out, shapes)):
        raise ValueError(f"{what}: out must be contiguous int32 {wh.noun}s of {shapes}{wh.at(b)}")
    if state is not None and not _fits(wh, state, wh.i32, (S, LINK_BOXES_STATE_WORDS), b) \
            and not (one and _fits(wh, state, wh.i32, (LINK_BOXES_STATE_WORDS,), b)):
        raise ValueError(f"{what}: state must be a contiguous int32 {wh.noun} of {(S, LINK_BOXES_STATE_WORDS)}{wh.at(b)}")
    with wh.side(b, "boxes") as up:
        if state is None:
            state = wh.zeros((S, LINK_BOXES_STATE_WORDS), wh.i32, b)
        ids, tracks, ost = out if out is not None else (wh.empty(shapes[0], wh.i32, b), wh.zeros(shapes[1], wh.i32, b),
                                                        wh.empty(shapes[2], wh.i32, b))
        _call(wh, what, "fusg_link_boxes", wh.ptr(up(b)), wh.ptr(up(st)), first.ctypes.data, t0a.ctypes.data, S, K, *par,
              wh.ptr(up(state)), wh.ptr(ids), wh.ptr(tracks), wh.ptr(ost))
    return _link_boxes_split(ids, tracks, ost, state.reshape(S, -1), one, first)


# ---------------------------------------------------------------------------------------------
# profiler hooks (bench.py roofline leg)
# ---------------------------------------------------------------------------------------------
def prof_enable(on: bool) -> None:
    L.lib().fusg_prof_enable(1 if on else 0)


def prof_reset() -> None:
    L.lib().fusg_prof_reset()


def prof_read(kind: int = 0):
    ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
    L.check(L.lib().fusg_prof_read(kind, C.byref(ms), C.byref(n), C.byref(fl)), "prof_read")
    return ms.value, n.value, fl.value
