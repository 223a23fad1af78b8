"""Batched, shardable driver of the per-vehicle hot path (replaces the reference's vehicle-serial,
batch-1 loop of trajectory_inference.py:55-250 for the network part).

One *crop* = one first-frame pass for one vehicle:
    hourglass heat-maps + argmax  ->  ICN completion  ->  VUnet enc_up/enc_down/dec_up/dec_down
    [-> EdgeGenerator -> InpaintGenerator with ``inpaint=True``]
Vehicles are independent, so a frame's vehicles are sharded contiguously over the
ranks of one node with NO collective in the data path; the only exchange is the final gather of
the rendered uint8 crops (and int32 keypoint indices) to rank 0, which pastes them in original
vehicle order (later vehicles overwrite earlier ones, trajectory_inference.py:197-198).
"""
from __future__ import annotations

import json
import os
from argparse import Namespace
from collections import OrderedDict
from typing import TYPE_CHECKING, Dict, List, Optional, Sequence, Tuple

import torch

if TYPE_CHECKING:
    from .edgeconnect.loss import VGG19

_REPO =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shard_range(n_items: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous, size-balanced shard [lo, hi) of `n_items` vehicles for `rank` of `world`."""
    base, rem = divmod(n_items, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


_GATHER_BUFS = {}


def _one_rank(group=None) -> bool:
    """No process group, or a group of one rank: the multi-rank code paths are skipped.  FUSG_DIST_FORCE=1 (test hook) keeps them for
    a group of ONE rank, so that a box with a single card executes the RCCL collectives of every sharded path (broadcast of the
    weights, gather of the crops / states, the comm-stream pipelining) with a one-rank communicator."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return True
    return dist.get_world_size(group) == 1 and os.environ.get("FUSG_DIST_FORCE") != "1"


def gather_in_order(local: torch.Tensor, n_items: int, group=None, dst: int = 0) -> Optional[torch.Tensor]:
    """Gather per-rank shards ([n_local, ...], same trailing shape) to `dst` in vehicle order.
    Works for any backend (RCCL on GPU tensors, gloo on CPU tensors).  Returns the full tensor on
    `dst`, None elsewhere.  Shards may be ragged (n_items not a multiple of the world size).
    The padded send buffer and rank `dst`'s receive buffers are allocated ONCE per (shape, dtype, device, world) and
    reused by every later call (a frame loop calls this once per pass): the result is a fresh tensor, the staging
    buffers never escape."""
    import torch.distributed as dist
    if _one_rank(group):
        return local
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    sizes = [shard_range(n_items, r, world) for r in range(world)]
    max_n = max(hi - lo for lo, hi in sizes)
    if local.is_cuda and dist.get_backend(group) == "gloo":       # rehearsal of the multi-rank path without RCCL
        local = local.cpu()
    stream_id = torch.cuda.current_stream(local.device).cuda_stream if local.is_cuda else 0     # staging buffers live on one stream
    key = (max_n, tuple(local.shape[1:]), local.dtype, str(local.device), world, rank == dst, id(group), stream_id)
    bufs = _GATHER_BUFS.get(key)
    if bufs is None:
        pad = torch.zeros((max_n,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        recv = [torch.empty_like(pad) for _ in range(world)] if rank == dst else None
        bufs = _GATHER_BUFS[key] = (pad, recv)
    pad, recv = bufs
    pad[: local.shape[0]].copy_(local)                             # (rows past a short shard keep their zeros: never read)
    dist.gather(pad, recv, dst=dst, group=group)
    if rank != dst:
        return None
    return torch.cat([recv[r][: hi - lo] for r, (lo, hi) in enumerate(sizes)], dim=0)


def broadcast_state_dicts(state_dicts: Optional[Dict[str, dict]], nets: Sequence[str] = ("hg", "icn", "vunet"),
                          src: int = 0, group=None, device=None) -> Dict[str, "OrderedDict[str, torch.Tensor]"]:
    """The start-up collective of the multi-GPU path (north_star: "RCCL ... for the broadcast of shared
    weights"): rank `src` holds the checkpoints of `nets` (state_dicts with the reference's keys), every rank returns
    identical CPU state_dicts.  The keys / shapes / dtypes are known everywhere (the schemas shipped with the package),
    so each network travels as ONE flat buffer per dtype class - a float32 blob (27 / 35 / 181 / 43 / 43 MB for hg / icn
    / vunet / edge / inpaint) and, for the hourglass, an int64 blob of the BatchNorm counters - i.e. few, large messages
    for xGMI's point-to-point links rather than one message per tensor (1174 tensors in total).  Works on any backend:
    with RCCL ("nccl") the blobs are staged on `device` (default: the current HIP device), with gloo on the host.
    Without an initialised process group (or world size 1) it returns rank src's dicts unchanged."""
    import torch.distributed as dist
    if _one_rank(group):
        assert state_dicts is not None, "broadcast_state_dicts: no process group and no state_dicts"
        return {n: state_dicts[n] for n in nets}
    rank = dist.get_rank(group)
    on_gpu = dist.get_backend(group) == "nccl"
    dev = torch.device(device) if device is not None else (torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu"))
    out = {}
    for net in nets:
        schema = load_schema(net)
        classes = {"f": [k for k, (_, dt) in schema.items() if dt.startswith("float")],
                   "i": [k for k, (_, dt) in schema.items() if not dt.startswith("float")]}
        sd = OrderedDict()
        for cls, keys in classes.items():
            if not keys:
                continue
            dtype = torch.float32 if cls == "f" else torch.int64
            numel = [int(torch.Size(schema[k][0]).numel()) for k in keys]
            if rank == src:
                assert state_dicts is not None and net in state_dicts, f"rank {src} has no state_dict for '{net}'"
                flat = torch.cat([state_dicts[net][k].detach().to("cpu", dtype).reshape(-1) for k in keys]).to(dev)
            else:
                flat = torch.empty(sum(numel), dtype=dtype, device=dev)
            dist.broadcast(flat, src=src, group=group)
            flat = flat.cpu()
            off = 0
            for k, n in zip(keys, numel):
                want = getattr(torch, schema[k][1])
                sd[k] = flat[off:off + n].view(schema[k][0]).to(want).clone()
                off += n
        out[net] = OrderedDict((k, sd[k]) for k in schema)              # the reference's key order
    return out


def load_schema(net: str):
    """state_dict schema (key -> (shape, dtype)) of one of the five reference networks, as dumped from the
    reference's own modules (tools/gen_golden.py); shipped inside the package (schemas/)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "schemas", f"schema_{net}.json")) as f:
        raw = json.load(f, object_pairs_hook=OrderedDict)
    return OrderedDict((k, (tuple(v[0]), v[1])) for k, v in raw.items())


# FUSG_PLAN_MT=1: a recorded pass is replayed by one host thread per recorded stream (fusg_plan_run_mt) instead of one thread for all
PLAN_THREADS = os.environ.get("FUSG_PLAN_MT", "0") == "1"
FRAME_PLANS = int(os.environ.get("FUSG_FRAME_PLANS", "6"))     # recorded passes kept by run_frame(replay=True), one per vehicle count

PER_VEHICLE_KEYS = ("bboxes", "masks", "src_sketch", "dst_sketch", "src_planes", "src_kp", "dst_kp", "src_vis", "dst_vis", "kp3d",
                    "vehicle_seeds")


def slice_scene(scene: Dict, lo: int, hi: int) -> Dict:
    """The scene of `run_frame` restricted to vehicles [lo, hi): per-vehicle entries sliced (views, nothing copied), frame-level
    entries (frame, background, focals, centers) shared."""
    out = dict(scene)
    for k in PER_VEHICLE_KEYS:
        if scene.get(k) is not None:
            out[k] = scene[k][lo:hi]
    if scene.get("inpaint") is not None:
        out["inpaint"] = {k: (_box_masks_of(v, range(lo, hi)) if k == "box_masks" else v[lo:hi]) for k, v in scene["inpaint"].items()}
    return out


def _box_masks_of(box_masks, keep):
    """scene['inpaint']['box_masks'] restricted to the vehicles `keep` (host indices): the ragged list of per-vehicle pieces
    indexed, a packed (buffer, offsets) pair with its offsets selected - the buffer is shared, nothing is copied."""
    import numpy as np

    from . import ops
    if not ops._is_packed_pair(box_masks):
        return [box_masks[v] for v in keep]
    buf, offs = box_masks
    idx = list(keep)
    if torch.is_tensor(offs):
        return (buf, offs.index_select(0, torch.as_tensor(idx, dtype=torch.long, device=offs.device)))
    return (buf, np.asarray(offs, dtype=np.int64)[np.asarray(idx, dtype=np.int64)])


# ---- the batched frame drivers' bookkeeping (pure Python).  What every row layout shares stands here once - the bounds of a
# group, the padded row count, "every scene carries a key or none does" - and the three layouts below (frame-major rows of one
# clip, scene-major rows of several first frames, clip-major rows of several clip tails) supply their offsets and their labels.
LATER_MAX_BATCH = 64     # rows per batched later pass: the largest batch the frame drivers run anyway (a frame of 64 vehicles)
FRAME_BATCH_MAX_FRAMES = 64   # scenes per group: what one launch of the frame-indexed glue kernels takes (fusg.h FUSG_MAX_FRAMES)


def _group_bounds(max_batch: Optional[int], max_frames: Optional[int] = None) -> Tuple[int, Optional[int]]:
    """(max_batch, max_frames) of a `*_groups` function as ints; max_batch None: LATER_MAX_BATCH.  ValueError below 1."""
    if max_batch is None:
        max_batch = LATER_MAX_BATCH
    if int(max_batch) < 1:
        raise ValueError(f"max_batch must be at least 1, got {max_batch}")
    if max_frames is not None and int(max_frames) < 1:
        raise ValueError(f"max_frames must be at least 1, got {max_frames}")
    return int(max_batch), None if max_frames is None else int(max_frames)


def _pad_defaults(replay: bool, max_batch: Optional[int], pad: Optional[bool]) -> Tuple[int, bool]:
    """(max_batch, pad) of a padded driver: max_batch None is LATER_MAX_BATCH, pad None pads when replay is on."""
    return LATER_MAX_BATCH if max_batch is None else max_batch, bool(replay) if pad is None else bool(pad)


def _all_or_none(what: str, key: str, ids: Sequence, values: Sequence, scope: str, label: str) -> bool:
    """Whether the scenes `ids` carry `key` (values[i] is not None): all of them or none - ValueError otherwise, raised in the
    name of the entry point `what`, listing the `label` (frames, scenes, (clip, frame)) without it."""
    have = [v is not None for v in values]
    if any(have) and not all(have):
        raise ValueError(f"{what}: either every scene {scope} carries {key!r} or none does "
                         f"({label} without: {[i for i, h in zip(ids, have) if not h]})")
    return any(have)


def _batch_seeds(what: str, ids: Sequence, seeds: Sequence, counts: Sequence[int], scope: str, label: str, name,
                 empty_counts: bool = False) -> Optional[List[int]]:
    """The scenes' 'vehicle_seeds' concatenated in row order (seeds[i]: a list of counts[i], or None); None when no scene
    carries seeds; ValueError (`_all_or_none`) when only some do, or when a list is not as long as its scene has vehicles
    (name(id): how the message calls that scene).  A scene without vehicles decides nothing unless empty_counts."""
    live = [(i, sd, int(n)) for i, sd, n in zip(ids, seeds, counts) if empty_counts or int(n) > 0]
    if not _all_or_none(what, "vehicle_seeds", [i for i, _, _ in live], [sd for _, sd, _ in live], scope, label):
        return None
    out: List[int] = []
    for i, sd, n in live:
        if len(sd) != n:
            raise ValueError(f"{what}: {name(i)} carries {len(sd)} vehicle_seeds for {n} vehicles")
        out.extend(int(x) for x in sd)
    return out


def _batch_inpaint(what: str, ids: Sequence, inps: Sequence, scope: str, label: str, required: bool = False) -> bool:
    """Whether the scenes `ids` carry 'inpaint' (all or none: `_all_or_none`), each entry checked with `inpaint_scene_form`
    before anything is issued (ValueError for a malformed one; required: for a missing one too - a first frame's refusal)."""
    has = _all_or_none(what, "inpaint", ids, inps, scope, label)
    for i in inps:
        if i is not None or required:
            inpaint_scene_form(i)
    return has


# ---- `run_later_frames_batched`: frame-major rows of F frames of V vehicles
def later_batch_row(f: int, v: int, V: int) -> int:
    """The row of (frame f, vehicle v) in a batched later pass: frame-major."""
    return f * V + v


def later_batch_slice(f: int, V: int) -> slice:
    """Frame f's V rows of a frame-major batch."""
    return slice(f * V, (f + 1) * V)


def later_batch_groups(F: int, V: int, max_batch: Optional[int] = None) -> List[Tuple[int, int]]:
    """The passes of F later frames of V vehicles: consecutive groups [lo, hi) of max(1, max_batch // V) frames, so that a
    pass holds at most max_batch rows - or one frame, where a single frame already has more (max_batch < V).  max_batch None:
    LATER_MAX_BATCH.  V = 0: one group (there is nothing to bound)."""
    max_batch, _ = _group_bounds(max_batch)
    if F <= 0:
        return []
    per = F if V == 0 else max(1, max_batch // V)
    return [(lo, min(F, lo + per)) for lo in range(0, F, per)]


def later_batch_seeds(seeds_per_frame: Sequence[Optional[Sequence[int]]], V: int,
                      what: str = "run_later_frames_batched") -> Optional[List[int]]:
    """The scenes' 'vehicle_seeds' (one list of V per frame, or None) concatenated in row order; None when no scene carries
    seeds; ValueError when only some do, or a list is not V long.  what: the entry point the messages name."""
    F = len(seeds_per_frame)
    return _batch_seeds(what, range(F), seeds_per_frame, [V] * F, "of the batch", "frames", lambda f: f"frame {f}", empty_counts=True)


# ---- `run_frames_batched`: scene-major rows of the first frames of several scenes
def frame_batch_groups(counts: Sequence[int], max_batch: Optional[int] = None,
                       max_frames: int = FRAME_BATCH_MAX_FRAMES) -> List[Tuple[int, int]]:
    """The passes of len(counts) scenes with counts[f] vehicles each: consecutive groups [lo, hi) packed greedily - a group is
    closed when the next scene would push it over max_batch rows or over max_frames scenes.  A scene with more than max_batch
    vehicles is a group of its own; every scene appears exactly once, in order.  max_batch None: LATER_MAX_BATCH."""
    max_batch, max_frames = _group_bounds(max_batch, max_frames)
    groups: List[Tuple[int, int]] = []
    lo, rows = 0, 0
    for f, c in enumerate(counts):
        c = int(c)
        if c < 0:
            raise ValueError(f"scene {f} has {c} vehicles")
        if f > lo and (rows + c > max_batch or f - lo >= max_frames):
            groups.append((lo, f))
            lo, rows = f, 0
        rows += c
    if len(counts) > lo:
        groups.append((lo, len(counts)))
    return groups


def frame_batch_offsets(counts: Sequence[int]) -> List[int]:
    """Row offsets of a group, scene-major: scene f's vehicles are rows offsets[f] .. offsets[f + 1] (len(counts) + 1 entries)."""
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + int(c))
    return offs


def frame_batch_pad(rows: int, max_batch: Optional[int] = None) -> int:
    """The row count a group of `rows` vehicles is padded to for a recorded pass: the next of 4, 8, 16, 32, 64, ..., capped at
    max_batch (default LATER_MAX_BATCH) - at most five shapes for the default, whatever the vehicle counts of a video.  A group
    that already exceeds max_batch (one scene with more vehicles) keeps its own count; 0 stays 0."""
    if max_batch is None:
        max_batch = LATER_MAX_BATCH
    rows, max_batch = int(rows), int(max_batch)
    if rows <= 0:
        return 0
    if rows > max_batch:
        return rows
    p = 4
    while p < rows:
        p *= 2
    return min(p, max_batch)


def frame_batch_seeds(seeds_per_scene: Sequence[Optional[Sequence[int]]], counts: Sequence[int],
                      what: str = "run_frames_batched") -> Optional[List[int]]:
    """The scenes' 'vehicle_seeds' concatenated in row order (scene-major); None when no scene that has vehicles carries seeds;
    ValueError when only some do, or a list is not as long as its scene has vehicles.  A scene without vehicles decides nothing.
    what: the entry point the messages name."""
    return _batch_seeds(what, range(len(counts)), seeds_per_scene, counts, "that has vehicles", "scenes", lambda f: f"scene {f}")


# ---- `run_later_clips_batched`: clip-major rows of the future frames of several clips
def clip_batch_offsets(frames: Sequence[int], vehicles: Sequence[int]) -> List[int]:
    """Row offsets of a group of clips with frames[c] future frames of vehicles[c] vehicles: clip c's rows are offsets[c] ..
    offsets[c + 1], frames[c] * vehicles[c] of them (len(frames) + 1 entries)."""
    if len(frames) != len(vehicles):
        raise ValueError(f"{len(frames)} frame counts for {len(vehicles)} vehicle counts")
    offs = [0]
    for c, (F, V) in enumerate(zip(frames, vehicles)):
        if int(F) < 0 or int(V) < 0:
            raise ValueError(f"clip {c} has {F} frames of {V} vehicles")
        offs.append(offs[-1] + int(F) * int(V))
    return offs


def clip_batch_row(offs: Sequence[int], vehicles: Sequence[int], c: int, f: int, v: int) -> int:
    """The row of (clip c, frame f, vehicle v): clip-major, frame-major inside a clip (offs: `clip_batch_offsets`)."""
    return int(offs[c]) + f * int(vehicles[c]) + v


def clip_batch_frame_rows(frames: Sequence[int], vehicles: Sequence[int]) -> List[int]:
    """The sum(frames) + 1 row offsets of the (clip, frame) frames in order - what the ragged paste takes: frame (c, f) owns
    rows frame_rows[k] .. frame_rows[k + 1] with k = frames[0] + ... + frames[c - 1] + f."""
    rows = [0]
    for F, V in zip(frames, vehicles):
        for _ in range(int(F)):
            rows.append(rows[-1] + int(V))
    return rows


def clip_batch_seeds(seeds_per_clip: Sequence[Sequence[Optional[Sequence[int]]]], vehicles: Sequence[int],
                     what: str = "run_later_clips_batched") -> Optional[List[int]]:
    """The scenes' 'vehicle_seeds' (seeds_per_clip[c][f]: a list of vehicles[c], or None) concatenated in row order; None when
    no scene that has vehicles carries seeds; ValueError naming the (clip, frame) offenders when only some do, or a list is not
    as long as its clip has vehicles.  A scene without vehicles decides nothing.  what: the entry point the messages name."""
    ids = [(c, f) for c, sds in enumerate(seeds_per_clip) for f in range(len(sds))]
    return _batch_seeds(what, ids, [seeds_per_clip[c][f] for c, f in ids], [vehicles[c] for c, _ in ids], "that has vehicles",
                        "(clip, frame)", lambda cf: f"clip {cf[0]} frame {cf[1]}")


def clip_batch_groups(frames: Sequence[int], vehicles: Sequence[int], max_batch: Optional[int] = None,
                      max_frames: int = FRAME_BATCH_MAX_FRAMES) -> List[Tuple[int, int, bool]]:
    """The passes of len(frames) clip tails: consecutive groups (lo, hi, oversized) of WHOLE clips packed greedily - a group is
    closed when the next clip would push it over max_batch rows (frames[c] * vehicles[c] per clip; default LATER_MAX_BATCH), over
    max_frames frames (what one ragged paste takes) or over max_frames clips (what one several-clip warp takes).  A clip that
    alone exceeds a bound is a group of its own with oversized = True: it runs through the one-clip path
    (`run_later_frames_batched`), which splits a clip by frames.  Every clip appears exactly once, in order."""
    max_batch, max_frames = _group_bounds(max_batch, max_frames)
    offs = clip_batch_offsets(frames, vehicles)                   # (ValueError for a negative count or lists of two lengths)
    groups: List[Tuple[int, int, bool]] = []
    lo, rows, fr = 0, 0, 0
    for c, F in enumerate(frames):
        r, F = offs[c + 1] - offs[c], int(F)
        big = r > max_batch or F > max_frames
        if c > lo and (big or rows + r > max_batch or fr + F > max_frames or c - lo >= max_frames):
            groups.append((lo, c, False))
            lo, rows, fr = c, 0, 0
        if big:
            groups.append((c, c + 1, True))
            lo, rows, fr = c + 1, 0, 0
            continue
        rows, fr = rows + r, fr + F
    if len(frames) > lo:
        groups.append((lo, len(frames), False))
    return groups


def later_geometry_batch_rows(scenes: Sequence[Dict], vehicles: Sequence[int], device_pose: bool, device_homography: bool,
                              inpaint: bool = False) -> Tuple[Optional[List[int]], bool]:
    """What `run_later_frames_batched_geometry` checks before it issues anything, for F geometry-mode scenes ('steps', no 'masks')
    and the first-frame indices `vehicles` of the state (pure Python).  The batched stage is the per-frame DEVICE path's
    arithmetic row by row, so it needs a pipeline built with device_pose=True and device_homography=True; 'vehicle_seeds' and
    'inpaint' list every first-frame vehicle like 'steps', and either every scene carries them or none does (`inpaint`: the
    pipeline holds the inpainting networks - without them the key is ignored).  ValueError otherwise.  Returns (the seeds of
    the F * V rows, frame-major, or None; whether the pass inpaints)."""
    what = "run_later_frames_batched_geometry"
    if not device_pose or not device_homography:
        raise ValueError(f"{what}: a geometry-mode state is batched only by a pipeline built with "
                         f"device_pose=True and device_homography=True (device_pose={bool(device_pose)}, "
                         f"device_homography={bool(device_homography)}): the batched stage is that path's arithmetic, row by row")
    veh = [int(v) for v in vehicles]
    for f, sc in enumerate(scenes):
        if "masks" in sc or sc.get("steps") is None:
            raise ValueError(f"{what}: scene {f} is not a geometry-mode scene ('steps', no 'masks')")
        for k in ("steps", "vehicle_seeds"):
            if sc.get(k) is not None and veh and len(sc[k]) <= max(veh):
                raise ValueError(f"{what}: scene {f} carries {len(sc[k])} {k!r} entries, the state's "
                                 f"vehicles reach first-frame index {max(veh)}")
    seeds = later_batch_seeds([None if sc.get("vehicle_seeds") is None else [sc["vehicle_seeds"][v] for v in veh] for sc in scenes],
                              len(veh), what)
    has = _batch_inpaint(what, range(len(scenes)), [sc.get("inpaint") if inpaint else None for sc in scenes], "of the batch", "frames")
    return seeds, has


def later_clips_geometry_batch_rows(clips: Sequence[Tuple[Sequence[Dict], Dict]], device_pose: bool, device_homography: bool,
                                    inpaint: bool = False) -> Tuple[List[int], Optional[List[int]], bool]:
    """What `run_later_clips_batched_geometry` checks before it issues anything, for (later_scenes, state) pairs of geometry-mode
    clips (pure Python apart from reading the frames' shapes): `later_geometry_batch_rows`' demands clip by clip - a pipeline built
    with device_pose=True and device_homography=True, scenes with 'steps' and without 'masks', 'steps' / 'vehicle_seeds' lists that
    reach the state's highest first-frame index -, and over the whole list: every state is a geometry-mode one (no mix with
    given-geometry clips), the frames have one size, and either every (clip, frame) whose clip has vehicles carries
    'vehicle_seeds' / 'inpaint' (`inpaint`: the pipeline holds the inpainting networks - without them the key is ignored) or none
    does.  ValueError otherwise.  Returns (vehicles per clip = the states' kept vehicles, the seeds of all rows - clip-major,
    selected to the states' vehicles: `clip_batch_seeds` - or None, whether the pass inpaints)."""
    what = "run_later_clips_batched_geometry"
    if not device_pose or not device_homography:
        raise ValueError(f"{what}: geometry-mode clips are batched only by a pipeline built with "
                         f"device_pose=True and device_homography=True (device_pose={bool(device_pose)}, "
                         f"device_homography={bool(device_homography)}): the batched stage is that path's arithmetic, row by row")
    clips = [(list(scs), st) for scs, st in clips]
    given = [c for c, (_, st) in enumerate(clips) if st.get("geometry") is None]
    if given and len(given) < len(clips):
        raise ValueError(f"{what}: the list mixes geometry-mode clips and given-geometry clips (given-geometry: {given})")
    vehs = [[int(v) for v in (st.get("geometry") or {}).get("vehicles", [])] for _, st in clips]
    for c, ((scs, _), veh) in enumerate(zip(clips, vehs)):
        for f, sc in enumerate(scs):
            if c in given or "masks" in sc or sc.get("steps") is None:
                raise ValueError(f"{what}: clip {c} scene {f} is not a geometry-mode scene ('steps', no 'masks', the state of a "
                                 "geometry-mode first frame)")
            for k in ("steps", "vehicle_seeds"):
                if sc.get(k) is not None and veh and len(sc[k]) <= max(veh):
                    raise ValueError(f"{what}: clip {c} scene {f} carries {len(sc[k])} {k!r} entries, the state's "
                                     f"vehicles reach first-frame index {max(veh)}")
    sizes = {tuple(sc["frame"].shape) for scs, _ in clips for sc in scs}
    if len(sizes) > 1:
        raise ValueError(f"{what}: the frames of one call have one size, got {sorted(sizes)}")
    vehicles = [len(veh) for veh in vehs]
    seeds = clip_batch_seeds([[None if sc.get("vehicle_seeds") is None else [sc["vehicle_seeds"][v] for v in veh] for sc in scs]
                              for (scs, _), veh in zip(clips, vehs)], vehicles, what)
    live = [(c, f) for c, (scs, _) in enumerate(clips) if vehicles[c] for f in range(len(scs))]
    has = _batch_inpaint(what, live, [clips[c][0][f].get("inpaint") if inpaint else None for c, f in live], "that has vehicles",
                         "(clip, frame)")
    return vehicles, seeds, has


def frame_geometry_batch_rows(scenes: Sequence[Dict], device_pose: bool, device_homography: bool, inpaint: bool = False,
                              classifier: bool = False) -> Tuple[List[int], Optional[List[int]], bool]:
    """What `run_frames_batched_geometry` checks before it issues anything, for geometry-mode first frames ('frame', 'bboxes',
    'focals', 'centers', no 'masks'; pure Python apart from reading the frames' shapes).  The batched stage is the per-frame DEVICE
    path's arithmetic row by row, so it needs a pipeline built with device_pose=True and device_homography=True; the frames have
    one size; either every scene that has vehicles carries 'vehicle_seeds' or none does, and with the inpainting networks
    (`inpaint`) the same holds for 'inpaint'; without a CAD classifier every scene that has vehicles carries 'cad_idx' [V_f].
    ValueError otherwise.  Returns (vehicles per scene, the seeds of all rows scene-major or None, whether the pass inpaints)."""
    import numpy as np
    if not device_pose or not device_homography:
        raise ValueError("run_frames_batched_geometry: geometry-mode first frames are batched only by a pipeline built with "
                         f"device_pose=True and device_homography=True (device_pose={bool(device_pose)}, "
                         f"device_homography={bool(device_homography)}): the batched stage is that path's arithmetic, row by row")
    for f, sc in enumerate(scenes):
        if "masks" in sc:
            raise ValueError(f"run_frames_batched_geometry: scene {f} is not a geometry-mode scene (it carries 'masks')")
    sizes = {tuple(sc["frame"].shape) for sc in scenes}
    if len(sizes) > 1:
        raise ValueError(f"run_frames_batched_geometry: the frames of one call have one size, got {sorted(sizes)}")
    counts = [int(np.asarray(sc["bboxes"]).reshape(-1, 4).shape[0]) for sc in scenes]
    seeds = frame_batch_seeds([sc.get("vehicle_seeds") for sc in scenes], counts, "run_frames_batched_geometry")
    live = [(f, sc) for f, (sc, c) in enumerate(zip(scenes, counts)) if c > 0]
    has_inpaint = bool(inpaint) and _batch_inpaint("run_frames_batched_geometry", [f for f, _ in live], [sc.get("inpaint") for _, sc in live],
                                             "that has vehicles", "scenes", required=True)
    if not classifier:
        for f, sc in live:
            if sc.get("cad_idx") is None:
                raise ValueError(f"geometry mode: scene {f} needs 'cad_idx' [V] (or a pipeline built with cad=True)")
            if int(np.asarray(sc["cad_idx"]).reshape(-1).shape[0]) != counts[f]:
                raise ValueError(f"run_frames_batched_geometry: scene {f} carries {int(np.asarray(sc['cad_idx']).reshape(-1).shape[0])} "
                                 f"'cad_idx' entries for {counts[f]} vehicles")
    return counts, seeds, has_inpaint


def _tensors(o):
    """Every tensor inside a nested dict / list / tuple, depth first."""
    if torch.is_tensor(o):
        yield o
    elif isinstance(o, dict):
        for v in o.values():
            yield from _tensors(v)
    elif isinstance(o, (list, tuple)):
        for v in o:
            yield from _tensors(v)


def _redo_f32(fn, rng_state=None, restore: bool = False):
    """fn() again in exact fp32, after a pass whose split-fp16 range status came back raised: under `rng_state` (the host
    RNG state the pass was first issued under; None: it draws no global noise).  restore=True puts the RNG state of NOW back
    afterwards - the pipelined drivers, whose next frame has already drawn its noise."""
    from . import ops
    cur = torch.get_rng_state() if (restore and rng_state is not None) else None
    if rng_state is not None:
        torch.set_rng_state(rng_state)
    with ops.defer_range_check(), ops.precision("f32"):
        out = fn()
    if cur is not None:
        torch.set_rng_state(cur)
    return out


class VehiclePipeline:
    """Holds the five networks on one device and runs batches of crops through them."""

    def __init__(self, device, inpaint: bool = False, state_dicts: Optional[Dict[str, dict]] = None, seed: int = 0,
                 broadcast_src: Optional[int] = None, group=None, cad: bool = False, cad_bank=None,
                 device_homography: bool = False, device_pose: bool = False, *, route_batch: Optional[int] = None):
        """state_dicts: checkpoints (the reference's keys) per network; a missing network gets the synthetic weights of
        `seed`; the VUnet is built in the configuration its checkpoint's keys show (`vunet.models.vunet_args_of`).  broadcast_src: with an initialised process group, only that rank needs to hold `state_dicts` (a real
        checkpoint read from disk on rank 0): they are distributed with `broadcast_state_dicts` first (north_star: RCCL
        broadcast of the shared weights), so every rank renders with identical parameters.
        cad: also hold the reference's CAD-model classifier (VGG-19, 10 classes; state_dicts['vgg'] = `cads/model.pth`,
        run_test.py:47-58) and run it on the hourglass's crop in every pass (trajectory_inference.py:66-69): 'cad_logits' /
        `run_frame`'s 'cad_idx'.  Not part of BASELINE's crop pass: `bench.py` leaves it off.
        cad_bank: a `render.CadBank` - enables the geometry mode of `run_frame` / `run_later_frame` (a scene without 'masks':
        the sketches, masks, planes and visibilities are rendered on the device from the fitted pose).
        device_homography: the frame drivers gate the planes and fit their homographies on the device
        (`planes_utils.plane_homographies_device` + `warp_planes_fitted`) instead of on the host (`warp_jobs_frame` +
        `warp_planes_batch`, the default and the reference-signature path).
        device_pose: geometry mode selects the fitted pose and derives its geometry - extrinsic, render jobs, visibility
        polygons, plane corner points - on the device (`render.vehicle_geometry_device`, fusg_pose_geometry) instead of in numpy
        between three read-backs (`render.vehicle_geometry`, the default): a frame's front stage then issues every launch through
        the plane cut-outs around ONE blocking device-to-host copy of the small results.  With device_homography as well the
        corner points reach the homography fit as device tensors.
        route_batch (keyword only): the routing batch (`ops.set_route_batch`) in force around every pass this pipeline issues - eager passes,
        recordings and their replays, the range guard's fp32 redo; None: whatever the process has set (off by default).  Every
        routing decision is then made as if the launch held `route_batch` images.  Contract: with route_batch set, one precision
        and `vehicle_seeds` given, the network outputs of a row ('kp_idx', 'icn_u8', 'vunet_u8', 'inpaint_u8', the appearance
        codes) are bit-identical whatever the batch size (1 ... 64), the row's position in the batch, the zero padding rows of
        a padded replay and the driver (`run`, `run_frame`, `run_frames_batched`, `run_later_frames_batched`,
        `run_later_clips_batched`).  One exception: a raised range status redoes the WHOLE pass in exact fp32, so a row's bits
        still depend on whether a neighbour overflowed.  Without `vehicle_seeds` the VUnet's noise stays batch-shaped as in the
        reference.  The recorded plans are kept per routing batch: a replay never mixes routings.  Pick a value near the typical
        batch of a pass (the cost of a routing batch far from the real one)."""
        if route_batch is not None and not 0 <= int(route_batch) <= (1 << 20):
            raise ValueError(f"route_batch {route_batch} is outside 0 (off) .. 2**20")
        self.route_batch = None if route_batch is None else int(route_batch)
        from .edgeconnect.models import EdgeModel, InpaintingModel
        from .stacked_hourglass.models import HourglassNet
        from .synth import synth_state_dict
        from .vunet.models import Vunet_fix_res, vunet_args_of
        from .warp_learn.models import G_Resnet
        self.device = torch.device(device)
        self.inpaint = inpaint
        self.group = group
        self.cad = None
        self.cad_bank = cad_bank
        self.device_homography = bool(device_homography)
        self.device_pose = bool(device_pose)
        if broadcast_src is not None:
            import torch.distributed as dist
            if not _one_rank(group):
                nets_ = ("hg", "icn", "vunet") + (("edge", "inpaint") if inpaint else ())
                coll_dev = self.device if dist.get_backend(group) == "nccl" else "cpu"
                state_dicts = broadcast_state_dicts(state_dicts if dist.get_rank(group) == broadcast_src else None,
                                                    nets=nets_, src=broadcast_src, group=group, device=coll_dev)

        def sd(net):
            if state_dicts is not None and net in state_dicts:
                return state_dicts[net]
            return synth_state_dict(net, load_schema(net), seed)

        self.hg = HourglassNet(num_stacks=2, num_blocks=1, num_classes=12)             # run_test.py:62
        self.icn = G_Resnet(21)                                                         # run_test.py:74
        # the VUnet the checkpoint was trained as (run_test.py:82 and the synthetic weights: subpixel, w_norm, 256; a
        # state_dicts['vunet'] of another --up_mode / w_norm / resolution builds that network)
        vunet_sd = sd("vunet")
        self.vunet = Vunet_fix_res(vunet_args_of(vunet_sd))
        self.hg.load_state_dict(sd("hg"))
        self.icn.load_state_dict(sd("icn"))
        self.vunet.load_state_dict(vunet_sd)
        nets = [self.hg, self.icn, self.vunet]
        if inpaint:
            self.edge, self.inp = EdgeModel(None), InpaintingModel(None)
            self.edge.generator.load_state_dict(sd("edge"))
            self.inp.generator.load_state_dict(sd("inpaint"))
            nets += [self.edge, self.inp]
        if cad:
            from .cad_classifier import VGG19Classifier, vgg19_schema
            self.cad = VGG19Classifier(10)
            self.cad.load_state_dict(state_dicts["vgg"] if state_dicts is not None and "vgg" in state_dicts
                                     else synth_state_dict("vgg", vgg19_schema(10), seed))
            nets.append(self.cad)
        for n in nets:
            n.to(self.device).eval()
        # the FusedNets whose packed-weight caches a recorded pass points into (EdgeModel / InpaintingModel wrap theirs)
        self._nets = [getattr(n, "generator", n) for n in nets]
        self._status = None                       # this pipeline's own range-status word (ops.status_scope), made on first use
        # made on first use: the branch streams of `_branches`; the geometry stage's stream and status word; the sharded
        # drivers' communication stream
        self._streams, self._geo_stream, self._geo_status, self._comm_stream = {}, None, None, None
        self._pins = []                           # free pinned int32 status words of the in-flight stages (`_issue_guarded`)
        self._frame_pins = []                     # free pinned triples for a frame's raw pose arrays (`_issue_frame`)
        self._frame_plans = {}                    # recorded passes of the frame drivers, least recently used first (`_replay`)

    # The networks of one crop pass do not depend on each other (hourglass / ICN / VUnet; edge -> inpaint is one
    # chain), so each branch runs on its own HIP stream: the many small, latency-bound launches of the hourglass
    # and of the VUnet's low-resolution levels fill the CUs the big ICN layers leave idle between their waves of
    # workgroups.  The VUnet - the longest chain of dependent launches - gets a high-priority stream, so that its
    # small kernels never queue behind the ICN's big ones (measured 1180 -> 1260 crops/s).
    # FUSG_STREAMS=0 serialises everything on the caller's stream.
    HIGH_PRIORITY = ("vunet",)

    def _branches(self, jobs):
        """jobs: list of (name, zero-argument callable returning a dict of output tensors); the first one runs on
        the caller's stream."""
        out = {}
        if os.environ.get("FUSG_STREAMS", "1") == "0" or self.device.type != "cuda" or len(jobs) == 1:
            for _, j in jobs:
                out.update(j())
            return out
        from . import ops
        rec = ops.RECORDER                                  # recording a fusg_plan: dependencies go through it
        main = torch.cuda.current_stream(self.device)
        pool = self._streams
        streams = []
        for name, _ in jobs[1:]:
            st = pool.get(name)
            if st is None:
                st = pool[name] = torch.cuda.Stream(device=self.device, priority=-1 if name in self.HIGH_PRIORITY else 0)
            streams.append(st)
        # fork: the side branches may start as soon as what is on the caller's stream NOW is done (not after branch 0)
        if rec is None:
            ready = torch.cuda.Event()
            ready.record(main)
            for st in streams:
                st.wait_event(ready)
        else:
            for st in streams:
                rec.dependency(st.cuda_stream, main.cuda_stream)
        used = []
        for i, (name, j) in enumerate(jobs):
            if i == 0:
                out.update(j())
                continue
            st = streams[i - 1]
            with torch.cuda.stream(st):
                res = j()
            for t in res.values():
                t.record_stream(main)
            out.update(res)
            used.append(st)
        for st in used:
            if rec is None:
                main.wait_stream(st)
            else:
                rec.dependency(main.cuda_stream, st.cuda_stream)
        return out

    def _side(self, name: str, fn):
        """Run fn() on the side stream `name`, forked from the CURRENT stream (what is queued there now is finished
        before fn's launches start); returns (fn's result, join): join() makes the current stream wait for the side
        stream.  Used for the VUnet's two independent encoders: the shape encoder (forward_dec_up) does not depend
        on the appearance half (forward_enc_up -> forward_enc_down), so the VUnet's chain of dependent launches - the
        longest of the pass - is a third shorter.  FUSG_VUNET_SPLIT=0 (or FUSG_STREAMS=0) keeps one stream."""
        from . import ops
        if not ops.side_streams_enabled() or self.device.type != "cuda":
            return fn(), (lambda: None)
        st = ops.side_stream(name, self.device)
        ops.fork_to(st)
        with torch.cuda.stream(st):
            res = fn()
        return res, (lambda: ops.join_from(st, list(_tensors(res))))

    def compile(self, batch: Dict[str, torch.Tensor], vehicle_seeds: Optional[Sequence[int]] = None, fn=None) -> "CompiledPass":
        """Record one crop pass for inputs of `batch`'s shapes into a fusg_plan and return the object that replays it:
        `compiled.run(batch, vehicle_seeds)` gives what `self.run` gives, with one library call instead of ~370 (the
        reference's batch-1 call pattern is bound by the interpreter, not by the GPU).  `fn(batch, vehicle_seeds) -> dict of
        tensors`: record that pass instead of `self._run` (e.g. `self._vunet_forward`: BASELINE configs[0])."""
        return CompiledPass(self, batch, vehicle_seeds, fn)

    @torch.no_grad()
    def _vunet_forward(self, batch, vehicle_seeds=None):
        """BASELINE configs[0]: `Vunet_fix_res.forward(y_tilde, x)` alone (vunet/models.py:461-481, mean_appearance: the
        decoder is conditioned on the SAMPLED appearance code z_app, :476).  batch: 'vu_y' [B,3,R,R], 'vu_x' [B,6,R,R]."""
        from . import ops
        vu = self.vunet
        vu.set_vehicle_seeds(vehicle_seeds)
        # forward()'s four calls (:472-476) with the shape encoder - which draws no noise and depends on nothing else - on
        # the side stream, as in `_run`: same launches, same noise order, same bits as `self.vunet.forward(y_tilde, x)`
        (do, ds), join = self._side("vunet_shape", lambda: vu.forward_dec_up(batch["vu_y"]))
        eo, es = vu.forward_enc_up(batch["vu_x"])
        mu_app, z_app = vu.forward_enc_down(eo, es)
        join()
        xt, mu_shape, _ = vu.forward_dec_down(do, ds, z_app)
        return {"x_tilde": xt, "vunet_u8": ops.to_image_u8(xt), "mu_app_0": mu_app[0], "mu_app_1": mu_app[1],
                "mu_shape_0": mu_shape[0], "mu_shape_1": mu_shape[1]}

    def vunet_forward(self, batch, vehicle_seeds=None, check: Optional[str] = "sync"):
        """`_vunet_forward` under the pipeline's range guard (see `run`)."""
        rng = torch.get_rng_state() if (vehicle_seeds is None and check == "sync") else None
        return self._guarded(self._vunet_forward, (batch, vehicle_seeds), check, rng)

    # Range guard of the split-fp16 contraction (ops.py): the networks' own per-call checks are deferred while a pass
    # is being issued (they would synchronise the host once per network and undo the stream overlap); the pass is
    # checked as a whole instead.  check="sync" (default): read the status word after the pass and, if an operand
    # left the split's range, redo the pass in exact fp32 - the returned tensors are always valid.  check="async":
    # return without synchronising (the caller keeps issuing passes); the status word is sticky, and `finish()`
    # says whether any pass since the last call was affected - call it before consuming outputs.
    def status_word(self) -> torch.Tensor:
        """The range-status word this pipeline's passes report to - its own, not the device-wide one the module entry
        points read and clear: an entry-point call between async passes and `finish()` can neither clear nor inherit
        a flag raised by those passes."""
        from . import ops
        if self._status is None:
            self._status = ops.new_status_word(self.device)
        return self._status

    def _routed(self):
        """The context every pass of this pipeline is issued in: its routing batch (`route_batch`; None: the process's)."""
        from . import ops
        return ops.route_batch(self.route_batch)

    def _guarded(self, fn, args, check: str, rng_state):
        from . import ops
        with self._routed():
            if not ops.range_guarded() or check is None:
                return fn(*args)
            word = self.status_word()
            with ops.defer_range_check(), ops.status_scope(word):
                out = fn(*args)
            if check == "async":
                return out
            with torch.cuda.device(self.device):
                hit = ops.range_exceeded(self.device, word=word)
            if not hit:
                return out
            return _redo_f32(lambda: fn(*args), rng_state)

    def finish(self) -> bool:
        """Synchronise the device and report (and clear) the range status of the passes issued with check="async":
        True = some pass staged an operand outside the split-fp16 range; its outputs must be recomputed
        (under `ops.precision`, in exact fp32)."""
        from . import ops
        torch.cuda.synchronize(self.device)
        if not ops.range_guarded():
            return False
        with torch.cuda.device(self.device):
            return ops.range_exceeded(self.device, word=self.status_word())

    def run(self, batch: Dict[str, torch.Tensor], vehicle_seeds: Optional[Sequence[int]] = None,
            check: Optional[str] = "sync") -> Dict[str, torch.Tensor]:
        """batch: 'hg_x' [B,3,R,R], 'icn_x' [B,21,R,R], 'vu_x' [B,6,R,R], 'vu_y' [B,3,R,R]
        (+ 'ec_img','ec_gray','ec_edge','ec_mask' with inpaint).  All device-resident.
        Returns 'kp_idx' int32 [B,12], 'icn_u8' / 'vunet_u8' uint8 [B,R,R,3] (+ 'inpaint_u8').
        vehicle_seeds: one VUnet noise seed per sample (e.g. base + global vehicle index) - makes the result of
        a vehicle independent of how the vehicles are sharded over ranks; None = the reference's global RNG.
        check: range guard of the split-fp16 path, see `_guarded`."""
        rng = torch.get_rng_state() if (vehicle_seeds is None and check == "sync") else None
        return self._guarded(self._run, (batch, vehicle_seeds), check, rng)

    # ------------------------------------------------------------------------------------------ quality of one pass against another
    COMPARED_IMAGES = ("icn_u8", "vunet_u8", "inpaint_u8")

    def compare_outputs(self, a: Dict[str, torch.Tensor], b: Dict[str, torch.Tensor], *, features: Optional[VGG19] = None) -> Dict:
        """Per-row quality of two output dicts of `run` (or of a frame driver) against each other, measured on the device
        (`ops.image_metrics_u8`: SSIM as the project's quality bars define it, PSNR, difference counts) and read back in ONE
        `ops.d2h`.  Compared: every key of `COMPARED_IMAGES` both dicts hold as uint8 [N, R, R, 3] of one shape, and 'kp_idx'.
        Returns {key: {'ssim' float64 [N], 'psnr' float64 [N], 'max_abs' int64 [N], 'n_diff' int64 [N]}, 'kp_equal' int64 [N]
        (equal keypoints per row, with 'kp_idx' in both), 'worst': {key: {'ssim': the smallest, 'max_abs': the largest, 'row':
        the row of the smallest ssim}}} as numpy arrays / Python scalars.
        features: an `edgeconnect.loss.VGG19` (the user's torchvision checkpoint loaded into it, on this device).  With it every
        compared image key also gets 'perceptual' (sum of the five PerceptualLoss terms) and 'style' (sum of the four StyleLoss
        terms) as float64 [N] (`edgeconnect.loss.feature_distances` on the crops / 255, same read-back; NaN where the split-fp16
        range guard fired), and 'worst'[key] gains 'perceptual': {'value': the largest, 'row': its row}.  R must be a
        multiple of 16."""
        import numpy as np
        from . import ops

        def is_image(t):
            return torch.is_tensor(t) and t.dtype == torch.uint8 and t.dim() == 4 and t.shape[-1] == 3

        keys = [k for k in self.COMPARED_IMAGES if is_image(a.get(k)) and is_image(b.get(k)) and a[k].shape == b[k].shape]
        kp = "kp_idx" in a and "kp_idx" in b and a["kp_idx"].shape == b["kp_idx"].shape
        if not keys and not kp:
            raise ValueError("compare_outputs: the two dicts share no uint8 [N, R, R, 3] image and no 'kp_idx'")
        N = int((a[keys[0]] if keys else a["kp_idx"]).shape[0])
        ncol = len(ops.IMAGE_METRIC_COLUMNS)
        with torch.cuda.device(self.device):
            cols = [ops.image_metrics_u8(a[k], b[k]) for k in keys]
            if features is not None:
                from .edgeconnect.loss import FEATURE_DISTANCE_COLUMNS, PERCEPTUAL_TAPS, feature_distances
                nfeat, nperc = len(FEATURE_DISTANCE_COLUMNS), len(PERCEPTUAL_TAPS)
                cols += [feature_distances(features, a[k], b[k]) for k in keys]
            if kp:                                                # the indices themselves (exact in float64): compared on the host
                cols += [a["kp_idx"].reshape(N, -1).to(torch.float64), b["kp_idx"].reshape(N, -1).to(torch.float64)]
            host = ops.d2h(torch.cat(cols, dim=1))
        col = {n: i for i, n in enumerate(ops.IMAGE_METRIC_COLUMNS)}
        res: Dict = {"worst": {}}
        for i, k in enumerate(keys):
            t = host[:, i * ncol:(i + 1) * ncol]
            res[k] = {"ssim": t[:, col["ssim"]].copy(), "psnr": t[:, col["psnr"]].copy(),
                      "max_abs": t[:, col["max_abs"]].astype(np.int64), "n_diff": t[:, col["n_diff"]].astype(np.int64)}
            if N:
                row = int(np.argmin(res[k]["ssim"]))
                res["worst"][k] = {"ssim": float(res[k]["ssim"][row]), "max_abs": int(res[k]["max_abs"].max()), "row": row}
        n_img = len(keys) * ncol                                  # columns ahead of the keypoints
        if features is not None:
            for i, k in enumerate(keys):
                t = host[:, n_img + i * nfeat:n_img + (i + 1) * nfeat]
                res[k]["perceptual"], res[k]["style"] = t[:, :nperc].sum(axis=1), t[:, nperc:].sum(axis=1)
                if N:
                    row = int(np.argmax(res[k]["perceptual"]))
                    res["worst"][k]["perceptual"] = {"value": float(res[k]["perceptual"][row]), "row": row}
            n_img += len(keys) * nfeat
        if kp:
            n_kp = (host.shape[1] - n_img) // 2
            ka, kb = host[:, n_img:n_img + n_kp], host[:, n_img + n_kp:]
            res["kp_equal"] = (ka == kb).sum(axis=1).astype(np.int64)
        return res

    def compare_precisions(self, batch: Dict[str, torch.Tensor], vehicle_seeds: Sequence[int], precision: str = "bf16",
                           against: str = "f16x3", check: Optional[str] = "sync", *, features: Optional[VGG19] = None) -> Dict:
        """`run(batch, vehicle_seeds)` once under `against` and once under `precision` (`ops.precision`, restored afterwards;
        this pipeline's routing batch in force around both), then `compare_outputs` of the two: what a faster arithmetic costs
        on the caller's own weights and crops, in the unit the quality bars are stated in.  The acceptance recipe for bf16:
        `rep = pipe.compare_precisions(batch, seeds, "bf16"); assert rep["worst"]["icn_u8"]["ssim"] >= 0.999`; the same
        recipe with "f16" measures the single-pass fp16 mode (11 significant bits per operand where bf16 keeps 8).
        vehicle_seeds is required: without it the two passes draw different VUnet noise and the comparison means nothing.
        features: as in `compare_outputs` (the feature-space distances of the two passes' crops, measured at the ambient
        precision, not at `precision`)."""
        from . import ops
        if vehicle_seeds is None:
            raise ValueError("compare_precisions: vehicle_seeds is required (without seeds the two passes draw different noise)")
        for p in (precision, against):
            if p not in ops._PREC:
                raise ValueError(f"compare_precisions: precision must be one of {list(ops._PREC)}, got {p!r}")
        with self._routed():
            with ops.precision(against):
                ref = self.run(batch, vehicle_seeds, check)
            with ops.precision(precision):
                out = self.run(batch, vehicle_seeds, check)
            return self.compare_outputs(out, ref) if features is None else self.compare_outputs(out, ref, features=features)

    def _no_vehicles(self, R: int, *keys) -> Dict[str, torch.Tensor]:
        """The named per-vehicle outputs for zero vehicles (a frame without vehicles, a rank whose shard is empty)."""
        u8 = ((0, R, R, 3), torch.uint8)
        kinds = {"kp_idx": ((0, 12), torch.int32), "geom": ((0, 8), torch.int32), "icn_u8": u8, "vunet_u8": u8, "inpaint_u8": u8,
                 "central": u8, "cad_logits": ((0, 10), torch.float32), "cad_idx": ((0,), torch.int64),
                 "mu_app_0": ((0, 128, R // 64, R // 64), torch.float32), "mu_app_1": ((0, 128, R // 32, R // 32), torch.float32)}
        return {k: torch.empty(kinds[k][0], dtype=kinds[k][1], device=self.device) for k in keys}

    @torch.no_grad()
    def _run(self, batch, vehicle_seeds):
        from . import ops
        B, R = batch["hg_x"].shape[0], batch["hg_x"].shape[-1]
        if B == 0:                                                # a rank whose shard is empty (fewer vehicles than ranks)
            return self._no_vehicles(R, "kp_idx", "icn_u8", "vunet_u8", *(("inpaint_u8",) if self.inpaint else ()),
                                     *(("cad_logits",) if self.cad is not None else ()))
        self.vunet.set_vehicle_seeds(vehicle_seeds)

        def hg():
            if "kp_idx" in batch:                                 # geometry mode: the hourglass ran before the render
                return {k: batch[k] for k in ("kp_idx", "cad_logits") if k in batch}
            out = {"kp_idx": ops.argmax_hw(self.hg(batch["hg_x"])["heatmaps"][-1])}
            if self.cad is not None:                              # same crop, same branch (:66-69): a stream of its own costs more
                out["cad_logits"] = self.cad(batch["hg_x"])
            return out

        def icn():
            return {"icn_u8": ops.to_image_u8(self.icn(batch["icn_x"]))}

        def vunet():
            vu = self.vunet
            # trajectory_inference.py:230-233; the shape encoder runs beside the appearance half (it draws no noise,
            # so the host-side draw order is the reference's either way)
            (do, ds), join = self._side("vunet_shape", lambda: vu.forward_dec_up(batch["vu_y"]))
            eo, es = vu.forward_enc_up(batch["vu_x"])
            mu_app, _ = vu.forward_enc_down(eo, es)
            join()
            xt, _, _ = vu.forward_dec_down(do, ds, mu_app)
            # (the appearance code is what a vehicle's FUTURE frames are rendered with, :424-426: run_frame hands it out)
            return {"vunet_u8": ops.to_image_u8(xt), "mu_app_0": mu_app[0], "mu_app_1": mu_app[1]}

        def inpaint():
            e = self.edge(batch["ec_gray"], batch["ec_edge"], batch["ec_mask"])      # :124-129
            p = self.inp(batch["ec_img"], e, batch["ec_mask"])
            return {"inpaint_u8": ops.merge_u8(p, batch["ec_img"], batch["ec_mask"])}

        # the ICN's big launches are issued first, on the caller's stream
        return self._branches([("icn", icn), ("vunet", vunet), ("hg", hg)] + ([("inpaint", inpaint)] if self.inpaint else []))

    # ------------------------------------------------------------------------------------------ per-frame chain
    def run_frame(self, scene: Dict, check: Optional[str] = "sync", replay: bool = False) -> Dict:
        """One frame's vehicles from detector boxes to the two composited frames, device-resident: the reference's
        per-vehicle order (trajectory_inference.py:55-250, first frame) batched over the V vehicles of the frame:

            box crop -> hourglass -> argmax -> keypoints in frame pixels -> pose fit (4 LM starts per vehicle)
            plane warp (homographies fitted on the host) -> ICN inputs -> ICN -> to_image(from_LAB=True)
            VUnet inputs -> VUnet first-frame -> to_image
            resize-back + masked paste of every vehicle, in vehicle order (later vehicles overwrite earlier ones)

        scene (see `synth_frame`): 'frame' uint8 [H, W, 3] (CUDA); 'bboxes' int [V, 4] (host: the detector's boxes);
        'masks' uint8 [V, H, W] (CUDA, non-zero = vehicle: the rendered sketch mask, the reference's ~sketch_mask);
        'src_sketch' / 'dst_sketch' uint8 [V, H, W, 3]; 'src_planes' uint8 [V, 5, H, W, 3]; 'src_kp' / 'dst_kp' host lists
        [V][5] of int32 [n, 2] plane corner points; 'src_vis' / 'dst_vis' host [V, 5]; 'kp3d' float32 [V, 12, 3] (host: the
        CAD model's keypoints); 'focals' / 'centers' [2] (host); optional 'background' uint8 [H, W, 3] (default: the frame).
        What the reference computes BETWEEN the pose fit and the plane warp - rendering the posed CAD model into sketches,
        masks and plane corner points with Open3D (warp_learn/vehicle_utils.py) - is out of scope: those
        are inputs here, and the pose is an output for that renderer.  A pipeline built with inpaint=True also takes
        'inpaint' = {'boxes' host int [V, 4] (bbox_new_img: the 1.3x detector box clipped to the frame), 'img' float32
        [V, 3, R, R], 'gray' / 'edge' / 'mask' float32 [V, 1, R, R] in [0, 1]} - what create_inpaint_inputs_shape hands
        EdgeConnect (utils/inpaint_utils.py:35-58) - or 'inpaint' = {'boxes', 'det_masks' uint8 [V, 1, H, W]}, the detector's
        (Mask R-CNN's, out of scope) masks in frame coordinates, from which dilation, whitening, resize, gray and Canny build
        the four tensors on the device (`ops.inpaint_inputs`, on the inpaint branch's stream beside the other glue), or
        'inpaint' = {'boxes', 'box_masks'}: the same masks in BOX coordinates, as a detector run on the box crop returns them
        (:113-119) - V pieces [h_v, w_v] uint8 / float32 or a packed (buffer, offsets) pair (`ops.inpaint_inputs_boxed`) - runs
        EdgeModel -> InpaintingModel -> merge as a fourth branch (:124-129), composites every vehicle's inpainted box under
        its pasted crop in the reference's per-vehicle order (:130-145) and returns 'inpaint_u8' [V, R, R, 3] as well.

        replay=True issues the three networks as ONE recorded-plan replay (`CompiledPass`, recorded on the first frame with
        this many vehicles and kept per vehicle count) instead of ~370 launches from Python: at 8 vehicles per frame the
        interpreter, not the GPU, bounds the eager form.

        A pipeline built with cad=True classifies every vehicle's box crop (VGG-19, :66-69) and returns 'cad_idx' int64 [V]; with
        'kp3d_bank' float32 [n_cad, 12, 3] in the scene the pose fit uses the chosen model's keypoints (:82-88) instead of 'kp3d'.
        With an initialised process group of more than one rank the frame's vehicles are sharded over the ranks (every rank
        passes the same scene; rank 0 returns the result, the other ranks a dict holding only 'state'; scene['shard'] = False
        keeps a rank on its own).  'state' is RANK-LOCAL then: the appearance codes and central crops of the rank's own
        vehicles [lo, hi) - all frames of a vehicle stay on one rank, `run_later_frame` picks the shard up from it.

        Returns 'kp_idx' int32 [V, 12], 'kp_xy' float32 [V, 12, 2], 'pose' = list of (error, rvec [3, 1], tvec [3, 1]),
        'icn_u8' / 'vunet_u8' uint8 [V, R, R, 3] (BGR), 'frame_icn' / 'frame_vunet' uint8 [H, W, 3], 'geom' int32 [V, 8],
        'state' = what `run_later_frame` needs to render the same vehicles' future frames (VUnet appearance code, central crop).

        Geometry mode (a pipeline built with cad_bank, a scene without 'masks'): see `_geometry_frame`."""
        if self._is_geometry(scene):
            return self._geometry_frame(scene, check, replay)
        rng = torch.get_rng_state() if check == "sync" else None
        import torch.distributed as dist
        world = dist.get_world_size(self.group) if (dist.is_available() and dist.is_initialized()) else 1
        if not _one_rank(self.group) and scene.get("shard", True):
            # One frame's vehicles over the ranks (BASELINE configs[3]: 64 vehicles of a frame, 8 shards of 8):
            # every rank holds the scene and renders vehicles shard_range(V, rank, world); the uint8 crops, keypoint indices
            # and crop rows travel to rank 0 (gather_in_order: five small messages per frame, no other exchange), which fits
            # the poses and pastes in vehicle order.  The range guard stays local to a rank's own vehicles - it runs
            # before the first collective, so a rank that redoes its shard in fp32 cannot desynchronise the gathers.
            rank = dist.get_rank(self.group)
            V = len(scene["bboxes"])
            lo, hi = shard_range(V, rank, world)
            local = self._guarded(self._frame_local, (slice_scene(scene, lo, hi), replay), check, rng)
            out = self._frame_gather_finish(scene, local, (lo, hi, V))
            if rank != 0:
                return out                                        # {'state': ...}: this rank's vehicles' appearance codes stay here
        else:
            out = self._guarded(self._run_frame, (scene, replay), check, rng)
        # the reference's host epilogue of the pose fit (argmin over the four starts, sign flip): 4 x 7 numbers per vehicle
        from .utils.pnp_utils import select_and_flip
        rv, tv, er = (t.cpu().numpy() for t in out.pop("_pose_raw"))
        out["pose"] = [select_and_flip(rv[i], tv[i], er[i]) for i in range(rv.shape[0])]
        return out

    # ------------------------------------------------------------------------------------------ geometry mode
    def _is_geometry(self, scene, state=None) -> bool:
        """A first frame's scene is in geometry mode when the pipeline holds a CAD bank, a later frame's (`state` given) when
        its first frame was."""
        return "masks" not in scene and (self.cad_bank if state is None else state.get("geometry")) is not None

    @staticmethod
    def _select(scene: Dict, keep, keys) -> Dict:
        """The scene restricted to the vehicles `keep` (host index list) for the per-vehicle `keys`."""
        import numpy as np
        out = dict(scene)
        idx = torch.as_tensor(keep, dtype=torch.long)
        for k in keys:
            v = scene.get(k)
            if v is None or k == "inpaint":
                continue
            if k == "box_masks":                                  # ragged pieces or a packed pair
                out[k] = _box_masks_of(v, keep)
            elif torch.is_tensor(v):
                out[k] = v.index_select(0, idx.to(v.device))
            elif isinstance(v, np.ndarray):
                out[k] = v[np.asarray(keep, dtype=np.int64)]
            else:
                out[k] = [v[i] for i in keep]
        if scene.get("inpaint") is not None and "inpaint" in keys:
            out["inpaint"] = VehiclePipeline._select(scene["inpaint"], keep, list(scene["inpaint"].keys()))
        return out

    @classmethod
    def _kept_planes(cls, geometry: Dict, keep) -> Dict:
        """The first frame's planes of the kept vehicles, what their later frames warp: 'src_planes', 'src_kp', 'src_vis'."""
        sel = cls._select(geometry, keep, ("src_planes", "src_kp", "src_vis"))
        return {k: sel[k] for k in ("src_planes", "src_kp", "src_vis")}

    @classmethod
    def _geometry_state(cls, f: Dict, lo: int = 0) -> Dict:
        """state['geometry'] of the kept vehicles of `_geometry_front`'s dict `f`; lo: the frame index of f's first vehicle."""
        keep, sc = f["keep"], f["scene"]
        st = {"vehicles": [lo + v for v in keep], "cad_idx": f["cad_idx"][keep], "pose": [f["pose"][v] for v in keep],
              "focals": sc["focals"], "centers": sc["centers"], **cls._kept_planes(f["geometry"], keep)}
        if f.get("dev") is not None:                              # device_pose: the same, kept on the device for the later frames
            sel = cls._select(f["dev"], keep, ("pose_d", "cad_idx_d", "src_kp_d"))
            st.update(pose_d=sel["pose_d"], cad_idx_d=sel["cad_idx_d"], src_kp_d=sel["src_kp_d"], kp_nv_d=f["dev"]["kp_nv_d"])
        return st

    # ---- what rank 0 gathers of a sharded geometry-mode first frame besides the crops: one int32 and one float32 row per vehicle
    @staticmethod
    def _pack_rows(f: Dict):
        """`_geometry_front`'s dict -> int32 [n, 14] (kp_idx 12, covered, cad_idx), float32 [n, 52] (kp_xy 24, rv 12, tv 12, er 4)."""
        import numpy as np
        n = f["V"]
        ints, flts = np.zeros((n, 14), np.int32), np.zeros((n, 52), np.float32)
        if n:
            ints[:, :12] = f["pre"]["kp_idx"].cpu().numpy()
            ints[:, 12] = f["g"]["covered"]
            ints[:, 13] = f["cad_idx"]
            flts[:, :24] = f["pre"]["kp_xy"].cpu().numpy().reshape(n, 24)
            raw = f["raw"] if f["raw"] is not None else tuple(t.cpu().numpy() for t in f["raw_d"])   # (device_pose: not read back before)
            flts[:, 24:36] = raw[0].reshape(n, 12)
            flts[:, 36:48] = raw[1].reshape(n, 12)
            flts[:, 48:52] = raw[2].reshape(n, 4)
        return ints, flts

    @staticmethod
    def _unpack_rows(ints, flts) -> Dict:
        """The gathered rows of `_pack_rows` (host arrays of all V vehicles) back into their named parts, each a copy."""
        import numpy as np
        V = ints.shape[0]
        return {"kp_idx": ints[:, :12].copy(), "covered": ints[:, 12].copy(), "cad_idx": ints[:, 13].astype(np.int64),
                "kp_xy": flts[:, :24].reshape(V, 12, 2).copy(), "rv": flts[:, 24:36].reshape(V, 4, 3).copy(),
                "tv": flts[:, 36:48].reshape(V, 4, 3).copy(), "er": flts[:, 48:52].copy()}

    @staticmethod
    def _spread(t: torch.Tensor, n: int, idx: torch.Tensor) -> torch.Tensor:
        """t's rows at the rows `idx` (device int64) of n rows of zeros: a rank's kept crops back at their vehicles' rows of its
        shard, so that ranks whose kept counts differ still send what the gather expects."""
        z = torch.zeros((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=idx.device)
        return z.index_copy_(0, idx, t) if idx.numel() else z

    def _rerender_masks(self, scene: Dict, focals, centers, cad_idx, poses, steps=None) -> torch.Tensor:
        """Rank 0's masks of vehicles it only holds the poses of (the render is deterministic per job, and a
        pose is 28 numbers where a mask is H x W bytes); steps: a later frame's (theta, tr) per vehicle.  The poses arrive as host
        numbers after the gather, so the host path (extrinsics_from_poses, render_jobs) serves here with device_pose as well:
        there is no device-resident fit to keep on the device."""
        import numpy as np

        from . import render as rd
        H, W = int(scene["frame"].shape[0]), int(scene["frame"].shape[1])
        K = rd.intrinsic(focals, centers)
        move = ()
        if steps is not None:
            move = (np.stack([rd.z_rot(th) for th, _ in steps]) if steps else np.zeros((0, 3, 3)),
                    np.stack([np.asarray(t, np.float64).reshape(3) for _, t in steps]) if steps else np.zeros((0, 3)))
        E = rd.extrinsics_from_poses([(p[1], p[2]) for p in poses])
        return rd.render_vehicles(self.cad_bank, cad_idx, E, float(K[0, 0]), float(K[1, 1]), (H, W), self.device, *move)["mask"]

    @torch.no_grad()
    def _geometry_front(self, scene: Dict, check) -> Dict:
        """Everything of a geometry-mode first frame before the networks, on the current stream, for the scene's vehicles (all of
        them, or one rank's shard): hourglass -> argmax -> keypoints -> pose fit on the device -> host select_and_flip ->
        extrinsics; render + plane visibility + plane cut-outs on the device (render.vehicle_geometry, one D2H of the counts).
        check: range guard of the keypoint stage (`_guarded`).  Returns 'pre' (device 'kp_idx', 'kp_xy' (+ 'cad_logits')),
        'raw' (the fit's host arrays rv, tv, er), 'pose', 'cad_idx', 'g' (vehicle_geometry's dict), 'keep' (vehicles whose render
        is not empty), 'geometry' (the derived scene keys of every vehicle) and 'sub' = the given-geometry scene of the kept
        vehicles ('_hg': their keypoint indices; '_pose_raw': their rows of this fit, passed through `_frame_finish`)."""
        import numpy as np

        from . import frame_ops as fo
        from . import ops
        from . import render as rd
        from .utils.pnp_utils import cpc_fit_device, select_and_flip
        dev, bank = self.device, self.cad_bank
        frame = scene["frame"]
        H, W, _ = frame.shape
        bboxes = np.asarray(scene["bboxes"]).reshape(-1, 4)
        V, R = bboxes.shape[0], 256

        def keypoints():
            geom_box = fo.box_geometry((H, W), bboxes, dev)
            hg_x = fo.crop_resize(frame, geom_box, (R, R), 1, fo.IMAGENET_MEAN, fo.IMAGENET_STD)        # :58-65
            pre = {"kp_idx": ops.argmax_hw(self.hg(hg_x)["heatmaps"][-1])}                              # :75-79
            if self.cad is not None:
                pre["cad_logits"] = self.cad(hg_x)                                                      # :66-69
            pre["kp_xy"] = fo.keypoints_to_frame(pre["kp_idx"], geom_box, (R // 4, R // 4))              # :95-97
            return pre

        if self.device_pose:
            return self._geometry_front_device(scene, check, keypoints)
        with torch.cuda.device(dev):
            pre = self._guarded(keypoints, (), check, None) if V else {}
            if self.cad is not None:
                cad_idx = pre["cad_logits"].argmax(1).cpu().numpy() if V else np.zeros(0, np.int64)
            else:
                if scene.get("cad_idx") is None:
                    raise ValueError("geometry mode: the scene needs 'cad_idx' [V] (or a pipeline built with cad=True)")
                cad_idx = np.asarray(scene["cad_idx"], np.int64).reshape(V)
            if V:
                f32 = lambda a: ops.h2d(np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32).reshape(-1, 2), (V, 2))), dev)   # noqa: E731
                raw_d = cpc_fit_device(f32(scene["focals"]), f32(scene["centers"]), pre["kp_xy"],
                                       ops.h2d(bank.kp3d[cad_idx], dev))                                     # :104-105
                raw = tuple(t.cpu().numpy() for t in raw_d)
                pose = [select_and_flip(raw[0][i], raw[1][i], raw[2][i]) for i in range(V)]
                kp_xy = pre["kp_xy"].cpu().numpy()
            else:
                raw_d, raw = None, tuple(np.zeros(sh, np.float32) for sh in ((0, 4, 3), (0, 4, 3), (0, 4)))
                pose, kp_xy = [], np.zeros((0, 12, 2), np.float32)
            K = rd.intrinsic(scene["focals"], scene["centers"])
            g = rd.vehicle_geometry(bank, frame, cad_idx, [(p[1], p[2]) for p in pose], K, kp_xy=kp_xy)
        return self._geometry_front_result(scene, pre, raw, raw_d, pose, cad_idx, g)

    def _geometry_front_result(self, scene: Dict, pre: Dict, raw, raw_d, pose, cad_idx, g: Dict, dev_keys: Optional[Dict] = None) -> Dict:
        """`_geometry_front`'s dict from the geometry `g` of either path; dev_keys (device_pose): the device copies of the pose,
        CAD indices and corner points, selected with the kept vehicles into 'sub' and kept for the state."""
        dev, bank = self.device, self.cad_bank
        V = len(pose)
        keep = [v for v in range(V) if g["covered"][v] > 0]
        geometry = {k: g[k] for k in ("masks", "src_sketch", "dst_sketch", "src_planes", "src_kp", "dst_kp", "src_vis", "dst_vis")}
        geometry["kp3d"] = bank.kp3d[cad_idx]
        geometry["cad_idx"] = cad_idx
        extra = {} if dev_keys is None else {"src_kp_d": dev_keys["src_kp_d"], "dst_kp_d": dev_keys["src_kp_d"]}
        sub = self._select({**scene, **geometry, **extra}, keep, PER_VEHICLE_KEYS + ("cad_idx", "inpaint") + tuple(extra))
        sub.pop("cad_idx", None)
        if dev_keys is not None:
            sub["kp_nv_d"] = dev_keys["kp_nv_d"]
        if V:
            hg = {"kp_idx": pre["kp_idx"]}
            if self.cad is not None:
                hg["cad_logits"] = pre["cad_logits"]
            sub["_hg"] = self._select(hg, keep, list(hg))
            sub["_pose_raw"] = tuple(t.index_select(0, torch.as_tensor(keep, dtype=torch.long, device=dev)) for t in raw_d)
        return {"pre": pre, "raw": raw, "raw_d": raw_d, "pose": pose, "cad_idx": cad_idx, "g": g, "keep": keep, "geometry": geometry,
                "sub": sub, "V": V, "scene": scene, "dev": dev_keys}

    @staticmethod
    def _pose_tuples(pose) -> list:
        """float32 [V, 7] (error, rvec, tvec) -> run_frame's 'pose': (error, rvec [3, 1], tvec [3, 1]) per vehicle."""
        return [(p[0], p[1:4].reshape(3, 1).copy(), p[4:7].reshape(3, 1).copy()) for p in pose]

    def _geometry_front_device(self, scene: Dict, check, keypoints) -> Dict:
        """`_geometry_front` with device_pose: the CAD index stays on the device (the classifier's argmax, or the scene's
        uploaded once), the fit takes the chosen models' keypoints from the bank's device table, and
        `render.vehicle_geometry_device` selects the pose and derives, renders and counts everything with one blocking read-back
        (pose, CAD indices, counts, corner points, extrinsic); the raw fit is not read back at all ('raw' is None)."""
        import numpy as np

        from . import ops
        from . import render as rd
        from .utils.pnp_utils import cpc_fit_device
        dev, bank = self.device, self.cad_bank
        frame = scene["frame"]
        V = np.asarray(scene["bboxes"]).reshape(-1, 4).shape[0]
        with torch.cuda.device(dev):
            pre = self._guarded(keypoints, (), check, None) if V else {}
            if self.cad is None and scene.get("cad_idx") is None:
                raise ValueError("geometry mode: the scene needs 'cad_idx' [V] (or a pipeline built with cad=True)")
            raw_d, kp_xy_d = None, None
            if V:
                cad_d = pre["cad_logits"].argmax(1) if self.cad is not None else \
                    ops.h2d(np.asarray(scene["cad_idx"], np.int64).reshape(V), dev)
                f32 = lambda a: ops.h2d(np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32).reshape(-1, 2), (V, 2))), dev)   # noqa: E731
                # (an index outside the bank is clamped for the fit only: fusg_pose_geometry flags it and the geometry raises)
                kp3d_d = bank.device_arrays(dev)["kp3d"].index_select(0, cad_d.clamp(0, len(bank) - 1))
                raw_d = cpc_fit_device(f32(scene["focals"]), f32(scene["centers"]), pre["kp_xy"], kp3d_d)        # :104-105
                kp_xy_d = pre["kp_xy"]
            else:
                cad_d = torch.zeros(0, dtype=torch.int64, device=dev)
            K = rd.intrinsic(scene["focals"], scene["centers"])
            g = rd.vehicle_geometry_device(bank, frame, cad_d, K, raw_d=raw_d, kp_xy_d=kp_xy_d)
        dev_keys = {"pose_d": g["pose_d"], "cad_idx_d": cad_d, "src_kp_d": g["tex_pts_d"], "kp_nv_d": g["tex_nv_d"]}
        return self._geometry_front_result(scene, pre, None, raw_d, self._pose_tuples(g["pose"]), g["cad_idx"], g, dev_keys)

    def _geometry_assemble(self, f: Dict, out: Dict) -> Dict:
        """run_frame's geometry-mode result from `_geometry_front`'s dict and the given-geometry result of the kept vehicles."""
        V, pre, keep = f["V"], f["pre"], f["keep"]
        out["kp_idx"] = pre["kp_idx"] if V else out["kp_idx"]
        out["kp_xy"] = pre["kp_xy"] if V else out["kp_xy"]
        out["pose"] = f["pose"]
        if self.cad is not None:
            out["cad_idx"] = torch.as_tensor(f["cad_idx"], device=self.device)
        out["geometry"] = f["geometry"]
        out["skipped"] = [v for v in range(V) if v not in keep]
        if out.get("state") is not None:
            out["state"]["geometry"] = self._geometry_state(f)
        return out

    def _geometry_frame(self, scene: Dict, check, replay) -> Dict:
        """run_frame in geometry mode: scene = 'frame', 'bboxes', 'focals', 'centers' (+ 'cad_idx' [V] when the pipeline has
        no CAD classifier, optional 'background', 'inpaint', 'vehicle_seeds', 'shard').  The reference's order (trajectory_inference.py:
        55-253, warp_learn/vehicle_utils.py:12-32): hourglass -> argmax -> keypoints -> pose fit on the device -> host
        select_and_flip -> extrinsics; render + plane visibility + plane cut-outs on the device (render.vehicle_geometry, one D2H of
        the counts); then the given-geometry path of `run_frame` on the vehicles whose render is not empty - replay=True replays its
        networks as the recorded pass of that many KEPT vehicles (the keypoint stage before the render stays eager).
        Returns run_frame's keys ('kp_idx', 'kp_xy', 'pose' (+ 'cad_idx') for every vehicle; 'icn_u8', 'vunet_u8', 'geom'
        (+ 'inpaint_u8') for the rendered ones, in order), 'geometry' = the derived scene keys of every vehicle ('masks',
        'src_sketch', 'dst_sketch', 'src_planes', 'src_kp', 'dst_kp', 'src_vis', 'dst_vis', 'kp3d', 'cad_idx'), 'skipped' =
        the vehicles whose render is empty (the reference's `except: continue`, :252-253: no networks, no paste) and
        'state' for `run_later_frame`.

        With a process group of more than one rank (and scene['shard'] not False) every rank runs its own vehicles
        shard_range(V, rank, world) end to end - crop, hourglass, pose fit, select_and_flip, render, visibility, cut-outs, networks -
        and rank 0 receives the crops, keypoint indices and frame keypoints, the fits and the covered counts of every vehicle
        (`_geometry_frame_sharded`).  Rank 0's 'geometry' then holds only 'cad_idx' and 'kp3d': the per-pixel and per-plane keys
        ('masks', 'src_sketch', 'dst_sketch', 'src_planes', 'src_kp', 'dst_kp', 'src_vis', 'dst_vis') stay on the ranks that own
        the vehicles.  Every rank returns a RANK-LOCAL 'state' (its own vehicles' appearance codes, crops and geometry)."""
        if not _one_rank(self.group) and scene.get("shard", True):
            return self._geometry_frame_sharded(scene, check, replay)
        with torch.cuda.device(self.device):
            f = self._geometry_front(scene, check)
        return self._geometry_assemble(f, self.run_frame(f["sub"], check=check, replay=replay))

    def _geometry_frame_sharded(self, scene: Dict, check, replay) -> Dict:
        """One rank's part of a sharded geometry-mode first frame (see `_geometry_frame`).  The range guard of the keypoint
        stage and of the networks runs before the first collective.  The gathers are `gather_in_order` over the shard_range
        sizes: a rank's crops and crop rows are spread back to their vehicles' rows of its shard (zeros where the render was
        empty), so ranks whose kept counts differ still send what the gather expects.  Rank 0 re-renders the masks of the kept
        vehicles from the gathered fits for its paste instead of gathering them: the render is deterministic
        per job, and a pose is 28 numbers where a mask is H x W bytes."""
        import numpy as np
        import torch.distributed as dist

        from .utils.pnp_utils import select_and_flip
        rng = torch.get_rng_state() if check == "sync" else None
        dev, bank = self.device, self.cad_bank
        rank, world = dist.get_rank(self.group), dist.get_world_size(self.group)
        bboxes = np.asarray(scene["bboxes"]).reshape(-1, 4)
        V = bboxes.shape[0]
        lo, hi = shard_range(V, rank, world)
        part = slice_scene(scene, lo, hi)
        if scene.get("cad_idx") is not None:
            part["cad_idx"] = np.asarray(scene["cad_idx"], np.int64).reshape(V)[lo:hi]
        with torch.cuda.device(dev):
            f = self._geometry_front(part, check)
            local = self._guarded(self._frame_local, (f["sub"], replay), check, rng)
            keep = f["keep"]
            kidx = torch.as_tensor(keep, dtype=torch.long, device=dev)
            ints, flts = self._pack_rows(f)
            crops = ("icn_u8", "vunet_u8", "geom") + (("inpaint_u8",) if self.inpaint else ())
            got = {k: gather_in_order(self._spread(local[k], hi - lo, kidx).contiguous(), V, self.group) for k in crops}
            gi = gather_in_order(torch.from_numpy(ints).to(dev), V, self.group)
            gf = gather_in_order(torch.from_numpy(flts).to(dev), V, self.group)
        state = self._local_state(local, (lo, hi, V))
        state["geometry"] = self._geometry_state(f, lo)
        if rank != 0:
            return {"state": state}
        u = self._unpack_rows(gi.cpu().numpy(), gf.cpu().numpy())
        cad_all, rv, tv, er = u["cad_idx"], u["rv"], u["tv"], u["er"]
        pose = [select_and_flip(rv[v], tv[v], er[v]) for v in range(V)]
        keep_all = [v for v in range(V) if u["covered"][v] > 0]
        with torch.cuda.device(dev):
            kall = torch.as_tensor(keep_all, dtype=torch.long, device=dev)
            masks = self._rerender_masks(scene, scene["focals"], scene["centers"], cad_all[keep_all], [pose[v] for v in keep_all])
            full = {k: got[k].to(dev).index_select(0, kall) for k in crops}
            full["kp_idx"] = torch.from_numpy(u["kp_idx"][keep_all]).to(dev)
            fin = self._select({**scene, "kp3d": bank.kp3d[cad_all]}, keep_all, ("bboxes", "kp3d", "inpaint"))
            fin["masks"] = masks
            fin["_pose_raw"] = tuple(torch.from_numpy(a[keep_all]).to(dev) for a in (rv, tv, er))
            out = self._frame_finish(fin, full)
            out.pop("_pose_raw")
            out["kp_idx"] = torch.from_numpy(u["kp_idx"]).to(dev)
            out["kp_xy"] = torch.from_numpy(u["kp_xy"]).to(dev)
            if self.cad is not None:
                out["cad_idx"] = torch.as_tensor(cad_all, device=dev)
        out["pose"] = pose
        out["geometry"] = {"cad_idx": cad_all, "kp3d": bank.kp3d[cad_all]}
        out["skipped"] = [v for v in range(V) if v not in keep_all]
        state["geometry"]["all"] = {"vehicles": keep_all, "cad_idx": cad_all[keep_all], "pose": [pose[v] for v in keep_all]}
        out["state"] = state
        return out

    @torch.no_grad()
    def _geometry_later_front(self, scene: Dict, state: Dict) -> Dict:
        """The render of a geometry-mode later frame for the vehicles of `state` (all, or one rank's), on the current stream:
        'g' (vehicle_geometry's dict), 'keep' (state positions whose render is not empty), 'geometry' and the given-geometry
        'sub' scene / 'sub_state' of the kept vehicles."""
        from . import render as rd
        gs = state["geometry"]
        veh = list(gs["vehicles"])
        steps = [scene["steps"][v] for v in veh]
        K = rd.intrinsic(gs["focals"], gs["centers"])
        extra = {}
        with torch.cuda.device(self.device):
            if self.device_pose:
                # the first frame's selected pose and CAD indices as it left them on the device; a state made without
                # device_pose holds the host copies only, which are uploaded then
                import numpy as np

                from . import ops
                pose_d, cad_d = gs.get("pose_d"), gs.get("cad_idx_d")
                if pose_d is None:
                    rows = [[p[0], *np.asarray(p[1]).reshape(3), *np.asarray(p[2]).reshape(3)] for p in gs["pose"]]
                    pose_d = ops.h2d(np.asarray(rows, np.float32).reshape(len(veh), 7), self.device)
                    cad_d = ops.h2d(np.asarray(gs["cad_idx"], np.int64).reshape(len(veh)), self.device)
                g = rd.vehicle_geometry_device(self.cad_bank, scene["frame"], cad_d, K, pose_d=pose_d, steps=steps)
                if gs.get("src_kp_d") is not None:
                    extra = {"src_kp_d": gs["src_kp_d"], "dst_kp_d": g["tex_pts_d"]}
            else:
                g = rd.vehicle_geometry(self.cad_bank, scene["frame"], gs["cad_idx"], [(p[1], p[2]) for p in gs["pose"]], K, steps=steps)
        keep = [i for i in range(len(veh)) if g["covered"][i] > 0]
        geometry = {k: g[k] for k in ("masks", "dst_sketch", "dst_kp", "dst_vis")}
        geometry["kp3d"] = g["kp3d"]
        sub = self._select({**scene, **geometry, **extra, "src_planes": gs["src_planes"], "src_kp": gs["src_kp"], "src_vis": gs["src_vis"]},
                           keep, ("masks", "dst_sketch", "dst_kp", "dst_vis", "src_planes", "src_kp", "src_vis") + tuple(extra))
        if extra:
            sub["kp_nv_d"] = gs["kp_nv_d"]
        if scene.get("vehicle_seeds") is not None:
            sub["vehicle_seeds"] = [scene["vehicle_seeds"][veh[i]] for i in keep]
        if self._later_inpaint(scene) is not None:               # per first-frame vehicle, like the seeds: a skipped one is not inpainted
            sub["inpaint"] = self._select(scene["inpaint"], [veh[i] for i in keep], list(scene["inpaint"].keys()))
        sub.pop("steps", None)
        sub_state = dict(state, geometry=None, sharded=False,
                         appearance=[self._select({"a": a}, keep, ("a",))["a"] for a in state["appearance"]],
                         central=self._select({"c": state["central"]}, keep, ("c",))["c"])
        return {"g": g, "keep": keep, "veh": veh, "geometry": geometry, "sub": sub, "sub_state": sub_state, "scene": scene}

    @staticmethod
    def _geometry_later_assemble(f: Dict, out: Dict) -> Dict:
        out["geometry"] = f["geometry"]
        kept = [f["veh"][i] for i in f["keep"]]
        out["skipped"] = [v for v in range(len(f["scene"]["steps"])) if v not in kept]
        return out

    def _geometry_later_frame(self, scene: Dict, state: Dict, check, replay) -> Dict:
        """run_later_frame in geometry mode: scene = 'frame' (+ 'background', 'vehicle_seeds') and 'steps' = (theta, tr) per
        vehicle of the first frame (`render.trajectory_steps`).  Each vehicle the first frame rendered is moved (mesh and
        3-D keypoints by v @ z_rot(theta) + tr, trajectory_inference.py:359-363), rendered at the first frame's extrinsic,
        its moved keypoints projected with K (:364-367) -> 'dst_sketch', 'masks', 'dst_kp', 'dst_vis'
        (render.vehicle_geometry); then the given-geometry path of `run_later_frame` for the vehicles whose render is not
        empty (replay=True: its recorded pass of that many vehicles); scene['inpaint'] lists every first-frame vehicle, like
        'steps', and is selected with the kept ones (a skipped vehicle is not inpainted).  Returns its keys (for those vehicles, in order),
        'geometry' (the derived keys of every vehicle of the state) and 'skipped' (first-frame vehicle indices: skipped there or
        rendering empty now - not pasted).  A RANK-LOCAL state of a sharded first frame: see `_geometry_later_sharded`."""
        if not _one_rank(self.group) and state.get("sharded"):
            return self._geometry_later_sharded(scene, state, check, replay)
        f = self._geometry_later_front(scene, state)
        return self._geometry_later_assemble(f, self.run_later_frame(f["sub"], f["sub_state"], check=check, replay=replay))

    def _geometry_later_sharded(self, scene: Dict, state: Dict, check, replay) -> Optional[Dict]:
        """A later frame of a sharded geometry-mode clip: every rank moves, renders and runs the vehicles of its own state; the
        crops, crop rows and covered counts travel to rank 0 over the first frame's shard_range sizes (spread to their vehicles'
        rows), and rank 0 re-renders the kept vehicles' masks from the poses of its state and the scene's steps and pastes.  Rank 0
        returns the result ('geometry' holds 'kp3d' of the first frame's rendered vehicles only), the other ranks None."""
        import numpy as np

        from . import render as rd
        if self._later_inpaint(scene) is not None:
            raise ValueError("run_later_frame: a sharded geometry-mode later frame with scene['inpaint'] is not supported (rank 0 would "
                             "need every rank's inpainted boxes spread over the kept vehicles); inpaint later frames in geometry mode "
                             "on one rank, or shard a given-geometry clip")
        rng = torch.get_rng_state() if (check == "sync" and scene.get("vehicle_seeds") is None) else None
        dev = self.device
        lo, hi, V = state["shard"]
        n = hi - lo
        f = self._geometry_later_front(scene, state)
        with torch.cuda.device(dev):
            local = self._guarded(self._later_local, (f["sub"], f["sub_state"], replay), check, rng)
            ridx = torch.as_tensor([f["veh"][i] - lo for i in f["keep"]], dtype=torch.long, device=dev)
            cov = np.zeros((n, 1), np.int32)
            for i, v in enumerate(f["veh"]):
                cov[v - lo, 0] = f["g"]["covered"][i]
            got = {k: gather_in_order(self._spread(local[k], n, ridx).contiguous(), V, self.group) for k in ("icn_u8", "vunet_u8", "geom")}
            gc = gather_in_order(torch.from_numpy(cov).to(dev), V, self.group)
        if gc is None:
            return None
        gc = gc.cpu().numpy()[:, 0]
        al = state["geometry"]["all"]
        keep = [i for i, v in enumerate(al["vehicles"]) if gc[v] > 0]
        kept = [al["vehicles"][i] for i in keep]
        gs = state["geometry"]
        with torch.cuda.device(dev):
            masks = self._rerender_masks(scene, gs["focals"], gs["centers"], al["cad_idx"][keep], [al["pose"][i] for i in keep],
                                         steps=[scene["steps"][v] for v in kept])
            kidx = torch.as_tensor(kept, dtype=torch.long, device=dev)
            full = {k: got[k].to(dev).index_select(0, kidx) for k in got}
            out = self._later_finish({**scene, "masks": masks}, full)
        cad = al["cad_idx"]
        out["geometry"] = {"kp3d": np.stack([self.cad_bank.kp3d[int(m)] @ rd.z_rot(scene["steps"][v][0])
                                             + np.asarray(scene["steps"][v][1], np.float64).reshape(3)
                                             for m, v in zip(cad, al["vehicles"])]) if len(cad) else np.zeros((0, 12, 3))}
        out["skipped"] = [v for v in range(len(scene["steps"])) if v not in kept]
        return out

    # ---- one frame in flight: the geometry stage of frame i+1 on a stream of its own
    def _scenes_ready(self, scenes):
        """The event a pipelined geometry stage waits for before it reads its scene: for a list or tuple of scenes (made before
        the loop started) the caller's stream as it is NOW, so frame i+1's keypoint stage does not queue behind frame i's
        networks; for any other iterable None (each stage then waits for the caller's stream as it is when the scene is drawn,
        which is correct for scenes made on the fly and overlaps nothing)."""
        if self.cad_bank is None or not isinstance(scenes, (list, tuple)) or self.device.type != "cuda":
            return None
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return ev

    def _issue_guarded(self, fn, word=None):
        """fn() issued on the current stream without waiting for it, under the status word `word()` (default: the pipeline's own,
        `status_word`): the word is copied to a pinned int32 behind fn's launches and cleared for the next stage, whose launches
        queue behind that copy, and one event is recorded.  In a precision without a range guard there is only the event.
        Returns (fn's result, ticket); `_status_raised(ticket)` redeems the ticket."""
        from . import ops
        pin = None
        if ops.range_guarded():
            word = (word or self.status_word)()
            with self._routed(), ops.defer_range_check(), ops.status_scope(word):
                out = fn()
            pin = self._pins.pop() if self._pins else torch.zeros(1, dtype=torch.int32, pin_memory=True)
            pin.copy_(word[:1], non_blocking=True)
            word.zero_()
        else:
            with self._routed():
                out = fn()
        ev = torch.cuda.Event()
        ev.record()
        return out, (pin, ev)

    def _status_raised(self, ticket, wait: bool = True) -> bool:
        """Wait for the stage behind `_issue_guarded`'s ticket (wait=False: the caller has waited for something queued behind
        it) and say whether it raised its status word; the pinned int goes back to the ring."""
        pin, ev = ticket
        if wait:
            ev.synchronize()
        if pin is None:
            return False
        hit = int(pin[0]) != 0
        self._pins.append(pin)
        return hit

    @staticmethod
    def _one_in_flight(items, issue, collect, direct=None):
        """The one-deep software pipeline of the frame drivers, a generator: issue(item i+1) -> ticket runs before
        collect(ticket of item i) is yielded; the last ticket is collected at the end.  An item for which issue returns None is
        not pipelined: what is in flight is collected first, then direct(item) is yielded."""
        pending = None
        for item in items:
            ticket = issue(item)
            if pending is not None:
                yield collect(pending)
            pending = ticket
            if ticket is None:
                yield direct(item)
        if pending is not None:
            yield collect(pending)

    def _geo_word(self) -> torch.Tensor:
        from . import ops
        if self._geo_status is None:
            self._geo_status = ops.new_status_word(self.device)
        return self._geo_status

    def _issue_geometry_front(self, fn, ready) -> Dict:
        """Run fn() (a geometry front: keypoints, pose fit and render with their host read-backs) on the pipeline's geometry
        stream, ordered after `ready` (or after the caller's stream as it is now), under a status word of its own
        (`_issue_guarded` on that stream); the caller's stream then waits for the stage.  The ticket is left in f['_ticket']."""
        main = torch.cuda.current_stream(self.device)
        if self._geo_stream is None:
            self._geo_stream = torch.cuda.Stream(device=self.device)
        if ready is None:
            ready = torch.cuda.Event()
            ready.record(main)
        self._geo_stream.wait_event(ready)
        with torch.cuda.stream(self._geo_stream):
            f, ticket = self._issue_guarded(fn, self._geo_word)
        main.wait_event(ticket[1])
        for t in _tensors({k: v for k, v in f.items() if k != "scene"}):    # made on the geometry stream, used on the caller's
            if t.is_cuda:
                t.record_stream(main)
        f["_ticket"] = ticket
        return f

    def run_frames(self, scenes, replay: bool = True):
        """`run_frame` over a sequence of frames (the reference's outer loop, trajectory_inference.py:283-300), software-
        pipelined one frame deep: frame i+1's host work (40 homography fits, ~40 launches of glue, the networks' replay)
        is issued while the GPU still runs frame i, and frame i's results are collected afterwards - its range status
        and raw pose come back through pinned buffers filled by stream-ordered copies and one event, so reading them
        waits for frame i only.  A generator: yields one `run_frame`-shaped dict per scene, in order; every tensor in it
        is the caller's (nothing aliases a later frame's buffers).  A frame whose split-fp16 range status is raised is
        redone in exact fp32 before it is yielded, with the RNG state it was issued under.
        Geometry-mode scenes (a pipeline with cad_bank, no 'masks') are pipelined the same way on one rank: frame i+1's keypoint
        stage, pose fit, render and their two host read-backs run on a stream of the pipeline's own (`_issue_geometry_front`), so
        they do not wait for frame i's networks, which frame i+1's then follow on the caller's stream; a raised status of either
        stage redoes the frame whole, geometry included.  For a list or tuple of scenes the geometry stage is ordered after what the
        caller's stream held when the loop began; for another iterable, after what it holds when each scene is drawn.  Sharded
        (process group), geometry scenes run frame by frame (`run_frame`)."""
        if not _one_rank(self.group):
            # sharded frames, one frame deep as well: every rank issues its shard of frame i+1 before frame i's crops are
            # gathered; the gather and rank 0's frame-level part run on a communication stream that waits for frame i's
            # launches only, so they overlap frame i+1's networks.  Yields `run_frame`'s sharded results (rank 0: the frame,
            # other ranks: {'state': ...}); a scene with shard = False, or a geometry-mode one, is not pipelined.
            def issue(scene):
                if scene.get("shard", True) and not self._is_geometry(scene):
                    return self._issue_sharded(scene, replay)

            yield from self._one_in_flight(scenes, issue, self._collect_sharded, lambda scene: self.run_frame(scene, replay=replay))
            return
        ready = self._scenes_ready(scenes)
        yield from self._one_in_flight(scenes, lambda scene: self._issue_frame(scene, replay, ready), self._collect_frame)

    def _issue_frame(self, scene, replay, ready=None):
        from . import ops
        rng = torch.get_rng_state() if (ops.range_guarded() and scene.get("vehicle_seeds") is None) else None
        front = None
        with torch.cuda.device(self.device):
            if self._is_geometry(scene):                         # keypoints -> pose -> render on the geometry stream first
                front = self._issue_geometry_front(lambda: self._geometry_front(scene, None), ready)
                scene_nets = front["sub"]
            else:
                scene_nets = scene

            def frame():
                # stream-ordered read-back: the three raw pose arrays into pinned memory behind the frame's launches; the
                # status word follows them (`_issue_guarded`), then the one event to wait on
                out = self._run_frame(scene_nets, replay)
                raw = out.pop("_pose_raw")
                ring = self._frame_pins
                hit = [i for i, pr in enumerate(ring) if all(a.shape == b.shape for a, b in zip(pr, raw))]
                pins = ring.pop(hit[0]) if hit else [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in raw]
                for h, t in zip(pins, raw):
                    h.copy_(t, non_blocking=True)
                return out, pins

            (out, pins), ticket = self._issue_guarded(frame)
        return {"out": out, "pins": pins, "ticket": ticket, "scene": scene, "rng": rng, "front": front}

    def _collect_frame(self, t):
        from .utils.pnp_utils import select_and_flip
        hit, front = self._status_raised(t["ticket"]), t["front"]
        if front is not None:                                     # (its event: the frame's was recorded behind it)
            hit = self._status_raised(front.pop("_ticket"), wait=False) or hit
        rv, tv, er = (h.numpy().copy() for h in t["pins"])
        self._frame_pins.append(t["pins"])
        if hit:                                                   # rare: this frame again (geometry included), in exact fp32
            return _redo_f32(lambda: self.run_frame(t["scene"], check=None, replay=False), t["rng"], restore=True)
        out = t["out"]
        if front is not None:                                     # the pose of the geometry stage (the same fit, passed through)
            return self._geometry_assemble(front, out)
        out["pose"] = [select_and_flip(rv[i], tv[i], er[i]) for i in range(rv.shape[0])]
        return out

    def _issue_sharded(self, scene, replay):
        """This rank's shard of a frame, issued without waiting for it (the sharded counterpart of `_issue_frame`)."""
        import torch.distributed as dist
        from . import ops
        rank, world = dist.get_rank(self.group), dist.get_world_size(self.group)
        V = len(scene["bboxes"])
        lo, hi = shard_range(V, rank, world)
        sub = slice_scene(scene, lo, hi)
        rng = torch.get_rng_state() if (ops.range_guarded() and scene.get("vehicle_seeds") is None) else None
        with torch.cuda.device(self.device):
            local, ticket = self._issue_guarded(lambda: self._frame_local(sub, replay))
        return {"local": local, "ticket": ticket, "scene": scene, "sub": sub, "shard": (lo, hi, V), "rng": rng}

    def _collect_sharded(self, t):
        from .utils.pnp_utils import select_and_flip
        local = t["local"]
        if self._status_raised(t["ticket"]):                      # (waits for this frame's launches only; the next frame's are already queued)
            # rare: this rank's shard again, in exact fp32 (before any collective)
            with self._routed():
                local = _redo_f32(lambda: self._frame_local(t["sub"], False), t["rng"], restore=True)
            torch.cuda.synchronize(self.device)
        main = torch.cuda.current_stream(self.device)
        if self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(device=self.device)
        comm = self._comm_stream
        for v in _tensors(local):
            if v.is_cuda:
                v.record_stream(comm)
        with torch.cuda.device(self.device), torch.cuda.stream(comm):
            out = self._frame_gather_finish(t["scene"], local, t["shard"])
            if "_pose_raw" in out:
                rv, tv, er = (x.cpu().numpy() for x in out.pop("_pose_raw"))          # waits for the communication stream only
                out["pose"] = [select_and_flip(rv[i], tv[i], er[i]) for i in range(rv.shape[0])]
        main.wait_stream(comm)                                    # the caller consumes the results on its own stream
        for v in _tensors(out):
            if v.is_cuda:
                v.record_stream(main)
        return out

    def _run_frame(self, scene, replay=False):
        """One rank, every vehicle: the per-vehicle part, then the frame-level part."""
        return self._frame_finish(scene, self._frame_local(scene, replay))

    GATHERED = ("kp_idx", "icn_u8", "vunet_u8", "geom")

    def _gather_keys(self, first_frame: bool, inpaint: bool = False):
        if not first_frame:                                       # (inpaint: the later scene carries 'inpaint')
            return ("icn_u8", "vunet_u8", "geom") + (("inpaint_u8",) if inpaint else ())
        return self.GATHERED + (("inpaint_u8",) if self.inpaint else ()) + (("cad_idx",) if self.cad is not None else ())

    def _gather_local(self, local, V, first_frame=True, inpaint=False):
        """The frame's only exchange: this rank's crops / keypoint indices / crop rows -> rank 0, in vehicle order (a few small
        messages; RCCL gather on device tensors, gloo through the host).  Returns the full dict on rank 0, None elsewhere."""
        import torch.distributed as dist
        full = {}
        for k in self._gather_keys(first_frame, inpaint):
            g = gather_in_order(local[k].contiguous(), V, self.group)
            full[k] = None if g is None else g.to(self.device)
        return full if dist.get_rank(self.group) == 0 else None

    @staticmethod
    def _local_state(local, shard):
        """What `run_later_frame` needs for THIS rank's vehicles (they never move: SURVEY.md 8e)."""
        if "mu_app_0" not in local:
            return None
        return {"appearance": [local["mu_app_0"], local["mu_app_1"]], "central": local["central"], "shard": tuple(shard), "sharded": True}

    def _frame_gather_finish(self, scene, local, shard):
        """Sharded first frame after the rank's local part: gather -> (rank 0) frame-level part.  Every rank gets 'state'."""
        state = self._local_state(local, shard)
        full = self._gather_local(local, shard[2], True)
        if full is None:
            return {"state": state}
        out = self._frame_finish(scene, full)                      # (no appearance codes in `full`: they stay on their ranks)
        out["state"] = state
        return out

    def _plan_key(self, key):
        """`key` as `_frame_plans` holds it: with a routing batch in force it gains ("route_batch", R), so a recording made
        under one routing is never replayed under another; without one it is `key` itself."""
        from . import ops
        r = ops.ROUTE_BATCH if self.route_batch is None else self.route_batch
        return tuple(key) + (("route_batch", r),) if r else key

    def _plan(self, key) -> Optional["CompiledPass"]:
        """The recorded pass kept under `key` (`_plan_key`), unless a network's packed weights have changed since it was recorded."""
        cp = self._frame_plans.get(self._plan_key(key))
        return cp if cp is not None and [n.generation for n in self._nets] == cp.generations else None

    def _replay(self, key, nets_in, seeds, fn=None, clone=None) -> Dict:
        """One replay of the recorded pass `fn` (default `_run`) kept under `key`: one recorded pass (with its private pool of
        intermediates) per vehicle count and precision, recorded on first use; a video whose count varies keeps the FRAME_PLANS
        most recently used ones.  The plan's output buffers belong to its next replay: the outputs `clone` names (default: all
        of them) are handed out as copies."""
        cps = self._frame_plans
        cp = self._plan(key)
        key = self._plan_key(key)
        if cp is None:
            cps.pop(key, None)
            while len(cps) >= FRAME_PLANS:
                cps.pop(next(iter(cps)))
            cp = cps[key] = CompiledPass(self, nets_in, seeds, fn)
        else:
            cps[key] = cps.pop(key)                               # most recently used last
        out = dict(cp._issue(nets_in, seeds))
        for k in (clone if clone is not None else list(out)):
            if k in out:
                out[k] = out[k].clone()
        return out

    # ---- the pass mechanics every frame driver shares, per-frame and batched.  Nothing here knows a row layout: a driver hands
    # in its row offsets, its padded row count B and its paste function.  All of it runs INSIDE the guarded function, so the range
    # guard's fp32 redo builds its own plan lookup and buffers (nothing of the first attempt is reused).
    def _guarded_pass(self, fn, args, check, seeds):
        """fn(*args) under the range guard (`_guarded`), with the host RNG state of now for its fp32 redo when the pass draws
        global noise (no 'vehicle_seeds')."""
        rng = torch.get_rng_state() if (check == "sync" and seeds is None) else None
        return self._guarded(fn, args, check, rng)

    def _pass_buffers(self, pkey, replay, B: int, N: int):
        """How a pass of N real rows at B >= N network rows meets its recorded plan: (replay - off while another plan is being
        recorded -, tgt = the inputs of the plan kept under pkey, written in place, or {}, buf).  buf(k, c) -> (the networks'
        input `k` at B rows of c channels, its padding rows zero; the view of its N real rows the glue writes)."""
        from . import ops
        replay = replay and ops.RECORDER is None
        cp = self._plan(pkey) if replay else None
        tgt = cp.inputs if cp is not None else {}                 # a recorded pass's inputs are written in place

        def buf(k, c):
            t = tgt.get(k)
            if t is None:
                t = ops.nhwc_empty(B, c, 256, 256, self.device, zero=True)
            elif B > N:
                t[N:].zero_()
            return t, t[:N]

        return replay, tgt, buf

    def _nets_pass(self, fn, pkey, replay, nets_in, seeds, N: Optional[int] = None, clone=None) -> Dict:
        """The networks `fn` (`_run`, `_later_nets`) over nets_in - one replay of the plan under pkey (`_replay`; clone: the
        outputs handed out as copies) or eagerly - and 'icn_u8' Lab -> BGR (consumed before the plan's next replay).  N: the real
        rows of a padded pass - the seeds are padded with 0 to the inputs' rows and every output is cut to N, so nothing behind
        knows about padding."""
        from .warp_learn import planes_utils as pu
        if N is not None and seeds is not None:
            seeds = seeds + [0] * (int(nets_in["icn_x"].shape[0]) - N)
        out = self._replay(pkey, nets_in, seeds, fn=fn, clone=clone) if replay else fn(nets_in, seeds)
        if N is not None:
            out = {k: v[:N] for k, v in out.items()}
        out["icn_u8"] = pu.lab2bgr(out["icn_u8"] if N is None else out["icn_u8"].contiguous())     # to_image(from_LAB=True), :182
        return out

    def _on_inpaint_stream(self, build, tgt):
        """build() -> EdgeConnect's four inputs, issued on the inpaint branch's stream, forked from the current one.  Returns (the
        four tensors, join): join() makes the current stream wait for them (`tgt`: they are a recorded pass's own buffers)."""
        from . import ops
        if os.environ.get("FUSG_STREAMS", "1") == "0" or self.device.type != "cuda":
            return build(), (lambda: None)
        st = self._streams.get("inpaint")
        if st is None:
            st = self._streams["inpaint"] = torch.cuda.Stream(device=self.device, priority=0)
        ops.fork_to(st)
        with torch.cuda.stream(st):
            res = build()
        return res, (lambda: ops.join_from(st, [] if tgt else list(res.values())))

    def _inpaint_inputs_rows(self, scenes, offs, B: int, tgt) -> Tuple[Dict, object]:
        """EdgeConnect's four inputs of a batch, [B, c, R, R] each (B >= offs[-1]: the padding rows are zero): scene f's rows
        offs[f] .. offs[f + 1] come from ITS image and boxes (`ops.inpaint_inputs` / `inpaint_inputs_boxed`, or the scene's
        given tensors copied in), all on the inpaint branch's stream, forked once; `tgt`: a recorded pass's input buffers,
        written in place.  The offsets are the driver's: f * V for a clip's frames, `frame_batch_offsets` for first frames,
        `clip_batch_frame_rows` for several clips.  Returns (the four tensors, join)."""
        from . import ops
        R, N = 256, offs[-1]

        def build():
            bufs = {k: tgt["ec_" + k] for k in ops.INPAINT_KEYS} if tgt else \
                {k: torch.empty((B, 3 if k == "img" else 1, R, R), dtype=torch.float32, device=self.device) for k in ops.INPAINT_KEYS}
            if B > N:                                             # (every real row is written below)
                for k in ops.INPAINT_KEYS:
                    bufs[k][N:].zero_()
            for f, sc in enumerate(scenes):
                if offs[f + 1] == offs[f]:
                    continue
                inp = sc["inpaint"]
                rows = {k: bufs[k][offs[f]:offs[f + 1]] for k in ops.INPAINT_KEYS}
                if "box_masks" in inp:
                    ops.inpaint_inputs_boxed(sc["frame"], inp["box_masks"], inp["boxes"], out=rows)
                elif "det_masks" in inp:
                    ops.inpaint_inputs(sc["frame"], inp["det_masks"], inp["boxes"], out=rows)
                else:                                             # given
                    for k in ops.INPAINT_KEYS:
                        rows[k].copy_(inp[k])
            return bufs

        return self._on_inpaint_stream(build, tgt)

    def _box_rows(self, boxes) -> torch.Tensor:
        """The paste box rows of the 'inpaint' boxes of a pass (a list of [n, 4] per scene, in row order): CUDA int32 [N, 8] =
        (x0, y0, x1, y1, 0, 0, 0, 0), one upload."""
        import numpy as np

        from . import ops
        boxes = np.concatenate([np.asarray(b).reshape(-1, 4) for b in boxes])
        rows = np.zeros((boxes.shape[0], 8), np.int32)
        rows[:, :4] = boxes
        return ops.h2d(rows, self.device, torch.int32)

    def _paste_base(self, scene) -> torch.Tensor:
        """What a scene's composites start from: with inpainting the frame (:133-143, :340), else 'background' or the frame."""
        inp = scene.get("inpaint") if self.inpaint else None
        return scene["frame"] if inp is not None else scene.get("background", scene["frame"])

    @staticmethod
    def background_indices(n: int, max_frames: int = 64) -> List[int]:
        """The scenes `estimate_background` samples out of n: all of them up to max_frames, else (i * n) // max_frames."""
        if n < 1 or not 1 <= max_frames <= 64:
            raise ValueError(f"estimate_background: {n} scenes, max_frames = {max_frames} (at least one scene, max_frames in 1..64)")
        return list(range(n)) if n <= max_frames else [(i * n) // max_frames for i in range(max_frames)]

    def _background_sample(self, scenes, max_frames: int, min_valid: Optional[int]) -> Tuple[List[int], int]:
        """(the scenes `background_indices` samples, min_valid with its default: max(1, T // 8) of the T sampled)."""
        idx = self.background_indices(len(scenes), max_frames)
        return idx, max(1, len(idx) // 8) if min_valid is None else int(min_valid)

    def estimate_background(self, scenes, max_frames: int = 64, margin: int = 8, min_valid: Optional[int] = None) -> Dict:
        """The 'background' the default mode's composites start from (`_paste_base`; the reference reads background_frame.png,
        trajectory_inference.py:42-53, and has no code that makes it), estimated from the video itself: per pixel and channel the
        lower median over the sampled frames in which no detector box, grown by `margin`, covers the pixel (`ops.background_median`:
        one launch, nothing read back).  scenes: `run_frames`-style, 'frame' uint8 [H, W, 3] (CUDA) and 'bboxes' int [V, 4] (host).
        min_valid=None: max(1, T // 8) of the T sampled frames; a pixel that fewer frames see takes all T.  Returns 'background'
        uint8 [H, W, 3] and 'count' uint8 [H, W] on the device (count < min_valid marks the fallback pixels), 'frames' (the indices
        used) and 'min_valid'.  Nothing is put into the scenes: the caller sets scene['background']."""
        import numpy as np

        from . import ops
        idx, mv = self._background_sample(scenes, max_frames, min_valid)
        boxes = [np.asarray(scenes[i]["bboxes"]).reshape(-1, 4) for i in idx]
        bg, count = ops.background_median([scenes[i]["frame"] for i in idx], boxes, margin=margin, min_valid=mv)
        return {"background": bg, "count": count, "frames": idx, "min_valid": mv}

    def foreground_inpaint(self, scene, background, core_frac: float = 0.5, **params) -> Dict:
        """scene['inpaint'] without a detector: {'boxes', 'box_masks', 'stats'} for the caller to assign.  boxes = `inpaint_box_rule`
        of every scene['bboxes'] row (the reference's bbox_new_img); box_masks = each vehicle's mask as what differs from
        `background` (uint8 [H, W, 3] on the device, e.g. `estimate_background`'s) inside that box and hangs together with the
        tracker box's core - the box shrunk about its centre to core_frac of its width and height (`ops.foreground_masks`, one
        launch, nothing read back; params: thr, open_r, close_r, grow, fallback - defaults untried on real video) - in the packed
        (buffer, offsets) form `ops.inpaint_inputs_boxed` takes; stats int32 [V, 4] stays on the device.  Nothing is put into the scene."""
        import numpy as np

        from . import ops
        frame = scene["frame"]
        tb = np.asarray(scene["bboxes"], dtype=np.int64).reshape(-1, 4)
        boxes = inpaint_box_rule(tb, (int(frame.shape[0]), int(frame.shape[1])))
        box_masks, stats = ops.foreground_masks(frame, background, boxes, foreground_cores(tb, core_frac), **params)
        return {"boxes": boxes, "box_masks": box_masks, "stats": stats}

    def erase_vehicles(self, scene, background, grow: int = 4, **params) -> torch.Tensor:
        """A third compositing base, uint8 [H, W, 3]: the scene's frame with only its own vehicles (scene['bboxes']) replaced by
        `background` inside their masks (`foreground_inpaint`'s, grown by `grow` pixels), the rest of the traffic kept.  Two more
        launches, nothing read back; the caller passes it as that scene's scene['background'].  Nothing is put into the scene."""
        from . import ops
        inp = self.foreground_inpaint(scene, background, grow=grow, **params)
        return ops.erase_to_background(scene["frame"], background, inp["box_masks"], inp["boxes"])

    def detect_vehicles(self, scenes, background, **params) -> list:
        """scene['bboxes'] without a tracker's detector: per scene {'bboxes' int64 [V_f, 4] (x0, y0, x1, y1) half-open and
        pixel-tight, 'area' int64 [V_f], 'stats' int32 [4] = `ops.FOREGROUND_BOXES_STATS`} on the host, for the caller to assign.
        A vehicle is a 4-connected blob of grid cells in which the frame differs from `background` (uint8 [H, W, 3] on the device,
        e.g. `estimate_background`'s, or one per scene) - `ops.foreground_boxes`, two launches per 64 scenes, and ONE `ops.d2h`
        for all of them (params: thr, cell, min_count, open_r, close_r, min_area, min_w, min_h, max_boxes, roi - defaults tried on
        synthetic scenes only).  Boxes are per frame (`track_vehicles` links them across frames), and the read-back is the only way
        the boxes reach `foreground_inpaint`.  Nothing is put into the scenes."""
        from . import ops
        if not scenes:
            return []
        rows = [self._pack_frame_tables(*tables) for tables in self._detect_windows(scenes, background, params)]
        return self._detected_rows(ops.d2h(rows[0] if len(rows) == 1 else torch.cat(rows, dim=0)))

    @staticmethod
    def _detect_windows(scenes, background, params):
        """`ops.foreground_boxes` over a video's scenes in windows of at most `ops.BACKGROUND_MAX_FRAMES` (background: one for all
        scenes, or one per scene): yields each window's device tables (boxes, box_stats, stats), launched when it is asked for."""
        from . import ops
        one = hasattr(background, "shape") and len(background.shape) == 3
        for a in range(0, len(scenes), ops.BACKGROUND_MAX_FRAMES):
            b = min(len(scenes), a + ops.BACKGROUND_MAX_FRAMES)
            yield ops.foreground_boxes([s["frame"] for s in scenes[a:b]], background if one else [background[f] for f in range(a, b)], **params)

    @staticmethod
    def _pack_frame_tables(boxes, mid, stats) -> torch.Tensor:
        """Per-frame device tables - boxes [T, K, 4], a [T, K] or [T, K, c] table and stats [T, 4] - side by side as ONE int32 row
        per frame, [T, (4 + c) K + 4], so that one `ops.d2h` reads them all; `_unpack_frame_tables` takes the read-back apart again."""
        return torch.cat([boxes.flatten(1), mid.flatten(1), stats], dim=1)

    @staticmethod
    def _unpack_frame_tables(table, K: int, c: int):
        T = table.shape[0]
        return table[:, :4 * K].reshape(T, K, 4), table[:, 4 * K:(4 + c) * K].reshape(T, K, c), table[:, (4 + c) * K:]

    @classmethod
    def _detected_rows(cls, table) -> list:
        """`detect_vehicles`' read-back, int32 [T, 6 K + 4] = per frame K boxes, K (area, n_cells) and the four stats -> the rows
        of each frame that hold a box (the first min(n_kept, K))."""
        import numpy as np
        K = (table.shape[1] - 4) // 6
        out = []
        for boxes, box_stats, stats in zip(*cls._unpack_frame_tables(table, K, 2)):
            v = min(int(stats[0]), K)
            out.append({"bboxes": boxes[:v].astype(np.int64), "area": box_stats[:v, 0].astype(np.int64), "stats": stats.copy()})
        return out

    def bootstrap_background(self, scenes, max_frames: int = 64, margin: int = 8, rounds: int = 1, min_valid: Optional[int] = None,
                             **params) -> Dict:
        """`estimate_background` for a video that comes without boxes: the median of the sampled frames with no boxes, then `rounds`
        times `detect_vehicles` on those frames against it and the median again with the boxes found (grown by `margin`) kept out.
        A vehicle that stands through the sampled frames but changes its look is baked into the first median and marked
        (count < min_valid) by the second; one that never changes is background to both.  params go to `detect_vehicles`.
        Returns `estimate_background`'s dict plus 'bboxes': the last round's int64 [V_f, 4] half-open boxes per sampled frame.
        Nothing is put into the scenes."""
        import numpy as np

        from . import ops
        idx, mv = self._background_sample(scenes, max_frames, min_valid)
        sampled = [scenes[i] for i in idx]
        frames = [s["frame"] for s in sampled]
        bg, count = ops.background_median(frames, None, margin=margin, min_valid=mv)
        found = [np.zeros((0, 4), dtype=np.int64) for _ in idx]
        for _ in range(int(rounds)):
            found = [d["bboxes"] for d in self.detect_vehicles(sampled, bg, **params)]
            bg, count = ops.background_median(frames, [b - np.asarray([0, 0, 1, 1]) for b in found], margin=margin, min_valid=mv)   # inclusive ends
        return {"background": bg, "count": count, "frames": idx, "min_valid": mv, "bboxes": found}

    def track_vehicles(self, scenes, background, iou=(3, 10), max_gap: int = 2, predict: int = 1, max_tracks: int = 1024,
                       min_hits: int = 3, **params):
        """A tracker's file without a tracker: the vehicles of a video's successive frames with an identity that lasts.  scenes:
        the video's scenes in frame order (scene f is frame f), or a list of such lists for several cameras; background: uint8
        [H, W, 3] on the device (e.g. `bootstrap_background`'s), one per camera for several.  Per window of at most 64 frames
        `ops.foreground_boxes` finds each camera's boxes (params: thr, cell, ..., max_boxes, roi) and ONE `ops.link_boxes` launch
        - a workgroup per camera, the state carried from window to window - gives them track ids (iou, max_gap, predict,
        max_tracks), all on the stream; ONE `ops.d2h` at the end reads everything back.  Returns, per camera (a dict for one
        video, a list of dicts for a list of videos):
          'trajectories' float64 [R, 6] = (frame, id, x, y, w, h), the rows `parse_tracking_files` returns, ordered by frame and
                         then detection, of the tracks with at least min_hits observations;
          'scenes'       per scene {'bboxes' int64 [V, 4] half-open (x0, y0, x1, y1), 'ids' int64 [V]} of those rows, for the caller
                         to assign;
          'boxes', 'ids', 'tracks', 'stats', 'box_stats': the raw tables - int32 [T, K, 4], [T, K], [max_tracks, 4] = (first_t,
                         last_t, hits, 0), [4] = `ops.LINK_BOXES_STATS` and the detector's [T, 4].
        The defaults are tried on synthetic scenes only.  Nothing is put into the scenes."""
        import numpy as np

        from . import ops
        one = len(scenes) == 0 or isinstance(scenes[0], dict)
        videos = [scenes] if one else list(scenes)
        bgs = [background] if one else list(background)
        if len(bgs) != len(videos):
            raise ValueError(f"track_vehicles: {len(bgs)} backgrounds for {len(videos)} videos")
        S, K, N, W = len(videos), int(params.get("max_boxes", ops.FOREGROUND_BOXES_MAX)), int(max_tracks), ops.BACKGROUND_MAX_FRAMES
        lens = [len(v) for v in videos]
        if max(lens) == 0:
            empty = [{"trajectories": np.zeros((0, 6)), "scenes": [], "boxes": np.zeros((0, K, 4), np.int32), "ids": np.zeros((0, K), np.int32),
                      "tracks": np.zeros((N, 4), np.int32), "stats": np.zeros((4,), np.int32), "box_stats": np.zeros((0, 4), np.int32)} for _ in videos]
            return empty[0] if one else empty
        dev = bgs[0].device
        state = tracks = ost = None
        parts = []                                                 # per window and camera: [frames, 5 K + 4] rows
        none = (torch.zeros((0, K, 4), dtype=torch.int32, device=dev), None, torch.zeros((0, 4), dtype=torch.int32, device=dev))
        windows = [self._detect_windows(v, bgs[s], params) for s, v in enumerate(videos)]
        for a in range(0, max(lens), W):
            wb, _, ws = zip(*[next(w, none) for w in windows])     # a camera that has ended brings no frames
            if state is None:
                tracks = torch.zeros((S, N, 4), dtype=torch.int32, device=dev)
                ost = torch.zeros((S, 4), dtype=torch.int32, device=dev)
            ids = torch.empty((sum(int(x.shape[0]) for x in wb), K), dtype=torch.int32, device=dev)
            idl, tracks, ost, state = ops.link_boxes(wb, ws, iou=iou, max_gap=max_gap, predict=predict, max_tracks=N, state=state, t0=a,
                                                     out=(ids, tracks, ost))
            parts.append([self._pack_frame_tables(x, i, y) for x, i, y in zip(wb, idl, ws)])
        flat = torch.cat([p.reshape(-1) for w in parts for p in w] + [tracks.reshape(-1), ost.reshape(-1)])
        host = ops.d2h(flat)
        rows, pos = [[] for _ in videos], 0
        for w in parts:
            for s, p in enumerate(w):
                rows[s].append(host[pos:pos + p.numel()].reshape(tuple(p.shape)))
                pos += p.numel()
        tr = host[pos:pos + S * N * 4].reshape(S, N, 4)
        st = host[pos + S * N * 4:].reshape(S, 4)
        out = [self._tracked_rows(np.concatenate(rows[s]), tr[s], st[s], K, int(min_hits)) for s in range(S)]
        return out[0] if one else out

    @classmethod
    def _tracked_rows(cls, table, tracks, stats, K: int, min_hits: int) -> Dict:
        """`track_vehicles`' read-back of one camera, int32 [T, 5 K + 4] = per frame K boxes, K ids and the detector's stats -> its
        dict: the rows of the tracks with at least min_hits observations, in the reference's (frame, id, x, y, w, h) form."""
        import numpy as np
        T = table.shape[0]
        boxes, ids, box_stats = cls._unpack_frame_tables(table, K, 1)
        ids = ids[:, :, 0]
        keep = (ids >= 0) & (tracks[np.maximum(ids, 0), 2] >= min_hits)
        f, k = np.nonzero(keep)                                    # row-major: by frame, then detection
        b = boxes[f, k].astype(np.float64)
        traj = np.stack([f.astype(np.float64), ids[f, k].astype(np.float64), b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1) \
            if len(f) else np.zeros((0, 6))
        per = [{"bboxes": boxes[t][keep[t]].astype(np.int64), "ids": ids[t][keep[t]].astype(np.int64)} for t in range(T)]
        return {"trajectories": traj, "scenes": per, "boxes": boxes.copy(), "ids": ids.copy(), "tracks": tracks.copy(), "stats": stats.copy(),
                "box_stats": box_stats.copy()}

    @staticmethod
    def _composites(paste, out: Dict, box_geom=None) -> Dict:
        """'frame_icn' and 'frame_vunet': paste(crops, **box) once per composite (:184-198, :236-250; :393-410, :428-445), the
        driver's paste function closed over its bases, rows, crop rows and masks.  box_geom (`_box_rows`): with inpainting every
        vehicle's inpainted box goes under its crop, in vehicle order (:130-145, :340-350)."""
        box = {} if box_geom is None else dict(box_images=out["inpaint_u8"], box_geom=box_geom)
        return {k: paste(out[c], **box) for k, c in (("frame_icn", "icn_u8"), ("frame_vunet", "vunet_u8"))}

    @staticmethod
    def _paste_frames(bases, frame_rows, crops, geom, masks, box_images=None, box_geom=None) -> torch.Tensor:
        """`paste_back_ragged_device` over any number of frames: consecutive chunks of at most `_lib.MAX_FRAMES` frames, one launch
        each over the chunk's own rows, the composites concatenated.  Up to MAX_FRAMES frames it is that one launch."""
        from . import _lib as L
        from .warp_learn import planes_utils as pu
        parts = []
        for lo in range(0, len(bases), L.MAX_FRAMES):
            hi = min(len(bases), lo + L.MAX_FRAMES)
            r = slice(frame_rows[lo], frame_rows[hi])
            parts.append(pu.paste_back_ragged_device(bases[lo:hi], [x - r.start for x in frame_rows[lo:hi + 1]], crops[r], geom[r], masks[r],
                                                     None if box_images is None else box_images[r],
                                                     None if box_geom is None else box_geom[r]))
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    @staticmethod
    def _cat_rows(scenes, k) -> torch.Tensor:
        """The scenes' per-vehicle tensor `k` in row order (one scene: its own tensor, nothing copied)."""
        return scenes[0][k] if len(scenes) == 1 else torch.cat([sc[k] for sc in scenes])

    @torch.no_grad()
    def _frame_local(self, scene, replay=False):
        """The per-vehicle part of a frame for the vehicles `scene` lists (all of them, or one rank's shard): glue, the
        networks, Lab -> BGR.  Returns 'kp_idx', 'icn_u8' (BGR), 'vunet_u8', 'geom' (+ 'inpaint_u8'), device tensors."""
        import numpy as np

        from . import frame_ops as fo
        from . import ops
        from .warp_learn import planes_utils as pu
        dev = self.device
        frame = scene["frame"]
        H, W, _ = frame.shape
        bboxes = np.asarray(scene["bboxes"]).reshape(-1, 4)
        V, R = bboxes.shape[0], 256
        seeds = scene.get("vehicle_seeds")
        with torch.cuda.device(dev):
            inp = scene.get("inpaint") if self.inpaint else None
            ec_form = inpaint_scene_form(inp) if self.inpaint else None
            if V == 0:                                            # no vehicle in the frame (or an empty shard)
                # an empty shard still hands out a (zero-vehicle) state, so that `run_later_frame` takes part in the gathers
                return self._no_vehicles(R, "kp_idx", "icn_u8", "vunet_u8", "geom", *(("inpaint_u8",) if inp is not None else ()),
                                         *(("cad_idx",) if self.cad is not None else ()), "mu_app_0", "mu_app_1", "central")
            pkey = (V, ops.PRECISION) + (("kp_given",) if scene.get("_hg") is not None else ())
            replay, tgt, _ = self._pass_buffers(pkey, replay, V, V)
            # ---- host: the homography fits of every plane of every vehicle (1.2 ms for 8 vehicles), before any launch
            jobs = None if self.device_homography else \
                pu.warp_jobs_frame(scene["src_kp"], scene["dst_kp"], scene["src_vis"], scene["dst_vis"])
            # ---- :121 from a detector mask: EdgeConnect's inputs built on the inpaint branch's stream, beside the glue below
            ec, ec_join = self._inpaint_inputs(frame, inp, tgt) if ec_form in ("det_masks", "box_masks") else (None, None)
            # ---- uint8 glue on the caller's stream
            geom_box = fo.box_geometry((H, W), bboxes, dev)
            img_bbox = fo.crop_resize(frame, geom_box, (R, R), 0)                              # :58-60
            hg_x = fo.crop_resize(frame, geom_box, (R, R), 1, fo.IMAGENET_MEAN, fo.IMAGENET_STD, out=tgt.get("hg_x"))   # :61-65
            central = fo.central_crop(img_bbox)                                                # vehicle_utils.py:49-52
            warped = self._warp_planes(scene, jobs)                                            # :171-175
            _, geom = fo.mask_bbox_geom(scene["masks"])
            icn_x = pu.icn_inputs_device(warped, scene["dst_sketch"], central, geom, R, R, out=tgt.get("icn_x"))   # :179-180
            vu_x, vu_y = fo.vunet_inputs(frame, scene["masks"], scene["src_sketch"], scene["dst_sketch"], geom, R,
                                         out=(tgt["vu_x"], tgt["vu_y"]) if tgt else None)       # :203-228
            # ---- the three networks: the crop pass of `run` (three stream branches), eagerly or as one plan replay
            nets_in = {"hg_x": hg_x, "icn_x": icn_x, "vu_x": vu_x, "vu_y": vu_y}
            if scene.get("_hg") is not None:                      # geometry mode: keypoints (and CAD logits) already computed
                nets_in.update(scene["_hg"])
            if ec is not None:                                    # :121: create_inpaint_inputs_shape's four tensors, built above
                ec_join()
                nets_in.update({"ec_" + k: ec[k] for k in ops.INPAINT_KEYS})
            elif inp is not None:                                 # ... or given
                nets_in.update(ec_img=inp["img"], ec_gray=inp["gray"], ec_edge=inp["edge"], ec_mask=inp["mask"])
            out = self._nets_pass(self._run, pkey, replay, nets_in, seeds,                     # :75-79, :182, :230-234
                                  clone=("vunet_u8", "kp_idx", "inpaint_u8", "cad_logits", "mu_app_0", "mu_app_1"))
            out["geom"] = geom
            out["central"] = central
            if "cad_logits" in out:
                out["cad_idx"] = out.pop("cad_logits").argmax(1)                               # :69
        return out

    def _inpaint_inputs(self, frame, inp, tgt):
        """EdgeConnect's four inputs from scene['inpaint'] = {'boxes', 'det_masks'} (`ops.inpaint_inputs`) or {'boxes',
        'box_masks'} (`ops.inpaint_inputs_boxed`), issued on the inpaint branch's stream, forked from the current one; `tgt`: a
        recorded pass's input buffers, written in place.  Returns (the four tensors, join): join() makes the current stream
        wait for them."""
        from . import ops
        out = {k: tgt["ec_" + k] for k in ops.INPAINT_KEYS} if tgt else None

        def build():
            if "box_masks" in inp:
                return ops.inpaint_inputs_boxed(frame, inp["box_masks"], inp["boxes"], out=out)
            return ops.inpaint_inputs(frame, inp["det_masks"], inp["boxes"], out=out)

        return self._on_inpaint_stream(build, tgt)

    def _warp_planes(self, scene, jobs):
        """The source planes warped to the destination pose: from the host-fitted `jobs`, or (device_homography) from the
        tables one kernel fits on the device."""
        from .warp_learn import planes_utils as pu
        if not self.device_homography:
            return pu.warp_planes_batch(scene["src_planes"], jobs)
        if scene.get("src_kp_d") is not None and scene.get("dst_kp_d") is not None:
            # device_pose: the corner points never left the device; the visibilities come from the read-back counts
            import numpy as np

            from . import ops
            vis = [ops.h2d((np.asarray(scene[k]).reshape(-1, 5) != 0).astype(np.uint8), self.device) for k in ("src_vis", "dst_vis")]
            minv, index = pu.plane_homographies_device(scene["src_kp_d"], scene["dst_kp_d"], vis[0], vis[1], nverts=scene["kp_nv_d"])
        else:
            minv, index = pu.plane_homographies_device(scene["src_kp"], scene["dst_kp"], scene["src_vis"], scene["dst_vis"], self.device)
        return pu.warp_planes_fitted(scene["src_planes"], minv, index)

    @torch.no_grad()
    def _frame_finish(self, scene, out):
        """The frame-level part, on the rank that holds every vehicle's crops (`out`: _frame_local's dict for ALL the
        scene's vehicles, in vehicle order): keypoints -> frame pixels -> pose fit, ordered paste into the two frames."""
        import numpy as np

        from . import frame_ops as fo
        from . import ops
        from .utils.pnp_utils import cpc_fit_device
        from .warp_learn import planes_utils as pu
        dev = self.device
        frame = scene["frame"]
        H, W, _ = frame.shape
        bboxes = np.asarray(scene["bboxes"]).reshape(-1, 4)
        V, R = bboxes.shape[0], 256
        inp = scene.get("inpaint") if self.inpaint else None
        out = dict(out)
        with torch.cuda.device(dev):
            back = self._paste_base(scene)
            if V == 0:
                out["kp_xy"] = torch.empty((0, 12, 2), dtype=torch.float32, device=dev)
                out["_pose_raw"] = tuple(torch.empty(sh, dtype=torch.float32, device=dev) for sh in ((0, 4, 3), (0, 4, 3), (0, 4)))
                out["frame_icn"], out["frame_vunet"] = back.clone(), back.clone()
                return out
            f32 = lambda a: ops.h2d(np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32).reshape(-1, 2), (V, 2))), dev)   # noqa: E731
            if scene.get("_pose_raw") is not None:
                kp3d = None
            elif self.cad is not None and scene.get("kp3d_bank") is not None:                  # :82-88: the chosen CAD model's keypoints
                kp3d = ops.h2d(np.asarray(scene["kp3d_bank"], np.float32), dev)[out["cad_idx"]]
            else:
                kp3d = ops.h2d(np.asarray(scene["kp3d"], np.float32), dev)
            geom_box = fo.box_geometry((H, W), bboxes, dev)
            out["kp_xy"] = fo.keypoints_to_frame(out["kp_idx"], geom_box, (R // 4, R // 4))   # :95-97 (64 x 64 heat-maps)
            if scene.get("_pose_raw") is not None:               # geometry mode: the pose was fitted before the render
                out["_pose_raw"] = scene["_pose_raw"]
            else:
                out["_pose_raw"] = cpc_fit_device(f32(scene["focals"]), f32(scene["centers"]), out["kp_xy"], kp3d)   # :104-105
            out.update(self._composites(lambda crops, **box: pu.paste_back_device(back, crops, out["geom"], scene["masks"], **box), out,
                                        None if inp is None else self._box_rows([inp["boxes"]])))
            if "mu_app_0" in out:                                 # what `run_later_frame` renders these vehicles' future frames with
                out["state"] = {"appearance": [out.pop("mu_app_0"), out.pop("mu_app_1")], "central": out.pop("central"),
                                "shard": (0, V, V), "sharded": False}
        return out

    # ------------------------------------------------------------------------------------------ future frames of a clip
    def run_later_frame(self, scene: Dict, state: Dict, check: Optional[str] = "sync", replay: bool = False) -> Dict:
        """A FUTURE frame of vehicles whose first frame `run_frame` rendered (trajectory_inference.py:283-450, per vehicle and
        trajectory step): no hourglass, no pose fit, no appearance encoder - the source planes warped to the new pose -> ICN
        inputs (with the first frame's central crop) -> ICN -> Lab image (:376-391); the new sketch -> VUnet shape encoder ->
        decoder conditioned on the FIRST frame's appearance code (:415-426); ordered paste of both (:393-410, :428-445).

        scene: as for `run_frame`, but rendered for the new pose - 'frame' (what is pasted onto; 'background' overrides),
        'masks', 'dst_sketch', 'dst_kp', 'dst_vis' of the new pose, 'src_planes' / 'src_kp' / 'src_vis' of the first frame,
        optional 'vehicle_seeds' (the shape decoder draws its sampler noise: a seed per vehicle and frame keeps a vehicle's
        images independent of batching); state: `run_frame(...)["state"]` of the same vehicles, same order.
        replay=True issues the two networks (ICN, VUnet shape half) as ONE recorded-plan replay per vehicle count, like
        `run_frame(replay=True)`: five of a clip's six frames are later frames, and at 8 vehicles the interpreter bounds the eager form.
        With a pipeline built with inpaint=True the scene may carry 'inpaint' in any of `run_frame`'s three forms, for THIS frame's
        boxes (:301-350): EdgeConnect's inputs come from this scene's frame, EdgeModel -> InpaintingModel -> merge runs as a third
        stream branch, the composite starts from the frame ('background' is ignored, :340) and every vehicle's inpainted box is
        pasted under its crop in vehicle order; the result gains 'inpaint_u8' [V, R, R, 3].  Without the key (or with
        inpaint=False, which ignores it) nothing changes.  replay=True keeps the inpaint pass as a recorded plan of its own.
        Returns 'icn_u8' / 'vunet_u8' uint8 [V, R, R, 3] (BGR), 'frame_icn' / 'frame_vunet' uint8 [H, W, 3], 'geom'.

        Geometry mode (state of a geometry-mode `run_frame`, a scene without 'masks'): see `_geometry_later_frame`."""
        if self._is_geometry(scene, state):
            return self._geometry_later_frame(scene, state, check, replay)
        rng = torch.get_rng_state() if (check == "sync" and scene.get("vehicle_seeds") is None) else None
        import torch.distributed as dist
        if not _one_rank(self.group) and state.get("sharded"):
            # a clip sharded over ranks (north_star: "vehicles-in-a-frame and frames-in-a-clip shard"): every rank passes the
            # same scene and ITS OWN state (run_frame's, rank-local); it renders its vehicles [lo, hi) from the appearance codes
            # it kept, the uint8 crops and crop rows travel to rank 0, which pastes in vehicle order.  As for the first
            # frame the range guard runs before the collectives.  Rank 0 returns the result, the others None.
            lo, hi, V = state["shard"]
            if int(scene["masks"].shape[0]) != V:
                raise ValueError(f"run_later_frame: the state was made for a frame of {V} vehicles, the scene holds {int(scene['masks'].shape[0])}")
            local = self._guarded(self._later_local, (slice_scene(scene, lo, hi), state, replay), check, rng)
            # (every rank holds the same scene, so all of them gather 'inpaint_u8' or none does)
            full = self._gather_local(local, V, False, self._later_inpaint(scene) is not None)
            return None if full is None else self._later_finish(scene, full)
        return self._guarded(self._run_later_frame, (scene, state, replay), check, rng)

    def _run_later_frame(self, scene, state, replay=False):
        return self._later_finish(scene, self._later_local(scene, state, replay))

    @torch.no_grad()
    def _later_nets(self, batch, vehicle_seeds=None):
        """The two networks of a later frame (trajectory_inference.py:389, :424-426) as a pass function (`CompiledPass(fn=...)`):
        batch = 'icn_x' [V, 21, R, R], 'vu_y' [V, 3, R, R], 'app0' / 'app1' = the first frame's appearance code; with 'ec_img',
        'ec_gray', 'ec_edge', 'ec_mask' EdgeModel -> InpaintingModel -> merge (:328-336) runs as a third branch -> 'inpaint_u8'."""
        from . import ops
        self.vunet.set_vehicle_seeds(vehicle_seeds)

        def icn():
            return {"icn_u8": ops.to_image_u8(self.icn(batch["icn_x"]))}                   # :389

        def vunet():
            vu = self.vunet
            do, ds = vu.forward_dec_up(batch["vu_y"])                                      # :424
            xt, _, _ = vu.forward_dec_down(do, ds, [batch["app0"], batch["app1"]])         # :425
            return {"vunet_u8": ops.to_image_u8(xt)}                                       # :426

        def inpaint():
            e = self.edge(batch["ec_gray"], batch["ec_edge"], batch["ec_mask"])            # :328-336
            p = self.inp(batch["ec_img"], e, batch["ec_mask"])
            return {"inpaint_u8": ops.merge_u8(p, batch["ec_img"], batch["ec_mask"])}

        return self._branches([("icn", icn), ("vunet", vunet)] + ([("inpaint", inpaint)] if "ec_img" in batch else []))

    def _later_inpaint(self, scene):
        """A later scene's 'inpaint' entry, for a pipeline built with inpaint=True (None: today's path without inpainting)."""
        return scene.get("inpaint") if self.inpaint else None

    @torch.no_grad()
    def _later_local(self, scene, state, replay=False):
        """The per-vehicle part of a later frame for the vehicles `scene` lists (all, or one rank's shard - `state` holds
        exactly these vehicles): warp, ICN, VUnet shape half (+ EdgeConnect on THIS frame's boxes when the scene carries
        'inpaint', :301-350).  Returns 'icn_u8' (BGR), 'vunet_u8', 'geom' (+ 'inpaint_u8')."""
        from . import frame_ops as fo
        from . import ops
        from .warp_learn import planes_utils as pu
        dev = self.device
        frame = scene["frame"]
        R = 256
        V = int(scene["masks"].shape[0])
        if state["central"].shape[0] != V:
            raise ValueError(f"run_later_frame: the state holds {state['central'].shape[0]} vehicles, the scene {V}")
        inp = self._later_inpaint(scene)
        ec_form = inpaint_scene_form(inp) if inp is not None else None
        with torch.cuda.device(dev):
            if V == 0:
                return self._no_vehicles(R, "icn_u8", "vunet_u8", "geom", *(("inpaint_u8",) if inp is not None else ()))
            # (an inpaint marker in the key: the plans of scenes without 'inpaint' are the ones recorded before)
            pkey = ("later", V, ops.PRECISION) + (("inpaint",) if inp is not None else ())
            replay, tgt, _ = self._pass_buffers(pkey, replay, V, V)   # (tgt: only a recorded pass's EdgeConnect inputs are written in place)
            jobs = None if self.device_homography else \
                pu.warp_jobs_frame(scene["src_kp"], scene["dst_kp"], scene["src_vis"], scene["dst_vis"])
            # ---- :326 from a detector mask: EdgeConnect's inputs of this frame's boxes, on the inpaint branch's stream
            ec, ec_join = self._inpaint_inputs(frame, inp, tgt) if ec_form in ("det_masks", "box_masks") else (None, None)
            warped = self._warp_planes(scene, jobs)                                            # :376-381
            _, geom = fo.mask_bbox_geom(scene["masks"])
            icn_x = pu.icn_inputs_device(warped, scene["dst_sketch"], state["central"], geom, R, R)   # :385-387
            _, vu_y = fo.vunet_inputs(frame, scene["masks"], scene["dst_sketch"], scene["dst_sketch"], geom, R)   # :415-420 (y_tilde only)
            seeds = scene.get("vehicle_seeds")
            nets_in = {"icn_x": icn_x, "vu_y": vu_y, "app0": state["appearance"][0], "app1": state["appearance"][1]}
            if ec is not None:
                ec_join()
                nets_in.update({"ec_" + k: ec[k] for k in ops.INPAINT_KEYS})
            elif inp is not None:                                 # given
                nets_in.update(ec_img=inp["img"], ec_gray=inp["gray"], ec_edge=inp["edge"], ec_mask=inp["mask"])
            out = self._nets_pass(self._later_nets, pkey, replay, nets_in, seeds)
            out["geom"] = geom
        return out

    @torch.no_grad()
    def _later_finish(self, scene, out):
        """The frame-level part of a later frame, on the rank that holds every vehicle's crops: the ordered paste."""
        from .warp_learn import planes_utils as pu
        out = dict(out)
        inp = self._later_inpaint(scene)
        with torch.cuda.device(self.device):
            back = self._paste_base(scene)
            if int(scene["masks"].shape[0]) == 0:
                out["frame_icn"], out["frame_vunet"] = back.clone(), back.clone()
                return out
            out.update(self._composites(lambda crops, **box: pu.paste_back_device(back, crops, out["geom"], scene["masks"], **box), out,
                                        None if inp is None else self._box_rows([inp["boxes"]])))
        return out

    def run_later_frames(self, scenes, state: Dict, replay: bool = False):
        """`run_later_frame` over the later frames of a clip with ONE frame in flight, like `run_frames` for first frames: frame i+1
        is issued - its homographies fitted on the host, its launches queued - before frame i's range status is read back (pinned,
        one event per frame), so the host part of a later frame (1 ms of homography fits) and the read-back overlap the previous
        frame's networks.  A generator: one `run_later_frame`-shaped dict per scene, in order; a frame whose status is raised is
        redone in exact fp32 before it is yielded.  The state of a geometry-mode first frame (scenes with 'steps', no 'masks') is
        pipelined the same way, its render and covered-count read-back on the pipeline's geometry stream.  A sharded state
        (process group, geometry mode included) is not pipelined: frame by frame."""
        if not _one_rank(self.group) and state.get("sharded"):
            for sc in scenes:
                yield self.run_later_frame(sc, state, replay=replay)
            return
        ready = self._scenes_ready(scenes)
        yield from self._one_in_flight(scenes, lambda scene: self._issue_later(scene, state, replay, ready), self._collect_later)

    def _issue_later(self, scene, state, replay, ready=None):
        """A later frame issued without waiting for it (the counterpart of `_issue_frame`)."""
        from . import ops
        rng = torch.get_rng_state() if (ops.range_guarded() and scene.get("vehicle_seeds") is None) else None
        front = None
        with torch.cuda.device(self.device):
            if self._is_geometry(scene, state):                  # the render on the geometry stream first
                front = self._issue_geometry_front(lambda: self._geometry_later_front(scene, state), ready)
                scene_nets, state_nets = front["sub"], front["sub_state"]
            else:
                scene_nets, state_nets = scene, state
            out, ticket = self._issue_guarded(lambda: self._run_later_frame(scene_nets, state_nets, replay))
        return {"out": out, "ticket": ticket, "scene": scene, "state": state, "rng": rng, "front": front}

    def _collect_later(self, t):
        hit, front = self._status_raised(t["ticket"]), t["front"]
        if front is not None:
            hit = self._status_raised(front.pop("_ticket"), wait=False) or hit
        if hit:                                                   # rare: this frame again, in exact fp32
            return _redo_f32(lambda: self.run_later_frame(t["scene"], t["state"], check=None, replay=False), t["rng"], restore=True)
        return t["out"] if front is None else self._geometry_later_assemble(front, t["out"])

    # ---- the future frames of a clip as ONE pass: the networks at B = F * V
    def run_later_frames_batched(self, scenes, state: Dict, replay: bool = False, check: Optional[str] = "sync",
                                 max_batch: Optional[int] = None) -> list:
        """`run_later_frame` for the F future frames of a clip at once: five of a clip's six frames are later frames of the SAME
        vehicles, and frame by frame each is a pass of ~300 dependent launches at batch V.  Here everything between the uint8
        frames and the composited uint8 frames is issued once for all F * V (frame, vehicle) pairs - one plane warp
        (fusg_warp_perspective_clips_u8, the first frame's planes passed by pointer, not copied), one mask_bbox_geom, icn_inputs
        and vunet_inputs, `_later_nets` once at B = F * V, one lab2bgr and one ordered paste per composite for every 64 frames
        (fusg_paste_layers_ragged_u8).  A group is run as the several-clip pass of ONE clip (`_run_later_clips`), whose rows
        are these: frame-major, row f * V + v is frame f, vehicle v; the first frame's central crops and appearance codes
        are repeated per frame, per-frame 'vehicle_seeds' concatenated in row order.

        scenes: a sequence of F later scenes as `run_later_frame` takes them (same vehicles and order as `state`; each its own
        'frame', 'masks', 'dst_*', optional 'background', 'vehicle_seeds', 'inpaint'); every scene's 'src_planes' is the first
        frame's tensor (one tensor, shared).  Either all scenes carry 'vehicle_seeds' or none (ValueError otherwise; without
        seeds the noise of the pass is drawn in row order, which is not the order of F separate frames).  With a pipeline built
        with inpaint=True either all scenes carry 'inpaint' (any of the three forms, per scene) or none (ValueError): each
        frame's EdgeConnect inputs are built from that frame's own image on the inpaint stream into its V rows of the batched
        buffers, then EdgeModel -> InpaintingModel -> merge runs once at F * V.
        replay=True: the two (three) networks are ONE recorded plan per (F, V, precision[, inpaint]), kept with the frame
        drivers' other plans under ("later_batch", F, V, ...) - apart from the ("later", V, ...) plans of `run_later_frame`.
        check: the range guard of `run` - one status word per pass; raised, the whole pass is redone in exact fp32 under the RNG
        state it was issued with.
        max_batch bounds the rows of a pass: the frames are split into consecutive groups of max(1, max_batch // V) frames, one
        pass each (`later_batch_groups`).  Default LATER_MAX_BATCH = 64 rows, the largest batch the frame drivers run anyway (a
        frame of 64 vehicles), so the networks' activations stay what that pass already needs; the warped planes take 5 * H * W
        * 3 bytes per row - 13.8 MB at 720 x 1280, 885 MB for 64 rows (553 MB for a clip tail of 5 frames of 8 vehicles).
        One warp launch takes 65535 (row, plane) jobs: a max_batch that makes a group of more than 13107 rows at 5 planes is a
        ValueError before anything is launched.
        Returns a list of F dicts with `run_later_frame`'s keys and shapes, in scene order ('icn_u8', 'vunet_u8', 'geom',
        'frame_icn', 'frame_vunet' (+ 'inpaint_u8')); a frame's tensors are views into the pass's stacked results.  V = 0: F
        results of `run_later_frame`'s no-vehicle shape; F = 0: [].
        A geometry-mode state (scenes without 'masks') and a sharded state (process group) go through `run_later_frames`, frame
        by frame - the results of today; `run_later_frames_batched_geometry` is the opt-in that batches a geometry-mode state
        (this method's parameter list is pinned, so the flag lives on a sibling)."""
        return self._later_frames_batched(scenes, state, replay, check, max_batch, False)

    def run_later_frames_batched_geometry(self, scenes, state: Dict, replay: bool = False, check: Optional[str] = "sync",
                                          max_batch: Optional[int] = None, batch_geometry: bool = True) -> list:
        """`run_later_frames_batched` that also batches a GEOMETRY-MODE state (scenes with 'steps', no 'masks'; batch_geometry=False:
        exactly `run_later_frames_batched`, the frame-by-frame fallback).  Frame by frame such a later frame blocks on a
        device-to-host copy between its render and its plane warp (`render.vehicle_geometry_device`), because the visibilities
        and the skip rule were decided on the host, and its networks run at batch "kept vehicles".  Here a group of
        `later_batch_groups(F, V, max_batch)` frames is queued whole before anything is read, as the several-clip pass of one
        clip: `render.later_geometry_clips_device` (one upload of the steps, the camera and the source visibilities ->
        fusg_pose_geometry_clips -> fusg_render_normals_u8 -> fusg_plane_visibility -> fusg_later_gate at F * V rows) ->
        `plane_homographies_device` from device corner points and gated visibilities -> the plane warp
        (fusg_warp_perspective_clips_u8, the state's planes passed by pointer) -> crop rows and both networks' inputs ->
        `_later_nets` at F * V -> Lab -> BGR -> the ordered paste of all frames (fusg_paste_layers_ragged_u8); then ONE `ops.d2h`
        of the stage's small packed buffer, from which the per-frame results are cut.  V = the state's vehicles, rows
        frame-major, the plan of replay=True is the ("later_batch", F, V, precision[, "inpaint"]) plan a given-geometry batch of that
        shape uses: its shape no longer depends on what rendered.
        A vehicle whose render is empty (covered == 0, the reference's `except: break`) stays in the batch as an INERT row:
        its gated visibilities are zero, so no plane is warped for it; its mask is empty, so its crop row is all zero, its network
        inputs are black and nothing of it is pasted; with inpainting its box row is zeroed by the gate ("a skipped vehicle is not
        inpainted").  Its network outputs are dropped from the result.
        Needs a pipeline built with device_pose=True and device_homography=True (ValueError before any launch otherwise: those
        are the paths whose per-row arithmetic this stage repeats, so it equals the per-frame device path byte for byte); a state
        made without device copies uploads its host pose and corner points once.  'vehicle_seeds' and 'inpaint' list every
        first-frame vehicle, like 'steps'; either every scene carries them or none does.  A sharded state keeps falling back; a
        non-geometry state ignores the flag.  The range guard is `run_later_frames_batched`'s: one status word per group, a raised
        word redoes the group in exact fp32.
        Memory per row at H x W: 19 * H * W bytes (sketch 3, mask 1, warped planes 15) - 17.5 MB at 720 x 1280, 1.1 GB at 64 rows
        (the given-geometry batch's 13.8 MB per row are the warped planes alone: its masks and sketches are the caller's).
        Returns a list of F dicts with `run_later_frame`'s geometry-mode keys: 'icn_u8', 'vunet_u8', 'geom' (+ 'inpaint_u8') of the
        kept vehicles in order, 'frame_icn', 'frame_vunet', 'geometry' ('masks', 'dst_sketch', 'dst_kp', 'dst_vis', 'kp3d' of
        every vehicle of the state) and 'skipped'."""
        return self._later_frames_batched(scenes, state, replay, check, max_batch, bool(batch_geometry))

    def _later_frames_batched(self, scenes, state, replay, check, max_batch, batch_geometry) -> list:
        scenes = list(scenes)
        F = len(scenes)
        if F == 0:
            return []
        geometry = any(self._is_geometry(sc, state) for sc in scenes)
        if (not _one_rank(self.group) and state.get("sharded")) or (geometry and not batch_geometry):
            return list(self.run_later_frames(scenes, state, replay=replay))
        if geometry:
            return self._later_geometry_batched(scenes, state, replay, check, max_batch)
        V = int(state["central"].shape[0])
        for f, sc in enumerate(scenes):
            if int(sc["masks"].shape[0]) != V:
                raise ValueError(f"run_later_frames_batched: the state holds {V} vehicles, scene {f} {int(sc['masks'].shape[0])}")
        seeds = later_batch_seeds([sc.get("vehicle_seeds") for sc in scenes], V)
        _batch_inpaint("run_later_frames_batched", range(F), [self._later_inpaint(sc) for sc in scenes], "of the batch", "frames")
        if V == 0:
            return [self._run_later_frame(sc, state) for sc in scenes]
        if any(sc["src_planes"].data_ptr() != scenes[0]["src_planes"].data_ptr() or sc["src_planes"].shape != scenes[0]["src_planes"].shape
               for sc in scenes):
            raise ValueError("run_later_frames_batched: the scenes of a batch share the first frame's 'src_planes' (one tensor)")
        return self._later_one_clip_groups(scenes, state, replay, check, max_batch, seeds, False)

    def _later_one_clip_groups(self, scenes, state, replay, check, max_batch, seeds, geometry: bool) -> list:
        """The validated later scenes of ONE clip with vehicles as guarded passes, one per group of `later_batch_groups`: each
        group is `_run_later_clips` over a group of one clip - whose rows ARE the frame-major F * V rows -, unpadded, its plan
        kept under the one-clip key ("later_batch", F, V, ...).  The several-clip warp takes at most 65535 (row, plane) jobs
        per launch, so a group of more than 65535 // P rows (13107 at 5 planes; a max_batch far beyond anything the project
        runs) is a ValueError before anything is launched."""
        V = int(state["central"].shape[0])
        P = int((state["geometry"] if geometry else scenes[0])["src_planes"].shape[1])
        groups = later_batch_groups(len(scenes), V, max_batch)
        rows = max(hi - lo for lo, hi in groups) * V
        if rows * P > 65535:
            raise ValueError(f"run_later_frames_batched{'_geometry' if geometry else ''}: a group of {rows} rows of {P} planes exceeds "
                             f"the 65535 warp jobs of one launch (max_batch at most {65535 // P})")
        return [res for lo, hi in groups
                for res in self._guarded_pass(lambda *a: self._run_later_clips(*a)[0],
                                              ([(scenes[lo:hi], state)], replay, None, geometry, ("later_batch", hi - lo, V)), check, seeds)]

    def _later_fits(self, scenes):
        """The plane homographies of the scenes' vehicles, in row order, from their host corner points and visibilities: the
        (minv, index) tables one kernel fits (device_homography), or the host-fitted jobs - what the driver's warp takes."""
        import numpy as np

        from .warp_learn import planes_utils as pu
        kp = {k: [veh for sc in scenes for veh in sc[k]] for k in ("src_kp", "dst_kp")}
        vis = {k: np.concatenate([np.asarray(sc[k]).reshape(-1, 5) for sc in scenes]) for k in ("src_vis", "dst_vis")}
        if self.device_homography:
            return pu.plane_homographies_device(kp["src_kp"], kp["dst_kp"], vis["src_vis"], vis["dst_vis"], self.device)
        return pu.warp_jobs_frame(kp["src_kp"], kp["dst_kp"], vis["src_vis"], vis["dst_vis"])

    # ---- the same for a geometry-mode state: the render, the visibilities and the skip rule stay on the device
    def _later_geometry_batched(self, scenes, state, replay, check, max_batch) -> list:
        """`run_later_frames_batched_geometry` for F geometry-mode scenes on one rank: validation, then one guarded pass per group."""
        gs = state["geometry"]
        veh = list(gs["vehicles"])
        V = len(veh)
        seeds, inpaint = later_geometry_batch_rows(scenes, veh, self.device_pose, self.device_homography, self.inpaint)
        if int(state["central"].shape[0]) != V:
            raise ValueError(f"run_later_frames_batched_geometry: the state holds {int(state['central'].shape[0])} crops for {V} vehicles")
        if any(tuple(sc["frame"].shape) != tuple(scenes[0]["frame"].shape) for sc in scenes):
            raise ValueError("run_later_frames_batched_geometry: the frames of a batch have one size")
        if V == 0:
            return list(self.run_later_frames(scenes, state, replay=replay))
        return self._later_one_clip_groups(self._geometry_row_scenes(scenes, veh, inpaint), state, replay, check, max_batch, seeds, True)

    def _geometry_row_scenes(self, scenes, veh, inpaint: bool) -> list:
        """The rows' scenes of a geometry-mode batch: 'vehicle_seeds' and 'inpaint' list every first-frame vehicle and are selected
        to the state's vehicles `veh` (inpaint False: the key is dropped)."""
        rows = []
        for sc in scenes:
            r = dict(sc)
            if sc.get("vehicle_seeds") is not None:
                r["vehicle_seeds"] = [sc["vehicle_seeds"][v] for v in veh]
            if inpaint:
                r["inpaint"] = self._select(sc["inpaint"], veh, list(sc["inpaint"].keys()))
            elif "inpaint" in r:
                del r["inpaint"]
            rows.append(r)
        return rows

    def _geometry_state_device(self, gs: Dict) -> Dict:
        """What a batched geometry stage reads of a first frame's state['geometry'], on the device: 'pose_d' float32 [V, 7],
        'cad_idx_d' int64 [V], 'src_kp_d' int32 [V, 5, 8, 2], 'kp_nv_d' int32 [5].  A state made without device copies uploads its
        host pose, CAD indices and corner points."""
        import numpy as np

        from . import ops
        from . import render as rd
        from .warp_learn import planes_utils as pu
        dev, V = self.device, len(gs["vehicles"])
        pose_d, cad_d = gs.get("pose_d"), gs.get("cad_idx_d")
        if pose_d is None:
            prow = [[p[0], *np.asarray(p[1]).reshape(3), *np.asarray(p[2]).reshape(3)] for p in gs["pose"]]
            pose_d = ops.h2d(np.asarray(prow, np.float32).reshape(V, 7), dev)
            cad_d = ops.h2d(np.asarray(gs["cad_idx"], np.int64).reshape(V), dev)
        src_kp_d, kp_nv_d = gs.get("src_kp_d"), gs.get("kp_nv_d")
        if src_kp_d is None:
            pts, nv = pu.pack_plane_points(gs["src_kp"], len(rd.TEXTURE_PLANES))
            src_kp_d, kp_nv_d = ops.h2d(pts, dev), ops.h2d(np.ascontiguousarray(nv[0]), dev)
        return {"pose_d": pose_d, "cad_idx_d": cad_d, "src_kp_d": src_kp_d, "kp_nv_d": kp_nv_d}

    def _geometry_cut(self, res: Dict, sl: slice, veh, scene: Dict, geo: Dict, host: Dict, inpaint: bool) -> Dict:
        """One frame of a batched geometry pass as `_geometry_later_frame` returns it: `res` holds the frame's rows `sl` of the
        stacked results; the inert rows' network outputs are dropped, 'geometry' and 'skipped' come from the stage (`geo`) and
        its read-back (`host`).  veh: the state's first-frame vehicle indices."""
        V = len(veh)
        keys = ("icn_u8", "vunet_u8", "geom") + (("inpaint_u8",) if inpaint else ())
        keep = [i for i in range(V) if host["covered"][sl][i] > 0]
        if len(keep) < V:                                         # the inert rows' network outputs are dropped
            idx = torch.as_tensor(keep, dtype=torch.long, device=self.device)
            res = {**res, **{k: res[k].index_select(0, idx) for k in keys}}
        res["geometry"] = {"masks": geo["mask"][sl], "dst_sketch": geo["sketch"][sl], "dst_kp": host["dst_kp"][sl],
                           "dst_vis": host["dst_vis"][sl], "kp3d": host["kp3d"][sl]}
        kept = [veh[i] for i in keep]
        res["skipped"] = [v for v in range(len(scene["steps"])) if v not in kept]
        return res

    # ------------------------------------------------------------------------------------------ first frames of several scenes
    def run_frames_batched(self, scenes, replay: bool = False, check: Optional[str] = "sync", max_batch: Optional[int] = None,
                           pad: Optional[bool] = None) -> list:
        """`run_frame` for the first frames of SEVERAL scenes at once, with ragged vehicle counts V_f: a video frame usually
        carries one to a few selected vehicles, and frame by frame each is a pass of ~300 dependent launches at batch V_f, the
        worst regime the pass has.  The frames are independent of each other and the networks do not know which frame a row came
        from, so everything between the uint8 frames and the composited frames is issued once for all sum(V_f) rows: the box
        geometry rows (one upload), `frame_ops.crop_resize_frames` twice (box crop, hourglass input), the central crop, one plane
        warp over the concatenated source planes (host-fitted jobs, or `device_homography`), `mask_bbox_geom`,
        `icn_inputs_device`, `frame_ops.vunet_inputs_frames`, `_run` once, `lab2bgr`, `keypoints_to_frame`, the pose fit with
        per-row focals and centers, and one ragged paste per composite (`paste_back_ragged_device`).  The three kernels that
        read the frame take a table of frames and row offsets (fusg_crop_resize_frames_u8, fusg_vunet_inputs_frames,
        fusg_paste_layers_ragged_u8); a group's read-back is ONE device-to-host copy of the raw pose fits.  Rows are
        scene-major: scene f's vehicles are rows offsets[f] .. offsets[f + 1] (`frame_batch_offsets`).

        scenes: a sequence of scenes as `run_frame` takes them on the given-geometry path, each with its own 'frame' (all of one
        size: ValueError otherwise, before anything is launched) and its own vehicles; V_f = 0 is allowed.  Per scene
        'background', 'vehicle_seeds', 'inpaint' (any of the three forms), 'kp3d' or 'kp3d_bank' (cad=True), 'focals' and
        'centers' mean what they mean to `run_frame`.  Either every scene that has vehicles carries 'vehicle_seeds' or none does,
        and with a pipeline built with inpaint=True the same holds for 'inpaint' (ValueError otherwise; where none does, the
        refusal is `run_frame`'s own: such a pipeline's first frames need the key); EdgeConnect's inputs are built per scene from
        its own image into its row slice, on the inpaint stream.
        max_batch bounds the rows of a pass and FRAME_BATCH_MAX_FRAMES its scenes: consecutive scenes are packed greedily
        (`frame_batch_groups`; default LATER_MAX_BATCH = 64 rows; a scene with more vehicles is a group of its own).
        pad (None: pad when replay is on): the networks run at `frame_batch_pad(rows, max_batch)` rows - the next of 4, 8, 16,
        32, 64 -, the padding rows of their inputs zero and their seeds 0; the glue writes the real rows and the outputs are cut
        to them before the pose fit and the paste, so no kernel knows about padding.  replay=True: the networks are ONE
        recorded plan per (padded rows, precision[, inpaint][, cad]), kept with the frame drivers' other plans under
        ("frame_batch", padded_rows, ...) - at most five keys for the default max_batch whatever the counts of the video;
        outputs are handed out as copies.  pad=True with replay=False is the eager pass over the same padded rows.
        check: the range guard of `run` - one status word per group; raised, the group is redone in exact fp32 under the RNG
        state it was issued with.
        A batch's crops are not bit for bit those of per-frame passes of the same scenes: another batch size may route the
        convolutions differently (the glue - crops, network inputs, paste - is byte-equal).
        Memory: the scenes' per-vehicle tensors are concatenated - 19 * H * W bytes per row (source planes 15, sketch 3, mask 1;
        17.5 MB at 720 x 1280) plus the warped planes' 15 * H * W, 2.0 GB for 64 rows at 720 x 1280.
        Returns a list of `run_frame`'s dicts in scene order ('kp_idx', 'kp_xy', 'pose', 'icn_u8', 'vunet_u8', 'geom',
        'frame_icn', 'frame_vunet' (+ 'inpaint_u8', 'cad_idx'), 'state' with that scene's rows of the appearance codes and central
        crops, shard (0, V_f, V_f), sharded False - `run_later_frame` and `run_later_frames_batched` take it as they take
        `run_frame`'s); per-vehicle tensors are views into the pass's stacked results.  A scene without vehicles gets
        `run_frame`'s no-vehicle shape, its composites are its base.  [] -> [].
        Geometry-mode scenes (a pipeline with cad_bank, scenes without 'masks') and a process group of more than one rank go
        through `run_frames`, frame by frame - the results of today; a list that mixes geometry-mode and given-geometry scenes
        is a ValueError."""
        import numpy as np

        from . import ops
        from .utils.pnp_utils import select_and_flip
        scenes = list(scenes)
        if not scenes:
            return []
        geo = [self._is_geometry(sc) for sc in scenes]
        if any(geo) and not all(geo):
            raise ValueError("run_frames_batched: the list mixes geometry-mode scenes (no 'masks') and given-geometry scenes "
                             f"(geometry-mode: {[f for f, g in enumerate(geo) if g]})")
        if all(geo) or not _one_rank(self.group):
            return list(self.run_frames(scenes, replay=replay))
        sizes = {tuple(sc["frame"].shape) for sc in scenes}
        if len(sizes) > 1:
            raise ValueError(f"run_frames_batched: the frames of one call have one size, got {sorted(sizes)}")
        counts = [int(np.asarray(sc["bboxes"]).reshape(-1, 4).shape[0]) for sc in scenes]
        seeds = frame_batch_seeds([sc.get("vehicle_seeds") for sc in scenes], counts)
        if self.inpaint:
            live = [f for f, c in enumerate(counts) if c > 0]
            _batch_inpaint("run_frames_batched", live, [scenes[f].get("inpaint") for f in live], "that has vehicles", "scenes", required=True)
        max_batch, pad = _pad_defaults(replay, max_batch, pad)
        out = []
        for lo, hi in frame_batch_groups(counts, max_batch):
            rows = frame_batch_pad(sum(counts[lo:hi]), max_batch) if pad else None
            res, raw = self._guarded_pass(self._run_frame_batch, (scenes[lo:hi], replay, rows), check, seeds)
            if raw is not None:                                   # the group's one read-back: rvec | tvec | err of every row and start
                raw = ops.d2h(raw)
                rv, tv, er = raw[:, :12].reshape(-1, 4, 3), raw[:, 12:24].reshape(-1, 4, 3), raw[:, 24:28]
            row = 0
            for o in res:                                         # the reference's host epilogue of the pose fit, per row
                n = int(o["kp_idx"].shape[0])
                o["pose"] = [select_and_flip(rv[i], tv[i], er[i]) for i in range(row, row + n)]
                row += n
            out.extend(res)
        return out

    def run_frames_batched_geometry(self, scenes, replay: bool = False, check: Optional[str] = "sync", max_batch: Optional[int] = None,
                                    pad: Optional[bool] = None, batch_geometry: bool = True) -> list:
        """`run_frames_batched` for GEOMETRY-MODE first frames (a pipeline with cad_bank, scenes without 'masks': 'frame',
        'bboxes', 'focals', 'centers' (+ 'cad_idx' [V_f] without a CAD classifier, optional 'background', 'inpaint',
        'vehicle_seeds')): the first frames of several scenes as ONE pass per group, render included, with one device-to-host copy
        per group where `run_frames` takes one blocking copy per frame between its render and its plane warp.  Rows are
        scene-major (`frame_batch_offsets`); grouping and padding are `run_frames_batched`'s (`frame_batch_groups`,
        `frame_batch_pad`, max_batch, pad), and each group is one range-guarded call: a raised status word redoes the group in
        exact fp32 under the RNG state it was issued with.  Order of work per group, on the current stream:
          1. the keypoint stage, eager, at the group's real N rows: `frame_ops.crop_resize_frames` (box crop, hourglass input),
             hourglass (+ CAD classifier), `argmax_hw`, `keypoints_to_frame`, the pose fit with per-row focals and centers and the
             bank's keypoints (an index outside the bank is clamped for the fit only).  It stays eager as in `_geometry_frame`: the
             plan cache holds FRAME_PLANS plans, and a second plan per padded row count would evict the first;
          2. `render.first_geometry_batch_device`: pose selection and geometry (one launch per camera), render, plane visibility,
             the gate, the plane cut-outs of every row from its own frame (fusg_fill_poly_planes_frames_u8);
          3. `plane_homographies_device` on the device corner points and gated visibilities -> `warp_planes_fitted` ->
             `mask_bbox_geom` -> `icn_inputs_device` -> `frame_ops.vunet_inputs_frames` (-> `_inpaint_inputs_rows`);
          4. `_run` with the keypoints (and CAD logits) given, at N rows or the padded rows; replay=True: one recorded plan under
             ("frame_batch", rows, precision, "kp_given"[, "inpaint"][, "cad"]);
          5. `lab2bgr`, one ragged paste per composite with the gated box rows, then ONE `ops.d2h` of the stage's small buffer.
        A vehicle whose render is empty stays in the batch as an INERT row: its visibilities are zero (no plane is warped for it),
        its mask is empty (its crop is a zero row, nothing is pasted), its box row is zeroed (not inpainted into the frame), and
        its network outputs are dropped from the result - it is listed in 'skipped'.
        Returns, per scene, `run_frame`'s geometry-mode dict (`_geometry_frame`): 'kp_idx', 'kp_xy', 'pose' (+ 'cad_idx') of every
        vehicle; 'icn_u8', 'vunet_u8', 'geom' (+ 'inpaint_u8') of the kept ones; 'frame_icn', 'frame_vunet'; 'geometry' (all ten
        keys, every vehicle); 'skipped'; 'state' with state['geometry'] as `run_frame` builds it, which `run_later_frame` and
        `run_later_frames_batched_geometry` take unchanged.  A scene without vehicles gets `run_frames_batched`'s no-vehicle
        shape plus 'geometry' (zero rows) and 'skipped' == [].  A 'cad_idx' outside the bank raises IndexError after the read-back.
        The batch's crops are not bit for bit those of per-frame passes where the batch sizes differ (see `run_frames_batched`);
        the stage - render, cut-outs, corner points, poses - is the per-frame device path's, byte for byte.
        Fallbacks, with the results of today: batch_geometry=False is `run_frames_batched` (whose geometry-mode branch is
        `run_frames`); a list without geometry-mode scenes ignores the flag; a process group of more than one rank goes through
        `run_frames`.  ValueError before anything is launched: a pipeline without device_pose=True and device_homography=True, a
        list that mixes geometry-mode and given-geometry scenes, frames of different sizes, 'vehicle_seeds' or 'inpaint' present
        for some scenes with vehicles and absent for others, no 'cad_idx' and no classifier.
        Memory: 34 * H * W bytes per row (sketch 3, mask 1, planes 15, warped planes 15): 31 MB at 720 x 1280, 2.0 GB for 64 rows.
        Without 'vehicle_seeds' the inert rows and the padding rows draw noise too, so the unseeded noise stream is not that of
        per-frame passes over the kept vehicles."""
        scenes = list(scenes)
        if not scenes:
            return []
        geo = [self._is_geometry(sc) for sc in scenes]
        if any(geo) and not all(geo):
            raise ValueError("run_frames_batched_geometry: the list mixes geometry-mode scenes (no 'masks') and given-geometry scenes "
                             f"(geometry-mode: {[f for f, g in enumerate(geo) if g]})")
        if not batch_geometry or not any(geo):
            return self.run_frames_batched(scenes, replay=replay, check=check, max_batch=max_batch, pad=pad)
        if not _one_rank(self.group):
            return list(self.run_frames(scenes, replay=replay))
        counts, seeds, _ = frame_geometry_batch_rows(scenes, self.device_pose, self.device_homography, self.inpaint, self.cad is not None)
        max_batch, pad = _pad_defaults(replay, max_batch, pad)
        out = []
        for lo, hi in frame_batch_groups(counts, max_batch):
            rows = frame_batch_pad(sum(counts[lo:hi]), max_batch) if pad else None
            out.extend(self._guarded_pass(self._run_frame_batch_geometry, (scenes[lo:hi], replay, rows), check, seeds))
        return out

    @torch.no_grad()
    def _run_frame_batch_geometry(self, scenes, replay=False, rows=None) -> list:
        """One group of `run_frames_batched_geometry`: everything through the paste is queued, then the stage's small buffer is
        read back ONCE and the per-scene results of `_geometry_frame` are cut from the stacked ones.  rows: the row count the
        networks run at (>= N, the padding rows zero); None: N."""
        import numpy as np

        from . import frame_ops as fo
        from . import ops
        from . import render as rd
        from .utils.pnp_utils import cpc_fit_device
        from .warp_learn import planes_utils as pu
        dev, bank, R = self.device, self.cad_bank, 256
        boxes, counts, offs, live = self._frame_batch_rows(scenes)
        N = offs[-1]
        frames = [sc["frame"] for sc in scenes]
        Ks = [rd.intrinsic(sc["focals"], sc["centers"]) for sc in scenes]
        inpaint = bool(N) and self.inpaint and live[0].get("inpaint") is not None
        out = comp = kp_idx = kp_xy = cad_logits = cad_d = central = geom = None
        with torch.cuda.device(dev):
            if N == 0:                                            # no vehicle in the group: nothing is launched, nothing read back
                cad_d = torch.zeros(0, dtype=torch.int64, device=dev)
                geo = rd.first_geometry_batch_device(bank, frames, offs, cad_d, Ks, None, None)
                host = geo["host"](np.zeros(0, np.uint8))
            else:
                B = N if rows is None else max(int(rows), N)
                seeds = frame_batch_seeds([sc.get("vehicle_seeds") for sc in scenes], counts)
                pkey = ("frame_batch", B, ops.PRECISION, "kp_given") + (("inpaint",) if inpaint else ()) + \
                    (("cad",) if self.cad is not None else ())
                replay, tgt, buf = self._pass_buffers(pkey, replay, B, N)

                def padded(t):
                    """A per-row tensor of the keypoint stage at B rows, the padding rows zero."""
                    if B == N:
                        return t
                    z = torch.zeros((B,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
                    z[:N].copy_(t)
                    return z

                ec, ec_join = self._inpaint_inputs_rows(scenes, offs, B, tgt) if inpaint else (None, None)
                # ---- 1. the keypoint stage, eager, at the N real rows
                geom_box, hg_x, hg_rows, central = self._frame_batch_crops(frames, offs, boxes, buf)
                kp_idx = ops.argmax_hw(self.hg(hg_rows)["heatmaps"][-1])                       # :75-79
                if self.cad is not None:
                    cad_logits = self.cad(hg_rows)                                             # :66-69
                    cad_d = cad_logits.argmax(1)
                else:
                    cad_d = ops.h2d(np.concatenate([np.asarray(sc["cad_idx"], np.int64).reshape(-1) for sc in live]), dev)
                kp_xy = fo.keypoints_to_frame(kp_idx, geom_box, (R // 4, R // 4))              # :95-97
                # (an index outside the bank is clamped for the fit only: fusg_pose_geometry flags it and the read-back raises)
                kp3d_d = bank.device_arrays(dev)["kp3d"].index_select(0, cad_d.clamp(0, len(bank) - 1))
                raw_d = cpc_fit_device(self._per_row(scenes, counts, "focals"), self._per_row(scenes, counts, "centers"), kp_xy,
                                       kp3d_d)                                                 # :104-105
                # ---- 2. pose, render, visibility, gate, plane cut-outs: nothing read back
                box_rows = self._box_rows([sc["inpaint"]["boxes"] for sc in live]) if inpaint else None
                geo = rd.first_geometry_batch_device(bank, frames, offs, cad_d, Ks, raw_d, kp_xy, box_rows=box_rows)
                # ---- 3. the glue, every step once for all rows
                minv, index = pu.plane_homographies_device(geo["tex_pts_d"], geo["tex_pts_d"], geo["vis_d"], geo["vis_d"],
                                                           nverts=geo["tex_nv_d"])
                warped = pu.warp_planes_fitted(geo["planes"], minv, index)                     # :171-175
                masks, sketch = geo["mask"], geo["sketch"]
                _, geom = fo.mask_bbox_geom(masks)
                icn_x, icn_rows = buf("icn_x", 3 * (int(warped.shape[1]) + 2))
                pu.icn_inputs_device(warped, sketch, central, geom, R, R, out=icn_rows)        # :179-180
                (vu_x, vx_rows), (vu_y, vy_rows) = buf("vu_x", 6), buf("vu_y", 3)
                fo.vunet_inputs_frames(frames, offs, masks, sketch, sketch, geom, R, out=(vx_rows, vy_rows))   # :203-228
                nets_in = {"hg_x": hg_x, "icn_x": icn_x, "vu_x": vu_x, "vu_y": vu_y, "kp_idx": padded(kp_idx)}
                if cad_logits is not None:
                    nets_in["cad_logits"] = padded(cad_logits)
                if ec is not None:
                    ec_join()
                    nets_in.update({"ec_" + k: ec[k] for k in ops.INPAINT_KEYS})
                # ---- 4. the networks, the keypoints given (their pass-through outputs are the keypoint stage's own)
                out = self._nets_pass(self._run, pkey, replay, nets_in, seeds, N,              # :182, :230-234
                                      clone=("vunet_u8", "inpaint_u8", "mu_app_0", "mu_app_1"))
                # ---- 5. one ragged paste per composite
                bases = [self._paste_base(sc) for sc in scenes]
                comp = self._composites(lambda crops, **box: pu.paste_back_ragged_device(bases, offs, crops, geom, masks, **box), out,
                                        box_rows)
                host = geo["host"](ops.d2h(geo["buf"]))           # the one read-back of the group, behind the queued paste
            # ---- the per-scene results of `_geometry_frame`, cut from the stacked ones
            keys = ("icn_u8", "vunet_u8") + (("inpaint_u8",) if inpaint else ())
            g_t = {"masks": geo["mask"], "src_sketch": geo["sketch"], "dst_sketch": geo["sketch"], "src_planes": geo["planes"]}
            res = []
            for f, (sc, c) in enumerate(zip(scenes, counts)):
                sl = slice(offs[f], offs[f + 1])
                cad_idx = host["cad_idx"][sl]
                geometry = {**{k: t[sl] for k, t in g_t.items()}, **{k: host[k][sl] for k in ("src_kp", "dst_kp", "src_vis", "dst_vis")},
                            "kp3d": bank.kp3d[cad_idx], "cad_idx": cad_idx}
                keep = [v for v in range(c) if host["covered"][sl][v] > 0]
                if c == 0:
                    o = self._frame_batch_empty(sc)
                else:
                    idx = torch.as_tensor(keep, dtype=torch.long, device=dev)
                    cut = (lambda t: t[sl]) if len(keep) == c else (lambda t: t[sl].index_select(0, idx))   # the inert rows are dropped
                    o = {k: cut(out[k]) for k in keys}
                    o["geom"], o["kp_idx"], o["kp_xy"] = cut(geom), kp_idx[sl], kp_xy[sl]
                    o["state"] = {"appearance": [cut(out["mu_app_0"]), cut(out["mu_app_1"])], "central": cut(central),
                                  "shard": (0, len(keep), len(keep)), "sharded": False}
                if comp is not None:
                    o["frame_icn"], o["frame_vunet"] = comp["frame_icn"][f], comp["frame_vunet"][f]
                pose = self._pose_tuples(host["pose"][sl])
                dev_keys = {"pose_d": geo["pose_d"][sl], "cad_idx_d": cad_d[sl], "src_kp_d": geo["tex_pts_d"][sl], "kp_nv_d": geo["tex_nv_d"]}
                front = {"V": c, "pre": {"kp_idx": o["kp_idx"], "kp_xy": o["kp_xy"]}, "keep": keep, "pose": pose, "cad_idx": cad_idx,
                         "geometry": geometry, "scene": sc, "dev": dev_keys}
                res.append(self._geometry_assemble(front, o))
        return res

    # ---- the front of a group of first frames, shared by the given-geometry and the geometry-mode group
    @staticmethod
    def _frame_batch_rows(scenes):
        """The scene-major row layout of a group: (the scenes' boxes [V_f, 4], their vehicle counts, `frame_batch_offsets`, the
        scenes that have vehicles)."""
        import numpy as np
        boxes = [np.asarray(sc["bboxes"]).reshape(-1, 4) for sc in scenes]
        counts = [int(b.shape[0]) for b in boxes]
        return boxes, counts, frame_batch_offsets(counts), [sc for sc, c in zip(scenes, counts) if c]

    def _frame_batch_crops(self, frames, offs, boxes, buf):
        """The box crops of every row from its own frame: (the box geometry rows - one upload -, the hourglass input at the
        padded rows and the view of its real rows (`_pass_buffers`' buf), the central crops)."""
        from . import frame_ops as fo
        from . import ops
        from .warp_learn import planes_utils as pu
        R, (H, W, _) = 256, frames[0].shape
        geom_box = ops.h2d([pu._geom_row(*pu.square_crop_geometry((H, W), bb)) for b in boxes for bb in b], self.device, torch.int32)
        img_bbox = fo.crop_resize_frames(frames, offs, geom_box, (R, R), 0)                    # :58-60
        hg_x, hg_rows = buf("hg_x", 3)
        fo.crop_resize_frames(frames, offs, geom_box, (R, R), 1, fo.IMAGENET_MEAN, fo.IMAGENET_STD, out=hg_rows)   # :61-65
        return geom_box, hg_x, hg_rows, fo.central_crop(img_bbox)                              # vehicle_utils.py:49-52

    def _per_row(self, scenes, counts, k) -> torch.Tensor:
        """The scenes' 'focals' or 'centers' per row, float32 [N, 2] on the device (one upload): the pose fit's."""
        import numpy as np

        from . import ops
        return ops.h2d(np.concatenate([np.broadcast_to(np.asarray(sc[k], np.float32).reshape(-1, 2), (c, 2))
                                       for sc, c in zip(scenes, counts) if c]), self.device)

    def _frame_batch_empty(self, scene) -> Dict:
        """A scene without vehicles in `run_frames_batched`: `run_frame`'s no-vehicle shape (its composites are its base), and a
        zero-vehicle 'state' the later-frame drivers take."""
        inp = scene.get("inpaint") if self.inpaint else None     # (not asked for: only a scene that has vehicles needs the key)
        o = self._no_vehicles(256, "kp_idx", "icn_u8", "vunet_u8", "geom", *(("inpaint_u8",) if inp is not None else ()),
                              *(("cad_idx",) if self.cad is not None else ()), "mu_app_0", "mu_app_1", "central")
        o = self._frame_finish(scene, o)
        o.pop("_pose_raw")
        o["state"] = {"appearance": [o["mu_app_0"], o["mu_app_1"]], "central": o["central"], "shard": (0, 0, 0), "sharded": False}
        return o

    @torch.no_grad()
    def _run_frame_batch(self, scenes, replay=False, rows=None):
        """One group of `run_frames_batched`: (the scenes' `run_frame` dicts without 'pose', the raw pose fits of all rows packed
        as float32 [N, 28] = rvec [4, 3] | tvec [4, 3] | err [4] on the device - None when no scene has a vehicle).  rows: the
        row count the networks run at (>= N, the padding rows zero); None: N."""
        import numpy as np

        from . import frame_ops as fo
        from . import ops
        from .utils.pnp_utils import cpc_fit_device
        from .warp_learn import planes_utils as pu
        dev, R = self.device, 256
        boxes, counts, offs, live = self._frame_batch_rows(scenes)
        N = offs[-1]
        if N == 0:
            return [self._frame_batch_empty(sc) for sc in scenes], None
        B = N if rows is None else max(int(rows), N)
        frames = [sc["frame"] for sc in scenes]
        cat = lambda k: self._cat_rows(live, k)                                                    # noqa: E731
        lst = lambda k: [veh for sc in live for veh in sc[k]]                                      # noqa: E731
        vis = lambda k: np.concatenate([np.asarray(sc[k]).reshape(-1, 5) for sc in live])         # noqa: E731
        with torch.cuda.device(dev):
            inpaint = self.inpaint and live[0].get("inpaint") is not None
            seeds = frame_batch_seeds([sc.get("vehicle_seeds") for sc in scenes], counts)
            pkey = ("frame_batch", B, ops.PRECISION) + (("inpaint",) if inpaint else ()) + (("cad",) if self.cad is not None else ())
            replay, tgt, buf = self._pass_buffers(pkey, replay, B, N)
            merged = {"src_planes": cat("src_planes"), "src_kp": lst("src_kp"), "dst_kp": lst("dst_kp"),
                      "src_vis": vis("src_vis"), "dst_vis": vis("dst_vis")}
            masks, src_sketch, dst_sketch = cat("masks"), cat("src_sketch"), cat("dst_sketch")
            # ---- host: the homography fits of every plane of every row, before any launch
            jobs = None if self.device_homography else \
                pu.warp_jobs_frame(merged["src_kp"], merged["dst_kp"], merged["src_vis"], merged["dst_vis"])
            ec, ec_join = self._inpaint_inputs_rows(scenes, offs, B, tgt) if inpaint else (None, None)
            # ---- uint8 glue on the caller's stream, every step once for all rows
            geom_box, hg_x, _, central = self._frame_batch_crops(frames, offs, boxes, buf)
            warped = self._warp_planes(merged, jobs)                                           # :171-175
            _, geom = fo.mask_bbox_geom(masks)
            icn_x, icn_rows = buf("icn_x", 3 * (int(warped.shape[1]) + 2))
            pu.icn_inputs_device(warped, dst_sketch, central, geom, R, R, out=icn_rows)        # :179-180
            (vu_x, vx_rows), (vu_y, vy_rows) = buf("vu_x", 6), buf("vu_y", 3)
            fo.vunet_inputs_frames(frames, offs, masks, src_sketch, dst_sketch, geom, R, out=(vx_rows, vy_rows))   # :203-228
            nets_in = {"hg_x": hg_x, "icn_x": icn_x, "vu_x": vu_x, "vu_y": vu_y}
            if ec is not None:
                ec_join()
                nets_in.update({"ec_" + k: ec[k] for k in ops.INPAINT_KEYS})
            out = self._nets_pass(self._run, pkey, replay, nets_in, seeds, N,                  # :75-79, :182, :230-234
                                  clone=("vunet_u8", "kp_idx", "inpaint_u8", "cad_logits", "mu_app_0", "mu_app_1"))
            if "cad_logits" in out:
                out["cad_idx"] = out.pop("cad_logits").argmax(1)                               # :69
            # ---- keypoints -> frame pixels -> pose fit, with per-row focals and centers
            out["kp_idx"] = out["kp_idx"].contiguous()
            kp_xy = fo.keypoints_to_frame(out["kp_idx"], geom_box, (R // 4, R // 4))           # :95-97 (64 x 64 heat-maps)
            banked = [self.cad is not None and sc.get("kp3d_bank") is not None for sc in live]
            if all(banked):                                       # :82-88: the chosen CAD model's keypoints, one gather
                banks, which = [], []
                for sc, c in zip(live, [c for c in counts if c]):
                    hit = [i for i, b in enumerate(banks) if b is sc["kp3d_bank"]]
                    if not hit:
                        banks.append(sc["kp3d_bank"])
                    which += [hit[0] if hit else len(banks) - 1] * c
                bank = ops.h2d(np.stack([np.asarray(b, np.float32) for b in banks]), dev)
                kp3d = bank[ops.h2d(np.asarray(which, np.int64), dev), out["cad_idx"]]
            elif not any(banked):
                kp3d = ops.h2d(np.concatenate([np.asarray(sc["kp3d"], np.float32).reshape(-1, 12, 3) for sc in live]), dev)
            else:
                kp3d = torch.cat([ops.h2d(np.asarray(sc["kp3d_bank"], np.float32), dev)[out["cad_idx"][offs[f]:offs[f + 1]]] if
                                  (self.cad is not None and sc.get("kp3d_bank") is not None) else
                                  ops.h2d(np.asarray(sc["kp3d"], np.float32).reshape(-1, 12, 3), dev)
                                  for f, sc in enumerate(scenes) if counts[f]])
            rv, tv, er = cpc_fit_device(self._per_row(scenes, counts, "focals"), self._per_row(scenes, counts, "centers"), kp_xy,
                                        kp3d)                                                  # :104-105
            raw = torch.cat([rv.reshape(N, 12), tv.reshape(N, 12), er.reshape(N, 4)], 1)
            # ---- one ragged paste per composite
            bases = [self._paste_base(sc) for sc in scenes]
            comp = self._composites(lambda crops, **box: pu.paste_back_ragged_device(bases, offs, crops, geom, masks, **box), out,
                                    self._box_rows([sc["inpaint"]["boxes"] for sc in live]) if inpaint else None)
        keys = ("kp_idx", "icn_u8", "vunet_u8") + (("inpaint_u8",) if inpaint else ()) + (("cad_idx",) if "cad_idx" in out else ())
        res = []
        for f, c in enumerate(counts):
            sl = slice(offs[f], offs[f + 1])
            if c == 0:
                o = self._frame_batch_empty(scenes[f])
            else:
                o = {k: out[k][sl] for k in keys}
                o["geom"], o["kp_xy"] = geom[sl], kp_xy[sl]
                o["state"] = {"appearance": [out["mu_app_0"][sl], out["mu_app_1"][sl]], "central": central[sl], "shard": (0, c, c),
                              "sharded": False}
            o["frame_icn"], o["frame_vunet"] = comp["frame_icn"][f], comp["frame_vunet"][f]
            res.append(o)
        return res, raw

    # ------------------------------------------------------------------------------------------ future frames of several clips
    def run_later_clips_batched(self, clips, replay: bool = False, check: Optional[str] = "sync", max_batch: Optional[int] = None,
                                pad: Optional[bool] = None) -> list:
        """`run_later_frames_batched` for the future frames of SEVERAL clips at once, with ragged F_c frames of V_c vehicles: every
        selected frame of a video is a clip of 1 + 5 frames that usually carries one or two vehicles, so clip by clip each tail is
        a pass of ~300 dependent launches at 5-10 rows.  The tails are independent of each other and `_later_nets` does not know
        which clip or frame a row came from, so everything between the uint8 frames and the composited frames is issued once for
        all sum(F_c * V_c) rows: the homography fits (host jobs, or `plane_homographies_device` over the concatenated corner
        points), ONE plane warp whose source stack is a property of the destination row (fusg_warp_perspective_clips_u8: each
        clip's planes stay where its first frame left them, passed by pointer - no torch.cat of source planes),
        `mask_bbox_geom`, `icn_inputs_device` with each clip's central crops repeated per frame, `vunet_inputs`, the appearance
        codes repeated per frame and concatenated, `_later_nets` once, `lab2bgr`, and one `paste_back_ragged_device` per
        composite over all (clip, frame) frames, each from its own base.  Rows are clip-major, frame-major inside a clip: row
        (c, f, v) = offsets[c] + f * V_c + v (`clip_batch_offsets`).

        clips: a sequence of (later_scenes, state) pairs, each as `run_later_frames_batched` takes one: the F_c later scenes of
        the clip (all sharing the first frame's 'src_planes' tensor; each its own 'frame', 'masks', 'dst_*', optional
        'background', 'vehicle_seeds', 'inpaint') and the state of its first frame (`run_frame`'s or `run_frames_batched`'s).
        F_c = 0 and V_c = 0 are allowed.  All frames of a call have one size.  Either every scene that has vehicles carries
        'vehicle_seeds' or none does, and with a pipeline built with inpaint=True the same holds for 'inpaint' (any of the three
        forms, per scene): each scene's EdgeConnect inputs are built from its own image into its row slice on the inpaint
        stream, and the box rows go to the paste.  All of this is a ValueError before anything is launched, as are a scene whose
        vehicle count differs from its state's, a clip whose scenes do not share one 'src_planes' tensor and a list that mixes
        geometry-mode and given-geometry clips.
        max_batch bounds the rows of a pass (default LATER_MAX_BATCH = 64), FRAME_BATCH_MAX_FRAMES its frames and clips:
        consecutive WHOLE clips are packed greedily (`clip_batch_groups`); a clip that alone exceeds a bound goes through
        `run_later_frames_batched` (which splits it by frames), with that method's results.
        pad (None: pad when replay is on): the networks run at `frame_batch_pad(rows, max_batch)` rows - the next of 4, 8, 16,
        32, 64 -, the padding rows of every input zero and their seeds 0; the outputs are cut to the real rows before `lab2bgr`
        and the paste.  replay=True: the networks are ONE recorded plan per ("later_rows", padded_rows, precision[, "inpaint"]) -
        at most five keys per video whatever its mix of F and V, apart from the ("later_batch", F, V, ...) plans of the one-clip
        driver; outputs are handed out as copies.
        check: the range guard of `run` - one status word per group; raised, the group is redone in exact fp32 under the RNG
        state it was issued with.
        A batch's crops are not bit for bit those of clip-by-clip passes: another batch size may route the convolutions
        differently (the glue - warped planes, crop rows, network inputs, paste - is byte-equal).
        Memory: the warped planes take 15 * H * W bytes per row (13.8 MB at 720 x 1280, 885 MB for 64 rows); the source planes
        are not copied.
        Returns one list per clip of `run_later_frame`'s dicts ('icn_u8', 'vunet_u8', 'geom', 'frame_icn', 'frame_vunet'
        (+ 'inpaint_u8')), the keys and shapes `run_later_frames_batched` returns; tensors are views into the pass's stacked
        results.  F_c = 0 -> []; V_c = 0 -> the no-vehicle shape, the composites equal to their base; [] -> [].
        Geometry-mode states (scenes without 'masks') and sharded states (process group) go clip by clip through
        `run_later_frames_batched` - the results of today; `run_later_clips_batched_geometry` is the opt-in that batches
        geometry-mode clips (this method's parameter list is pinned, so the flag lives on a sibling)."""
        what = "run_later_clips_batched"
        clips = [(list(scs), st) for scs, st in clips]
        if not clips:
            return []
        geo = [any(self._is_geometry(sc, st) for sc in scs) for scs, st in clips]
        given = [bool(scs) and not g for (scs, _), g in zip(clips, geo)]
        if any(geo) and any(given):
            raise ValueError(f"{what}: the list mixes geometry-mode clips (scenes without 'masks') and given-geometry clips "
                             f"(geometry-mode: {[c for c, g in enumerate(geo) if g]})")
        if any(geo) or (not _one_rank(self.group) and any(st.get("sharded") for _, st in clips)):
            return [self._later_frames_batched(scs, st, replay, check, max_batch, False) for scs, st in clips]
        sizes = {tuple(sc["frame"].shape) for scs, _ in clips for sc in scs}
        if len(sizes) > 1:
            raise ValueError(f"{what}: the frames of one call have one size, got {sorted(sizes)}")
        frames = [len(scs) for scs, _ in clips]
        vehicles = [int(st["central"].shape[0]) for _, st in clips]
        for c, ((scs, _), V) in enumerate(zip(clips, vehicles)):
            for f, sc in enumerate(scs):
                if int(sc["masks"].shape[0]) != V:
                    raise ValueError(f"{what}: the state of clip {c} holds {V} vehicles, its scene {f} {int(sc['masks'].shape[0])}")
            if V and any(sc["src_planes"].data_ptr() != scs[0]["src_planes"].data_ptr() or sc["src_planes"].shape != scs[0]["src_planes"].shape
                         for sc in scs):
                raise ValueError(f"{what}: the scenes of clip {c} share the first frame's 'src_planes' (one tensor)")
        seeds = clip_batch_seeds([[sc.get("vehicle_seeds") for sc in scs] for scs, _ in clips], vehicles)
        live = [(c, f) for c, (scs, _) in enumerate(clips) if vehicles[c] for f in range(len(scs))]
        _batch_inpaint(what, live, [self._later_inpaint(clips[c][0][f]) for c, f in live], "that has vehicles", "(clip, frame)")
        max_batch, pad = _pad_defaults(replay, max_batch, pad)
        out = []
        for lo, hi, oversized in clip_batch_groups(frames, vehicles, max_batch):
            if oversized:                                         # more rows or frames than a pass takes: the one-clip path splits by frames
                out.append(self._later_frames_batched(clips[lo][0], clips[lo][1], replay, check, max_batch, False))
                continue
            rows = frame_batch_pad(sum(f * v for f, v in zip(frames[lo:hi], vehicles[lo:hi])), max_batch) if pad else None
            out.extend(self._guarded_pass(self._run_later_clips, (clips[lo:hi], replay, rows), check, seeds))
        return out

    @torch.no_grad()
    def _later_clips_stages(self, clips, icn_out=None, vu_out=None, geo=None) -> Dict:
        """The data movement of a several-clip later pass in front of the networks, clip-major over the (scenes, state) pairs and
        frame-major inside a clip: 'warped' uint8 [N, P, H, W, 3], 'masks' uint8 [N, H, W], 'geom' int32 [N, 8], 'icn_x' [N, 21,
        R, R], 'vu_y' [N, 3, R, R] for the N = sum(F_c * V_c) rows (icn_out / vu_out: the N real rows of a padded or recorded
        pass's buffers, written in place).  Nothing here depends on the batch size: every row holds the bytes `_later_local`
        builds for its frame; a clip without frames or without vehicles contributes no row.  At least one row.  geo (geometry
        mode, `_later_clips_geometry_stage`): the masks, sketches, corner points and gated visibilities come from the device
        stage, the planes from the states."""
        from . import frame_ops as fo
        from .warp_learn import planes_utils as pu
        live = [(list(scs), st) for scs, st in clips if len(scs) and int(st["central"].shape[0])]
        scenes = [sc for scs, _ in live for sc in scs]
        with torch.cuda.device(self.device):
            counts = [len(scs) for scs, _ in live]
            if geo is not None:
                planes = [st["geometry"]["src_planes"].contiguous() for _, st in live]    # by pointer, as below
                minv, index = pu.plane_homographies_device(geo["src_kp_d"], geo["tex_pts_d"], geo["src_vis_d"], geo["dst_vis_d"],
                                                           nverts=geo["kp_nv_d"])
                warped = pu.warp_planes_clips_fitted(planes, counts, minv, index)              # :376-381
                masks, sketch = geo["mask"], geo["sketch"]
            else:
                planes = [scs[0]["src_planes"].contiguous() for scs, _ in live]   # by pointer: each clip's planes stay where they are
                fit = self._later_fits(scenes)
                warped = pu.warp_planes_clips_fitted(planes, counts, *fit) if self.device_homography else \
                    pu.warp_planes_clips_batch(planes, counts, fit)                            # :376-381
                masks, sketch = self._cat_rows(scenes, "masks"), self._cat_rows(scenes, "dst_sketch")
            # ---- behind the warp, once for all rows: crop rows, the ICN's inputs with each clip's central crops repeated per frame
            # in row order, the VUnet's y_tilde
            R = 256
            _, geom = fo.mask_bbox_geom(masks)
            central = [st["central"].repeat(len(scs), 1, 1, 1) for scs, st in live]
            icn_x = pu.icn_inputs_device(warped, sketch, central[0] if len(central) == 1 else torch.cat(central), geom, R, R,
                                         out=icn_out)                                          # :385-387
            _, vu_y = fo.vunet_inputs(scenes[0]["frame"], masks, sketch, sketch, geom, R,      # :415-420 (y_tilde reads no frame)
                                      out=None if vu_out is None else (None, vu_out))
            return {"warped": warped, "masks": masks, "geom": geom, "icn_x": icn_x, "vu_y": vu_y}

    @torch.no_grad()
    def _run_later_clips(self, clips, replay=False, rows=None, geometry=False, plan_key=None) -> list:
        """One group of later frames - of `run_later_clips_batched`, or of the one-clip drivers, whose group is a list of one clip:
        one list of `run_later_frame` dicts per clip.  rows: the row count the networks run at (>= N, the padding rows zero);
        None: N.  geometry: a group of the geometry-mode drivers - the clips' scenes carry 'steps' instead of masks, sketches and
        corner points, which come from the device stage (`_later_clips_geometry_stage`), the results are
        `_geometry_later_frame`'s, cut after the stage's ONE read-back.  plan_key: what the recorded plan is kept under, in front
        of the precision and the inpaint marker; None: ("later_rows", B)."""
        from . import ops
        dev, R = self.device, 256
        frames = [len(scs) for scs, _ in clips]
        vehicles = [int(st["central"].shape[0]) for _, st in clips]
        offs = clip_batch_offsets(frames, vehicles)
        N = offs[-1]
        # (a geometry-mode scene of a clip without vehicles: the per-frame path, which launches nothing for it)
        empty = (lambda sc, st: self._geometry_later_frame(sc, st, None, False)) if geometry else self._run_later_frame
        if N == 0:
            return [[empty(sc, st) for sc in scs] for scs, st in clips]
        B = N if rows is None else max(int(rows), N)
        scenes = [sc for scs, _ in clips for sc in scs]                           # the (clip, frame) frames, in order
        frame_rows = clip_batch_frame_rows(frames, vehicles)
        live = [(scs, st) for (scs, st), F, V in zip(clips, frames, vehicles) if F and V]
        inpaint = self._later_inpaint(live[0][0][0]) is not None
        seeds = clip_batch_seeds([[sc.get("vehicle_seeds") for sc in scs] for scs, _ in clips], vehicles)
        with torch.cuda.device(dev):
            pkey = tuple(plan_key or ("later_rows", B)) + (ops.PRECISION,) + (("inpaint",) if inpaint else ())
            replay, tgt, buf = self._pass_buffers(pkey, replay, B, N)

            def per_row(i):
                """The clips' appearance code i repeated per frame, concatenated in row order, zero rows up to B."""
                parts = [st["appearance"][i].repeat(len(scs), 1, 1, 1) for scs, st in live]
                if B > N:
                    parts.append(parts[0].new_zeros((B - N,) + tuple(parts[0].shape[1:])))
                return parts[0] if len(parts) == 1 else torch.cat(parts)

            ec, ec_join = self._inpaint_inputs_rows(scenes, frame_rows, B, tgt) if inpaint else (None, None)
            # geometry mode: the box rows are uploaded in front of the stage, whose gate zeroes the rows of empty renders
            box_rows = self._box_rows([sc["inpaint"]["boxes"] for scs, _ in live for sc in scs]) if inpaint and geometry else None
            geo = self._later_clips_geometry_stage(live, box_rows) if geometry else None
            if B > N or tgt:
                (icn_x, icn_rows), (vu_y, vu_rows) = buf("icn_x", 21), buf("vu_y", 3)
                st = self._later_clips_stages(clips, icn_out=icn_rows, vu_out=vu_rows, geo=geo)
            else:
                st = self._later_clips_stages(clips, geo=geo)
                icn_x, vu_y = st["icn_x"], st["vu_y"]
            geom, masks = st["geom"], st["masks"]
            nets_in = {"icn_x": icn_x, "vu_y": vu_y, "app0": per_row(0), "app1": per_row(1)}
            if ec is not None:
                ec_join()
                nets_in.update({"ec_" + k: ec[k] for k in ops.INPAINT_KEYS})
            out = self._nets_pass(self._later_nets, pkey, replay, nets_in, seeds, N)
            # ---- one ragged paste per composite over all (clip, frame) frames
            bases = [self._paste_base(sc) for sc in scenes]
            if inpaint and not geometry:
                box_rows = self._box_rows([sc["inpaint"]["boxes"] for scs, _ in live for sc in scs])
            comp = self._composites(lambda crops, **box: self._paste_frames(bases, frame_rows, crops, geom, masks, **box), out,
                                    box_rows if inpaint else None)
            # geometry mode: the one read-back of the group, behind the queued paste
            host = geo["host"](ops.d2h(geo["buf"])) if geometry else None
        keys = ("icn_u8", "vunet_u8") + (("inpaint_u8",) if inpaint else ())
        res, k0 = [], 0
        for c, (scs, cst) in enumerate(clips):
            one = []
            for f, sc in enumerate(scs):
                if vehicles[c] == 0 and geometry:
                    o = empty(sc, cst)
                elif vehicles[c] == 0:
                    o = self._no_vehicles(R, "icn_u8", "vunet_u8", "geom", *(("inpaint_u8",) if self._later_inpaint(sc) is not None else ()))
                else:
                    sl = slice(frame_rows[k0 + f], frame_rows[k0 + f + 1])
                    o = {k: out[k][sl] for k in keys}
                    o["geom"] = geom[sl]
                o["frame_icn"], o["frame_vunet"] = comp["frame_icn"][k0 + f], comp["frame_vunet"][k0 + f]
                if vehicles[c] and geometry:
                    o = self._geometry_cut(o, sl, list(cst["geometry"]["vehicles"]), sc, geo, host, inpaint)
                one.append(o)
            k0 += len(scs)
            res.append(one)
        return res

    # ---- the same for geometry-mode clips: the render, the visibilities and the skip rule of ALL clips' rows stay on the device
    def run_later_clips_batched_geometry(self, clips, replay: bool = False, check: Optional[str] = "sync", max_batch: Optional[int] = None,
                                         pad: Optional[bool] = None, batch_geometry: bool = True) -> list:
        """`run_later_clips_batched` that also batches GEOMETRY-MODE clips (states of geometry-mode first frames, scenes with
        'steps' and no 'masks'; batch_geometry=False: exactly `run_later_clips_batched`, which takes such clips one by one).  Clip
        by clip a geometry-mode video pays one pass of ~300 dependent launches at 5-10 rows and one blocking read-back per clip;
        here a group of `clip_batch_groups` over (F_c, V_c = the state's kept vehicles) is queued whole before anything is read:
        `render.later_geometry_clips_device` (ONE upload of every clip's steps, camera and source visibilities ->
        fusg_pose_geometry_clips, each clip's pose table, CAD indices and source corner points passed by pointer ->
        fusg_render_normals_u8 -> fusg_plane_visibility -> fusg_later_gate, once each for all rows) ->
        `plane_homographies_device` over all rows -> the several-clip plane warp, each clip's state['geometry']['src_planes']
        passed by pointer -> crop rows and both networks' inputs -> `_later_nets` once at N or the padded rows -> Lab -> BGR -> one
        ragged paste per composite with the gated box rows; then ONE `ops.d2h` of the stage's small packed buffer, from which the
        per-(clip, frame) results are cut.  Rows are clip-major, frame-major inside a clip (`clip_batch_offsets`).
        A vehicle whose render is empty stays in the batch as an INERT row, exactly as in `run_later_frames_batched_geometry`;
        'vehicle_seeds' and 'inpaint' list every first-frame vehicle, like 'steps', and are selected to the state's vehicles;
        either every (clip, frame) whose clip has vehicles carries them or none does.  Needs a pipeline built with
        device_pose=True and device_homography=True; all frames of a call have one size; every clip may have its own camera
        (state['geometry'] 'focals' / 'centers').  All of this is a ValueError before anything is launched
        (`later_clips_geometry_batch_rows`).  A state made without device copies uploads its host pose, CAD indices and corner
        points once per call.
        max_batch, pad, replay, check: `run_later_clips_batched`'s; the plan of replay=True is the ("later_rows", padded_rows,
        precision[, "inpaint"]) plan a given-geometry group of that shape records - they share it.  A clip that alone exceeds a
        bound goes through `run_later_frames_batched_geometry` (which splits it by frames).  Sharded states (process group) keep
        going clip by clip; a given-geometry list ignores the flag.
        Memory per row at H x W: 19 * H * W bytes (sketch 3, mask 1, warped planes 15) - 17.5 MB at 720 x 1280, 1.1 GB for 64 rows.
        Returns one list per clip of `run_later_frames_batched_geometry`'s dicts ('icn_u8', 'vunet_u8', 'geom' (+ 'inpaint_u8') of
        the kept vehicles, 'frame_icn', 'frame_vunet', 'geometry', 'skipped'); F_c = 0 -> []; V_c = 0 -> the no-vehicle shape."""
        clips = [(list(scs), st) for scs, st in clips]
        geo = [any(self._is_geometry(sc, st) for sc in scs) for scs, st in clips]
        sharded = not _one_rank(self.group) and any(st.get("sharded") for _, st in clips)
        if not batch_geometry or not any(geo) or sharded:
            return self.run_later_clips_batched(clips, replay=replay, check=check, max_batch=max_batch, pad=pad)
        vehicles, seeds, inpaint = later_clips_geometry_batch_rows(clips, self.device_pose, self.device_homography, self.inpaint)
        frames = [len(scs) for scs, _ in clips]
        for c, ((_, st), V) in enumerate(zip(clips, vehicles)):
            if int(st["central"].shape[0]) != V:
                raise ValueError(f"run_later_clips_batched_geometry: the state of clip {c} holds {int(st['central'].shape[0])} crops "
                                 f"for {V} vehicles")
        rows = [(self._geometry_row_scenes(scs, list(st["geometry"]["vehicles"]), inpaint), st) for scs, st in clips]
        max_batch, pad = _pad_defaults(replay, max_batch, pad)
        out = []
        for lo, hi, oversized in clip_batch_groups(frames, vehicles, max_batch):
            if oversized:                                         # more rows or frames than a pass takes: the one-clip path splits by frames
                out.append(self._later_frames_batched(clips[lo][0], clips[lo][1], replay, check, max_batch, True))
                continue
            n = frame_batch_pad(sum(f * v for f, v in zip(frames[lo:hi], vehicles[lo:hi])), max_batch) if pad else None
            out.extend(self._guarded_pass(self._run_later_clips, (rows[lo:hi], replay, n, True), check, seeds))
        return out

    @torch.no_grad()
    def _later_clips_geometry_stage(self, live, box_rows=None) -> Dict:
        """The device geometry of a group of geometry-mode clip tails (`render.later_geometry_clips_device`): live = the (scenes,
        state) pairs that own rows, in order.  Nothing is read back."""
        from . import render as rd
        clips = []
        for scs, st in live:
            gs = st["geometry"]
            veh = list(gs["vehicles"])
            sd = self._geometry_state_device(gs)
            clips.append({"cad_idx_d": sd["cad_idx_d"].contiguous(), "pose_d": sd["pose_d"].to(torch.float32).reshape(len(veh), 7).contiguous(),
                          "src_kp_d": sd["src_kp_d"].contiguous(), "src_vis": gs["src_vis"], "cad_idx": gs["cad_idx"],
                          "K": rd.intrinsic(gs["focals"], gs["centers"]),
                          "steps_per_frame": [[sc["steps"][v] for v in veh] for sc in scs]})
        frame = live[0][0][0]["frame"]
        return rd.later_geometry_clips_device(self.cad_bank, (int(frame.shape[0]), int(frame.shape[1])), clips, box_rows=box_rows)

    def run_clips_batched_geometry(self, clips, replay: bool = False, check: Optional[str] = "sync", max_batch: Optional[int] = None,
                                   pad: Optional[bool] = None, batch_geometry: bool = True) -> list:
        """`run_clips_batched` for geometry-mode clips: clips is a sequence of (first_scene, later_scenes) pairs; the first frames
        go through `run_frames_batched_geometry`, all tails through `run_later_clips_batched_geometry` with the states it
        returned (batch_geometry: both methods' flag).  Returns, per clip, [first_result, later_results...]."""
        clips = [(first, list(later)) for first, later in clips]
        firsts = self.run_frames_batched_geometry([first for first, _ in clips], replay=replay, check=check, max_batch=max_batch, pad=pad,
                                                  batch_geometry=batch_geometry)
        tails = self.run_later_clips_batched_geometry([(later, f["state"]) for (_, later), f in zip(clips, firsts)], replay=replay,
                                                      check=check, max_batch=max_batch, pad=pad, batch_geometry=batch_geometry)
        return [[f] + t for f, t in zip(firsts, tails)]

    def run_clips_batched(self, clips, replay: bool = False, check: Optional[str] = "sync", max_batch: Optional[int] = None,
                          pad: Optional[bool] = None) -> list:
        """Whole clips of a video as batched passes: clips is a sequence of (first_scene, later_scenes) pairs; the first frames
        go through `run_frames_batched`, all tails through `run_later_clips_batched` with the states it returned.  Returns, per
        clip, [first_result, later_results...]."""
        clips = [(first, list(later)) for first, later in clips]
        firsts = self.run_frames_batched([first for first, _ in clips], replay=replay, check=check, max_batch=max_batch, pad=pad)
        tails = self.run_later_clips_batched([(later, f["state"]) for (_, later), f in zip(clips, firsts)], replay=replay, check=check,
                                             max_batch=max_batch, pad=pad)
        return [[f] + t for f, t in zip(firsts, tails)]

    def run_clip_frames(self, first_scene: Dict, later_scenes, replay: bool = False, batched: bool = False,
                        batch_geometry: bool = False):
        """A vehicle clip the reference's way (trajectory_inference.py:55-250 then :267-450): the first frame through
        `run_frame`, every future frame through `run_later_frame` with the first frame's state.  Generator of 1 + len(later_scenes)
        results.  Under a process group the whole clip is sharded by vehicle: a vehicle's six frames stay on one rank (frame by
        frame).  A geometry-mode clip (cad_bank, scenes without 'masks') goes through the same drivers.
        batched=True renders the future frames as batched passes (`run_later_frames_batched`) instead of one frame in flight:
        the same sequence of results, each frame's within that method's bars of the frame-by-frame form.  A geometry-mode clip
        then still runs frame by frame unless batch_geometry=True (`run_later_frames_batched_geometry`: a pipeline built with
        device_pose=True and device_homography=True)."""
        first = self.run_frame(first_scene, replay=replay)
        state = first["state"]
        yield first if len(first) > 1 else None
        if batched:
            yield from self._later_frames_batched(list(later_scenes), state, replay, "sync", None, bool(batch_geometry))
            return
        yield from self.run_later_frames(later_scenes, state, replay=replay)       # one later frame in flight

    def run_clip(self, clip: Dict[str, torch.Tensor], vehicle_seeds: Optional[Sequence[int]] = None,
                 check: Optional[str] = "sync") -> Dict[str, torch.Tensor]:
        rng = torch.get_rng_state() if (vehicle_seeds is None and check == "sync") else None
        return self._guarded(self._run_clip, (clip, vehicle_seeds), check, rng)

    @torch.no_grad()
    def _run_clip(self, clip, vehicle_seeds):
        """Clip mode = what traj_test does per vehicle over a 6-frame clip: 1x hourglass,
        F x ICN, 1x VUnet appearance half, F x VUnet shape half with the frame-0 appearance code reused
        (trajectory_inference.py:75-79, 182, 387-391, 230-233, 424-426) - but batched over vehicles AND
        frames instead of the reference's two nested serial loops.

        clip: 'hg_x' [V,3,R,R], 'icn_x' [V,F,21,R,R], 'vu_x' [V,6,R,R], 'vu_y' [V,F,3,R,R].
        Returns 'kp_idx' int32 [V,12], 'icn_u8' / 'vunet_u8' uint8 [V,F,R,R,3]."""
        from . import ops
        V, F = clip["icn_x"].shape[:2]
        R = clip["hg_x"].shape[-1]

        def hg():
            return {"kp_idx": ops.argmax_hw(self.hg(clip["hg_x"])["heatmaps"][-1])}

        def icn():
            y = self.icn(clip["icn_x"].reshape(V * F, 21, R, R))
            return {"icn_u8": ops.to_image_u8(y).view(V, F, R, R, 3)}

        def vunet():
            vu = self.vunet
            vu.set_vehicle_seeds(vehicle_seeds)                   # appearance half: one stream per vehicle
            eo, es = vu.forward_enc_up(clip["vu_x"])
            mu_app, _ = vu.forward_enc_down(eo, es)
            if vehicle_seeds is not None:                         # shape half: one stream per (vehicle, frame)
                vu.set_vehicle_seeds([int(sd) * 64 + f + 1 for sd in vehicle_seeds for f in range(F)])
            # every frame of a vehicle conditions on that vehicle's appearance code: frame-major repeat
            mu_rep = [m.repeat_interleave(F, dim=0) for m in mu_app]
            do, ds = vu.forward_dec_up(clip["vu_y"].reshape(V * F, 3, R, R))
            xt, _, _ = vu.forward_dec_down(do, ds, mu_rep)
            return {"vunet_u8": ops.to_image_u8(xt).view(V, F, R, R, 3)}

        return self._branches([("icn", icn), ("vunet", vunet), ("hg", hg)])


def _like_layout(t: torch.Tensor) -> torch.Tensor:
    """A zeroed tensor with exactly `t`'s sizes and strides (an NHWC-physical view keeps its padded channel pitch, so
    the glue kernels of `run_frame` can write a recorded pass's inputs in place and the stems read them unchanged)."""
    extent = 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride())) if t.numel() else 0
    base = torch.zeros(extent + 4, dtype=t.dtype, device=t.device)
    v = base.as_strided(t.shape, t.stride())
    v._fusg_zero_pad = True             # only ever written through views of the logical channels (ops.as_nhwc)
    return v


class CompiledPass:
    """A recorded crop pass of a VehiclePipeline (include/fusg.h, fusg_plan): fixed input shapes, persistent input /
    intermediate / output buffers (a private torch memory pool that lives as long as this object), per-pass host data
    (the VUnet's CPU-drawn sampler noise: same generator, order and shapes as the reference) refreshed before every
    replay.  The returned tensors are the plan's output buffers: the next `run` overwrites them."""

    def __init__(self, pipe: "VehiclePipeline", batch: Dict[str, torch.Tensor], vehicle_seeds=None, fn=None):
        from . import _lib as L
        from . import ops
        self.pipe, self.device = pipe, pipe.device
        self.fn = fn if fn is not None else pipe._run                          # the pass being recorded
        self.precision = ops.PRECISION                                        # recorded into every conv descriptor
        self.keys = sorted(batch.keys())
        with pipe._routed():
            # the routing batch every recorded launch carries (fusg.h: a replay routes as the recording did); the fp32 redo
            # of `run`, which is eager, is issued under it too
            self.route_batch = ops.ROUTE_BATCH
            self._record(batch, vehicle_seeds)

    def _record(self, batch, vehicle_seeds):
        from . import _lib as L
        from . import ops
        pipe = self.pipe
        with torch.cuda.device(self.device):
            pipe._guarded(self.fn, (batch, vehicle_seeds), None, None)        # warm-up: weight upload, workspaces, streams
            torch.cuda.synchronize(self.device)
            self.stream = torch.cuda.current_stream(self.device)
            self.pool = torch.cuda.MemPool()
            self.rec = ops.PlanRecorder()
            with torch.cuda.use_mem_pool(self.pool, device=self.device):
                self.inputs = {k: _like_layout(batch[k]).copy_(batch[k]) for k in self.keys}
                L.check(L.lib().fusg_plan_begin(self.rec.handle), "plan_begin")
                ops.RECORDER = self.rec
                try:
                    with ops.defer_range_check(), ops.status_scope(pipe.status_word()):
                        self.outputs = self.fn(self.inputs, vehicle_seeds)
                finally:
                    ops.RECORDER = None
                    L.check(L.lib().fusg_plan_end(self.rec.handle), "plan_end")
            torch.cuda.synchronize(self.device)
        self.size = int(L.lib().fusg_plan_size(self.rec.handle))
        # the plan holds raw pointers into each network's packed-weight cache: remember which cache it was recorded on
        self.generations = [n.generation for n in pipe._nets]

    def __del__(self):
        try:
            from . import _lib as L
            torch.cuda.synchronize(self.device)
            L.lib().fusg_plan_destroy(self.rec.handle)
        except Exception:                                                     # interpreter shutdown
            pass

    def _refresh(self, batch, vehicle_seeds, next_slot, what: str) -> None:
        """What precedes every replay: the inputs refreshed in place, the VUnet's noise drawn (the reference's draw order) into
        the pinned ring slot `next_slot(plan)` says this replay reads."""
        from . import _lib as L
        for k in self.keys:
            src = batch[k]
            if src.data_ptr() != self.inputs[k].data_ptr():
                if src.shape != self.inputs[k].shape:
                    raise ValueError(f"CompiledPass: input '{k}' has shape {tuple(src.shape)}, recorded {tuple(self.inputs[k].shape)}")
                self.inputs[k].copy_(src, non_blocking=True)
        slot = next_slot(self.rec.handle)
        if slot < 0:
            L.check(-1, what)
        vu = self.pipe.vunet
        vu.set_vehicle_seeds(vehicle_seeds)
        gens = vu.__dict__.get("_vehicle_gens")
        for ring, shapes in self.rec.noise_slots:
            vu._fill_noise(ring[slot], shapes, gens)

    def _issue(self, batch, vehicle_seeds):
        from . import _lib as L
        lib = L.lib()
        self._refresh(batch, vehicle_seeds, lib.fusg_plan_next_slot, "plan_next_slot")
        if PLAN_THREADS:
            L.check(lib.fusg_plan_run_mt(self.rec.handle), "plan_run_mt")     # one issuing host thread per recorded stream
        else:
            L.check(lib.fusg_plan_run(self.rec.handle), "plan_run")
        return self.outputs

    # ---- the recording as one hipGraph: a measurement path (tools/graph_capture_probe.py), not used by the product
    def capture_graph(self) -> int:
        """Capture this recording into ONE hipGraph (fusg_plan_graph_capture: the library re-issues its launch closures
        under a thread-local stream capture; no Python runs inside the capture).  Returns the graph's node count."""
        from . import _lib as L
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            L.check(L.lib().fusg_plan_graph_capture(self.rec.handle, self.stream.cuda_stream, 0), "plan_graph_capture")
        return int(L.lib().fusg_plan_graph_nodes(self.rec.handle))

    def run_graph(self, batch, vehicle_seeds=None):
        """`_issue` through the captured graph: inputs refreshed in place, the noise drawn into the graph's pinned slot."""
        from . import _lib as L
        lib = L.lib()
        with torch.cuda.device(self.device):
            self._refresh(batch, vehicle_seeds, lib.fusg_plan_graph_slot, "plan_graph_slot")
            L.check(lib.fusg_plan_graph_launch(self.rec.handle, self.stream.cuda_stream), "plan_graph_launch")
        return self.outputs

    def run(self, batch: Dict[str, torch.Tensor], vehicle_seeds: Optional[Sequence[int]] = None,
            check: Optional[str] = "sync") -> Dict[str, torch.Tensor]:
        """Same contract as VehiclePipeline.run (incl. the range guard: on a raised status the pass is redone eagerly in
        exact fp32).  Must be called with the stream that was current at compile time."""
        from . import ops
        with torch.cuda.device(self.device):
            if torch.cuda.current_stream(self.device) != self.stream:
                raise RuntimeError("CompiledPass.run: the current stream differs from the one the pass was recorded on")
            if ops.PRECISION != self.precision:
                raise RuntimeError(f"CompiledPass.run: recorded with precision {self.precision}, now {ops.PRECISION}")
            if [n.generation for n in self.pipe._nets] != self.generations:
                raise RuntimeError("CompiledPass.run: a network's parameters changed (load_state_dict / .to() / refresh()) "
                                   "after this pass was recorded - its launches point into the old packed weights; "
                                   "call pipe.compile() again")
            rng = torch.get_rng_state() if (vehicle_seeds is None and check == "sync" and ops.range_guarded()) else None
            out = self._issue(batch, vehicle_seeds)
            if not ops.range_guarded() or check != "sync":
                return out
            if not ops.range_exceeded(self.device, word=self.pipe.status_word()):
                return out
            with ops.route_batch(self.route_batch):
                return _redo_f32(lambda: self.fn(batch, vehicle_seeds), rng)


def synth_clip(vehicles: int, frames: int, res: int, device, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Synthetic clip-mode inputs (vehicle-major, then frame)."""
    from .synth import synth_inputs
    v = synth_inputs("vunet", vehicles, res, seed)
    return {"hg_x": synth_inputs("hg", vehicles, res, seed)["x"].to(device),
            "icn_x": synth_inputs("icn", vehicles * frames, res, seed)["x"].view(vehicles, frames, 21, res, res).to(device),
            "vu_x": v["x"].to(device),
            "vu_y": synth_inputs("vunet", vehicles * frames, res, seed + 1)["y_tilde"].view(vehicles, frames, 3, res, res).to(device)}


INPAINT_SCENE_FORMS = ("{'boxes' [V, 4], 'img' [V, 3, R, R], 'gray' / 'edge' / 'mask' [V, 1, R, R]} (EdgeConnect's inputs, given) or "
                       "{'boxes' [V, 4], 'det_masks' uint8 [V, 1, H, W]} (the detector's masks: the inputs are built on the device) or "
                       "{'boxes' [V, 4], 'box_masks' V pieces [h_v, w_v] uint8 / float32, or a packed (buffer, offsets) pair} (the "
                       "detector's masks in box coordinates)")


def inpaint_scene_form(inp) -> str:
    """Which of its three forms scene['inpaint'] has: 'given' (the four tensors), 'det_masks' (frame coordinates) or
    'box_masks' (box coordinates); ValueError when it is missing, mixes them or completes none."""
    keys = set(inp.keys()) if inp is not None else set()
    given, some = {"img", "gray", "edge", "mask"} <= keys, bool({"img", "gray", "edge", "mask"} & keys)
    if "boxes" in keys and given and not {"det_masks", "box_masks"} & keys:
        return "given"
    if "boxes" in keys and "det_masks" in keys and not some and "box_masks" not in keys:
        return "det_masks"
    if "boxes" in keys and "box_masks" in keys and not some and "det_masks" not in keys:
        return "box_masks"
    raise ValueError("run_frame: this pipeline was built with inpaint=True; the scene needs 'inpaint' = " + INPAINT_SCENE_FORMS
                     + (f", got the keys {sorted(keys)}" if keys else ""))


def synth_batch(batch: int, res: int, device, inpaint: bool = False, seed: int = 0, nhwc: bool = False) -> Dict[str, torch.Tensor]:
    """Synthetic, device-resident inputs of the shapes/ranges the reference feeds.
    nhwc=True (CUDA devices): the tensors are handed over in the layout the frame driver's glue kernels write and the
    stems read in place - NHWC-physical, channel pitch padded with zeros to the stem's K-channels (4 / 24 / 8 / 4; logical
    shape and values unchanged) - so a pass starts without the four NCHW -> NHWC conversion launches a caller with
    standard-contiguous tensors pays (`ops.as_nhwc` at every network's entry)."""
    from .synth import synth_inputs
    b = {"hg_x": synth_inputs("hg", batch, res, seed)["x"], "icn_x": synth_inputs("icn", batch, res, seed)["x"]}
    v = synth_inputs("vunet", batch, res, seed)
    b["vu_x"], b["vu_y"] = v["x"], v["y_tilde"]
    if inpaint:
        e = synth_inputs("edge", batch, res, seed)
        b.update(ec_img=e["img"], ec_gray=e["gray"], ec_edge=e["edge"], ec_mask=e["mask"])
    out = {k: t.to(device) for k, t in b.items()}
    if nhwc and torch.device(device).type == "cuda":
        from . import ops
        pitch = {"hg_x": 4, "icn_x": 24, "vu_x": 8, "vu_y": 4}
        with torch.cuda.device(device):
            for k, cp in pitch.items():
                out[k] = ops.as_nhwc(out[k].contiguous(), cpad=cp)
    return out


def synth_frame(vehicles: int, frame_hw=(720, 1280), device="cuda", seed: int = 0, inpaint=False) -> Dict:
    """A synthetic frame for `VehiclePipeline.run_frame`: smooth random texture, `vehicles` detector boxes, and per
    vehicle what the reference's renderer would hand over - an elliptical sketch (normal-map colours) with its mask,
    five texture-plane quadrilaterals (corner points before and after a small pose change, visibilities) and the planes
    cut out of the frame with them (`fusg_fill_poly_planes_u8`), plus 12 CAD keypoints and camera intrinsics.  All
    pixel data lives on `device`; point lists and boxes are host arrays, as in the reference.  inpaint=True adds
    scene['inpaint'] with EdgeConnect's four (synthetic) input tensors, inpaint="masks" with stand-in detector masks instead."""
    import numpy as np

    from .warp_learn import planes_utils as pu
    H, W = frame_hw
    g = np.random.default_rng(seed)
    dev = torch.device(device)
    tg = torch.Generator().manual_seed(seed)
    low = torch.rand((1, 3, H // 16 + 2, W // 16 + 2), generator=tg)
    tex = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)[0]
    tex = (tex + 0.08 * torch.rand((3, H, W), generator=tg)).clamp(0, 1)
    frame = (tex.permute(1, 2, 0) * 255).to(torch.uint8).contiguous().to(dev)
    yy, xx = np.mgrid[0:H, 0:W]
    bboxes, masks, sk_src, sk_dst, planes, src_kp, dst_kp, src_vis, dst_vis, kp3d = [], [], [], [], [], [], [], [], [], []
    for v in range(vehicles):
        bw, bh = int(g.integers(W // 8, W // 4)), int(g.integers(H // 6, H // 3))
        x0 = int(g.integers(-bw // 6, W - bw + bw // 6))                       # some boxes run off the frame
        y0 = int(g.integers(-bh // 6, H - bh + bh // 6))
        bboxes.append([x0, y0, x0 + bw, y0 + bh])
        cx, cy = x0 + bw / 2, y0 + bh / 2
        ell = (((xx - cx) / (0.45 * bw)) ** 2 + ((yy - cy) / (0.42 * bh)) ** 2) <= 1.0
        if not ell.any():
            ell[min(max(int(cy), 0), H - 1), min(max(int(cx), 0), W - 1)] = True
        m = ell.astype(np.uint8)
        nrm = np.stack([(xx - cx) / (0.45 * bw), (yy - cy) / (0.42 * bh), np.ones_like(xx, dtype=np.float64) * 0.6], -1)
        col = np.clip((nrm * 0.5 + 0.5) * 255, 1, 255).astype(np.uint8) * m[..., None]
        masks.append(m)
        sk_src.append(col)
        sk_dst.append(np.ascontiguousarray(col[..., ::-1]) if v % 2 else col)
        # five quadrilaterals / hexagons inside the box, and the same after a small perturbation
        def poly(n, ox, oy, sx, sy):
            ang = np.sort(g.uniform(0, 2 * np.pi, n))
            return np.stack([cx + ox * bw + sx * bw * np.cos(ang), cy + oy * bh + sy * bh * np.sin(ang)], 1)
        spec = [(6, -0.18, 0.0, 0.22, 0.3), (6, 0.18, 0.0, 0.22, 0.3), (4, 0.0, -0.2, 0.25, 0.15), (4, 0.0, 0.05, 0.2, 0.2),
                (4, 0.0, 0.25, 0.25, 0.12)]
        s_pts = [poly(*sp) for sp in spec]
        d_pts = [p + g.normal(0, 0.02 * bw, p.shape) for p in s_pts]
        src_kp.append([np.int32(p) for p in s_pts])
        dst_kp.append([np.int32(p) for p in d_pts])
        vis = g.integers(0, 2, 5).astype(np.uint8)
        vis[2] = 1
        src_vis.append(vis)
        dv = vis.copy()
        if v % 3 == 1:                                                        # exercise the left/right symmetry swap
            dv[0], dv[1] = 0, 1
        dst_vis.append(dv)
        planes.append(pu.fill_planes(frame, src_kp[-1]))
        kp3d.append((g.uniform(-1, 1, (12, 3)) * np.array([0.9, 0.5, 2.0]) * 5).astype(np.float32))
    t8 = lambda a: torch.from_numpy(np.ascontiguousarray(np.stack(a))).to(dev)   # noqa: E731
    extra = {}
    if inpaint:                                                               # EdgeConnect's inputs per vehicle (given, see run_frame)
        from .synth import synth_inputs
        e = synth_inputs("edge", vehicles, 256, seed) if inpaint != "masks" else None
        boxes = synth_inpaint_boxes(bboxes, (H, W))
        if inpaint == "masks":                                                # ... or a stand-in for the detector's masks (built on the device)
            extra["inpaint"] = {"boxes": np.asarray(boxes, dtype=np.int64), "det_masks": synth_det_masks(masks, boxes).to(dev)}
        else:
            extra["inpaint"] = {"boxes": np.asarray(boxes, dtype=np.int64), "img": e["img"].to(dev), "gray": e["gray"].to(dev),
                                "edge": e["edge"].to(dev), "mask": e["mask"].to(dev)}
    return {**extra, "frame": frame, "bboxes": np.asarray(bboxes, dtype=np.int64), "masks": t8(masks), "src_sketch": t8(sk_src),
            "dst_sketch": t8(sk_dst), "src_planes": torch.stack(planes), "src_kp": src_kp, "dst_kp": dst_kp,
            "src_vis": np.stack(src_vis), "dst_vis": np.stack(dst_vis), "kp3d": np.stack(kp3d),
            "focals": np.array([1.1 * W, 1.1 * W], np.float32), "centers": np.array([W / 2, H / 2], np.float32)}


def synth_inpaint_boxes(bboxes, frame_hw, shift=None) -> list:
    """bbox_new_img of every detector box: the 1.3x box (its centre moved by shift[v] = (dx, dy)), clipped to the frame."""
    H, W = frame_hw
    boxes = []
    for v, (x0, y0, x1, y1) in enumerate(bboxes):
        dx, dy = (0, 0) if shift is None else shift[v]
        cx, cy, bw, bh = (x0 + x1) / 2 + dx, (y0 + y1) / 2 + dy, 1.3 * (x1 - x0), 1.3 * (y1 - y0)
        bx0, by0 = max(0, int(cx - bw / 2)), max(0, int(cy - bh / 2))
        boxes.append([bx0, by0, max(bx0 + 2, min(W - 1, int(cx + bw / 2))), max(by0 + 2, min(H - 1, int(cy + bh / 2)))])
    return boxes


def inpaint_box_rule(bboxes, frame_hw):
    """bbox_new_img of every tracker box (x0, y0, x1, y1) by the reference's own rule (utils/inpaint_utils.py:22-23:
    BoundingBox(..., scale=1.3, bounds=(0, W - 1, 0, H - 1)), utils/bounding_box.py): each side moves out by int(1.3 w - w) // 2
    (resp. h), then the box is clipped to 0 .. W - 1 and 0 .. H - 1 -> int64 [V, 4], half-open.  `synth_inpaint_boxes` above is the
    synthetic scenes' stand-in (a centre shift, a minimum extent of 2): it rounds differently by up to a pixel and is kept as it
    is, since the recorded outputs of the synthetic passes depend on it."""
    import numpy as np
    H, W = frame_hw
    b = np.asarray(bboxes, dtype=np.int64).reshape(-1, 4)
    out = np.zeros_like(b)
    for v, (x0, y0, x1, y1) in enumerate(b.tolist()):
        w, h = x1 - x0, y1 - y0
        dw, dh = int(w * 1.3 - w) // 2, int(h * 1.3 - h) // 2
        out[v] = (max(0, x0 - dw), max(0, y0 - dh), min(W - 1, x1 + dw), min(H - 1, y1 + dh))
    return out


def foreground_cores(bboxes, core_frac: float = 0.5):
    """Every tracker box (x0, y0, x1, y1) shrunk about its centre to core_frac of its width and height, in integers: the core is
    floor(core_frac * w + 0.5) wide, and (w - that) // 2 comes off both sides (likewise h) -> int64 [V, 4]."""
    import numpy as np
    if not 0.0 < core_frac <= 1.0:
        raise ValueError(f"foreground_cores: core_frac = {core_frac} (0 < core_frac <= 1)")
    b = np.asarray(bboxes, dtype=np.int64).reshape(-1, 4)
    out = np.zeros_like(b)
    for v, (x0, y0, x1, y1) in enumerate(b.tolist()):
        w, h = x1 - x0, y1 - y0
        mx, my = (w - int(core_frac * w + 0.5)) // 2, (h - int(core_frac * h + 0.5)) // 2
        out[v] = (x0 + mx, y0 + my, x1 - mx, y1 - my)
    return out


def synth_box_masks(masks: torch.Tensor, boxes, dtype=torch.uint8) -> list:
    """`synth_det_masks`'s planes [V, 1, H, W] cut to their boxes, as a detector run on the box crop returns them: V pieces
    [h_v, w_v], uint8 as they are or float32 in [0, 1]."""
    out = []
    for v, (x0, y0, x1, y1) in enumerate(boxes):
        m = masks[v, 0, int(y0):int(y1), int(x0):int(x1)]
        out.append(m.contiguous() if dtype == torch.uint8 else (m.to(torch.float32) / 255.0).contiguous())
    return out


def synth_det_masks(masks, boxes, grow: int = 3) -> torch.Tensor:
    """A stand-in for a detector's masks, uint8 [V, 1, H, W] (255 = vehicle): each vehicle mask of `synth_frame` grown by
    `grow` pixels (a square max filter) and cut to its inpaint box."""
    import numpy as np
    m = torch.from_numpy(np.ascontiguousarray(np.stack(masks))).float()[:, None]
    m = torch.nn.functional.max_pool2d(m, 2 * grow + 1, stride=1, padding=grow)
    out = torch.zeros(m.shape, dtype=torch.uint8)
    for v, (x0, y0, x1, y1) in enumerate(boxes):
        out[v, 0, y0:y1, x0:x1] = (m[v, 0, y0:y1, x0:x1] > 0).to(torch.uint8) * 255
    return out


def synth_later_frame(scene: Dict, step: int, inpaint=None) -> Dict:
    """The scene of `synth_frame` one trajectory step later, for `run_later_frame`: the same vehicles (masks, first-frame planes
    and their corner points), new plane corner points for the new pose (seeded by `step`), the source sketch as the new pose's
    sketch, and one noise seed per (vehicle, step) when the first frame had per-vehicle seeds.  inpaint: None (the scene as it
    always was; a first frame's 'inpaint' entry passes through untouched) or the form of scene['inpaint'] for this step's boxes
    (the 1.3x boxes moved by a few pixels, seeded by `step`): "given" (synthetic tensors), "masks" (`synth_det_masks`) or
    "box_masks" (`synth_box_masks`, uint8)."""
    import numpy as np
    g = np.random.default_rng(1000 + step)
    out = dict(scene)
    out["dst_kp"] = [[np.int32(p + g.normal(0, 3.0, p.shape)) for p in veh] for veh in scene["src_kp"]]
    out["dst_sketch"] = scene["src_sketch"]
    if scene.get("vehicle_seeds") is not None:
        out["vehicle_seeds"] = [int(sd) * 64 + step for sd in scene["vehicle_seeds"]]
    if inpaint is not None:
        if inpaint not in ("given", "masks", "box_masks"):
            raise ValueError(f"synth_later_frame: inpaint must be None, 'given', 'masks' or 'box_masks', got {inpaint!r}")
        dev = scene["frame"].device
        H, W = int(scene["frame"].shape[0]), int(scene["frame"].shape[1])
        V = len(scene["bboxes"])
        gb = np.random.default_rng(2000 + step)                                # (its own generator: the draws above stay as they were)
        boxes = synth_inpaint_boxes(np.asarray(scene["bboxes"]).reshape(-1, 4).tolist(), (H, W), gb.integers(-6, 7, (V, 2)).tolist())
        inp = {"boxes": np.asarray(boxes, dtype=np.int64).reshape(-1, 4)}
        if inpaint == "given":
            from .synth import synth_inputs
            e = synth_inputs("edge", V, 256, 1000 + step)
            inp.update({k: e[k].to(dev) for k in ("img", "gray", "edge", "mask")})
        else:
            planes = synth_det_masks(list(scene["masks"].cpu().numpy()), boxes) if V else torch.zeros((0, 1, H, W), dtype=torch.uint8)
            if inpaint == "masks":
                inp["det_masks"] = planes.to(dev)
            else:
                inp["box_masks"] = [m.to(dev) for m in synth_box_masks(planes, boxes)]
        out["inpaint"] = inp
    return out
