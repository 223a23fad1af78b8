"""The reference for an inpainted FUTURE frame (trajectory_inference.py:301-350 inside :283-450), vehicle-serial on the CPU, from
pieces that exist: oracle.later_frame_pass for the crops and their geometry, oracle.edgeconnect for EdgeModel ->
InpaintingModel and the merge as oracle.frame_pass runs them, oracle.cv_host for the resizes and the paste, and the
reference's per-vehicle loop: the inpainted box first, then the vehicle's crop.  Not a test module."""
import numpy as np
import torch

import oracle
from oracle import cv_host as cv
from oracle.edgeconnect import edge_model_forward, inpaint_model_forward


def scene_cpu(scene):
    out = {}
    for k, v in scene.items():
        if isinstance(v, dict):
            out[k] = scene_cpu(v)
        elif isinstance(v, (list, tuple)) and v and torch.is_tensor(v[0]):
            out[k] = [t.cpu().numpy() for t in v]
        else:
            out[k] = v.cpu().numpy() if torch.is_tensor(v) else v
    return out


def overlapping_boxes(masks, boxes):
    """`boxes` (host [2, 4]) with each box grown to reach the middle of the OTHER vehicle's mask.  Box 1 over vehicle 0's mask is
    what shows the order: the reference pastes box 0, crop 0, box 1, crop 1, so box 1 covers part of crop 0 (all boxes first,
    then all crops, would leave crop 0 on top there)."""
    boxes = np.array(boxes, dtype=np.int64).reshape(-1, 4)
    for v, o in ((0, 1), (1, 0)):
        ys, xs = np.nonzero(np.asarray(masks[o]))
        cx, cy = int(xs.mean()), int(ys.mean())
        boxes[v] = (min(boxes[v, 0], cx), min(boxes[v, 1], cy), max(boxes[v, 2], cx + 1), max(boxes[v, 3], cy + 1))
    return boxes


def inpaint_crops(state_dicts, four):
    """EdgeModel -> InpaintingModel -> merge -> uint8 (truncation), one vehicle at a time (:328-336 as :124-129)."""
    out = []
    for v in range(four["img"].shape[0]):
        t = lambda k: torch.from_numpy(np.ascontiguousarray(four[k][v:v + 1]))     # noqa: E731
        e = edge_model_forward(state_dicts["edge"], t("gray"), t("edge"), t("mask"))
        p = inpaint_model_forward(state_dicts["inpaint"], t("img"), e, t("mask"))
        merged = (p * t("mask") + t("img") * (1 - t("mask"))) * 255.0
        out.append(merged.permute(0, 2, 3, 1)[0].numpy().astype(np.uint8))
    return np.stack(out)


def later_inpaint_pass(state_dicts, scene, state, four, boxes):
    """scene: the later scene on the host (numpy); state: oracle.frame_pass(...)['state']; four: EdgeConnect's inputs of this
    frame's boxes (numpy).  -> 'icn_u8', 'vunet_u8', 'geom', 'inpaint_u8', 'frame_icn', 'frame_vunet'."""
    ref = oracle.later_frame_pass(state_dicts, {k: v for k, v in scene.items() if k != "inpaint"}, state)
    ref["inpaint_u8"] = inpaint_crops(state_dicts, four)
    frame = scene["frame"]
    out = {"frame_icn": frame.copy(), "frame_vunet": frame.copy()}                 # :340: the composite starts from the frame
    for v in range(len(scene["masks"])):
        x0, y0, x1, y1 = (int(q) for q in boxes[v])
        box = cv.resize_linear_u8(ref["inpaint_u8"][v], (x1 - x0, y1 - y0))         # dsize = (w, h)
        g = [int(q) for q in ref["geom"][v]]
        info = {"crop_xy_min": (g[0], g[1]), "crop_size_orig": (g[3] - g[1], g[2] - g[0]), "pad_xy_before": (g[4], g[5]),
                "pad_xy_after": (g[6], g[7])}
        for k, crop in (("frame_icn", "icn_u8"), ("frame_vunet", "vunet_u8")):
            out[k][y0:y1, x0:x1] = box                                             # the box ...
            cv.paste_back(out[k], ref[crop][v], info, scene["masks"][v].astype(bool))   # ... then the crop
    ref.update(out)
    return ref
