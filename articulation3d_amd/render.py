"""The clip's 2-D visualisation: the four panels per frame of the reference's output.mp4 (tools/inference.py:230-276),
`[opt seg | opt normal | raw seg | raw normal]`, rendered on the GPU by one launch per pair of panels (a3d_render_panels,
csrc/render.hip; the law is stated in include/a3d.h).

`build_layers` is pure host code (numpy, no GPU): it turns a clip's list[Instances] into the kernel's tables.  What it
restates of the reference's drawing:

  * instances drawn: score > conf_threshold, as get_pred_labeled (arti_vis.py:218-225) filters the boxes.  The same
    filter is applied to the arrows.  For the raw panels that is what draw_pred draws (everything create_instances kept,
    the same set at the same threshold).  For the OPTIMISED panels it is a deliberate departure: the reference draws
    an arrow for every detection, also one whose score the optimiser re-weighted below the threshold, and filters that
    panel's boxes at draw_pred's default 0.7 whatever --conf-threshold says; here one threshold decides arrows and boxes of
    both pairs of panels.  The NORMAL panel takes every instance of the frame, as get_normal_map does.
  * colours: the arti metadata (builtin.py), class 0 arti_rot (0,130,200), class 1 arti_tran (230,25,75).
  * per-frame layer order: detectron2's overlay_instances sorts by box area, largest first (here with ties in ascending
    index), and draw_pred draws its arrows before it:
        1. if mask_alpha > 0, one MASK layer per drawn instance, descending area (the reference passes `#masks=masks`,
           i.e. no masks: the default mask_alpha = 0 gives none);
        2. one arrow layer per drawn instance, ascending index, alpha 256;
        3. one box layer per drawn instance, descending area, alpha 128 (detectron2's 0.5).
  * box layer: 4 non-overlapping axis-aligned strips of width 2.5 px centred on the box edges (detectron2's
    linewidth max(font / 4, 1) with its default font size 10 at 480x640): top and bottom strips span the outer width, left
    and right strips the height between them.
  * arrow layer: end points as draw_pred (arti_vis.py:366-402): angle_offset_to_axis with H = h_box, W = w_box and the
    centre (w_box / 2, h_box / 2), shifted by the box origin; for arti_tran the zero offset is appended.  draw_pred zips
    the WHOLE translation table with that one centre, so every arti_tran arrow of a frame takes row 0 of pred_tran_axis:
    kept as it is.  Geometry: matplotlib's FancyArrow with width = 10 / 3, head_width = 5 width, head_length = 1.5
    head_width, overhang = 0.5, length_includes_head = True.  Its outline has two reflex vertices (the notches), so with
    at most 4 half-planes per convex piece the exact decomposition takes four pieces: the shaft quad, the two head
    triangles (tip, barb, notch) and the core triangle (tip, left notch, right notch) between them.  A degenerate axis
    (both end points equal) gives no arrow layer.  A head longer than the arrow: FancyArrow itself does not rescale
    (its outline then folds over itself); here the head is CLAMPED -- head length and head width are scaled by
    length / head_length, so the head ends at the tail and the shaft keeps its width up to the notch.
  * half-planes are computed in float64 and rounded to fp32, oriented so that inside is >= 0.
  * text labels ("idx: score") are out of scope: there is no font rasteriser here.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

COLORS = ((0, 130, 200), (230, 25, 75))  # arti_rot, arti_tran
BOX_ALPHA, ARROW_ALPHA = 128, 256
BOX_LINE = 2.5
ARROW_WIDTH = 10.0 / 3.0
ARROW_HEAD_WIDTH = 5.0 * ARROW_WIDTH
ARROW_HEAD_LENGTH = 1.5 * ARROW_HEAD_WIDTH
ARROW_OVERHANG = 0.5

LAYER_DTYPE = np.dtype(_lib.RenderLayer)
PIECE_DTYPE = np.dtype(_lib.RenderPiece)


@dataclass
class LayerTables:
    """The tables of a3d_render_panels for one clip, on the host."""
    H: int
    W: int
    layer_off: np.ndarray  # [F+1] int32
    layers: np.ndarray     # [L] LAYER_DTYPE
    pieces: np.ndarray     # [P] PIECE_DTYPE
    inst_off: np.ndarray   # [F+1] int32
    inst_row: np.ndarray   # [n_inst] int32: row of the mask table
    mask_keys: List[Tuple[int, int]]  # (frame, instance) of every mask-table row, = of every normal-panel instance

    @property
    def num_frames(self) -> int:
        return len(self.layer_off) - 1


def _np(v) -> np.ndarray:
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def convex_piece(verts) -> Optional[np.ndarray]:
    """Convex polygon (3 or 4 vertices, either winding) -> [4,3] fp32 half-planes with inside >= 0 (float64, then rounded),
    rows past the vertex count zero; None for a polygon without area."""
    v = np.asarray(verts, dtype=np.float64)
    n = len(v)
    assert 3 <= n <= 4
    area2 = sum(v[i, 0] * v[(i + 1) % n, 1] - v[(i + 1) % n, 0] * v[i, 1] for i in range(n))
    if area2 == 0.0:
        return None
    sgn = 1.0 if area2 > 0 else -1.0
    out = np.zeros((4, 3), np.float64)
    for i in range(n):
        (xa, ya), (xb, yb) = v[i], v[(i + 1) % n]
        a, b = -(yb - ya) * sgn, (xb - xa) * sgn  # the inward normal of edge a -> b
        norm = np.hypot(a, b)
        if norm == 0.0:
            return None
        out[i] = (a / norm, b / norm, -(a * xa + b * ya) / norm)
    return out.astype(np.float32)


def _cull_box(verts, H: int, W: int) -> Tuple[int, int, int, int]:
    """Integer pixel box [x0,x1) x [y0,y1) that holds every pixel whose centre can test inside the polygon (one pixel of
    slack for the fp32 rounding of the half-planes), clamped to the image."""
    v = np.asarray(verts, dtype=np.float64)
    lim = 1 << 24  # (far-away garbage coordinates: keep the arithmetic in int32)
    x0, y0 = np.floor(np.clip(v.min(0), -lim, lim)).astype(np.int64) - 1
    x1, y1 = np.ceil(np.clip(v.max(0), -lim, lim)).astype(np.int64) + 1
    return int(min(max(x0, 0), W)), int(min(max(y0, 0), H)), int(min(max(x1, 0), W)), int(min(max(y1, 0), H))


def box_polys(box) -> List[np.ndarray]:
    """The four strips of a box outline (vertex lists): top, bottom, left, right."""
    x0, y0, x1, y1 = (float(t) for t in box)
    h = BOX_LINE / 2
    rect = lambda xa, ya, xb, yb: np.array([[xa, ya], [xb, ya], [xb, yb], [xa, yb]], np.float64)
    return [rect(x0 - h, y0 - h, x1 + h, y0 + h), rect(x0 - h, y1 - h, x1 + h, y1 + h),
            rect(x0 - h, y0 + h, x0 + h, y1 - h), rect(x1 - h, y0 + h, x1 + h, y1 - h)]


def arrow_polys(x0: float, y0: float, x1: float, y1: float) -> List[np.ndarray]:
    """FancyArrow's outline from (x0,y0) to the tip (x1,y1) as convex pieces: shaft quad, left / right head triangles
    (tip, barb, notch), core triangle (tip, left notch, right notch).  [] for a degenerate axis."""
    dx, dy = float(x1) - float(x0), float(y1) - float(y0)
    length = float(np.hypot(dx, dy))
    if length == 0.0:
        return []
    hw, hl, lw = ARROW_HEAD_WIDTH, ARROW_HEAD_LENGTH, ARROW_WIDTH
    if hl > length:  # the clamp (see the module docstring)
        hw, hl = hw * length / hl, length
    nx = hl * (1.0 - ARROW_OVERHANG)  # where the head meets the stem
    cx, sx = dx / length, dy / length
    M = np.array([[cx, sx], [-sx, cx]])
    place = lambda pts: np.dot(np.asarray(pts, np.float64), M) + [float(x1), float(y1)]  # FancyArrow._make_verts
    tip = [0.0, 0.0]
    return [place([[-length, -lw / 2], [-nx, -lw / 2], [-nx, lw / 2], [-length, lw / 2]]),
            place([tip, [-hl, -hw / 2], [-nx, -lw / 2]]),
            place([tip, [-hl, hw / 2], [-nx, lw / 2]]),
            place([tip, [-nx, -lw / 2], [-nx, lw / 2]])]


def axis_end_points(inst, i: int) -> Tuple[float, float, float, float]:
    """draw_pred's arrow end points of instance i (arti_vis.py:370-400), in float32 as there."""
    from .utils.opt_utils import angle_offset_to_axis

    box = inst.pred_boxes.tensor[i].detach().cpu().float()
    w_box, h_box = box[2] - box[0], box[3] - box[1]
    if int(_np(inst.pred_classes)[i]) == 1:
        tran = torch.as_tensor(_np(inst.pred_tran_axis), dtype=torch.float32).reshape(-1, 2)
        ao = torch.cat((tran, torch.zeros(len(tran), 1)), 1)[:1]  # (zip with ONE centre: row 0, see the module docstring)
    else:
        ao = torch.as_tensor(_np(inst.pred_rot_axis), dtype=torch.float32).reshape(-1, 3)[i:i + 1]
    centre = torch.stack((w_box / 2, h_box / 2))[None]
    pts = angle_offset_to_axis(ao, centre, H=float(h_box), W=float(w_box)).float()[0]
    return float(pts[0] + box[0]), float(pts[1] + box[1]), float(pts[2] + box[0]), float(pts[3] + box[1])


def build_layers(preds: Sequence, H: int, W: int, mask_alpha: float = 0.0, conf_threshold: float = 0.7) -> LayerTables:
    """list[Instances] of a clip -> the tables of a3d_render_panels (module docstring: order, colours, geometry)."""
    a_mask = int(round(float(mask_alpha) * 256))
    if not 0 <= a_mask <= 256:
        raise ValueError(f"mask_alpha {mask_alpha} outside [0, 1]")
    layers: list = []
    pieces: list = []
    layer_off, inst_off, mask_keys = [0], [0], []

    def poly_layer(polys, color, alpha):
        p0 = len(pieces)
        kept = []
        for v in polys:
            hp = convex_piece(v)
            if hp is not None:
                pieces.append((len(v), hp, _cull_box(v, H, W)))
                kept.append(v)
        if not kept:
            return
        x0, y0, x1, y1 = _cull_box(np.concatenate(kept), H, W)
        layers.append((_lib.RENDER_POLY, alpha, tuple(color) + (0,), x0, y0, x1, y1, p0, len(pieces)))

    for f, inst in enumerate(preds):
        n = len(inst.pred_boxes)
        boxes = _np(inst.pred_boxes.tensor).reshape(-1, 4).astype(np.float64)
        scores, classes = _np(inst.scores).reshape(-1), _np(inst.pred_classes).reshape(-1)
        masks = inst.pred_masks if inst.has("pred_masks") else None
        has_masks = masks is not None and len(masks) == n
        row_of = {}
        if has_masks:
            for i in range(n):
                row_of[i] = len(mask_keys)
                mask_keys.append((f, i))
        drawn = [i for i in range(n) if float(scores[i]) > conf_threshold]
        area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
        by_area = sorted(drawn, key=lambda i: (-area[i], i))
        if a_mask > 0 and has_masks:
            for i in by_area:
                layers.append((_lib.RENDER_MASK, a_mask, COLORS[int(classes[i])] + (0,), 0, 0, W, H, row_of[i], row_of[i] + 1))
        for i in drawn:
            poly_layer(arrow_polys(*axis_end_points(inst, i)), COLORS[int(classes[i])], ARROW_ALPHA)
        for i in by_area:
            poly_layer(box_polys(boxes[i]), COLORS[int(classes[i])], BOX_ALPHA)
        layer_off.append(len(layers))
        inst_off.append(len(mask_keys))

    piece_arr = np.zeros(len(pieces), PIECE_DTYPE)
    for k, (nh, hp, box) in enumerate(pieces):
        piece_arr[k]["n"], piece_arr[k]["abc"] = nh, hp
        piece_arr[k]["x0"], piece_arr[k]["y0"], piece_arr[k]["x1"], piece_arr[k]["y1"] = box
    return LayerTables(H=int(H), W=int(W), layer_off=np.asarray(layer_off, np.int32), layers=np.array(layers, LAYER_DTYPE) if layers else np.zeros(0, LAYER_DTYPE),
                       pieces=piece_arr, inst_off=np.asarray(inst_off, np.int32), inst_row=np.arange(len(mask_keys), dtype=np.int32),
                       mask_keys=mask_keys)


def unit_normals(preds: Sequence, tables: LayerTables) -> torch.Tensor:
    """F.normalize(pred_planes) per frame in torch fp32 on the host -- the very operation of get_normal_map -- one row per
    normal-panel instance."""
    by_frame = {}
    for f, _i in tables.mask_keys:
        if f not in by_frame:
            by_frame[f] = torch.nn.functional.normalize(torch.as_tensor(_np(preds[f].pred_planes), dtype=torch.float32).reshape(-1, 3), p=2)
    rows = [by_frame[f][i] for f, i in tables.mask_keys]
    return torch.stack(rows) if rows else torch.zeros((0, 3), dtype=torch.float32)


def _dev_bytes(arr: np.ndarray, device) -> Optional[torch.Tensor]:
    if arr.size == 0:
        return None
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).to(device)


def launch(frames_u8: torch.Tensor, tables: LayerTables, normals: torch.Tensor, bits: Optional[torch.Tensor], out: torch.Tensor,
           col: int = 0, inst_row: Optional[np.ndarray] = None) -> torch.Tensor:
    """One a3d_render_panels launch on the current stream: uploads the tables and fills out[:, :, col : col + 2W]."""
    from . import opt_ops

    F, H, W, _ = frames_u8.shape
    if (H, W) != (tables.H, tables.W) or F != tables.num_frames:
        raise ValueError(f"frames {tuple(frames_u8.shape)} do not match tables for {tables.num_frames} x {tables.H} x {tables.W}")
    dev = frames_u8.device
    inst_row = tables.inst_row if inst_row is None else np.asarray(inst_row, np.int32)
    keep = [_dev_bytes(tables.layer_off, dev), _dev_bytes(tables.layers, dev), _dev_bytes(tables.pieces, dev), _dev_bytes(tables.inst_off, dev),
            _dev_bytes(inst_row, dev), normals.to(dev, torch.float32).contiguous() if len(normals) else None]
    opt_ops.render_panels_tables(frames_u8, *keep, bits if bits is not None and len(bits) else None, out, col=col)
    for t in keep:  # uploaded on this stream, possibly freed by a caller on another one
        if t is not None:
            t.record_stream(torch.cuda.current_stream())
    return out


def render_panels(frames_u8: torch.Tensor, preds: Sequence, out: Optional[torch.Tensor] = None, col: int = 0, mask_alpha: float = 0.0,
                  bank=None, conf_threshold: float = 0.7) -> torch.Tensor:
    """frames uint8 [F,H,W,3] on the device + the frames' Instances -> out[:, :, col : col+W] = seg panels,
    out[:, :, col+W : col+2W] = normal panels (out uint8 [F,H,pitch,3]; default a fresh [F,H,2W,3]).  The masks are
    bit-packed here, or taken from `bank` (an opt_utils._MaskBank over the same preds that holds every instance)."""
    from . import opt_ops

    F, H, W, _ = frames_u8.shape
    tables = build_layers(preds, H, W, mask_alpha=mask_alpha, conf_threshold=conf_threshold)
    if out is None:
        out = torch.empty((F, H, 2 * W, 3), device=frames_u8.device, dtype=torch.uint8)
    inst_row, bits = None, None
    if tables.mask_keys:
        if bank is not None:
            missing = [k for k in tables.mask_keys if k not in bank.index]
            if missing or (bank.H, bank.W) != (H, W):
                raise KeyError(f"the mask bank does not hold {len(missing)} of the clip's instances (first: {missing[:1]})")
            inst_row, bits = np.asarray([bank.index[k] for k in tables.mask_keys], np.int32), bank.bits
            for rec in tables.layers:  # MASK layers point at mask-table rows too
                if rec["kind"] == _lib.RENDER_MASK:
                    rec["p0"] = inst_row[rec["p0"]]
                    rec["p1"] = rec["p0"] + 1
        else:
            u8 = torch.cat([(torch.as_tensor(preds[f].pred_masks) > 0.5).to(torch.uint8) for f in sorted({f for f, _ in tables.mask_keys})])
            bits = opt_ops.pack_masks(u8.to(frames_u8.device).contiguous())
    return launch(frames_u8, tables, unit_normals(preds, tables), bits, out, col=col, inst_row=inst_row)


def render_clip(frames_u8: torch.Tensor, preds_raw: Sequence, preds_opt: Sequence, chunk: int = 32, mask_alpha: float = 0.0,
                conf_threshold: float = 0.7) -> Iterator[np.ndarray]:
    """Yields the clip's rows `[opt seg | opt normal | raw seg | raw normal]` as host arrays [f,H,4W,3], `chunk` frames at a
    time.  frames_u8: uint8 [F,H,W,3] on the device (or on the host: each chunk is uploaded as it is needed).  Rendering is
    double-buffered on the device and the D2H copies run on streams.side(2), the pool's copy-pipeline role: chunk k's copy
    runs while chunk k+1 renders.  The host side is a ring of THREE pinned buffers: asking for chunk k+1 starts the copy of
    chunk k+2 behind the caller's back, so with two buffers that copy would land in the array of chunk k the caller has
    just been given.  With three, a yielded array stays valid while the NEXT chunk is requested and used, and is
    overwritten when the one after that is requested: be done with chunk k (or copy it) before asking for chunk k+2."""
    from . import streams

    F, H, W, _ = frames_u8.shape
    assert len(preds_raw) == F and len(preds_opt) == F
    dev = frames_u8.device if frames_u8.is_cuda else torch.device("cuda", torch.cuda.current_device())
    copy_stream, main = streams.side(2, dev), torch.cuda.current_stream(dev)
    chunk = max(1, min(int(chunk), max(F, 1)))
    pinned = [torch.empty((chunk, H, 4 * W, 3), dtype=torch.uint8).pin_memory() for _ in range(3)]
    stage = [torch.empty((chunk, H, 4 * W, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
    left = [None, None]  # the event behind the last D2H copy out of each staging buffer
    pending = None       # (pinned buffer, frames, copy event) of the chunk that is handed over next
    for k, lo in enumerate(range(0, F, chunk)):
        hi, b = min(lo + chunk, F), k % 2
        if left[b] is not None:
            main.wait_event(left[b])  # the staging buffer is overwritten only after its copy has left
        fr = frames_u8[lo:hi].to(dev, non_blocking=True).contiguous()
        out = stage[b][:hi - lo]
        render_panels(fr, preds_opt[lo:hi], out=out, col=0, mask_alpha=mask_alpha, conf_threshold=conf_threshold)
        render_panels(fr, preds_raw[lo:hi], out=out, col=2 * W, mask_alpha=mask_alpha, conf_threshold=conf_threshold)
        rendered = torch.cuda.Event()
        rendered.record(main)
        host = pinned[k % 3][:hi - lo]  # (chunk k-3's array: the caller let go of it when it asked for chunk k-1)
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(rendered)
            host.copy_(out, non_blocking=True)
            left[b] = torch.cuda.Event()
            left[b].record(copy_stream)
        fr.record_stream(copy_stream)
        if pending is not None:  # hand the previous chunk over while this one renders / copies
            pending[1].synchronize()
            yield pending[0].numpy()
        pending = (host, left[b])
    if pending is not None:
        pending[1].synchronize()
        yield pending[0].numpy()
