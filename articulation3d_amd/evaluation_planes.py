"""Evaluate the plane stage: the reference's ScanNet box / mask / plane AP and plane statistics (ScannetEvaluator ->
evaluate_for_planes, pkg/evaluation/scannet_evaluation.py:254-450, over compare_planes of pkg/utils/metrics.py:6-19 and
pkg/utils/VOCap.py) and its depth_l1_dist, computed on the GPU.  Three VOC-style APs per class -- `box_ap@0.5`, `mask_ap@0.5`,
`plane_ap@iou0.5normal30.0offset0.3` --, their class means, and eight statistics of the plane errors.  Every detection is assigned the
ground truth its BOX overlaps most; it is a true positive of a metric if its class is that ground truth's, the metric's test holds
(box IoU > 0.5; mask IoU > 0.5; normal within 30 degrees and offset within 0.3 m) and no detection of higher score claimed the
ground truth for that metric before.

The masks are the heavy part: 307 KB per detection at 480 x 640.  process() and process_records() compare them AT ONCE, where the
detector left them (a3d_eval_mask_counts: one read of the mask bytes, no packed copy), and keep three int32 per detection -- its
ground truth, intersection and union --; no mask outlives its batch.  evaluate() then matches every detection of every image in ONE
launch (a3d_eval_plane_match), sorts the entries with torch.sort and reuses a3d_eval_ap.  The law of each launch is stated in
include/a3d.h and in numpy float64 by tests/plane_eval_ref.py.  Bookkeeping, depth rows and the gather are ArtiEvaluator's
(evaluation._EvaluatorBase).

The records' plane columns are used as they are: normal * the offset refitted to the depth map (csrc/heads_post.hip does the
reference's override_depth).  That offset may be negative and flip the normal, exactly as the reference's `normal * offset_new` does.

DEPARTURES from the reference, on purpose:
  * Box IoU, compare_planes and AP are float64 from the fp32 inputs; the reference computes them in fp32 (and the mask IoU in
    float64, as here).
  * Score ties: detections are ranked by (score descending, index) within an image and the AP entries sorted by score with a STABLE
    sort over (image index in the ground-truth table, rank); the statistics take the errors in that order too.  The reference's
    torch.sort is unstable and follows the order images were processed in; here nothing depends on batching, sharding or order.
  * An image without ground truth gives false positives (and no plane errors); the reference's argmax over an empty row raises.
  * Two empty masks have IoU 0 (pycocotools divides 0 by 0).
  * Polygon ground truth is refused: pycocotools' rasteriser is not here to pin against.  Convert to RLE first.
  * "Already covered" is decided as "the first qualifying detection per ground truth and metric, by rank", which equals the reference's
    sequential loop and runs in parallel.
  * Out of scope: COCO mAP, EVAL_GT_BOX, dataset registration.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .evaluation import _depth_l1_dist, _EvaluatorBase, _join64
from .utils import rle

STAT_KEYS = ("%normal<10", "%normal<30", "%offset<0.5", "%offset<0.3", "mean_normal", "median_normal", "mean_offset", "median_offset")
_PACK_CHUNK = 256  # ground-truth masks decoded, uploaded and packed per step (79 MB of bytes at 480 x 640)


def metric_keys(iou_thresh: float = 0.5, normal_threshold: float = 30.0, offset_threshold: float = 0.3):
    """The reference's three AP keys, formatted as it formats them."""
    return ("box_ap@%.1f" % iou_thresh, "mask_ap@%.1f" % iou_thresh,
            "plane_ap@iou%.1fnormal%.1foffset%.1f" % (iou_thresh, normal_threshold, offset_threshold))


def plane_statistics(normal_err: np.ndarray, offset_err: np.ndarray) -> "OrderedDict[str, float]":
    """The reference's eight plane statistics (scannet_evaluation.py:437-447) of float64 error lists, {} when they are empty."""
    n, o = np.asarray(normal_err, np.float64), np.asarray(offset_err, np.float64)
    res = OrderedDict()
    if len(n) == 0:
        return res
    res["%normal<10"] = float(np.sum(n < 10) / len(n) * 100)
    res["%normal<30"] = float(np.sum(n < 30) / len(n) * 100)
    res["%offset<0.5"] = float(np.sum(o < 0.5) / len(o) * 100)
    res["%offset<0.3"] = float(np.sum(o < 0.3) / len(o) * 100)
    res["mean_normal"], res["median_normal"] = float(n.mean()), float(np.median(n))
    res["mean_offset"], res["median_offset"] = float(o.mean()), float(np.median(o))
    return res


def parse_plane_coco(coco_dict: Dict, thing_classes: Optional[Sequence[str]] = None, image_hw=(480, 640)):
    """The host half of PlaneGroundTruth.from_coco: every check and every table but the packed masks.
    -> dict image_ids, gt [M,8] fp32 (box xyxy, plane, contiguous class), gt_off [I+1], npos [C], names, thing_classes, and
    `segmentations`: the RLE of every row of gt, in order (rle.decode turns one into its [H,W] mask)."""
    H, W = int(image_hw[0]), int(image_hw[1])
    cats = sorted(coco_dict["categories"], key=lambda c: c["id"])
    names = [c["name"] for c in cats]
    thing_classes = list(names if thing_classes is None else thing_classes)
    if len(thing_classes) != len(cats):
        raise ValueError(f"{len(thing_classes)} thing_classes for {len(cats)} categories")
    if not 1 <= len(cats) <= _lib.EVAL_MAX_CLASSES:
        raise ValueError(f"{len(cats)} categories: 1 .. {_lib.EVAL_MAX_CLASSES} are supported")
    contiguous = {c["id"]: i for i, c in enumerate(cats)}
    image_ids = [im["id"] for im in coco_dict["images"]]
    if len(set(image_ids)) != len(image_ids):
        raise ValueError("duplicate image ids")
    per_image = {iid: [] for iid in image_ids}
    npos = np.zeros(len(cats), np.int32)
    for ann in coco_dict["annotations"]:
        what = f"annotation {ann.get('id')}"
        if ann["category_id"] not in contiguous:
            raise ValueError(f"{what}: unknown category_id {ann['category_id']}")
        if ann["image_id"] not in per_image:
            raise ValueError(f"{what}: unknown image_id {ann['image_id']}")
        if ann.get("plane") is None or len(ann["plane"]) != 3:
            raise ValueError(f"{what}: no `plane` (three floats, normal * offset)")
        seg = ann.get("segmentation")
        if isinstance(seg, (list, tuple)):
            raise ValueError(f"{what}: polygon segmentation is not supported (there is no rasteriser to pin against pycocotools'); convert it to RLE")
        if not isinstance(seg, dict) or "counts" not in seg or "size" not in seg:
            raise ValueError(f"{what}: segmentation must be a COCO RLE dict (size, counts)")
        if [int(v) for v in seg["size"]] != [H, W]:
            raise ValueError(f"{what}: mask size {list(seg['size'])} is not image_hw {[H, W]}")
        per_image[ann["image_id"]].append(ann)
        npos[contiguous[ann["category_id"]]] += 1
    rows, gt_off, segs = [], [0], []
    for iid in image_ids:
        anns = per_image[iid]
        if len(anns) > _lib.EVAL_MAX_GT:
            raise ValueError(f"image {iid}: {len(anns)} annotations, at most {_lib.EVAL_MAX_GT} are supported")
        gt_off.append(gt_off[-1] + len(anns))
        for a in anns:
            x, y, w, h = (float(v) for v in a["bbox"])
            rows.append([x, y, x + w, y + h, *[float(v) for v in a["plane"]], float(contiguous[a["category_id"]])])  # (xyxy in float64, then fp32)
            segs.append(a["segmentation"])
    gt = np.asarray(rows, np.float64).reshape(-1, _lib.PLANE_GT_COLS).astype(np.float32)
    return dict(image_ids=image_ids, gt=gt, gt_off=np.asarray(gt_off, np.int32), npos=npos, names=names, thing_classes=thing_classes,
                segmentations=segs, image_hw=(H, W))


def decode_mask(seg: Dict, image_hw) -> np.ndarray:
    """One RLE (compressed string or uncompressed counts) -> [H,W] uint8, ValueError if its runs do not fill the image."""
    counts = seg["counts"]
    runs = rle._from_string(counts) if isinstance(counts, (str, bytes)) else [int(v) for v in counts]
    if any(r < 0 for r in runs) or sum(runs) != int(image_hw[0]) * int(image_hw[1]):
        raise ValueError(f"RLE runs sum to {sum(runs)}, not H*W = {int(image_hw[0]) * int(image_hw[1])}")
    return np.ascontiguousarray(rle.decode({"size": [int(image_hw[0]), int(image_hw[1])], "counts": runs}))  # (the runs are column-major)


class PlaneGroundTruth:
    """The annotations of a plane dataset as device tables (include/a3d.h, a3d_eval_mask_counts): images in the order of
    coco_dict["images"], `gt` [M,8] fp32 (box xyxy, plane, class), `gt_bits` [M, ceil(H*W/32)] int32 (the masks, bit-packed once by
    a3d_masks_pack_bits), `gt_off` [I+1].  `npos[c]` counts every annotation of contiguous class c.
    Footprint on the device: H*W/8 bytes of bits per annotation -- 38 KB at 480 x 640 (3.8 GB for 100 000 annotations) -- plus 32 bytes."""

    def __init__(self, image_ids, gt, gt_bits, gt_off, npos, names, thing_classes, device, image_hw=(480, 640)):
        from . import opt_ops

        self.image_ids = list(image_ids)
        self.index = {iid: i for i, iid in enumerate(self.image_ids)}
        self.gt_off = np.asarray(gt_off, np.int32)
        self.npos = np.asarray(npos, np.int32)
        self.names, self.thing_classes = list(names), list(thing_classes)
        self.image_hw = (int(image_hw[0]), int(image_hw[1]))
        self.device = torch.device(device)
        self.gt = torch.from_numpy(np.ascontiguousarray(gt, np.float32)).to(self.device)
        self.gt_bits = gt_bits
        self.gt_off_dev = torch.from_numpy(self.gt_off.copy()).to(self.device)
        if tuple(gt_bits.shape) != (self.gt.shape[0], opt_ops.words_per_mask(*self.image_hw)) or gt_bits.dtype != torch.int32:
            raise ValueError(f"gt_bits {tuple(gt_bits.shape)} {gt_bits.dtype}: want int32 [{self.gt.shape[0]},{opt_ops.words_per_mask(*self.image_hw)}]")

    def __len__(self):
        return len(self.image_ids)

    @classmethod
    def from_coco(cls, coco_dict: Dict, thing_classes: Optional[Sequence[str]] = None, device="cuda", image_hw=(480, 640)) -> "PlaneGroundTruth":
        """coco_dict: `images`, `categories` and `annotations`, each with bbox (xywh), category_id, plane (3 floats: normal * offset)
        and segmentation -- a COCO RLE dict, compressed string or uncompressed counts, of size image_hw.  Category ids map to
        contiguous ids in ascending order, as detectron2 does.  Every mask is decoded on the host (utils/rle.py), uploaded and packed
        ONCE, 256 at a time; afterwards an annotation costs 38 KB of device memory at 480 x 640.
        ValueError, naming the cause: polygon lists (convert to RLE), a mask size other than image_hw, a missing plane, more than 64
        annotations in an image.  The packing runs on the GPU: a cpu `device` is refused there (no CPU fallback)."""
        from . import opt_ops

        t = parse_plane_coco(coco_dict, thing_classes, image_hw)
        H, W = t["image_hw"]
        dev, M = torch.device(device), len(t["segmentations"])
        bits = torch.empty((M, opt_ops.words_per_mask(H, W)), device=dev, dtype=torch.int32)
        for at in range(0, M, _PACK_CHUNK):
            dense = np.stack([decode_mask(s, (H, W)) for s in t["segmentations"][at:at + _PACK_CHUNK]])
            bits[at:at + dense.shape[0]] = opt_ops.pack_masks(torch.from_numpy(dense).to(dev))
        return cls(t["image_ids"], t["gt"], bits, t["gt_off"], t["npos"], t["names"], t["thing_classes"], dev, (H, W))

    def rows_of(self, idx: Sequence[int]):
        """The tables of the images `idx` (indices into image_ids), in that order -> (gt, gt_bits, gt_off list).  Consecutive images
        are views; any other order is gathered on the device."""
        off = [0]
        for i in idx:
            off.append(off[-1] + int(self.gt_off[i + 1] - self.gt_off[i]))
        if all(b == a + 1 for a, b in zip(idx, idx[1:])):
            lo, hi = int(self.gt_off[idx[0]]), int(self.gt_off[idx[-1] + 1])
            return self.gt[lo:hi], self.gt_bits[lo:hi], off
        rows = np.concatenate([np.arange(self.gt_off[i], self.gt_off[i + 1], dtype=np.int64) for i in idx])
        rows = torch.from_numpy(rows).to(self.device)
        return self.gt[rows].contiguous(), self.gt_bits[rows].contiguous(), off


def record_slots(keep: torch.Tensor) -> torch.Tensor:
    """keep [B,R] (non-zero = the slot made a record) -> int32 [B*R]: the row of masks.reshape(B*R, H, W) of record k of image b, the
    k-th slot r with keep[b,r] != 0 (the mapping of evaluation.record_normals); -1 past the image's records.  Device work only."""
    B, R = keep.shape
    live = keep != 0
    order = torch.sort((~live).to(torch.int8), dim=1, stable=True)[1]  # the kept slots first, in slot order
    k = torch.arange(R, device=keep.device)
    slot = torch.where(k[None, :] < live.sum(1, keepdim=True), order + torch.arange(B, device=keep.device)[:, None] * R, torch.full_like(order, -1))
    return slot.reshape(-1).to(torch.int32).contiguous()


class PlaneEvaluator(_EvaluatorBase):
    """The reference's ScannetEvaluator protocol -- reset / process / evaluate -- over a PlaneGroundTruth.  process() and
    process_records() launch the mask comparison of their batch and queue device tensors (no host read of a detection); evaluate()
    reads the detection counts once."""

    def __init__(self, gt: PlaneGroundTruth, iou_thresh: float = 0.5, normal_threshold: float = 30.0, offset_threshold: float = 0.3):
        self.gt = gt
        self.iou_thresh, self.normal_threshold, self.offset_threshold = float(iou_thresh), float(normal_threshold), float(offset_threshold)
        self.reset()

    def reset(self):
        super().reset()
        self._counts = []  # per entry of _rows: int32 [n,3] or [B*R,3] -- gt_id, inter, uni of a3d_eval_mask_counts

    def _count_masks(self, idx, rows, det_off, masks, det_slot):
        from . import opt_ops

        H, W = self.gt.image_hw
        if masks.dim() != 3 or tuple(masks.shape[1:]) != (H, W):
            raise ValueError(f"masks {tuple(masks.shape)}: want [*,{H},{W}], the ground truth's image size")
        gt, bits, gt_off = self.gt.rows_of(idx)
        self._counts.append(torch.stack(opt_ops.eval_mask_counts(rows, det_off, gt, gt_off, masks, det_slot, bits), 1))

    @staticmethod
    def _as_u8(masks: torch.Tensor, dev) -> torch.Tensor:
        masks = masks.to(dev).contiguous()
        return masks.view(torch.uint8) if masks.dtype == torch.bool else masks.to(torch.uint8)

    def process(self, inputs: Sequence[Dict], outputs: Sequence[Dict]):
        """The reference's call shape (DatasetEvaluator.process): inputs[i]["image_id"]; outputs[i]["instances"] with pred_boxes,
        scores, pred_classes, pred_plane and pred_masks [n,H,W] (bool or uint8, non-zero = set).  pred_plane is evaluated as it is
        given: normal * offset.  The reference's evaluator refits that offset to the depth map itself (override_depth) before it
        evaluates; here the detector has done so in the records' plane columns (process_records), while the Instances of
        PlaneRCNN.forward carry the plane head's raw output -- put the plane to be scored into pred_plane.
        An outputs[i]["depth"] is scored against inputs[i]["depth"] where the input carries one."""
        if len(inputs) != len(outputs):
            raise ValueError(f"{len(inputs)} inputs for {len(outputs)} outputs")
        dev = self.gt.device
        for inp, outp in zip(inputs, outputs):
            if "image_id" not in inp:
                raise ValueError("an input without image_id")
            inst = outp.get("instances")
            n = 0
            if inst is not None:
                for f in ("pred_boxes", "scores", "pred_classes", "pred_plane", "pred_masks"):
                    if not inst.has(f):
                        raise ValueError(f"instances of image {inp['image_id']!r} lack {f}")
                n = len(inst)
                if inst.pred_masks.dim() != 3 or inst.pred_masks.shape[0] != n:
                    raise ValueError(f"pred_masks {tuple(inst.pred_masks.shape)} for {n} instances: want [n,H,W]")
            i = self._image_index(inp["image_id"])
            if n:
                cols = [inst.pred_boxes.tensor.reshape(n, 4), inst.scores.reshape(n, 1), inst.pred_classes.reshape(n, 1), inst.pred_plane.reshape(n, 3)]
                rows = torch.cat([c.to(dev, torch.float32) for c in cols] + [torch.zeros((n, 5), device=dev)], 1).contiguous()
                self._count_masks([i], rows, [0, n], self._as_u8(inst.pred_masks, dev), torch.arange(n, device=dev, dtype=torch.int32))
                self._rows.append(([i], rows, None))
            if "depth" in inp and outp.get("depth") is not None:
                self._score_depth([i], outp["depth"], inp["depth"])

    def process_records(self, image_ids: Sequence, records: torch.Tensor, rec_count: torch.Tensor, masks: torch.Tensor, keep: torch.Tensor,
                        depth=None, gt_depth=None):
        """A batch of PlaneRCNN.inference_batched(want_masks=True): records [B,R,F >= 14], rec_count [B], masks [B,R,H,W] uint8 and keep
        [B,R] as BatchedOutput carries them, on the device, without a host round trip.  Record k of image b is the k-th slot r with
        keep[b,r] != 0; its mask is masks[b,r].  depth / gt_depth: [B,H,W] maps, scored when both are given."""
        B = len(image_ids)
        if masks is None:
            raise ValueError("masks is None: run the detector with its masks materialised (inference_batched(want_masks=True))")
        if records.dim() != 3 or records.shape[0] != B or records.shape[2] < _lib.EVAL_DET_COLS or rec_count.numel() != B:
            raise ValueError(f"records {tuple(records.shape)} / rec_count {tuple(rec_count.shape)} for {B} image ids: want [B,R,>=14] and [B]")
        R = records.shape[1]
        if masks.dim() != 4 or tuple(masks.shape[:2]) != (B, R) or tuple(keep.shape) != (B, R):
            raise ValueError(f"masks {tuple(masks.shape)} / keep {tuple(keep.shape)}: want [B,R,H,W] and [B,R] = {(B, R)}")
        if (depth is None) != (gt_depth is None):
            raise ValueError("depth and gt_depth go together")
        dev = self.gt.device
        if tuple(masks.shape[2:]) != self.gt.image_hw:
            raise ValueError(f"masks {tuple(masks.shape)}: want [B,R,{self.gt.image_hw[0]},{self.gt.image_hw[1]}], the ground truth's image size")
        idx = [self._image_index(iid) for iid in image_ids]
        rows = records[:, :, :_lib.EVAL_DET_COLS].to(dev, torch.float32).clone()
        if B and R:
            m = self._as_u8(masks, dev)
            # every record slot is counted (the live count stays on the device); slots past an image's records have no mask
            self._count_masks(idx, rows.reshape(B * R, -1), [b * R for b in range(B + 1)], m.reshape(B * R, *m.shape[2:]), record_slots(keep.to(dev)))
        else:
            self._counts.append(torch.zeros((B * R, 3), device=dev, dtype=torch.int32))
        self._rows.append((idx, rows, rec_count.to(dev, torch.int32).clone()))
        if depth is not None:
            self._score_depth(idx, depth, gt_depth)

    # ------------------------------------------------------------------------------------------------------------------------------
    def evaluate(self) -> "OrderedDict[str, float]":
        """-> OrderedDict in the reference's order: the eight plane statistics (over the detections that have a ground truth; left out
        when there is none), per class with annotations the three APs "<metric> - <category name>", the three class means and, when
        depth was processed, depth_l1_dist.  Afterwards `detections` holds this process' per-detection arrays (gt_id, rank, box_iou,
        mask_iou, normal_err, offset_err, tp, inter, uni, det, det_off; in the order of the ground-truth table) and `table` the
        compact rows the result was computed from.  Under an initialised torch.distributed the compact rows are gathered, rank 0
        returns the result and every other rank {}."""
        import torch.distributed as dist

        from . import opt_ops

        gt, dev = self.gt, self.gt.device
        pick, det_off = self._pick()
        if len(pick):
            at = torch.from_numpy(pick).to(dev)
            det = torch.cat([rows.reshape(-1, _lib.EVAL_DET_COLS) for _, rows, _ in self._rows])[at].contiguous()
            cnt = torch.cat(self._counts)[at]
        else:
            det, cnt = torch.zeros((0, _lib.EVAL_DET_COLS), device=dev), torch.zeros((0, 3), device=dev, dtype=torch.int32)
        inter, uni = cnt[:, 1].contiguous(), cnt[:, 2].contiguous()
        m = opt_ops.eval_plane_match(det, det_off.tolist(), gt.gt, gt.gt_off.tolist(), inter, uni, iou_thresh=self.iou_thresh,
                                     normal_thresh=self.normal_threshold, offset_thresh=self.offset_threshold, gt_off_dev=gt.gt_off_dev)
        self.detections = dict(m, inter=inter, uni=uni, det=det, det_off=det_off)
        img = torch.repeat_interleave(torch.arange(len(gt), device=dev), torch.from_numpy(np.diff(det_off)).to(dev))
        has_gt = m["gt_id"] >= 0
        table = torch.cat([torch.stack([img.float(), m["rank"].float(), det[:, 4], det[:, 5], has_gt.float(), m["tp"].float()], 1),
                           _split64(torch.where(has_gt, m["normal_err"], 0.0)), _split64(torch.where(has_gt, m["offset_err"], 0.0))], 1)
        depth_rows = self._depth_rows()
        if dist.is_available() and dist.is_initialized():  # (a one-rank group takes this path too: it is the rig that exercises it)
            table, depth_rows = self._gather(table.contiguous(), depth_rows)
            if dist.get_rank() != 0:
                return OrderedDict()
        self.table = table
        C = len(gt.names)
        # (image, rank) order first: the statistics read the errors in it, then two stable sorts -- by score, descending, and by class
        key = table[:, 0].long() * (int(table[:, 1].max().item()) + 1 if len(table) else 1) + table[:, 1].long()
        table = table[torch.sort(key, stable=True)[1]]
        host = table.cpu().numpy()
        with_gt = host[:, 4] != 0
        res = plane_statistics(_join64(host[with_gt, 6:9]), _join64(host[with_gt, 9:12]))
        cls = table[:, 3].long()
        table = table[(cls >= 0) & (cls < C)]
        table = table[torch.sort(table[:, 2], descending=True, stable=True)[1]]
        table = table[torch.sort(table[:, 3], stable=True)[1]]
        seg = np.concatenate([[0], np.cumsum(np.bincount(table[:, 3].long().cpu().numpy(), minlength=C)[:C])])
        ap, n_entries = opt_ops.eval_ap(table[:, 5].to(torch.uint8).contiguous(), seg.tolist(), gt.npos.tolist())
        ap = ap.cpu().numpy()  # (row 3 belongs to a bit this evaluator never sets)
        self.n_entries = n_entries.cpu().numpy()
        keys = metric_keys(self.iou_thresh, self.normal_threshold, self.offset_threshold)
        sums, valid = [0.0, 0.0, 0.0], 0
        for c, name in enumerate(gt.names):
            if gt.npos[c] > 0:
                valid += 1
                for k, metric in enumerate(keys):
                    res[f"{metric} - {name}"] = float(ap[k, c])
                    sums[k] += float(ap[k, c])
        if valid:
            for k, metric in enumerate(keys):
                res[metric] = sums[k] / valid
        if len(depth_rows):
            res["depth_l1_dist"] = _depth_l1_dist(depth_rows)
        return res


def _split64(v: torch.Tensor) -> torch.Tensor:
    """float64 [n] -> [n,3] fp32 whose float64 sum (evaluation._join64) is v exactly: 24 + 24 + 5 bits, like _depth_rows' sums."""
    hi = v.float()
    mid = (v - hi.double()).float()
    lo = (v - hi.double() - mid.double()).float()
    return torch.stack([hi, mid, lo], 1)
