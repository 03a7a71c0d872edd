"""Evaluate a checkpoint: the reference's articulation AP (ArtiEvaluator, pkg/evaluation/arti_evaluation.py:39-259 ->
evaluate_for_arti_axis :262-665 over pkg/utils/metrics.py and pkg/utils/VOCap.py) and its depth_l1_dist
(pkg/evaluation/scannet_evaluation.py:234-248), computed on the GPU.  Four VOC-style APs per class -- `bbox`, `bbox+axis`,
`bbox+normal`, `bbox+normal+axis` -- in which a detection is a true positive only if its box matches a ground-truth box and, where
the metric names them, its articulation axis is close to the ground truth's (EA score > 0.5) and its plane normal within 30 degrees.

The detections stay on the device as the rows the detector packs (csrc/pack.hip's record head).  `evaluate()` matches every detection
of every image processed so far in ONE launch (a3d_eval_match), sorts the valid ones by score with torch.sort and turns the sorted
true-positive bits into the AP table in ONE launch (a3d_eval_ap); depth maps are scored per batch by a3d_depth_l1.  The law of each
launch is stated in include/a3d.h and in numpy float64 by tests/eval_ref.py.

DEPARTURES from the reference, on purpose:
  * A detection is VALID iff the IoU with its best ground truth exceeds filter_iou.  The reference's `valid_pred_ids[idx] == 0`
    (arti_evaluation.py:456) tests a whole row of the IoU matrix, which is only well defined for one ground truth per image; this is
    that line for G == 1 and, for G > 1, the intent scannet_evaluation.py:332 shows.
  * The detection's OWN normal is compared.  The reference indexes pred_normals by rank (`pred_normals[pred_id]`, :479) where every
    other field goes through idx_sorted; the two agree when detections arrive sorted by score, as the detector hands them over.
  * The normal's dot product is clamped to [-1, 1].  The reference's acos returns NaN -- "not a true positive" -- for identical
    normals whose fp32 dot product rounds above 1.
  * The slope of a predicted axis line is k = -(cos / sin); the reference takes tan(-arctan(cos / sin)) through fp32, the same number
    up to rounding (it moves an end point by one pixel in about 1 of 20 000 random lines).  The line's first steps (offset * 100, the
    point on the line) are fp32 as in the reference; the boundary candidates, IoU, EA, the normal error and AP are float64, where the
    reference computes IoU, the normal and rec / prec / AP in fp32.
  * Boxes are compared as the detector produced them; the reference sends them through instances_to_coco_json (xyxy -> xywh in a JSON
    list) and back, which may move a coordinate by an ulp.
  * "Already covered" is decided as "the first qualifying detection per ground truth and metric, by rank": a ground truth is only ever
    covered by a true positive, so this equals the reference's sequential loop and runs in parallel.
  * Score ties: within an image detections are ranked by (score descending, index); the AP entries are sorted by score with a STABLE
    sort over (image index in the ground-truth table, rank).  The reference's torch.sort is unstable and follows the order images were
    processed in; here the result does not depend on how the images were batched, sharded or ordered.
  * Out of scope: COCO mAP (_eval_predictions), evaluate_for_recognition, dataset registration.  The mask IoU metrics of the plane
    stage (ScannetEvaluator -> evaluate_for_planes) are evaluation_planes.PlaneEvaluator, over the base class both share.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .structures import Boxes
from .utils.opt_utils import angle_offset_to_axis, axis_to_angle_offset

METRICS = ("bbox", "bbox+axis", "bbox+normal", "bbox+normal+axis")
KIND_ROT, KIND_TRAN = 0, 1
_NO_AXIS = [0, 0, 1, 1]  # what the reference's axis_to_angle_offset puts in a None axis' place (valid = 0)


def _kind_of(class_name: str) -> int:
    if "rot" in class_name:
        return KIND_ROT
    if "tran" in class_name:
        return KIND_TRAN
    raise ValueError(f"class {class_name!r} is neither a rotation ('rot') nor a translation ('tran') class")


def gt_axis_lines(axes: Sequence, boxes_xyxy: torch.Tensor, translation: bool, image_hw=(480, 640)):
    """Ground-truth axes (a list of [x1,y1,x2,y2] or None) -> (integer lines [G,4], valid [G]) the way the reference makes them
    (arti_evaluation.py:373-385): through (sin, cos, offset) about the box centre and back, the offset zeroed for a translation."""
    if len(axes) == 0:
        return np.zeros((0, 4), np.int32), np.zeros((0,), np.int32)
    centers = Boxes(boxes_xyxy).get_centers()
    ao = axis_to_angle_offset([_NO_AXIS if a is None else [float(v) for v in a] for a in axes], centers)
    if translation:
        ao[:, 2] = 0
    lines = angle_offset_to_axis(ao[:, :3], centers, int(image_hw[0]), int(image_hw[1]))
    return lines.numpy().astype(np.int32), np.array([0 if a is None else 1 for a in axes], np.int32)


class ArtiGroundTruth:
    """The annotations of a dataset as device tables (include/a3d.h, a3d_eval_match): images in the order of coco_dict["images"],
    `gt_f` [M,7] fp32 (box xyxy, raw normal), `gt_i` [M,12] int32 (class, kind, rotation line + valid, translation line + valid),
    `gt_off` [I+1].  `npos[c]` counts every annotation of contiguous class c; `names[c]` is its category name."""

    def __init__(self, image_ids, gt_f, gt_i, gt_off, npos, names, thing_classes, device, image_hw=(480, 640)):
        self.image_ids = list(image_ids)
        self.index = {iid: i for i, iid in enumerate(self.image_ids)}
        self.gt_off = np.asarray(gt_off, np.int32)
        self.npos = np.asarray(npos, np.int32)
        self.names, self.thing_classes = list(names), list(thing_classes)
        self.image_hw = (int(image_hw[0]), int(image_hw[1]))
        self.device = torch.device(device)
        self.gt_f = torch.from_numpy(np.ascontiguousarray(gt_f, np.float32)).to(self.device)
        self.gt_i = torch.from_numpy(np.ascontiguousarray(gt_i, np.int32)).to(self.device)
        self.gt_off_dev = torch.from_numpy(self.gt_off.copy()).to(self.device)

    def __len__(self):
        return len(self.image_ids)

    @classmethod
    def from_coco(cls, coco_dict: Dict, thing_classes: Optional[Sequence[str]] = None, device="cuda", image_hw=(480, 640)) -> "ArtiGroundTruth":
        """coco_dict: `images`, `annotations` (each with bbox xywh, category_id, rot_axis, tran_axis, normal) and `categories`, the
        shape the reference's convert_to_coco_dict writes.  Category ids map to contiguous ids in ascending order, as detectron2 does;
        thing_classes[c] (the category names when None) decides rot / tran."""
        cats = sorted(coco_dict["categories"], key=lambda c: c["id"])
        names = [c["name"] for c in cats]
        thing_classes = list(names if thing_classes is None else thing_classes)
        if len(thing_classes) != len(cats):
            raise ValueError(f"{len(thing_classes)} thing_classes for {len(cats)} categories")
        if not 1 <= len(cats) <= _lib.EVAL_MAX_CLASSES:
            raise ValueError(f"{len(cats)} categories: 1 .. {_lib.EVAL_MAX_CLASSES} are supported")
        kinds = [_kind_of(n) for n in thing_classes]
        contiguous = {c["id"]: i for i, c in enumerate(cats)}
        image_ids = [im["id"] for im in coco_dict["images"]]
        if len(set(image_ids)) != len(image_ids):
            raise ValueError("duplicate image ids")
        per_image = {iid: [] for iid in image_ids}
        npos = np.zeros(len(cats), np.int32)
        for ann in coco_dict["annotations"]:
            if ann["category_id"] not in contiguous:
                raise ValueError(f"annotation {ann.get('id')}: unknown category_id {ann['category_id']}")
            if ann["image_id"] not in per_image:
                raise ValueError(f"annotation {ann.get('id')}: unknown image_id {ann['image_id']}")
            per_image[ann["image_id"]].append(ann)
            npos[contiguous[ann["category_id"]]] += 1
        gt_f, gt_i, gt_off = [], [], [0]
        for iid in image_ids:
            anns = per_image[iid]
            if len(anns) > _lib.EVAL_MAX_GT:
                raise ValueError(f"image {iid}: {len(anns)} annotations, at most {_lib.EVAL_MAX_GT} are supported")
            gt_off.append(gt_off[-1] + len(anns))
            if not anns:
                continue
            xywh = np.array([a["bbox"] for a in anns], np.float64).reshape(-1, 4)
            xyxy = xywh.copy()
            xyxy[:, 2:] += xyxy[:, :2]
            boxes = torch.as_tensor(xyxy, dtype=torch.float32)
            rot, rot_ok = gt_axis_lines([a.get("rot_axis") for a in anns], boxes, False, image_hw)
            tran, tran_ok = gt_axis_lines([a.get("tran_axis") for a in anns], boxes, True, image_hw)
            normals = np.array([[-1, -1, -1] if a.get("normal") is None else a["normal"] for a in anns], np.float32).reshape(-1, 3)
            gt_f.append(np.concatenate([boxes.numpy(), normals], 1))
            c = np.array([contiguous[a["category_id"]] for a in anns], np.int32)
            k = np.array([kinds[v] for v in c], np.int32)
            gt_i.append(np.concatenate([c[:, None], k[:, None], rot, rot_ok[:, None], tran, tran_ok[:, None]], 1))
        gt_f = np.concatenate(gt_f) if gt_f else np.zeros((0, _lib.EVAL_GT_FCOLS), np.float32)
        gt_i = np.concatenate(gt_i) if gt_i else np.zeros((0, _lib.EVAL_GT_ICOLS), np.int32)
        return cls(image_ids, gt_f, gt_i, gt_off, npos, names, thing_classes, device, image_hw)


def record_normals(out) -> torch.Tensor:
    """The plane head's raw output per record slot, [B,R,3], from a BatchedOutput of PlaneRCNN.inference_batched: record k of frame b
    is the k-th kept detection of the frame (csrc/pack.hip), its head row is det.row_offset[b] + r.  Device work only."""
    det = out.det
    B, R = out.keep.shape
    dev = out.keep.device
    if not det.total or det.pred_plane is None:
        return torch.zeros((B, R, 3), device=dev)
    r = torch.arange(R, device=dev)
    live = (r[None, :] < det.count[:B, None]) & (out.keep != 0)
    rows = (det.row_offset[:B, None].long() + r[None, :]).clamp_(max=det.pred_plane.shape[0] - 1)
    vals = det.pred_plane[rows].float()
    dst = torch.where(live, live.long().cumsum(1) - 1, torch.full_like(rows, R))  # dead slots land in a spare row
    ext = torch.zeros((B, R + 1, 3), device=dev)
    ext.scatter_(1, dst[..., None].expand(B, R, 3), vals)
    return ext[:, :R].contiguous()


class _EvaluatorBase:
    """What ArtiEvaluator and evaluation_planes.PlaneEvaluator share: the image bookkeeping, the queue of detection rows and its
    collection in the order of the ground-truth table, the depth rows and the gather.  `self.gt` carries index, device and __len__."""

    def reset(self):
        self._seen = set()
        self._rows: List = []    # (image indices, rows [n,14] or [B,R,14], counts [B] int32 on the device or None)
        self._depth: List = []   # (image indices, sums [B] float64, counts [B] int32)
        self.detections = None   # evaluate(): this process' per-detection arrays
        self.table = None        # evaluate(): the compact per-detection table AP was computed from (rank 0 under torch.distributed)

    def _image_index(self, image_id) -> int:
        if image_id not in self.gt.index:
            raise ValueError(f"image_id {image_id!r} is not in the ground truth")
        i = self.gt.index[image_id]
        if i in self._seen:
            raise ValueError(f"image_id {image_id!r} was processed before (reset() starts a new evaluation)")
        self._seen.add(i)
        return i

    def _score_depth(self, idx: List[int], pred, gt_depth):
        from . import opt_ops

        dev = self.gt.device
        pred = torch.as_tensor(pred).to(dev, torch.float32)
        gt_depth = torch.as_tensor(gt_depth).to(dev, torch.float32)
        pred, gt_depth = pred.reshape(-1, *pred.shape[-2:]).contiguous(), gt_depth.reshape(-1, *gt_depth.shape[-2:]).contiguous()
        if pred.shape != gt_depth.shape or pred.shape[0] != len(idx):
            raise ValueError(f"depth {tuple(pred.shape)} / ground-truth depth {tuple(gt_depth.shape)} for {len(idx)} images")
        self._depth.append((list(idx), *opt_ops.depth_l1(pred, gt_depth)))

    # ------------------------------------------------------------------------------------------------------------------------------
    def _pick(self):
        """-> (pick: for every detection, in the order of the ground-truth table, its row in the queue's flattened rows -- int64
        numpy --, det_off [I+1] numpy): the one host read of the counts."""
        I = len(self.gt)
        counted = [c for _, _, c in self._rows if c is not None]
        counts = torch.cat(counted).tolist() if counted else []
        per_image, base, k = {}, 0, 0
        for idx, rows, c in self._rows:
            if c is None:
                per_image[idx[0]] = (base, rows.shape[0])
                base += rows.shape[0]
            else:
                R = rows.shape[1]
                for b, i in enumerate(idx):
                    per_image[i] = (base + b * R, min(max(int(counts[k + b]), 0), R))
                k += len(idx)
                base += rows.shape[0] * R
        det_off = np.zeros(I + 1, np.int64)
        pick = []
        for i in range(I):
            b, n = per_image.get(i, (0, 0))
            det_off[i + 1] = det_off[i] + n
            pick.append(np.arange(b, b + n, dtype=np.int64))
        return (np.concatenate(pick) if pick else np.zeros(0, np.int64)), det_off

    def _collect(self):
        """-> (det [N,14] in the order of the ground-truth table, det_off [I+1] numpy)."""
        dev = self.gt.device
        pick, det_off = self._pick()
        if len(pick) == 0:
            return torch.zeros((0, _lib.EVAL_DET_COLS), device=dev), det_off
        flats = [rows.reshape(-1, _lib.EVAL_DET_COLS) for _, rows, _ in self._rows]
        return torch.cat(flats)[torch.from_numpy(pick).to(dev)].contiguous(), det_off

    def _gather(self, table: torch.Tensor, depth_rows: torch.Tensor):
        """Under an initialised torch.distributed: every rank's compact rows to every rank through parallel.gather_records (counts,
        then the live rows only).  The rows are fp32: image index, rank, score, class, valid, tp -- all exact in fp32 -- and the depth
        rows of _depth_rows, which carry their float64 sums exactly."""
        import torch.distributed as dist

        from . import parallel

        out = []
        for rows in (table, depth_rows):
            n = torch.tensor([rows.shape[0]], device="cpu" if dist.get_backend() == "gloo" else rows.device, dtype=torch.int64)
            dist.all_reduce(n, op=dist.ReduceOp.MAX)  # one common slot count: gather_records clamps every rank's count to the local one
            R = max(int(n.item()), 1)
            block = rows.new_zeros((1, R, rows.shape[1]))
            block[0, :rows.shape[0]] = rows
            got, _cnt = parallel.gather_records_async(block, torch.tensor([rows.shape[0]], device=rows.device, dtype=torch.int32), rows=1).wait_compact()
            out.append(got)
        return out

    def _depth_rows(self) -> torch.Tensor:
        """[n,6] fp32: image index, the float64 sum as three fp32 terms (exact: 24 + 24 + 5 bits), the count as two 16-bit halves."""
        dev = self.gt.device
        if not self._depth:
            return torch.zeros((0, 6), device=dev)
        idx = torch.tensor([i for ids, _, _ in self._depth for i in ids], device=dev, dtype=torch.float32)
        s = torch.cat([s for _, s, _ in self._depth])
        c = torch.cat([c for _, _, c in self._depth]).long()
        hi = s.float()
        mid = (s - hi.double()).float()
        lo = (s - hi.double() - mid.double()).float()
        return torch.stack([idx, hi, mid, lo, (c >> 16).float(), (c & 0xFFFF).float()], 1)


def _depth_l1_dist(depth_rows: torch.Tensor) -> float:
    """depth_l1_dist from the (gathered) rows of _depth_rows: the mean over images, in image order, of sum / max(count, 1)."""
    d = depth_rows.cpu().numpy()
    order = np.argsort(d[:, 0], kind="stable")
    sums = _join64(d[order, 1:4])
    cnts = d[order, 4].astype(np.float64) * 65536.0 + d[order, 5].astype(np.float64)
    return float(np.mean(sums / np.maximum(cnts, 1.0)))


class ArtiEvaluator(_EvaluatorBase):
    """The reference's ArtiEvaluator protocol -- reset / process / evaluate -- over an ArtiGroundTruth.  process() and
    process_records() only queue device tensors (no host read of a detection); evaluate() reads the detection counts once."""

    def __init__(self, gt: ArtiGroundTruth, filter_iou: float = 0.7, iou_thresh: float = 0.5, normal_threshold: float = 30.0):
        self.gt = gt
        self.filter_iou, self.iou_thresh, self.normal_threshold = float(filter_iou), float(iou_thresh), float(normal_threshold)
        self.reset()

    def process(self, inputs: Sequence[Dict], outputs: Sequence[Dict]):
        """The reference's call shape (DatasetEvaluator.process): inputs[i]["image_id"]; outputs[i]["instances"] with pred_boxes,
        scores, pred_classes, pred_plane, pred_rot_axis, pred_tran_axis -- what PlaneRCNN.forward returns in eval mode.  An
        outputs[i]["depth"] is scored against inputs[i]["depth"] where the input carries one."""
        if len(inputs) != len(outputs):
            raise ValueError(f"{len(inputs)} inputs for {len(outputs)} outputs")
        dev = self.gt.device
        for inp, outp in zip(inputs, outputs):
            if "image_id" not in inp:
                raise ValueError("an input without image_id")
            inst = outp.get("instances")
            if inst is not None:
                for f in ("pred_boxes", "scores", "pred_classes", "pred_plane", "pred_rot_axis", "pred_tran_axis"):
                    if not inst.has(f):
                        raise ValueError(f"instances of image {inp['image_id']!r} lack {f}")
                n = len(inst)
                cols = [inst.pred_boxes.tensor.reshape(n, 4), inst.scores.reshape(n, 1), inst.pred_classes.reshape(n, 1), inst.pred_plane.reshape(n, 3),
                        inst.pred_rot_axis.reshape(n, 3), inst.pred_tran_axis.reshape(n, 2)]
            i = self._image_index(inp["image_id"])
            if inst is not None and n:
                self._rows.append(([i], torch.cat([c.to(dev, torch.float32) for c in cols], 1).contiguous(), None))
            if "depth" in inp and outp.get("depth") is not None:
                self._score_depth([i], outp["depth"], inp["depth"])

    def process_records(self, image_ids: Sequence, records: torch.Tensor, rec_count: torch.Tensor, depth=None, gt_depth=None, *, normals=None):
        """A batch of PlaneRCNN.inference_batched: records [B,R,F >= 14] and rec_count [B] as BatchedOutput carries them, on the device,
        without a host round trip.  depth / gt_depth: [B,H,W] maps, scored when both are given.

        The plane columns of a record are normal * the offset fitted to the depth map (csrc/heads_post.hip: the mean of n . ray * depth
        over the mask), and that offset CAN be negative, which negates the normal.  So the records alone do not carry the normal the
        reference evaluates: pass `normals=record_normals(out)` (the plane head's own output per record slot, [B,R,3]) and it replaces
        those columns.  Without `normals` the records' plane columns are used as they are."""
        B = len(image_ids)
        if records.dim() != 3 or records.shape[0] != B or records.shape[2] < _lib.EVAL_DET_COLS or rec_count.numel() != B:
            raise ValueError(f"records {tuple(records.shape)} / rec_count {tuple(rec_count.shape)} for {B} image ids: want [B,R,>=14] and [B]")
        if normals is not None and tuple(normals.shape) != (B, records.shape[1], 3):
            raise ValueError(f"normals {tuple(normals.shape)}: want [B,R,3] = {(B, records.shape[1], 3)}")
        if (depth is None) != (gt_depth is None):
            raise ValueError("depth and gt_depth go together")
        idx = [self._image_index(iid) for iid in image_ids]
        dev = self.gt.device
        rows = records[:, :, :_lib.EVAL_DET_COLS].to(dev, torch.float32).clone()
        if normals is not None:
            rows[:, :, 6:9] = normals.to(dev, torch.float32)
        self._rows.append((idx, rows, rec_count.to(dev, torch.int32).clone()))
        if depth is not None:
            self._score_depth(idx, depth, gt_depth)

    def evaluate(self) -> "OrderedDict[str, float]":
        """-> OrderedDict of "<metric> - <category name>" (classes with annotations only, as the reference logs them) and, when depth
        was processed, depth_l1_dist.  Afterwards `detections` holds this process' per-detection arrays (gt_id, iou, ea, normal_err,
        rank, tp, det, det_off; in the order of the ground-truth table) and `table` the compact rows AP was computed from.  Under an
        initialised torch.distributed the compact rows are gathered, rank 0 returns the result and every other rank {}."""
        import torch.distributed as dist

        from . import opt_ops

        gt, dev = self.gt, self.gt.device
        det, det_off = self._collect()
        m = opt_ops.eval_match(det, det_off.tolist(), gt.gt_f, gt.gt_i, gt.gt_off.tolist(), filter_iou=self.filter_iou, iou_thresh=self.iou_thresh,
                               normal_thresh=self.normal_threshold, img_hw=gt.image_hw, gt_off_dev=gt.gt_off_dev)
        self.detections = dict(m, det=det, det_off=det_off)
        img = torch.repeat_interleave(torch.arange(len(gt), device=dev), torch.from_numpy(np.diff(det_off)).to(dev))
        valid = m["gt_id"] >= 0
        table = torch.stack([img.float(), m["rank"].float(), det[:, 4], det[:, 5], valid.float(), m["tp"].float()], 1)[valid]
        depth_rows = self._depth_rows()
        if dist.is_available() and dist.is_initialized():  # (a one-rank group takes this path too: it is the rig that exercises it)
            table, depth_rows = self._gather(table.contiguous(), depth_rows)
            if dist.get_rank() != 0:
                return OrderedDict()
        self.table = table
        res = OrderedDict()
        C = len(gt.names)
        cls = table[:, 3].long()
        table = table[(cls >= 0) & (cls < C)]
        # (image, rank) order first, then two stable sorts: by score, descending, and by class
        key = table[:, 0].long() * (int(table[:, 1].max().item()) + 1 if len(table) else 1) + table[:, 1].long()
        table = table[torch.sort(key, stable=True)[1]]
        table = table[torch.sort(table[:, 2], descending=True, stable=True)[1]]
        table = table[torch.sort(table[:, 3], stable=True)[1]]
        seg = np.concatenate([[0], np.cumsum(np.bincount(table[:, 3].long().cpu().numpy(), minlength=C)[:C])])
        ap, n_entries = opt_ops.eval_ap(table[:, 5].to(torch.uint8).contiguous(), seg.tolist(), gt.npos.tolist())
        ap = ap.cpu().numpy()
        self.n_entries = n_entries.cpu().numpy()
        for c, name in enumerate(gt.names):
            if gt.npos[c] > 0:
                for k, metric in enumerate(METRICS):
                    res[f"{metric} - {name}"] = float(ap[k, c])
        if len(depth_rows):
            res["depth_l1_dist"] = _depth_l1_dist(depth_rows)
        return res


def _join64(parts: np.ndarray) -> np.ndarray:
    """The float64 a _depth_rows triple stands for."""
    p = parts.astype(np.float64)
    return (p[:, 0] + p[:, 1]) + p[:, 2]
