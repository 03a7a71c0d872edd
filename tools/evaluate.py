#!/usr/bin/env python3
"""Evaluate a checkpoint on an annotated dataset: the reference's `tools/train_net.py --eval-only` (ArtiEvaluator) -> the
articulation AP table and depth_l1_dist, printed and written to <output>/metrics.json.

    python tools/evaluate.py --config configs/planercnn_inference.yaml --weights model_final.pth \
        --annotations coco.json --image-root images/ [--batch 16] [--output out/]

`coco.json` has the shape the reference's convert_to_coco_dict writes: images (id, file_name), annotations (bbox xywh, category_id,
rot_axis, tran_axis, normal) and categories.  An image entry may carry `depth_file_name`, a 16-bit PNG in millimetres (or a .npy in
metres) under --image-root, which is then scored as depth_l1_dist.  Images are decoded with PIL, detected in batches by
PlaneRCNN.inference_batched and handed to ArtiEvaluator.process_records as packed records, without a host round trip.

`--evaluator planes` scores the plane stage instead (the reference's ScannetEvaluator -> evaluate_for_planes): box / mask / plane AP
per class, their means and the eight plane statistics.  Its annotations carry bbox, category_id, plane (normal * offset) and an RLE
segmentation of the images' size (`--image-hw`, default 480 640); the detector runs with its masks materialised and
PlaneEvaluator.process_records compares them on the device, batch by batch.
Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--weights", default=None, help="checkpoint (.pth); overrides MODEL.WEIGHTS")
    ap.add_argument("--annotations", required=True, help="COCO-style json with the articulation fields")
    ap.add_argument("--image-root", required=True)
    ap.add_argument("--batch", default=16, type=int, help="images per detector batch")
    ap.add_argument("--output", default=".", help="directory of metrics.json")
    ap.add_argument("--score-thresh", default=None, type=float, help="MODEL.ROI_HEADS.SCORE_THRESH_TEST (the reference evaluates at its config's value)")
    ap.add_argument("--filter-iou", default=0.7, type=float, help="arti only")
    ap.add_argument("--evaluator", default="arti", choices=("arti", "planes"), help="arti: articulation AP (ArtiEvaluator); planes: box / mask / plane AP (PlaneEvaluator)")
    ap.add_argument("--image-hw", default=(480, 640), type=int, nargs=2, metavar=("H", "W"), help="planes only: the size of the ground-truth masks")
    ap.add_argument("--random-init", action="store_true", help="no checkpoint: a seeded random initialisation (smoke runs)")
    ap.add_argument("opts", nargs=argparse.REMAINDER, default=[], help="KEY VALUE config overrides")
    return ap


def read_depth(path: str) -> np.ndarray:
    if path.endswith(".npy"):
        return np.load(path).astype(np.float32)
    from PIL import Image

    return np.asarray(Image.open(path)).astype(np.float32) / 1000.0


def format_table(res) -> str:
    w = max((len(k) for k in res), default=10)
    return "\n".join(f"| {k:<{w}} | {v:.4f} |" for k, v in res.items())


def main():
    args = build_parser().parse_args()
    from PIL import Image

    from articulation3d_amd.config import get_cfg, get_planercnn_cfg_defaults
    from articulation3d_amd.evaluation import ArtiEvaluator, ArtiGroundTruth, record_normals
    from articulation3d_amd.utils.arti_vis import DefaultPredictor

    cfg = get_cfg()
    get_planercnn_cfg_defaults(cfg)
    cfg.merge_from_file(args.config)
    if args.opts:
        cfg.merge_from_list(args.opts)
    if args.weights:
        cfg.MODEL.WEIGHTS = args.weights
    if args.score_thresh is not None:
        cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = args.score_thresh
    if not str(cfg.MODEL.DEVICE).startswith("cuda"):
        raise SystemExit(f"MODEL.DEVICE={cfg.MODEL.DEVICE!r}: evaluation runs on the GPU; there is no CPU fallback")
    if args.random_init:
        torch.manual_seed(2020)
    elif not cfg.MODEL.WEIGHTS:
        raise SystemExit("no checkpoint: pass --weights (or --random-init for a smoke run)")
    with open(args.annotations) as f:
        coco = json.load(f)
    model = DefaultPredictor(cfg, load_weights=not args.random_init).model
    dev = model.device
    planes = args.evaluator == "planes"
    if planes:
        from articulation3d_amd.evaluation_planes import PlaneEvaluator, PlaneGroundTruth

        gt = PlaneGroundTruth.from_coco(coco, device=dev, image_hw=tuple(args.image_hw))
        ev = PlaneEvaluator(gt)
    else:
        gt = ArtiGroundTruth.from_coco(coco, device=dev)
        ev = ArtiEvaluator(gt, filter_iou=args.filter_iou)
    images = coco["images"]
    for at in range(0, len(images), max(args.batch, 1)):
        chunk = images[at:at + max(args.batch, 1)]
        frames = np.stack([np.asarray(Image.open(os.path.join(args.image_root, im["file_name"])).convert("RGB")) for im in chunk])
        out = model.inference_batched(torch.from_numpy(frames).to(dev), want_masks=planes, source_rgb=True)
        depth = gt_depth = None
        if out.depth is not None and all("depth_file_name" in im for im in chunk):
            gt_depth = torch.from_numpy(np.stack([read_depth(os.path.join(args.image_root, im["depth_file_name"])) for im in chunk])).to(dev)
            depth = out.depth  # [B,H,W]
            if tuple(depth.shape) != tuple(gt_depth.shape):
                raise SystemExit(f"depth maps {tuple(gt_depth.shape)} do not match the detector's {tuple(depth.shape)}")
        if planes:
            ev.process_records([im["id"] for im in chunk], out.records, out.rec_count, out.masks, out.keep, depth, gt_depth)
        else:
            ev.process_records([im["id"] for im in chunk], out.records, out.rec_count, depth, gt_depth, normals=record_normals(out))
    res = ev.evaluate()
    print(format_table(res))
    os.makedirs(args.output, exist_ok=True)
    with open(os.path.join(args.output, "metrics.json"), "w") as f:
        json.dump(res, f, indent=1)
    n_det = int(ev.detections["det_off"][-1])
    matched = "with a ground truth" if planes else f"matched above IoU {args.filter_iou}"
    print(f"{len(images)} images, {n_det} detections, {int((ev.detections['gt_id'] >= 0).sum())} {matched} -> {os.path.join(args.output, 'metrics.json')}")


if __name__ == "__main__":
    main()
