#!/usr/bin/env python
"""Writes tests/golden/plane_eval.json: a seeded synthetic plane dataset of small images and what the REFERENCE's own
evaluate_for_planes (pkg/evaluation/scannet_evaluation.py:254) returns for it.  Runs where a checkout of the reference is at hand
(--reference); no test reads the reference, only the JSON travels.

The reference's modules import detectron2, pycocotools and fvcore at module scope; none of them is installed here.  They are stood in
for the way tools/make_eval_golden.py does it (its stand-ins are reused); pycocotools.mask.iou is float64 inter / union on the masks
utils/rle.py decodes, which is what pycocotools computes.

The dataset stays inside the region where the reference is well defined (articulation3d_amd/evaluation_planes.py lists why) and where
its fp32 arithmetic cannot decide differently from the float64 law; check_conditions asserts all of it with tests/plane_eval_ref.py,
and main() walks seeds until one dataset holds every condition -- a dataset is taken or left whole, no case is dropped from it.
For the four mean / median statistics the file also records the gap between the reference's value (fp32 compare_planes) and the numpy
law's, both computed here.

    python tools/make_plane_eval_golden.py --reference /path/to/articulation3d [--out tests/golden/plane_eval.json]
"""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CATEGORIES = [{"id": 1, "name": "plane"}, {"id": 3, "name": "door"}, {"id": 7, "name": "spare"}]  # (no annotation of `spare`)
THING_CLASSES = [c["name"] for c in CATEGORIES]
N_IMAGES, FIRST_SEED = 14, 20240901
H, W = 48, 64
IOU, NORMAL, OFFSET = 0.5, 30.0, 0.3
GAP_KEYS = ("mean_normal", "median_normal", "mean_offset", "median_offset")


def _q(v):
    """Multiples of 1/4 pixel: the reference's xyxy -> xywh -> xyxy trip is exact."""
    return np.round(np.asarray(v, np.float64) * 4) / 4


def _f32(v):
    return [float(np.float32(x)) for x in np.asarray(v).ravel()]


def _blob(rng, box, bite):
    """A mask inside `box` (xyxy): its rectangle with a corner of relative size `bite` cut away."""
    from articulation3d_amd.utils import rle

    m = np.zeros((H, W), np.uint8)
    x1, y1, x2, y2 = (int(round(v)) for v in box)
    x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, W), min(y2, H)
    m[y1:y2, x1:x2] = 1
    bw, bh = int((x2 - x1) * bite), int((y2 - y1) * bite)
    if bw and bh:
        if rng.uniform() < 0.5:
            m[y1:y1 + bh, x1:x1 + bw] = 0
        else:
            m[y2 - bh:y2, x2 - bw:x2] = 0
    if m.sum() == 0:
        m[min(max(y1, 0), H - 1), min(max(x1, 0), W - 1)] = 1  # (never an empty mask: pycocotools divides 0 by 0 for two of them)
    return rle.encode(m)


def make_dataset(seed):
    """-> (coco dict, predictions: per image {image_id, boxes xyxy, scores, classes, plane, masks (RLE)} as lists)."""
    rng = np.random.default_rng(seed)
    images, anns, preds = [], [], []
    all_scores = np.sort(rng.uniform(0.05, 1.0, 40 * N_IMAGES))[::-1]
    taken = 0
    for i in range(N_IMAGES):
        iid = 500 + 7 * i
        images.append({"id": iid, "file_name": f"{iid}.png", "height": H, "width": W})
        G = int(rng.integers(1, 5))
        gts = []
        for _ in range(G):
            w, h = _q(rng.uniform(12, 30)), _q(rng.uniform(10, 24))
            x, y = _q(rng.uniform(0, W - w)), _q(rng.uniform(0, H - h))
            n = rng.normal(size=3)
            plane = n / np.linalg.norm(n) * rng.uniform(0.6, 4.0)
            cat = 1 if rng.uniform() < 0.6 else 3
            box = np.array([x, y, x + w, y + h])
            gts.append((box, plane, cat))
            anns.append({"id": len(anns) + 1, "image_id": iid, "category_id": cat, "bbox": [float(x), float(y), float(w), float(h)],
                         "plane": _f32(plane), "segmentation": _blob(rng, box, rng.choice([0.0, 0.3, 0.5])), "iscrowd": 0})
        D = int(rng.integers(0, 9))
        scores = np.sort(rng.choice(all_scores[taken:taken + 40], D, replace=False))[::-1]  # (disjoint ranges: distinct over the dataset)
        taken += 40
        rec = {"image_id": iid, "boxes": [], "scores": _f32(scores), "classes": [], "plane": [], "masks": []}
        for _ in range(D):
            box, plane, cat = gts[int(rng.integers(0, G))]
            b = _q(box + rng.uniform(-1, 1, 4) * rng.choice([1.0, 4.0, 9.0]))
            b[2:] = np.maximum(b[2:], b[:2] + 2)
            mbox = box + rng.uniform(-1, 1, 4) * rng.choice([1.0, 4.0, 9.0])  # the mask moves on its own: mask and box verdicts differ
            rec["boxes"].append(b.tolist())
            rec["classes"].append({1: 0, 3: 1}[cat] if rng.uniform() < 0.85 else int(rng.integers(0, 2)))
            p = plane + rng.normal(size=3) * rng.choice([0.03, 0.25, 1.0])
            rec["plane"].append(_f32(p * rng.choice([1.0, 1.0, 1.15, -1.0])))  # (a negative refitted offset flips the normal)
            rec["masks"].append(_blob(rng, mbox, rng.choice([0.0, 0.3, 0.5])))
        preds.append(rec)
    return {"images": images, "annotations": anns, "categories": CATEGORIES}, preds


def law(coco, preds):
    import plane_eval_ref as P

    fx = {"coco": coco, "predictions": preds, "image_hw": [H, W]}
    images, npos, names = P.fixture_images(fx)
    res, matches, entries = P.evaluate(images, npos, names, IOU, NORMAL, OFFSET)
    return images, res, matches, entries


def check_conditions(coco, preds):
    """The conditions the fixture is recorded under, all of them, with the numpy law.  AssertionError names the first that fails."""
    from eval_ref import box_iou

    images, _res, matches, _ = law(coco, preds)
    scores = [s for p in preds for s in np.asarray(p["scores"], np.float32).tolist()]
    assert len(set(scores)) == len(scores), "scores must be distinct over the dataset"
    claimed = [0, 0, 0]
    mask_not_box = box_not_mask = 0
    for im, m in zip(images, matches):
        assert len(im["gt"]) >= 1, "every image has a ground truth"
        s = im["det"][:, 4]
        assert (np.diff(s) < 0).all(), "scores descend within an image"
        for d in range(len(im["det"])):
            ious = np.array([box_iou(im["det"][d, :4], g[:4]) for g in im["gt"]])
            assert (np.abs(ious - 0.5) >= 1e-3).all(), "a box IoU within 1e-3 of 0.5"
            top = np.sort(ious)[::-1]
            assert len(top) < 2 or top[0] - top[1] >= 1e-3, "the best box IoU is not 1e-3 above the runner-up"
            assert m["uni"][d] > 0 and 2 * int(m["inter"][d]) != int(m["uni"][d]), "a mask IoU of exactly 0.5 (or two empty masks)"
        assert (np.abs(m["normal_err"] - 10) >= 1e-2).all() and (np.abs(m["normal_err"] - 30) >= 1e-2).all(), "a normal error within 1e-2 of 10 / 30"
        assert (np.abs(m["offset_err"] - 0.3) >= 1e-4).all() and (np.abs(m["offset_err"] - 0.5) >= 1e-4).all(), "an offset error within 1e-4 of 0.3 / 0.5"
        for k in range(3):
            q = (m["qual"] >> k) & 1
            claimed[k] += int(any(np.sum((m["gt_id"] == g) & (q == 1)) >= 2 for g in range(len(im["gt"]))))
        mask_not_box += int(np.sum(((m["tp"] & 2) != 0) & ((m["tp"] & 1) == 0)))
        box_not_mask += int(np.sum(((m["tp"] & 1) != 0) & ((m["tp"] & 2) == 0)))
    assert all(claimed), f"a ground truth claimed by two qualifying detections, per metric: {claimed}"
    assert mask_not_box and box_not_mask, "a mask true positive that is a box false positive, and the other way round"


class _Dataset:
    """The calls evaluate_for_planes makes on a pycocotools COCO object."""

    def __init__(self, coco):
        self.dataset = coco

    def getCatIds(self):
        return [c["id"] for c in self.dataset["categories"]]

    def getAnnIds(self, imgIds):
        return [a["id"] for a in self.dataset["annotations"] if a["image_id"] in imgIds]

    def loadAnns(self, ids):
        return [a for a in self.dataset["annotations"] if a["id"] in ids]

    def loadCats(self, ids):
        return [c for c in self.dataset["categories"] if c["id"] in ids]

    def loadImgs(self, ids):
        return [im for im in self.dataset["images"] if im["id"] in ids]


def _mask_iou(dt, gt, iscrowd):
    """pycocotools.mask.iou for RLE lists without crowd regions: float64 inter / union, [len(dt), len(gt)]."""
    from articulation3d_amd.utils import rle

    assert not any(iscrowd)
    a, b = [rle.decode(r).astype(bool) for r in dt], [rle.decode(r).astype(bool) for r in gt]
    out = np.zeros((len(a), len(b)), np.float64)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i, j] = np.float64((x & y).sum()) / np.float64((x | y).sum())
    return out


def run_reference(ref_root, coco, preds):
    import make_eval_golden as G

    ref_pkg = os.path.join(ref_root, "articulation3d")
    G._install_stand_ins(ref_pkg)
    for name in ("scipy", "scipy.special", "sklearn", "sklearn.metrics"):  # imported at module scope, never called by evaluate_for_planes
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = G._Mod(name)
    sys.modules["pycocotools.mask"].iou = _mask_iou
    sys.modules["pycocotools"].mask = sys.modules["pycocotools.mask"]  # (`import a.b as x` walks the attribute)
    sys.modules["detectron2.structures"].PolygonMasks = type("PolygonMasks", (), {})
    mod = G._load(os.path.join(ref_pkg, "evaluation", "scannet_evaluation.py"), "articulation3d.evaluation.scannet_evaluation")
    metadata = types.SimpleNamespace(thing_classes=THING_CLASSES, thing_dataset_id_to_contiguous_id={c["id"]: k for k, c in enumerate(CATEGORIES)})
    predictions = []
    for p in preds:
        b = np.asarray(p["boxes"], np.float64).reshape(-1, 4)
        inst = [{"score": s, "bbox": [x1, y1, x2 - x1, y2 - y1], "category_id": c, "segmentation": m}
                for (x1, y1, x2, y2), s, c, m in zip(b.tolist(), p["scores"], p["classes"], p["masks"])]
        predictions.append({"image_id": p["image_id"], "instances": inst, "pred_plane": np.asarray(p["plane"], np.float32).reshape(-1, 3)})
    res = mod.evaluate_for_planes(predictions, _Dataset(coco), metadata, 0.7, iou_thresh=IOU, normal_threshold=NORMAL, offset_threshold=OFFSET)
    return {k: float(v) for k, v in res.items()}  # (a dict keeps the reference's key order, in Python and in JSON)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds articulation3d/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "plane_eval.json"))
    args = ap.parse_args()
    for seed in range(FIRST_SEED, FIRST_SEED + 400):
        coco, preds = make_dataset(seed)
        try:
            check_conditions(coco, preds)
            break
        except AssertionError as e:
            print(f"seed {seed}: {e}")
    else:
        raise SystemExit("no seed holds every condition")
    metrics = run_reference(args.reference, coco, preds)
    _, res, _, _ = law(coco, preds)
    assert list(metrics) == list(res), (list(metrics), list(res))
    gap = {k: abs(metrics[k] - res[k]) for k in GAP_KEYS}
    with open(args.out, "w") as f:
        json.dump({"thing_classes": THING_CLASSES, "image_hw": [H, W], "seed": seed, "iou_thresh": IOU, "normal_threshold": NORMAL,
                   "offset_threshold": OFFSET, "coco": coco, "predictions": preds, "metrics": metrics, "stat_gap": gap},
                  f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(json.dumps(metrics, indent=1))
    print("gap", gap)
    print(f"seed {seed}: wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
