#!/usr/bin/env python
"""Writes tests/golden/arti_eval.json: a seeded synthetic dataset and what the REFERENCE's own evaluate_for_arti_axis
(pkg/evaluation/arti_evaluation.py:262) returns for it.  Runs where a checkout of the reference is at hand (--reference); no test
reads the reference, only the JSON travels.

The reference's modules import detectron2, pycocotools and fvcore at module scope; none of them is installed here.  They are stood in
for the way oracle/make_golden.py does it: Boxes / pairwise_iou of this package back detectron2.structures, everything the function
never calls is an inert placeholder.

The dataset stays inside the region where the reference is well defined (articulation3d_amd/evaluation.py lists why): one ground
truth per image, detections sorted by score, no duplicate scores, no identical normals.  Coordinates are multiples of 1/4 pixel, so the
reference's xyxy -> xywh -> xyxy trip is exact.  Every decision keeps a margin (asserted below with tests/eval_ref.py) that the
reference's fp32 arithmetic cannot cross.

    python tools/make_eval_golden.py --reference /path/to/articulation3d [--out tests/golden/arti_eval.json]
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

THING_CLASSES = ["arti_rot", "arti_tran"]
CATEGORIES = [{"id": 1, "name": "arti_rot"}, {"id": 2, "name": "arti_tran"}]
N_IMAGES, SEED = 40, 20240607
H, W = 480, 640


class _Inert:
    def __getattr__(self, k):
        return _Inert()

    def __call__(self, *a, **k):
        raise NotImplementedError("placeholder for a third-party name evaluate_for_arti_axis never uses")


class _Mod(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _Inert()


class _BoxMode:
    XYWH_ABS, XYXY_ABS = "xywh", "xyxy"

    @staticmethod
    def convert(box, from_mode, to_mode):
        assert (from_mode, to_mode) == ("xywh", "xyxy")
        out = np.array(box, dtype=np.float64).reshape(-1, 4)
        out[:, 2:] += out[:, :2]
        return out


def _install_stand_ins(ref_pkg: str):
    from articulation3d_amd.structures import Boxes, pairwise_iou

    for name in ("detectron2", "detectron2.utils", "detectron2.utils.comm", "detectron2.utils.logger", "detectron2.data",
                 "detectron2.data.detection_utils", "detectron2.data.transforms", "detectron2.evaluation",
                 "detectron2.evaluation.coco_evaluation", "detectron2.structures", "pycocotools", "pycocotools.mask", "pycocotools.coco",
                 "fvcore", "fvcore.common", "fvcore.common.file_io", "cv2", "articulation3d", "articulation3d.evaluation",
                 "articulation3d.evaluation.detectron2coco", "articulation3d.utils", "articulation3d.data"):
        if name not in sys.modules:
            m = _Mod(name)
            m.__path__ = []
            sys.modules[name] = m
    for name in ("utils", "data", "structures", "evaluation"):
        setattr(sys.modules["detectron2"], name, sys.modules["detectron2." + name])
    sys.modules["detectron2.evaluation"].COCOEvaluator = type("COCOEvaluator", (), {})
    st = sys.modules["detectron2.structures"]
    st.Boxes, st.pairwise_iou, st.BoxMode = Boxes, pairwise_iou, _BoxMode
    lg = sys.modules["detectron2.utils.logger"]
    lg.setup_logger = lambda *a, **k: None
    lg.create_small_table = lambda d: str(dict(d))
    # the reference's own utils / data modules load from their files, without the packages' __init__ (which pull in everything)
    sys.modules["articulation3d.utils"].__path__ = [os.path.join(ref_pkg, "utils")]
    sys.modules["articulation3d.data"].__path__ = [os.path.join(ref_pkg, "data")]
    for name in ("utils", "data", "evaluation"):  # (`import a.b.c as x` walks the attributes: they must be the modules, not placeholders)
        setattr(sys.modules["articulation3d"], name, sys.modules["articulation3d." + name])


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


class _Dataset:
    """The five calls evaluate_for_arti_axis makes on a pycocotools COCO object."""

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


def _q(v):
    """Multiples of 1/4 pixel."""
    return np.round(np.asarray(v, np.float64) * 4) / 4


def _f32(v):
    return [float(np.float32(x)) for x in np.asarray(v).ravel()]


def make_dataset():
    """-> (coco dict, predictions: per image {image_id, boxes xyxy, scores, classes, plane, rot_axis, tran_axis} as lists)."""
    from articulation3d_amd.structures import Boxes
    from articulation3d_amd.utils.opt_utils import axis_to_angle_offset

    rng = np.random.default_rng(SEED)
    images, anns, preds = [], [], []
    for i in range(N_IMAGES):
        iid = 100 + 3 * i
        images.append({"id": iid, "file_name": f"{iid}.png", "height": H, "width": W})
        cat = 1 + int(rng.integers(0, 2))
        x, y = _q(rng.uniform(20, 300)), _q(rng.uniform(20, 200))
        w, h = _q(rng.uniform(120, 300)), _q(rng.uniform(120, 240))
        line = [int(v) for v in (rng.uniform(x, x + w), rng.uniform(y, y + h / 3), rng.uniform(x, x + w), rng.uniform(y + 2 * h / 3, y + h))]
        normal = rng.normal(size=3)
        normal = (normal / np.linalg.norm(normal)).tolist()
        u = rng.uniform()
        ann = {"id": i + 1, "image_id": iid, "category_id": cat, "bbox": [float(x), float(y), float(w), float(h)],
               "rot_axis": line if cat == 1 else None, "tran_axis": line if cat == 2 else None,
               "normal": None if u < 0.1 else ([-1, -1, -1] if u < 0.2 else normal)}
        if rng.uniform() < 0.15:  # an articulated object without its axis
            ann["rot_axis"] = ann["tran_axis"] = None
        anns.append(ann)
        D = int(rng.integers(0, 7))
        scores = np.sort(rng.uniform(0.05, 1.0, D))[::-1]
        boxes, classes, plane, rot, tran = [], [], [], [], []
        for _ in range(D):
            j = rng.uniform(-1, 1, 4) * rng.choice([4.0, 12.0, 40.0])
            b = _q([x + j[0], y + j[1], x + w + j[2], y + h + j[3]])
            boxes.append(b.tolist())
            classes.append(cat - 1 if rng.uniform() < 0.8 else 2 - cat)
            g = np.array([normal[0], normal[2], normal[1]])  # (what the evaluator's re-ordering maps onto the ground truth's axes)
            p = g + rng.normal(size=3) * rng.choice([0.05, 0.3, 1.0])
            plane.append(_f32(p * rng.uniform(0.5, 3.0)))
            near = np.array(line, np.float64) + rng.normal(size=4) * rng.choice([2.0, 25.0, 90.0])
            centre = Boxes(torch.tensor([b.tolist()])).get_centers()
            ao = axis_to_angle_offset([near.tolist()], centre)[0].numpy()
            rot.append(_f32(ao[:3]))
            far = np.array(line, np.float64) + rng.normal(size=4) * rng.choice([2.0, 25.0, 90.0])
            tran.append(_f32(axis_to_angle_offset([far.tolist()], centre)[0].numpy()[:2]))
        preds.append({"image_id": iid, "boxes": boxes, "scores": _f32(scores), "classes": classes, "plane": plane, "rot_axis": rot, "tran_axis": tran})
    return {"images": images, "annotations": anns, "categories": CATEGORIES}, preds


def check_margins(coco, preds):
    """Every decision of the law is far from its threshold: the reference's fp32 IoU / normal / EA cannot decide otherwise."""
    import eval_ref
    from articulation3d_amd.evaluation import ArtiGroundTruth

    gt = ArtiGroundTruth.from_coco(coco, THING_CLASSES, device="cpu")
    gt_f, gt_i = gt.gt_f.numpy(), gt.gt_i.numpy()
    for i, p in enumerate(preds):
        s = np.asarray(p["scores"], np.float32)
        assert len(set(s.tolist())) == len(s) and (np.diff(s) < 0).all(), "scores must be distinct and descending"
        if not len(s):
            continue
        det = np.concatenate([np.asarray(p["boxes"], np.float32).reshape(-1, 4), s[:, None], np.asarray(p["classes"], np.float32)[:, None],
                              np.asarray(p["plane"], np.float32).reshape(-1, 3), np.asarray(p["rot_axis"], np.float32).reshape(-1, 3),
                              np.asarray(p["tran_axis"], np.float32).reshape(-1, 2)], 1)
        m = eval_ref.match_image(det, gt_f[gt.gt_off[i]:gt.gt_off[i + 1]], gt_i[gt.gt_off[i]:gt.gt_off[i + 1]])
        assert (np.abs(m["iou"] - 0.7) > 1e-3).all() and (np.abs(m["iou"] - 0.5) > 1e-3).all()
        v = m["gt_id"] >= 0
        assert (np.abs(m["ea"][v] - 0.5) > 1e-4).all() and (np.abs(m["normal_err"][v] - 30.0) > 1e-2).all()
        assert (m["normal_err"][v] > 0.1).all(), "no identical normals"


def run_reference(ref_root: str, coco, preds):
    ref_pkg = os.path.join(ref_root, "articulation3d")
    _install_stand_ins(ref_pkg)
    mod = _load(os.path.join(ref_pkg, "evaluation", "arti_evaluation.py"), "articulation3d.evaluation.arti_evaluation")
    metadata = types.SimpleNamespace(thing_classes=THING_CLASSES, thing_dataset_id_to_contiguous_id={c["id"]: k for k, c in enumerate(CATEGORIES)})
    predictions = []
    for p in preds:
        b = np.asarray(p["boxes"], np.float64).reshape(-1, 4)
        inst = [{"score": s, "bbox": [x1, y1, x2 - x1, y2 - y1], "category_id": c} for (x1, y1, x2, y2), s, c in zip(b.tolist(), p["scores"], p["classes"])]
        predictions.append({"image_id": p["image_id"], "instances": inst,
                            "pred_plane": torch.tensor(p["plane"], dtype=torch.float32).reshape(-1, 3),
                            "pred_rot_axis": torch.tensor(p["rot_axis"], dtype=torch.float32).reshape(-1, 3),
                            "pred_tran_axis": torch.tensor(p["tran_axis"], dtype=torch.float32).reshape(-1, 2)})
    res = mod.evaluate_for_arti_axis(predictions, _Dataset(coco), metadata, 0.7)
    return {k: float(v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds articulation3d/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "arti_eval.json"))
    args = ap.parse_args()
    coco, preds = make_dataset()
    check_margins(coco, preds)
    metrics = run_reference(args.reference, coco, preds)
    with open(args.out, "w") as f:
        json.dump({"thing_classes": THING_CLASSES, "filter_iou": 0.7, "iou_thresh": 0.5, "normal_threshold": 30.0, "coco": coco,
                   "predictions": preds, "detection_metrics": metrics}, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(json.dumps(metrics, indent=1))
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
