"""The law of a3d_eval_match / a3d_eval_ap / a3d_depth_l1 (include/a3d.h) in numpy float64, written as loops per detection and per
ground truth from the stated law.  It shares no code with articulation3d_amd/evaluation.py; it reads plain arrays only.

An image is a dict:
    det      [D,14] fp32   box xyxy 0:4, score 4, class 5, plane 6:9, rot (sin, cos, off/100) 9:12, tran (sin, cos) 12:14
    gt_f     [G,7]  fp32   box xyxy 0:4, raw normal 4:7
    gt_i     [G,12] int32  class 0, kind 1 (0 rot, 1 tran), rot line x1 y1 x2 y2 2:6, rot valid 6, tran line 7:11, tran valid 11
The first steps of a predicted line are fp32, as the reference rounds them; everything after that is float64, one rounded operator at
a time (numpy scalars never contract).
"""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
METRICS = ("bbox", "bbox+axis", "bbox+normal", "bbox+normal+axis")
H_IMG, W_IMG = 480, 640


def pred_line(box, sin, cos, off, H=H_IMG, W=W_IMG):
    """(sin, cos, offset / 100) about the box centre -> [x1, y1, x2, y2] float64, every coordinate truncated toward zero."""
    box = np.asarray(box, F32)
    return axis_line(sin, cos, off, F32(F32(box[0] + box[2]) / F32(2)), F32(F32(box[1] + box[3]) / F32(2)), H, W)


def axis_line(sin, cos, off, cx, cy, H=H_IMG, W=W_IMG):
    """The line law about a given centre (fp32)."""
    sin, cos, off, cx, cy = F32(sin), F32(cos), F32(off), F32(cx), F32(cy)
    p = F32(off * F32(100))
    x, y = F64(F32(F32(p * cos) + cx)), F64(F32(F32(p * sin) + cy))
    if sin == 0:
        return [np.trunc(x), 0.0, np.trunc(x), float(H - 1)]
    with np.errstate(all="ignore"):
        k = -(F64(cos) / F64(sin))
        if k == 0:
            return [0.0, np.trunc(y), float(W - 1), np.trunc(y)]
        cands = []
        v = y - k * x
        if 0 <= v < H:
            cands.append((0.0, float(np.trunc(v))))
        v = (k * F64(W - 1) + y) - k * x
        if 0 <= v < H:
            cands.append((float(W - 1), float(np.trunc(v))))
        v = x - y / k
        if 0 <= v < W:
            cands.append((float(np.trunc(v)), 0.0))
        v = (x - y / k) + F64(H - 1) / k
        if 0 <= v < W:
            cands.append((float(np.trunc(v)), float(H - 1)))
    if not cands:
        return [0.0, 0.0, 1.0, 1.0]
    p1 = cands[0]
    p2 = next((c for c in cands[1:] if c != p1), p1)
    return [p1[0], p1[1], p2[0], p2[1]]


def line_angle(l):
    x1, y1, x2, y2 = (F64(v) for v in l)
    return F64(-np.pi / 2) if x1 == x2 else F64(math.atan((y1 - y2) / (x1 - x2)))


def ea_score(lp, lg, size=max(W_IMG, H_IMG)):
    """EA_metric(Line([y1,x1,y2,x2]) of each) with size (640, 480); 0 for a line whose end points coincide."""
    lp, lg = [F64(v) for v in lp], [F64(v) for v in lg]
    if (lp[0] == lp[2] and lp[1] == lp[3]) or (lg[0] == lg[2] and lg[1] == lg[3]):
        return F64(0)
    d = abs(line_angle(lp) - line_angle(lg))
    d = min(d, F64(np.pi) - d)
    d = d * 2 / F64(np.pi)
    sa = max(F64(0), 1 - d) ** 2
    dy = abs((lp[1] + lp[3]) / 2 - (lg[1] + lg[3]) / 2)
    dx = abs((lp[0] + lp[2]) / 2 - (lg[0] + lg[2]) / 2)
    dc = np.sqrt(dy * dy + dx * dx) / F64(size)
    se = max(F64(0), 1 - dc) ** 2
    return F64(sa * se)


def normal_err(plane, g):
    p0, p1, p2 = (F64(F32(v)) for v in plane)
    g0, g1, g2 = (F64(F32(v)) for v in g)
    with np.errstate(all="ignore"):
        length = np.sqrt((p0 * p0 + p1 * p1) + p2 * p2)
        den = length if length > 1e-12 else F64(1e-12)
        n0, n1, n2 = p0 / den, p1 / den, p2 / den
        dot = (n0 * g0 + (-n2) * (-g1)) + n1 * g2
        dot = F64(1) if dot > 1 else (F64(-1) if dot < -1 else dot)
        err = F64(math.acos(dot)) / F64(np.pi) * F64(180) if dot == dot else F64(np.nan)
    return F64(180) if np.sqrt((g0 * g0 + g1 * g1) + g2 * g2) > 1.1 else err


def box_iou(a, b):
    ax1, ay1, ax2, ay2 = (F64(F32(v)) for v in a)
    bx1, by1, bx2, by2 = (F64(F32(v)) for v in b)
    area_a, area_b = (ax2 - ax1) * (ay2 - ay1), (bx2 - bx1) * (by2 - by1)
    w = max(min(ax2, bx2) - max(ax1, bx1), F64(0))
    h = max(min(ay2, by2) - max(ay1, by1), F64(0))
    inter = w * h
    return inter / ((area_a + area_b) - inter) if inter > 0 else F64(0)


def match_image(det, gt_f, gt_i, filter_iou=0.7, iou_thresh=0.5, normal_thresh=30.0, H=H_IMG, W=W_IMG):
    """-> dict of per-detection arrays: gt_id int32, iou / ea / normal_err float64, rank int32, tp uint8, and `qual` (the qualifying
    bits before "already covered")."""
    det, gt_f, gt_i = np.asarray(det, F32).reshape(-1, 14), np.asarray(gt_f, F32).reshape(-1, 7), np.asarray(gt_i, np.int32).reshape(-1, 12)
    D, G = len(det), len(gt_f)
    out = dict(gt_id=np.full(D, -1, np.int32), iou=np.zeros(D, F64), ea=np.zeros(D, F64), normal_err=np.full(D, 180.0, F64),
               rank=np.zeros(D, np.int32), tp=np.zeros(D, np.uint8), qual=np.zeros(D, np.uint8))
    for d in range(D):
        sc = det[d, 4]
        out["rank"][d] = sum(1 for j in range(D) if det[j, 4] > sc or (det[j, 4] == sc and j < d))
        gid, best = 0, F64(0)
        for g in range(G):
            v = box_iou(det[d, :4], gt_f[g, :4])
            if g == 0 or v > best:
                gid, best = g, v
        out["iou"][d] = best
        if not (G > 0 and best > filter_iou):
            continue
        out["gt_id"][d] = gid
        tran = gt_i[gid, 1] != 0
        gl = gt_i[gid, 7:12] if tran else gt_i[gid, 2:7]
        ea = F64(0)
        if gl[4] != 0:
            lp = pred_line(det[d, :4], det[d, 12], det[d, 13], 0.0, H, W) if tran else pred_line(det[d, :4], det[d, 9], det[d, 10], det[d, 11], H, W)
            ea = ea_score(lp, gl[:4], max(W, H))
        err = normal_err(det[d, 6:9], gt_f[gid, 4:7])
        out["ea"][d], out["normal_err"][d] = ea, err
        if int(det[d, 5]) == gt_i[gid, 0] and best > iou_thresh:
            ax, nm = bool(ea > iou_thresh), bool(err < normal_thresh)
            out["qual"][d] = 1 | (2 if ax else 0) | (4 if nm else 0) | (8 if ax and nm else 0)
    # the reference's loop: by rank, a ground truth is covered by its first true positive per metric
    covered = [set() for _ in METRICS]
    for d in np.argsort(out["rank"], kind="stable"):
        for m in range(4):
            if (out["qual"][d] >> m) & 1 and out["gt_id"][d] not in covered[m]:
                out["tp"][d] |= 1 << m
                covered[m].add(int(out["gt_id"][d]))
    return out


def voc_ap(tp_sorted, npos):
    """compute_ap / xVOCap (VOCap.py) in float64 on the 0/1 labels already sorted by descending score."""
    tp_sorted = np.asarray(tp_sorted, F64)
    if len(tp_sorted) == 0:
        return 0.0
    tp, fp = np.cumsum(tp_sorted), np.cumsum(1.0 - tp_sorted)
    rec, prec = tp / F64(npos), tp / (fp + tp)
    mrec, mpre = np.concatenate(([0.0], rec, [1.0])), np.concatenate(([0.0], prec, [0.0]))
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = F64(0)
    for i in np.nonzero(mrec[1:] != mrec[:-1])[0] + 1:
        ap = ap + (mrec[i] - mrec[i - 1]) * mpre[i]
    return float(ap)


def sorted_entries(images, matches, n_classes):
    """Per class c: the tp bytes of the valid detections predicted as c, by descending score, stable over (image index, rank)."""
    per = [[] for _ in range(n_classes)]
    for i, (im, mt) in enumerate(zip(images, matches)):
        det = np.asarray(im["det"], F32).reshape(-1, 14)
        for d in np.argsort(mt["rank"], kind="stable"):
            if mt["gt_id"][d] >= 0 and 0 <= int(det[d, 5]) < n_classes:
                per[int(det[d, 5])].append((float(det[d, 4]), int(mt["tp"][d])))
    out = []
    for rows in per:
        order = sorted(range(len(rows)), key=lambda r: -rows[r][0])  # (sorted is stable)
        out.append(np.array([rows[r][1] for r in order], np.uint8))
    return out


def evaluate(images, npos, names, **thresholds):
    """images in the order of the ground-truth table -> ({"<metric> - <name>": ap}, matches, entries per class)."""
    matches = [match_image(im["det"], im["gt_f"], im["gt_i"], **thresholds) for im in images]
    entries = sorted_entries(images, matches, len(names))
    res = {}
    for c, name in enumerate(names):
        if npos[c] <= 0:
            continue
        for m, metric in enumerate(METRICS):
            res[f"{metric} - {name}"] = voc_ap((entries[c] >> m) & 1, npos[c])
    return res, matches, entries


def det_rows(pred):
    """One entry of a fixture's `predictions` (boxes xyxy, scores, classes, plane, rot_axis, tran_axis as lists) -> [D,14] fp32."""
    n = len(pred["scores"])
    col = lambda k, w: np.asarray(pred[k], F32).reshape(n, w)
    return np.concatenate([col("boxes", 4), col("scores", 1), col("classes", 1), col("plane", 3), col("rot_axis", 3), col("tran_axis", 2)], 1)


def depth_l1(pred, gt):
    """-> (sum [B] float64, count [B]) of |pred - gt| over gt > 1e-4."""
    pred, gt = np.asarray(pred, F32), np.asarray(gt, F32)
    mask = gt > F32(1e-4)
    diff = np.abs(pred.astype(F64) - gt.astype(F64)) * mask
    return diff.reshape(len(pred), -1).sum(1), mask.reshape(len(pred), -1).sum(1)
