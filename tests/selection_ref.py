"""Host reference of the selection stage (csrc/proposals.hip: rpn_select, box_candidates, group_nms / nms_mask, merge_topk) and
the deterministic case lists it is held on.  Plain numpy; imported by tests/test_selection_ref_host.py (CPU, against the oracle) and
tests/test_gpu_selection.py (GPU, against the kernels).

SEMANTICS (SURVEY.md A.4-A.8 and the oracle's restatement of detectron2 / torchvision; nothing here is read off the kernels).
  order      Scores sort descending.  Equal scores keep the lower index first (anchor index (y W + x) 3 + a inside a level, proposal
             row inside a class).  -0 equals +0.  Every NaN, whatever its sign bit or payload, sorts before every number (torch.sort)
             and is then invalid; NaNs keep index order among themselves.
  top-k      Per (image, level): the first k = min(pre_topk, H W A) of that order.
  decode     Box2BoxTransform.apply_deltas, then Boxes.clip.  min(d, scale_clamp) is torch.clamp(max=): a NaN dw / dh stays NaN.
  valid      RPN: the decoded (unclipped) box and the score are finite and the clipped box is wider AND taller than min_size (strict).
             Box head: every probability and every class's decoded box of the ROW is finite; candidates are (row, class) with
             probability > score_thresh (strict), enumerated row-major; the background column never is one.
  NMS        Per group (level / class), over the score-ordered candidates: a valid box not yet suppressed is kept and suppresses every
             later valid box with IoU > thr (strict).  Invalid boxes neither survive nor suppress.
  merge      Per image: the kept boxes of its groups by (score descending, position ascending), the first K.  Position = (level <<
             CB) | rank-in-level for the RPN (CB = 10 in the 1024-slot layout, 11 in the 2048-slot one: include/a3d.h) and row * C +
             class for the box head -- the order of detectron2's concatenation / `nonzero`.  Unused output slots are zero boxes and
             scores with level / class / pos -1.
  dispatch   (the project's launch rule, asserted by the GPU file)  pre_topk <= 1024: 1024-slot groups; up to 1024 groups keep their
             suppression words in global memory, more keep them in LDS.  pre_topk > 1024: 2048-slot groups, words in global
             memory, formed by 64 row blocks per group up to 40 groups and by 16 above.

ARITHMETIC.  Decode, clip and IoU are np.float32 in the operator order of A.5 / A.6, one rounding per operation (the kernel file is
built with -ffp-contract=off):  w = x2 - x1;  cx = x1 + 0.5 w;  d / weight;  pcx = dx w + cx;  pw = exp(dw) w;  x1' = pcx - 0.5 pw;
IoU = inter / ((a_i + a_j) - inter).  With dw = dh = 0, exp is exactly 1 and every output is reproducible bit for bit; such cases are
marked `exact`.  Otherwise two correct implementations differ through exp's last place: boxes are then held to 2e-3 px and the
NMS / merge are re-run on the boxes under test (`boxes_from`).  Softmax is float32, max-subtracted, the denominator summed in class
order; exact where every exponent is 0 or underflows to 0 (logits 0 / -200), to 1e-6 otherwise.

VARIANTS are deliberately wrong readings of the rules.  The case lists must tell each of them from the truth.
"""
import functools
import math
import types

import numpy as np

f32 = np.float32
VARIANTS = ("tie_high", "nms_ge", "invalid_suppress", "thresh_ge", "merge_pos_rev", "neg_nan_last")
FPN_STRIDES = (4, 8, 16, 32, 64)
SCALE_CLAMP = math.log(1000.0 / 16)
SIZES = (32, 64, 128, 256, 512)
RATIOS = (0.5, 1.0, 2.0)
NEG_NAN = np.array([0xFFC00000], dtype=np.uint32).view(f32)[0]
POS_NAN = np.array([0x7FC00000], dtype=np.uint32).view(f32)[0]
INF = f32(np.inf)


def route(n_groups, pre_topk=1000):
    """The launch rule of DESIGN.md's selection contract (the constants are those of csrc/proposals.hip: A3D_NMS_SPLIT_GROUPS, `G <= 40`)."""
    if pre_topk <= 1024:
        return ("slots1024", "global-words" if n_groups <= 1024 else "lds-words")
    return ("slots2048", "rows64" if n_groups <= 40 else "rows16")


def cell_anchors(sizes, ratios):
    """A.4: for size s, ratio r: w = sqrt(s^2 / r), h = r w, box (-w/2, -h/2, w/2, h/2) -> float32 [L, A, 4]."""
    out = []
    for s in sizes:
        rows = []
        for r in ratios:
            w = math.sqrt(float(s) ** 2 / r)
            h = r * w
            rows.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
        out.append(rows)
    return np.array(out, dtype=f32)


def order_desc(scores, variant=None):
    """Indices of `scores` in selection order: NaN first, descending, -0 == +0, ties by lower index."""
    s = np.asarray(scores, dtype=f32)
    idx = np.arange(len(s))
    nan = np.isnan(s)
    last = nan & np.signbit(s) if variant == "neg_nan_last" else np.zeros_like(nan)
    cls = np.where(nan & ~last, 0, np.where(last, 2, 1))
    val = np.where(nan, f32(0), s)
    tie = -idx if variant == "tie_high" else idx
    with np.errstate(invalid="ignore"):
        return np.lexsort((tie, -val, cls))


def decode_clip(anchors, deltas, weights, scale_clamp, img_hw):
    """A.5 in float32 -> (clipped boxes [N, 4], finite [N] of the unclipped box)."""
    a = np.asarray(anchors, dtype=f32).reshape(-1, 4)
    d = np.asarray(deltas, dtype=f32).reshape(-1, 4)
    wx, wy, ww, wh = (f32(v) for v in weights)
    cl, half = f32(scale_clamp), f32(0.5)
    with np.errstate(all="ignore"):
        w, h = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        cx, cy = a[:, 0] + half * w, a[:, 1] + half * h
        dx, dy, dw, dh = d[:, 0] / wx, d[:, 1] / wy, d[:, 2] / ww, d[:, 3] / wh
        dw = np.where(dw > cl, cl, dw)
        dh = np.where(dh > cl, cl, dh)
        pcx, pcy = dx * w + cx, dy * h + cy
        pw, ph = np.exp(dw) * w, np.exp(dh) * h
        box = np.stack([pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph], axis=1).astype(f32)
        fin = np.isfinite(box).all(axis=1)
        lim = np.array([img_hw[1], img_hw[0], img_hw[1], img_hw[0]], dtype=f32)
        box = np.minimum(np.maximum(box, f32(0)), lim)
    return box, fin


def iou_row(b, i):
    """A.6: IoU of box i against every box of b, float32."""
    with np.errstate(all="ignore"):
        bi = b[i]
        ai = (bi[2] - bi[0]) * (bi[3] - bi[1])
        iw = np.maximum(f32(0), np.minimum(bi[2], b[:, 2]) - np.maximum(bi[0], b[:, 0]))
        ih = np.maximum(f32(0), np.minimum(bi[3], b[:, 3]) - np.maximum(bi[1], b[:, 1]))
        inter = iw * ih
        aj = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        return inter / ((ai + aj) - inter)


def nms(boxes, valid, thr, variant=None):
    """Greedy NMS over score-ordered boxes -> keep [n] bool."""
    b = np.ascontiguousarray(boxes, dtype=f32).reshape(-1, 4)
    n = len(b)
    valid = np.asarray(valid, dtype=bool)
    keep = np.zeros(n, dtype=bool)
    sup = np.zeros(n, dtype=bool)
    thr = f32(thr)
    for i in range(n):
        if sup[i]:
            continue
        if valid[i]:
            keep[i] = True
        elif variant != "invalid_suppress":
            continue
        o = iou_row(b, i)
        with np.errstate(invalid="ignore"):
            hit = (o >= thr) if variant == "nms_ge" else (o > thr)
        hit[: i + 1] = False
        sup |= hit
    return keep


def merge(scores, pos, keep, n, K, variant=None):
    """Groups of ONE image ([NG, cap] arrays, n [NG]) -> (group, slot) of the first K kept boxes by (score desc, pos asc)."""
    gl, r = np.nonzero(keep & (np.arange(keep.shape[1])[None, :] < np.asarray(n)[:, None]))
    s, p = scores[gl, r], pos[gl, r].astype(np.int64)
    o = np.lexsort((-p if variant == "merge_pos_rev" else p, -s))[:K]
    return gl[o], r[o]


def _finish(G, NG, B, K, cat_name, variant):
    """NMS per group and merge per image on the group arrays G -> the reference's result namespace."""
    out = types.SimpleNamespace(boxes=np.zeros((B, K, 4), f32), scores=np.zeros((B, K), f32), pos=np.full((B, K), -1, np.int32),
                                count=np.zeros(B, np.int32), groups=G)
    cat = np.full((B, K), -1, np.int32)
    for g in range(B * NG):
        n = int(G["n"][g])
        G["keep"][g, :n] = nms(G["boxes"][g, :n], G["valid"][g, :n], G["thr"], variant)
    for b in range(B):
        sl = slice(b * NG, (b + 1) * NG)
        gl, r = merge(G["scores"][sl], G["pos"][sl], G["keep"][sl], G["n"][sl], K, variant)
        c = len(gl)
        out.count[b] = c
        out.boxes[b, :c] = G["boxes"][sl][gl, r]
        out.scores[b, :c] = G["scores"][sl][gl, r]
        out.pos[b, :c] = G["pos"][sl][gl, r]
        cat[b, :c] = gl
    setattr(out, cat_name, cat)
    return out


def _groups(n_groups, cap, thr):
    return dict(boxes=np.zeros((n_groups, cap, 4), f32), scores=np.zeros((n_groups, cap), f32), pos=np.zeros((n_groups, cap), np.int32),
                valid=np.zeros((n_groups, cap), bool), keep=np.zeros((n_groups, cap), bool), n=np.zeros(n_groups, np.int32),
                idx=np.full((n_groups, cap), -1, np.int64), thr=thr)


def rpn_reference(heads, strides, cell_anchors, img_hw, pre_topk, post_topk, nms_thresh, min_size, weights, scale_clamp, *,
                  variant=None, boxes_from=None):
    """heads[l]: [B, Hf, Wf, CH] float32 (channels 0..2 objectness, 3..14 deltas a*4+coord).  -> namespace with per image boxes
    [B, K, 4], scores, level, pos [B, K], count [B], and .groups: per group (g = image * L + level) scores / boxes / valid / keep
    [G, cap], n [G], idx (anchor index of every slot), pos.  boxes_from [G, cap, 4]: run NMS and merge on these boxes instead of the
    reference's own (validity stays the reference's)."""
    L, B = len(heads), heads[0].shape[0]
    cap, cb = (1024, 10) if pre_topk <= 1024 else (2048, 11)
    assert pre_topk <= 2048
    G = _groups(B * L, cap, nms_thresh)
    for b in range(B):
        for l in range(L):
            h = np.asarray(heads[l][b], dtype=f32)
            Hf, Wf = h.shape[:2]
            logits = h[:, :, :3].reshape(-1)
            k = min(int(pre_topk), logits.size)
            idx = order_desc(logits, variant)[:k]
            pix, an = idx // 3, idx % 3
            y, x = pix // Wf, pix % Wf
            shift = np.stack([x, y, x, y], axis=1) * int(strides[l])
            anchors = shift.astype(f32) + np.asarray(cell_anchors[l], dtype=f32)[an]
            deltas = h.reshape(Hf * Wf, -1)[pix[:, None], 3 + an[:, None] * 4 + np.arange(4)[None, :]]
            box, fin = decode_clip(anchors, deltas, weights, scale_clamp, img_hw)
            sc = logits[idx]
            with np.errstate(invalid="ignore"):
                ne = ((box[:, 2] - box[:, 0]) > f32(min_size)) & ((box[:, 3] - box[:, 1]) > f32(min_size))
            g = b * L + l
            G["n"][g] = k
            G["idx"][g, :k] = idx
            G["scores"][g, :k] = sc
            G["boxes"][g, :k] = box if boxes_from is None else np.asarray(boxes_from[g, :k], dtype=f32)
            G["valid"][g, :k] = fin & np.isfinite(sc) & ne
            G["pos"][g] = (l << cb) | np.arange(cap)
    return _finish(G, L, B, int(post_topk), "level", variant)


def softmax32(logits):
    """[N, C+1] -> probabilities, float32: max-subtracted, denominator summed in class order."""
    p = np.asarray(logits, dtype=f32)
    with np.errstate(all="ignore"):
        mx = p[:, 0]
        for j in range(1, p.shape[1]):
            mx = np.fmax(mx, p[:, j])
        e = np.exp(p - mx[:, None])
        den = np.zeros(len(p), f32)
        for j in range(p.shape[1]):
            den = den + e[:, j]
        return e / den[:, None]


def boxdet_reference(pred, prop_boxes, prop_count, img_hw, num_classes, score_thresh, nms_thresh, topk, weights, scale_clamp, *,
                     variant=None, boxes_from=None):
    """pred [B*R, CH] (class logits 0..C, background last; deltas C+1 + c*4 + coord), prop_boxes [B, R, 4], prop_count [B].
    -> as rpn_reference with .classes; groups g = image * C + class, idx = proposal row of every slot, pos = row * C + class."""
    C = int(num_classes)
    B, R = prop_boxes.shape[:2]
    pred = np.asarray(pred, dtype=f32).reshape(B, R, -1)
    G = _groups(B * C, 1024, nms_thresh)
    G["probs"] = []
    thr = f32(score_thresh)
    for b in range(B):
        n = min(int(prop_count[b]), R)
        pr = pred[b, :n]
        probs = softmax32(pr[:, : C + 1])
        ok = np.isfinite(probs).all(axis=1)
        dec = []
        for c in range(C):
            box, fin = decode_clip(prop_boxes[b, :n], pr[:, C + 1 + 4 * c: C + 5 + 4 * c], weights, scale_clamp, img_hw)
            dec.append(box)
            ok &= fin
        G["probs"].append(np.where(ok[:, None], probs[:, :C], f32(np.nan)))
        for c in range(C):
            with np.errstate(invalid="ignore"):
                cand = ok & ((probs[:, c] >= thr) if variant == "thresh_ge" else (probs[:, c] > thr))
            rows = np.nonzero(cand)[0]
            rows = rows[order_desc(probs[rows, c], variant)]
            g, k = b * C + c, len(rows)
            G["n"][g] = k
            G["idx"][g, :k] = rows
            G["scores"][g, :k] = probs[rows, c]
            G["boxes"][g, :k] = dec[c][rows] if boxes_from is None else np.asarray(boxes_from[g, :k], dtype=f32)
            G["valid"][g, :k] = True
            G["pos"][g, :k] = rows * C + c
    return _finish(G, C, B, int(topk), "classes", variant)


# ------------------------------------------------------------------------------------------------------------------ RPN cases
P5 = ((24, 31), (13, 17), (8, 10), (5, 6), (3, 4))          # 2232 / 663 / 240 / 90 / 36 anchors, image 96 x 124
T3 = ((26, 27), (13, 17), (8, 10))                           # 2106 / 663 / 240
D2000 = ((26, 27), (20, 23), (8, 10), (4, 5), (2, 3))        # 2106 / 1380 / 240 / 60 / 18: rows past 1024 in two levels
D1000 = ((7, 6), (5, 6), (3, 4), (2, 3), (1, 2))             # 126 / 90 / 36 / 18 / 6: tiny levels, a thousand groups in seconds
FEW = np.array([-1.0, -0.5, 0.0, 0.5, 2.0], dtype=f32)


def _normal(rng, shape):
    return rng.standard_normal(shape).astype(f32)


def _few(rng, shape):
    return rng.choice(FEW, size=shape)


def _pm_zero(rng, shape):
    return rng.choice(np.array([-0.0, 0.0, 1.0, -1.0], dtype=f32), size=shape, p=[0.45, 0.45, 0.01, 0.09])  # rank k falls among the zeros


def _heads(seed, B, shapes, CH, logits, deltas):
    """Image b of a case is a function of (seed, b) alone: the same image in batches of different size.  Channels past 15 hold noise."""
    heads = [np.empty((B, h, w, CH), f32) for h, w in shapes]
    for b in range(B):
        rng = np.random.default_rng([seed, b])
        for l, (h, w) in enumerate(shapes):
            t = _normal(rng, (h, w, max(CH, 15)))
            fn = logits[l] if isinstance(logits, (list, tuple)) else logits
            t[..., :3] = fn(rng, (h, w, 3))
            d = t[..., 3:15]
            d *= f32(0.5)
            if deltas == "zero":
                d[...] = 0
            elif deltas == "exact":  # dw = dh = 0: exp is exactly 1
                d[..., 2::4] = 0
                d[..., 3::4] = 0
            heads[l][b] = t[..., :CH]
    return heads


def _rpn(name, heads, *, img_hw, pre_topk, exact, post_topk=1000, nms_thresh=0.7, min_size=0.0, sizes=SIZES, ratios=RATIOS,
         nan_scores=False):
    L = len(heads)
    return types.SimpleNamespace(name=name, family=name.split("/")[0], heads=heads, L=L, B=heads[0].shape[0], CH=heads[0].shape[3],
                                 strides=FPN_STRIDES[:L], sizes=tuple(sizes), ratios=tuple(ratios), cell=cell_anchors(sizes[:L], ratios),
                                 img_hw=img_hw, pre_topk=pre_topk, post_topk=post_topk, nms_thresh=nms_thresh, min_size=min_size,
                                 weights=(1.0, 1.0, 1.0, 1.0), scale_clamp=SCALE_CLAMP, exact=exact, nan_scores=nan_scores)


def _const(v):
    return lambda rng, shape: np.full(shape, v, dtype=f32)


def _nonfinite_case():
    heads = _heads(31, 2, P5, 16, _normal, "general")
    spots = []  # (level, image, y, x, a)
    for l, (h, w) in enumerate(P5[:3]):
        for j in range(8):
            spots.append((l, j % 2, (3 * j + 1) % h, (5 * j + 2) % w, j % 3))
    vals = [POS_NAN, NEG_NAN, INF, -INF]
    for j, (l, b, y, x, a) in enumerate(spots):  # non-finite objectness logits, each kind on every level that has n > k
        heads[l][b, y, x, a] = vals[j % 4]
    j = 0
    for coord in range(4):  # a non-finite value in each delta of an anchor that ranks high
        for v in vals:
            l, b = j % 3, (j // 3) % 2
            y, x, a = (2 * j + 5) % P5[l][0], (3 * j + 7) % P5[l][1], (j + 1) % 3
            heads[l][b, y, x, a] = f32(4.0 + 0.01 * j)
            heads[l][b, y, x, 3 + 4 * a + coord] = v
            j += 1
    return _rpn("nonfinite/logits_and_deltas", heads, img_hw=(96, 124), pre_topk=100, exact=False, nan_scores=True)


def _degenerate_case():
    heads = _heads(41, 3, ((8, 10), (4, 5)), 16, _normal, "zero")
    for h in heads:
        h[0, ..., 5:15:4] = -INF  # image 0: dw = -Inf on every anchor -> zero-width boxes: all invalid
        h[2, ..., :3] = POS_NAN        # image 2: every score NaN: all invalid
    # image 1: anchors far larger than the image all clip to the whole image: one box per level survives, the rest are suppressed
    return _rpn("degenerate/invalid_suppressed", heads, img_hw=(32, 40), pre_topk=1000, exact=True, sizes=(4096,) * 5,
                ratios=(1.0, 1.0, 1.0), nan_scores=True)


RPN_BUILDERS = {
    # ---- tie families
    "ties/few_values_k20": lambda: _rpn("ties/few_values_k20", _heads(1, 2, P5, 16, _few, "general"), img_hw=(96, 124), pre_topk=20, exact=False),
    "ties/few_values_k1000": lambda: _rpn("ties/few_values_k1000", _heads(2, 1, P5[:1], 16, _few, "exact"), img_hw=(96, 124), pre_topk=1000, exact=True),
    "ties/few_values_k2000": lambda: _rpn("ties/few_values_k2000", _heads(3, 1, ((26, 27), (24, 31)), 16, _few, "exact"), img_hw=(104, 124), pre_topk=2000, exact=True),
    "ties/all_equal_level": lambda: _rpn("ties/all_equal_level", _heads(4, 2, P5[:3], 16, [_normal, _const(0.25), _normal], "exact"), img_hw=(96, 124), pre_topk=240, exact=True),
    "ties/pm_zero": lambda: _rpn("ties/pm_zero", _heads(5, 1, P5[:3], 16, _pm_zero, "exact"), img_hw=(96, 124), pre_topk=240, exact=True),
    # three identical square anchors per cell; neighbours one stride apart overlap by exactly IoU 1/2 = thr (12-px boxes 4 px apart)
    "ties/duplicates_iou_at_thr": lambda: _rpn("ties/duplicates_iou_at_thr", _heads(6, 1, ((24, 31), (12, 16), (6, 8)), 16, _few, "zero"), img_hw=(96, 124),
                                               pre_topk=1000, exact=True, nms_thresh=0.5, sizes=(12, 24, 48, 96, 192), ratios=(1.0, 1.0, 1.0)),
    "ties/duplicates_iou_at_thr_k2000": lambda: _rpn("ties/duplicates_iou_at_thr_k2000", _heads(6, 1, ((24, 31), (12, 16), (6, 8)), 16, _few, "zero"), img_hw=(96, 124),
                                                     pre_topk=2000, exact=True, nms_thresh=0.5, sizes=(12, 24, 48, 96, 192), ratios=(1.0, 1.0, 1.0)),
    # ---- count families
    **{f"count/pre_topk_{k}": (lambda k=k: _rpn(f"count/pre_topk_{k}", _heads(7, 2, T3, 16, _normal, "exact"), img_hw=(104, 108), pre_topk=k, exact=True))
       for k in (1, 240, 1000, 1024, 1025, 2000, 2048)},
    "count/post_topk_50": lambda: _rpn("count/post_topk_50", _heads(7, 2, T3, 16, _normal, "exact"), img_hw=(104, 108), pre_topk=1000, post_topk=50, exact=True),
    "count/min_size_8": lambda: _rpn("count/min_size_8", _heads(8, 1, P5, 16, _normal, "general"), img_hw=(96, 124), pre_topk=1000, min_size=8.0, exact=False),
    "count/L1_CH15": lambda: _rpn("count/L1_CH15", _heads(9, 2, P5[:1], 15, _normal, "general"), img_hw=(96, 124), pre_topk=1000, exact=False),
    "count/L5_CH32": lambda: _rpn("count/L5_CH32", _heads(10, 2, P5, 32, _normal, "general"), img_hw=(96, 124), pre_topk=1000, exact=False),
    # 128 x 171 x 3 = 65 664 anchors: a 24-bit index.  Level 0 distinct scores, level 1 (the same shape) few values: ties across rank k
    "count/index_24_bits": lambda: _rpn("count/index_24_bits", _heads(11, 1, ((128, 171), (128, 171)), 16, [_normal, _few], "exact"), img_hw=(512, 684), pre_topk=1000, exact=True),
    # ---- non-finite and degenerate families
    "nonfinite/logits_and_deltas": _nonfinite_case,
    "degenerate/invalid_suppressed": _degenerate_case,
    # ---- group-count families: both sides of each dispatch switch
    **{f"dispatch/k2000_G{5 * B}": (lambda B=B: _rpn(f"dispatch/k2000_G{5 * B}", _heads(12, B, D2000, 16, _normal, "exact"), img_hw=(104, 108), pre_topk=2000, exact=True))
       for B in (1, 8, 9)},
    "dispatch/k1000_G5": lambda: _rpn("dispatch/k1000_G5", _heads(13, 1, D1000, 16, _normal, "exact"), img_hw=(28, 24), pre_topk=1000, exact=True),
    "dispatch/k1000_G1024": lambda: _rpn("dispatch/k1000_G1024", _heads(13, 256, D1000[:4], 16, _normal, "exact"), img_hw=(28, 24), pre_topk=1000, exact=True),
    "dispatch/k1000_G1025": lambda: _rpn("dispatch/k1000_G1025", _heads(13, 205, D1000, 16, _normal, "exact"), img_hw=(28, 24), pre_topk=1000, exact=True),
}
RPN_CASES = tuple(RPN_BUILDERS)


@functools.lru_cache(maxsize=None)
def rpn_case(name):
    return RPN_BUILDERS[name]()


def rpn_args(c):
    return (c.heads, c.strides, c.cell, c.img_hw, c.pre_topk, c.post_topk, c.nms_thresh, c.min_size, c.weights, c.scale_clamp)


@functools.lru_cache(maxsize=None)
def rpn_expected(name, variant=None):
    """The reference on a committed case: computed once per process, shared by the tests, never modified."""
    return rpn_reference(*rpn_args(rpn_case(name)), variant=variant)


# ------------------------------------------------------------------------------------------------------------------ box-head cases
def _boxdet(name, seed, *, B, C, R, counts, exact, score_thresh, topk, CH=None, empty_class=None, at_thresh=None, bad_rows=False, img_hw=(120, 160)):
    rng = np.random.default_rng(seed)
    CH = 5 * C + 1 if CH is None else CH
    pred = _normal(rng, (B, R, CH))
    if exact:
        pred[..., : C + 1] = rng.choice(np.array([0.0, -200.0], dtype=f32), size=(B, R, C + 1), p=[0.4, 0.6])
        pred[..., C + 1:] *= f32(0.5)
        pred[..., C + 3: 5 * C + 1: 4] = 0  # dw
        pred[..., C + 4: 5 * C + 1: 4] = 0  # dh
    else:
        pred[..., : C + 1] *= f32(2.0)
    x1 = rng.integers(0, img_hw[1] - 24, size=(B, R))
    y1 = rng.integers(0, img_hw[0] - 24, size=(B, R))
    props = np.stack([x1, y1, x1 + rng.integers(8, 60, size=(B, R)), y1 + rng.integers(8, 60, size=(B, R))], axis=2).astype(f32)
    props[..., 2] = np.minimum(props[..., 2], img_hw[1])
    props[..., 3] = np.minimum(props[..., 3], img_hw[0])
    if R >= 7:
        # rows 0 / 1: 12-px boxes 4 px apart, IoU exactly 1/2 = thr, identical predictions, no shift; rows 2 / 3: identical in everything
        props[:, 0] = [20, 20, 32, 32]
        props[:, 1] = [24, 20, 36, 32]
        pred[:, 1] = pred[:, 0]
        pred[:, 0:2, C + 1:] = 0
        pred[:, 0:2, : C + 1] = -200.0
        pred[:, 0:2, 0] = 0  # (class 0 alone is live: probability 1, or 1/2 where `empty_class` revives the background below; either way they lead their group, in row order)
        props[:, 3] = props[:, 2]
        pred[:, 2, 0] = 0
        pred[:, 3] = pred[:, 2]
    if empty_class is not None:
        pred[..., empty_class] = -200.0
        pred[..., C] = 0.0  # (the background is live everywhere, so the class's probability is 0 in exact cases and ~e^-200 otherwise)
    if bad_rows and R >= 12:
        b = B - 1
        pred[b, 7, 0] = POS_NAN
        pred[b, 8, C + 1] = INF          # dx of class 0
        pred[b, 9, C + 1 + 4 + 2] = NEG_NAN  # dw of class 1: min(NaN, clamp) stays NaN
        pred[b, 10, 1] = INF
        pred[b, 11, C + 1 + 3] = -INF    # dh = -Inf: a finite, zero-height box: the row stays
    for b in range(B if not exact else 0):  # general logits: move apart, deterministically, what an exp ulp could reorder
        for it in range(50):
            rows = [r for r in _unseparated_rows(pred[b, :, : C + 1], softmax32(pred[b, :, : C + 1])[:, :C], score_thresh) if r > 3]
            if not rows:
                break
            pred[b, rows, 0] += f32(0.013) * (1 + np.arange(len(rows), dtype=f32))
    case = types.SimpleNamespace(name=name, family="boxdet", pred=pred.reshape(B * R, CH), prop_boxes=props, prop_count=np.array(counts, dtype=np.int32),
                                 img_hw=img_hw, C=C, R=R, B=B, CH=CH, score_thresh=float(score_thresh), nms_thresh=0.5, topk=topk,
                                 weights=(10.0, 10.0, 5.0, 5.0), scale_clamp=SCALE_CLAMP, exact=exact)
    if at_thresh is not None:
        # the threshold IS a probability the reference computes: the first row that has exactly `at_thresh` live logits
        live = (pred[..., : C + 1] == 0).sum(axis=2)
        b, r = np.argwhere((live == at_thresh) & (pred[..., 0] == 0))[0]
        case.score_thresh = float(softmax32(pred[b, r: r + 1, : C + 1])[0, 0])
    return case


def _cyc(B, R):
    return [(0, 1, R - 1, R)[b % 4] for b in range(B)]


BOXDET_BUILDERS = {
    "boxdet/C2_R1000_general": lambda: _boxdet("boxdet/C2_R1000_general", 21, B=4, C=2, R=1000, counts=_cyc(4, 1000), exact=False, score_thresh=0.05, topk=100, bad_rows=True),
    "boxdet/C2_R1000_exact_thr0": lambda: _boxdet("boxdet/C2_R1000_exact_thr0", 22, B=4, C=2, R=1000, counts=_cyc(4, 1000), exact=True, score_thresh=0.0, topk=100),
    "boxdet/C1_R7_exact": lambda: _boxdet("boxdet/C1_R7_exact", 23, B=4, C=1, R=7, counts=_cyc(4, 7), exact=True, score_thresh=0.0, topk=5),
    "boxdet/C8_R1024_exact_at_third": lambda: _boxdet("boxdet/C8_R1024_exact_at_third", 24, B=4, C=8, R=1024, counts=_cyc(4, 1024), exact=True, score_thresh=0.0, topk=300,
                                                      CH=48, empty_class=5, at_thresh=3),
    "boxdet/C2_R7_general_thr0.05_empty_class": lambda: _boxdet("boxdet/C2_R7_general_thr0.05_empty_class", 25, B=4, C=2, R=7, counts=_cyc(4, 7), exact=False, score_thresh=0.05,
                                                               topk=100, empty_class=1),
    "boxdet/G1024_exact": lambda: _boxdet("boxdet/G1024_exact", 26, B=128, C=8, R=7, counts=_cyc(128, 7), exact=True, score_thresh=0.0, topk=100),
    "boxdet/G1026_general": lambda: _boxdet("boxdet/G1026_general", 27, B=513, C=2, R=7, counts=_cyc(513, 7), exact=False, score_thresh=0.05, topk=10),
}
BOXDET_CASES = tuple(BOXDET_BUILDERS)
SCORE_TOL = 1e-6   # kernel vs reference probabilities (the project's bound for this comparison)
SEPARATION = 4e-6  # distinct probabilities of a general case lie further apart than both sides' errors together, with margin


@functools.lru_cache(maxsize=None)
def boxdet_case(name):
    return BOXDET_BUILDERS[name]()


def boxdet_args(c):
    return (c.pred, c.prop_boxes, c.prop_count, c.img_hw, c.C, c.score_thresh, c.nms_thresh, c.topk, c.weights, c.scale_clamp)


@functools.lru_cache(maxsize=None)
def boxdet_expected(name, variant=None):
    return boxdet_reference(*boxdet_args(boxdet_case(name)), variant=variant)


def _unseparated_rows(logits, probs, thresh):
    """Rows of ONE image ([n, C+1] logits, [n, C] probabilities, NaN rows = dropped) whose candidates an exp ulp could reorder or move
    across the threshold: a probability within SEPARATION of the threshold, or of a candidate of another row / class unless the two
    come from bit-identical logits in the same class."""
    bad = set()
    with np.errstate(invalid="ignore"):
        near = np.abs(probs.astype(np.float64) - thresh) <= SEPARATION
        rows, cls = np.nonzero(probs > f32(thresh))
    bad.update(np.nonzero(near.any(axis=1))[0].tolist())
    v = probs[rows, cls].astype(np.float64)
    o = np.argsort(v, kind="stable")
    for i in np.nonzero(np.diff(v[o]) <= SEPARATION)[0]:
        r0, r1 = rows[o[i]], rows[o[i + 1]]
        if not (cls[o[i]] == cls[o[i + 1]] and np.array_equal(logits[r0].view(np.uint32), logits[r1].view(np.uint32))):
            bad.add(int(r1))
    return sorted(bad)


def separated(case, ref):
    """True when no exp ulp can decide a discrete output of a general box-head case (asserted on the reference by both test files)."""
    pred = case.pred.reshape(case.B, case.R, -1)
    return all(not _unseparated_rows(pred[b, : len(p), : case.C + 1], p, case.score_thresh) for b, p in enumerate(ref.groups["probs"]))


def same(a, b, nan_ok=False):
    """Bit-level equality of two float arrays up to the sign of zero (and, with nan_ok, up to which NaN it is)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=nan_ok))
