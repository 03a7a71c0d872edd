"""The target contract of the training step, stated once in plain numpy ("The target contract"): what
a3d_match_boxes, a3d_sample_labels, a3d_sample_rois, a3d_append_gt_boxes, a3d_rpn_loss and a3d_box_loss must return.  Never
imports the product; tests/test_train_targets_ref_host.py holds it to the oracle on the CPU, tests/test_gpu_train_targets.py holds
the kernels to it on the GPU.

* Matcher: detectron2's pairwise_iou and Matcher in np.float32, one rounding per operation (the kernels are built without
  contraction, so these are their bits).
* Samplers: the hash of csrc/train_sample.hip replayed; the k smallest keys of each class.
* Losses: targets are get_deltas in np.float32 in the kernel's operation order, with log taken in float64 of the float32 ratio;
  every loss term and gradient element in float64, and next to each sum the sum of the magnitudes of the pieces that were added.
* VARIANTS: deliberately wrong readings of the rules.  The case tables below must tell each of them from the right one.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

f32 = np.float32
U = 2.0 ** -24          # unit roundoff of float32
DENORM = 2.0 ** -149    # spacing of the float32 denormals
ULP_EXP = ULP_LOG = ULP_LOG1P = 2  # device expf / logf / log1pf: not stated by the installed headers or documents -> 2 ulp each

VARIANTS = ("thr_le", "last_max", "lq_skip_zero", "lq_moves_idx", "sign0_plus", "box_div_M", "ignored_counted", "roi_index_order",
            "seed_hi_dropped")

# dispatch limits of the kernels
MATCH_MAX_GT = 64
SAMPLE_LABELS_MAX_N = (1 << 17) - 1
SAMPLE_ROIS_MAX_N = 2048
LOSS_BLOCKS, LOSS_THREADS = 64, 256


def gamma(k: float) -> float:
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------------------------------------
# matcher
# ------------------------------------------------------------------------------------------------------------------------------
def pair_iou(gt: np.ndarray, boxes: np.ndarray) -> np.ndarray:
    """[G,4] x [N,4] -> [G,N] float32: inter > 0 ? inter / (ga + ba - inter) : 0."""
    gt, boxes = np.asarray(gt, f32).reshape(-1, 4), np.asarray(boxes, f32).reshape(-1, 4)
    ga = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    ba = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    w = np.minimum(gt[:, None, 2], boxes[None, :, 2]) - np.maximum(gt[:, None, 0], boxes[None, :, 0])
    h = np.minimum(gt[:, None, 3], boxes[None, :, 3]) - np.maximum(gt[:, None, 1], boxes[None, :, 1])
    w = np.where(w > 0, w, f32(0))
    h = np.where(h > 0, h, f32(0))
    inter = (w * h).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = inter / ((ga[:, None] + ba[None, :]) - inter)
    return np.where(inter > 0, q, f32(0)).astype(f32)


def matcher(iou: np.ndarray, thresholds, labels, allow_low_quality: bool, variant: str | None = None):
    """Matcher on a [G,N] float32 quality matrix -> (matched index int32 [N], label int8 [N], best IoU float32 [N])."""
    G, N = iou.shape
    if G == 0:
        return np.zeros(N, np.int32), np.full(N, labels[0], np.int8), np.zeros(N, f32)
    idx = (G - 1 - np.argmax(iou[::-1], 0)) if variant == "last_max" else np.argmax(iou, 0)  # np.argmax: the first maximum
    val = iou[idx, np.arange(N)]
    thr = [f32(t) for t in thresholds]  # compared in float32
    below = (lambda v, t: v <= t) if variant == "thr_le" else (lambda v, t: v < t)
    if len(thr) == 2:
        lab = np.where(below(val, thr[0]), labels[0], np.where(below(val, thr[1]), labels[1], labels[2]))
    else:
        lab = np.where(below(val, thr[0]), labels[0], labels[1])
    idx = idx.astype(np.int32)
    if allow_low_quality and N > 0:
        best = iou.max(1)
        hit = iou == best[:, None]
        if variant == "lq_skip_zero":
            hit &= (best > 0)[:, None]
        lab = np.where(hit.any(0), 1, lab)
        if variant == "lq_moves_idx":
            idx = np.where(hit.any(0), np.argmax(hit, 0), idx).astype(np.int32)
    return idx, lab.astype(np.int8), val.astype(f32)


def match(c, variant: str | None = None):
    """A whole launch: case `c` (see match_case) -> (matched_idx [B,N] int32, label [B,N] int8, iou [B,N] float32).  Rows at or
    past box_count keep the wrapper's prefill (0, -1, 0)."""
    B, Gmax = c.gt_boxes.shape[:2]
    N = c.boxes.shape[-2]
    midx, lab, val = np.zeros((B, N), np.int32), np.full((B, N), -1, np.int8), np.zeros((B, N), f32)
    for b in range(B):
        G = min(int(c.gt_count[b]), Gmax)
        nb = N if c.box_count is None else max(0, min(int(c.box_count[b]), N))
        bx = c.boxes if c.shared else c.boxes[b]
        i, l, v = matcher(pair_iou(c.gt_boxes[b, :G], bx[:nb]), c.thresholds, c.labels, c.lq, variant)
        midx[b, :nb], lab[b, :nb], val[b, :nb] = i, l, v
    return midx, lab, val


A_ = (0, 0, 10, 10)  # the ground-truth box the tie cases are built around (area 100: IoU k/100 from integer boxes)
TIE_BOXES = np.array([
    (0, 0, 10, 10),       # 0 equal to the ground truth: IoU exactly 1
    (0, 0, 10, 5),        # 1 IoU exactly 1/2
    (0, 0, 10, 3),        # 2 IoU fl(3/10)
    (0, 0, 10, 7),        # 3 IoU fl(7/10)
    (0, 0, 10, 2.75),     # 4 just under 0.3
    (0, 0, 10, 3.25),     # 5 just over 0.3
    (0, 0, 10, 6.75),     # 6 just under 0.7
    (0, 0, 10, 7.25),     # 7 just over 0.7
    (0, 0, 10, 4.75),     # 8 just under 1/2
    (5, 5, 5, 5),         # 9 zero area inside the ground truth
    (3, 3, 3, 8),         # 10 zero width
    (4, 0, 22, 10),       # 11 overlaps A (0.27) and the ground truth at x 20..30 (0.077): promoted by the latter, argmax the former
    (200, 200, 210, 210),  # 12 disjoint from everything
    (0, 0, 20, 10),       # 13 IoU exactly 1/2 from the other side (box contains the ground truth)
    (10, 0, 20, 10),      # 14 touches A: intersection width 0
    (0, 0, 10, 10),       # 15 a duplicate of box 0
], f32)
TIE_ROLE = {"equal": 0, "half": 1, "f03": 2, "f07": 3, "zero_area": 9, "promoted": 11, "half_outer": 13}
TIE_GT = [  # per image: the ground truth of the tie launch
    [A_],
    [A_, A_, (0, 0, 10, 5)],                 # duplicated ground truth: the first wins
    [A_, (20, 0, 30, 10)],                   # box 11 is the best of gt 1 while its own argmax is gt 0
    [A_, (2, 2, 2, 6)],                      # zero-area ground truth: best IoU 0, attained by every box
    [A_, (500, 500, 510, 510)],              # ground truth disjoint from every box
]


def _int_boxes(rng, n, lo_size):
    xy = rng.integers(0, 48, (n, 2))
    wh = rng.integers(lo_size, 17, (n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(f32)


MATCH_CASES = ["rpn_ties", "prop_ties", "rpn_G", "prop_G"] + [f"rpn_N{n}" for n in (1, 255, 257, 32769)] + \
              [f"prop_N{n}" for n in (1, 255, 257, 32769)]


def match_case(name: str):
    """rpn_*: two thresholds, labels (0,-1,1), low quality on, shared anchors.  prop_*: one threshold, per-image boxes, box_count."""
    rpn = name.startswith("rpn")
    c = SimpleNamespace(name=name, thresholds=(0.3, 0.7) if rpn else (0.5,), labels=(0, -1, 1) if rpn else (0, 1), lq=rpn, shared=rpn,
                        box_count=None)
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.endswith("ties"):
        B, Gmax = len(TIE_GT), 4
        c.gt_boxes = np.zeros((B, Gmax, 4), f32)
        for b, g in enumerate(TIE_GT):
            c.gt_boxes[b, : len(g)] = np.array(g, f32)
        c.gt_count = np.array([len(g) for g in TIE_GT], np.int32)
        c.boxes = TIE_BOXES.copy() if rpn else np.repeat(TIE_BOXES[None], B, 0).copy()
        if not rpn:
            c.box_count = np.array([16, 16, 0, 7, 21], np.int32)  # N, N, 0, mid, N + 5
        return c
    if name.endswith("_G"):  # G in {0, 1, 64} in one launch, Gmax = 64
        B, Gmax, N = 3, 64, 257
        c.gt_count = np.array([0, 1, 64], np.int32)
    else:
        N = int(name.split("_N")[1])
        B, Gmax = 4, 8
        c.gt_count = np.array([3, 8, 0, 11], np.int32)  # (11: above Gmax, clamped)
    c.gt_boxes = _int_boxes(rng, B * Gmax, 1).reshape(B, Gmax, 4)
    c.boxes = _int_boxes(rng, N if rpn else B * N, 0).reshape((N, 4) if rpn else (B, N, 4))  # small integers: ties and zero areas abound
    if not rpn:
        c.box_count = np.array([0, (N + 1) // 2, N, N + 5], np.int32)[:B] if not name.endswith("_G") else np.array([N, 100, N + 5], np.int32)
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# samplers
# ------------------------------------------------------------------------------------------------------------------------------
def _mix32(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def fold_seed(seed: int) -> int:
    return (seed ^ (seed >> 32)) & 0xFFFFFFFF


def sample_key(seed: int, b: int, n: int, variant: str | None = None) -> np.ndarray:
    """The keys of candidates 0..n-1 of image b: 31 hashed bits above the 17-bit index (distinct by construction)."""
    s = (seed & 0xFFFFFFFF) if variant == "seed_hi_dropped" else fold_seed(seed)
    i = np.arange(n, dtype=np.uint64)
    hb = _mix32(np.uint64(s ^ ((0x9E3779B9 * (b + 1)) & 0xFFFFFFFF)))
    h = _mix32(hb ^ ((np.uint64(0x85EBCA6B) * (i + np.uint64(1))) & np.uint64(0xFFFFFFFF)))
    return ((h >> np.uint64(1)) << np.uint64(17)) | i


def subsample_labels(labels: np.ndarray, num: int, max_pos: int, seed: int, variant: str | None = None) -> np.ndarray:
    """[B,N] int8 -> the same with the k_pos smallest keys among label 1 kept as 1, the k_neg smallest among label 0 kept as 0
    (k_pos = min(#1, max_pos), k_neg = min(#0, num - k_pos)), everything else -1.  Labels outside {0, 1} are ignored."""
    B, N = labels.shape
    out = np.full((B, N), -1, np.int8)
    for b in range(B):
        key = sample_key(seed, b, N, variant)
        k_pos = min(int((labels[b] == 1).sum()), max_pos)
        k_neg = min(int((labels[b] == 0).sum()), num - k_pos)
        for cls, k in ((1, k_pos), (0, k_neg)):
            ids = np.nonzero(labels[b] == cls)[0]
            out[b, ids[np.argsort(key[ids])[:k]]] = cls
    return out


def append_gt(props, count, gt, gt_count):
    """[B,R,4] + [B,Gmax,4] -> ([B,R+Gmax,4] = live proposals | ground truth | zeros, count); both counts clamped to their buffers."""
    B, R = props.shape[:2]
    Gmax = gt.shape[1]
    out, cnt = np.zeros((B, R + Gmax, 4), f32), np.zeros(B, np.int32)
    for b in range(B):
        n, g = min(int(count[b]), R), min(int(gt_count[b]), Gmax)
        out[b, :n], out[b, n : n + g] = props[b, :n], gt[b, :g]
        cnt[b] = n + g
    return out, cnt


def sample_rois(c, variant: str | None = None):
    """Case c (boxes [B,N,4], box_count, gt_boxes [B,Gmax,4], gt_classes, gt_count, matched_idx, match_label, K, num, max_fg, seed)
    -> (boxes [B,num,4], gt_boxes [B,num,4], classes [B,num], index [B,num], count [B]).  A sample's slot is its key rank inside
    its class, foreground first; slots past the count are zeros, class K, index -1."""
    B, N = c.boxes.shape[:2]
    K, num = c.K, c.num
    ob, og = np.zeros((B, num, 4), f32), np.zeros((B, num, 4), f32)
    oc, oi, on = np.full((B, num), K, np.int32), np.full((B, num), -1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        n = max(0, min(int(c.box_count[b]), N))
        G = int(c.gt_count[b])
        cls = np.full(n, K, np.int64)
        if G > 0:
            fgm = c.match_label[b, :n] == 1
            cls[fgm] = c.gt_classes[b, c.matched_idx[b, :n][fgm]]
        key = sample_key(c.seed, b, n, variant)
        fg, bg = np.nonzero(cls < K)[0], np.nonzero(cls >= K)[0]
        k_fg = min(len(fg), c.max_fg)
        k_bg = min(len(bg), num - k_fg)
        pick = np.concatenate([fg[np.argsort(key[fg])[:k_fg]], bg[np.argsort(key[bg])[:k_bg]]]).astype(np.int64)
        if variant == "roi_index_order":
            pick = np.concatenate([np.sort(pick[:k_fg]), np.sort(pick[k_fg:])])
        m = len(pick)
        on[b] = m
        ob[b, :m], oc[b, :m], oi[b, :m] = c.boxes[b, pick], cls[pick], pick
        og[b, :m] = c.gt_boxes[b, c.matched_idx[b, pick]] if G > 0 else c.boxes[b, pick]
    return ob, og, oc, oi, on


SAMPLE_LABEL_CASES = ["n1", "n255", "n1025", "n131071", "edges", "rows3", "seed_hi"]


def sample_labels_case(name: str):
    """-> labels [B,N] int8, num, max_pos, seed."""
    rng = np.random.default_rng(sum(map(ord, name)) + 11)
    c = SimpleNamespace(name=name, num=16, max_pos=8, seed=5)
    if name.startswith("n"):
        N = int(name[1:])
        c.labels = rng.choice(np.array([-1, 0, 1, 2], np.int8), (2, N), p=[0.3, 0.4, 0.25, 0.05])  # (2: neither class, ignored)
        if N > 1000:
            c.num, c.max_pos = 256, 128
    elif name == "edges":  # per row: no positives, no negatives, all positives, more wanted than there are candidates, a label 2
        N = 300
        lab = np.full((5, N), -1, np.int8)
        lab[0, ::3] = 0
        lab[1, ::4] = 1
        lab[2, :] = 1
        lab[3, :5], lab[3, 5:9] = 1, 0
        lab[4] = rng.choice(np.array([0, 1, 2], np.int8), N)
        c.labels = lab
    elif name == "rows3":  # identical rows must draw differently
        row = rng.choice(np.array([-1, 0, 1], np.int8), 1025)
        c.labels = np.stack([row, row, row])
    else:  # a seed >= 2^32; SEED_SAME_FOLD folds to the same word and must draw the same
        c.labels = rng.choice(np.array([-1, 0, 1], np.int8), (2, 1025))
        c.seed = SEED_HI
    c.labels = np.ascontiguousarray(c.labels, np.int8)
    return c


SEED_HI = (0x1234 << 32) | 0x0BADF00D
SEED_SAME_FOLD = fold_seed(SEED_HI)  # a 32-bit seed with the same folded word
SEED_SAME_LOW = SEED_HI & 0xFFFFFFFF  # the same low word: another draw

SAMPLE_ROI_CASES = ["counts", "n1", "n1025", "n2048"]


def sample_rois_case(name: str):
    rng = np.random.default_rng(sum(map(ord, name)) + 3)
    c = SimpleNamespace(name=name, K=2, num=32, max_fg=8, seed=(7 << 32) | 9)
    if name == "counts":
        # images: box_count 0 | 1 | N | N+3 | G = 0 | G = 0 with match_label 1 | foreground below max_fg | background too short to fill num
        B, N, Gmax = 8, 200, 4
        c.box_count = np.array([0, 1, N, N + 3, N, N, N, 20], np.int32)
        c.gt_count = np.array([2, 2, 4, 3, 0, 0, 2, 2], np.int32)
        c.match_label = (rng.random((B, N)) < 0.3).astype(np.int8)  # ~60 foreground of 200: above max_fg
        c.match_label[5] = 1
        c.match_label[6] = 0
        c.match_label[6, [3, 50, 120]] = 1  # 3 foreground: below max_fg
        c.match_label[7, :20] = (np.arange(20) % 2)  # 10 fg (-> 8) + 10 bg: 18 < num
    else:
        N = int(name[1:])
        B, Gmax = 2, 4
        c.box_count = np.array([N, max(N - 1, 0)], np.int32)
        c.gt_count = np.array([4, 1], np.int32)
        c.match_label = (rng.random((B, N)) < 0.3).astype(np.int8)
        c.num, c.max_fg = (32, 8) if N < 1000 else (512, 128)
    c.boxes = (rng.integers(0, 400, (B, N, 4)) / 4).astype(f32)
    c.gt_boxes = (rng.integers(0, 400, (B, Gmax, 4)) / 4).astype(f32)
    c.gt_classes = rng.integers(0, c.K, (B, Gmax)).astype(np.int32)
    c.matched_idx = np.stack([rng.integers(0, max(1, min(int(g), Gmax)), N) for g in c.gt_count]).astype(np.int32)
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------------------------------------
def get_deltas(src: np.ndarray, tgt: np.ndarray, w) -> np.ndarray:
    """Box2BoxTransform.get_deltas, [n,4] x [n,4] -> [n,4] float64: every operation in np.float32 in the kernel's order, except the
    logarithm, taken in float64 of the float32 ratio (so dx, dy are the kernel's bits and dw, dh its targets before logf's error)."""
    src, tgt = np.asarray(src, f32), np.asarray(tgt, f32)
    w = [f32(x) for x in w]
    h = f32(0.5)
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    sx, sy = src[:, 0] + h * sw, src[:, 1] + h * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tx, ty = tgt[:, 0] + h * tw, tgt[:, 1] + h * th
    with np.errstate(divide="ignore", invalid="ignore"):
        dx, dy = (w[0] * (tx - sx)) / sw, (w[1] * (ty - sy)) / sh
        rw, rh = tw / sw, th / sh
        assert dx.dtype == f32 and rw.dtype == f32
        return np.stack([dx.astype(np.float64), dy.astype(np.float64), float(w[2]) * np.log(rw.astype(np.float64)),
                         float(w[3]) * np.log(rh.astype(np.float64))], 1)


SIGN_MARGIN = 4 * 2.0 ** -23  # relative to |target|: logf's 2 ulp + the product's rounding, doubled


def _sign(df, variant):
    s = np.sign(df)
    return np.where(df == 0, 1.0, s) if variant == "sign0_plus" else s


def level_anchors(c, l: int) -> np.ndarray:
    """[Hf*Wf*A, 4] float32 in (y, x, a) order: cell anchor + (x*stride, y*stride), added in float32."""
    Hf, Wf, st = c.levels[l]
    ys, xs = np.meshgrid(np.arange(Hf), np.arange(Wf), indexing="ij")
    sh = np.stack([xs * st, ys * st, xs * st, ys * st], -1).astype(f32)  # [Hf,Wf,4]
    return (c.cell_anchors[l][None, None, : c.A, :] + sh[:, :, None, :]).astype(f32).reshape(-1, 4)


def rpn_loss64(c, variant: str | None = None):
    """Case c -> result with loss[2] float64 (cls, loc), abs[2] (the sums of magnitudes of the added pieces), nterm (fp32 additions on
    the longest per-thread chain, per loss) and per level: glogit [B,Hf,Wf,A] float64, p64, t, gdelta [B,Hf,Wf,A,4] (sign / normalizer
    as float32), df [B,Hf,Wf,A,4] float64 with its target magnitude tgmag (NaN off the positives)."""
    B, A = c.B, c.A
    norm = float(f32(c.normalizer))
    r = SimpleNamespace(loss=np.zeros(2), abs=np.zeros(2), glogit=[], p64=[], t=[], gdelta=[], df=[], tgmag=[], nterm=[0, 0])
    off = 0
    inv32 = f32(1) / f32(c.normalizer)
    for l, (Hf, Wf, st) in enumerate(c.levels):
        n = Hf * Wf * A
        lab = c.labels[:, off : off + n].astype(np.int64)
        mi = c.matched_idx[:, off : off + n]
        h = c.heads[l].astype(np.float64)
        z = h[..., :A].reshape(B, n)
        live = (lab != -2) if variant == "ignored_counted" else (lab >= 0)
        t = np.where(lab == 1, 1.0, 0.0)
        sp = np.log1p(np.exp(-np.abs(z)))
        term = np.maximum(z, 0) - z * t + sp
        r.loss[0] += term[live].sum()
        r.abs[0] += (np.maximum(z, 0) + np.abs(z * t) + sp)[live].sum()
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-z))
        r.glogit.append(np.where(live, (p - t) / norm, 0.0).reshape(B, Hf, Wf, A))
        r.p64.append(np.where(live, p, 0.0).reshape(B, Hf, Wf, A))
        r.t.append(np.where(live, t, 0.0).reshape(B, Hf, Wf, A))
        anc = level_anchors(c, l)
        pos = lab == 1
        gd, df, tm = np.zeros((B, n, 4), f32), np.full((B, n, 4), np.nan), np.full((B, n, 4), np.nan)
        hd = h[..., A : 5 * A].reshape(B, n, 4)
        for b in range(B):
            ids = np.nonzero(pos[b])[0]
            if len(ids):
                tg = get_deltas(anc[ids], c.gt_boxes[b, mi[b, ids]], c.weights)
                d = hd[b, ids] - tg
                df[b, ids], tm[b, ids] = d, np.abs(tg)
                gd[b, ids] = (_sign(d, variant).astype(f32) * inv32).astype(f32)
                r.loss[1] += np.abs(d).sum()
                r.abs[1] += (np.abs(hd[b, ids]) + np.abs(tg)).sum()
        r.gdelta.append(gd.reshape(B, Hf, Wf, A, 4))
        r.df.append(df.reshape(B, Hf, Wf, A, 4))
        r.tgmag.append(tm.reshape(B, Hf, Wf, A, 4))
        cells = B * Hf * Wf
        blocks = min(LOSS_BLOCKS, -(-cells // LOSS_THREADS))
        per_thread = -(-cells // (blocks * LOSS_THREADS))
        r.nterm = [max(r.nterm[0], per_thread * A), max(r.nterm[1], per_thread * A * 4)]
        off += n
    assert off == c.labels.shape[1]
    r.loss /= norm
    r.scale = 1.0 / norm
    return r


def box_loss64(c, variant: str | None = None):
    """Case c -> result with loss[2] float64, abs[2], nterm, scale = 1/live, glogit [M,K+1] float64, p64, t, lse, logse, gdelta
    [M,4K] float32, df [M,4] (NaN off the foreground), tgmag, live [M] bool."""
    M, K = c.M, c.K
    pred = c.pred.astype(np.float64)
    live = np.ones(M, bool)
    if c.count is not None:
        cnt = np.minimum(c.count, c.R)
        live = (np.arange(M) % c.R) < np.repeat(cnt, c.R)
    nlive = max(int(live.sum()), 1)
    div = float(M) if variant == "box_div_M" else float(nlive)
    inv32 = f32(1) / f32(div)
    sc = pred[:, : K + 1]
    mx = sc.max(1)
    se = np.exp(sc - mx[:, None]).sum(1)
    lse = mx + np.log(se)
    cls = c.cls.astype(np.int64)
    t = np.zeros((M, K + 1))
    t[np.arange(M), cls] = 1.0
    p = np.exp(sc - lse[:, None])
    r = SimpleNamespace(live=live, scale=1.0 / div, lse=lse, logse=np.log(se))
    r.glogit = np.where(live[:, None], (p - t) / div, 0.0)
    r.p64, r.t = np.where(live[:, None], p, 0.0), np.where(live[:, None], t, 0.0)
    r.loss, r.abs = np.zeros(2), np.zeros(2)
    r.loss[0] = (lse - sc[np.arange(M), cls])[live].sum() / div
    # pieces: mx, log(se), the class's score, and 1 for the relative error of se, which enters log(se) as an absolute one
    r.abs[0] = (np.abs(mx) + np.abs(np.log(se)) + np.abs(sc[np.arange(M), cls]) + 1.0)[live].sum()
    fg = live & (cls >= 0) & (cls < K)
    ids = np.nonzero(fg)[0]
    r.gdelta, r.df, r.tgmag = np.zeros((M, 4 * K), f32), np.full((M, 4), np.nan), np.full((M, 4), np.nan)
    if len(ids):
        tg = get_deltas(c.boxes[ids], c.gt_boxes[ids], c.weights)
        col = K + 1 + cls[ids, None] * 4 + np.arange(4)[None]
        hd = pred[ids[:, None], col]
        d = hd - tg
        r.df[ids], r.tgmag[ids] = d, np.abs(tg)
        r.gdelta[ids[:, None], col - (K + 1)] = (_sign(d, variant).astype(f32) * inv32).astype(f32)
        r.loss[1] = np.abs(d).sum() / div
        r.abs[1] = (np.abs(hd) + np.abs(tg)).sum()
    blocks = min(LOSS_BLOCKS, -(-M // LOSS_THREADS))
    per_thread = -(-M // (blocks * LOSS_THREADS))
    r.nterm = [per_thread, per_thread * 4]
    return r


# The law: roundings counted from the kernels' source.
K_SIGMOID = 2 * ULP_EXP + 4  # expf (its error passes through 1/(1+e) at most once), 1 + e, the division, sg - t, / normalizer
TREE = 8                     # the 256-thread tree: 8 additions on every partial's path
KP_BCE = 2 * ULP_EXP + 2 * ULP_LOG1P + 2 + 2   # expf, log1pf, the two additions of a term; float(1/normalizer) and the final cast
KP_L1 = 2 * ULP_LOG + 1 + 1 + 3                # logf, its weight, h - target; the scale (rounded twice in the box kernel) and the final cast


def k_softmax(K, lse, logse, score):
    """Roundings of g = (expf(score - lse) - t) * inv, lse = mx + logf(sum expf(score_c - mx)), per element.  A rounding of a sum
    that feeds expf is an absolute error of the exponent, i.e. a relative error of p of that sum's magnitude in units of u."""
    se = 2 * K + 2 * ULP_EXP + 1  # sum of K+1 exponentials: K additions, their expf and (score_c - mx)'s rounding weighted by e^-d d <= 1/e each
    return np.ceil(np.abs(lse) + 2 * ULP_LOG * np.abs(logse) + se + np.abs(score - lse) + 2 * ULP_EXP + 3)


def kp_ce(K):
    return (2 * K + 2 * ULP_EXP + 1) + 2 * ULP_LOG + 2 + 3


def grad_bound(k, p64, t, scale):
    return gamma(k) * (p64 + t) * abs(scale) + 4 * DENORM


def loss_bound(n, kp, sum_abs, scale):
    return gamma(n + TREE + kp) * sum_abs * abs(scale) + DENORM


CELL = np.array([(-4, -2, 4, 2), (-8, -4, 8, 4), (-16, -8, 16, 8)], f32)  # power-of-two sides: dx, dy and the log's ratio are exact

RPN_CASES = {
    # name: (A, CH, B, [(Hf, Wf, stride)], mode)
    "a1_ch5_l2": (1, 5, 2, [(5, 7, 8), (2, 3, 16)], ""),
    "a2_ch16_l5": (2, 16, 3, [(7, 9, 4), (4, 5, 8), (3, 3, 16), (2, 2, 32), (1, 1, 64)], ""),
    "a3_ch15_l2_nopos": (3, 15, 2, [(6, 5, 8), (3, 3, 16)], "nopos"),       # image 1 has no positive
    "a3_ch20_big": (3, 20, 1, [(129, 128, 4), (2, 2, 8)], ""),              # 16 512 cells: past 64 x 256 threads
    "a1_ch8_ignored": (1, 8, 2, [(4, 4, 8), (2, 2, 16)], "ignored"),        # every anchor ignored
    "a3_ch15_ratio": (3, 15, 2, [(5, 4, 8), (2, 3, 16)], "ratio"),          # sides 24 / 12: divisions that round (not exact in float64 terms)
}
SPECIAL_LOGITS = (0.0, 88.0, -88.0, 104.0, -104.0)
TINY = float(np.nextafter(f32(0), f32(1)))


def rpn_case(name: str):
    A, CH, B, levels, mode = RPN_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    L, Gmax = len(levels), 8
    c = SimpleNamespace(name=name, A=A, CH=CH, B=B, levels=levels, Gmax=Gmax, weights=(1.0, 1.0, 1.0, 1.0), normalizer=float(8 * B),
                        dyadic=mode != "ratio")
    c.cell_anchors = np.stack([(CELL if mode != "ratio" else CELL * f32(1.5)) * f32(2 ** l) for l in range(L)]).astype(f32)  # [L,3,4]
    Atotal = sum(h * w * A for h, w, _ in levels)
    c.labels = rng.choice(np.array([-1, 0, 1], np.int8), (B, Atotal), p=[0.4, 0.35, 0.25])
    if mode == "nopos":
        c.labels[1][c.labels[1] == 1] = 0
    c.labels[0, [1, 4, 7]] = 1  # (level 0 of image 0 always has the three positives the exact-zero targets are planted on)
    if mode == "ignored":
        c.labels[:] = -1
    c.labels = np.ascontiguousarray(c.labels, np.int8)
    c.matched_idx = rng.integers(0, 4, (B, Atotal)).astype(np.int32)
    xy = rng.integers(0, 256, (B, Gmax, 2)) / 4
    wh = rng.integers(4, 256, (B, Gmax, 2)) / 4
    c.gt_boxes = np.concatenate([xy, xy + wh], 2).astype(f32)
    c.heads = [(rng.standard_normal((B, h, w, CH)) * 3).astype(f32) for h, w, _ in levels]
    # special logits on live anchors of level 0, image 0
    Hf, Wf, _ = levels[0]
    n0 = Hf * Wf * A
    live0 = np.nonzero(c.labels[0, :n0] >= 0)[0]
    h0 = c.heads[0][0].reshape(Hf * Wf, CH)
    for j, ai in enumerate(live0[: 2 * len(SPECIAL_LOGITS)]):
        h0[ai // A, ai % A] = SPECIAL_LOGITS[j % len(SPECIAL_LOGITS)]
    # positives whose ground truth IS their anchor (slots 4..6): targets exactly 0; head deltas 0, one float above, one float below
    c.zero_rows = []
    pos0 = np.nonzero(c.labels[0, :n0] == 1)[0]
    anc = level_anchors(c, 0)
    for j, ai in enumerate(pos0[:3]):
        c.gt_boxes[0, 4 + j] = anc[ai]
        c.matched_idx[0, ai] = 4 + j
        d = [(0.0, 0.0, 0.0, 0.0), (TINY, -TINY, TINY, -TINY), (-TINY, TINY, 0.0, TINY)][j]
        h0[ai // A, A + (ai % A) * 4 : A + (ai % A) * 4 + 4] = d
        c.zero_rows.append((int(ai), d))
    return c


BOX_CASES = {
    # name: (K, pitch, M, R, count)
    "k1_min_m1": (1, 6, 1, 0, None),
    "k2_pad_m257": (2, 16, 257, 0, None),
    "k1_pad_m16385": (1, 8, 16385, 0, None),                 # 65 blocks wanted: the 64-block cap is crossed
    "k2_min_ragged": (2, 11, 256, 64, (0, 31, 64, 71)),      # count 0 | mid | R | R + 7
    "k2_pad_ragged_dead": (2, 12, 24, 8, (0, 0, 0)),         # no live row at all: both losses and every gradient exactly 0
}


def box_case(name: str):
    K, pitch, M, R, count = BOX_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 2)
    c = SimpleNamespace(name=name, K=K, pitch=pitch, M=M, R=R, count=None if count is None else np.array(count, np.int32),
                        weights=(10.0, 10.0, 5.0, 5.0), dyadic=True)
    c.pred = (rng.standard_normal((M, pitch)) * 2).astype(f32)
    c.cls = (np.arange(M) % (K + 1)).astype(np.int32)  # every value in [0, K]
    if M > 1:
        c.cls[1:] = rng.permutation(c.cls[1:])
    # logit spreads up to 80, at both ends of the scale
    sp = rng.choice(np.array([1.0, 10.0, 40.0]), M)
    c.pred[:, : K + 1] = np.clip(c.pred[:, : K + 1] * sp[:, None].astype(f32), -40, 40)
    wide = np.arange(M) % 7 == 3
    c.pred[wide, : K + 1] = np.clip(c.pred[wide, : K + 1], -80, 0)
    c.pred[wide, 0], c.pred[wide, K] = 0.0, -80.0
    wide2 = np.arange(M) % 11 == 5
    c.pred[wide2, 0], c.pred[wide2, K] = 40.0, -40.0
    xy = rng.integers(0, 512, (M, 2)) / 4
    wh = 2.0 ** rng.integers(2, 7, (M, 2))  # power-of-two sides
    c.boxes = np.concatenate([xy, xy + wh], 1).astype(f32)
    gxy = xy + rng.integers(-16, 17, (M, 2)) / 4
    gwh = rng.integers(4, 320, (M, 2)) / 4
    c.gt_boxes = np.concatenate([gxy, gxy + gwh], 1).astype(f32)
    # foreground rows whose ground truth IS their box: targets exactly 0; deltas 0 / one float above / below
    c.zero_rows = []
    fg = np.nonzero(c.cls < K)[0]
    if c.count is not None:
        fg = fg[(fg % R) < np.minimum(c.count, R)[fg // R]]
    for j, r in enumerate(fg[:3]):
        c.gt_boxes[r] = c.boxes[r]
        d = [(0.0, 0.0, 0.0, 0.0), (TINY, -TINY, TINY, -TINY), (-TINY, TINY, 0.0, TINY)][j]
        c.pred[r, K + 1 + c.cls[r] * 4 : K + 5 + c.cls[r] * 4] = d
        c.zero_rows.append((int(r), d))
    return c
