"""Float64 / exact references of the detection tail: a3d_paste_lsq, a3d_plane_offset_dense(_u8) (csrc/heads_post.hip),
a3d_detections_pack and a3d_mask_rle (csrc/pack.hip), with the bounds they are held to and the deterministic case lists.
Plain numpy; imported by tests/test_post_ref_host.py (CPU) and tests/test_gpu_post.py (GPU).

THE PASTE.  paste64 is the bilinear sample of the zero-padded probability map at  ix = ((px + .5 - x0) / (x1 - x0)) MS - .5  (and iy
alike), in float64 from the float32 inputs.  A pasted mask is a THRESHOLD of that value, and the fp32 paths (ATen's grid_sample, the
kernel) round the coordinate, so a pixel whose float64 value lies within band(MS) of the threshold may fall on either side: it is
"undecided".  Everywhere else the masks must be equal.  The band is counted, not fitted (u = 2^-24, q = (px + .5 - x0) / (x1 - x0),
|q| <= Q = 1 + 1 / (2 MS) wherever a sample is taken):

    q in fp32: one rounding each for  px + .5 - x0,  x1 - x0  and the division                         |dq| <= gamma(3) Q
    t = 2 q - 1: one rounding, |t| <= 2 Q;    t + 1: one rounding, |t + 1| <= 2 Q                        2 u Q each
    ix = ((t + 1) MS - 1) / 2 as one fused multiply-add (or (t + 1) (MS / 2) - .5): one rounding        u |ix| <= u MS
    =>  |d ix| <= (MS / 2) (2 gamma(3) Q + 4 u Q) + u MS  <=  (6 MS + 3) u  to first order

For probabilities in [0, 1] the sample value is 1-Lipschitz in ix and in iy, so the coordinates move it by at most 2 (6 MS + 3) u.
The four-tap sum adds: w = ix - floor(ix) is exact for ix >= 0 and one rounding for ix in (-1, 0); e = 1 - w is one rounding; the same
for the rows (4 u, each weight 1-Lipschitz); a weight product, the product with the value and at most three additions or fused steps per
tap (gamma(5) on a sum of weights of 1): 10 u in all.  band(MS) = gamma(12 MS + 16), 2.1e-5 at MS = 28.

THE PLANE FIT.  plane_fit64 is arti_vis.py:125-149 in float64: p = (x, -z, y) of the input normal, n = p / max(|p|, 1e-8),
off = mean over the mask of n . (ray depth) with rays ((px - cx) / f, (py - cy) / f, 1), result n off swapped back (x, z, -y).
The kernels form every pixel's term in fp32 and sum in double.  Roundings of a term  n0 X + n1 Y + n2 d:  n_k carries 4 (p.p is three
products and two additions of non-negative terms, gamma(3), halved by the root, which adds one, and the division one more: 3.5 u);
the ray's cast to fp32 1; X = ray d 1; n0 X 1; the two additions 2: at most 9 on the magnitude |n0 X| + |n1 Y| + |n2 d|.  The mean is in
double.  Its cast to fp32 is 1, the product n_k off 1, and n_k brings its own 4 again; |off| <= M = mean(|n0 X| + |n1 Y| + |n2 d|):

    |plane_k - plane64_k| <= gamma(15) |n_k| M

An empty mask returns the input normal itself (M = 0: equality)."""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from roi_ref64 import gamma, law_ratio  # noqa: E402,F401

f32, f64 = np.float32, np.float64
REC_HEAD = 14
PLANE_TERMS = 15
UNDECIDED_CAP = 2000  # at most one undecided pixel in this many pixels of a case


def band(MS):
    return float(gamma(12 * MS + 16))


# ------------------------------------------------------------------------------------------ paste
def _axis(i, MS):
    with np.errstate(invalid="ignore"):
        ok = (i > -1.0) & (i < MS)  # outside the padded map (or NaN): nothing is sampled
    i = np.where(ok, i, -1.0)
    lo = np.floor(i)
    return ok, lo.astype(np.int64) + 1, i - lo  # (index into the map padded with one ring of zeros)


def paste64(mask_prob, boxes, H, W):
    """mask_prob [D, MS, MS] fp32, boxes [D, 4] fp32 -> [D, H, W] float64 sample values (bilinear, zeros outside, align_corners=False)."""
    mp = np.asarray(mask_prob, dtype=f32).astype(f64)
    bx = np.asarray(boxes, dtype=f32).astype(f64).reshape(-1, 4)
    D, MS = mp.shape[0], mp.shape[-1]
    pad = np.zeros((D, MS + 2, MS + 2))
    pad[:, 1:-1, 1:-1] = mp
    out = np.zeros((D, H, W))
    px, py = np.arange(W) + 0.5, np.arange(H) + 0.5
    for d in range(D):
        x0, y0, x1, y1 = bx[d]
        with np.errstate(invalid="ignore", divide="ignore"):
            okx, xl, wx = _axis((px - x0) / (x1 - x0) * MS - 0.5, MS)
            oky, yl, wy = _axis((py - y0) / (y1 - y0) * MS - 0.5, MS)
        P, Y, X = pad[d], yl[:, None], xl[None, :]
        v = (P[Y, X] * (1 - wx) + P[Y, X + 1] * wx) * (1 - wy)[:, None] + (P[Y + 1, X] * (1 - wx) + P[Y + 1, X + 1] * wx) * wy[:, None]
        out[d] = np.where(oky[:, None] & okx[None, :], v, 0.0)
    return out


def postprocess64(boxes, scores, count, row_offset, mask_prob, H, W, post_score_thresh, mask_thresh, clip=True):
    """The contract of a3d_paste_lsq without the plane: boxes [B, R, 4], scores [B, R], count [B], row_offset [B],
    mask_prob [rows, MS, MS] -> keep [B, R], out_boxes [B, R, 4] fp32, rows [B, R], val [B, R, H, W] float64 (0 in dead slots),
    mask = val >= mask_thresh, undecided = |val - mask_thresh| < band(MS) in live slots."""
    bx = np.asarray(boxes, dtype=f32)
    sc = np.asarray(scores, dtype=f32)
    B, R = sc.shape
    MS = mask_prob.shape[-1]
    cnt = np.minimum(np.asarray(count, dtype=np.int64), R)
    live = np.arange(R)[None, :] < cnt[:, None]
    ob = np.where(live[..., None], bx, f32(0))
    keep = live.copy()
    if clip:
        ob = ob.copy()
        ob[..., 0::2] = np.clip(ob[..., 0::2], f32(0), f32(W))
        ob[..., 1::2] = np.clip(ob[..., 1::2], f32(0), f32(H))
        keep = live & (sc >= f32(post_score_thresh)) & ((ob[..., 2] - ob[..., 0]) > 0) & ((ob[..., 3] - ob[..., 1]) > 0)
    ob = ob.astype(f32)
    rows = np.asarray(row_offset, dtype=np.int64)[:, None] + np.arange(R)[None, :]
    val = np.zeros((B, R, H, W))
    k = np.nonzero(keep)
    if len(k[0]):
        val[k] = paste64(np.asarray(mask_prob)[rows[k]], ob[k], H, W)
    thr = f64(f32(mask_thresh))
    und = (np.abs(val - thr) < band(MS)) & keep[..., None, None]
    return types.SimpleNamespace(keep=keep.astype(np.int32), out_boxes=ob, rows=rows, val=val, mask=(val >= thr) & keep[..., None, None],
                                 undecided=und)


# ------------------------------------------------------------------------------------------ plane fit
def plane_fit64(depth, mask, normal, focal, cx, cy):
    """depth [H, W] fp32, mask [H, W] (non-zero = set), normal [3] fp32; focal, cx, cy as the code under test holds them.
    -> plane [3] float64 in the output axes, mag = mean(|n0 X| + |n1 Y| + |n2 d|), unit = |n| in the output axes, count."""
    d = np.asarray(depth, dtype=f32).astype(f64)
    m = np.asarray(mask) != 0
    nv = np.asarray(normal, dtype=f32).astype(f64)
    p = np.array([nv[0], -nv[2], nv[1]])
    n = p / max(np.sqrt((p * p).sum()), 1e-8)
    c = int(m.sum())
    if c == 0:
        return types.SimpleNamespace(plane=nv, mag=0.0, unit=np.abs(np.array([n[0], n[2], n[1]])), count=0)
    H, W = d.shape
    X = ((np.arange(W, dtype=f64) - f64(cx)) / f64(focal))[None, :] * d
    Y = ((np.arange(H, dtype=f64) - f64(cy)) / f64(focal))[:, None] * d
    off = (n[0] * X + n[1] * Y + n[2] * d)[m].sum() / c
    mag = (np.abs(n[0] * X) + np.abs(n[1] * Y) + np.abs(n[2] * d))[m].sum() / c
    o = n * off
    return types.SimpleNamespace(plane=np.array([o[0], o[2], -o[1]]), mag=float(mag), unit=np.abs(np.array([n[0], n[2], n[1]])), count=c)


def plane_bound(fit):
    return gamma(PLANE_TERMS) * fit.unit * fit.mag


# ------------------------------------------------------------------------------------------ records
def pack_ref(boxes, scores, classes, count, row_offset, keep, planes, rot_axis, tran_axis, mask_prob, MS):
    """-> records [B, R, 14 + MS^2] fp32 and rec_count [B]: the kept rows r < min(count, R) in slot order, then zeros.
    planes is per slot [B, R, 3]; rot_axis [rows, 3], tran_axis [rows, 2] and mask_prob [rows, MS, MS] per compact row; None -> zeros."""
    bx = np.asarray(boxes, dtype=f32)
    B, R = bx.shape[:2]
    rec = REC_HEAD + MS * MS
    out = np.zeros((B, R, rec), dtype=f32)
    n = np.zeros(B, dtype=np.int32)
    for b in range(B):
        for r in range(min(int(count[b]), R)):
            if not keep[b, r]:
                continue
            o = out[b, n[b]]
            row = int(row_offset[b]) + r
            o[0:4] = bx[b, r]
            o[4] = scores[b, r]
            o[5] = f32(classes[b, r])
            if planes is not None:
                o[6:9] = planes[b, r]
            if rot_axis is not None:
                o[9:12] = rot_axis[row]
            if tran_axis is not None:
                o[12:14] = tran_axis[row]
            if mask_prob is not None:
                o[REC_HEAD:] = np.asarray(mask_prob[row]).reshape(-1)
            n[b] += 1
    return out, n


# ------------------------------------------------------------------------------------------ run-length boundaries
def rle_boundaries(mask):
    """mask [H, W] (non-zero = set) -> (column-major positions i >= 1 with m[i] != m[i - 1], ascending; the first pixel as 0 / 1)."""
    flat = (np.asarray(mask) != 0).reshape(-1, order="F")
    return (np.flatnonzero(flat[1:] != flat[:-1]) + 1).astype(np.int64), int(flat[0])


def rle_patterns(H, W, seed=0):
    """[(name, mask [H, W] uint8)]: the mask patterns of the RLE suite."""
    rng = np.random.default_rng(seed + 31 * H + W)
    z = np.zeros((H, W), dtype=np.uint8)
    first, last = z.copy(), z.copy()
    first[0, 0] = 1
    last[H - 1, W - 1] = 1
    yy, xx = np.mgrid[0:H, 0:W]
    # column 0 set from its middle to its end, column 1 set from its top: in the column-major walk the two are ONE run (no boundary
    # at the column's end), which a row-major or per-column scan would split
    wrap = z.copy()
    wrap[H // 2:, 0] = 1
    if W > 1:
        wrap[: max(H // 3, 1), 1] = 1
    return [("empty", z), ("full", z + 1), ("first", first), ("last", last), ("checker", ((yy + xx) & 1).astype(np.uint8)),
            ("wrap", wrap), ("random", (rng.random((H, W)) < 0.4).astype(np.uint8) * 255)]


RLE_SIZES = [(1, 1), (1, 40), (40, 1), (4, 8), (5, 7), (31, 33), (33, 31), (512, 768)]


# ------------------------------------------------------------------------------------------ paste inputs
# The kernel walks H * ceil(W / 16) groups of 16 pixels with 1024 threads.  One group per row; vector stores; odd H; byte stores;
# W < 16; 40 x 64: four groups per row (160 groups, still one pass); 25 x 40: byte stores with H W % 16 != 0 at W > 16 (24 x 40 = 960
# pixels is a multiple of 16: its dead slots are cleared by vectors, and 17 x 13 alone would reach the byte form of that loop);
# 65 x 256 (1040 groups, vector stores) and 72 x 250 (1152 groups, byte stores, a ragged last group): a SECOND pass of the strided
# loop for the first threads, none for the rest -- the group decode, the per-thread sums and the stores of a second pass.
PASTE_SIZES = [(24, 16), (24, 48), (25, 48), (24, 40), (17, 13), (40, 64), (25, 40), (65, 256), (72, 250)]
assert max(h * -(-w // 16) for h, w in PASTE_SIZES[:-2]) <= 1024 < min(h * -(-w // 16) for h, w in PASTE_SIZES[-2:])
POST_THRESH = 0.1


def box_cases(H, W):
    """[(class, box, score)] for an H x W image."""
    below = float(np.nextafter(f32(POST_THRESH), f32(0)))
    return [
        ("inside", [0.2 * W + 0.3, 0.25 * H + 0.1, 0.7 * W + 0.4, 0.8 * H - 0.2], 0.9),
        ("edge_left", [-0.3 * W, 0.2 * H, 0.35 * W + 0.2, 0.7 * H], 0.8),
        ("edge_right", [0.6 * W + 0.1, 0.3 * H, 1.3 * W, 0.9 * H], 0.7),
        ("edge_top", [0.3 * W, -0.4 * H, 0.8 * W, 0.45 * H + 0.3], 0.6),
        ("edge_bottom", [0.1 * W, 0.55 * H, 0.6 * W, 1.5 * H], 0.5),
        ("outside_right", [W + 2.0, 0.2 * H, W + 9.0, 0.6 * H], 0.95),  # clipped empty
        ("outside_above", [2.0, -9.0, W - 2.0, -1.0], 0.95),
        ("subpixel", [0.5 * W + 0.2, 0.1 * H, 0.5 * W + 0.9, 0.9 * H], 0.4),
        ("cover", [-0.1 * W - 1.0, -0.1 * H - 1.0, 1.1 * W + 1.0, 1.1 * H + 1.0], 0.3),
        ("whole", [0.0, 0.0, float(W), float(H)], 0.2),
        ("centres", [2.5, 3.5, W - 3.5, H - 2.5], 0.15),  # every edge on a pixel centre
        ("at_thresh", [1.3, 2.1, W - 2.2, H - 1.7], float(f32(POST_THRESH))),
        ("below_thresh", [1.3, 2.1, W - 2.2, H - 1.7], below),
    ]


def make_prob(n, MS, seed):
    """[n, MS, MS] fp32 in [0, 1]: uniform noise and sigmoid blobs alternate; the map of row 3 lies wholly below one half."""
    rng = np.random.default_rng(seed)
    out = rng.random((n, MS, MS))
    g = (np.arange(MS) + 0.5) / MS
    for k in range(1, n, 2):
        cy, cx, s = rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7), rng.uniform(0.15, 0.4)
        r2 = (g[:, None] - cy) ** 2 + (g[None, :] - cx) ** 2
        out[k] = 1.0 / (1.0 + np.exp(-(1.0 - r2 / (s * s)) * 4.0))
    if n > 3:
        out[3] *= 0.49
    return out.astype(f32)


def paste_inputs(H, W, MS, B, R, seed=0):
    """Slots, ragged counts (a 0 and a value above R where B allows), a row_offset that is not b R, maps, normals and depth."""
    rng = np.random.default_rng(1000 * seed + 7 * H + W + MS)
    cases = box_cases(H, W)
    boxes = np.tile(np.array([1.0, 1.0, W - 1.0, H - 1.0], dtype=f32), (B, R, 1))  # dead slots hold a live-looking box and score
    scores = np.full((B, R), 0.99, dtype=f32)
    names = np.full((B, R), "", dtype=object)
    count = np.array([R + 3, 0, R - 3][:B] if B > 1 else [1], dtype=np.int32)
    k = 0
    for b in range(B):
        for r in range(min(int(count[b]), R)):
            names[b, r], bx, sc = cases[(k + seed) % len(cases)]
            boxes[b, r], scores[b, r] = np.array(bx, dtype=f32), f32(sc)
            k += 1
    row_offset = (np.cumsum(np.minimum(count, R)) - np.minimum(count, R) + 2).astype(np.int32)  # compact rows behind two spare ones
    rows = int(row_offset[-1]) + R
    prob = make_prob(rows, MS, seed + 5)
    nrm = rng.standard_normal((rows, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[2] *= 3.0  # not unit: the kernel normalises
    nrm[4 % rows] = [0.0, 0.0, 1.0]
    depth = rng.uniform(0.5, 5.0, (B, H, W)).astype(f32)
    return types.SimpleNamespace(boxes=boxes, scores=scores, count=count, row_offset=row_offset, prob=prob, normals=nrm.astype(f32),
                                 depth=depth, names=names, rows=rows)


def paste_seeds(H, W, br):
    """The launches of one case of the paste grid: a 1 x 1 launch per box class, or the one batch that holds them all."""
    return range(len(box_cases(H, W))) if tuple(br) == (1, 1) else (0,)


def intrinsics(H, W):
    """A focal length of the order of the image, so that the rays are O(1) and a wrong pixel index moves the fit far past the law."""
    return float(f32(0.6 * W + 0.37)), float(f32((W - 1) / 2.0 + 0.25)), float(f32((H - 1) / 2.0 - 0.125))
