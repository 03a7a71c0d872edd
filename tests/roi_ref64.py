"""Float64 reference of the FPN ROI pooler (csrc/roi_align.hip) with the kernel's fp32 geometry, the error law the pooler is held
to, the walk the kernel takes for a ROI, and the deterministic case lists.  Plain numpy; imported by tests/test_roi_ref64_host.py
(CPU) and tests/test_gpu_roi_geometry.py (GPU).

GEOMETRY.  Everything that decides WHERE a sample falls is computed in np.float32 in torchvision's operation order -- the level, x1, y1,
rw, rh, bw, bh, gh, gw, count, every sample coordinate  v = (start + p * bsz) + ((i + .5) * bsz) / g,  its skip (v < -1 or v > L) and
clamp (v <= 0 -> 0; lo >= L - 1 -> lo = hi = L - 1, v = lo) decisions, lo, hi, l = v - lo, h = 1 - l.  roi_align.hip is compiled with
-ffp-contract=off, so these are the kernel's values bit for bit.

ARITHMETIC.  y64[bin, c] = (1 / count) * sum over samples, sum over corners (double)w * f in float64, with w the product of the fp32
l / h of the two axes.  A bilinear weight factorises, so the sum is evaluated as  sum_rows sum_cols WY[row] WX[col] f[row][col]  with
WY / WX the float64 sums of the fp32 l / h (equal to the per-sample form up to float64 rounding, 2^-29 of the law's unit).
A[bin, c] is the same sum over |f|: the magnitude the law scales with.  The backward is the float64 adjoint with the same weights.

THE LAW (u = 2^-24, gamma(n) = n u / (1 - n u); nothing fitted).  A table entry is a sum of at most g terms (each h = 1 - l carries one
rounding, g - 1 additions; the first addition is to zero), a cell weight is one product wy * wx, its product with f is one more,
a bin is a sum of n such products (n - 1 additions) and one division:

    bin-by-bin walks (cells <= NC, cells > NC, the C != 256 loop):   |y - y64| <= gamma(gh + gw + n + 4) A,   n = ny * nx cells of the bin
    per-sample "general" path:  w = hy * hx, w * f, three additions per sample, gh * gw additions, one division -- gh gw + 6 roundings,
                                held to the same form with n = 4 gh gw
    rolling-window walk:  column sum  c = sum_u wy[u] f[u]  over the at most RMAX = 8 cell rows of the wave's bin-row pair (one product,
                          at most RMAX - 1 additions; rows outside the bin carry weight 0 and add exactly), then acc += wx * c over the
                          bin's nx columns (one product, at most nx - 1 additions), one division:  gh + gw + nx + 9 roundings, held to
                          gamma(gh + gw + RMAX + nx + 4) A
    backward, per cell:  a term is  (wy * wx) * (g / count).  Scatter form: two table entries (gh + gw), three roundings of its own, and
                         the atomics add N terms in any order (N - 1 additions onto a zeroed cell): N + gh + gw + 2.  Gather form: the
                         same tables and division, then per ROI  t[k] = fma(wx, g', t[k])  over the cx bin columns that touch the cell's
                         column and  acc = fma(wy, t, acc)  over the cy bin rows that touch its row: cx + cy <= cx cy + 1 roundings per
                         ROI, i.e. N + (number of ROIs on the cell) in all.  Both are held to
                         gamma(N + ROIs + max(gh + gw) + 2) Aabs,   Aabs = sum |w| |g| / count
                         with N counted once per pass of the scatter form's multi-pass tables that can reach the cell (at most two per
                         axis).  This is the worst case over every summation order, so it covers the atomics.
"""
import types

import numpy as np

f32 = np.float32
U = 2.0 ** -24
KMAX, PMAX, NC, RMAX = 16, 16, 9, 8
VARIANTS = ("shift_sample", "skip_L", "count_nomax", "table_g", "clamp_off_by_one")


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def assign_level(boxes, L=4):
    """roi_align.hip's statement of the FPN level: floor(4 + log2(sqrt(area) / 224 + 1e-8)) clamped to [2, 2 + L - 1], minus 2, in fp32
    (fmaxf / fminf drop a NaN, so a box with negative area lands on level 0)."""
    b = np.asarray(boxes, dtype=f32).reshape(-1, 4)
    with np.errstate(invalid="ignore", divide="ignore"):
        size = np.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
        lvf = np.floor(f32(4) + np.log2(size / f32(224) + f32(1e-8)))
    lvf = np.fmin(np.fmax(lvf, f32(2)), f32(2 + L - 1))
    return lvf.astype(np.int64) - 2


def _axis(start, bsz, g, L, P, variant=None, shift=False):
    """One axis of one ROI.  Returns the fp32 per-sample record and the per-bin-row tables (base cell, cell count, dense float64 weights)."""
    gg = max(int(g), 0)
    p = np.arange(P, dtype=f32)[:, None]
    i = np.arange(gg, dtype=f32)[None, :]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        v = (start + p * bsz) + ((i + f32(0.5)) * bsz) / f32(g)
    v = v.astype(f32)
    if shift and gg:
        v[P // 2, 0] = v[P // 2, 0] + f32(1e-4)
    skip = (v < f32(-1.0)) | (v >= f32(L) if variant == "skip_L" else v > f32(L)) | ~np.isfinite(v)
    vc = np.where(skip | (v <= 0), f32(0), v).astype(f32)
    lo = vc.astype(np.int64)
    edge = L - 2 if variant == "clamp_off_by_one" and L >= 2 else L - 1
    cl = lo >= edge
    lo = np.where(cl, edge, lo)
    hi = np.where(cl, edge, lo + 1)
    vc = np.where(cl, f32(edge), vc).astype(f32)
    l = (vc - lo.astype(f32)).astype(f32)
    h = (f32(1.0) - l).astype(f32)
    live = ~skip
    W = np.zeros((P, L), dtype=np.float64)
    pi = np.broadcast_to(np.arange(P)[:, None], lo.shape)
    np.add.at(W, (pi[live], lo[live]), h[live].astype(np.float64))
    np.add.at(W, (pi[live], hi[live]), l[live].astype(np.float64))
    base = np.zeros(P, dtype=np.int64)
    n = np.zeros(P, dtype=np.int64)
    for q in range(P):
        idx = np.nonzero(live[q])[0]
        if len(idx):
            base[q] = lo[q, idx[0]]
            n[q] = hi[q, idx[-1]] - base[q] + 1
            if variant == "table_g":  # a table of g entries instead of g + 1
                W[q, base[q] + gg:] = 0.0
    return types.SimpleNamespace(v=v, skip=skip, lo=lo, hi=hi, l=l, h=h, W=W, base=base, n=n)


def roi_geometry(box, sizes, scales, P, ratio, aligned, variant=None):
    """box [4] fp32, sizes [(H, W)] and scales per level -> the kernel's fp32 geometry of the ROI and its weight tables."""
    b = np.asarray(box, dtype=f32)
    L = len(sizes)
    lv = int(assign_level(b, L)[0])
    H, W = sizes[lv]
    s = f32(scales[lv])
    off = f32(0.5) if aligned else f32(0.0)
    x1, y1, x2, y2 = b[0] * s - off, b[1] * s - off, b[2] * s - off, b[3] * s - off
    rw, rh = f32(x2 - x1), f32(y2 - y1)
    if not aligned:
        rw, rh = max(rw, f32(1.0)), max(rh, f32(1.0))
    bh, bw = f32(rh / f32(P)), f32(rw / f32(P))
    gh = int(ratio) if ratio > 0 else int(np.ceil(f32(rh / f32(P))))
    gw = int(ratio) if ratio > 0 else int(np.ceil(f32(rw / f32(P))))
    prod = gh * gw
    count = f32(prod) if variant == "count_nomax" else f32(max(prod, 1))
    g = types.SimpleNamespace(lv=lv, H=H, W=W, x1=x1, y1=y1, rw=rw, rh=rh, bw=bw, bh=bh, gh=gh, gw=gw, count=count, P=P, ratio=ratio)
    g.y = _axis(y1, bh, gh, H, P, variant)
    g.x = _axis(x1, bw, gw, W, P, variant, shift=(variant == "shift_sample"))
    # the table path holds KMAX cells from the first sample's low cell on; a fixed ratio is admitted to it by the span of its lattice
    fits = True
    if ratio > 0:
        with np.errstate(over="ignore", invalid="ignore"):
            fits = bool(f32(gh - 1) * f32(bh / f32(gh)) + f32(3.0) < f32(KMAX)) and bool(f32(gw - 1) * f32(bw / f32(gw)) + f32(3.0) < f32(KMAX))
    g.separable = gh < KMAX and gw < KMAX and P <= PMAX and fits
    if g.separable:
        assert g.y.n.max(initial=0) <= KMAX and g.x.n.max(initial=0) <= KMAX, "a weight table of more than KMAX cells on the table path"
    g.cells = g.y.n[:, None] * g.x.n[None, :]  # cells read per bin on the table path
    return g


def walk_class(g, C=256, rolling=True):
    """The walk roi_align_fpn_kernel takes for this ROI: 'general', 'rolling', or the bin-by-bin form ('cells<=NC' / 'cells>NC') and,
    where the rolling walk was asked for (7 x 7, C = 256) and refused, the reason.  The rolling walk needs: every bin row and column with
    at least one sample; at most three bins on any cell column (bin p + 3 starts past the last column of bin p); at most RMAX cell rows
    under each pair of bin rows (0-1, 2-3, 4-5, and 6 alone); windows that do not move backwards."""
    if not g.separable:
        return "general", None
    reason = None
    if rolling and g.P == 7 and C == 256:
        X0, NX, Y0, NY = g.x.base, g.x.n, g.y.base, g.y.n
        ex, ey = X0 + NX - 1, Y0 + NY - 1
        if (NX <= 0).any() or (NY <= 0).any():
            reason = "empty_bin"
        elif (np.diff(X0) < 0).any() or (np.diff(ex) < 0).any() or (np.diff(Y0) < 0).any() or (np.diff(ey) < 0).any():
            reason = "not_monotone"
        elif any(X0[p + 3] <= ex[p] for p in range(4)):
            reason = "four_bins_on_a_column"
        elif any((NY[p] if p == 6 else Y0[p + 1] + NY[p + 1] - Y0[p]) > RMAX for p in (0, 2, 4, 6)):
            reason = "more_than_RMAX_rows"
        else:
            return "rolling", None
    return ("cells<=NC" if g.cells.max(initial=0) <= NC else "cells>NC"), reason


def forward_terms(g, walk):
    """[P, P] number of roundings the law allows a bin (module docstring)."""
    if walk == "general":
        n = np.full((g.P, g.P), 4 * g.gh * g.gw)
    elif walk == "rolling":
        n = np.broadcast_to(RMAX + g.x.n[None, :], (g.P, g.P))
    else:
        n = g.cells
    return max(g.gh, 0) + max(g.gw, 0) + n + 4


def _window(W):
    nz = np.nonzero(W.any(axis=0))[0]
    return (int(nz[0]), int(nz[-1]) + 1) if len(nz) else (0, 0)


def pool_ref(feats, scales, boxes, img, P, ratio, aligned, variant=None):
    """feats: per level float64 [B, H, W, C]; boxes [N, 4] fp32; img [N] -> y64 [N, P, P, C], A [N, P, P, C], geometries."""
    C = feats[0].shape[3]
    sizes = [f.shape[1:3] for f in feats]
    absf = [np.abs(f) for f in feats]
    y = np.zeros((len(boxes), P, P, C))
    A = np.zeros_like(y)
    geoms = []
    for k, box in enumerate(boxes):
        g = roi_geometry(box, sizes, scales, P, ratio, aligned, variant)
        geoms.append(g)
        (ya, yb), (xa, xb) = _window(g.y.W), _window(g.x.W)
        with np.errstate(invalid="ignore", divide="ignore"):
            for dst, src in ((y, feats), (A, absf)):
                if yb > ya and xb > xa:
                    f = src[g.lv][img[k], ya:yb, xa:xb]
                    t = (g.y.W[:, ya:yb] @ f.reshape(yb - ya, -1)).reshape(P, xb - xa, C)
                    dst[k] = np.matmul(g.x.W[None, :, xa:xb], t) / np.float64(g.count)
                else:
                    dst[k] = np.zeros((P, P, C)) / np.float64(g.count)
    return y, A, geoms


def pool_bwd_ref(sizes, scales, boxes, img, dout, B, P, ratio, aligned, variant=None):
    """dout float64 [N, P, P, C] -> per level d64 [B, H, W, C], Aabs, the per-cell term count of the law, geometries."""
    C = dout.shape[3]
    d = [np.zeros((B, h, w, C)) for h, w in sizes]
    Aabs = [np.zeros((B, h, w, C)) for h, w in sizes]
    nbin = [np.zeros((B, h, w), dtype=np.int64) for h, w in sizes]
    nroi = [np.zeros((B, h, w), dtype=np.int64) for h, w in sizes]
    tbl = [np.zeros((B, h, w), dtype=np.int64) for h, w in sizes]
    geoms = []
    for k, box in enumerate(boxes):
        g = roi_geometry(box, sizes, scales, P, ratio, aligned, variant)
        geoms.append(g)
        (ya, yb), (xa, xb) = _window(g.y.W), _window(g.x.W)
        if yb <= ya or xb <= xa:
            continue
        WY, WX = g.y.W[:, ya:yb], g.x.W[:, xa:xb]
        for dst, src in ((d, dout[k]), (Aabs, np.abs(dout[k]))):
            t = np.matmul(WX.T[None], src / np.float64(g.count))  # [P, nx, C]
            dst[g.lv][img[k], ya:yb, xa:xb] += (WY.T @ t.reshape(P, -1)).reshape(yb - ya, xb - xa, C)
        passes = lambda gg: min((max(gg, 1) + KMAX - 2) // (KMAX - 1), 2)
        cy, cx = (WY > 0).sum(0) * passes(g.gh), (WX > 0).sum(0) * passes(g.gw)
        hit = cy[:, None] * cx[None, :]
        nbin[g.lv][img[k], ya:yb, xa:xb] += hit
        nroi[g.lv][img[k], ya:yb, xa:xb] += hit > 0
        tb = tbl[g.lv][img[k], ya:yb, xa:xb]
        np.maximum(tb, np.where(hit > 0, max(g.gh, 0) + max(g.gw, 0), 0), out=tb)
    terms = [nb + nr + tb + 2 for nb, nr, tb in zip(nbin, nroi, tbl)]
    return d, Aabs, terms, geoms


def law_ratio(got, want, bound):
    """max of |got - want| / bound over the elements (0 / 0 counts as 0: an exact zero must be an exact zero); NaN fails."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    if r.size == 0:
        return 0.0
    return float("inf") if np.isnan(r).any() else float(r.max())


# ------------------------------------------------------------------------------------------ deterministic case lists
STRIDES = (4, 8, 16, 32)
SCALES = tuple(1.0 / s for s in STRIDES)
POOLERS = {"box": (7, 0, True), "mask": (14, 2, False), "plane": (14, 0, False)}
FRAMES = {"480x640": (480, 640), "96x128": (96, 128), "61x75": (61, 75)}


def pyramid_sizes(hw):
    return [(-(-hw[0] // s), -(-hw[1] // s)) for s in STRIDES]


def make_pyramid(hw, B, C, seed):
    """Random normal NHWC pyramid, float32; level 1 scaled by 1e3 and level 2 by 1e-3, so no max-normalised metric could hide a level."""
    rng = np.random.default_rng(seed)
    gain = (1.0, 1e3, 1e-3, 1.0)
    return [(rng.standard_normal((B, h, w, C)) * gn).astype(f32) for (h, w), gn in zip(pyramid_sizes(hw), gain)]


def _xyxy(cx, cy, w, h):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]


def is_interior(g):
    """Every sample of the ROI is live and strictly inside (0, L - 1): no skip, no clamp."""
    return all((not ax.skip.any()) and ax.v.size and ax.v.min() > 0 and ax.v.max() < L - 1 for ax, L in ((g.x, g.W), (g.y, g.H)))


def frame_cases(hw, seed=0):
    """[(class name, box)] for a frame of hw pixels: the geometry classes of the four-level pooler."""
    Hh, Ww = hw
    rng = np.random.default_rng(1000 + seed)
    out = []
    add = lambda name, b: out.append((name, [float(v) for v in b]))
    sizes = pyramid_sizes(hw)
    for lv, side in enumerate((40.0, 150.0, 300.0, 520.0)):  # interior boxes of every level the frame holds (rejection-sampled, seeded)
        kept = 0
        for _ in range(200):
            w, h = side * np.exp(rng.uniform(-0.3, 0.3)), side * np.exp(rng.uniform(-0.3, 0.3))
            if kept == 3 or w >= Ww - 2 or h >= Hh - 2:
                continue
            b = _xyxy(rng.uniform(w / 2 + 1, Ww - w / 2 - 1), rng.uniform(h / 2 + 1, Hh - h / 2 - 1), w, h)
            if all(is_interior(roi_geometry(b, sizes, SCALES, *pl)) for pl in POOLERS.values()):
                add("interior", b)
                kept += 1
    if tuple(hw) == (480, 640):  # the coarsest level leaves an interior box of its size hardly any room: placed by hand
        add("interior", [16.0, 40.0, 612.0, 440.0])
    m = 0.3 * min(Hh, Ww)
    for name, (cx, cy) in {"edge_left": (0, Hh / 2), "edge_right": (Ww, Hh / 2), "edge_top": (Ww / 2, 0), "edge_bottom": (Ww / 2, Hh),
                           "corner_tl": (0, 0), "corner_tr": (Ww, 0), "corner_bl": (0, Hh), "corner_br": (Ww, Hh)}.items():
        for f in (1.0, 0.37):
            add(name, _xyxy(cx + rng.uniform(-2, 2), cy + rng.uniform(-2, 2), m * f, m * f * 0.8))
    add("cover", [-0.1 * Ww, -0.1 * Hh, 1.1 * Ww, 1.1 * Hh])
    for name, (x, y) in {"outside_left": (-3 * m, Hh / 2), "outside_right": (Ww + 3 * m, Hh / 2), "outside_top": (Ww / 2, -3 * m),
                         "outside_bottom": (Ww / 2, Hh + 3 * m)}.items():
        add(name, _xyxy(x, y, m, m))
    for _ in range(2):
        x, y = rng.uniform(5, Ww - 5), rng.uniform(5, Hh - 5)
        add("zero_area", [x, y, x, y])
        add("sub_cell", [x, y, x + rng.uniform(0.1, 2.0), y + rng.uniform(0.1, 2.0)])
    add("zero_area", [Ww / 2, Hh / 4, Ww / 2 + 20, Hh / 4])  # zero height only
    long_ = 0.95 * min(Hh, Ww)
    for a in (80.0, 30.0):  # aspect ratios up to 1:80 and 80:1 inside the image
        add("aspect", _xyxy(Ww / 2 + 3.3, Hh / 2, long_, long_ / a))
        add("aspect", _xyxy(Ww / 2, Hh / 2 - 1.7, long_ / a, long_))
    return out


def box_walk_cases():
    """Boxes for the 7 x 7 aligned pooler on a 480 x 640 pyramid that reach each fallback of the rolling walk, each bin size class and
    the rolling walk itself: [(expected walk, expected reason, box)].  Level 0 (stride 4) unless noted."""
    return [
        ("rolling", None, [100.0, 100.0, 156.0, 156.0]),                      # 2-cell bins
        ("rolling", None, [201.3, 98.2, 290.1, 170.9]),
        ("rolling", None, [33.0, 41.0, 120.5, 99.5]),
        ("cells<=NC", "empty_bin", [-120.0, 60.0, 20.0, 170.0]),             # the first bin columns lie wholly left of the map
        ("cells<=NC", "empty_bin", [300.0, 452.0, 356.0, 508.0]),            # the last bin rows lie below it
        ("cells<=NC", "four_bins_on_a_column", [50.0, 50.0, 57.0, 120.0]),   # bins a quarter of a cell wide
        ("cells<=NC", "four_bins_on_a_column", [400.2, 300.1, 402.0, 302.3]),
        ("cells>NC", "more_than_RMAX_rows", [10.0, 10.0, 60.0, 214.0]),      # level 0 by area, bins 7.3 cells high
        ("cells>NC", "more_than_RMAX_rows", [200.0, 20.0, 240.0, 300.0]),
        ("cells<=NC", "exactly_9", [64.0, 64.0, 120.0, 120.0]),
        ("cells>NC", "ten_or_more", [64.0, 64.0, 160.0, 161.0]),
    ]


def single_level_cases(Lh=128, Lw=128):
    """Single-level calls (one map at scale 1, P = 7, aligned, adaptive lattice): lattices of 15 and of 16 and more samples, which
    the four-level assignment cannot reach.  [(class, box)]"""
    return [
        ("lattice15", [3.0, 5.0, 3.0 + 7 * 14.5, 5.0 + 7 * 14.2]),       # gh = gw = 15: the longest table
        ("lattice15", [10.25, 2.5, 10.25 + 7 * 15.0, 2.5 + 7 * 15.0]),   # bins of exactly 15 cells: samples exactly one cell apart
        ("lattice16", [2.0, 3.0, 2.0 + 7 * 15.5, 3.0 + 7 * 15.3]),       # gh = gw = 16: the per-sample path; two backward passes
        ("lattice16", [1.0, 40.0, 1.0 + 7 * 17.8, 40.0 + 7 * 4.0]),      # gw = 18 only
        ("lattice16", [-30.0, -20.0, 150.0, 140.0]),                     # past every edge, gh = gw >= 23
        ("lattice31", [4.0, 4.0, 4.0 + 7 * 2.0, 4.0 + 7 * 2.0]),         # (filler: an ordinary ROI next to the long ones)
    ]


def wide_bin_cases(P=7):
    """Fixed ratio 2 on one 512 x 512 map at scale 1: bins of 20, 31 and 68 cells (P = 7 aligned; P = 14 for the mask pooler's form, where
    the widest box leaves the map).  The two samples of a bin are bw / 2 cells apart: 20 stays on the table path, 31 and 68 do not fit
    a KMAX-cell table row and must take the per-sample path."""
    return [("wide20", [8.0, 8.0, 8.0 + P * 20.0, 8.0 + P * 20.0]), ("wide31", [10.5, 20.25, 10.5 + P * 31.0, 20.25 + P * 31.0]),
            ("wide68", [16.0, 16.0, 16.0 + P * 68.0, 16.0 + P * 68.0]), ("wide31x2", [40.0, 100.0, 40.0 + P * 31.0, 100.0 + P * 2.0])]


def exact_edge_cases(aligned=True):
    """Boxes whose every intermediate is exactly representable, with samples exactly on -1, 0, integer cells, L - 1 and L.
    [(name, box, level)] on the 480 x 640 pyramid.

    aligned (the 7 x 7 box pooler): a box of 56 * 2^j pixels lies on level j (stride 4 * 2^j) and is 14 cells wide: bw = 2, g = 2, and
    sample i of bin p sits at  x1 s - .5 + 2 p + (i + .5) = x1 s + 2 p + i.  With x1 = m * stride the samples are the integers m .. m + 13.
    not aligned (the 14 x 14 poolers, ratio 2 or adaptive): 896 pixels on the coarsest level (stride 32, 15 x 20 cells) are 28 cells:
    bw = 2, g = 2 for both, samples at  x1 s + 2 p + i + .5;  x1 = 32 m + 16 puts them on m + 1 .. m + 28.  m = -8 (x) and -13 (y) end
    exactly on L = 20 and L = 15 and pass -1, 0 and L - 1 on the way (the samples below -1 are skipped).
    On a ramp map every bin is the mean of four map values at clamped integer cells: the tests write it out and compare for equality."""
    if not aligned:
        return [("all_edges_p5", [-240.0, -400.0, 656.0, 496.0], 3)]
    return [
        ("on_minus1_and_0", [-4.0, -4.0, 52.0, 52.0], 0),                   # m = -1: the first sample ON the skip boundary, kept
        ("interior_integers", [40.0, 80.0, 96.0, 136.0], 0),
        # level 0 is 120 x 160 cells: m + 13 = 160 -> m = 147 (x), m + 13 = 120 -> m = 107 (y): the last two samples on L - 1 and L
        ("on_Lm1_and_L", [4.0 * 147, 4.0 * 107, 4.0 * 147 + 56.0, 4.0 * 107 + 56.0], 0),
        ("on_Lm1_and_L_p3", [8.0 * 67, 8.0 * 47, 8.0 * 67 + 112.0, 8.0 * 47 + 112.0], 1),  # level 1: 60 x 80 cells
        ("interior_p4", [16.0 * 3, 16.0 * 2, 16.0 * 3 + 224.0, 16.0 * 2 + 224.0], 2),
    ]
