"""GPU suite (-m gpu): the detection tail -- a3d_paste_lsq, a3d_plane_offset_dense, a3d_plane_offset_dense_u8 (csrc/heads_post.hip),
a3d_detections_pack and a3d_mask_rle (csrc/pack.hip) -- against the float64 / exact references of tests/post_ref.py (held to the oracle
and to the reference's fixture on the CPU by tests/test_post_ref_host.py).

Every kernel is reached through the C ABI with buffers of this file's own, filled with a sentinel and followed by a guard, so that a
store that was skipped and a store that went to the wrong place both show.  Masks are compared exactly outside the undecided band of the
threshold (post_ref.band); planes are held to the counted law gamma(15) |n_k| M on the kernel's OWN mask read back.  Each law test
prints its worst err / bound: MEASUREMENTS.md."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
SENT = -7.0
ISENT = -77
BSENT = 0xAB
ERR_ARG = -1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from articulation3d_amd import ops as o

    return o


def _lib():
    from articulation3d_amd import _lib as L

    return L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------ a3d_paste_lsq
def paste(ops, inp, H, W, *, clip=1, masks=True, normals=True, depth=True, mask_thresh=0.5):
    """One launch into sentinel-filled buffers (one guard slot behind each) -> host arrays."""
    L = _lib()
    B, R = inp.scores.shape
    n = B * R
    focal, cx, cy = P.intrinsics(H, W)
    t = dict(boxes=_dev(inp.boxes), scores=_dev(inp.scores), count=_dev(inp.count), row_offset=_dev(inp.row_offset), prob=_dev(inp.prob),
             normals=_dev(inp.normals), depth=_dev(inp.depth))
    mk = torch.full(((n + 1) * H * W,), BSENT, dtype=torch.uint8, device="cuda") if masks else None
    planes = torch.full((n + 1, 3), SENT, device="cuda")
    area = torch.full((n + 1,), ISENT, dtype=torch.int32, device="cuda")
    keep = torch.full((n + 1,), ISENT, dtype=torch.int32, device="cuda")
    ob = torch.full((n + 1, 4), SENT, device="cuda")
    d = L.PasteDesc()
    d.boxes, d.scores, d.count, d.row_offset, d.mask_prob = (t[k].data_ptr() for k in ("boxes", "scores", "count", "row_offset", "prob"))
    d.normals = t["normals"].data_ptr() if normals else None
    d.depth = t["depth"].data_ptr() if depth else None
    d.B, d.R, d.MS, d.H, d.W = B, R, inp.prob.shape[-1], H, W
    d.post_score_thresh, d.mask_thresh = P.POST_THRESH, mask_thresh
    d.focal, d.cx, d.cy, d.clip_boxes = focal, cx, cy, clip
    d.masks, d.planes, d.area, d.keep, d.out_boxes = ops._p(mk), planes.data_ptr(), area.data_ptr(), keep.data_ptr(), ob.data_ptr()
    L.check(L.lib().a3d_paste_lsq(C.byref(d), ops._stream()), "a3d_paste_lsq")
    torch.cuda.synchronize()
    for name, buf, s in (("planes", planes, SENT), ("area", area, ISENT), ("keep", keep, ISENT), ("out_boxes", ob, SENT)):
        assert bool((buf[n:] == s).all()), f"{name}: the guard slot was written"
    out = dict(planes=planes[:n].cpu().numpy().reshape(B, R, 3), area=area[:n].cpu().numpy().reshape(B, R),
               keep=keep[:n].cpu().numpy().reshape(B, R), out_boxes=ob[:n].cpu().numpy().reshape(B, R, 4), masks=None)
    if masks:
        assert bool((mk[n * H * W:] == BSENT).all()), "masks: the guard slot was written"
        out["masks"] = mk[: n * H * W].cpu().numpy().reshape(B, R, H, W)
    return out


def check_paste(inp, out, H, W, clip):
    """Every assertion of the paste contract on one launch -> (worst plane err / bound, undecided pixels, pixels)."""
    ref = P.postprocess64(inp.boxes, inp.scores, inp.count, inp.row_offset, inp.prob, H, W, P.POST_THRESH, 0.5, clip)
    focal, cx, cy = P.intrinsics(H, W)
    assert np.array_equal(out["keep"], ref.keep)
    assert np.array_equal(out["out_boxes"], ref.out_boxes)
    m = out["masks"]
    assert bool(np.isin(m, (0, 1)).all()), "a byte of the mask buffer was not written (or is neither 0 nor 1)"
    und = ref.undecided
    assert np.array_equal(m[~und] != 0, ref.mask[~und])
    assert np.array_equal(out["area"], m.reshape(*m.shape[:2], -1).sum(-1))
    dead = ref.keep == 0
    assert not m[dead].any() and not out["area"][dead].any() and not _bits(out["planes"][dead]).any()  # (+0.0: all bits clear)
    worst = 0.0
    for b, r in zip(*np.nonzero(ref.keep)):
        nrm = inp.normals[ref.rows[b, r]]
        fit = P.plane_fit64(inp.depth[b], m[b, r], nrm, focal, cx, cy)
        if fit.count == 0:  # an empty pasted mask: the input normal, bit for bit
            assert np.array_equal(_bits(out["planes"][b, r]), _bits(nrm)), (b, r)
        worst = max(worst, P.law_ratio(out["planes"][b, r], fit.plane, P.plane_bound(fit)))
    return worst, int(und.sum()), und.size


PASTE_GRID = [(hw, MS, br) for hw in P.PASTE_SIZES for MS in (28, 7, 1) for br in ((1, 1), (3, 8))]


@pytest.mark.parametrize("hw,MS,br", PASTE_GRID, ids=lambda v: str(v).replace(" ", ""))
def test_paste_lsq_masks_exact_outside_the_band_and_planes_within_the_law(ops, hw, MS, br):
    H, W = hw
    worst, n_und, npix, empties = 0.0, 0, 0, 0
    for seed in P.paste_seeds(H, W, br):
        inp = P.paste_inputs(H, W, MS, *br, seed=seed)
        out = paste(ops, inp, H, W)
        w, u, n = check_paste(inp, out, H, W, True)
        worst, n_und, npix = max(worst, w), n_und + u, npix + n
        empties += int(((out["keep"] == 1) & (out["area"] == 0)).sum())
        if br == (3, 8):
            assert out["keep"][0, 1] == 1 and out["area"][0, 1] == 0  # the map that lies wholly below the threshold (row 3)
            assert out["area"].max() > 0.25 * H * W
    print(f"LAW paste_lsq plane: {H}x{W} MS{MS} {br[0]}x{br[1]} worst err/bound = {worst:.3f}  (undecided {n_und} of {npix} pixels, "
          f"{empties} empty pasted masks)")
    assert n_und <= npix // P.UNDECIDED_CAP
    assert worst <= 1.0


@pytest.mark.parametrize("hw", [(24, 48), (24, 40), (72, 250)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_paste_lsq_switches(ops, hw):
    H, W = hw
    inp = P.paste_inputs(H, W, 7, 3, 8)
    base = paste(ops, inp, H, W)
    # clip_boxes = 0: every slot below the count is kept and pasted from its raw box
    raw = paste(ops, inp, H, W, clip=0)
    worst, _, _ = check_paste(inp, raw, H, W, False)
    print(f"LAW paste_lsq plane: {H}x{W} MS7 3x8 clip_boxes=0 worst err/bound = {worst:.3f}")
    assert worst <= 1.0 and raw["keep"].sum() == 8 + 5 > base["keep"].sum()
    # masks = NULL: the other four outputs keep their bits
    nom = paste(ops, inp, H, W, masks=False)
    for k in ("area", "keep"):
        assert np.array_equal(nom[k], base[k]), k
    for k in ("planes", "out_boxes"):
        assert np.array_equal(_bits(nom[k]), _bits(base[k])), k
    # normals = NULL or depth = NULL: zero planes, everything else as before
    for kw in ({"normals": False}, {"depth": False}, {"normals": False, "depth": False}):
        o = paste(ops, inp, H, W, **kw)
        assert not o["planes"].any(), kw  # (zero by value: a live slot's third component is the negated 0 of the axis swap, -0.0)
        for k in ("masks", "area", "keep", "out_boxes"):
            assert np.array_equal(o[k], base[k]), (kw, k)


@pytest.mark.parametrize("hw", [(24, 48), (24, 40), (17, 13), (65, 256), (72, 250)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_paste_lsq_a_detection_does_not_depend_on_its_batch(ops, hw):
    H, W = hw
    MS = 28
    rng = np.random.default_rng(5)
    cases = P.box_cases(H, W)
    B, R = 3, 8
    count = np.array([8, 3, 6], dtype=np.int32)
    row_offset = np.array([2, 10, 13], dtype=np.int32)
    rows = 13 + R
    prob = P.make_prob(rows, MS, 9)
    nrm = rng.standard_normal((rows, 3)).astype(np.float32)
    depth = rng.uniform(0.5, 5.0, (B, H, W)).astype(np.float32)
    for name in ("inside", "edge_left", "cover"):
        box = np.array([b for n, b, _ in cases if n == name][0], dtype=np.float32)
        boxes = np.tile(np.array([1.0, 1.0, W - 1.0, H - 1.0], dtype=np.float32), (B, R, 1))
        boxes[2, 5] = box
        scores = np.full((B, R), 0.9, dtype=np.float32)
        big = types.SimpleNamespace(boxes=boxes, scores=scores, count=count, row_offset=row_offset, prob=prob, normals=nrm, depth=depth)
        one = types.SimpleNamespace(boxes=box.reshape(1, 1, 4), scores=scores[:1, :1], count=np.array([1], dtype=np.int32),
                                    row_offset=np.array([0], dtype=np.int32), prob=prob[18:19], normals=nrm[18:19], depth=depth[2:3])
        a, b = paste(ops, big, H, W), paste(ops, one, H, W)
        assert a["keep"][2, 5] == 1 == b["keep"][0, 0] and b["area"][0, 0] > 0
        assert np.array_equal(a["masks"][2, 5], b["masks"][0, 0]) and a["area"][2, 5] == b["area"][0, 0]
        assert np.array_equal(_bits(a["planes"][2, 5]), _bits(b["planes"][0, 0])), name


# ------------------------------------------------------------------------------------------ the dense plane fits
def dense(ops, which, depth, masks, normals, H, W, *, byte_offset=0, D=None):
    """-> (return code, out [D + 1, 3] on the host; the last row is the guard)."""
    L = _lib()
    D = masks.shape[0] if D is None else D
    focal, cx, cy = P.intrinsics(H, W)
    dm = _dev(depth)
    if which == "u8":
        raw = torch.full((masks.size + 8,), BSENT, dtype=torch.uint8, device="cuda")
        raw[byte_offset: byte_offset + masks.size] = _dev(masks.astype(np.uint8)).reshape(-1)
        mptr, fn = raw.data_ptr() + byte_offset, L.lib().a3d_plane_offset_dense_u8
    else:
        raw = _dev(masks.astype(np.float32))
        mptr, fn = raw.data_ptr(), L.lib().a3d_plane_offset_dense
    nm = _dev(normals)
    out = torch.full((masks.shape[0] + 1, 3), SENT, device="cuda")
    rc = fn(dm.data_ptr(), mptr, nm.data_ptr(), out.data_ptr(), D, H, W, focal, cx, cy, ops._stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def dense_inputs(H, W, seed=0):
    """Four masks: random with byte values other than 1, empty, full (255), and a single pixel -- the last of the image."""
    rng = np.random.default_rng(100 + 13 * H + W + seed)
    m = np.zeros((4, H, W), dtype=np.uint8)
    m[0] = rng.choice(np.array([0, 0, 1, 2, 128, 255], dtype=np.uint8), size=(H, W))
    m[2] = 255
    m[3, H - 1, W - 1] = 1
    nrm = rng.standard_normal((4, 3)).astype(np.float32)  # (no component is zero: every mask sees the rays of both axes)
    depth = rng.uniform(0.5, 5.0, (H, W)).astype(np.float32)
    return depth, m, nrm


def check_dense(got, depth, m, nrm, H, W):
    focal, cx, cy = P.intrinsics(H, W)
    worst = 0.0
    for k in range(len(m)):
        fit = P.plane_fit64(depth, m[k], nrm[k], focal, cx, cy)
        if fit.count == 0:
            assert np.array_equal(_bits(got[k]), _bits(nrm[k]))  # an empty mask: the input normal comes back
        worst = max(worst, P.law_ratio(got[k], fit.plane, P.plane_bound(fit)))
    assert bool((got[len(m):] == SENT).all()), "the guard row was written"
    return worst


# W < 256, == 256, > 256 for the float kernel's dx / dy stepping; for the byte kernel: quads in one pass of 1024 threads (7 x 300,
# 11 x 100; 2 x 2048 is exactly 1024 quads), in two (18 x 300: 1350 quads), and the scalar walk because H W % 4 != 0 (103 x 5, 41 x 30, 3 x 257) or W % 4 != 0 alone (300 x 1, 6 x 6, 52 x 102).
# 103 x 5 is two full passes of the float kernel's 256 threads and a part of a third, so that the wrap of px at W = 5 is taken often.
DENSE_SIZES = [(300, 1), (103, 5), (11, 100), (5, 256), (7, 300), (18, 300), (41, 30), (3, 257), (6, 6), (52, 102), (2, 2048)]


@pytest.mark.parametrize("hw", DENSE_SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_dense_plane_fits_hold_the_law(ops, hw):
    H, W = hw
    depth, m, nrm = dense_inputs(H, W)
    # u8 + 1: a mask base one byte past a word boundary.  A value test only: the kernel falls back to bytes there, and a word load from
    # such a base would read the same bytes on this hardware, so it cannot show that the alignment test exists.
    for which, off in (("f32", 0), ("u8", 0), ("u8", 1)):
        rc, got = dense(ops, which, depth, m, nrm, H, W, byte_offset=off)
        assert rc == 0
        worst = check_dense(got, depth, m, nrm, H, W)
        print(f"LAW plane_offset_dense {which}{'+1' if off else ''}: {H}x{W} worst err/bound = {worst:.3f}")
        assert worst <= 1.0


def test_dense_plane_fits_refuse_more_than_2048_and_accept_no_detection(ops):  # (and refuse an image without pixels)
    depth, m, nrm = dense_inputs(3, 2049)
    for which in ("f32", "u8"):
        for H, W in ((3, 2049), (2049, 3)):
            rc, got = dense(ops, which, depth.reshape(H, W), m.reshape(4, H, W), nrm, H, W)
            assert rc == ERR_ARG and bool((got == SENT).all()), (which, H, W)
        depth2, m2, nrm2 = dense_inputs(6, 6)
        for H, W in ((6, 0), (0, 6), (6, -1), (-1, 6)):  # (the kernels divide by W)
            rc, got = dense(ops, which, depth2, m2, nrm2, H, W)
            assert rc == ERR_ARG and bool((got == SENT).all()), (which, H, W)
        rc, got = dense(ops, which, depth2, m2, nrm2, 6, 6, D=0)
        assert rc == 0 and bool((got == SENT).all()), which


# ------------------------------------------------------------------------------------------ a3d_detections_pack
def pack_inputs(R, MS, seed=0):
    """Six images: (keep pattern, count) = (all, above R), (none, R), (alternating, below R), (only the last, R), (all, 0) and
    (all, below R: keep set in rows at and beyond the count); row_offset is not b R."""
    rng = np.random.default_rng(seed + R + MS)
    B = 6
    below = max(R - 2, 0)
    count = np.array([R + 4, R, below, R, 0, below], dtype=np.int32)
    keep = np.zeros((B, R), dtype=np.int32)
    keep[0] = 1
    keep[2, ::2] = 1
    keep[3, R - 1] = 1
    keep[4] = 1
    keep[5] = 3  # (any non-zero value keeps)
    row_offset = (np.cumsum(np.minimum(count, R)) - np.minimum(count, R) + 3).astype(np.int32)
    rows = int(row_offset[-1]) + R
    return dict(boxes=rng.standard_normal((B, R, 4)).astype(np.float32), scores=rng.random((B, R)).astype(np.float32),
                classes=rng.integers(0, 90, (B, R)).astype(np.int32), count=count, row_offset=row_offset, keep=keep,
                planes=rng.standard_normal((B, R, 3)).astype(np.float32), rot_axis=rng.standard_normal((rows, 3)).astype(np.float32),
                tran_axis=rng.standard_normal((rows, 2)).astype(np.float32), mask_prob=rng.random((rows, MS, MS)).astype(np.float32))


OPTIONAL = ("planes", "rot_axis", "tran_axis", "mask_prob")


def pack(ops, inp, MS):
    L = _lib()
    B, R = inp["scores"].shape
    rec = P.REC_HEAD + MS * MS
    t = {k: (None if v is None else _dev(v)) for k, v in inp.items()}
    records = torch.full((B + 1, R, rec), SENT, device="cuda")
    rc_ = torch.full((B + 1,), ISENT, dtype=torch.int32, device="cuda")
    d = L.PackDesc()
    for k in ("boxes", "scores", "classes", "count", "row_offset", "keep") + OPTIONAL:
        setattr(d, k, ops._p(t[k]))
    d.B, d.R, d.MS = B, R, MS
    d.records, d.rec_count = records.data_ptr(), rc_.data_ptr()
    rc = L.lib().a3d_detections_pack(C.byref(d), ops._stream())
    torch.cuda.synchronize()
    return rc, records.cpu().numpy(), rc_.cpu().numpy()


def check_pack(ops, inp, MS):
    B = inp["scores"].shape[0]
    rc, rec, n = pack(ops, inp, MS)
    want, wn = P.pack_ref(*(inp[k] for k in ("boxes", "scores", "classes", "count", "row_offset", "keep") + OPTIONAL), MS)
    assert rc == 0
    assert np.array_equal(n[:B], wn) and n[B] == ISENT
    assert np.array_equal(_bits(rec[:B]), _bits(want))  # kept rows in slot order, +0.0 everywhere else: no sentinel, no other row
    assert bool((rec[B] == SENT).all()), "the guard image was written"
    return wn


@pytest.mark.parametrize("MS", [1, 7, 28])
@pytest.mark.parametrize("R", [1, 5, 1024])
def test_detections_pack_equals_the_reference(ops, R, MS):
    inp = pack_inputs(R, MS)
    wn = check_pack(ops, inp, MS)
    below = max(R - 2, 0)
    assert wn.tolist() == [R, 0, (below + 1) // 2, 1, 0, below]


@pytest.mark.parametrize("absent", [(k,) for k in OPTIONAL] + [OPTIONAL], ids=lambda v: "+".join(v))
def test_detections_pack_optional_inputs_come_out_as_zeros(ops, absent):
    inp = pack_inputs(5, 7)
    for k in absent:
        inp[k] = None
    check_pack(ops, inp, 7)


def test_detections_pack_refuses_more_than_1024_slots(ops):
    inp = pack_inputs(1025, 1)
    rc, rec, n = pack(ops, inp, 1)
    assert rc == ERR_ARG and bool((rec == SENT).all()) and bool((n == ISENT).all())


# ------------------------------------------------------------------------------------------ a3d_mask_rle
def mask_rle(ops, masks, cap, H=None, W=None):
    """masks [D, H, W] uint8 -> (return code, pos [D + 1, cap], count [D + 1], first [D + 1]); the last rows are the guard."""
    L = _lib()
    D = masks.shape[0]
    H, W = masks.shape[1] if H is None else H, masks.shape[2] if W is None else W
    m = _dev(masks)
    pos = torch.full((D + 1, cap), -1, dtype=torch.int32, device="cuda")
    count = torch.full((D + 1,), ISENT, dtype=torch.int32, device="cuda")
    first = torch.full((D + 1,), ISENT, dtype=torch.int32, device="cuda")
    rc = L.lib().a3d_mask_rle(m.data_ptr(), D, H, W, cap, pos.data_ptr(), count.data_ptr(), first.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    return rc, pos.cpu().numpy(), count.cpu().numpy(), first.cpu().numpy()


@pytest.mark.parametrize("hw", P.RLE_SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_mask_rle_boundaries_are_exact(ops, hw):
    H, W = hw
    pats = P.rle_patterns(H, W)
    masks = np.stack([m for _, m in pats])
    D, cap = len(pats), H * W
    rc, pos, count, first = mask_rle(ops, masks, cap)
    assert rc == 0
    for d, (name, m) in enumerate(pats):
        want, f = P.rle_boundaries(m)
        assert count[d] == len(want) and first[d] == f, (name, count[d], len(want))
        assert np.array_equal(pos[d, : len(want)], want), name
        assert bool((pos[d, len(want):] == -1).all()), name  # nothing behind the last boundary
    assert count[D] == ISENT and first[D] == ISENT and bool((pos[D] == -1).all())


def test_mask_rle_refuses_one_pixel_more_than_the_largest_mask(ops):
    m = np.zeros((1, 1, 512 * 768 + 1), dtype=np.uint8)
    for H, W in ((1, 512 * 768 + 1), (512 * 768 + 1, 1)):
        rc, pos, count, first = mask_rle(ops, m, 8, H, W)
        assert rc == ERR_ARG and count[0] == ISENT and first[0] == ISENT and bool((pos == -1).all())


@pytest.mark.parametrize("hw", [(31, 33), (5, 7)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_mask_rle_cap_overflow_counts_everything_and_writes_cap_positions(ops, hw):
    from articulation3d_amd.utils import rle

    H, W = hw
    pats = P.rle_patterns(H, W)
    masks = np.stack([m for _, m in pats])
    cap = 5
    rc, pos, count, first = mask_rle(ops, masks, cap)
    assert rc == 0
    over = 0
    for d, (name, m) in enumerate(pats):
        want, f = P.rle_boundaries(m)
        k = min(len(want), cap)
        over += len(want) > cap
        assert count[d] == len(want) and first[d] == f, name  # the true number, however few fit
        assert np.array_equal(pos[d, :k], want[:k]) and bool((pos[d, k:] == -1).all()), name  # [D, cap]: no row runs into the next
    assert over >= 2 and bool((pos[len(pats)] == -1).all())
    got = rle.encode_device(torch.from_numpy(masks).cuda(), cap=4)  # the host retries with room for the fullest mask
    assert [dict(g) for g in got] == [rle.encode(m != 0) for _, m in pats]
