"""GPU suite: a3d_eval_mask_counts / a3d_eval_plane_match (csrc/plane_eval.hip) against tests/plane_eval_ref.py, the law in numpy
float64, then PlaneEvaluator end to end on the fixture recorded from the reference (tests/golden/plane_eval.json) and the ABI's
refusals."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import eval_ref as E
import plane_eval_ref as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(0, 2), (1, 1), (3, 0), (70, 5), (100, 33), (3, 2)]  # (detections, ground truths) per image; the last has twin ground truths
MARGIN = 1e-9
LOOSE = dict(iou_thresh=0.4, normal_thresh=60.0, offset_thresh=0.6)


def _boxes(rng, D, G, twin=False):
    """-> det [D,14], gt [G,8]: ground truths scattered, detections jittered around them, several per ground truth, some of the wrong
    class, scores from a short list (duplicates), planes near the ground truth's or far from it."""
    gt = np.zeros((G, 8), np.float32)
    for g in range(G):
        x, y, w, h = rng.uniform(0, 400), rng.uniform(0, 300), rng.uniform(60, 220), rng.uniform(60, 170)
        n = rng.normal(size=3)
        gt[g] = [x, y, x + w, y + h, *(n / np.linalg.norm(n) * rng.uniform(0.5, 4)), rng.integers(0, 2)]
    if twin:
        gt[1, :4] = gt[0, :4]  # the argmax tie: the lower index wins
    det = np.zeros((D, 14), np.float32)
    for d in range(D):
        if G:
            g = int(rng.integers(0, G))
            det[d, :4] = gt[g, :4] + rng.uniform(-1, 1, 4) * rng.choice([2.0, 10.0, 30.0])
            det[d, 5] = gt[g, 7] if rng.uniform() < 0.8 else 1 - gt[g, 7]
            det[d, 6:9] = (gt[g, 4:7] + rng.normal(size=3) * rng.choice([0.05, 0.4, 1.5])) * rng.choice([1.0, 1.05, 1.3, -1.0])
        else:
            det[d, :4] = [10, 10, 100, 100]
            det[d, 6:9] = [0, 0, 1]
        det[d, 4] = rng.choice([0.3, 0.5, 0.7, 0.9, round(float(rng.uniform()), 2)])
    return det, gt


# ---- a3d_eval_mask_counts -------------------------------------------------------------------------------------------------------------
def _mask_case(H, W, shapes, shift, seed):
    """One batch: per image (det, gt, masks as rows of ONE [S,H,W] table reached through det_slot, gt masks).  det_slot is a
    permutation with gaps (and two slots outside the table), mask bytes come from {0, 1, 2, 255}, some masks are empty on either side,
    the spare bits of gt_bits' last word are set, and the table starts `shift` bytes into its allocation."""
    rng = np.random.default_rng(seed)
    hw = H * W
    images = [dict(zip(("det", "gt"), _boxes(rng, D, G, twin=(k == 5)))) for k, (D, G) in enumerate(shapes)]
    N = sum(len(im["det"]) for im in images)
    S = 2 * N + 3
    slots = rng.permutation(S)[:N].astype(np.int32)
    table = np.zeros((S, H, W), np.uint8)
    for s in range(S):  # every row holds something, so that a wrong slot shows
        yy, xx = np.mgrid[:H, :W]
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.2, 0.8) * max(H, W)
        table[s] = np.where((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r, rng.choice([1, 2, 255], (H, W)), 0) if rng.uniform() < 0.85 else 0
    if N > 4:
        table[slots[3]] = 0       # an empty detection mask
        slots[1], slots[2] = -1, S + 5  # outside the table: empty masks
    at = 0
    for im in images:
        D, G = len(im["det"]), len(im["gt"])
        im["slot"] = slots[at:at + D]
        at += D
        gm = np.zeros((G, H, W), np.uint8)
        for g in range(G):
            yy, xx = np.mgrid[:H, :W]
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.2, 0.8) * max(H, W)
            gm[g] = (np.abs(yy - cy) + np.abs(xx - cx) <= r) & (rng.uniform(size=(H, W)) < 0.9)
        if G:
            gm[0] = 0  # an empty ground-truth mask (with the empty detection mask: both sides empty, IoU 0 / 0)
        im["gt_bits"] = P.pack_bits(gm)
        if G and hw % 32:
            im["gt_bits"][:, -1] |= np.uint32((0xFFFFFFFF << (hw % 32)) & 0xFFFFFFFF)  # spare bits: never pixels
    want = [P.mask_counts(im["det"], im["gt"], table, im["slot"], im["gt_bits"], hw) for im in images]
    buf = torch.zeros(S * hw + 16, dtype=torch.uint8, device="cuda")
    masks = buf[shift:shift + S * hw].view(S, H, W)
    masks.copy_(torch.from_numpy(table))
    return images, masks, want


def _run_counts(images, masks):
    from articulation3d_amd import opt_ops

    hw = masks.shape[1] * masks.shape[2]
    cat = lambda k, w, dt: torch.from_numpy(np.concatenate([np.asarray(im[k]).reshape(-1, w) for im in images]).astype(dt)).cuda()
    off = lambda k: np.concatenate([[0], np.cumsum([len(im[k]) for im in images])]).tolist()
    bits = cat("gt_bits", (hw + 31) // 32, np.uint32).view(torch.int32)
    return opt_ops.eval_mask_counts(cat("det", 14, np.float32), off("det"), cat("gt", 8, np.float32), off("gt"), masks, cat("slot", 1, np.int32).reshape(-1), bits)


@pytest.mark.parametrize("H,W,shift", [(1, 1, 0), (5, 7, 0), (33, 50, 3), (48, 64, 0), (48, 64, 5), (130, 127, 1)])
def test_mask_counts_equal_the_law(H, W, shift):
    """Mask rows at every alignment (the row pitch H*W is odd, or the table is shifted), one word of bits and less, 16 510 pixels = one
    whole block of 16 384 and a short second one."""
    images, masks, want = _mask_case(H, W, SHAPES, shift, seed=H * 1000 + W + shift)
    got = [t.cpu().numpy() for t in _run_counts(images, masks)]
    for k, name in enumerate(("gt_id", "inter", "uni")):
        w = np.concatenate([x[k] for x in want])
        assert got[k].dtype == np.int32 and np.array_equal(got[k], w), name
    gt_id, inter, uni = got
    starts = {(masks.data_ptr() + int(s) * H * W) % 16 for im in images for s in im["slot"] if 0 <= s < masks.shape[0]}
    if H * W % 16:
        assert len(starts) >= 8, starts
    assert (gt_id == -1).sum() == 3 and (gt_id[-3:] == 0).all()  # the image without ground truth; the twins' tie goes to index 0
    assert ((uni == 0) & (gt_id >= 0)).any() or H * W == 1  # both sides empty
    if H * W > 1:
        assert (inter > 0).any() and (inter < uni).any()


def test_mask_counts_at_the_detectors_size():
    """480 x 640 once: 19 blocks per detection, a table that starts 7 bytes off alignment, three detections of one image."""
    images, masks, want = _mask_case(480, 640, [(3, 2)], 7, seed=4)
    got = [t.cpu().numpy() for t in _run_counts(images, masks)]
    assert all(np.array_equal(g, w) for g, w in zip(got, want[0]))
    assert got[2].max() > 16384 and masks.data_ptr() % 16 == 7
    again = [t.cpu().numpy() for t in _run_counts(images, masks)]
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


# ---- a3d_eval_plane_match -------------------------------------------------------------------------------------------------------------
def _law_matches(images, **thr):
    return [P.match_image(im["det"], im["gt"], im["inter"], im["uni"], **thr) for im in images]


def _margins_hold(matches, normal, offset):
    for m in matches:
        ok = m["gt_id"] >= 0
        if not ((np.abs(m["normal_err"][ok] - normal) >= MARGIN).all() and (np.abs(m["offset_err"][ok] - offset) >= MARGIN).all()):
            return False
    return True


@pytest.fixture(scope="module")
def dataset():
    """The seeded 6-image dataset and its reference, made once: resampled (fixed seeds) until every normal / offset error keeps its
    distance from both sets of thresholds."""
    for seed in range(300, 340):
        rng = np.random.default_rng(seed)
        images = []
        for k, (D, G) in enumerate(SHAPES):
            det, gt = _boxes(rng, D, G, twin=(k == 5))
            uni = rng.integers(0, 5000, D).astype(np.int32)
            inter = (uni * rng.choice([0.0, 0.3, 0.5, 0.7, 1.0], D)).astype(np.int32)
            uni[::7], inter[::7] = 0, 0             # two empty masks: IoU 0
            uni[1::9] = 2 * (uni[1::9] // 2 + 1)    # an IoU of exactly 0.5 is not above the threshold
            inter[1::9] = uni[1::9] // 2
            images.append(dict(det=det, gt=gt, inter=inter, uni=uni))
        matches, loose = _law_matches(images), _law_matches(images, **LOOSE)
        if _margins_hold(matches, 30.0, 0.3) and _margins_hold(loose, 60.0, 0.6):
            return images, matches, loose
    raise AssertionError("no seed keeps the margins")


def test_the_match_dataset_holds_every_case_the_law_distinguishes(dataset):
    images, matches, loose = dataset
    assert [(len(im["det"]), len(im["gt"])) for im in images] == SHAPES
    assert _margins_hold(matches, 30.0, 0.3) and _margins_hold(loose, 60.0, 0.6)  # on the CPU, no case dropped
    big = matches[4]
    assert len(set(images[4]["det"][:, 4].tolist())) < 100                      # duplicate scores within an image
    for bit in (1, 2, 4):  # "already covered" decides, per metric
        assert any(((m["qual"] & bit) != (m["tp"] & bit)).any() for m in matches[3:5]) and (big["tp"] & bit).any()
    assert (big["qual"] == 0).any() and (big["tp"] & 8 == 0).all()
    assert len({int(t) for m in matches for t in m["tp"]}) >= 6                  # the three bits fall apart
    assert (matches[2]["gt_id"] == -1).all() and np.isinf(matches[2]["offset_err"]).all()
    assert np.array_equal(images[5]["gt"][0, :4], images[5]["gt"][1, :4]) and (matches[5]["gt_id"] == 0).all()
    assert any((im["uni"] == 0).any() for im in images) and any((m["mask_iou"] == 0.5).any() for m in matches)
    assert any(not np.array_equal(a["tp"], b["tp"]) for a, b in zip(matches, loose))


def test_plane_match_kernel_equals_the_law(dataset):
    from articulation3d_amd import opt_ops

    images, matches, loose = dataset
    cat = lambda k, w, dt: torch.from_numpy(np.concatenate([im[k].reshape(-1, w) for im in images]).astype(dt)).cuda()
    off = lambda k: np.concatenate([[0], np.cumsum([len(im[k]) for im in images])]).tolist()
    args = (cat("det", 14, np.float32), off("det"), cat("gt", 8, np.float32), off("gt"), cat("inter", 1, np.int32).reshape(-1), cat("uni", 1, np.int32).reshape(-1))
    got = {k: v.cpu().numpy() for k, v in opt_ops.eval_plane_match(*args).items()}
    want = {k: np.concatenate([m[k] for m in matches]) for k in got}
    for k in ("gt_id", "rank", "tp"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    for k in ("box_iou", "mask_iou"):
        assert got[k].dtype == np.float64 and got[k].tobytes() == want[k].tobytes(), k
    has = want["gt_id"] >= 0
    dn, do = np.abs(got["normal_err"][has] - want["normal_err"][has]).max(), np.abs(got["offset_err"][has] - want["offset_err"][has]).max()
    print("largest normal_err difference", dn, "largest offset_err difference", do)
    assert dn <= 1e-12 and do <= 1e-12
    assert (got["normal_err"][~has] == 180).all() and np.isposinf(got["offset_err"][~has]).all() and (got["mask_iou"][~has] == 0).all()
    for thr_n, thr_o in ((30.0, 0.3), (60.0, 0.6)):
        assert np.array_equal(got["normal_err"] < thr_n, want["normal_err"] < thr_n) and np.array_equal(got["offset_err"] < thr_o, want["offset_err"] < thr_o)
    # other thresholds move the decisions with them
    got2 = opt_ops.eval_plane_match(*args, **LOOSE)
    assert np.array_equal(got2["tp"].cpu().numpy(), np.concatenate([m["tp"] for m in loose]))
    assert not np.array_equal(got2["tp"].cpu().numpy(), got["tp"])


# ---- PlaneEvaluator on the fixture recorded from the reference ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "plane_eval.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def law(fixture):
    images, npos, names = P.fixture_images(fixture)
    res, matches, entries = P.evaluate(images, npos, names, fixture["iou_thresh"], fixture["normal_threshold"], fixture["offset_threshold"])
    return images, names, res, matches, entries


def _instances(im, hw):
    from articulation3d_amd.structures import Boxes, Instances

    inst = Instances(tuple(hw))
    t = torch.from_numpy(im["det"]).cuda()
    inst.pred_boxes, inst.scores, inst.pred_classes, inst.pred_plane = Boxes(t[:, :4]), t[:, 4], t[:, 5].long(), t[:, 6:9]
    inst.pred_masks = torch.from_numpy(im["masks"]).cuda().bool()
    return inst


def _records(ims, hw, rng, R=12, F=30):
    """What inference_batched leaves: records packed from the front, their masks in the slots keep marks (scattered, in order), other
    slots full of ones."""
    B = len(ims)
    rec, keep = torch.full((B, R, F), 3.0), torch.zeros((B, R), dtype=torch.uint8)
    masks = torch.ones((B, R, *hw), dtype=torch.uint8)
    for b, im in enumerate(ims):
        n = len(im["det"])
        rec[b, :n, :14] = torch.from_numpy(im["det"])
        slots = np.sort(rng.permutation(R)[:n])
        keep[b, slots] = 1
        if n:
            masks[b, slots] = torch.from_numpy(im["masks"]) * 255
    return rec.cuda(), torch.tensor([len(im["det"]) for im in ims], dtype=torch.int32).cuda(), masks.cuda(), keep.cuda()


def _evaluator(fixture):
    from articulation3d_amd import evaluation_planes

    gt = evaluation_planes.PlaneGroundTruth.from_coco(fixture["coco"], fixture["thing_classes"], "cuda", fixture["image_hw"])
    return gt, lambda: evaluation_planes.PlaneEvaluator(gt, fixture["iou_thresh"], fixture["normal_threshold"], fixture["offset_threshold"])


def test_ground_truth_masks_are_packed_from_their_rle(fixture, law):
    from articulation3d_amd import opt_ops

    images = law[0]
    gt, _ = _evaluator(fixture)
    H, W = fixture["image_hw"]
    dense = np.concatenate([im["gt_masks"] for im in images])
    assert gt.gt_bits.dtype == torch.int32 and tuple(gt.gt_bits.shape) == (len(dense), (H * W + 31) // 32)
    assert np.array_equal(opt_ops.unpack_masks(gt.gt_bits, H, W).cpu().numpy(), dense)
    assert np.array_equal(gt.gt_bits.cpu().numpy().view(np.uint32), P.pack_bits(dense))
    assert gt.gt.cpu().numpy().tobytes() == np.concatenate([im["gt"] for im in images]).tobytes() and gt.npos.tolist()[2] == 0
    sub_gt, sub_bits, off = gt.rows_of([3, 1])  # any order of images: gathered on the device
    assert off == [0, len(images[3]["gt"]), len(images[3]["gt"]) + len(images[1]["gt"])]
    assert np.array_equal(sub_gt.cpu().numpy(), np.concatenate([images[3]["gt"], images[1]["gt"]]))
    assert np.array_equal(sub_bits.cpu().numpy().view(np.uint32), P.pack_bits(np.concatenate([images[3]["gt_masks"], images[1]["gt_masks"]])))


def test_evaluator_end_to_end_on_the_reference_fixture(fixture, law, tmp_path):
    images, names, law_res, matches, entries = law
    hw = fixture["image_hw"]
    gt, new = _evaluator(fixture)
    ids = [im["image_id"] for im in images]
    rng = np.random.default_rng(11)
    depth_gt = (rng.uniform(0, 4, (len(ids), 24, 32)) * (rng.uniform(size=(len(ids), 24, 32)) < 0.8)).astype(np.float32)
    depth = rng.uniform(0, 4, (len(ids), 24, 32)).astype(np.float32)

    def run(how, order, splits):
        ev = new()
        for part in np.array_split(np.asarray(order), splits):
            if how == "process":
                ev.process([{"image_id": ids[i], "depth": torch.from_numpy(depth_gt[i])} for i in part],
                           [{"instances": _instances(images[i], hw), "depth": torch.from_numpy(depth[i]).cuda()} for i in part])
            else:
                rec, cnt, masks, keep = _records([images[i] for i in part], hw, np.random.default_rng(len(part)))
                ev.process_records([ids[i] for i in part], rec, cnt, masks, keep, torch.from_numpy(depth[part]).cuda(), torch.from_numpy(depth_gt[part]).cuda())
        return ev.evaluate(), ev

    n = len(ids)
    base, ev = run("process", range(n), 1)
    want = fixture["metrics"]
    assert list(base) == list(want) + ["depth_l1_dist"]  # exactly the reference's keys, in its order
    assert ev.n_entries.tolist() == [len(e) for e in entries]
    bounds = P.reference_bounds(fixture, names, entries)
    for key, v in want.items():
        print(f"{key}: {base[key]!r} reference {v!r} law {law_res[key]!r}")
        assert abs(base[key] - v) <= bounds[key], key
        assert abs(base[key] - law_res[key]) <= 1e-12, key
    s, c = E.depth_l1(depth, depth_gt)
    assert abs(base["depth_l1_dist"] - np.mean(s / np.maximum(c, 1))) <= 1e-10 * base["depth_l1_dist"]
    for k in ("gt_id", "rank", "tp", "inter", "uni"):
        assert np.array_equal(ev.detections[k].cpu().numpy(), np.concatenate([m[k] for m in matches])), k
    assert ev.detections["det_off"].tolist() == np.concatenate([[0], np.cumsum([len(im["det"]) for im in images])]).tolist()
    # the same bits whatever the call shape, the batching and the order
    same = lambda a, b: list(a) == list(b) and all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in b)
    perm = np.random.default_rng(2).permutation(n)
    for how, order, splits in (("records", range(n), 1), ("records", range(n), 2), ("process", perm, 5), ("records", perm, 5), ("records", perm, 2)):
        other, _ = run(how, order, splits)
        assert same(other, base), (how, splits)
    # a one-rank process group takes the gather path: the same bits again
    import torch.distributed as dist

    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        grouped, _ = run("records", perm, 2)
    finally:
        dist.destroy_process_group()
    assert same(grouped, base)
    # the depth value is ArtiEvaluator's, bit for bit
    from articulation3d_amd import evaluation

    arti = evaluation.ArtiEvaluator(types_gt(gt))
    for i in range(n):
        arti._score_depth([arti._image_index(ids[i])], torch.from_numpy(depth[i]).cuda(), torch.from_numpy(depth_gt[i]))
    assert evaluation._depth_l1_dist(arti._depth_rows()) == base["depth_l1_dist"]


def types_gt(gt):
    """The three things ArtiEvaluator's depth path reads from a ground truth."""
    import types

    return types.SimpleNamespace(index=gt.index, device=gt.device, image_ids=gt.image_ids)


def test_an_image_without_ground_truth_gives_false_positives_and_no_statistics(fixture, law):
    from articulation3d_amd import evaluation_planes

    images = law[0]
    coco = dict(fixture["coco"], annotations=[a for a in fixture["coco"]["annotations"] if a["image_id"] == images[0]["image_id"]])
    gt = evaluation_planes.PlaneGroundTruth.from_coco(coco, None, "cuda", fixture["image_hw"])
    k = next(i for i, im in enumerate(images) if i > 0 and len(im["det"]))
    ev = evaluation_planes.PlaneEvaluator(gt)
    ev.process([{"image_id": images[k]["image_id"]}], [{"instances": _instances(images[k], fixture["image_hw"])}])
    res = ev.evaluate()
    assert not any(s in res for s in P.STAT_KEYS) and all(v == 0 for v in res.values()) and len(res) >= 6
    assert (ev.detections["gt_id"] == -1).all() and (ev.detections["tp"] == 0).all() and ev.n_entries.sum() == len(images[k]["det"])
    assert ev.detections["uni"].cpu().numpy().tolist() == [int((m != 0).sum()) for m in images[k]["masks"]]


def test_the_detectors_two_call_shapes_give_the_same_result(hip_model, oracle):
    """model(inputs) -> process and inference_batched(want_masks=True) -> process_records on the same frames, against ground truth made
    from the detections themselves (boxes, planes and RLE masks): the record -> mask slot mapping is the detector's, every detection
    finds its own mask, and both call shapes give the same bits."""
    from articulation3d_amd import evaluation_planes
    from articulation3d_amd.utils import rle

    model = hip_model
    saved = model.roi_heads.box_predictor.test_score_thresh
    model.roi_heads.box_predictor.test_score_thresh = 0.5
    try:
        frames = oracle.synthetic_frames(2, seed=3000)
        out = model.inference_batched(torch.from_numpy(frames).cuda(), want_masks=True)
        inputs = [{"image": torch.as_tensor(f.transpose(2, 0, 1).astype("float32")), "image_id": 10 + b} for b, f in enumerate(frames)]
        outs = model(inputs)
    finally:
        model.roi_heads.box_predictor.test_score_thresh = saved
    counts = out.rec_count.tolist()
    assert all(0 < c <= 60 for c in counts) and out.masks is not None
    hw = tuple(out.masks.shape[2:])
    slots = evaluation_planes.record_slots(out.keep).reshape(len(counts), -1)
    anns = []
    for b, c in enumerate(counts):
        rec = out.records[b, :c, :14].cpu().numpy().astype(np.float64)
        assert (slots[b, :c] >= 0).all() and (slots[b, c:] == -1).all()
        own = out.masks.reshape(-1, *hw)[slots[b, :c].long()].cpu().numpy()
        for k in range(c):
            x1, y1, x2, y2 = rec[k, :4]
            anns.append({"id": len(anns) + 1, "image_id": 10 + b, "category_id": int(rec[k, 5]) + 1, "bbox": [x1, y1, x2 - x1, y2 - y1],
                         "plane": rec[k, 6:9].tolist(), "segmentation": rle.encode((own[k] != 0).astype(np.uint8))})
    coco = {"images": [{"id": 10}, {"id": 11}], "annotations": anns, "categories": [{"id": 1, "name": "arti_rot"}, {"id": 2, "name": "arti_tran"}]}
    gt = evaluation_planes.PlaneGroundTruth.from_coco(coco, None, "cuda", hw)
    a, b = evaluation_planes.PlaneEvaluator(gt), evaluation_planes.PlaneEvaluator(gt)
    for k, o in enumerate(outs):  # (forward()'s Instances carry the head's raw normal; the evaluated plane is the record's, refitted to the depth map)
        o["instances"].pred_plane = out.records[k, :counts[k], 6:9]
    a.process(inputs, outs)
    b.process_records([10, 11], out.records, out.rec_count, out.masks, out.keep)
    ra, rb = a.evaluate(), b.evaluate()
    assert ra == rb and len(ra) >= 14
    assert torch.equal(a.detections["det"][:, :9], b.detections["det"][:, :9])  # (the axis columns are not part of this evaluation)
    assert torch.equal(a.detections["inter"], b.detections["inter"]) and torch.equal(a.detections["uni"], b.detections["uni"])
    d = b.detections
    assert bool((d["box_iou"] > 0.999).all()) and bool((d["normal_err"] < 1e-3).all()) and bool((d["offset_err"] < 1e-6).all())
    # every detection's own mask is among the ground truths, so the mask it was counted against is at least its own box's best match;
    # where no other box ties with its own, the counts are those of a mask with itself
    sole = d["gt_id"].cpu().numpy() == np.concatenate([np.arange(c) for c in counts])
    assert sole.mean() > 0.5 and bool((d["inter"].cpu().numpy()[sole] == d["uni"].cpu().numpy()[sole]).all())
    assert all(abs(v - 1.0) < 1e-12 for k, v in ra.items() if k.startswith("plane_ap")), ra


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_inconsistent_arguments_are_refused_before_any_launch():
    """A3D_ERR_ARG (-1) and untouched outputs.  Every pointer is a real allocation large enough for the widest reading of the
    arguments, so a call that was wrongly accepted would still stay inside it."""
    from articulation3d_amd import _lib, evaluation_planes, opt_ops

    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    big = lambda n, dt, fill=0: torch.full((n,), fill, dtype=dt, device="cuda")
    f32, i32, u8, off_dev = big(8192, torch.float32), big(8192, torch.int32), big(1 << 16, torch.uint8), big(64, torch.int32)
    outs = [big(4096, torch.float64, 7), big(4096, torch.int32, 7), big(4096, torch.uint8, 7)]
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    null_ints = ctypes.POINTER(ctypes.c_int)()

    def counts(**kw):
        d = _lib.EvalMaskCountsDesc()
        d.det, d.gt, d.det_off, d.gt_off = f32.data_ptr(), f32.data_ptr(), off_dev.data_ptr(), off_dev.data_ptr()
        d.det_off_host, d.gt_off_host = ints(0, 2, 4), ints(0, 1, 3)
        d.masks, d.det_slot, d.gt_bits = u8.data_ptr(), i32.data_ptr(), i32.data_ptr()
        d.I, d.N, d.M, d.S, d.H, d.W = 2, 4, 3, 4, 8, 8
        d.gt_id = d.inter = d.uni = outs[1].data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    offsets = [dict(det_off_host=null_ints), dict(gt_off_host=null_ints), dict(det_off_host=ints(1, 2, 4)), dict(det_off_host=ints(0, 3, 2)),
               dict(det_off_host=ints(0, 2, 5)), dict(gt_off_host=ints(0, 1, 2)), dict(gt_off_host=ints(0, 4, 3)),
               dict(M=66, gt_off_host=ints(0, 65, 66)), dict(I=-1), dict(N=-1), dict(M=-1), dict(I=0), dict(det_off=None), dict(gt_off=None)]
    bad = offsets + [dict(S=-1), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(det=None), dict(gt=None), dict(gt_bits=None), dict(masks=None),
                     dict(det_slot=None), dict(gt_id=None), dict(inter=None), dict(uni=None)]
    for kw in bad:
        assert lib.a3d_eval_mask_counts(ctypes.byref(counts(**kw)), stream) == -1, kw
    assert lib.a3d_eval_mask_counts(None, stream) == -1
    assert lib.a3d_eval_mask_counts(ctypes.byref(counts(I=0, N=0, M=0, det_off_host=null_ints, gt_off_host=null_ints)), stream) == 0  # zero images
    assert lib.a3d_eval_mask_counts(ctypes.byref(counts(N=0, det_off_host=ints(0, 0, 0), M=64, gt_off_host=ints(0, 64, 64))), stream) == 0  # 64 is in range

    def match(**kw):
        d = _lib.EvalPlaneMatchDesc()
        d.det, d.gt, d.det_off, d.gt_off = f32.data_ptr(), f32.data_ptr(), off_dev.data_ptr(), off_dev.data_ptr()
        d.det_off_host, d.gt_off_host = ints(0, 2, 4), ints(0, 1, 3)
        d.inter = d.uni = i32.data_ptr()
        d.I, d.N, d.M = 2, 4, 3
        d.iou_thresh, d.normal_thresh, d.offset_thresh = 0.5, 30.0, 0.3
        d.box_iou = d.mask_iou = d.normal_err = d.offset_err = outs[0].data_ptr()
        d.gt_id = d.rank = outs[1].data_ptr()
        d.tp = outs[2].data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    nan = float("nan")
    bad = offsets + [dict(det=None), dict(gt=None), dict(inter=None), dict(uni=None), dict(gt_id=None), dict(rank=None), dict(box_iou=None),
                     dict(mask_iou=None), dict(normal_err=None), dict(offset_err=None), dict(tp=None), dict(iou_thresh=nan), dict(normal_thresh=nan),
                     dict(offset_thresh=nan)]
    for kw in bad:
        assert lib.a3d_eval_plane_match(ctypes.byref(match(**kw)), stream) == -1, kw
    assert lib.a3d_eval_plane_match(None, stream) == -1
    assert lib.a3d_eval_plane_match(ctypes.byref(match(I=0, N=0, M=0, det_off_host=null_ints, gt_off_host=null_ints)), stream) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)

    # the wrappers' own shape checks, and the evaluator's
    det, gt = torch.zeros(4, 14, device="cuda"), torch.zeros(3, 8, device="cuda")
    masks, slot, bits = torch.zeros(4, 8, 8, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(3, 2, dtype=torch.int32, device="cuda")
    ok = opt_ops.eval_mask_counts(det, [0, 2, 4], gt, [0, 1, 3], masks, slot, bits)
    assert [t.tolist() for t in ok] == [[0, 0, 0, 0], [0] * 4, [0] * 4]
    for args in ((det[:, :13].contiguous(), [0, 2, 4], gt, [0, 1, 3], masks, slot, bits), (det, [0, 2, 4], gt[:, :7].contiguous(), [0, 1, 3], masks, slot, bits),
                 (det, [0, 2, 4], gt, [0, 3], masks, slot, bits), (det, [0, 2, 4], gt, [0, 1, 3], masks[0], slot, bits),
                 (det, [0, 2, 4], gt, [0, 1, 3], masks, slot[:3], bits), (det, [0, 2, 4], gt, [0, 1, 3], masks, slot, bits[:, :1].contiguous())):
        with pytest.raises(ValueError):
            opt_ops.eval_mask_counts(*args)
    with pytest.raises(RuntimeError, match="A3D_ERR_ARG|-1"):
        opt_ops.eval_mask_counts(det, [0, 2, 3], gt, [0, 1, 3], masks, slot, bits)
    with pytest.raises(ValueError):
        opt_ops.eval_plane_match(det, [0, 2, 4], gt, [0, 1, 3], slot[:3], slot)
    with pytest.raises(RuntimeError, match="contiguous"):
        opt_ops.eval_mask_counts(det, [0, 2, 4], gt, [0, 1, 3], masks.bool(), slot, bits)
    tgt = evaluation_planes.PlaneGroundTruth([10, 11], gt.cpu().numpy(), bits, [0, 1, 3], [3], ["plane"], ["plane"], "cuda", (8, 8))
    ev = evaluation_planes.PlaneEvaluator(tgt)
    rec, cnt, keep = torch.zeros(2, 2, 20, device="cuda"), torch.ones(2, dtype=torch.int32, device="cuda"), torch.ones(2, 2, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="masks is None"):
        ev.process_records([10, 11], rec, cnt, None, keep)
    with pytest.raises(ValueError, match="image size"):
        ev.process_records([10, 11], rec, cnt, torch.zeros(2, 2, 8, 9, dtype=torch.uint8, device="cuda"), keep)
    ev.process_records([10, 11], rec, cnt, masks.reshape(2, 2, 8, 8), keep)
    res = ev.evaluate()  # (no box has an area, every plane is zero: statistics of zeros, three APs and their means)
    assert list(res)[:8] == list(P.STAT_KEYS) and len(res) == 14 and res["mean_normal"] == 0.0
