"""GPU suite: a3d_eval_match / a3d_eval_ap / a3d_depth_l1 (csrc/eval.hip) against tests/eval_ref.py, the law in numpy float64, then
ArtiEvaluator end to end on the fixture recorded from the reference (tests/golden/arti_eval.json) and the ABI's refusals."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import eval_ref as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(0, 2), (1, 1), (3, 0), (70, 5), (100, 33), (3, 2), (70, 1), (100, 2)]  # (detections, ground truths) per image
MARGIN = 1e-9


def _make_image(rng, D, G, twin_gt=False, corner=False):
    """Ground truths scattered over the image, detections jittered around them: several per ground truth, some of the wrong class,
    scores from a short list (duplicates), some ground truths without axis or normal."""
    gt_f, gt_i = np.zeros((G, 7), np.float32), np.zeros((G, 12), np.int32)
    for g in range(G):
        x, y, w, h = rng.uniform(0, 400), rng.uniform(0, 300), rng.uniform(60, 220), rng.uniform(60, 170)
        gt_f[g, :4] = [x, y, x + w, y + h]
        n = rng.normal(size=3)
        gt_f[g, 4:] = [-1, -1, -1] if rng.uniform() < 0.2 else n / np.linalg.norm(n)
        gt_i[g, :2] = rng.integers(0, 2, 2)  # class and kind, independently
        for base in (2, 7):
            gt_i[g, base:base + 4] = [rng.integers(0, 640), rng.integers(0, 480), rng.integers(0, 640), rng.integers(0, 480)]
            gt_i[g, base + 4] = rng.uniform() < 0.8
    if twin_gt:
        gt_f[1, :4] = gt_f[0, :4]  # the argmax tie: the lower index wins
    if corner and G:  # a box centred on (0.5, 479.5) with a translation axis of slope 1: the line meets the image in one corner only
        gt_f[0, :4] = [-50, 429, 51, 530]
        gt_i[0, 1], gt_i[0, 11] = 1, 1
    det = np.zeros((D, 14), np.float32)
    for d in range(D):
        if G:
            g = int(rng.integers(0, G))
            det[d, :4] = gt_f[g, :4] + rng.uniform(-1, 1, 4) * rng.choice([2.0, 10.0, 30.0])
            det[d, 5] = gt_i[g, 0] if rng.uniform() < 0.8 else 1 - gt_i[g, 0]
            det[d, 6:9] = (np.array([gt_f[g, 4], gt_f[g, 6], gt_f[g, 5]]) + rng.normal(size=3) * rng.choice([0.05, 0.4])) * rng.uniform(0.5, 2)
            line = gt_i[g, 7:11] if gt_i[g, 1] else gt_i[g, 2:6]
            ang = np.arctan2(line[3] - line[1], line[2] - line[0]) + rng.normal() * rng.choice([0.02, 0.3])
            det[d, 9:12] = [np.cos(ang), -np.sin(ang), rng.uniform(0, 1.5)]   # the line's normal, roughly
            det[d, 12:14] = [np.cos(ang), -np.sin(ang)]
        else:
            det[d, :4] = [10, 10, 100, 100]
        det[d, 4] = rng.choice([0.3, 0.5, 0.7, 0.9, round(float(rng.uniform()), 2)])
    if corner and D:
        det[0, :4] = gt_f[0, :4]
        det[0, 12:14] = [np.float32(np.sqrt(0.5)), -np.float32(np.sqrt(0.5))]
        det[1, 9:11] = [0.0, 1.0]   # sin == 0: the vertical line
        det[2, 9:11] = [1.0, 0.0]   # cos == 0: the horizontal line
        det[2, 12:14] = [1.0, 0.0]
    return dict(det=det, gt_f=gt_f, gt_i=gt_i)


@pytest.fixture(scope="module")
def dataset():
    """The seeded 8-image dataset and its reference, made once: resampled (fixed seeds) until every ea / normal_err keeps its
    distance from the thresholds in eval_ref."""
    for seed in range(100, 140):
        rng = np.random.default_rng(seed)
        images = [_make_image(rng, D, G, twin_gt=(k == 5), corner=(k == 6)) for k, (D, G) in enumerate(SHAPES)]
        matches = [E.match_image(**im) for im in images]
        v = [m["gt_id"] >= 0 for m in matches]
        if all((np.abs(m["ea"][ok] - 0.5) >= MARGIN).all() and (np.abs(m["normal_err"][ok] - 30.0) >= MARGIN).all() for m, ok in zip(matches, v)):
            return images, matches
    raise AssertionError("no seed keeps the margins")


def _tables(images):
    cat = lambda k, w, dt: torch.from_numpy(np.concatenate([im[k].reshape(-1, w) for im in images]).astype(dt)).cuda()
    off = lambda k: np.concatenate([[0], np.cumsum([len(im[k]) for im in images])]).tolist()
    return cat("det", 14, np.float32), off("det"), cat("gt_f", 7, np.float32), cat("gt_i", 12, np.int32), off("gt_f")


def test_the_dataset_holds_every_case_the_law_distinguishes(dataset):
    images, matches = dataset
    assert sorted({len(im["det"]) for im in images}) == [0, 1, 3, 70, 100] and sorted({len(im["gt_f"]) for im in images}) == [0, 1, 2, 5, 33]
    for m in matches:  # the margins, on the CPU, no case dropped
        ok = m["gt_id"] >= 0
        assert (np.abs(m["ea"][ok] - 0.5) >= MARGIN).all() and (np.abs(m["normal_err"][ok] - 30.0) >= MARGIN).all()
    big = matches[4]
    assert len(set(images[4]["det"][:, 4].tolist())) < 100                            # duplicate scores within an image
    assert (big["qual"] != big["tp"]).any() and big["tp"].any()                        # "already covered" decides
    assert ((big["qual"] & 1) == 0)[big["gt_id"] >= 0].any()                           # valid detections of the wrong class
    assert (big["gt_id"] < 0).any() and (big["gt_id"] >= 0).any()
    twin = matches[5]
    assert np.array_equal(images[5]["gt_f"][0, :4], images[5]["gt_f"][1, :4]) and (twin["gt_id"] != 1).all()  # the tie goes to index 0
    assert any((im["gt_i"][:, 6] == 0).any() and (im["gt_i"][:, 11] == 0).any() and (im["gt_f"][:, 4] == -1).any() for im in images)
    c = images[6]["det"][0]
    l = E.pred_line(c[:4], c[12], c[13], 0.0)
    assert l[:2] == l[2:] == [0.0, 479.0] and matches[6]["gt_id"][0] == 0 and matches[6]["ea"][0] == 0.0  # the degenerate predicted line
    assert sum(len(np.unique(m["tp"])) for m in matches) > 8


def test_match_kernel_equals_the_law(dataset):
    from articulation3d_amd import opt_ops

    images, matches = dataset
    det, det_off, gt_f, gt_i, gt_off = _tables(images)
    got = {k: v.cpu().numpy() for k, v in opt_ops.eval_match(det, det_off, gt_f, gt_i, gt_off).items()}
    want = {k: np.concatenate([m[k] for m in matches]) for k in ("gt_id", "iou", "ea", "normal_err", "rank", "tp")}
    assert np.array_equal(got["gt_id"], want["gt_id"]) and np.array_equal(got["rank"], want["rank"])
    assert got["iou"].dtype == np.float64 and got["iou"].tobytes() == want["iou"].tobytes()
    print("largest ea difference", np.abs(got["ea"] - want["ea"]).max(), "largest normal_err difference", np.abs(got["normal_err"] - want["normal_err"]).max())
    assert np.abs(got["ea"] - want["ea"]).max() <= 1e-12 and np.abs(got["normal_err"] - want["normal_err"]).max() <= 1e-12
    valid = want["gt_id"] >= 0
    assert np.array_equal(got["ea"][valid] > 0.5, want["ea"][valid] > 0.5) and np.array_equal(got["normal_err"][valid] < 30, want["normal_err"][valid] < 30)
    assert np.array_equal(got["ea"] == 0, want["ea"] == 0)  # invalid ground-truth axes and degenerate lines: exactly 0
    assert got["tp"].dtype == np.uint8 and np.array_equal(got["tp"], want["tp"])
    # other thresholds move the decisions with them
    loose = dict(filter_iou=0.3, iou_thresh=0.4, normal_thresh=60.0)
    got2 = opt_ops.eval_match(det, det_off, gt_f, gt_i, gt_off, **loose)
    want2 = [E.match_image(**im, **loose) for im in images]
    assert np.array_equal(got2["tp"].cpu().numpy(), np.concatenate([m["tp"] for m in want2]))
    assert np.array_equal(got2["gt_id"].cpu().numpy(), np.concatenate([m["gt_id"] for m in want2]))


def test_ap_kernel_equals_the_law():
    from articulation3d_amd import opt_ops

    rng = np.random.default_rng(5)
    # several passes of the workgroup (1024 entries each), npos == 0, empty, the hand case, exactly one pass, one past it, all false positives
    lengths, npos = [3500, 40, 0, 3, 1024, 1025, 9], [1500, 0, 5, 2, 600, 600, 4]
    segs = [rng.integers(0, 16, n).astype(np.uint8) for n in lengths]
    segs[0][2000:3000] |= rng.integers(0, 2, 1000).astype(np.uint8) * 15  # precision that rises again, passes later: the envelope carries over
    segs[3] = np.array([15, 0, 15], np.uint8)
    segs[6][:] = 0
    for m in range(4):  # at most npos true positives per class and metric, as the matcher guarantees
        for s, n in zip(segs, npos):
            on = np.flatnonzero((s >> m) & 1)
            s[on[n:]] &= ~np.uint8(1 << m)
    off = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    ap, n_entries = opt_ops.eval_ap(torch.from_numpy(np.concatenate(segs)).cuda(), off, npos)
    ap = ap.cpu().numpy()
    assert ap.shape == (4, 7) and n_entries.tolist() == lengths
    for c, (s, n) in enumerate(zip(segs, npos)):
        for m in range(4):
            want = E.voc_ap((s >> m) & 1, n) if n > 0 else 0.0
            assert abs(ap[m, c] - want) <= 1e-12, (c, m, ap[m, c], want)
    assert (ap[:, 3] == pytest.approx(5 / 6, abs=1e-12)) and (ap[:, 1] == 0).all() and (ap[:, 2] == 0).all() and (ap[:, 6] == 0).all()
    assert (ap[:, 0] > 0.1).all() and len(set(ap[:, 0].tolist())) == 4


@pytest.mark.parametrize("B,H,W", [(3, 48, 64), (1, 480, 640)])
def test_depth_l1_equals_a_float64_sum(B, H, W):
    from articulation3d_amd import opt_ops

    rng = np.random.default_rng(B * H)
    gt = (rng.uniform(0, 5, (B, H, W)) * (rng.uniform(size=(B, H, W)) < 0.7)).astype(np.float32)
    gt[0, 0, :5] = [1e-4, 1.0001e-4, 0.99e-4, 0.0, -1.0]  # the mask is gt > 1e-4 in fp32
    if B > 1:
        gt[1] = 0
    pred = rng.uniform(0, 5, (B, H, W)).astype(np.float32)
    want_s, want_n = E.depth_l1(pred, gt)
    s1, n1 = opt_ops.depth_l1(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda())
    s2, n2 = opt_ops.depth_l1(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda())
    assert s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes() and torch.equal(n1, n2)
    assert n1.tolist() == want_n.tolist()
    assert np.all(np.abs(s1.cpu().numpy() - want_s) <= 1e-10 * want_s)
    if B > 1:
        assert float(s1[1]) == 0.0 and int(n1[1]) == 0


# ---- ArtiEvaluator on the fixture recorded from the reference -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "arti_eval.json")) as f:
        return json.load(f)


def _instances(rows):
    from articulation3d_amd.structures import Boxes, Instances

    inst = Instances((480, 640))
    t = torch.from_numpy(rows).cuda()
    inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(t[:, :4]), t[:, 4], t[:, 5].long()
    inst.pred_plane, inst.pred_rot_axis, inst.pred_tran_axis = t[:, 6:9], t[:, 9:12], t[:, 12:14]
    return inst


def _records(rows_list, R=8, F=30):
    rec = torch.full((len(rows_list), R, F), 3.0)
    for k, r in enumerate(rows_list):
        rec[k, :len(r), :14] = torch.from_numpy(r)
    return rec.cuda(), torch.tensor([len(r) for r in rows_list], dtype=torch.int32).cuda()


def test_evaluator_end_to_end_on_the_reference_fixture(fixture):
    from articulation3d_amd import evaluation

    gt = evaluation.ArtiGroundTruth.from_coco(fixture["coco"], fixture["thing_classes"], device="cuda")
    preds = fixture["predictions"]
    rows, ids = [E.det_rows(p) for p in preds], [p["image_id"] for p in preds]
    rng = np.random.default_rng(11)
    depth_gt = (rng.uniform(0, 4, (len(ids), 24, 32)) * (rng.uniform(size=(len(ids), 24, 32)) < 0.8)).astype(np.float32)
    depth = rng.uniform(0, 4, (len(ids), 24, 32)).astype(np.float32)

    def run(how, order, splits):
        ev = evaluation.ArtiEvaluator(gt, fixture["filter_iou"], fixture["iou_thresh"], fixture["normal_threshold"])
        for part in np.array_split(np.asarray(order), splits):
            if how == "process":
                ev.process([{"image_id": ids[i], "depth": torch.from_numpy(depth_gt[i])} for i in part],
                           [{"instances": _instances(rows[i]), "depth": torch.from_numpy(depth[i]).cuda()} for i in part])
            else:
                rec, cnt = _records([rows[i] for i in part])
                ev.process_records([ids[i] for i in part], rec, cnt, torch.from_numpy(depth[part]).cuda(), torch.from_numpy(depth_gt[part]).cuda())
        return ev.evaluate(), ev

    n = len(ids)
    base, ev = run("process", range(n), 1)
    want = fixture["detection_metrics"]
    assert list(base) == list(want) + ["depth_l1_dist"]
    entries = dict(zip(gt.names, ev.n_entries.tolist()))
    for key, v in want.items():
        assert abs(base[key] - v) <= (entries[key.split(" - ")[1]] + 3) * 2.0 ** -24, key
    s, c = E.depth_l1(depth, depth_gt)
    assert abs(base["depth_l1_dist"] - np.mean(s / np.maximum(c, 1))) <= 1e-10 * base["depth_l1_dist"]
    # the law in numpy on the same tables, to float64 accuracy
    gt_f, gt_i = gt.gt_f.cpu().numpy(), gt.gt_i.cpu().numpy()
    images = [dict(det=r, gt_f=gt_f[gt.gt_off[i]:gt.gt_off[i + 1]], gt_i=gt_i[gt.gt_off[i]:gt.gt_off[i + 1]]) for i, r in enumerate(rows)]
    law, matches, _ = E.evaluate(images, gt.npos, gt.names)
    assert all(abs(base[k] - law[k]) <= 1e-12 for k in law)
    assert np.array_equal(ev.detections["tp"].cpu().numpy(), np.concatenate([m["tp"] for m in matches]))
    assert ev.detections["det_off"].tolist() == np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist()
    # the same bits whatever the call shape, the batching and the order
    perm = np.random.default_rng(2).permutation(n)
    for how, order, splits in (("records", range(n), 1), ("records", range(n), 2), ("process", perm, 3), ("records", perm, 5)):
        other, _ = run(how, order, splits)
        assert list(other) == list(base) and all(np.float64(other[k]).tobytes() == np.float64(base[k]).tobytes() for k in base), (how, splits)


def test_a_class_without_annotations_is_left_out_and_normals_can_replace_the_plane_columns(fixture):
    from articulation3d_amd import evaluation

    coco = dict(fixture["coco"], categories=fixture["coco"]["categories"] + [{"id": 9, "name": "spare_rot"}])
    gt = evaluation.ArtiGroundTruth.from_coco(coco, device="cuda")
    preds = fixture["predictions"]
    rows, ids = [E.det_rows(p) for p in preds], [p["image_id"] for p in preds]
    ev = evaluation.ArtiEvaluator(gt)
    ev.process([{"image_id": i} for i in ids], [{"instances": _instances(r)} for r in rows])
    res = ev.evaluate()
    assert list(res) == list(fixture["detection_metrics"]) and gt.npos.tolist()[2] == 0
    # records whose plane columns were negated by a negative fitted offset: the raw normals restore the result
    rec, cnt = _records(rows)
    normals = rec[:, :, 6:9].clone()
    rec[:, :, 6:9] *= -1
    flipped, fixed = evaluation.ArtiEvaluator(gt), evaluation.ArtiEvaluator(gt)
    flipped.process_records(ids, rec, cnt)
    fixed.process_records(ids, rec, cnt, normals=normals)
    assert fixed.evaluate() == res
    bad = flipped.evaluate()
    assert all(bad[k] == res[k] for k in res if "normal" not in k) and any(bad[k] != res[k] for k in res if "normal" in k)


def test_the_detectors_two_call_shapes_give_the_same_result(hip_model, oracle):
    """model(inputs) -> process and inference_batched -> process_records(normals=record_normals(out)) on the same frames, against
    ground truth made from the detections themselves: every AP is 1, so the record slots' normals are the detections' own."""
    from articulation3d_amd import evaluation

    model = hip_model
    saved = model.roi_heads.box_predictor.test_score_thresh
    model.roi_heads.box_predictor.test_score_thresh = 0.5
    try:
        frames = oracle.synthetic_frames(2, seed=3000)
        out = model.inference_batched(torch.from_numpy(frames).cuda())
        inputs = [{"image": torch.as_tensor(f.transpose(2, 0, 1).astype("float32")), "image_id": 10 + b} for b, f in enumerate(frames)]
        outs = model(inputs)
    finally:
        model.roi_heads.box_predictor.test_score_thresh = saved
    counts = out.rec_count.tolist()
    assert all(0 < c <= 60 for c in counts)
    normals = evaluation.record_normals(out)
    anns = []
    for b, c in enumerate(counts):
        rec = out.records[b, :c, :14].cpu().numpy().astype(np.float64)
        n = torch.nn.functional.normalize(normals[b, :c].cpu().double()).numpy()
        for k in range(c):
            x1, y1, x2, y2 = rec[k, :4]
            line = [int(x1), int(y1), int(x2), int(y2)]
            anns.append({"id": len(anns) + 1, "image_id": 10 + b, "category_id": int(rec[k, 5]) + 1, "bbox": [x1, y1, x2 - x1, y2 - y1],
                         "rot_axis": line, "tran_axis": line, "normal": [n[k, 0], n[k, 2], n[k, 1]]})
    coco = {"images": [{"id": 10}, {"id": 11}], "annotations": anns, "categories": [{"id": 1, "name": "arti_rot"}, {"id": 2, "name": "arti_tran"}]}
    gt = evaluation.ArtiGroundTruth.from_coco(coco, device="cuda")
    gt_depth = out.depth + 0.25
    a, b = evaluation.ArtiEvaluator(gt), evaluation.ArtiEvaluator(gt)
    a.process([dict(i, depth=gt_depth[k]) for k, i in enumerate(inputs)], outs)
    b.process_records([10, 11], out.records, out.rec_count, out.depth, gt_depth, normals=normals)
    ra, rb = a.evaluate(), b.evaluate()
    assert ra == rb and len(ra) > 1
    assert all(abs(v - 1.0) < 1e-12 for k, v in ra.items() if k.startswith(("bbox - ", "bbox+normal - "))), ra
    assert abs(ra["depth_l1_dist"] - 0.25) < 1e-6
    assert torch.equal(a.detections["det"], b.detections["det"]) and bool((a.detections["gt_id"] >= 0).all())
    # (the ground-truth normal is the detection's own, rounded to fp32: acos near 1 turns 1e-7 into a few hundredths of a degree)
    assert bool((a.detections["normal_err"] < 0.1).all()) and bool((a.detections["iou"] > 0.999).all())


def test_evaluate_through_a_one_rank_process_group(fixture, tmp_path):
    """The gather path of evaluate() on the one-rank rig: same dict as without a process group."""
    import torch.distributed as dist

    from articulation3d_amd import evaluation

    gt = evaluation.ArtiGroundTruth.from_coco(fixture["coco"], fixture["thing_classes"], device="cuda")
    preds = fixture["predictions"]

    def run():
        ev = evaluation.ArtiEvaluator(gt)
        rec, cnt = _records([E.det_rows(p) for p in preds])
        ones = torch.ones(len(preds), 8, 8, device="cuda")
        ev.process_records([p["image_id"] for p in preds], rec, cnt, ones * 1.5, ones)
        return ev.evaluate()

    alone = run()
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        grouped = run()
    finally:
        dist.destroy_process_group()
    assert grouped == alone and alone["depth_l1_dist"] == 0.5


def test_inconsistent_arguments_are_refused_before_any_launch():
    """A3D_ERR_ARG (-1) and untouched outputs.  Every pointer is a real allocation large enough for the widest reading of the
    arguments, so a call that was wrongly accepted would still stay inside it."""
    from articulation3d_amd import _lib

    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    big = lambda n, dt, fill=0: torch.full((n,), fill, dtype=dt, device="cuda")
    f32, i32, off_dev = big(4096, torch.float32), big(4096, torch.int32), big(64, torch.int32)
    outs = [big(4096, torch.float64, 7), big(4096, torch.int32, 7), big(4096, torch.uint8, 7)]
    ints = lambda *v: (ctypes.c_int * len(v))(*v)

    def match(**kw):
        d = _lib.EvalMatchDesc()
        d.det, d.gt_f, d.gt_i, d.det_off, d.gt_off = f32.data_ptr(), f32.data_ptr(), i32.data_ptr(), off_dev.data_ptr(), off_dev.data_ptr()
        d.det_off_host, d.gt_off_host = ints(0, 2, 4), ints(0, 1, 3)
        d.I, d.N, d.M, d.img_h, d.img_w = 2, 4, 3, 480, 640
        d.filter_iou, d.iou_thresh, d.normal_thresh = 0.7, 0.5, 30.0
        d.iou = d.ea = d.normal_err = outs[0].data_ptr()
        d.gt_id = d.rank = outs[1].data_ptr()
        d.tp = outs[2].data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    null_ints = ctypes.POINTER(ctypes.c_int)()
    bad = [dict(I=-1), dict(N=-1), dict(M=-1), dict(img_h=0), dict(img_w=0), dict(det_off_host=null_ints), dict(gt_off_host=null_ints),
           dict(det_off_host=ints(1, 2, 4)), dict(det_off_host=ints(0, 3, 2)), dict(det_off_host=ints(0, 2, 5)), dict(gt_off_host=ints(0, 1, 2)),
           dict(gt_off_host=ints(0, 4, 3)), dict(M=66, gt_off_host=ints(0, 65, 66)),  # G > 64
           dict(det=None), dict(gt_f=None), dict(gt_i=None), dict(det_off=None), dict(gt_off=None), dict(tp=None), dict(iou=None),
           dict(rank=None), dict(gt_id=None), dict(filter_iou=float("nan")), dict(I=0)]  # (I == 0 with rows left over)
    for kw in bad:
        assert lib.a3d_eval_match(ctypes.byref(match(**kw)), stream) == -1, kw
    assert lib.a3d_eval_match(None, stream) == -1
    assert lib.a3d_eval_match(ctypes.byref(match(I=0, N=0, M=0, det_off_host=null_ints, gt_off_host=null_ints)), stream) == 0  # zero images
    assert lib.a3d_eval_match(ctypes.byref(match(M=64, gt_off_host=ints(0, 64, 64), N=0, det_off_host=ints(0, 0, 0))), stream) == 0  # 64 is in range

    def ap(**kw):
        d = _lib.EvalApDesc()
        d.tp, d.seg_off_host, d.npos_host, d.C, d.ap, d.n_entries = outs[2].data_ptr(), ints(0, 2, 5), ints(3, 3), 2, outs[0].data_ptr(), outs[1].data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw in [dict(C=0), dict(C=65), dict(seg_off_host=null_ints), dict(npos_host=null_ints), dict(seg_off_host=ints(1, 2, 5)),
               dict(seg_off_host=ints(0, 3, 2)), dict(tp=None), dict(ap=None), dict(n_entries=None)]:
        assert lib.a3d_eval_ap(ctypes.byref(ap(**kw)), stream) == -1, kw
    assert lib.a3d_eval_ap(None, stream) == -1

    def depth(**kw):
        d = _lib.DepthL1Desc()
        d.pred, d.gt, d.B, d.H, d.W, d.sum, d.count = f32.data_ptr(), f32.data_ptr(), 2, 8, 8, outs[0].data_ptr(), outs[1].data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw in [dict(B=-1), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(pred=None), dict(gt=None), dict(sum=None), dict(count=None)]:
        assert lib.a3d_depth_l1(ctypes.byref(depth(**kw)), stream) == -1, kw
    assert lib.a3d_depth_l1(None, stream) == -1
    assert lib.a3d_depth_l1(ctypes.byref(depth(B=0, pred=None, gt=None, sum=None, count=None)), stream) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
