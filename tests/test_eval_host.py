"""Host suite of the evaluation feature: tests/eval_ref.py's statement of the law against the reference's recorded results
(tests/golden/axis_transforms.npz, tests/golden/arti_eval.json) and against answers worked out by hand, and the host side of
articulation3d_amd/evaluation.py (tables, argument checks, the order detections are collected in).  No device."""
import json
import os
import types

import numpy as np
import pytest
import torch

import eval_ref as E
from articulation3d_amd import evaluation
from articulation3d_amd.structures import Boxes, Instances
from articulation3d_amd.utils import opt_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "arti_eval.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def gt_cpu(fixture):
    return evaluation.ArtiGroundTruth.from_coco(fixture["coco"], fixture["thing_classes"], device="cpu")


def _images(fixture, gt):
    gt_f, gt_i = gt.gt_f.numpy(), gt.gt_i.numpy()
    return [dict(det=E.det_rows(p), gt_f=gt_f[gt.gt_off[i]:gt.gt_off[i + 1]], gt_i=gt_i[gt.gt_off[i]:gt.gt_off[i + 1]])
            for i, p in enumerate(fixture["predictions"])]


def test_line_law_reproduces_the_reference_on_all_64_golden_cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "axis_transforms.npz"))
    for ao, centers, want in ((z["ao"], z["ao_centers"], z["axis_back"]), (z["angle_offset"][:, :3], z["centers"], z["axis_round_trip"])):
        assert len(ao) == 32
        got = np.array([E.axis_line(a[0], a[1], a[2], c[0], c[1]) for a, c in zip(ao, centers)])
        assert np.array_equal(got, want.astype(np.float64))


def test_line_law_against_the_package_on_20000_random_lines():
    """k = -(cos / sin) in float64 where the package (as the reference) takes tan(float32(-arctan(cos / sin))): the same number up to
    rounding, so a truncation may land one pixel away, rarely."""
    rng = np.random.default_rng(0)
    n = 20000
    theta = rng.uniform(0, 2 * np.pi, n)
    off = rng.uniform(0, 3, n).astype(np.float32)
    cx, cy = rng.uniform(0, 640, n).astype(np.float32), rng.uniform(0, 480, n).astype(np.float32)
    s, c = np.sin(theta).astype(np.float32), np.cos(theta).astype(np.float32)
    want = opt_utils.angle_offset_to_axis(torch.from_numpy(np.stack([s, c, off], 1)), torch.from_numpy(np.stack([cx, cy], 1))).numpy()
    got = np.array([E.axis_line(s[i], c[i], off[i], cx[i], cy[i]) for i in range(n)])
    diff = np.abs(got - want)
    print("lines that differ:", int((diff.max(1) > 0).sum()), "largest difference:", diff.max())
    assert (diff.max(1) > 0).sum() <= 10 and diff.max() <= 1


def test_line_law_special_cases():
    assert E.axis_line(0.0, 1.0, 0.5, 100.25, 50.0) == [150.0, 0.0, 150.0, 479.0]        # sin == 0: vertical through x = 50 + 100.25
    assert E.axis_line(1.0, 0.0, 0.5, 100.0, 50.75) == [0.0, 100.0, 639.0, 100.0]        # k == 0: horizontal through y = 50 + 50.75
    assert E.axis_line(1.0, 1.0, 0.0, -500.0, -500.0) == [0.0, 0.0, 1.0, 1.0]            # never crosses the image
    assert E.axis_line(np.float32(np.sqrt(0.5)), np.float32(np.sqrt(0.5)), 0.0, 100.0, 100.0) == [0.0, 200.0, 200.0, 0.0]  # k = -1: left and top
    assert E.pred_line([90.0, 40.0, 110.0, 60.0], 0.0, 1.0, 0.5) == [150.0, 0.0, 150.0, 479.0]


def test_ea_known_answers():
    assert E.ea_score([10, 20, 300, 400], [10, 20, 300, 400]) == 1.0
    assert E.ea_score([100, 200, 300, 200], [200, 100, 200, 300]) == 0.0   # same mid point, perpendicular
    # a vertical line takes the -pi/2 branch: against the line at +45 degrees through the same mid point, d = 3pi/4 -> pi/4 -> sa = 1/4
    assert E.line_angle([200, 100, 200, 300]) == -np.pi / 2
    assert E.ea_score([200, 100, 200, 300], [100, 100, 300, 300]) == pytest.approx(0.25, abs=1e-15)
    # parallel lines 64 px apart: sa = 1, se = (1 - 64/640)^2
    assert E.ea_score([0, 100, 639, 100], [0, 164, 639, 164]) == pytest.approx(0.81, abs=1e-15)
    assert E.ea_score([5, 5, 5, 5], [0, 0, 10, 10]) == 0.0 and E.ea_score([0, 0, 10, 10], [7, 7, 7, 7]) == 0.0  # degenerate lines


def test_ap_known_answers():
    assert E.voc_ap([1, 0, 1], 2) == pytest.approx(5 / 6, abs=1e-15)   # scores .9 / .8 / .7: 1/2 * 1 + 1/2 * 2/3
    assert E.voc_ap([], 3) == 0.0
    assert E.voc_ap([0, 0, 0, 0], 2) == 0.0
    assert E.voc_ap([1, 1], 2) == 1.0
    assert E.voc_ap([0, 1], 4) == pytest.approx(1 / 8, abs=1e-15)


def test_normal_error_known_answers():
    assert E.normal_err([0, 0, 2], [0, 1, 0]) == 0.0            # plane (0,0,2) -> n = (0,0,1) -> (0,-1,0); ground truth (0,1,0) -> (0,-1,0)
    assert E.normal_err([0, 0, 2], [0, -1, 0]) == 180.0
    assert E.normal_err([1, 0, 0], [0, 0, 1]) == pytest.approx(90.0, abs=1e-12)
    assert E.normal_err([1, 0, 0], [-1, -1, -1]) == 180.0       # the invalid ground truth
    assert E.normal_err([3, 0, 0], [1.0000001, 0, 0]) == 0.0    # a dot product above 1 is clamped, not NaN
    assert E.normal_err([0, 0, 0], [1, 0, 0]) == pytest.approx(90.0, abs=1e-12)  # zero plane: n = 0


def test_covered_ground_truth_and_ranks_by_hand():
    """Two ground truths; four detections on the first, equal scores among them: rank by (score, index), the first qualifying
    detection per ground truth wins, per metric."""
    gt_f = np.array([[100, 100, 200, 200, 0, 0, 1], [300, 100, 400, 200, -1, -1, -1]], np.float32)
    gt_i = np.array([[0, 0, 150, 0, 150, 479, 1, 0, 0, 1, 1, 0], [1, 1, 0, 0, 1, 1, 0, 0, 150, 639, 150, 1]], np.int32)
    det = np.zeros((5, 14), np.float32)
    det[:, :4] = [[100, 100, 200, 200], [101, 100, 200, 200], [100, 100, 200, 200], [300, 100, 400, 200], [100, 100, 200, 170]]
    det[:, 4] = [0.5, 0.9, 0.5, 0.9, 0.95]
    det[:, 5] = [0, 0, 0, 1, 0]
    det[:, 6:9] = [[0, 1, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0]]   # plane (0,1,0) -> (0,0,1) = the first ground truth's normal
    det[:, 9:12] = [[0, 1, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0]]  # sin 0: the vertical line through the centre, x = 150; detection 1: horizontal
    det[:, 12:14] = [[0, 1], [0, 1], [0, 1], [1, 0], [0, 1]]                # detection 3: horizontal through y = 150
    m = E.match_image(det, gt_f, gt_i)
    assert m["rank"].tolist() == [3, 1, 4, 2, 0]
    assert m["gt_id"].tolist() == [0, 0, 0, 1, -1]         # detection 4: IoU 0.7 is not > 0.7
    assert m["iou"][4] == 0.7 and m["iou"][1] == 0.99
    # detection 1 (rank 1) takes bbox; its axis is horizontal (ea 0) and its normal 90 degrees off, so detection 0 (rank 3) takes the rest
    assert m["tp"].tolist() == [2 | 4 | 8, 1, 0, 1 | 2, 0]  # detection 3: right class and axis, invalid normal
    assert m["qual"].tolist() == [15, 1, 15, 3, 0]


def test_reference_results_on_the_fixture(fixture, gt_cpu):
    """eval_ref against what the reference's own evaluate_for_arti_axis returned.  The reference computes rec, prec and the sum in
    fp32: N entries give a sum of at most N + 1 terms, each a product of two roundings -- (N + 3) * 2^-24 bounds it; the float64 law
    carries none of it."""
    res, matches, entries = E.evaluate(_images(fixture, gt_cpu), gt_cpu.npos, gt_cpu.names)
    want = fixture["detection_metrics"]
    assert list(res) == list(want) and len(want) == 8
    for key, v in want.items():
        n = len(entries[gt_cpu.names.index(key.split(" - ")[1])])
        print(key, res[key], v, abs(res[key] - v), (n + 3) * 2.0 ** -24)
        assert abs(res[key] - v) <= (n + 3) * 2.0 ** -24, key
    assert 0 < min(want.values()) and len(set(want.values())) == 8  # the fixture tells the four metrics and the two classes apart


def test_ground_truth_tables(fixture, gt_cpu):
    coco = fixture["coco"]
    assert len(gt_cpu) == 40 and gt_cpu.gt_off.tolist() == list(range(41)) and gt_cpu.npos.sum() == 40 and (gt_cpu.npos > 0).all()
    gt_f, gt_i = gt_cpu.gt_f.numpy(), gt_cpu.gt_i.numpy()
    seen = set()
    for r, ann in enumerate(coco["annotations"]):
        x, y, w, h = ann["bbox"]
        assert gt_f[r, :4].tolist() == [x, y, x + w, y + h]
        assert gt_i[r, 0] == ann["category_id"] - 1 and gt_i[r, 1] == (0 if ann["category_id"] == 1 else 1)
        assert gt_i[r, 6] == (ann["rot_axis"] is not None) and gt_i[r, 11] == (ann["tran_axis"] is not None)
        assert gt_f[r, 4:].tolist() == ([-1, -1, -1] if ann["normal"] is None else np.float32(ann["normal"]).tolist())
        seen.add((ann["rot_axis"] is None, ann["tran_axis"] is None, ann["normal"] is None or ann["normal"] == [-1, -1, -1]))
        if ann["tran_axis"] is not None:  # a translation line goes through the box centre (offset zeroed), parallel to the annotation
            l, a = gt_i[r, 7:11].astype(np.float64), np.asarray(ann["tran_axis"], np.float64)
            d_l, d_a = l[2:] - l[:2], a[2:] - a[:2]
            assert abs(d_l[0] * d_a[1] - d_l[1] * d_a[0]) / (np.linalg.norm(d_l) * np.linalg.norm(d_a)) < 0.01
    assert len(seen) >= 4  # missing axes and invalid normals are in the fixture


def test_malformed_arguments_fail_on_the_host(fixture, gt_cpu):
    coco = fixture["coco"]
    with pytest.raises(ValueError, match="neither"):
        evaluation.ArtiGroundTruth.from_coco(coco, ["arti_rot", "door"], device="cpu")
    with pytest.raises(ValueError, match="thing_classes"):
        evaluation.ArtiGroundTruth.from_coco(coco, ["arti_rot"], device="cpu")
    bad = dict(coco, annotations=coco["annotations"][:1] + [dict(coco["annotations"][1], category_id=7)])
    with pytest.raises(ValueError, match="category_id"):
        evaluation.ArtiGroundTruth.from_coco(bad, fixture["thing_classes"], device="cpu")
    crowded = dict(coco, annotations=[dict(coco["annotations"][0], id=k) for k in range(65)])
    with pytest.raises(ValueError, match="at most 64"):
        evaluation.ArtiGroundTruth.from_coco(crowded, fixture["thing_classes"], device="cpu")
    ev = evaluation.ArtiEvaluator(gt_cpu)
    with pytest.raises(ValueError, match="not in the ground truth"):
        ev.process([{"image_id": 99999}], [{}])
    iid = coco["images"][0]["id"]
    ev.process([{"image_id": iid}], [{}])
    with pytest.raises(ValueError, match="processed before"):
        ev.process([{"image_id": iid}], [{}])
    inst = Instances((480, 640))
    inst.pred_boxes, inst.scores = Boxes(torch.zeros(1, 4)), torch.zeros(1)
    with pytest.raises(ValueError, match="lack pred_classes"):
        ev.process([{"image_id": coco["images"][1]["id"]}], [{"instances": inst}])
    with pytest.raises(ValueError, match=r"want \[B,R,>=14\]"):
        ev.process_records([coco["images"][2]["id"]], torch.zeros(1, 4, 13), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="normals"):
        ev.process_records([coco["images"][2]["id"]], torch.zeros(1, 4, 14), torch.zeros(1, dtype=torch.int32), normals=torch.zeros(1, 3, 3))
    with pytest.raises(ValueError, match="go together"):
        ev.process_records([coco["images"][2]["id"]], torch.zeros(1, 4, 14), torch.zeros(1, dtype=torch.int32), depth=torch.zeros(1, 4, 4))


def _instances(rows):
    inst = Instances((480, 640))
    t = torch.from_numpy(rows)
    inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(t[:, :4]), t[:, 4], t[:, 5].long()
    inst.pred_plane, inst.pred_rot_axis, inst.pred_tran_axis = t[:, 6:9], t[:, 9:12], t[:, 12:14]
    return inst


def test_detections_are_collected_in_ground_truth_order_whatever_the_call_order(fixture, gt_cpu):
    preds = fixture["predictions"]
    rows = [E.det_rows(p) for p in preds]
    want = np.concatenate(rows)
    want_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    ids = [p["image_id"] for p in preds]

    a = evaluation.ArtiEvaluator(gt_cpu)
    a.process([{"image_id": i} for i in ids], [{"instances": _instances(r)} for r in rows])
    b = evaluation.ArtiEvaluator(gt_cpu)  # permuted, partly as packed records with dead slots, some images never processed with D = 0
    order = np.random.default_rng(3).permutation(len(ids))
    rec_part, inst_part = order[:17], order[17:]
    R = 8
    records = torch.full((len(rec_part), R, 20), 7.0)
    counts = torch.zeros(len(rec_part), dtype=torch.int32)
    for k, i in enumerate(rec_part):
        records[k, :len(rows[i]), :14] = torch.from_numpy(rows[i])
        counts[k] = len(rows[i])
    b.process_records([ids[i] for i in rec_part[:9]], records[:9], counts[:9])
    b.process([{"image_id": ids[i]} for i in inst_part if len(rows[i])], [{"instances": _instances(rows[i])} for i in inst_part if len(rows[i])])
    b.process_records([ids[i] for i in rec_part[9:]], records[9:], counts[9:])
    for ev in (a, b):
        det, det_off = ev._collect()
        assert det.numpy().tobytes() == want.tobytes() and det_off.tolist() == want_off.tolist()


def _gather_worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ev = evaluation.ArtiEvaluator.__new__(evaluation.ArtiEvaluator)  # (_gather reads no state)
    table = torch.arange((3 * rank + 2) * 6, dtype=torch.float32).reshape(-1, 6) + 1000 * rank   # 2 rows on rank 0, 5 on rank 1
    depth = torch.full((2 - 2 * rank, 6), 0.5 + rank)                                            # 2 rows on rank 0, none on rank 1
    got_t, got_d = ev._gather(table, depth)
    q.put((rank, got_t.tolist(), got_d.tolist()))
    dist.barrier()
    dist.destroy_process_group()


def test_compact_rows_of_two_ranks_are_gathered_in_rank_order():
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    want_t = torch.cat([torch.arange(12, dtype=torch.float32).reshape(-1, 6), torch.arange(30, dtype=torch.float32).reshape(-1, 6) + 1000]).tolist()
    for rank, got_t, got_d in res:
        assert got_t == want_t and got_d == [[0.5] * 6] * 2, rank


def test_record_normals_follow_the_packers_slot_order():
    """Record k of a frame is its k-th kept detection; its head row is row_offset[b] + r."""
    B, R = 3, 5
    count = torch.tensor([4, 0, 5], dtype=torch.int32)
    keep = torch.tensor([[1, 0, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 1]], dtype=torch.int32)
    row_offset = torch.tensor([0, 4, 4, 9], dtype=torch.int32)
    plane = torch.arange(27, dtype=torch.float32).reshape(9, 3)
    out = types.SimpleNamespace(keep=keep, det=types.SimpleNamespace(total=9, pred_plane=plane, count=count, row_offset=row_offset))
    got = evaluation.record_normals(out)
    want = torch.zeros(B, R, 3)
    want[0, :3] = plane[[0, 2, 3]]
    want[2, :2] = plane[[6, 8]]
    assert torch.equal(got, want)
