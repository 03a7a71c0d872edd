"""Host suite of the plane evaluation: tests/plane_eval_ref.py's statement of the law against the reference's recorded results
(tests/golden/plane_eval.json) and against answers worked out by hand, the conditions the fixture was recorded under, and the host
side of articulation3d_amd/evaluation_planes.py (ground-truth tables, refusals, the record -> mask slot table).  No device."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

import plane_eval_ref as P
from articulation3d_amd import _lib, evaluation_planes
from articulation3d_amd.utils import rle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "plane_eval.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def law(fixture):
    images, npos, names = P.fixture_images(fixture)
    res, matches, entries = P.evaluate(images, npos, names, fixture["iou_thresh"], fixture["normal_threshold"], fixture["offset_threshold"])
    return images, npos, names, res, matches, entries


def test_the_law_gives_the_references_recorded_metrics(fixture, law):
    _images, _npos, names, res, _matches, entries = law
    want = fixture["metrics"]
    assert list(res) == list(want)  # the reference's keys in the reference's order
    assert list(want)[:8] == list(P.STAT_KEYS) and not any("spare" in k for k in want)  # (a class without annotations is left out)
    bounds = P.reference_bounds(fixture, names, entries)
    for key, v in want.items():
        print(f"{key}: law {res[key]!r} reference {v!r} |diff| {abs(res[key] - v):.3e} bound {bounds[key]:.3e}")
        assert abs(res[key] - v) <= bounds[key], key
    assert max(fixture["stat_gap"].values()) < 1e-3  # (fp32 against float64 on errors of tens of degrees)


def test_the_fixture_holds_the_conditions_it_was_recorded_under(fixture, law):
    """tools/make_plane_eval_golden.py's own check, on the committed file, with no case dropped; plus what it stands on."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_plane_eval_golden as tool
    finally:
        sys.path.pop(0)
    tool.check_conditions(fixture["coco"], fixture["predictions"])
    images, npos, _names, _res, matches, _ = law
    assert fixture["image_hw"] == [48, 64] and len(images) == len(fixture["coco"]["images"]) >= 10
    assert npos.tolist()[2] == 0 and min(npos.tolist()[:2]) > 0
    assert any(len(im["det"]) == 0 for im in images) and max(len(im["gt"]) for im in images) >= 3
    assert (np.concatenate([m["normal_err"] for m in matches]) > 150).any()  # a negated plane (negative refitted offset) is in the data
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "plane_eval.json")) < 66 * 1024


def test_compare_planes_and_counts_by_hand():
    n, o = P.compare_planes([0, 0, 2], [0, 0, 2])
    assert n == 0 and o == 0
    n, o = P.compare_planes([0, 0, 2], [0, 0, -0.5])
    assert 179 < n < 180 and abs(o - 1.5) < 1e-15  # (the 1e-5 in the divisors leaves |n_p - n_g| a few 1e-5 short of 2: asin is steep there)
    n, o = P.compare_planes([3, 0, 0], [0, 1, 0])
    assert abs(n - 90) < 1e-3 and abs(o - 2) < 1e-12  # (the 1e-5 in the divisor leaves the normals a little short of unit length)
    n, o = P.compare_planes([0, 0, 0], [0, 0, 1])  # a zero plane: the normal is 0 / 1e-5 = 0, one unit from any unit normal
    assert abs(n - 60) < 1e-3 and abs(o - 1) < 1e-12
    # pack / unpack: bit p & 31 of word p >> 5, spare bits dropped
    m = np.zeros((1, 5, 7), np.uint8)
    m[0, 0, 0] = m[0, 4, 6] = 2
    bits = P.pack_bits(m)
    assert bits.shape == (1, 2) and bits[0, 0] == 1 and bits[0, 1] == 1 << 2
    bits[0, 1] |= np.uint32(0xFFFFFFF8)
    assert np.array_equal(P.unpack_bits(bits, 35)[0], m.reshape(-1) != 0)
    # counts: the ground truth is chosen by the BOX (a tie goes to the lower index), the counts come from the masks
    det = np.zeros((3, 14), np.float32)
    det[:, :4] = [[0, 0, 4, 4], [3, 0, 7, 4], [0, 0, 4, 4]]
    gt = np.zeros((2, 8), np.float32)
    gt[:, :4] = [[0, 0, 4, 4], [0, 0, 4, 4]]
    masks = np.zeros((2, 5, 7), np.uint8)
    masks[0, :4, :4] = 1
    masks[1, :4, 3:7] = 255
    gt_masks = np.zeros((2, 5, 7), np.uint8)
    gt_masks[0, :2, :4] = 1
    gt_id, inter, uni = P.mask_counts(det, gt, masks, [0, 1, 9], P.pack_bits(gt_masks), 35)
    assert gt_id.tolist() == [0, 0, 0] and inter.tolist() == [8, 2, 0] and uni.tolist() == [16, 22, 8]  # (slot 9: an empty mask)
    gt_id, inter, uni = P.mask_counts(det, gt[:0], masks, [0, 1, 9], np.zeros((0, 2), np.uint32), 35)
    assert gt_id.tolist() == [-1, -1, -1] and inter.tolist() == [0, 0, 0] and uni.tolist() == [16, 16, 0]
    # match: the first qualifying detection by rank takes the ground truth, per metric; two empty masks have IoU 0
    det[:, 4], det[:, 6:9] = [0.5, 0.9, 0.7], [0, 0, 1]
    gt[:, 4:7] = [0, 0, 1.2]
    m = P.match_image(det, gt, [8, 9, 0], [16, 10, 0])
    assert m["rank"].tolist() == [2, 0, 1] and m["gt_id"].tolist() == [0, 0, 0]
    assert m["qual"].tolist() == [1 | 4, 2 | 4, 1 | 4] and m["tp"].tolist() == [0, 2 | 4, 1] and m["mask_iou"].tolist() == [0.5, 0.9, 0.0]
    m = P.match_image(det, gt[:0], [0, 0, 0], [16, 16, 0])
    assert m["gt_id"].tolist() == [-1] * 3 and m["tp"].tolist() == [0] * 3 and (m["normal_err"] == 180).all() and np.isinf(m["offset_err"]).all()
    stats = evaluation_planes.plane_statistics([5.0, 20.0, 40.0], [0.1, 0.4, 0.6])
    assert list(stats) == list(P.STAT_KEYS) == list(evaluation_planes.STAT_KEYS)
    assert stats["%normal<10"] == pytest.approx(100 / 3) and stats["%offset<0.5"] == pytest.approx(200 / 3) and stats["median_normal"] == 20.0
    assert evaluation_planes.plane_statistics([], []) == {}
    assert evaluation_planes.metric_keys() == P.metric_keys() == ("box_ap@0.5", "mask_ap@0.5", "plane_ap@iou0.5normal30.0offset0.3")


def test_ground_truth_tables_are_parsed_as_the_law_parses_them(fixture, law):
    images, npos, names, *_ = law
    t = evaluation_planes.parse_plane_coco(fixture["coco"], fixture["thing_classes"], fixture["image_hw"])
    assert t["names"] == names and t["npos"].tolist() == npos.tolist() and t["gt"].dtype == np.float32 and t["gt"].shape[1] == _lib.PLANE_GT_COLS == 8
    assert t["image_ids"] == [im["id"] for im in fixture["coco"]["images"]]
    assert t["gt_off"].tolist() == np.concatenate([[0], np.cumsum([len(im["gt"]) for im in images])]).tolist()
    assert t["gt"].tobytes() == np.concatenate([im["gt"] for im in images]).tobytes()
    dense = np.stack([evaluation_planes.decode_mask(s, fixture["image_hw"]) for s in t["segmentations"]])
    assert np.array_equal(dense, np.concatenate([im["gt_masks"] for im in images]))
    # an RLE with uncompressed counts, or a bytes string, decodes to the same mask
    seg = t["segmentations"][0]
    runs = rle._from_string(seg["counts"])
    for other in ({"size": seg["size"], "counts": runs}, {"size": seg["size"], "counts": seg["counts"].encode("ascii")}):
        assert np.array_equal(evaluation_planes.decode_mask(other, fixture["image_hw"]), dense[0])
    with pytest.raises(ValueError, match="runs sum"):
        evaluation_planes.decode_mask({"size": seg["size"], "counts": runs[:-1]}, fixture["image_hw"])


def test_from_coco_refuses_what_it_cannot_evaluate(fixture):
    hw = fixture["image_hw"]

    def broken(change):
        coco = copy.deepcopy(fixture["coco"])
        change(coco)
        return coco

    def polygon(c):
        c["annotations"][3]["segmentation"] = [[1.0, 1.0, 9.0, 1.0, 9.0, 9.0]]

    def no_plane(c):
        del c["annotations"][2]["plane"]

    def crowd(c):
        first = c["annotations"][0]
        c["annotations"] += [dict(first, id=1000 + k) for k in range(64)]

    cases = [(polygon, "convert it to RLE"), (no_plane, "no `plane`"), (crowd, "at most 64"),
             (lambda c: c["annotations"][1]["segmentation"].update(size=[hw[0], hw[1] + 1]), "is not image_hw"),
             (lambda c: c["annotations"][1].update(category_id=99), "unknown category_id"),
             (lambda c: c["annotations"][1].update(image_id=-5), "unknown image_id"),
             (lambda c: c["annotations"][1].update(segmentation="abc"), "RLE dict"),
             (lambda c: c["images"].append(dict(c["images"][0])), "duplicate image ids")]
    for change, message in cases:
        for parse in (lambda c: evaluation_planes.parse_plane_coco(c, None, hw), lambda c: evaluation_planes.PlaneGroundTruth.from_coco(c, None, "cpu", hw)):
            with pytest.raises(ValueError, match=message):
                parse(broken(change))
    with pytest.raises(ValueError, match="is not image_hw"):
        evaluation_planes.parse_plane_coco(fixture["coco"])  # (the default image size is the reference's 480 x 640)
    with pytest.raises(ValueError, match="thing_classes"):
        evaluation_planes.parse_plane_coco(fixture["coco"], ["a"], hw)
    # 64 annotations in one image are in range
    ok = broken(lambda c: c["annotations"].extend(dict(c["annotations"][0], id=1000 + k) for k in range(64 - sum(a["image_id"] == c["annotations"][0]["image_id"] for a in c["annotations"]))))
    assert max(np.diff(evaluation_planes.parse_plane_coco(ok, None, hw)["gt_off"])) == 64
    # the masks are packed by the GPU: a cpu device is refused there, after every check above
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation_planes.PlaneGroundTruth.from_coco(fixture["coco"], fixture["thing_classes"], "cpu", hw)


def test_record_slots_follow_the_keep_flags():
    keep = torch.tensor([[0, 3, 0, 1, 1], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 7]], dtype=torch.uint8)
    got = evaluation_planes.record_slots(keep).reshape(4, 5).tolist()
    assert got == [[1, 3, 4, -1, -1], [-1] * 5, [10, 11, 12, 13, 14], [19, -1, -1, -1, -1]]
    assert evaluation_planes.record_slots(keep).dtype == torch.int32


def test_evaluator_argument_checks_come_before_any_device_work(fixture):
    """A PlaneEvaluator over hand-made (empty) tables on the cpu: the refusals need no kernel."""
    gt = evaluation_planes.PlaneGroundTruth([10, 11], np.zeros((0, 8), np.float32), torch.zeros((0, 96), dtype=torch.int32), [0, 0, 0], [0], ["plane"],
                                            ["plane"], "cpu", (48, 64))
    ev = evaluation_planes.PlaneEvaluator(gt)
    rec, cnt, keep = torch.zeros(2, 4, 20), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.uint8)
    masks = torch.zeros(2, 4, 48, 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="masks is None"):
        ev.process_records([10, 11], rec, cnt, None, keep)
    with pytest.raises(ValueError, match="want \\[B,R,>=14\\]"):
        ev.process_records([10, 11], rec[:, :, :9], cnt, masks, keep)
    with pytest.raises(ValueError, match="want \\[B,R,H,W\\]"):
        ev.process_records([10, 11], rec, cnt, masks[:, :3], keep)
    with pytest.raises(ValueError, match="want \\[B,R,H,W\\]"):
        ev.process_records([10, 11], rec, cnt, masks, keep[:, :3])
    with pytest.raises(ValueError, match="image size"):
        ev.process_records([10, 11], rec, cnt, masks[:, :, :40], keep)
    with pytest.raises(ValueError, match="go together"):
        ev.process_records([10, 11], rec, cnt, masks, keep, depth=torch.zeros(2, 4, 4))
    assert not ev._seen and not ev._rows  # a refused batch leaves no trace
    with pytest.raises(ValueError, match="not in the ground truth"):
        ev.process_records([10, 12], rec, cnt, masks, keep)
    with pytest.raises(ValueError, match="int32"):
        evaluation_planes.PlaneGroundTruth([10], np.zeros((1, 8), np.float32), torch.zeros((1, 95), dtype=torch.int32), [0, 1], [1], ["plane"], ["plane"], "cpu", (48, 64))
