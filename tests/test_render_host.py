"""Host side of the visualisation panels (no GPU): build_layers on hand-made Instances, checked through tests/render_ref.py
(the law of a3d_render_panels in numpy), and render_ref's normal panel against the reference's get_normal_map formula."""
import numpy as np
import pytest
import torch

import render_ref as R

H, W = 24, 40
ROT, TRAN = (0, 130, 200), (230, 25, 75)


def _inst(boxes, classes, scores, rot=None, tran=None, masks=None, planes=None, hw=(H, W)):
    from articulation3d_amd.structures import Boxes, Instances

    n = len(boxes)
    inst = Instances(hw)
    inst.pred_boxes = Boxes(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4))
    inst.scores = np.asarray(scores, np.float32)
    inst.pred_classes = torch.tensor(classes, dtype=torch.int64)
    inst.pred_planes = torch.tensor(planes if planes is not None else [[0.0, 0.0, 1.0]] * n, dtype=torch.float32).reshape(-1, 3)
    inst.pred_rot_axis = torch.tensor(rot if rot is not None else [[1.0, 0.0, 0.0]] * n, dtype=torch.float32).reshape(-1, 3)
    inst.pred_tran_axis = torch.tensor(tran if tran is not None else [[0.0, 1.0]] * n, dtype=torch.float32).reshape(-1, 2)
    inst.pred_masks = torch.tensor(masks if masks is not None else np.zeros((n,) + tuple(hw)), dtype=torch.float32).reshape((-1,) + tuple(hw))
    return inst


def test_layer_order_counts_colours_alphas_and_score_filter():
    from articulation3d_amd import _lib, render

    masks = np.zeros((4, H, W), np.float32)
    masks[:, 2:6, 2:6] = 1
    # areas: #0 = 100, #1 = 300, #2 = 100 (tie with #0), #3 = 500 but below the threshold
    f1 = _inst([[2, 2, 12, 12], [5, 3, 35, 13], [20, 10, 30, 20], [1, 1, 26, 21]], [0, 1, 1, 0], [0.9, 0.8, 0.95, 0.7], masks=masks)
    preds = [_inst([], [], []), f1]
    t = render.build_layers(preds, H, W, mask_alpha=0.5)
    assert t.layer_off.tolist() == [0, 0, 9] and t.layer_off.dtype == np.int32  # 3 drawn instances x (mask, arrow, box); the empty frame has none
    L = t.layers
    assert L["kind"].tolist() == [_lib.RENDER_MASK] * 3 + [_lib.RENDER_POLY] * 6
    assert L["alpha"].tolist() == [128] * 3 + [256] * 3 + [128] * 3
    colours = [tuple(c[:3]) for c in L["color"].tolist()]
    # masks and boxes: descending area, ties in ascending index (1, 0, 2); arrows: ascending index (0, 1, 2)
    assert colours == [TRAN, ROT, TRAN, ROT, TRAN, TRAN, TRAN, ROT, TRAN]
    assert L["p0"][:3].tolist() == [1, 0, 2] and t.mask_keys == [(1, 0), (1, 1), (1, 2), (1, 3)]
    # the normal panel takes every instance of the frame, drawn or not
    assert t.inst_off.tolist() == [0, 0, 4] and t.inst_row.tolist() == [0, 1, 2, 3]
    # arrow layers: 4 pieces each (shaft, two head triangles, core triangle); box layers: 4 strips
    assert [int(l["p1"] - l["p0"]) for l in L[3:]] == [4, 4, 4, 4, 4, 4]
    assert t.pieces["n"].tolist() == [4, 3, 3, 3] * 3 + [4] * 12
    # score == threshold is not drawn (strict >), and a higher threshold drops more
    assert render.build_layers(preds, H, W, conf_threshold=0.9).layer_off.tolist() == [0, 0, 2]
    # mask_alpha = 0 (the default, as the reference's `#masks=masks`): no MASK layer at all
    t0 = render.build_layers(preds, H, W)
    assert t0.layer_off.tolist() == [0, 0, 6] and (t0.layers["kind"] == _lib.RENDER_POLY).all()
    with pytest.raises(ValueError):
        render.build_layers(preds, H, W, mask_alpha=1.5)


def test_degenerate_axis_gives_no_arrow_layer(monkeypatch):
    from articulation3d_amd import render

    preds = [_inst([[4, 4, 30, 20], [6, 2, 20, 18]], [0, 0], [0.9, 0.9])]
    assert render.build_layers(preds, H, W).layer_off.tolist() == [0, 4]
    real = render.axis_end_points
    monkeypatch.setattr(render, "axis_end_points", lambda inst, i: (7.0, 9.0, 7.0, 9.0) if i == 0 else real(inst, i))
    t = render.build_layers(preds, H, W)
    assert t.layer_off.tolist() == [0, 3] and t.layers["alpha"].tolist() == [256, 128, 128]
    assert render.arrow_polys(3.0, 3.0, 3.0, 3.0) == []


def test_axis_end_points_follow_draw_pred():
    """angle_offset_to_axis in the box's own frame (H = h_box, W = w_box, centre = half the box), shifted by the box origin; a
    translation axis takes row 0 of pred_tran_axis with the zero offset appended (draw_pred zips the table with one centre)."""
    from articulation3d_amd import render
    from articulation3d_amd.utils.opt_utils import angle_offset_to_axis

    rot = [[0.6, 0.8, 0.02], [0.0, 1.0, 0.0]]
    tran = [[0.8, 0.6], [1.0, 0.0]]
    inst = _inst([[4, 2, 34, 22], [10, 5, 30, 17]], [0, 1], [0.9, 0.9], rot=rot, tran=tran)
    for i, ao in ((0, rot[0]), (1, tran[0] + [0.0])):
        b = inst.pred_boxes.tensor[i]
        w, h = float(b[2] - b[0]), float(b[3] - b[1])
        want = angle_offset_to_axis(torch.tensor([ao]), torch.tensor([[w / 2, h / 2]]), H=h, W=w)[0].float()
        want = (want[0] + b[0], want[1] + b[1], want[2] + b[0], want[3] + b[1])
        assert render.axis_end_points(inst, i) == tuple(float(v) for v in want)


def test_box_strips_are_disjoint_and_cover_the_ring():
    from articulation3d_amd import render

    box = [5.3, 4.2, 30.7, 18.9]
    t = render.build_layers([_inst([box], [0], [0.9])], H, W)
    layer = t.layers[-1]
    assert int(layer["alpha"]) == 128 and int(layer["p1"] - layer["p0"]) == 4
    strips = [R.piece_coverage(t.pieces[q], H, W) for q in range(int(layer["p0"]), int(layer["p1"]))]
    assert sum(s.astype(int) for s in strips).max() == 1  # disjoint
    cx, cy = np.arange(W) + 0.5, np.arange(H) + 0.5
    outer = ((cx >= box[0] - 1.25) & (cx <= box[2] + 1.25))[None, :] & ((cy >= box[1] - 1.25) & (cy <= box[3] + 1.25))[:, None]
    inner = ((cx > box[0] + 1.25) & (cx < box[2] - 1.25))[None, :] & ((cy > box[1] + 1.25) & (cy < box[3] - 1.25))[:, None]
    assert np.array_equal(np.logical_or.reduce(strips), outer & ~inner) and (outer & ~inner).sum() > 100


def test_arrow_covers_the_tip_side_only():
    from articulation3d_amd import render

    x0, y0, x1, y1 = 4.0, 6.0, 36.0, 18.0  # 34 px long: the full-size head (25 px) fits
    polys = render.arrow_polys(x0, y0, x1, y1)
    assert [len(p) for p in polys] == [4, 3, 3, 3]
    pieces = np.zeros(4, render.PIECE_DTYPE)
    for k, p in enumerate(polys):
        pieces[k]["n"], pieces[k]["abc"] = len(p), render.convex_piece(p)
    cov = np.logical_or.reduce([R.piece_coverage(q, H, W) for q in pieces])
    d = np.array([x1 - x0, y1 - y0]) / np.hypot(x1 - x0, y1 - y0)
    yy, xx = np.mgrid[0:H, 0:W] + 0.5
    along = (xx - x0) * d[0] + (yy - y0) * d[1]  # 0 at the tail, length at the tip
    across = np.abs(-(xx - x0) * d[1] + (yy - y0) * d[0])
    length = np.hypot(x1 - x0, y1 - y0)
    assert cov.any() and not cov[(along < 0) | (along > length)].any()  # nothing beyond the segment, at either end
    assert across[cov & (along < length - 25)].max() <= 10 / 6 + 1e-6  # the shaft is 10/3 wide ...
    assert across[cov & (along > length - 25)].max() > 5.0  # ... and the head, on the tip side, is much wider
    assert cov[int(y1 - 2 * d[1]), int(x1 - 2 * d[0])] and cov[int(y0 + 2 * d[1]), int(x0 + 2 * d[0])]


def test_arrow_pieces_cover_exactly_matplotlibs_fancyarrow():
    """The four convex pieces against the polygon matplotlib itself builds for the reference's draw_arrow call."""
    patches = pytest.importorskip("matplotlib.patches")
    from matplotlib.path import Path

    from articulation3d_amd import render

    x0, y0, x1, y1 = 4.0, 6.0, 36.0, 18.0
    pieces = np.zeros(4, render.PIECE_DTYPE)
    for k, p in enumerate(render.arrow_polys(x0, y0, x1, y1)):
        pieces[k]["n"], pieces[k]["abc"] = len(p), render.convex_piece(p)
    cov = np.logical_or.reduce([R.piece_coverage(q, H, W) for q in pieces])
    yy, xx = np.mgrid[0:H, 0:W] + 0.5
    fa = patches.FancyArrow(x0, y0, x1 - x0, y1 - y0, width=10 / 3, head_width=50 / 3, length_includes_head=True, overhang=0.5)
    inside = Path(fa.get_xy()).contains_points(np.stack([xx.ravel(), yy.ravel()], 1)).reshape(H, W)
    edge = np.zeros((H, W), bool)  # (pixel centres within 1e-3 of the outline may fall either way)
    v = fa.get_xy()
    for a, b in zip(v, np.roll(v, -1, 0)):
        ab = b - a
        if not ab.any():
            continue
        tt = np.clip(((xx - a[0]) * ab[0] + (yy - a[1]) * ab[1]) / (ab @ ab), 0, 1)
        edge |= np.hypot(xx - (a[0] + tt * ab[0]), yy - (a[1] + tt * ab[1])) < 1e-3
    assert np.array_equal(cov[~edge], inside[~edge]) and inside.sum() > 150


def test_arrow_head_is_clamped_to_a_short_arrow():
    """A head longer than the arrow is scaled (length and width) by length / head_length: the barbs sit at the tail."""
    from articulation3d_amd import render

    polys = render.arrow_polys(10.0, 12.0, 20.0, 12.0)  # 10 px long, head_length 25
    shaft, left, right, core = polys
    assert np.allclose(left, [[20, 12], [10, 12 - 50 / 3 * 10 / 25 / 2], [15, 12 - 10 / 6]])
    assert np.allclose(right, [[20, 12], [10, 12 + 50 / 3 * 10 / 25 / 2], [15, 12 + 10 / 6]])
    assert np.allclose(shaft[:, 0], [10, 15, 15, 10]) and np.allclose(core[:, 0], [20, 15, 15])
    assert min(p[:, 0].min() for p in polys) >= 10 - 1e-9


def test_every_cull_box_contains_its_layers_coverage():
    from articulation3d_amd import render

    rng = np.random.default_rng(5)
    preds = [R.make_instances(rng, H, W, 4), R.make_instances(rng, H, W, 3)]
    # boxes that stick out of the image and a huge one
    preds.append(_inst([[-6.0, -3.0, 12.0, 9.0], [30.0, 15.0, 47.0, 29.0], [-100.0, -100.0, 200.0, 200.0]], [0, 1, 0], [0.9, 0.9, 0.9]))
    t = render.build_layers(preds, H, W, mask_alpha=0.5)
    bits = R.pack_bits(np.concatenate([p.pred_masks.numpy() for p in preds]))
    assert t.layer_off.tolist() == [0, 12, 21, 30]  # (mask, arrow, box) per instance: no axis here is degenerate
    for layer in t.layers:
        cov = R.layer_coverage(layer, t.pieces, bits, H, W)
        box = np.zeros((H, W), bool)
        box[int(layer["y0"]):int(layer["y1"]), int(layer["x0"]):int(layer["x1"])] = True
        assert not (cov & ~box).any()
        assert 0 <= layer["x0"] <= layer["x1"] <= W and 0 <= layer["y0"] <= layer["y1"] <= H
    for piece in t.pieces:  # every piece carries a box of its own, inside its layer's
        box = np.zeros((H, W), bool)
        box[int(piece["y0"]):int(piece["y1"]), int(piece["x0"]):int(piece["x1"])] = True
        assert not (R.piece_coverage(piece, H, W) & ~box).any()
    for layer in t.layers[t.layers["kind"] == 1]:
        ps = t.pieces[int(layer["p0"]):int(layer["p1"])]
        assert layer["x0"] <= ps["x0"].min() and ps["x1"].max() <= layer["x1"] and layer["y0"] <= ps["y0"].min() and ps["y1"].max() <= layer["y1"]


def test_half_planes_are_fp32_oriented_inwards():
    from articulation3d_amd import render

    for verts in ([[1, 1], [9, 2], [8, 7], [2, 8]], [[2, 8], [8, 7], [9, 2], [1, 1]], [[0, 0], [4, 0], [0, 4]]):
        hp = render.convex_piece(verts)
        assert hp.dtype == np.float32 and hp.shape == (4, 3)
        c = np.mean(np.asarray(verts, np.float64), 0)
        assert all(hp[i, 0] * c[0] + hp[i, 1] * c[1] + hp[i, 2] > 0 for i in range(len(verts)))
        assert not hp[len(verts):].any()
    assert render.convex_piece([[0, 0], [1, 1], [2, 2]]) is None


def _three_masks():
    m = np.zeros((3, H, W), np.float32)
    m[0, 2:14, 3:20] = 1
    m[1, 8:20, 12:30] = 1
    m[2, 4:22, 28:38] = 1
    return m


NORMAL_SEED = 5  # chosen so that every v of the case lies in [0, 256) (asserted below): sums of two unit normals can leave it


def test_render_ref_normal_panel_is_the_references_get_normal_map():
    """arti_vis.py:197-215 written out: mask > 0.5, F.normalize(plane), matmul, (n + 1) / 2 * 255, astype(uint8)."""
    masks = _three_masks()
    assert (masks.sum(0) <= 2).all() and (masks.sum(0) == 2).any()
    plane = torch.from_numpy(np.random.default_rng(NORMAL_SEED).normal(size=(3, 3)).astype(np.float32))
    normals = torch.nn.functional.normalize(plane, p=2)
    bits = R.pack_bits(masks)
    v = R.normal_value([0, 1, 2], normals.numpy(), bits, H, W)
    assert (v >= 0).all() and (v < 256).all()  # the range in which the reference's cast is defined
    mask = (torch.from_numpy(masks) > 0.5).float()
    normal_map = torch.matmul(mask.permute(1, 2, 0), normals)
    want = ((normal_map.numpy() + 1.0) / 2.0 * 255.0).astype(np.uint8)
    got = R.normal_panel([0, 1, 2], normals.numpy(), bits, H, W)
    assert np.array_equal(got, want) and len(np.unique(got.reshape(-1, 3), axis=0)) >= 6


def test_render_ref_wrap_and_blend_laws():
    # three unit normals over one pixel: n = 3 -> v = 510 -> 510 & 255 = 254; n = -3 -> v = -255 -> int32 -255 & 255 = 1
    bits = R.pack_bits(np.ones((3, 1, 2), np.uint8))
    nrm = np.array([[1, -1, 0.5]] * 3, np.float32)
    assert R.normal_panel([0, 1, 2], nrm, bits, 1, 2)[0, 0].tolist() == [254, 1, (int(np.float32(2.5) / np.float32(2) * np.float32(255))) & 255]
    # blend: alpha 0 keeps, 256 replaces, 128 is the rounded mean; a pixel under two pieces of one layer is blended once
    frame = np.full((2, 2, 3), 100, np.uint8)
    piece = np.zeros(2, dtype=[("n", "i4"), ("abc", "f4", (4, 3))])
    piece["n"] = 1
    piece["abc"][:, 0] = (0, 0, 1)  # e = 1 everywhere
    layer = np.zeros(1, dtype=[("kind", "i4"), ("alpha", "i4"), ("color", "u1", 4), ("p0", "i4"), ("p1", "i4")])
    layer["kind"], layer["color"], layer["p1"] = R.POLY, (201, 0, 255, 0), 2
    for a, want in ((0, [100, 100, 100]), (256, [201, 0, 255]), (128, [(100 * 128 + 201 * 128 + 128) >> 8, 50, (100 * 128 + 255 * 128 + 128) >> 8])):
        layer["alpha"] = a
        assert R.seg_panel(frame, layer, piece, None)[1, 1].tolist() == want
    # words straddling rows: bit i of word w is pixel 32w + i
    m = np.zeros((1, 7, 37), np.uint8)
    m[0, 1, 0] = m[0, 6, 36] = 1
    b = R.pack_bits(m)
    assert b.shape == (1, 9) and b[0, 1] == 1 << 5 and b[0, 8] == 1 << 2 and np.array_equal(R.mask_of(b, 0, 7, 37), m[0].astype(bool))


def test_snapshot_keeps_the_raw_translation_axis_the_optimiser_overwrites():
    """tools/inference.py keeps the raw predictions for the raw panels: the optimiser's re-weighting writes a translation track's
    consensus axis into pred_tran_axis IN PLACE (and scales scores), so the snapshot must own its small fields."""
    import importlib.util
    import os

    from articulation3d_amd.utils import opt_utils

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("a3d_inference_tool", os.path.join(root, "tools", "inference.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    tran = [[0.6, 0.8], [1.0, 0.0]]
    preds = [_inst([[4, 2, 34, 22], [10, 5, 30, 17]], [1, 1], [0.9, 0.8], tran=tran) for _ in range(2)]
    snap = tool.snapshot_predictions(preds)
    track = {"ids": {0: 0, 1: 0}, "has_rot": True, "std_axis": torch.tensor([0.0, -1.0])}
    opt = opt_utils._reweight(preds, [track], "trans")
    assert opt[0].pred_tran_axis[0].tolist() == [0.0, -1.0] and preds[0].pred_tran_axis[0].tolist() == [0.0, -1.0]  # written in place
    assert opt[0].scores.tolist() == pytest.approx([0.9, 0.8 * 0.6])  # the untracked detection is down-weighted
    for s_, p in zip(snap, preds):
        assert torch.equal(s_.pred_tran_axis, torch.tensor(tran)) and s_.scores.tolist() == pytest.approx([0.9, 0.8])
        assert s_.pred_boxes is p.pred_boxes and s_.pred_masks is p.pred_masks  # never written: shared
        assert s_.pred_tran_axis.data_ptr() != p.pred_tran_axis.data_ptr()
