"""CPU suite, part 1: the oracle against the golden vectors produced by the REFERENCE's own modules
(oracle/make_golden.py) and against slow literal restatements of the third-party operators."""
import os

import numpy as np
import pytest
import torch
from hypothesis import given, settings, strategies as st

from oracle import golden_inputs as G


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def test_paste_masks_matches_reference(oracle, golden_dir):
    g = _load(golden_dir, "paste_masks.npz")
    masks, boxes, hw = G.paste_case()
    assert abs(float(masks.double().sum()) - float(g["masks_sum"])) < 1e-9, "seeded inputs drifted"
    out = oracle.paste_masks(masks, boxes, hw[0], hw[1], 0.5)
    ref = np.unpackbits(g["packed"])[: int(np.prod(g["shape"]))].reshape(g["shape"]).astype(bool)
    assert out.shape == tuple(g["shape"])
    assert (out.numpy() != ref).sum() == 0  # bit-exact bool masks


def test_plane_head_matches_reference(oracle, golden_dir):
    g = _load(golden_dir, "plane_head.npz")
    x = G.head_input()
    assert abs(float(x.double().sum()) - float(g["x_sum"])) < 1e-6
    with torch.no_grad():
        out = oracle.plane_head(x, G.head_params("plane"))
    np.testing.assert_allclose(out.numpy(), g["pred_plane"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(np.linalg.norm(out.numpy(), axis=1), 1.0, atol=1e-6)


def test_axis_head_matches_reference(oracle, golden_dir):
    """In float64 the oracle gives the reference module's float64 outputs (the fixture's *_f64) to 1e-10; in fp32 it is no further from
    them than a small factor of the reference's own fp32 result.  (One ROI's translation axis nearly cancels: the reference's fp32 value
    is 1.1e-5 from exact there, so fp32 against fp32 within 1e-6 holds only on a CPU whose kernels sum in the fixture's order.)"""
    g = _load(golden_dir, "axis_head.npz")
    x, P = G.head_input(), G.head_params("axis")
    with torch.no_grad():
        rot, tran = oracle.axis_head(x, P)
        rot64, tran64 = oracle.axis_head(x.double(), {k: v.double() if v.is_floating_point() else v for k, v in P.items()})
    np.testing.assert_allclose(rot.numpy(), g["pred_rot_axis"], rtol=1e-5, atol=1e-6)
    for key, got, got64 in (("pred_rot_axis", rot, rot64), ("pred_tran_axis", tran, tran64)):
        truth = g[key + "_f64"]
        np.testing.assert_allclose(got64.numpy(), truth, rtol=1e-10, atol=1e-12)
        err, ref_err = float(np.abs(got.numpy() - truth).max()), float(np.abs(g[key] - truth).max())
        assert err < 8 * ref_err + 2e-6, (key, err, ref_err)


def test_depth_head_matches_reference(oracle, golden_dir):
    g = _load(golden_dir, "depth_head.npz")
    with torch.no_grad():
        d = oracle.depth_head(G.depth_features(), G.head_params("depth"))
    assert tuple(d.shape) == tuple(g["shape"])
    np.testing.assert_allclose(d[:, ::16, ::16].numpy(), g["depth_strided"], rtol=1e-4, atol=1e-5)
    assert abs(float(d.double().sum()) - float(g["depth_sum"])) < 1e-4 * float(g["depth_abs_sum"])


# ---- third-party operators (parity unpinned): C kernels vs literal python statements of Appendix A ----
def _rand_boxes(rng, n, w=160.0, h=120.0):
    x1 = rng.uniform(-5, w, n)
    y1 = rng.uniform(-5, h, n)
    bw = rng.uniform(0.5, 80, n)
    bh = rng.uniform(0.5, 60, n)
    return torch.tensor(np.stack([x1, y1, x1 + bw, y1 + bh], 1), dtype=torch.float32)


@pytest.mark.parametrize("P,ratio,aligned", [(7, 0, True), (14, 2, False), (14, 0, False)])
def test_roi_align_c_vs_python(oracle, P, ratio, aligned):
    rng = np.random.default_rng(P + ratio)
    feat = torch.randn(2, 3, 30, 40)
    boxes = _rand_boxes(rng, 6) * 0.25
    rois = torch.cat([torch.tensor([[0.], [1.], [0.], [1.], [0.], [1.]]), boxes * 4], 1)
    a = oracle.roi_align(feat, rois, P, 0.25, ratio, aligned)
    b = oracle.roi_align_py(feat, rois, P, 0.25, ratio, aligned)
    np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-5, atol=1e-6)


def test_roi_align_constant_and_ramp(oracle):
    # constant map -> constant; linear ramp in x -> bin centre value (sampling is symmetric about the centre)
    feat = torch.full((1, 1, 32, 32), 3.25)
    rois = torch.tensor([[0, 4.0, 4.0, 100.0, 90.0]])
    out = oracle.roi_align(feat, rois, 7, 0.25, 0, True)
    assert torch.allclose(out, torch.full_like(out, 3.25))
    ramp = torch.arange(32, dtype=torch.float32).view(1, 1, 1, 32).expand(1, 1, 32, 32).contiguous()
    out = oracle.roi_align(ramp, rois, 7, 0.25, 2, True)
    x1, x2 = 4.0 * 0.25 - 0.5, 100.0 * 0.25 - 0.5
    centres = x1 + (torch.arange(7) + 0.5) * (x2 - x1) / 7
    np.testing.assert_allclose(out[0, 0, 0].numpy(), centres.numpy(), rtol=1e-5)


@settings(max_examples=25, deadline=None)
@given(st.integers(0, 10_000), st.integers(1, 60))
def test_nms_c_vs_python_and_properties(seed, n):
    from oracle import planercnn_oracle as O

    rng = np.random.default_rng(seed)
    boxes = _rand_boxes(rng, n)
    if n > 3:  # exact duplicates and ties
        boxes[1] = boxes[0]
    cats = torch.tensor(rng.integers(0, 2, n))
    keep_c = O.nms_sorted(boxes, cats, 0.5)
    keep_py = O.nms_sorted_py(boxes, cats, 0.5)
    assert torch.equal(keep_c, keep_py)
    assert keep_c[0]  # the top-scoring box always survives
    # idempotence: NMS of the kept set keeps everything
    again = O.nms_sorted(boxes[keep_c], cats[keep_c], 0.5)
    assert bool(again.all())


def test_topk_stable_ties(oracle):
    s = torch.tensor([[0.5, 0.9, 0.5, 0.9, 0.1]])
    v, i = oracle.topk_stable(s, 3)
    assert i.tolist() == [[1, 3, 0]] and torch.equal(v, torch.tensor([[0.9, 0.9, 0.5]]))


def test_batched_nms_categories_do_not_interact(oracle):
    b = torch.tensor([[0., 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 10]])
    keep = oracle.batched_nms(b, torch.tensor([0.9, 0.8, 0.7]), torch.tensor([0, 1, 0]), 0.5)
    assert keep.tolist() == [0, 1]


def test_override_depth_empty_mask_and_axis_swap(oracle):
    depth = torch.full((480, 640), 2.0)
    rays = oracle.k_inv_dot_xy1()
    masks = torch.zeros(2, 480, 640, dtype=torch.bool)
    masks[1, 200:280, 300:340] = True
    planes = torch.tensor([[0.0, 0.6, 0.8], [0.0, 0.0, 1.0]])
    out = oracle.override_depth(depth, masks, planes, rays)
    # empty mask keeps the plane (swap forth and back = identity)
    np.testing.assert_allclose(out[0].numpy(), planes[0].numpy(), atol=1e-7)
    # normal (0,0,1) -> swapped (0,-1,0): offset = mean(-Y) over the mask; rows 200..279 are above the principal point
    ys = (np.arange(200, 280) - 239.5) / 571.623718 * 2.0
    off = -ys.mean()
    np.testing.assert_allclose(out[1].numpy(), [0.0, 0.0, off], rtol=1e-5, atol=1e-6)


def test_detect_runs_and_filters(oracle, oracle_params):
    frames = oracle.synthetic_frames(1)
    outs = oracle.detect(oracle.frames_to_chw(frames), oracle_params, oracle.OracleCfg(score_thresh=0.7))
    assert len(outs[0]["scores"]) == 0 and outs[0]["pred_masks"].shape == (0, 480, 640)
    assert outs[0]["depth"].shape == (480, 640)


# ---- torchvision's two batched_nms formulations (oracle switch OracleCfg.nms_strategy) ----
def test_batched_nms_strategies_agree_away_from_the_threshold(oracle):
    """torchvision >= 0.9 shifts every category by idx * (max + 1) and runs one NMS ("offset") while a call holds few boxes, and loops
    over the categories ("plain", the parity definition) above that.  The two differ only where an IoU lies within fp32 rounding of
    the threshold: on random boxes whose decisions all have a margin above 1e-5 the kept sets are identical, for every strategy."""
    from oracle import matching as M

    rng = np.random.default_rng(11)
    checked = 0
    for trial in range(40):
        n = int(rng.integers(5, 400))
        boxes = _rand_boxes(rng, n, 640.0, 480.0)
        scores = torch.tensor(rng.uniform(0, 1, n), dtype=torch.float32)
        cats = torch.tensor(rng.integers(0, 5, n), dtype=torch.int64)
        thr = float(rng.choice([0.5, 0.7]))
        order = torch.sort(scores, descending=True, stable=True)[1]
        keep_mask = oracle.nms_sorted(boxes[order], cats[order], thr)
        if M.nms_margin(boxes[order], cats[order], keep_mask, thr) < 1e-5:
            continue
        checked += 1
        base = oracle.batched_nms(boxes, scores, cats, thr, "plain")
        for s in ("offset", "tv-gpu", "tv-cpu"):
            assert torch.equal(oracle.batched_nms(boxes, scores, cats, thr, s), base), (trial, s)
    assert checked >= 30


def test_batched_nms_size_rule_and_offset_form(oracle):
    """The size rule ([tv-spec] boxes.numel() > 4000 on the CPU / > 20000 on a GPU -> per-category loop) and the offset form itself:
    boxes of different categories never suppress each other although the single NMS sees them all."""
    b = torch.tensor([[10.0, 10, 110, 110], [12, 12, 112, 112], [10, 10, 110, 110]])
    s = torch.tensor([0.9, 0.8, 0.7])
    c = torch.tensor([0, 0, 1])
    for strat in ("plain", "offset", "tv-gpu", "tv-cpu"):
        assert oracle.batched_nms(b, s, c, 0.5, strat).tolist() == [0, 2]
    # 1001 boxes: "tv-cpu" takes the loop (4004 > 4000), "tv-gpu" the trick; far from any threshold they agree
    rng = np.random.default_rng(3)
    boxes = _rand_boxes(rng, 1001, 640.0, 480.0)
    scores = torch.tensor(rng.uniform(0, 1, 1001), dtype=torch.float32)
    cats = torch.tensor(rng.integers(0, 2, 1001), dtype=torch.int64)
    k0 = oracle.batched_nms(boxes, scores, cats, 0.5, "plain")
    assert torch.equal(oracle.batched_nms(boxes, scores, cats, 0.5, "tv-cpu"), k0)


def test_committed_frames_do_not_depend_on_the_nms_formulation(oracle, oracle_params, golden_dir):
    """oracle/nms_strategy_report.py evaluates every committed frame (end-to-end seeds, stage frames, smoke frame) under the four
    strategies; the committed report says none differs.  Re-checked here on one frame (the full run takes a minute)."""
    import json

    from oracle import nms_strategy_report as R

    doc = json.load(open(os.path.join(golden_dir, "nms_strategy_report.json")))
    seeds = {f["seed"] for f in json.load(open(os.path.join(golden_dir, "e2e_frames.json")))["frames"]} | {2020, 3000}
    assert {f["seed"] for f in doc["frames"]} == seeds
    assert doc["differing"] == [], doc["summary"]
    with torch.no_grad():
        r = R.frame_report(3000, oracle_params, thresholds=(0.0,))
    for k, v in r.items():
        if isinstance(v, dict):
            assert v["proposals_identical"] and v["detections_identical"], (k, v)


# ---- round 5: the temporal optimiser's helpers, pinned against the reference's own functions (SURVEY 8c fixture 4) ----------------
def test_axis_transforms_match_the_reference(golden_dir):
    """oracle/opt_oracle.py's restatements of axis_to_angle_offset / angle_offset_to_axis / get_boundary_point against the outputs of
    the reference's functions (planercnn_transforms.py:31-68,101-176; oracle/make_golden.py section 5): both directions, the boundary
    cases of get_boundary_point (vertical, horizontal = angle -0.0, corners, lines that miss the image -> [0,0,1,1]), and the round
    trip the optimiser performs on a predicted axis."""
    from oracle import opt_oracle as O

    g = _load(golden_dir, "axis_transforms.npz")
    axes, centers, ao, ao_c, bp = G.axis_cases()
    assert np.array_equal(axes, g["axes"]) and np.array_equal(ao, g["ao"]), "seeded inputs drifted"
    fwd = O.axis_to_angle_offset(axes, centers)
    ref = g["angle_offset"]
    ok = np.isfinite(ref).all(1)  # (an axis through its box centre has C = 0: sign(C) = 0 -> sin = cos = 0 in both; none is NaN)
    assert ok.all()
    np.testing.assert_allclose(fwd, ref, rtol=2e-6, atol=2e-7)
    back = O.angle_offset_to_axis(ao, ao_c)
    assert np.array_equal(back, g["axis_back"]), np.nonzero((back != g["axis_back"]).any(1))
    rt = O.angle_offset_to_axis(ref[:, :3], centers)
    assert np.array_equal(rt, g["axis_round_trip"])
    for (y, x, ang), want in zip(g["boundary_in"], g["boundary_out"]):
        p1, p2 = O.get_boundary_point(np.float64(y), np.float64(x), np.float64(ang), 480, 640)
        got = [-1] * 4 if p1 is None else [p1[0], p1[1], p2[0], p2[1]]
        assert [float(v) for v in got] == [float(v) for v in want], ((y, x, ang), got, want)


def test_point_cloud_lift_and_projection_match_the_reference(golden_dir):
    """get_pcd in float64 and project2D (vis.py:62-102) against the reference's own outputs: the lift to 1e-12 (the oracle writes K^-1 q
    out instead of calling np.linalg.inv: the same numbers to float64 rounding), the fp32 projection the oracle fixes the evaluation
    order of to fp32 rounding of the reference's float64 product, and the truncated pixel index equal wherever the exact value is not
    within that rounding of a pixel edge."""
    from oracle import opt_oracle as O

    g = _load(golden_dir, "pcd_project.npz")
    verts, planes = G.pcd_cases()
    assert np.array_equal(verts, g["verts"])
    for i, (normal, offset) in enumerate(planes):
        pcd = O.get_pcd(verts, normal, offset)
        np.testing.assert_allclose(pcd, g["pcd"][i], rtol=1e-12, atol=1e-12)
        uv = O.project2d(pcd.astype(np.float32))
        ref = g["proj_from_f32"][i]
        np.testing.assert_allclose(uv, ref, rtol=0, atol=640 * 2.0 ** -22)
        # the lift followed by the projection is the identity on pixel coordinates (every point lands ON a pixel edge: the truncation
        # is decided by the last bit, which is why the oracle fixes the fp32 evaluation order): to fp32 rounding here
        np.testing.assert_allclose(g["proj"][i], verts.astype(np.float64), rtol=0, atol=1e-9)
        far = np.abs(ref - np.round(ref)) > 1e-3
        assert np.array_equal(uv.astype(np.int64)[far], ref.astype(np.int64)[far])


def test_host_side_axis_helpers_match_the_reference(golden_dir):
    """The product's own host-side mirror of the two transforms (articulation3d_amd/utils/opt_utils.py: the optimiser stays on the host,
    north star) against the same reference outputs -- the mirror the reference's callers would switch to."""
    import torch as _t

    from articulation3d_amd.utils import opt_utils as PU

    g = _load(golden_dir, "axis_transforms.npz")
    axes, centers, ao, ao_c, _ = G.axis_cases()
    fwd = PU.axis_to_angle_offset([list(map(float, a)) for a in axes], _t.from_numpy(centers)).numpy()
    np.testing.assert_allclose(fwd, g["angle_offset"], rtol=2e-6, atol=2e-7)
    assert np.array_equal(PU.angle_offset_to_axis(_t.from_numpy(ao), _t.from_numpy(ao_c)).numpy(), g["axis_back"])
    assert np.array_equal(PU.angle_offset_to_axis(_t.from_numpy(g["angle_offset"][:, :3]), _t.from_numpy(centers)).numpy(), g["axis_round_trip"])
