"""CPU checks of tests/roi_ref64.py, the float64 reference tests/test_gpu_roi_geometry.py holds the ROI poolers to.

(a) the reference agrees with the oracle's fp32 C statement of ROIAlign (pinned to detectron2's known answers by
    tests/test_known_answers.py) within the law -- the fp32 C result stands in for a correct kernel;
(b) its adjoint agrees with the oracle's C backward (reached through autograd) within the backward law;
(c) the law has teeth: each deliberately wrong variant of the reference FAILS it on the committed case list, and the note next to each
    variant says whether today's whole-tensor metric (max|a-b| / max|b| < 1e-5 on the 87 boxes of test_roi_align_fpn_vs_oracle) sees it;
(d) the walk predictor puts the committed boxes into the classes they were built for, and every class holds its stated minimum."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roi_ref64 as R  # noqa: E402

NAMES = ("p2", "p3", "p4", "p5")
C_HOST = 8


def _oracle_pool(oracle, feats, boxes, img, B, P, ratio, aligned):
    """oracle.roi_pool_fpn on NHWC numpy levels -> [N, P, P, C] fp32 in the order of `boxes`."""
    tf = {n: torch.from_numpy(np.ascontiguousarray(f.transpose(0, 3, 1, 2))) for n, f in zip(NAMES, feats)}
    lists = [torch.from_numpy(boxes[img == b]) for b in range(B)]
    out = oracle.roi_pool_fpn(tf, lists, P, ratio, aligned)
    order = np.concatenate([np.nonzero(img == b)[0] for b in range(B)])
    res = np.empty((len(boxes), P, P, feats[0].shape[3]), dtype=np.float32)
    res[order] = out.permute(0, 2, 3, 1).numpy()
    return res


def _case_boxes(frame, pooler):
    cases = R.frame_cases(R.FRAMES[frame])
    if frame == "480x640":
        cases = cases + [(f"walk:{w}:{r}", b) for w, r, b in R.box_walk_cases()] + [(f"exact:{n}", b) for n, b, _ in R.exact_edge_cases(R.POOLERS[pooler][2])]
    boxes = np.array([b for _, b in cases], dtype=np.float32)
    img = (np.arange(len(boxes)) % 2).astype(np.int64)
    return [n for n, _ in cases], boxes, img


def _general_bound(geoms, A):
    terms = np.stack([R.forward_terms(g, "general") for g in geoms])  # the oracle sums per sample, as torchvision does
    return R.gamma(terms)[..., None] * A


@pytest.mark.parametrize("frame", list(R.FRAMES))
@pytest.mark.parametrize("pooler", list(R.POOLERS))
def test_reference_agrees_with_the_oracle_within_the_law(oracle, frame, pooler):
    P, ratio, aligned = R.POOLERS[pooler]
    _, boxes, img = _case_boxes(frame, pooler)
    feats = R.make_pyramid(R.FRAMES[frame], 2, C_HOST, seed=11)
    y64, A, geoms = R.pool_ref([f.astype(np.float64) for f in feats], R.SCALES, boxes, img, P, ratio, aligned)
    got = _oracle_pool(oracle, feats, boxes, img, 2, P, ratio, aligned)
    assert np.array_equal(np.array([g.lv for g in geoms]), oracle.assign_levels(torch.from_numpy(boxes)).numpy())
    ratio_ = R.law_ratio(got, y64, _general_bound(geoms, A))
    print(f"reference vs oracle {pooler} {frame}: worst err / bound = {ratio_:.3f}")
    assert ratio_ <= 1.0


@pytest.mark.parametrize("name", ["single_level", "wide_bin"])
def test_reference_agrees_with_the_oracle_on_single_level_calls(oracle, name):
    cases, hw, ratio = (R.single_level_cases(), (128, 128), 0) if name == "single_level" else (R.wide_bin_cases(), (512, 512), 2)
    boxes = np.array([b for _, b in cases], dtype=np.float32)
    rng = np.random.default_rng(5)
    feat = rng.standard_normal((1, hw[0], hw[1], 4)).astype(np.float32)
    y64, A, geoms = R.pool_ref([feat.astype(np.float64)], [1.0], boxes, np.zeros(len(boxes), dtype=np.int64), 7, ratio, True)
    rois = torch.cat((torch.zeros(len(boxes), 1), torch.from_numpy(boxes)), 1)
    got = oracle.roi_align(torch.from_numpy(np.ascontiguousarray(feat.transpose(0, 3, 1, 2))), rois, 7, 1.0, ratio, True)
    r = R.law_ratio(got.permute(0, 2, 3, 1).numpy(), y64, _general_bound(geoms, A))
    print(f"reference vs oracle {name}: worst err / bound = {r:.3f}")
    assert r <= 1.0
    walks = {n: R.walk_class(g)[0] for (n, _), g in zip(cases, geoms)}
    if name == "single_level":
        assert [g.gh for g in geoms[:2]] == [15, 15] and [g.gw for g in geoms[:2]] == [15, 15]
        assert geoms[1].y.n.max() == R.KMAX and geoms[1].x.n.max() == R.KMAX  # the longest table row there is: all KMAX entries
        for (n, _), g in zip(cases, geoms):
            assert (R.walk_class(g)[0] == "general") == (n == "lattice16") == (max(g.gh, g.gw) >= 16), n
    else:
        assert walks == {"wide20": "cells>NC", "wide31": "general", "wide68": "general", "wide31x2": "general"}
        assert [round(float(g.bw)) for g in geoms] == [20, 31, 68, 31]


def test_adjoint_agrees_with_the_oracle_backward_within_the_law(oracle):
    from oracle import train_oracle as TO

    P, ratio, aligned = R.POOLERS["box"]
    _, boxes, img = _case_boxes("480x640", "box")
    feats = R.make_pyramid((480, 640), 2, 4, seed=12)
    rng = np.random.default_rng(13)
    dout = rng.standard_normal((len(boxes), P, P, 4)).astype(np.float32)
    tf = {n: torch.from_numpy(np.ascontiguousarray(f.transpose(0, 3, 1, 2))).requires_grad_(True) for n, f in zip(NAMES, feats)}
    order = np.concatenate([np.nonzero(img == b)[0] for b in range(2)])
    pooled = TO.roi_pool_fpn_diff(tf, [torch.from_numpy(boxes[img == b]) for b in range(2)], P, ratio, aligned)
    pooled.backward(torch.from_numpy(np.ascontiguousarray(dout[order].transpose(0, 3, 1, 2))))
    d64, Aabs, terms, _ = R.pool_bwd_ref([f.shape[1:3] for f in feats], R.SCALES, boxes, img, dout.astype(np.float64), 2, P, ratio, aligned)
    for l, n in enumerate(NAMES):
        got = tf[n].grad.permute(0, 2, 3, 1).numpy()
        r = R.law_ratio(got, d64[l], R.gamma(terms[l])[..., None] * Aabs[l])
        print(f"adjoint vs oracle backward {n}: worst err / bound = {r:.3f}")
        assert r <= 1.0
        assert np.abs(d64[l]).max() > 0


# Whether today's whole-tensor metric on today's 87 boxes sees the variant in at least one of the three poolers (measured by this test
# and kept as an assertion, so that the note stays true).  shift_sample: 1e-4 cell on one sample moves its bins by ~1e-4 / g of a cell
# difference, a few 1e-5 of the tensor's maximum: seen, just.  skip_L: no random box puts a sample exactly on v == L: NOT seen.
# count_nomax: the old test's zero-area box divides 0 by 0 in the aligned pooler (a not-aligned box is at least one cell wide): seen
# there only.  table_g and clamp_off_by_one lose whole cells: seen.
SEEN_TODAY = {"shift_sample": True, "skip_L": False, "count_nomax": True, "table_g": True, "clamp_off_by_one": True}


def _todays_boxes(P):
    """The boxes of tests/test_gpu_parity.py::test_roi_align_fpn_vs_oracle."""
    rng = np.random.default_rng(P)
    lists = []
    for b in range(2):
        n = 40 + 7 * b
        side = np.exp(rng.uniform(np.log(4), np.log(600), n))
        ar = np.exp(rng.uniform(-1, 1, n))
        w_, h_ = side * np.sqrt(ar), side / np.sqrt(ar)
        cx, cy = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
        bx = np.stack([cx - w_ / 2, cy - h_ / 2, cx + w_ / 2, cy + h_ / 2], 1)
        bx[0] = [10, 10, 10, 10]
        bx[1] = [-50, -40, 700, 500]
        lists.append(bx.astype(np.float32))
    return np.concatenate(lists), np.concatenate([np.full(len(l), b) for b, l in enumerate(lists)])


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_the_law_has_teeth(variant):
    """A reference that is wrong in one of the ways a pooler kernel goes wrong must fail the law on the committed case list."""
    worst, seen_any = {}, False
    for pooler, (P, ratio, aligned) in R.POOLERS.items():
        _, boxes, img = _case_boxes("480x640", pooler)
        feats = [f.astype(np.float64) for f in R.make_pyramid((480, 640), 2, C_HOST, seed=11)]
        y64, A, geoms = R.pool_ref(feats, R.SCALES, boxes, img, P, ratio, aligned)
        bad, _, _ = R.pool_ref(feats, R.SCALES, boxes, img, P, ratio, aligned, variant=variant)
        terms = np.stack([R.forward_terms(g, R.walk_class(g)[0]) for g in geoms])
        worst[pooler] = R.law_ratio(bad, y64, R.gamma(terms)[..., None] * A)
        # today's metric on today's boxes (plain N(0, 1) pyramid, as that test draws it)
        rng = np.random.default_rng(6)
        plain = [rng.standard_normal((2, h, w, C_HOST)) for h, w in R.pyramid_sizes((480, 640))]
        tb, ti = _todays_boxes(P)
        ref, _, _ = R.pool_ref(plain, R.SCALES, tb, ti, P, ratio, aligned)
        bad_t, _, _ = R.pool_ref(plain, R.SCALES, tb, ti, P, ratio, aligned, variant=variant)
        with np.errstate(invalid="ignore"):
            rel = np.abs(bad_t - ref).max() / np.abs(ref).max()
        seen = not (rel < 1e-5)
        print(f"{variant} {pooler}: law ratio on the case list {worst[pooler]:.3g}; today's metric on today's boxes {rel:.3g} ({'seen' if seen else 'NOT seen'})")
        seen_any = seen_any or seen
    assert seen_any == SEEN_TODAY[variant]
    # count_nomax shows only where a lattice is empty: the aligned pooler's zero-area boxes
    must_fail = ("box",) if variant == "count_nomax" else tuple(R.POOLERS)
    for pooler in must_fail:
        assert worst[pooler] > 1.0, (variant, pooler, worst)


# minimum number of boxes per geometry class in a frame's case list (frame_cases)
MIN_PER_CLASS = {"interior": 3, "edge_left": 2, "edge_right": 2, "edge_top": 2, "edge_bottom": 2, "corner_tl": 2, "corner_tr": 2,
                 "corner_bl": 2, "corner_br": 2, "cover": 1, "outside_left": 1, "outside_right": 1, "outside_top": 1, "outside_bottom": 1,
                 "zero_area": 3, "sub_cell": 2, "aspect": 4}


@pytest.mark.parametrize("frame", list(R.FRAMES))
def test_every_geometry_class_is_populated_and_is_what_its_name_says(frame):
    hw = R.FRAMES[frame]
    cases = R.frame_cases(hw)
    sizes = R.pyramid_sizes(hw)
    names = [n for n, _ in cases]
    for cls, k in MIN_PER_CLASS.items():
        assert names.count(cls) >= k, (cls, names.count(cls))
    levels = set()
    for pooler, (P, ratio, aligned) in R.POOLERS.items():
        for name, box in cases:
            g = R.roi_geometry(box, sizes, R.SCALES, P, ratio, aligned)
            live_y, live_x = ~g.y.skip, ~g.x.skip
            if name.startswith("outside"):
                assert not (live_y.any() and live_x.any()), (name, pooler)  # every sample skipped: exact zeros
            if name == "interior":
                levels.add(g.lv)
                assert R.is_interior(g), (box, pooler)
            if name.startswith(("edge", "corner", "cover")):
                lowx, highx = (g.x.v <= 0).any(), (g.x.v >= g.W - 1).any()
                lowy, highy = (g.y.v <= 0).any(), (g.y.v >= g.H - 1).any()
                want = {"edge_left": lowx, "edge_right": highx, "edge_top": lowy, "edge_bottom": highy, "corner_tl": lowx and lowy,
                        "corner_tr": highx and lowy, "corner_bl": lowx and highy, "corner_br": highx and highy,
                        "cover": lowx and highx and lowy and highy}[name]
                assert want, (name, pooler)
            if name == "aspect":
                a = max(float(g.rw / g.rh), float(g.rh / g.rw))
                assert a >= 7.0  # (in cells, after the one-cell floor of the not-aligned poolers)
        if frame == "480x640":
            assert levels == {0, 1, 2, 3}
    b = np.array([bx for n, bx in cases if n == "aspect"])
    ar = (b[:, 2] - b[:, 0]) / (b[:, 3] - b[:, 1])
    assert ar.max() >= 79.9 and ar.min() <= 1 / 79.9


def test_walk_predictor_on_the_committed_walk_cases():
    sizes = R.pyramid_sizes((480, 640))
    for walk, reason, box in R.box_walk_cases():
        g = R.roi_geometry(box, sizes, R.SCALES, 7, 0, True)
        w, why = R.walk_class(g)
        if reason == "exactly_9":
            assert R.walk_class(g, rolling=False)[0] == "cells<=NC" and g.cells.max() == 9, (box, g.cells.max())
        elif reason == "ten_or_more":
            assert R.walk_class(g, rolling=False)[0] == "cells>NC" and g.cells.max() >= 10, (box, g.cells.max())
        else:
            assert (w, why) == (walk, reason), (box, w, why)
        assert R.walk_class(g, C=64)[1] is None  # the rolling walk is the C = 256 pooler's alone
    # the exact-edge boxes: samples exactly on -1, 0, integer cells, L - 1 and L
    for aligned, P in ((True, 7), (False, 14)):
        for ratio in ((0,) if aligned else (0, 2)):
            for name, box, lv in R.exact_edge_cases(aligned):
                g = R.roi_geometry(box, sizes, R.SCALES, P, ratio, aligned)
                assert g.lv == lv and g.gh == g.gw == 2 and float(g.bw) == 2.0 and float(g.bh) == 2.0
                for ax, L in ((g.x, g.W), (g.y, g.H)):
                    live = ax.v[~ax.skip]
                    assert np.array_equal(ax.v, np.round(ax.v)) and live.size
                    if name in ("on_minus1_and_0", "all_edges_p5"):
                        assert live[0] == -1.0 and live[1] == 0.0
                    if name.startswith("on_Lm1_and_L") or name == "all_edges_p5":
                        assert live[-1] == L and live[-2] == L - 1
                    if aligned:
                        assert not ax.skip.any()
