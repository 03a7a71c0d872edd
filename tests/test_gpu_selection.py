"""GPU suite (-m gpu): the selection kernels (csrc/proposals.hip) through ops.rpn_proposals / ops.box_detections / ops.group_nms, held to
tests/selection_ref.py (the host reference; held to the oracle on the CPU by tests/test_selection_ref_host.py) on every committed case.

Discrete outputs (count, scores, level / class, pos, keep masks, validity) are bit-exact; boxes are bit-exact where dw = dh = 0
(`exact` cases) and within 2e-3 px otherwise, with NMS and merge then re-run by the reference on the kernel's own boxes.  Box-head
probabilities are within 1e-6, and exact where every exponent is 0 or underflows.  No case is skipped or filtered here.

Kernel instance -> a case that reaches it (G = groups of the launch):
  rpn_select<1024>                    every RPN case with pre_topk <= 1024; index passes: ties/*; 24-bit index: count/index_24_bits
  rpn_select<2048>                    count/pre_topk_1025 / _2000 / _2048, ties/few_values_k2000, dispatch/k2000_*
  nms_mask<1024> + group_nms<1024,true>   every 1024-slot case of up to 1024 groups: dispatch/k1000_G5, _G1024, boxdet/G1024_exact, ...
  group_nms<1024,false>, inner 1      test_keep_masks_agree_through_all_three_routes (ops.group_nms), the existing keep-mask tests
  group_nms<1024,false>, inner > 1    dispatch/k1000_G1025 (inner 5), boxdet/G1026_general (inner 2)
  nms_mask<2048>, 64 row blocks       dispatch/k2000_G5, dispatch/k2000_G40, count/pre_topk_2000 (G 6)
  nms_mask<2048>, 16 row blocks       dispatch/k2000_G45
  group_nms<2048>                     every pre_topk > 1024 case
  merge_topk<1024,8192>               every 1024-slot case; 8192 keys at most: boxdet/C8_R1024_exact_at_third
  merge_topk<2048,16384>              every pre_topk > 1024 case
  box_candidates                      every boxdet/* case (C 1, 2, 8; R 7, 1000, 1024; counts 0, 1, R-1, R)
Which form a launch takes is not observable from its outputs: the map holds while the switches in proposals.hip stand where
selection_ref.route() states them (A3D_NMS_SPLIT_GROUPS = 1024 groups; `G <= 40` for 64 row blocks).  The host file asserts that the
dispatch cases sit on both sides of each switch as route() states it; whoever moves a switch moves route() and the cases with it.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import selection_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
BOX_TOL = 2e-3


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from articulation3d_amd import ops as o

    return o


def _np(t):
    return t.detach().cpu().numpy()


def run_rpn(ops, c, workspace=None):
    heads = [torch.from_numpy(h).cuda() for h in c.heads]
    out = ops.rpn_proposals(heads, c.strides, torch.from_numpy(c.cell), c.img_hw, pre_topk=c.pre_topk, post_topk=c.post_topk, nms_thresh=c.nms_thresh,
                            min_size=c.min_size, weights=c.weights, scale_clamp=c.scale_clamp, return_groups=c.pre_topk <= 1024, workspace=workspace)
    torch.cuda.synchronize()
    names = ("boxes", "scores", "level", "pos", "count")
    res = {k: _np(v) for k, v in zip(names, out)}
    res["groups"] = {k: _np(v) for k, v in out[5].items()} if len(out) > 5 else None
    return res


def run_boxdet(ops, c, workspace=None):
    out = ops.box_detections(torch.from_numpy(c.pred).cuda(), torch.from_numpy(c.prop_boxes).cuda(), torch.from_numpy(c.prop_count).cuda(), c.img_hw,
                             num_classes=c.C, score_thresh=c.score_thresh, nms_thresh=c.nms_thresh, topk=c.topk, weights=c.weights,
                             scale_clamp=c.scale_clamp, return_groups=True, workspace=workspace)
    torch.cuda.synchronize()
    res = {k: _np(v) for k, v in zip(("boxes", "scores", "classes", "pos", "count"), out)}
    res["groups"] = {k: _np(v) for k, v in out[5].items()}
    return res


def check_groups(got, ref, *, exact, nan_ok=False, score_tol=0.0, pos_live_only=False):
    """Group buffers of a 1024-slot launch against the reference's: n, scores, validity, positions exact; boxes exact or to BOX_TOL on
    every slot whose reference box is a number."""
    g, r = got["groups"], ref.groups
    assert np.array_equal(g["n"], r["n"])
    live = np.arange(1024)[None, :] < r["n"][:, None]
    if score_tol:
        assert float(np.abs(g["scores"] - r["scores"]).max(initial=0.0)) < score_tol
    else:
        assert S.same(g["scores"], r["scores"], nan_ok)
    assert np.array_equal(g["valid"].astype(bool), r["valid"])
    assert np.array_equal(g["pos"][live], r["pos"][live]) if pos_live_only else np.array_equal(g["pos"], r["pos"])
    num = np.isfinite(r["boxes"]).all(axis=2)
    d = np.abs(g["boxes"][num] - r["boxes"][num])
    print(f"group boxes: worst |kernel - reference| = {float(d.max(initial=0.0)):.3g} px over {int(num.sum())} slots")
    if exact:
        assert S.same(g["boxes"][num], r["boxes"][num])
    else:
        assert float(d.max(initial=0.0)) < BOX_TOL
    assert not g["boxes"][~live].any() and not g["scores"][~live].any()


def check_final(got, ref, cat, *, nan_ok=False, score_tol=0.0, exact_boxes=True):
    assert np.array_equal(got["count"], ref.count)
    assert np.array_equal(got[cat], getattr(ref, cat)) and np.array_equal(got["pos"], ref.pos)  # (-1 past count included)
    if score_tol:
        assert float(np.abs(got["scores"] - ref.scores).max(initial=0.0)) < score_tol
    else:
        assert S.same(got["scores"], ref.scores, nan_ok)
    assert S.same(got["boxes"], ref.boxes) if exact_boxes else float(np.abs(got["boxes"] - ref.boxes).max(initial=0.0)) < BOX_TOL
    assert np.isfinite(got["boxes"]).all() and np.isfinite(got["scores"]).all()
    past = np.arange(got["scores"].shape[1])[None, :] >= got["count"][:, None]
    assert not got["boxes"][past].any() and not got["scores"][past].any() and (got[cat][past] == -1).all() and (got["pos"][past] == -1).all()


@pytest.mark.parametrize("name", S.RPN_CASES)
def test_rpn_selection_equals_the_reference(ops, name):
    c = S.rpn_case(name)
    ref = S.rpn_expected(name)
    got = run_rpn(ops, c)
    if c.pre_topk > 1024:  # the 2048-slot layout does not expose its groups: exact-decode cases only, the final outputs bit for bit
        assert c.exact and got["groups"] is None
        check_final(got, ref, "level", nan_ok=c.nan_scores)
        return
    check_groups(got, ref, exact=c.exact, nan_ok=c.nan_scores)
    if not c.exact:  # no exp ulp decides a case: the reference's NMS and merge on the kernel's own boxes
        ref = S.rpn_reference(*S.rpn_args(c), boxes_from=got["groups"]["boxes"])
    assert np.array_equal(got["groups"]["keep"].astype(bool), ref.groups["keep"])
    check_final(got, ref, "level", nan_ok=c.nan_scores)


@pytest.mark.parametrize("name", S.BOXDET_CASES)
def test_box_detections_equal_the_reference(ops, name):
    c = S.boxdet_case(name)
    ref = S.boxdet_expected(name)
    tol = 0.0 if c.exact else S.SCORE_TOL
    if not c.exact:
        assert S.separated(c, ref)  # probabilities further apart than both sides' errors: the discrete outputs are exact all the same
    got = run_boxdet(ops, c)
    check_groups(got, ref, exact=c.exact, score_tol=tol, pos_live_only=True)
    if not c.exact:
        ref = S.boxdet_reference(*S.boxdet_args(c), boxes_from=got["groups"]["boxes"])
    assert np.array_equal(got["groups"]["keep"].astype(bool), ref.groups["keep"])
    check_final(got, ref, "classes", score_tol=tol)


def test_keep_masks_agree_through_all_three_routes(ops):
    """The same five groups (image 0 of the dispatch cases) through the global-words pair (G = 5), the LDS form inside a 1025-group launch
    (inner = 5) and ops.group_nms (LDS form, inner = 1) -- and all 1025 groups of the large launch through ops.group_nms as well."""
    small, large = S.rpn_case("dispatch/k1000_G5"), S.rpn_case("dispatch/k1000_G1025")
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(small.heads, large.heads))
    gs, gl = run_rpn(ops, small)["groups"], run_rpn(ops, large)["groups"]
    for k in ("boxes", "scores", "valid", "n", "keep"):
        assert np.array_equal(gs[k], gl[k][:5], equal_nan=True), k
    alone = _np(ops.group_nms(torch.from_numpy(gl["boxes"]).cuda(), torch.from_numpy(gl["valid"]).cuda(), torch.from_numpy(gl["n"]).cuda(), large.nms_thresh))
    assert np.array_equal(alone, gl["keep"])
    assert np.array_equal(alone.astype(bool), S.rpn_expected("dispatch/k1000_G1025").groups["keep"])
    # and a group that fills its thousand slots: the global-words pair of a small launch against the stand-alone LDS form
    full = run_rpn(ops, S.rpn_case("count/pre_topk_1000"))["groups"]
    assert full["n"].max() == 1000
    alone = _np(ops.group_nms(torch.from_numpy(full["boxes"]).cuda(), torch.from_numpy(full["valid"]).cuda(), torch.from_numpy(full["n"]).cuda(), 0.7))
    assert np.array_equal(alone, full["keep"])


@pytest.mark.parametrize("layout", [1000, 2000])
def test_a_small_launch_over_a_used_workspace_equals_one_over_a_fresh_one(ops, layout):
    """Rows at or past a group's n keep whatever the last launch left in the suppression words; nothing may read them."""
    from articulation3d_amd import _lib

    big = S.rpn_case(f"count/pre_topk_{layout}")                       # groups of 1000 / 2000 candidates
    small = S.rpn_case("ties/few_values_k20") if layout == 1000 else S.rpn_case("count/pre_topk_1025")
    small = S.types.SimpleNamespace(**{**small.__dict__, "heads": [h[:2, :5, :4].copy() for h in small.heads[:3]], "L": 3, "strides": small.strides[:3],
                                       "cell": small.cell[:3]})       # 2 images x 3 levels as `big`, 60 anchors a level: n = 20 / 60
    assert big.B * big.L == small.B * small.L == 6
    nbytes = _lib.lib().a3d_rpn_workspace_bytes(big.B, big.L, big.pre_topk)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    first = run_rpn(ops, big, workspace=ws)
    check_final(first, S.rpn_expected(big.name), "level")               # the caller's workspace serves the large launch ...
    used = run_rpn(ops, small, workspace=ws)                            # ... and then the small one, over the same bytes
    fresh_ws = torch.full((nbytes,), 0xFF, device="cuda", dtype=torch.uint8)  # every float a NaN, every count -1
    fresh = run_rpn(ops, small, workspace=fresh_ws)
    for k in ("boxes", "scores", "level", "pos", "count"):
        assert np.array_equal(used[k], fresh[k]), k
    if layout == 1000:
        for k in used["groups"]:
            assert np.array_equal(used["groups"][k], fresh["groups"][k]), k
    ref = S.rpn_reference(*S.rpn_args(small), boxes_from=None if small.exact or layout == 2000 else used["groups"]["boxes"])
    check_final(used, ref, "level")
    with pytest.raises(ValueError):
        run_rpn(ops, big, workspace=ws[: nbytes // 2])                    # a workspace too small is refused, not overrun


def test_box_detections_over_a_used_workspace(ops):
    c = S.boxdet_case("boxdet/C2_R1000_exact_thr0")
    ws = ops.group_workspace(c.B * c.C, "cuda")
    first = run_boxdet(ops, c, workspace=ws)
    check_final(first, S.boxdet_expected(c.name), "classes")
    few = S.types.SimpleNamespace(**{**c.__dict__, "prop_count": np.array([3, 0, 64, 65], dtype=np.int32)})
    used = run_boxdet(ops, few, workspace=ws)
    fresh = run_boxdet(ops, few, workspace=torch.full((ws.numel(),), 0xFF, device="cuda", dtype=torch.uint8))
    for k in ("boxes", "scores", "classes", "pos", "count"):
        assert np.array_equal(used[k], fresh[k]), k
    for k in used["groups"]:
        assert np.array_equal(used["groups"][k], fresh["groups"][k]), k
    check_final(used, S.boxdet_reference(*S.boxdet_args(few)), "classes")


def test_degenerate_images_give_finite_empty_outputs(ops):
    c = S.rpn_case("degenerate/invalid_suppressed")
    got = run_rpn(ops, c)
    assert got["count"].tolist() == [0, 2, 0]                              # all invalid / all but one per level suppressed / all NaN
    assert not got["groups"]["valid"][:2].any() and not got["groups"]["keep"][[0, 1, 4, 5]].any()
    assert got["groups"]["keep"][2:4].sum(axis=1).tolist() == [1, 1]
    check_final(got, S.rpn_expected(c.name), "level", nan_ok=True)
    c = S.boxdet_case("boxdet/C1_R7_exact")
    zero = S.types.SimpleNamespace(**{**c.__dict__, "prop_count": np.zeros(c.B, dtype=np.int32)})
    got = run_boxdet(ops, zero)
    assert not got["count"].any() and not got["groups"]["n"].any() and not got["groups"]["keep"].any()
    check_final(got, S.boxdet_reference(*S.boxdet_args(zero)), "classes")
    high = S.types.SimpleNamespace(**{**c.__dict__, "score_thresh": 1.0})     # nothing is above 1: no candidate in any class
    got = run_boxdet(ops, high)
    assert not got["count"].any()
    check_final(got, S.boxdet_reference(*S.boxdet_args(high)), "classes")
