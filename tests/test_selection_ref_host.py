"""CPU suite: tests/selection_ref.py (the host reference the selection kernels are held to on the GPU) against the in-repo oracle, two
independent statements of SURVEY.md A.4-A.8, on every committed case -- and the proof that the case lists can tell each deliberately
wrong reading of the rules (selection_ref.VARIANTS) from the right one."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import selection_ref as S  # noqa: E402

BOX_TOL = 2e-3  # px: two float32 decodes that differ only through exp (test_stage_proposals_bit_exact_on_identical_heads)


def _oracle_rpn(O, c):
    cfg = O.OracleCfg(anchor_sizes=c.sizes, anchor_ratios=c.ratios, rpn_pre_topk=c.pre_topk, rpn_post_topk=c.post_topk,
                      rpn_nms_thresh=c.nms_thresh, rpn_min_size=c.min_size, rpn_weights=c.weights)
    lg = [torch.from_numpy(np.ascontiguousarray(h[..., :3])).reshape(c.B, -1) for h in c.heads]
    dl = [torch.from_numpy(np.ascontiguousarray(h[..., 3:15])).reshape(c.B, -1, 4) for h in c.heads]
    sources = []
    out, groups = O.rpn_select(lg, dl, [h.shape[1:3] for h in c.heads], [c.img_hw] * c.B, cfg, return_groups=True, sources=sources)
    return out, groups, sources


@pytest.mark.parametrize("name", S.RPN_CASES)
def test_rpn_reference_agrees_with_the_oracle(oracle, name):
    O, c = oracle, S.rpn_case(name)
    out, ogroups, sources = _oracle_rpn(O, c)
    ref = S.rpn_expected(name)
    cap = ref.groups["boxes"].shape[1]
    if not c.exact:  # exp's last place may differ between numpy and torch: NMS and merge on the ORACLE's boxes, compared bit for bit
        ob = np.zeros_like(ref.groups["boxes"])
        for b in range(c.B):
            for l in range(c.L):
                og = ogroups[b][l]
                ob[b * c.L + l, : len(og["scores"])] = np.nan_to_num(og["boxes"].numpy(), nan=0.0)
        own = ref.groups["boxes"]
        ref = S.rpn_reference(*S.rpn_args(c), boxes_from=ob)
    g = ref.groups
    for b in range(c.B):
        for l in range(c.L):
            gi, og = b * c.L + l, ogroups[b][l]
            k = len(og["scores"])
            assert int(g["n"][gi]) == k
            assert np.array_equal(g["idx"][gi, :k], og["idx"].numpy())                    # which anchors, in which order
            assert np.array_equal(g["scores"][gi, :k], og["scores"].numpy(), equal_nan=True)
            v = og["valid"].numpy()
            assert np.array_equal(g["valid"][gi, :k], v)
            if c.exact:
                assert np.array_equal(g["boxes"][gi, :k][v], og["boxes"].numpy()[v])
            else:
                assert float(np.abs(own[gi, :k][v] - og["boxes"].numpy()[v]).max(initial=0.0)) < BOX_TOL
            okeep = np.zeros(k, dtype=bool)
            okeep[v] = O.nms_sorted(torch.from_numpy(g["boxes"][gi, :k][v]), torch.zeros(int(v.sum()), dtype=torch.int64), c.nms_thresh).numpy()
            assert np.array_equal(g["keep"][gi, :k], okeep)
            assert not g["keep"][gi, k:].any() and not g["valid"][gi, k:].any()
        n = int(ref.count[b])
        oboxes, oscores = out[b]
        olev, oidx = sources[b]
        assert n == len(oboxes)
        assert np.array_equal(ref.scores[b, :n], oscores.numpy())
        assert np.array_equal(ref.level[b, :n], olev.numpy())
        sl = ref.pos[b, :n] & (cap - 1)
        assert np.array_equal(g["idx"][b * c.L + ref.level[b, :n], sl], oidx.numpy())    # the same anchors in the same order
        assert np.array_equal(ref.boxes[b, :n], oboxes.numpy())
        assert not ref.boxes[b, n:].any() and not ref.scores[b, n:].any() and (ref.level[b, n:] == -1).all() and (ref.pos[b, n:] == -1).all()


def _oracle_boxdet(O, c, b):
    n = int(c.prop_count[b])
    pr = torch.from_numpy(c.pred.reshape(c.B, c.R, -1)[b, :n])
    cfg = O.OracleCfg(score_thresh=c.score_thresh, nms_thresh=c.nms_thresh, num_classes=c.C, dets_per_image=c.topk, box_weights=c.weights)
    dec = O.apply_deltas(pr[:, c.C + 1: 5 * c.C + 1], torch.from_numpy(c.prop_boxes[b, :n]), cfg.box_weights, cfg.scale_clamp)
    return O.fast_rcnn_inference_single(dec, F.softmax(pr[:, : c.C + 1], dim=-1), c.img_hw, cfg)


@pytest.mark.parametrize("name", S.BOXDET_CASES)
def test_boxdet_reference_agrees_with_the_oracle(oracle, name):
    O, c = oracle, S.boxdet_case(name)
    ref = S.boxdet_expected(name)
    if not c.exact:
        assert S.separated(c, ref)  # no exp ulp decides a candidate, an order or a truncation: the discrete outputs are exact
    for b in range(c.B):
        ob, osc, ocl, orow = _oracle_boxdet(O, c, b)
        n = int(ref.count[b])
        assert n == len(ob)
        assert np.array_equal(ref.classes[b, :n], ocl.numpy())
        assert np.array_equal(ref.pos[b, :n], orow.numpy() * c.C + ocl.numpy())
        if c.exact:
            assert np.array_equal(ref.scores[b, :n], osc.numpy()) and np.array_equal(ref.boxes[b, :n], ob.numpy())
        else:
            assert float(np.abs(ref.scores[b, :n] - osc.numpy()).max(initial=0.0)) < S.SCORE_TOL
            assert float(np.abs(ref.boxes[b, :n] - ob.numpy()).max(initial=0.0)) < BOX_TOL
        assert not ref.boxes[b, n:].any() and not ref.scores[b, n:].any() and (ref.classes[b, n:] == -1).all() and (ref.pos[b, n:] == -1).all()


def test_order_agrees_with_topk_stable_and_nms_with_both_oracle_forms(oracle):
    O = oracle
    rng = np.random.default_rng(3)
    s = rng.choice(np.array([-0.0, 0.0, 1.0, -2.0, S.POS_NAN, S.NEG_NAN, S.INF, -S.INF], dtype=S.f32), size=500)
    for k in (1, 17, 499, 500):
        vals, idx = O.topk_stable(torch.from_numpy(s), k)
        mine = S.order_desc(s)[:k]
        assert np.array_equal(mine, idx.numpy()) and np.array_equal(s[mine], vals.numpy(), equal_nan=True)
    xy = rng.integers(0, 40, size=(120, 2))
    b = np.concatenate([xy, xy + rng.integers(0, 30, size=(120, 2))], axis=1).astype(S.f32)  # integer boxes: duplicates, zero areas, exact IoUs
    for thr in (0.5, 0.25, 0.7):
        mine = S.nms(b, np.ones(len(b), bool), thr)
        cats = torch.zeros(len(b), dtype=torch.int64)
        assert np.array_equal(mine, O.nms_sorted(torch.from_numpy(b), cats, thr).numpy())
        with np.errstate(invalid="ignore"):  # (0 / 0 between two zero-area boxes: NaN, not above any threshold)
            assert np.array_equal(mine, O.nms_sorted_py(torch.from_numpy(b), cats, thr).numpy())


def test_dispatch_cases_sit_on_both_sides_of_each_switch():
    want = {"dispatch/k2000_G5": ("slots2048", "rows64"), "dispatch/k2000_G40": ("slots2048", "rows64"), "dispatch/k2000_G45": ("slots2048", "rows16"),
            "dispatch/k1000_G5": ("slots1024", "global-words"), "dispatch/k1000_G1024": ("slots1024", "global-words"),
            "dispatch/k1000_G1025": ("slots1024", "lds-words")}
    for name, w in want.items():
        c = S.rpn_case(name)
        assert S.route(c.B * c.L, c.pre_topk) == w and c.B * c.L == int(name.rsplit("G", 1)[1]), name
    c = S.rpn_case("dispatch/k1000_G1025")
    assert c.L == 5  # the LDS form with the level-major group walk (inner = 5)
    for name, w in (("boxdet/G1024_exact", "global-words"), ("boxdet/G1026_general", "lds-words")):
        c = S.boxdet_case(name)
        assert S.route(c.B * c.C) == ("slots1024", w) and c.B * c.C == int(name.split("G")[1].split("_")[0])


# ------------------------------------------------------------------------------------------------------------------ teeth
def _differs(a, b, cat):
    return not (np.array_equal(a.count, b.count) and np.array_equal(a.scores, b.scores, equal_nan=True) and np.array_equal(a.pos, b.pos)
                and np.array_equal(getattr(a, cat), getattr(b, cat)) and np.array_equal(a.boxes, b.boxes))


TEETH = {  # every listed case must tell the variant from the truth
    "tie_high": ("ties/few_values_k20", "ties/all_equal_level", "boxdet/C1_R7_exact"),
    "nms_ge": ("ties/duplicates_iou_at_thr", "boxdet/C2_R1000_exact_thr0"),
    "invalid_suppress": ("nonfinite/logits_and_deltas", "count/min_size_8"),
    "thresh_ge": ("boxdet/C8_R1024_exact_at_third", "boxdet/C1_R7_exact"),
    "merge_pos_rev": ("ties/few_values_k20", "boxdet/G1024_exact"),
    "neg_nan_last": ("nonfinite/logits_and_deltas",),
}


@pytest.mark.parametrize("variant", S.VARIANTS)
def test_the_case_lists_catch_each_wrong_variant(variant):
    for name in TEETH[variant]:
        if name.startswith("boxdet/"):
            assert _differs(S.boxdet_expected(name), S.boxdet_expected(name, variant), "classes"), (variant, name)
        else:
            assert _differs(S.rpn_expected(name), S.rpn_expected(name, variant), "level"), (variant, name)


# ------------------------------------------------------------------------------------------------------------------ non-degeneracy
def _straddles(c, b, l):
    """Rank k of (image b, level l) falls inside a run of equal scores."""
    s = c.heads[l][b, :, :, :3].reshape(-1)
    k = min(c.pre_topk, s.size)
    o = S.order_desc(s)
    return k < s.size and s[o[k - 1]] == s[o[k]]


def test_tie_cases_really_tie_across_rank_k():
    c = S.rpn_case("ties/few_values_k20")
    assert all(_straddles(c, b, l) for b in range(c.B) for l in range(c.L))  # every level of every image
    for name, where in (("ties/few_values_k1000", (0, 0)), ("ties/few_values_k2000", (0, 0)), ("ties/few_values_k2000", (0, 1)), ("ties/all_equal_level", (0, 1)),
                        ("ties/pm_zero", (0, 0)), ("ties/duplicates_iou_at_thr", (0, 0)), ("ties/duplicates_iou_at_thr_k2000", (0, 0)), ("count/index_24_bits", (0, 1))):
        assert _straddles(S.rpn_case(name), *where), name
    c = S.rpn_case("ties/pm_zero")  # both zeros are selected, and in index order: they are one value
    sc = S.rpn_expected("ties/pm_zero").groups["scores"]
    z = sc[0, : c.pre_topk][sc[0, : c.pre_topk] == 0]
    assert np.signbit(z).any() and not np.signbit(z).all()
    assert not _straddles(S.rpn_case("count/index_24_bits"), 0, 0)  # and the early exit of a tie-free level is reached as well
    assert S.rpn_case("count/index_24_bits").heads[0].shape[1] * S.rpn_case("count/index_24_bits").heads[0].shape[2] * 3 > 65536


def test_cases_really_suppress_empty_truncate_and_touch_the_threshold():
    for name in S.RPN_CASES:
        c, r = S.rpn_case(name), S.rpn_expected(name)
        g = r.groups
        if name != "count/pre_topk_1":
            assert (g["valid"] & ~g["keep"]).any(), name  # some box is suppressed
        assert r.count.max() > 0, name
    for name in S.BOXDET_CASES:
        r = S.boxdet_expected(name)
        assert (r.groups["valid"] & ~r.groups["keep"]).any() and (r.groups["n"] == 0).any() and r.count.min() == 0 and r.count.max() > 0, name
    # an IoU exactly at the threshold between two KEPT boxes
    for r, thr in ((S.rpn_expected("ties/duplicates_iou_at_thr"), 0.5), (S.rpn_expected("ties/duplicates_iou_at_thr_k2000"), 0.5),
                   (S.boxdet_expected("boxdet/C2_R1000_exact_thr0"), 0.5)):
        g = r.groups
        hit = False
        for gi in range(len(g["n"])):
            kept = g["boxes"][gi][g["keep"][gi]]
            hit = hit or any((S.iou_row(kept, i) == S.f32(thr)).any() for i in range(min(len(kept), 40)))
        assert hit
    # empty groups and images; truncation at K and its absence
    d = S.rpn_expected("degenerate/invalid_suppressed")
    assert d.count.tolist() == [0, 2, 0] and not d.groups["valid"][:2].any() and d.groups["valid"][2:4].sum() == d.groups["n"][2:4].sum() == 240 + 60
    assert (S.rpn_expected("count/post_topk_50").count == 50).all() and (S.rpn_expected("count/post_topk_50").groups["keep"].reshape(2, -1).sum(1) > 50).all()
    full = S.rpn_expected("count/pre_topk_1000")
    assert (full.count < 1000).all() and np.array_equal(full.count, full.groups["keep"].reshape(2, -1).sum(1))
    for name in S.BOXDET_CASES:
        c, r = S.boxdet_case(name), S.boxdet_expected(name)
        kept = r.groups["keep"].reshape(c.B, -1).sum(1)
        assert np.array_equal(r.count, np.minimum(kept, c.topk))
    assert (S.boxdet_expected("boxdet/C2_R1000_exact_thr0").groups["keep"].reshape(4, -1).sum(1) > 100).any()   # truncates
    assert (S.boxdet_expected("boxdet/G1024_exact").groups["keep"].reshape(128, -1).sum(1) < 100).all()          # never does
    # a probability exactly at the threshold, in both exact-threshold cases
    for name in ("boxdet/C8_R1024_exact_at_third", "boxdet/C1_R7_exact", "boxdet/C2_R1000_exact_thr0", "boxdet/G1024_exact"):
        c, r = S.boxdet_case(name), S.boxdet_expected(name)
        assert any((p == S.f32(c.score_thresh)).any() for p in r.groups["probs"]), name
    assert S.boxdet_case("boxdet/C8_R1024_exact_at_third").score_thresh == float(S.f32(1.0) / S.f32(3.0))
    # equal scores in different groups of one image reach the merge
    r = S.boxdet_expected("boxdet/G1024_exact")
    assert any(len(set(r.classes[b, : r.count[b]])) > 1 and len(set(r.scores[b, : r.count[b]])) < r.count[b] for b in range(128))
    # non-finite rows of the box head are dropped whole, a -Inf dh keeps its row
    c, r = S.boxdet_case("boxdet/C2_R1000_general"), S.boxdet_expected("boxdet/C2_R1000_general")
    bad = ~np.isfinite(r.groups["probs"][3]).all(axis=1)
    assert bad[[7, 8, 9, 10]].all() and not bad[11] and bad.sum() == 4
    # the non-finite RPN case selects NaNs of both signs and Infs, and invalidates a box through each delta
    c, r = S.rpn_case("nonfinite/logits_and_deltas"), S.rpn_expected("nonfinite/logits_and_deltas")
    sc = r.groups["scores"]
    assert (np.isnan(sc) & np.signbit(sc)).any() and (np.isnan(sc) & ~np.signbit(sc)).any() and np.isposinf(sc).any()
    assert ((sc > 3.9) & ~r.groups["valid"]).sum() >= 10 and np.isfinite(r.boxes).all() and np.isfinite(r.scores).all()
    # boxes narrower than min_size with a positive area exist where min_size is set
    r = S.rpn_expected("count/min_size_8")
    b = r.groups["boxes"]
    assert (~r.groups["valid"] & ((b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) > 0)).any()
