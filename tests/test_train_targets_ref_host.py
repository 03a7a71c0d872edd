"""CPU suite: tests/train_targets_ref.py (the reference the matcher, the samplers and the RPN / box losses are held to on the GPU)
against the in-repo oracle wherever the oracle defines the answer, the proof that the committed case tables tell every deliberately
wrong reading (train_targets_ref.VARIANTS) from the right one, and the conditions the GPU tests rely on."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_targets_ref as R  # noqa: E402

from oracle import train_oracle as TO  # noqa: E402


# ---------------------------------------------------------------------------------------------- matcher
@pytest.mark.parametrize("name", R.MATCH_CASES)
def test_matcher_reference_equals_the_oracle_bit_for_bit(name):
    c = R.match_case(name)
    midx, lab, val = R.match(c)
    B, Gmax = c.gt_boxes.shape[:2]
    N = c.boxes.shape[-2]
    for b in range(B):
        G = min(int(c.gt_count[b]), Gmax)
        nb = N if c.box_count is None else max(0, min(int(c.box_count[b]), N))
        bx = torch.from_numpy(c.boxes if c.shared else c.boxes[b])[:nb]
        q = TO.pairwise_iou(torch.from_numpy(c.gt_boxes[b, :G]), bx)
        assert np.array_equal(q.numpy(), R.pair_iou(c.gt_boxes[b, :G], bx.numpy()))
        ri, rl = TO.matcher(q, c.thresholds, c.labels, c.lq)
        assert np.array_equal(midx[b, :nb], ri.numpy().astype(np.int32)), (name, b)
        assert np.array_equal(lab[b, :nb], rl.numpy()), (name, b)
        if G and nb:
            assert np.array_equal(val[b, :nb], q.max(0)[0].numpy())
        # rows past the live boxes keep the prefill
        assert not midx[b, nb:].any() and (lab[b, nb:] == -1).all() and not val[b, nb:].any()


def test_tie_cases_sit_exactly_on_their_thresholds_in_float32():
    q = R.pair_iou(np.array([R.A_], np.float32), R.TIE_BOXES)[0]
    role = R.TIE_ROLE
    assert q[role["equal"]] == np.float32(1.0) and q[15] == np.float32(1.0)
    assert q[role["half"]] == np.float32(0.5) == q[role["half_outer"]]
    assert q[role["f03"]] == np.float32(0.3) and q[role["f07"]] == np.float32(0.7)
    # the float32 threshold is below the double one for 0.7 and above it for 0.3: a double compare labels these boxes differently
    assert float(np.float32(0.7)) < 0.7 and float(np.float32(0.3)) > 0.3
    assert q[4] < np.float32(0.3) < q[5] and q[6] < np.float32(0.7) < q[7] and q[8] < np.float32(0.5)
    assert q[role["zero_area"]] == 0 and q[10] == 0 and q[12] == 0 and q[14] == 0
    # what the right reading makes of them
    rpn, prop = R.match_case("rpn_ties"), R.match_case("prop_ties")
    mi, lab, _ = R.match(rpn)
    assert lab[0, role["f03"]] == -1 and lab[0, role["f07"]] == 1 and lab[0, 4] == 0 and lab[0, 6] == -1
    assert (mi[1] != 1).all() and (mi[1] == 0).any()                # duplicated ground truth: the first wins, never the second
    assert mi[2, role["promoted"]] == 0 and lab[2, role["promoted"]] == 1 and lab[0, role["promoted"]] == 0  # promoted by gt 1, argmax gt 0
    assert (lab[3] == 1).all() and (lab[4] == 1).all()              # a best IoU of 0 is attained by every box
    assert lab[0, role["zero_area"]] == 0
    mi, lab, _ = R.match(prop)
    assert lab[0, role["half"]] == 1 and lab[0, role["half_outer"]] == 1 and lab[0, 8] == 0
    assert (lab[2] == -1).all() and (lab[3, 7:] == -1).all() and (lab[4] >= 0).all()  # box_count 0, mid, N + 5


def test_match_case_classes_are_populated():
    gs, ns, counts = set(), set(), set()
    for name in R.MATCH_CASES:
        c = R.match_case(name)
        N = c.boxes.shape[-2]
        gs |= {min(int(g), c.gt_boxes.shape[1]) for g in c.gt_count}
        ns.add(N)
        if c.box_count is not None:
            counts |= {"0" if k == 0 else "N" if k == N else "over" if k > N else "mid" for k in c.box_count}
        if name.endswith("_G"):
            assert sorted(c.gt_count.tolist()) == [0, 1, 64] and c.gt_boxes.shape[1] == R.MATCH_MAX_GT
    assert {0, 1, 64} <= gs and {1, 255, 257, 32769} <= ns and counts == {"0", "mid", "N", "over"}
    assert 32769 > 128 * 256  # the grid stride is live


MATCH_VARIANTS = ("thr_le", "last_max", "lq_skip_zero", "lq_moves_idx")


@pytest.mark.parametrize("variant", MATCH_VARIANTS)
def test_each_wrong_matcher_fails_on_the_case_list(variant):
    failing = [n for n in R.MATCH_CASES if any(not np.array_equal(a, b) for a, b in zip(R.match(R.match_case(n)), R.match(R.match_case(n), variant)))]
    assert failing, variant
    assert any(n.endswith("ties") for n in failing), (variant, failing)  # the hand-built launch alone tells it


# ---------------------------------------------------------------------------------------------- samplers
@pytest.mark.parametrize("name", R.SAMPLE_LABEL_CASES)
def test_subsample_reference_keeps_the_oracles_counts(name):
    c = R.sample_labels_case(name)
    out = R.subsample_labels(c.labels, c.num, c.max_pos, c.seed)
    for b in range(c.labels.shape[0]):
        lab = torch.from_numpy(np.where((c.labels[b] == 0) | (c.labels[b] == 1), c.labels[b], -1).astype(np.int64))  # (2 is ignored)
        pos, neg = TO.subsample_labels(lab, c.num, c.max_pos / c.num, 0, torch.Generator().manual_seed(0))
        assert int((out[b] == 1).sum()) == len(pos) and int((out[b] == 0).sum()) == len(neg)
        assert ((out[b] == 1) <= (c.labels[b] == 1)).all() and ((out[b] == 0) <= (c.labels[b] == 0)).all()
        assert ((out[b] == -1) | (out[b] == 0) | (out[b] == 1)).all()


def test_sampler_case_conditions():
    c = R.sample_labels_case("rows3")
    out = R.subsample_labels(c.labels, c.num, c.max_pos, c.seed)
    assert np.array_equal(c.labels[0], c.labels[1]) and not np.array_equal(out[0], out[1]) and not np.array_equal(out[1], out[2])
    c = R.sample_labels_case("seed_hi")
    assert c.seed >= 2 ** 32 and R.SEED_SAME_FOLD < 2 ** 32 and R.fold_seed(R.SEED_SAME_FOLD) == R.fold_seed(c.seed)
    out = R.subsample_labels(c.labels, c.num, c.max_pos, c.seed)
    assert np.array_equal(out, R.subsample_labels(c.labels, c.num, c.max_pos, R.SEED_SAME_FOLD))
    assert not np.array_equal(out, R.subsample_labels(c.labels, c.num, c.max_pos, R.SEED_SAME_LOW))
    e = R.sample_labels_case("edges")
    n1, n0 = (e.labels == 1).sum(1), (e.labels == 0).sum(1)
    assert n1[0] == 0 and n0[1] == 0 and n1[2] == e.labels.shape[1] and n1[3] + n0[3] < e.num and (e.labels[4] == 2).any()
    assert {R.sample_labels_case(n).labels.shape[1] for n in R.SAMPLE_LABEL_CASES} >= {1, 255, 1025, R.SAMPLE_LABELS_MAX_N}
    # ROI cases: every class of image in "counts"
    c = R.sample_rois_case("counts")
    ob, og, oc, oi, on = R.sample_rois(c)
    N = c.boxes.shape[1]
    assert c.box_count.tolist()[:4] == [0, 1, N, N + 3] and c.gt_count[4] == 0 and c.gt_count[5] == 0 and (c.match_label[5] == 1).all()
    assert on[0] == 0 and on[1] == 1 and on[2] == c.num and on[7] == 18
    assert (oc[4] == c.K).all() and (oc[5] == c.K).all() and np.array_equal(og[5], ob[5])  # no ground truth: background, gt box = the box
    nfg = (oc < c.K).sum(1)
    assert nfg[2] == c.max_fg and nfg[6] == 3 and nfg[7] == c.max_fg
    assert (oi[7, 18:] == -1).all() and (oc[7, 18:] == c.K).all() and not ob[7, 18:].any() and not og[7, 18:].any()
    for b in range(len(on)):  # the slot rule: keys ascend inside each class, foreground first
        key = R.sample_key(c.seed, b, N)
        k = key[oi[b, : on[b]]]
        f = int(nfg[b])
        assert (np.diff(k[:f].astype(np.int64)) > 0).all() and (np.diff(k[f:].astype(np.int64)) > 0).all()
        assert (oc[b, :f] < c.K).all() and (oc[b, f:] == c.K).all()
    assert {R.sample_rois_case(n).boxes.shape[1] for n in R.SAMPLE_ROI_CASES} >= {1, 1025, R.SAMPLE_ROIS_MAX_N}


def test_each_wrong_sampler_fails_on_the_case_list():
    assert any(not np.array_equal(R.subsample_labels(c.labels, c.num, c.max_pos, c.seed), R.subsample_labels(c.labels, c.num, c.max_pos, c.seed, "seed_hi_dropped"))
               for c in map(R.sample_labels_case, R.SAMPLE_LABEL_CASES))
    for variant in ("roi_index_order", "seed_hi_dropped"):
        assert any(any(not np.array_equal(a, b) for a, b in zip(R.sample_rois(c), R.sample_rois(c, variant))) for c in map(R.sample_rois_case, R.SAMPLE_ROI_CASES)), variant


def test_append_gt_reference_clamps_both_counts():
    p, g = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4) + 1, -np.arange(2 * 2 * 4, dtype=np.float32).reshape(2, 2, 4) - 1
    out, cnt = R.append_gt(p, [5, 1], g, [1, 9])
    assert cnt.tolist() == [4, 3]
    assert np.array_equal(out[0, :3], p[0]) and np.array_equal(out[0, 3], g[0, 0]) and not out[0, 4:].any()
    assert np.array_equal(out[1, 0], p[1, 0]) and np.array_equal(out[1, 1:3], g[1]) and not out[1, 3:].any()


# ---------------------------------------------------------------------------------------------- losses
def _f64_close(a, b, scale):
    return abs(a - b) <= 1e-12 * max(scale, 1e-300)


@pytest.mark.parametrize("name", list(R.RPN_CASES))
def test_rpn_reference_equals_the_oracle_in_float64(name):
    c = R.rpn_case(name)
    r = R.rpn_loss64(c)
    A, B = c.A, c.B
    anchors = torch.from_numpy(np.concatenate([R.level_anchors(c, l) for l in range(len(c.levels))])).double()
    logits = [torch.from_numpy(h[..., :A].astype(np.float64)).reshape(B, -1).requires_grad_(True) for h in c.heads]
    deltas = [torch.from_numpy(h[..., A : 5 * A].astype(np.float64)).reshape(B, -1, 4).requires_grad_(True) for h in c.heads]
    labels = torch.from_numpy(c.labels.astype(np.int64))
    mgt = torch.stack([torch.from_numpy(c.gt_boxes[b]).double()[torch.from_numpy(c.matched_idx[b]).long()] for b in range(B)])
    per = c.normalizer / B
    ref = TO.rpn_losses(logits, deltas, anchors, labels, mgt, SimpleNamespace(rpn_weights=c.weights), SimpleNamespace(rpn_batch_per_image=per))
    total = ref["loss_rpn_cls"] + ref["loss_rpn_loc"]
    if total.requires_grad:
        total.backward()
    # dyadic cases: the float32 targets ARE the float64 ones, so the two statements agree to float64 rounding.  Otherwise the float32
    # roundings of get_deltas (4 per target) separate them
    tol_loc = 1e-12 * r.abs[1] / c.normalizer if c.dyadic else R.gamma(4) * r.abs[1] / c.normalizer
    assert _f64_close(r.loss[0], ref["loss_rpn_cls"].item(), r.abs[0] / c.normalizer)
    assert abs(r.loss[1] - ref["loss_rpn_loc"].item()) <= tol_loc + 1e-300
    for l in range(len(c.levels)):
        g = logits[l].grad.numpy().reshape(r.glogit[l].shape) if logits[l].grad is not None else np.zeros_like(r.glogit[l])
        assert np.abs(g - r.glogit[l]).max() <= 1e-13 * r.scale
        gd = deltas[l].grad.numpy().reshape(r.gdelta[l].shape) if deltas[l].grad is not None else np.zeros(r.gdelta[l].shape)
        # torch's |x| has subgradient 0 at 0, like the contract; elsewhere +-1/normalizer
        assert np.array_equal(np.sign(gd), np.sign(r.gdelta[l].astype(np.float64))), name
        assert np.abs(gd - np.sign(gd) / c.normalizer).max() <= 1e-13 * r.scale


@pytest.mark.parametrize("name", list(R.BOX_CASES))
def test_box_reference_equals_the_oracle_in_float64(name):
    c = R.box_case(name)
    r = R.box_loss64(c)
    K = c.K
    live = torch.from_numpy(np.nonzero(r.live)[0])
    if len(live) == 0:
        assert r.loss[0] == 0 and r.loss[1] == 0 and not r.glogit.any() and not r.gdelta.any()
        return
    sc = torch.from_numpy(c.pred[:, : K + 1].astype(np.float64))[live].requires_grad_(True)
    dl = torch.from_numpy(c.pred[:, K + 1 : K + 1 + 4 * K].astype(np.float64))[live].requires_grad_(True)
    cfg = SimpleNamespace(num_classes=K, box_weights=c.weights)
    ref = TO.box_losses(sc, dl, torch.from_numpy(c.boxes).double()[live], torch.from_numpy(c.cls.astype(np.int64))[live],
                        torch.from_numpy(c.gt_boxes).double()[live], cfg)
    (ref["loss_cls"] + ref["loss_box_reg"]).backward()
    assert _f64_close(r.loss[0], ref["loss_cls"].item(), r.abs[0] * r.scale)
    assert _f64_close(r.loss[1], ref["loss_box_reg"].item(), r.abs[1] * r.scale)
    assert np.abs(sc.grad.numpy() - r.glogit[r.live]).max() <= 1e-13 * r.scale
    gd = dl.grad.numpy()
    assert np.array_equal(np.sign(gd), np.sign(r.gdelta[r.live].astype(np.float64)))
    assert np.abs(gd - np.sign(gd) * r.scale).max() <= 1e-13 * r.scale
    assert not r.glogit[~r.live].any() and not r.gdelta[~r.live].any()


def test_loss_case_conditions():
    """What the GPU tests rely on: exact-zero targets where they are planted, every other |df64| clear of 0 by the stated margin, and every
    class of case present."""
    seen_logits, levels, As, wide_ch, big = set(), set(), set(), set(), False
    for name in R.RPN_CASES:
        c = R.rpn_case(name)
        r = R.rpn_loss64(c)
        As.add(c.A)
        levels.add(len(c.levels))
        wide_ch.add(c.CH > 5 * c.A)
        big |= any(h * w > R.LOSS_BLOCKS * R.LOSS_THREADS for h, w, _ in c.levels)
        Hf, Wf, _ = c.levels[0]
        z0 = c.heads[0][0, ..., : c.A].reshape(-1)
        seen_logits |= {float(z) for z, lab in zip(z0, c.labels[0, : Hf * Wf * c.A]) if lab >= 0 and float(z) in R.SPECIAL_LOGITS}
        planted = np.zeros(r.df[0].shape, bool)
        for ai, d in c.zero_rows:
            planted[0].reshape(-1, 4)[ai] = True
            got = r.df[0][0].reshape(-1, 4)[ai]
            assert np.array_equal(got, np.array(d, np.float64)), (name, ai)  # the target is exactly 0: df is the head's value
            assert np.array_equal(r.gdelta[0][0].reshape(-1, 4)[ai], (np.sign(d) / np.float32(c.normalizer)).astype(np.float32))
        for l in range(len(c.levels)):
            df, tm = r.df[l], r.tgmag[l]
            m = ~np.isnan(df) & ~(planted if l == 0 else np.zeros(df.shape, bool))
            assert (np.abs(df[m]) > R.SIGN_MARGIN * tm[m] + 1e-30).all(), name
        if name.endswith("nopos"):
            assert not (c.labels[1] == 1).any() and (c.labels[0] == 1).any()
        if name.endswith("ignored"):
            assert (c.labels == -1).all() and r.loss[0] == 0 and r.loss[1] == 0
        else:
            assert len(c.zero_rows) == 3
    assert As == {1, 2, 3} and {2, 5} <= levels and wide_ch == {True, False} and big and seen_logits == set(R.SPECIAL_LOGITS)
    Ks, Ms, pads = set(), set(), set()
    for name in R.BOX_CASES:
        c = R.box_case(name)
        r = R.box_loss64(c)
        Ks.add(c.K)
        Ms.add(c.M)
        pads.add(c.pitch > 1 + 5 * c.K)
        assert set(c.cls[r.live].tolist()) == set(range(c.K + 1)) or c.M == 1 or not r.live.any()
        sc = c.pred[:, : c.K + 1]
        assert float((sc.max(1) - sc.min(1)).max()) == 80.0 or c.M == 1
        planted = np.zeros(c.M, bool)
        for row, d in c.zero_rows:
            planted[row] = True
            assert np.array_equal(r.df[row], np.array(d, np.float64))
        m = ~np.isnan(r.df) & ~planted[:, None]
        assert (np.abs(r.df[m]) > R.SIGN_MARGIN * r.tgmag[m] + 1e-30).all(), name
        if c.count is not None and r.live.any():
            assert sorted(("0" if k == 0 else "R" if k == c.R else "over" if k > c.R else "mid") for k in c.count) == ["0", "R", "mid", "over"]
            assert len(c.zero_rows) == 3
    assert Ks == {1, 2} and {1, 257, 16385} <= Ms and pads == {True, False}
    assert not R.box_loss64(R.box_case("k2_pad_ragged_dead")).live.any()


def test_each_wrong_loss_fails_on_the_case_list():
    def differs(a, b, fields):
        return any(not np.array_equal(np.asarray(x), np.asarray(y)) for f in fields for x, y in zip(np.atleast_1d(getattr(a, f)) if not isinstance(getattr(a, f), list) else getattr(a, f),
                                                                                                   np.atleast_1d(getattr(b, f)) if not isinstance(getattr(b, f), list) else getattr(b, f)))

    rpn = [R.rpn_case(n) for n in R.RPN_CASES if "big" not in n]
    box = [R.box_case(n) for n in R.BOX_CASES if "16385" not in n]
    assert any(differs(R.rpn_loss64(c), R.rpn_loss64(c, "sign0_plus"), ["gdelta"]) for c in rpn)
    assert any(differs(R.box_loss64(c), R.box_loss64(c, "sign0_plus"), ["gdelta"]) for c in box)
    assert any(differs(R.rpn_loss64(c), R.rpn_loss64(c, "ignored_counted"), ["glogit"]) for c in rpn)
    # dividing by M: beyond the law's bound on the ragged case, and not exactly zero... the losses move by a factor live / M
    c = R.box_case("k2_min_ragged")
    a, b = R.box_loss64(c), R.box_loss64(c, "box_div_M")
    assert abs(a.loss[0] - b.loss[0]) > 100 * R.loss_bound(a.nterm[0], R.kp_ce(c.K), a.abs[0], a.scale)
    assert differs(a, b, ["gdelta"])
    # the ignored anchors counted: far outside the law as well
    c = R.rpn_case("a2_ch16_l5")
    a, b = R.rpn_loss64(c), R.rpn_loss64(c, "ignored_counted")
    assert abs(a.loss[0] - b.loss[0]) > 100 * R.loss_bound(a.nterm[0], R.KP_BCE, a.abs[0], a.scale)
    assert set(R.VARIANTS) == set(MATCH_VARIANTS) | {"sign0_plus", "box_div_M", "ignored_counted", "roi_index_order", "seed_hi_dropped"}
