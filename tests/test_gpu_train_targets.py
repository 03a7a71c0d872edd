"""GPU suite (-m gpu): the kernels that decide what a training step learns from -- a3d_match_boxes, a3d_sample_labels,
a3d_sample_rois, a3d_append_gt_boxes, a3d_rpn_loss, a3d_box_loss -- held to tests/train_targets_ref.py ("The
target contract").  Discrete outputs bit for bit on every committed case; every gradient element and both loss totals inside the
rounding law of the reference module, whose constants are counted from the kernels' source, not fitted."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_targets_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from articulation3d_amd import train_ops

    return train_ops


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- matcher
def _match_launch(c, fill):
    """a3d_match_boxes through the C entry point, the gt_best scratch pre-filled with `fill` bytes."""
    import ctypes as C

    from articulation3d_amd import _lib

    B, Gmax = c.gt_boxes.shape[:2]
    N = c.boxes.shape[-2]
    boxes, gtb, gtc = cu(c.boxes), cu(c.gt_boxes), cu(c.gt_count)
    bc = cu(c.box_count) if c.box_count is not None else None
    best = torch.full((B, Gmax), fill, dtype=torch.uint8).repeat_interleave(4, 1).cuda()
    midx = torch.zeros((B, N), device="cuda", dtype=torch.int32)
    lab = torch.full((B, N), -1, device="cuda", dtype=torch.int8)
    iou = torch.zeros((B, N), device="cuda", dtype=torch.float32)
    d = _lib.MatchDesc()
    d.boxes, d.box_count, d.gt_boxes, d.gt_count = boxes.data_ptr(), (bc.data_ptr() if bc is not None else None), gtb.data_ptr(), gtc.data_ptr()
    d.B, d.N, d.Gmax, d.box_batch_stride = B, N, Gmax, 0 if c.shared else N
    for i, t in enumerate(c.thresholds):
        d.thresholds[i] = float(t)
    for i, l in enumerate(c.labels):
        d.labels[i] = int(l)
    d.n_thresholds, d.allow_low_quality = len(c.thresholds), int(c.lq)
    d.gt_best, d.matched_idx, d.label, d.matched_iou = best.data_ptr(), midx.data_ptr(), lab.data_ptr(), iou.data_ptr()
    rc = _lib.lib().a3d_match_boxes(C.byref(d), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return midx.cpu().numpy(), lab.cpu().numpy(), iou.cpu().numpy()


@pytest.mark.parametrize("name", R.MATCH_CASES)
def test_matcher_is_bit_exact_on_every_edge_class(T, name):
    c = R.match_case(name)
    want = R.match(c)
    a, b = _match_launch(c, 0x00), _match_launch(c, 0xFF)  # whatever the scratch held before
    for w, x, y, what in zip(want, a, b, ("matched_idx", "label", "iou")):
        assert np.array_equal(x, y), (name, what, "depends on the scratch's old bytes")
        assert np.array_equal(w.view(np.uint32) if w.dtype == np.float32 else w, x.view(np.uint32) if x.dtype == np.float32 else x), \
            (name, what, np.argwhere(w != x)[:5].tolist())
    # the wrapper gives the same
    m2 = T.match_boxes(cu(c.boxes), cu(c.gt_boxes), cu(c.gt_count), thresholds=c.thresholds, labels=c.labels, allow_low_quality=c.lq,
                       shared=c.shared, box_count=None if c.box_count is None else cu(c.box_count), return_iou=True)
    for w, x in zip(want, m2):
        assert np.array_equal(w, x.cpu().numpy())


def test_matcher_refuses_more_ground_truth_than_it_stages(T):
    gt = torch.zeros(1, R.MATCH_MAX_GT + 1, 4).cuda()
    with pytest.raises(RuntimeError):
        T.match_boxes(torch.zeros(4, 4).cuda(), gt, torch.zeros(1, dtype=torch.int32).cuda(), thresholds=(0.5,), labels=(0, 1),
                      allow_low_quality=False, shared=True)


# ---------------------------------------------------------------------------------------------- samplers
@pytest.mark.parametrize("name", R.SAMPLE_LABEL_CASES)
def test_sample_labels_is_the_replay(T, name):
    c = R.sample_labels_case(name)
    want = R.subsample_labels(c.labels, c.num, c.max_pos, c.seed)
    got = T.sample_labels(cu(c.labels), num=c.num, max_pos=c.max_pos, seed=c.seed).cpu().numpy()
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5].tolist())
    if name == "edges":  # max_pos = 0: negatives only
        want = R.subsample_labels(c.labels, c.num, 0, c.seed)
        assert not (want == 1).any()
        assert np.array_equal(T.sample_labels(cu(c.labels), num=c.num, max_pos=0, seed=c.seed).cpu().numpy(), want)
    if name == "rows3":
        assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    if name == "seed_hi":
        assert np.array_equal(T.sample_labels(cu(c.labels), num=c.num, max_pos=c.max_pos, seed=R.SEED_SAME_FOLD).cpu().numpy(), got)
        assert not np.array_equal(T.sample_labels(cu(c.labels), num=c.num, max_pos=c.max_pos, seed=R.SEED_SAME_LOW).cpu().numpy(), got)


def test_sample_labels_refuses_an_index_that_does_not_fit_the_key(T):
    with pytest.raises(RuntimeError):
        T.sample_labels(torch.zeros((1, 1 << 17), dtype=torch.int8).cuda(), num=4, max_pos=2, seed=1)


@pytest.mark.parametrize("name", R.SAMPLE_ROI_CASES)
def test_sample_rois_fills_every_slot_by_the_rule(T, name):
    c = R.sample_rois_case(name)
    want = R.sample_rois(c)
    got = T.sample_rois(cu(c.boxes), cu(c.box_count), cu(c.gt_boxes), cu(c.gt_classes), cu(c.gt_count), cu(c.matched_idx), cu(c.match_label),
                        num_classes=c.K, num=c.num, max_fg=c.max_fg, seed=c.seed)
    for w, g, what in zip(want, got, ("boxes", "gt_boxes", "classes", "index", "count")):
        g = g.cpu().numpy()
        assert np.array_equal(w, g), (name, what, np.argwhere(w != g)[:5].tolist())


def test_sample_rois_refuses_more_candidates_than_it_stages(T):
    N = R.SAMPLE_ROIS_MAX_N + 1
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt).cuda()  # noqa: E731
    with pytest.raises(RuntimeError):
        T.sample_rois(z(1, N, 4, dt=torch.float32), z(1), z(1, 2, 4, dt=torch.float32), z(1, 2), z(1), z(1, N), z(1, N, dt=torch.int8),
                      num_classes=2, num=8, max_fg=2, seed=1)


def test_append_gt_boxes_clamps_both_counts(T):
    rng = np.random.default_rng(4)
    props, gt = rng.random((4, 6, 4)).astype(np.float32) + 1, -rng.random((4, 3, 4)).astype(np.float32) - 1
    count, gcount = np.array([0, 4, 6, 9], np.int32), np.array([3, 0, 5, 2], np.int32)  # count above R, gt_count above Gmax
    want, wcnt = R.append_gt(props, count, gt, gcount)
    out, cnt = T.append_gt_boxes(cu(props), cu(count), cu(gt), cu(gcount))
    assert np.array_equal(cnt.cpu().numpy(), wcnt) and wcnt.tolist() == [3, 4, 9, 8]
    assert np.array_equal(out.cpu().numpy(), want)  # (the zero tail included)


# ---------------------------------------------------------------------------------------------- losses
RATIOS = {}


def _note(kernel, what, ratio):
    key = (kernel, what)
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(ratio))
    print(f"[law] {kernel} {what}: worst ratio to the bound {float(ratio):.3f}")


def _check_total(kernel, what, got, want, bound):
    err = abs(float(got) - float(want))
    _note(kernel, what, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
    assert err <= bound, (kernel, what, float(got), float(want), err, bound)


def _rpn_launch(T, c, labels=None, midx=None, out=None):
    cell = torch.from_numpy(c.cell_anchors)
    return T.rpn_loss([cu(h) for h in c.heads], [st for _, _, st in c.levels], cell, cu(c.labels if labels is None else labels),
                      cu(c.matched_idx if midx is None else midx), cu(c.gt_boxes), A=c.A, weights=c.weights, normalizer=c.normalizer, out=out)


@pytest.mark.parametrize("name", list(R.RPN_CASES))
def test_rpn_loss_obeys_the_law_per_element(T, name):
    c = R.rpn_case(name)
    r = R.rpn_loss64(c)
    loss, dheads = _rpn_launch(T, c)
    loss = loss.cpu().numpy().astype(np.float64)
    A = c.A
    worst = 0.0
    for l, dh in enumerate(dheads):
        dh = dh.cpu().numpy()
        assert not dh[..., 5 * A :].any(), (name, l, "columns past 5A")
        gd = dh[..., A : 5 * A].reshape(r.gdelta[l].shape)
        assert np.array_equal(gd.view(np.uint32), r.gdelta[l].view(np.uint32)), (name, l, np.argwhere(gd != r.gdelta[l])[:5].tolist())
        err = np.abs(dh[..., :A].astype(np.float64) - r.glogit[l])
        bound = R.grad_bound(R.K_SIGMOID, r.p64[l], r.t[l], r.scale)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (name, l, float((err / bound).max()))
        dead = (r.p64[l] == 0) & (r.t[l] == 0) & (r.glogit[l] == 0)
        assert not dh[..., :A][dead].any()  # ignored anchors: exactly 0
    _note("a3d_rpn_loss", "logit gradient", worst)
    for ai, d in c.zero_rows:  # a target of exactly 0: the gradient is the sign of the head's own value, 0 at 0
        g = dheads[0][0].cpu().numpy().reshape(-1, c.CH)[ai // A, A + (ai % A) * 4 : A + (ai % A) * 4 + 4]
        assert np.array_equal(g, (np.sign(d) / np.float32(c.normalizer)).astype(np.float32)), (name, ai, g)
    _check_total("a3d_rpn_loss", "loss_cls", loss[0], r.loss[0], R.loss_bound(r.nterm[0], R.KP_BCE, r.abs[0], r.scale))
    _check_total("a3d_rpn_loss", "loss_loc", loss[1], r.loss[1], R.loss_bound(r.nterm[1], R.KP_L1, r.abs[1], r.scale))
    if name.endswith("ignored"):
        assert loss[0] == 0 and loss[1] == 0 and all(not dh.any() for dh in dheads)


def test_rpn_loss_refuses_a_misdeclared_atotal_before_any_launch(T):
    """labels / matched_idx wider than the levels' sum: refused, with not a byte of the gradients or the losses written."""
    c = R.rpn_case("a2_ch16_l5")
    pad = 6
    labels = np.concatenate([c.labels, np.full((c.B, pad), -1, np.int8)], 1)
    midx = np.concatenate([c.matched_idx, np.zeros((c.B, pad), np.int32)], 1)
    sentinel = -123.25
    loss = torch.full((2,), sentinel, device="cuda")
    dheads = [torch.full(h.shape, sentinel, device="cuda") for h in c.heads]
    with pytest.raises(RuntimeError):
        _rpn_launch(T, c, labels, midx, out=(loss, dheads))
    torch.cuda.synchronize()
    assert bool((loss == sentinel).all()) and all(bool((g == sentinel).all()) for g in dheads)
    # the same buffers with the right width are written
    l2, _ = _rpn_launch(T, c, out=(loss, dheads))
    assert l2.data_ptr() == loss.data_ptr() and not bool((loss == sentinel).any()) and all(not bool((g == sentinel).any()) for g in dheads)


@pytest.mark.parametrize("name", list(R.BOX_CASES))
def test_box_loss_obeys_the_law_per_row(T, name):
    c = R.box_case(name)
    r = R.box_loss64(c)
    K = c.K
    kw = {} if c.count is None else dict(count=cu(c.count), rows_per_image=c.R)
    loss, dpred = T.box_loss(cu(c.pred), cu(c.cls), cu(c.boxes), cu(c.gt_boxes), num_classes=K, weights=c.weights, **kw)
    loss, dpred = loss.cpu().numpy().astype(np.float64), dpred.cpu().numpy()
    assert not dpred[~r.live].any(), (name, "dead rows over the whole pitch")
    assert not dpred[:, 1 + 5 * K :].any(), (name, "padding columns")
    gd = np.ascontiguousarray(dpred[:, K + 1 : K + 1 + 4 * K])
    assert np.array_equal(gd.view(np.uint32), r.gdelta.view(np.uint32)), (name, np.argwhere(gd != r.gdelta)[:5].tolist())
    for row, d in c.zero_rows:
        g = dpred[row, K + 1 + c.cls[row] * 4 : K + 5 + c.cls[row] * 4]
        assert np.array_equal(g, (np.sign(d) * (np.float32(1) / np.float32(1.0 / r.scale))).astype(np.float32)), (name, row, g)
    err = np.abs(dpred[:, : K + 1].astype(np.float64) - r.glogit)
    k = R.k_softmax(K, r.lse[:, None], r.logse[:, None], c.pred[:, : K + 1].astype(np.float64))
    bound = R.grad_bound(k, r.p64, r.t, r.scale)
    _note("a3d_box_loss", "logit gradient", (err / bound).max())
    assert (err <= bound).all(), (name, float((err / bound).max()), np.argwhere(err > bound)[:5].tolist())
    if not r.live.any():
        assert loss[0] == 0 and loss[1] == 0 and not dpred.any()
        return
    _check_total("a3d_box_loss", "loss_cls", loss[0], r.loss[0], R.loss_bound(r.nterm[0], R.kp_ce(K), r.abs[0], r.scale))
    _check_total("a3d_box_loss", "loss_box_reg", loss[1], r.loss[1], R.loss_bound(r.nterm[1], R.KP_L1, r.abs[1], r.scale))
