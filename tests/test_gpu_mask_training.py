"""GPU suite (-m gpu) for the stage-3 training step (configs/step3_mask.yaml, articulation3d_amd/training_mask.py): the two new kernels
(a3d_mask_targets, a3d_mask_loss) against the references of tests/mask_train_ref.py, the frozen detector against stage 1's step bit for
bit, the whole step against float64 autograd of the reference's mask head on the trainer's own pooled rows, the SGD update, training
progress and the reference-style drop-in call."""
import os

import pytest
import torch
import torch.nn.functional as F

import mask_train_ref as R

pytestmark = pytest.mark.gpu

MH = R.MH


def l2rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from articulation3d_amd import train_ops

    return train_ops


# ------------------------------------------------------------------------------------------ a3d_mask_targets
SENTINEL = 0xA5


def _run_targets(T, masks, boxes, gt, cap=128):
    """The boxes of a target_case as the compact rows of a batch: `cap` slots per image, rows past the live count filled with a sentinel."""
    B, n = boxes.shape[:2]
    slots = torch.full((B, cap, 4), float("nan"))
    slots[:, :n] = boxes
    count = torch.full((B,), n, dtype=torch.int32)
    row_offset = torch.arange(B + 1, dtype=torch.int32) * n
    rows = B * cap
    row_gt = torch.full((rows,), 10 ** 6, dtype=torch.int32)  # (dead rows: an index that must never be used)
    row_gt[: B * n] = gt.reshape(-1)
    live = torch.tensor([B * n], dtype=torch.int32)
    out = torch.full((rows, 28, 28), SENTINEL, dtype=torch.uint8, device="cuda")
    c = lambda t: t.cuda().contiguous()
    T.mask_targets(c(masks), c(slots), c(count), c(row_offset), c(row_gt), c(live), rows=rows, size=28, out=out)
    torch.cuda.synchronize()
    return out.cpu(), B * n


@pytest.mark.parametrize("hw", [(480, 640), (96, 128)])
def test_mask_targets_match_the_float64_roi_align_outside_the_tie_margin(T, oracle, hw):
    masks, boxes, gt = R.target_case(hw[0], hw[1], seed=5)
    v64 = R.target_case_values(oracle, masks, boxes, gt, torch.float64)
    out, live = _run_targets(T, masks, boxes, gt)
    assert live == 240 and bool((out[live:] == SENTINEL).all())  # rows past the live count are not written
    R.check_targets(out[:live], v64)
    t = out[:live].view(2, 120, 28, 28)
    assert not t[:, 2].any() and not t[:, 3].any()  # zero-width / zero-height boxes: all-zero targets
    out2, _ = _run_targets(T, masks, boxes, gt)
    assert torch.equal(out, out2)  # bit-reproducible
    # 0 / non-zero bytes and bool masks are the same mask
    out3, _ = _run_targets(T, masks * 255, boxes, gt)
    assert torch.equal(out, out3)


def test_mask_targets_edge_rows(T, oracle):
    """A slot past its image's count, a ground-truth index out of range and non-finite / inverted boxes give zeros; no live row: nothing
    is written."""
    masks, boxes, gt = R.target_case(96, 128, seed=9, per_image=8)
    boxes[0, 7] = torch.tensor([50.0, 40.0, 20.0, 10.0])  # inverted
    boxes[1, 6] = torch.tensor([float("nan"), 0.0, 30.0, 30.0])
    boxes[1, 7] = torch.tensor([0.0, 0.0, float("inf"), 30.0])
    gt[1, 5] = 6  # past max_gt
    v64 = R.target_case_values(oracle, masks, boxes[:, :6].contiguous(), gt[:, :6].clamp(max=5).contiguous(), torch.float64).view(2, 6, 28, 28)
    out, live = _run_targets(T, masks, boxes, gt, cap=16)
    t = out[:live].view(2, 8, 28, 28)
    assert not t[0, 7].any() and not t[1, 5:].any()
    R.check_targets(torch.cat((t[0, :6], t[1, :5])), torch.cat((v64[0], v64[1, :5])), fraction=1.0)
    c = lambda x: x.cuda().contiguous()
    keep = torch.full((32, 28, 28), SENTINEL, dtype=torch.uint8, device="cuda")
    slots = torch.zeros(2, 16, 4)
    T.mask_targets(c(masks), c(slots), c(torch.zeros(2, dtype=torch.int32)), c(torch.zeros(3, dtype=torch.int32)),
                   c(torch.zeros(32, dtype=torch.int32)), c(torch.zeros(1, dtype=torch.int32)), rows=32, size=28, out=keep)
    torch.cuda.synchronize()
    assert bool((keep == SENTINEL).all())


# ------------------------------------------------------------------------------------------ a3d_mask_loss
def _loss_case(rows=40, live=23, seed=11):
    g = torch.Generator().manual_seed(seed)
    P, C = 14, 256
    yu = torch.randn(rows, P, P, 4 * C, generator=g)  # positive and non-positive entries
    yu[torch.rand(yu.shape, generator=g) < 0.05] = 0.0  # exact zeros: the gate is closed at 0
    w = torch.randn(C, generator=g) * 0.05
    b = torch.tensor([0.1])
    t = (torch.rand(rows, 2 * P, 2 * P, generator=g) < 0.4).to(torch.uint8)
    # |z| = 40 and 100 on a few pixels, both signs and both targets: y = w (z - b) / |w|^2 gives w . y + b = z
    big = [(0, 0, 0, 0, 40.0), (1, 3, 5, 1, -40.0), (2, 13, 13, 2, 100.0), (3, 7, 0, 3, -100.0), (22, 0, 13, 0, 100.0), (22, 13, 0, 3, -40.0)]
    big = [e for e in big if e[0] < rows]
    for n, (r, iy, ix, q, z) in enumerate(big):
        yu[r, iy, ix, q * C:(q + 1) * C] = w * ((z - b.item()) / float(w.double().pow(2).sum()))
        t[r, 2 * iy + (q >> 1), 2 * ix + (q & 1)] = n % 2
    yu[live:] = float("nan")  # dead rows: never read
    t[live:] = 255
    return yu, t, w, b, big


def _loss_ref(yu, t, w, b, live):
    x = R.shuffle(yu[:live].double()).requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    z = F.conv2d(x, wd.view(1, -1, 1, 1), bd)[:, 0]
    loss = F.binary_cross_entropy_with_logits(z, t[:live].double(), reduction="mean")
    loss.backward()
    dyu = R.unshuffle(x.grad) * (yu[:live] > 0)
    return loss.detach(), dyu, wd.grad, bd.grad, z.detach()


def _run_loss(T, yu, t, w, b, live, want_z=False):
    c = lambda x: x.cuda().contiguous()
    dyu = torch.full_like(yu, 7.0).cuda()
    z = torch.full(t.shape, 7.0, device="cuda") if want_z else None
    out, dyu = T.mask_loss(c(yu), c(t), c(w), c(b), torch.tensor([live], dtype=torch.int32, device="cuda"), dyu=dyu, z=z)
    torch.cuda.synchronize()
    return out.cpu(), dyu.cpu(), None if z is None else z.cpu()


def test_mask_loss_matches_float64_autograd(T):
    rows, live = 40, 23
    yu, t, w, b, big = _loss_case(rows, live)
    out, dyu, z = _run_loss(T, yu, t, w, b, live, want_z=True)
    loss, rdyu, rdw, rdb, rz = _loss_ref(yu, t, w, b, live)
    C = 256
    print("loss", out[C + 1].item(), loss.item(), "dyu", l2rel(dyu[:live], rdyu), "dw", l2rel(out[:C], rdw), "db", l2rel(out[C:C + 1], rdb))
    assert bool(torch.isfinite(out).all())
    for r, iy, ix, q, zz in big:  # the large logits are where they were put
        assert abs(rz[r, 2 * iy + (q >> 1), 2 * ix + (q & 1)].item() - zz) < 1e-3
    assert abs(out[C + 1].item() - loss.item()) <= 1e-6 * abs(loss.item()), (out[C + 1].item(), loss.item())
    assert l2rel(dyu[:live], rdyu) < 1e-5 and l2rel(out[:C], rdw) < 1e-5 and l2rel(out[C:C + 1], rdb) < 1e-5
    assert l2rel(z[:live], rz) < 1e-5
    assert bool((dyu[:live][yu[:live] <= 0] == 0).all())  # the ReLU gate: exactly 0 where the activation is not positive
    assert bool((dyu[live:] == 7.0).all()) and bool((z[live:] == 7.0).all())  # rows past the live count: untouched
    out2, dyu2, _ = _run_loss(T, yu, t, w, b, live)
    assert torch.equal(out, out2) and torch.equal(dyu[:live], dyu2[:live])  # bit-reproducible


def test_mask_loss_without_live_rows_is_zero(T):
    yu, t, w, b, _ = _loss_case(8, 0, seed=12)
    out, dyu, z = _run_loss(T, yu, t, w, b, 0, want_z=True)
    assert out.tolist() == [0.0] * 258  # loss 0.0 and every gradient exactly 0 (detectron2: pred_mask_logits.sum() * 0)
    assert bool((dyu == 7.0).all()) and bool((z == 7.0).all())


def test_mask_loss_full_rows_and_one_row(T):
    """live == rows, and a single row (fewer units than waves: most workgroups hold empty partials)."""
    for rows, live in ((5, 5), (3, 1)):
        yu, t, w, b, _ = _loss_case(rows, rows, seed=13)
        yu, t = yu.clone(), t.clone()
        yu[live:] = float("nan")
        out, dyu, _ = _run_loss(T, yu, t, w, b, live)
        loss, rdyu, rdw, rdb, _ = _loss_ref(yu, t, w, b, live)
        assert abs(out[257].item() - loss.item()) <= 1e-6 * abs(loss.item())
        assert l2rel(dyu[:live], rdyu) < 1e-5 and l2rel(out[:256], rdw) < 1e-5 and l2rel(out[256:257], rdb) < 1e-5


# ------------------------------------------------------------------------------------------ the step
def _ellipse_masks(boxes, H=480, W=640):
    """The ellipse inscribed in each ground-truth box, [G, H, W] bool."""
    yy, xx = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    out = []
    for x1, y1, x2, y2 in boxes.tolist():
        out.append((((xx - (x1 + x2) / 2) / ((x2 - x1) / 2)) ** 2 + ((yy - (y1 + y2) / 2) / ((y2 - y1) / 2)) ** 2) <= 1)
    return torch.stack(out)


@pytest.fixture(scope="module")
def batch(oracle):
    from oracle import train_oracle as TO

    frames = torch.from_numpy(oracle.synthetic_frames(2)).cuda()
    tg = TO.synthetic_targets(2)
    return frames, [t[0] for t in tg], [t[1] for t in tg], [_ellipse_masks(t[0]) for t in tg]


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_frozen_forward_is_stage_ones_forward_bit_for_bit(hip_model, batch, precision):
    from articulation3d_amd.training import DetectorTrainer
    from articulation3d_amd.training_mask import MaskTrainer

    frames, gb, gc, gm = batch
    t1 = DetectorTrainer(hip_model, seed=13, precision=precision)
    l1, a1 = t1.forward_backward(frames, gb, gc)
    t2 = MaskTrainer(hip_model, seed=13, precision=precision)
    l2, a2 = t2.forward_backward(frames, gb, gc, gm)
    torch.cuda.synchronize()
    assert set(l2) == {"loss_cls", "loss_box_reg", "loss_mask"}
    for k in ("loss_cls", "loss_box_reg"):
        assert torch.equal(l1[k], l2[k]), k
    for k in ("roi_index", "roi_count", "roi_cls", "roi_boxes"):
        assert torch.equal(a1[k], a2[k]), k
    assert torch.equal(a1["proposals"][0], a2["proposals"][0]) and torch.equal(a1["proposals"][1], a2["proposals"][1])


def _fg_restated(aux, s, B):
    """select_foreground_proposals on the host: per image the sampled rows whose class is not background, in sample order."""
    rc, cls, ri, pm = aux["roi_count"].cpu(), aux["roi_cls"].cpu(), aux["roi_index"].cpu().long(), aux["proposal_match"].cpu().long()
    rows = []
    for b in range(B):
        for r in range(int(rc[b])):
            if int(cls[b, r]) < s.num_classes:
                rows.append((b, r, int(pm[b, ri[b, r]])))
    return rows


@pytest.mark.parametrize("precision,shuffled", [("bf16x3", False), ("fp32", False), ("bf16", False), ("bf16x3", True)])
def test_mask_step_matches_float64_autograd(hip_model, oracle, batch, precision, shuffled):
    """shuffled: the samples= hook with the drawn ROI index sets in a random order (foreground rows scattered among the background)."""
    from articulation3d_amd.training import lr_at
    from articulation3d_amd.training_mask import MaskTrainer

    frames, gb, gc, gm = batch
    tr = MaskTrainer(hip_model, seed=21, precision=precision)
    p0 = {k: v.clone() for k, v in tr.export_state_dict().items()}
    samples = None
    if shuffled:
        _, a0 = MaskTrainer(hip_model, seed=21, precision=precision).forward_backward(frames, gb, gc, gm)
        rc, ri = a0["roi_count"].cpu(), a0["roi_index"].cpu()
        g = torch.Generator().manual_seed(4)
        sets = [ri[i, : int(rc[i])].long() for i in range(frames.shape[0])]
        samples = dict(roi_idx=[s_[torch.randperm(len(s_), generator=g)] for s_ in sets])
        del a0
    model_before = {k: v.clone() for k, v in hip_model.state_dict().items()}
    losses, aux = tr.forward_backward(frames, gb, gc, gm, samples=samples)
    torch.cuda.synchronize()
    B = frames.shape[0]
    if shuffled:
        for i in range(B):
            assert torch.equal(aux["roi_index"][i, : len(samples["roi_idx"][i])].cpu().long(), samples["roi_idx"][i])
    # the foreground rows, restated on the host
    fg = aux["fg"]
    rows = _fg_restated(aux, tr.s, B)
    live = int(fg["live"])
    assert live == len(rows) > 0
    assert fg["count"].cpu().tolist() == [sum(1 for r in rows if r[0] == b) for b in range(B)]
    assert fg["row_img"][:live].cpu().tolist() == [r[0] for r in rows] and fg["row_gt"][:live].cpu().tolist() == [r[2] for r in rows]
    # the pooled rows: the oracle's pooler with the mask pooler's own settings on the trainer's pyramid
    mp = hip_model.roi_heads.mask_pooler
    assert (tr.pool_size, tr.pool_ratio, tr.pool_aligned) == (mp.output_size, mp.sampling_ratio, mp.aligned) == (14, 2, False)
    feats = {n: aux["feats"][n].permute(0, 3, 1, 2).cpu() for n in ("p2", "p3", "p4", "p5")}
    boxes = [aux["roi_boxes"][b].cpu()[[r[1] for r in rows if r[0] == b]] for b in range(B)]
    pooled_ref = oracle.roi_pool_fpn(feats, boxes, mp.output_size, mp.sampling_ratio, mp.aligned)
    pooled = aux["pooled"][:live].permute(0, 3, 1, 2).cpu()
    assert l2rel(pooled, pooled_ref) < 1e-6
    # the targets of every live row: the float64 ROIAlign of the matched ellipse in the row's proposal box
    G = max(len(m) for m in gm)
    flat = torch.zeros(B * G, 480, 640, dtype=torch.uint8)
    for b, m in enumerate(gm):
        flat[b * G: b * G + len(m)] = m
    v64 = R.roi_values(oracle, flat, torch.cat(boxes), torch.tensor([b * G + g_ for b, _, g_ in rows]), 28, torch.float64)
    targets = aux["mask_targets"][:live].cpu()
    R.check_targets(targets, v64)
    assert 0 < int(targets.sum()) < targets.numel()
    # float64 autograd of the reference's mask head + mask_rcnn_loss on the trainer's own pooled rows and targets
    P = {k: v.double().requires_grad_(True) for k, v in p0.items()}
    want = R.mask_loss_ref(pooled.cuda().double(), P, targets.cuda())
    want.backward()
    got = losses["loss_mask"]
    assert abs(got.item() - want.item()) <= (1e-5 if precision != "bf16" else 2e-2) * abs(want.item()), (got.item(), want.item())
    g = tr.export_grads()
    assert set(g) == set(P) and len(g) == 12 and sum(v.numel() for v in p0.values()) == 4 * (256 * 256 * 9 + 256) + 256 * 256 * 4 + 256 + 257
    assert g[MH + "deconv.weight"].shape == (256, 256, 2, 2) and g[MH + "predictor.weight"].shape == (1, 256, 1, 1)
    errs = {k: l2rel(g[k], P[k].grad) for k in g}
    print(precision, "loss_mask", got.item(), want.item(), "relative L2 gradient errors:", {k[len(MH):]: f"{v:.2e}" for k, v in errs.items()})
    bound = 2e-4 if precision != "bf16" else 5e-2
    for k, e in errs.items():
        assert e < bound, (k, e)
    # update: the float64 SGD formula on the mask parameters
    tr.optimizer_step()
    s = tr.s
    lr0 = lr_at(0, s)
    p1 = tr.export_state_dict()
    for k in p0:
        d = g[k].double() + s.weight_decay * p0[k].double()
        want_p = p0[k].double() - lr0 * d  # first step: the momentum buffer starts as the gradient
        assert l2rel(p1[k], want_p) < 1e-6, k
    assert any(not torch.equal(p0[k], p1[k]) for k in p0)
    # every parameter and buffer of the model outside the mask head, after the step and after the write-back of leaving training mode
    assert all(torch.equal(v, hip_model.state_dict()[k]) for k, v in model_before.items())
    hip_model.train()
    hip_model._trainer = tr
    hip_model.train(False)
    del hip_model._trainer
    try:
        after = hip_model.state_dict()
        for k, v in model_before.items():
            if k.startswith(MH):
                assert torch.equal(after[k].float(), p1[k].float()), k  # (the trained mask head reaches the model)
            else:
                assert torch.equal(after[k], v), k
        # the inference forward of the updated head
        x = torch.randn(5, 256, 14, 14, device="cuda")
        with torch.no_grad():
            prob = hip_model.roi_heads.mask_head.forward_rows(nhwc(x))
            ref = R.mask_head_logits(x.double(), {k: v.double() for k, v in p1.items()}).sigmoid()
        assert prob.shape == (5, 28, 28) and l2rel(prob, ref) < 1e-4, l2rel(prob, ref)
    finally:
        hip_model.load_state_dict(model_before)  # (the session-scoped model goes back to the weights the other tests expect)


def test_mask_loss_decreases_on_a_fixed_batch(hip_model, batch):
    from articulation3d_amd.training import SolverCfg
    from articulation3d_amd.training_mask import MaskTrainer

    frames, gb, gc, gm = batch
    tr = MaskTrainer(hip_model, SolverCfg(base_lr=0.02, warmup_iters=0), seed=3)
    hist = []
    for _ in range(8):
        l, _ = tr.step(frames, gb, gc, gm)
        hist.append(l["loss_mask"])
    hist = torch.stack(hist).cpu()
    print("loss_mask over 8 steps:", hist.tolist())
    assert bool(torch.isfinite(hist).all()) and hist[-1] < hist[0], hist.tolist()


def test_reference_training_loop_is_a_drop_in_for_the_mask_stage(oracle, oracle_params, batch):
    """model.train(); losses = model(data); sum(losses.values()).backward(); build_optimizer(cfg, model).step(); model.eval(): the
    trained mask weights reach inference."""
    from conftest import ROOT
    from articulation3d_amd.config import get_cfg, get_planercnn_cfg_defaults
    from articulation3d_amd.engine import build_optimizer
    from articulation3d_amd.modeling import build_model
    from articulation3d_amd.structures import BitMasks, Boxes, Instances

    cfg = get_cfg()
    get_planercnn_cfg_defaults(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "step3_mask.yaml"))
    cfg.MODEL.DEVICE = "cuda"
    model = build_model(cfg)
    missing, unexpected = model.load_state_dict(oracle_params, strict=False)
    assert not unexpected and all("num_batches_tracked" in k for k in missing)
    assert model.training_stage() == 3
    frames, gb, gc, gm = batch
    data = []
    for i in range(frames.shape[0]):
        inst = Instances((480, 640), gt_boxes=Boxes(gb[i].cuda()), gt_classes=gc[i].cuda(), gt_masks=BitMasks(gm[i]))
        data.append({"image": frames[i].permute(2, 0, 1).cpu(), "instances": inst})
    model.train()
    losses = model(data)
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_mask"}
    sum(losses.values()).backward()
    optimizer = build_optimizer(cfg, model)
    from articulation3d_amd.training_mask import MaskTrainer

    assert isinstance(model.trainer(), MaskTrainer)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    optimizer.step()
    model.eval()
    after = model.state_dict()
    want = model.trainer().export_state_dict()
    assert set(want) == {k for k in before if k.startswith(MH)}
    assert any(not torch.equal(before[k], after[k]) for k in want)
    for k, v in before.items():
        if k in want:
            assert torch.equal(after[k].float(), want[k].float()), k
        else:
            assert torch.equal(after[k], v), k
    x = torch.randn(4, 256, 14, 14, device="cuda")
    with torch.no_grad():
        prob = model.roi_heads.mask_head.forward_rows(nhwc(x))
        ref = R.mask_head_logits(x.double(), {k: v.double() for k, v in want.items()}).sigmoid()
    assert l2rel(prob, ref) < 1e-4, l2rel(prob, ref)
