"""GPU suite (-m gpu) for the stage-4 training step (configs/step3_planehead.yaml, articulation3d_amd/training_plane.py): the new kernel
(a3d_plane_loss) against float64 autograd of its contract (tests/plane_train_ref.py), the frozen detector against stage 1's step bit
for bit, the whole step against float64 autograd of the reference's plane head on the trainer's own pooled rows, the SGD update,
training progress and the reference-style drop-in call."""
import ctypes as C
import os

import pytest
import torch

import plane_train_ref as R

pytestmark = pytest.mark.gpu

PH = R.PH
SENTINEL = 7.0


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


# ------------------------------------------------------------------------------------------ a3d_plane_loss
def _run_loss(T, case, live, normal_only=True, loss_weight=1.0):
    h, w, b, ri, rg, gt = case
    c = lambda x: x.cuda().contiguous()
    dh = torch.full_like(h, SENTINEL).cuda()
    raw = torch.full((h.shape[0], 3), SENTINEL, device="cuda")
    out = torch.full((3 * h.shape[1] + 4,), SENTINEL, device="cuda")
    T.plane_loss(c(h), c(w), c(b), torch.tensor([live], dtype=torch.int32, device="cuda"), c(ri), c(rg), c(gt), loss_weight=loss_weight,
                 normal_only=normal_only, out=out, dh=dh, raw=raw)
    torch.cuda.synchronize()
    return out.cpu(), dh.cpu(), raw.cpu()


def _check_loss(case, live, got, ref, tag):
    """The issue's tolerances, those tests/test_gpu_mask_training.py holds a3d_mask_loss to: loss 1e-6 relative; dh, dw, db, raw 1e-5 relative L2."""
    out, dh, raw = got
    loss, rdh, rdw, rdb, rraw, _ = ref
    K = case[0].shape[1]
    errs = dict(dh=l2rel(dh[:live], rdh), dw=l2rel(out[:3 * K].view(3, K), rdw), db=l2rel(out[3 * K:3 * K + 3], rdb), raw=l2rel(raw[:live], rraw))
    print(tag, "loss", out[3 * K + 3].item(), loss.item(), {k: f"{v:.2e}" for k, v in errs.items()})
    assert bool(torch.isfinite(out).all())
    assert abs(out[3 * K + 3].item() - loss.item()) <= 1e-6 * abs(loss.item()), (out[3 * K + 3].item(), loss.item())
    for k, e in errs.items():
        assert e < 1e-5, (tag, k, e)
    assert bool((dh[:live][case[0][:live] <= 0] == 0).all())  # the ReLU gate: exactly 0 where the activation is not positive
    assert bool((dh[live:] == SENTINEL).all()) and bool((raw[live:] == SENTINEL).all())  # rows past the live count: untouched


@pytest.mark.parametrize("K,loss_weight", [(1024, 1.0), (256, 0.75)])
def test_plane_loss_matches_float64_autograd(T, K, loss_weight):
    """40 rows, 23 live (more rows than the waves of a workgroup, ragged), the crafted rows of plane_train_ref.loss_case among them."""
    rows, live, c = 40, 23, R.CRAFTED
    case = R.loss_case(K=K, rows=rows, live=live)
    h = case[0]
    assert bool(h[live:].isnan().all()) and 0.03 < (h[:live] == 0).float().mean() and 0.03 < (h[:live] < 0).float().mean()
    ref = R.loss_case_ref(*case, live, loss_weight=loss_weight)
    res = ref[5]
    ordinary = [r for r in range(live) if r not in c.values()]
    assert res[ordinary].abs().min().item() > R.MIN_RESIDUAL  # no sign of an ordinary row hangs on fp32 rounding
    got = _run_loss(T, case, live, loss_weight=loss_weight)
    _check_loss(case, live, got, ref, f"K={K}")
    out, dh, raw = got
    # the crafted rows, exactly
    assert raw[c["eps"]].tolist() == [0.0, 0.0, 0.0] and raw[c["equal"]].tolist() == [0.0, 3.0, 4.0] == raw[c["mirrored"]].tolist()
    for name in ("eps", "equal", "bad_gt", "bad_img"):  # closed gate / sign 0 in every component / no ground truth: a zero dh row
        assert bool((dh[c[name]] == 0).all()), name
    # mirrored: the gradient of the raw vector is tangential, (0, -12, 9) k / 125, and the one open column of the row holds the raw
    # vector itself, (0, 3, 4): the float64 dh row is exactly 0 and the fp32 one a rounding of 36 k / 125 - 36 k / 125 (a few ulp of 0.02)
    assert bool((ref[1][c["mirrored"]] == 0).all()) and dh[c["mirrored"]].abs().max().item() < 1e-7
    assert l2rel(dh[c["zero_gt"]], ref[1][c["zero_gt"]]) < 1e-5 and bool(ref[1][c["zero_gt"]].abs().max() > 0)
    # db is the eps row's 1 / 1e-12 almost alone; dw and dh hold the other rows to the bound (that row's h is 0)
    assert abs(ref[3]).max().item() > 1e9
    got2 = _run_loss(T, case, live, loss_weight=loss_weight)
    assert torch.equal(out, got2[0]) and torch.equal(dh[:live], got2[1][:live]) and torch.equal(raw[:live], got2[2][:live])  # bit-reproducible


@pytest.mark.parametrize("K,crafted,loss_weight", [(1024, True, 1.0), (256, False, 0.75)])
def test_plane_loss_with_more_live_rows_than_waves(T, K, crafted, loss_weight):
    """600 rows, 531 live: the grid has 256 waves, so every wave walks two rows and the first 19 a third, carrying its dw / db / loss
    partials in registers from row to row -- the path of 8 images per GPU.  Out-of-range rows sit in the second pass (261 behind the
    crafted out-of-range row 5, 300 behind an ordinary row) and in the third (517, behind both 5 and 261): such a row must neither
    inherit the gradient of the row before it nor drop the partials gathered so far.  K = 256 runs without the crafted rows and with
    a bias, so its db is not the eps row's alone."""
    rows, live, bad = 600, 531, {261, 300, 517}
    case = R.loss_case(K=K, rows=rows, live=live, crafted=crafted, bad_gt=(300,), bad_img=(261, 517))
    ref = R.loss_case_ref(*case, live, loss_weight=loss_weight)
    special = bad | (set(R.CRAFTED.values()) if crafted else set())
    ordinary = [r for r in range(live) if r not in special]
    assert ref[5][ordinary].abs().min().item() > R.MIN_RESIDUAL and bool(ref[5][sorted(bad)].isnan().all())
    got = _run_loss(T, case, live, loss_weight=loss_weight)
    _check_loss(case, live, got, ref, f"K={K} {live}/{rows}")
    out, dh, raw = got
    for r in sorted(bad):
        assert bool((dh[r] == 0).all()), r
    for r in (5, 260, 262, 299, 301, 516, 518, 530):  # the rows around them, pass by pass, each held on its own
        assert l2rel(raw[r], ref[4][r]) < 1e-5, r
        if r != 5 or not crafted:
            assert l2rel(dh[r], ref[1][r]) < 1e-5 and bool(ref[1][r].abs().max() > 0), r
    got2 = _run_loss(T, case, live, loss_weight=loss_weight)
    assert torch.equal(out, got2[0]) and torch.equal(dh[:live], got2[1][:live]) and torch.equal(raw[:live], got2[2][:live])  # bit-reproducible


def test_plane_loss_normalised_with_bias_and_no_crafted_row(T):
    """23 of 40 rows with a non-zero bias and without the eps row, whose 1 / 1e-12 term is all the crafted case's db holds to its bound:
    here db is the ordinary rows'."""
    rows, live = 40, 23
    case = R.loss_case(rows=rows, live=live, crafted=False)
    ref = R.loss_case_ref(*case, live)
    assert ref[5].abs().min().item() > R.MIN_RESIDUAL and 1e-3 < ref[3].abs().max().item() < 10
    _check_loss(case, live, _run_loss(T, case, live), ref, "no crafted row")


def test_plane_loss_without_normalisation(T):
    rows, live = 40, 23
    case = R.loss_case(rows=rows, live=live)
    ref = R.loss_case_ref(*case, live, normal_only=False)
    ordinary = [r for r in range(live) if r not in R.CRAFTED.values()]
    assert ref[5][ordinary].abs().min().item() > R.MIN_RESIDUAL
    _check_loss(case, live, _run_loss(T, case, live, normal_only=False), ref, "normal_only=0")


def test_plane_loss_without_live_rows_is_zero(T):
    case = R.loss_case(rows=8, live=0, crafted=False)
    out, dh, raw = _run_loss(T, case, 0)
    assert out.tolist() == [0.0] * (3 * 1024 + 4)  # loss 0.0 and dw / db exactly 0 (the reference: plane_pred.sum() * 0)
    assert bool((dh == SENTINEL).all()) and bool((raw == SENTINEL).all())


@pytest.mark.parametrize("rows,live,given", [(5, 5, 5), (3, 1, 1), (5, 5, 9), (5, 0, -3)])
def test_plane_loss_edge_row_counts(T, rows, live, given):
    """live == rows, a single row (all but one wave idle), and a device count outside [0, rows]: clamped."""
    case = R.loss_case(rows=rows, live=live, seed=13, crafted=False)
    ref = R.loss_case_ref(*case, live)
    got = _run_loss(T, case, given)
    if live == 0:
        assert got[0].tolist() == [0.0] * (3 * 1024 + 4) and bool((got[1] == SENTINEL).all())
        return
    assert ref[5].abs().min().item() > R.MIN_RESIDUAL
    _check_loss(case, live, got, ref, f"{live}/{rows} given {given}")


def test_plane_loss_refuses_bad_descriptors_without_a_launch(T):
    from articulation3d_amd import _lib

    def desc(K=1024, rows=4):
        keep = [torch.full((rows, K), SENTINEL, device="cuda"), torch.zeros(3, K, device="cuda"), torch.zeros(3, device="cuda"),
                torch.full((1,), rows, dtype=torch.int32, device="cuda"), torch.zeros(rows, dtype=torch.int32, device="cuda"),
                torch.zeros(rows, dtype=torch.int32, device="cuda"), torch.ones(1, 2, 3, device="cuda"),
                torch.empty(max(4, _lib.lib().a3d_plane_loss_workspace_bytes(1024) // 4), device="cuda"),
                torch.full((3 * K + 4,), SENTINEL, device="cuda"), torch.full((rows, K), SENTINEL, device="cuda")]
        d = _lib.PlaneLossDesc()
        for name, t in zip(("h", "w", "b", "live", "row_img", "row_gt", "gt_planes", "workspace", "out", "dh"), keep):
            setattr(d, name, t.data_ptr())
        d.rows, d.K, d.B, d.max_gt, d.loss_weight, d.normal_only = rows, K, 1, 2, 1.0, 1
        return d, keep

    call = lambda d: _lib.lib().a3d_plane_loss(C.byref(d), torch.cuda.current_stream().cuda_stream)
    assert _lib.lib().a3d_plane_loss(None, None) == -1
    bad = [("h", None), ("w", None), ("b", None), ("live", None), ("row_img", None), ("row_gt", None), ("gt_planes", None),
           ("workspace", None), ("out", None), ("dh", None), ("K", 1000), ("K", 0), ("K", -256), ("rows", -1), ("B", 0), ("max_gt", 0)]
    for field, value in bad:
        d, keep = desc()
        setattr(d, field, value)
        assert call(d) == -1, field
        torch.cuda.synchronize()
        assert bool((keep[8] == SENTINEL).all()) and bool((keep[9] == SENTINEL).all()), field  # nothing ran
    assert _lib.lib().a3d_plane_loss_workspace_bytes(1000) == 0 and _lib.lib().a3d_plane_loss_workspace_bytes(256) > 0
    d, keep = desc()
    assert call(d) == 0  # (and the descriptor these were made from is a good one)
    torch.cuda.synchronize()
    # zero weights: every prediction is 0 against the unit vector (1, 1, 1) / sqrt(3)
    assert abs(keep[8][-1].item() - 3 ** 0.5) < 1e-5 and bool((keep[8] != SENTINEL).all()) and bool((keep[9] == 0).all())


# ------------------------------------------------------------------------------------------ the step
@pytest.fixture(scope="module")
def batch(oracle):
    from oracle import train_oracle as TO

    frames = torch.from_numpy(oracle.synthetic_frames(2)).cuda()
    tg = TO.synthetic_targets(2)
    g = torch.Generator().manual_seed(17)
    planes = []
    for t in tg:  # random non-zero plane parameters (normal x offset), one row per ground-truth box
        n = torch.randn(len(t[0]), 3, generator=g)
        planes.append(n / n.norm(dim=1, keepdim=True) * (0.5 + 3 * torch.rand(len(t[0]), 1, generator=g)))
    return frames, [t[0] for t in tg], [t[1] for t in tg], planes


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_frozen_forward_is_stage_ones_forward_bit_for_bit(hip_model, batch, precision):
    from articulation3d_amd.training import DetectorTrainer
    from articulation3d_amd.training_plane import PlaneTrainer

    frames, gb, gc, gp = batch
    t1 = DetectorTrainer(hip_model, seed=13, precision=precision)
    l1, a1 = t1.forward_backward(frames, gb, gc)
    t2 = PlaneTrainer(hip_model, seed=13, precision=precision)
    l2, a2 = t2.forward_backward(frames, gb, gc, gp)
    torch.cuda.synchronize()
    assert set(l2) == {"loss_cls", "loss_box_reg", "loss_plane"}
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
def test_plane_step_matches_float64_autograd(hip_model, oracle, batch, precision, shuffled):
    """shuffled: the samples= hook with the drawn ROI index sets in a random order (foreground rows scattered among the background)."""
    from articulation3d_amd.training import lr_at
    from articulation3d_amd.training_plane import PlaneTrainer

    frames, gb, gc, gp = batch
    tr = PlaneTrainer(hip_model, seed=21, precision=precision)
    p0 = {k: v.clone() for k, v in tr.export_state_dict().items()}
    samples = None
    if shuffled:
        _, a0 = PlaneTrainer(hip_model, seed=21, precision=precision).forward_backward(frames, gb, gc, gp)
        rc, ri = a0["roi_count"].cpu(), a0["roi_index"].cpu()
        g = torch.Generator().manual_seed(4)
        sets = [ri[i, : int(rc[i])].long() for i in range(frames.shape[0])]
        samples = dict(roi_idx=[s_[torch.randperm(len(s_), generator=g)] for s_ in sets])
        del a0
    model_before = {k: v.clone() for k, v in hip_model.state_dict().items()}
    losses, aux = tr.forward_backward(frames, gb, gc, gp, samples=samples)
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
    assert fg["row_img"][:live].cpu().tolist() == [r[0] for r in rows] and fg["row_gt"][:live].cpu().tolist() == [r[2] for r in rows]
    # the pooled rows: the oracle's pooler with the plane pooler's own settings on the trainer's pyramid
    pp = hip_model.roi_heads.plane_pooler
    assert (tr.pool_size, tr.pool_ratio, tr.pool_aligned) == (pp.output_size, pp.sampling_ratio, pp.aligned) and tr.pool_size == 14
    feats = {n: aux["feats"][n].permute(0, 3, 1, 2).cpu() for n in ("p2", "p3", "p4", "p5")}
    boxes = [aux["roi_boxes"][b].cpu()[[r[1] for r in rows if r[0] == b]] for b in range(B)]
    pooled_ref = oracle.roi_pool_fpn(feats, boxes, pp.output_size, pp.sampling_ratio, pp.aligned)
    pooled = aux["pooled"][:live].permute(0, 3, 1, 2).cpu()
    assert l2rel(pooled, pooled_ref) < 1e-6
    # the ground truth the kernel read, and the rows' matched vectors
    assert tuple(aux["gt_planes"].shape[::2]) == (B, 3)
    for b in range(B):
        assert torch.equal(aux["gt_planes"][b, : len(gp[b])].cpu(), gp[b])
    gt_rows = torch.stack([gp[b][g_] for b, _, g_ in rows])
    # float64 autograd of the reference's plane head + plane_rcnn_loss on the trainer's own pooled rows
    ph = hip_model.roi_heads.plane_head
    P = {k: v.double().requires_grad_(True) for k, v in p0.items()}
    x64 = pooled.cuda().double()
    # (the ReLU gates within GATE_MARGIN of a kink follow the trainer's own forward pass: plane_train_ref.plane_head_raw)
    acts = tr._tower_forward(tr.convs, aux["pooled"], (fg["live"] * tr.pool_size ** 2).to(torch.int32))
    gates, ties = [a[:live].permute(0, 3, 1, 2) > 0 for a in acts[1:]], []
    want = R.plane_loss_ref(x64, P, gt_rows.cuda(), loss_weight=ph._loss_weight, normal_only=ph._plane_normal_only, gates=gates, ties=ties)
    want.backward()
    print("reference gates within", R.GATE_MARGIN, "of 0 per layer:", ties, "of", gates[0].numel())
    assert len(ties) == 4 and sum(ties) <= R.GATE_FRACTION * 4 * gates[0].numel(), ties
    got = losses["loss_plane"]
    assert abs(got.item() - want.item()) <= (1e-5 if precision != "bf16" else 2e-2) * abs(want.item()), (got.item(), want.item())
    with torch.no_grad():
        raw_err = l2rel(aux["raw_plane"][:live], R.plane_head_raw(x64, P, gates))
    g = tr.export_grads()
    assert set(g) == set(P) and len(g) == 12 and sum(v.numel() for v in p0.values()) == 4 * (256 * 256 * 9 + 256) + 1024 * 50176 + 1024 + 3 * 1024 + 3
    assert g[PH + "plane_fc1.weight"].shape == (1024, 50176) and g[PH + "param_pred.weight"].shape == (3, 1024) and g[PH + "param_pred.bias"].shape == (3,)
    assert all(g[PH + f"plane_conv{k}.weight"].shape == (256, 256, 3, 3) for k in range(1, 5))
    errs = {k: l2rel(g[k], P[k].grad) for k in g}
    print(precision, "loss_plane", got.item(), want.item(), "raw", f"{raw_err:.2e}", "relative L2 gradient errors:",
          {k[len(PH):]: f"{v:.2e}" for k, v in errs.items()})
    bound = 2e-4 if precision != "bf16" else 5e-2
    assert raw_err < bound
    for k, e in errs.items():
        assert e < bound, (k, e)
    # ... and free-running, every gate the float64 head's own, as tests/test_gpu_training.py holds stage 1: one gate of 351 232 on the
    # other side of a kink moves every gradient below it by about 1 / sqrt(active units) ~ 2e-3, so this bound is that test's 5e-2
    Pf = {k: v.double().requires_grad_(True) for k, v in p0.items()}
    free = R.plane_loss_ref(x64, Pf, gt_rows.cuda(), loss_weight=ph._loss_weight, normal_only=ph._plane_normal_only)
    free.backward()
    flips = [int((gk != (a > 0)).sum()) for gk, a in zip(gates, R.plane_head_acts(x64, Pf))]
    errs_free = {k: l2rel(g[k], Pf[k].grad) for k in g}
    print(precision, "free-running: gates that differ per layer", flips, "loss", free.item(), "worst gradient error", max(errs_free.values()),
          {k[len(PH):]: f"{v:.2e}" for k, v in errs_free.items()})
    assert abs(got.item() - free.item()) <= (1e-5 if precision != "bf16" else 2e-2) * abs(free.item())
    assert sum(flips) <= sum(ties)  # (a gate differs only where the reference stands within the margin of a kink)
    for k, e in errs_free.items():
        assert e < 5e-2, (k, e)
    if sum(flips) == 0:  # no gate differs: the borrowed gates changed nothing and the free-running reference holds the tight bound too
        assert all(e < bound for e in errs_free.values()), errs_free
    del Pf
    # update: the float64 SGD formula on the plane parameters
    tr.optimizer_step()
    s = tr.s
    lr0 = lr_at(0, s)
    p1 = tr.export_state_dict()
    for k in p0:
        d = g[k].double() + s.weight_decay * p0[k].double()
        want_p = p0[k].double() - lr0 * d  # first step: the momentum buffer starts as the gradient
        assert l2rel(p1[k], want_p) < 1e-6, k
    assert any(not torch.equal(p0[k], p1[k]) for k in p0)
    # every parameter and buffer of the model outside the plane head, after the step and after the write-back of leaving training mode
    assert all(torch.equal(v, hip_model.state_dict()[k]) for k, v in model_before.items())
    try:
        hip_model.train()
        hip_model._trainer = tr
        hip_model.train(False)
        after = hip_model.state_dict()
        for k, v in model_before.items():
            if k.startswith(PH):
                assert torch.equal(after[k].float(), p1[k].float()), k  # (the trained plane head reaches the model)
            else:
                assert torch.equal(after[k], v), k
        # the inference forward of the updated head
        x = torch.randn(5, 256, 14, 14, device="cuda")
        with torch.no_grad():
            normals = ph.forward_rows(nhwc(x))
            ref = R.plane_head_forward(x.double(), {k: v.double() for k, v in p1.items()}, ph._plane_normal_only)
        assert normals.shape == (5, 3) and l2rel(normals, ref) < 1e-4, l2rel(normals, ref)
    finally:  # (the session-scoped model goes back to the state the other tests expect, whatever failed above)
        hip_model.__dict__.pop("_trainer", None)
        hip_model.train(False)
        hip_model.load_state_dict(model_before)


def test_plane_loss_decreases_on_a_fixed_batch(hip_model, batch):
    from articulation3d_amd.training import SolverCfg
    from articulation3d_amd.training_plane import PlaneTrainer

    frames, gb, gc, gp = batch
    tr = PlaneTrainer(hip_model, SolverCfg(base_lr=0.02, warmup_iters=0), seed=3)
    hist = []
    for _ in range(8):
        l, _ = tr.step(frames, gb, gc, gp)
        hist.append(l["loss_plane"])
    hist = torch.stack(hist).cpu()
    print("loss_plane over 8 steps:", hist.tolist())
    assert bool(torch.isfinite(hist).all()) and hist[-1] < hist[0], hist.tolist()


def test_reference_training_loop_is_a_drop_in_for_the_plane_stage(oracle, oracle_params, batch):
    """model.train(); losses = model(data); sum(losses.values()).backward(); build_optimizer(cfg, model).step(); model.eval(): the
    trained plane weights reach inference."""
    from conftest import ROOT
    from articulation3d_amd.config import get_cfg, get_planercnn_cfg_defaults
    from articulation3d_amd.engine import build_optimizer
    from articulation3d_amd.modeling import build_model
    from articulation3d_amd.structures import Boxes, Instances
    from articulation3d_amd.training_plane import PlaneTrainer

    cfg = get_cfg()
    get_planercnn_cfg_defaults(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "step3_planehead.yaml"))
    cfg.MODEL.DEVICE = "cuda"
    model = build_model(cfg)
    missing, unexpected = model.load_state_dict(oracle_params, strict=False)
    assert not unexpected and all("num_batches_tracked" in k for k in missing)
    assert model.training_stage() == 4
    frames, gb, gc, gp = batch
    data = []
    for i in range(frames.shape[0]):
        inst = Instances((480, 640), gt_boxes=Boxes(gb[i].cuda()), gt_classes=gc[i].cuda(), gt_planes=gp[i].cuda())
        data.append({"image": frames[i].permute(2, 0, 1).cpu(), "instances": inst})
    model.train()
    losses = model(data)
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_plane"}
    sum(losses.values()).backward()
    optimizer = build_optimizer(cfg, model)
    assert isinstance(model.trainer(), PlaneTrainer)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    optimizer.step()
    model.eval()
    after = model.state_dict()
    want = model.trainer().export_state_dict()
    assert set(want) == {k for k in before if k.startswith(PH)}
    assert any(not torch.equal(before[k], after[k]) for k in want)
    for k, v in before.items():
        if k in want:
            assert torch.equal(after[k].float(), want[k].float()), k
        else:
            assert torch.equal(after[k], v), k
    x = torch.randn(4, 256, 14, 14, device="cuda")
    with torch.no_grad():
        normals = model.roi_heads.plane_head.forward_rows(nhwc(x))
        ref = R.plane_head_forward(x.double(), {k: v.double() for k, v in want.items()})
    assert l2rel(normals, ref) < 1e-4, l2rel(normals, ref)
