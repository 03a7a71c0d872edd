"""GPU suite (-m gpu) for the stage-2 training step (config/step2_axis.yaml, articulation3d_amd/training_axis.py): the new kernels
(a3d_axis_loss, the live-count weight gradient a3d_wgrad_desc.p_dev, a3d_colsum_rows) against float64 restatements, the frozen
detector against stage 1's step bit for bit, the whole step against float64 autograd of the reference's axis head on the trainer's
own pooled rows, the SGD update, training progress, the tower stream and the reference-style drop-in call."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from test_axis_training_host import axis_loss_ref

pytestmark = pytest.mark.gpu

AH = "roi_heads.axis_head."


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


# ------------------------------------------------------------------------------------------ a3d_axis_loss
def _loss_case(rows, live, B, G, seed, valid_p=0.6):
    g = torch.Generator().manual_seed(seed)
    raw_rot = torch.randn(rows, 3, generator=g)
    raw_tran = torch.randn(rows, 2, generator=g)
    row_img = torch.randint(0, B, (rows,), generator=g, dtype=torch.int32)
    row_gt = torch.randint(0, G, (rows,), generator=g, dtype=torch.int32)
    ang = torch.rand(B, G, 2, generator=g) * 2 * math.pi
    gr = torch.stack((ang[..., 0].sin(), ang[..., 0].cos(), torch.randn(B, G, generator=g), (torch.rand(B, G, generator=g) < valid_p).float()), -1)
    gt = torch.stack((ang[..., 1].sin(), ang[..., 1].cos(), torch.zeros(B, G), (torch.rand(B, G, generator=g) < valid_p).float()), -1)
    raw_rot[live:] = float("nan")  # dead rows: must never be read
    raw_tran[live:] = float("nan")
    return raw_rot, raw_tran, row_img, row_gt, gr, gt


def _run_loss(T, case, live, beta, w=1.0):
    raw_rot, raw_tran, row_img, row_gt, gr, gt = case
    c = lambda t: t.cuda().contiguous()
    lv = torch.tensor([live], dtype=torch.int32, device="cuda")
    loss, dr, dt = T.axis_loss(c(raw_rot), c(raw_tran), lv, c(row_img), c(row_gt), c(gr), c(gt), beta=beta, loss_weight=w)
    return loss.cpu(), dr.cpu(), dt.cpu()


def _ref_loss(case, live, beta, w=1.0):
    raw_rot, raw_tran, row_img, row_gt, gr, gt = case
    rr = raw_rot[:live].double().requires_grad_(True)
    rt = raw_tran[:live].double().requires_grad_(True)
    gsel = lambda a: a[row_img[:live].long(), row_gt[:live].long()].double()
    lr, lt = axis_loss_ref(rr, rt, gsel(gr), gsel(gt), beta=beta, loss_weight=w)
    (lr + lt).backward()
    return lr.detach(), lt.detach(), rr.grad, rt.grad


@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_axis_loss_matches_float64_autograd(T, beta):
    rows, live = 300, 233
    case = _loss_case(rows, live, B=4, G=5, seed=3)
    b7, g7 = case[2][7].long(), case[3][7].long()
    case[4][b7, g7] = torch.tensor([0.0, 1.0, 0.25, 1.0])  # an exact tie: (0, 2) normalises to (0, 1) in any precision
    case[0][7] = torch.tensor([0.0, 2.0, 0.25])
    case[0][9, :2] = 1e-14  # raw vectors with a norm below F.normalize's eps (gradients ~1 / eps: compared on their own)
    case[1][11] = 3e-15
    loss, dr, dt = _run_loss(T, case, live, beta, w=1.5)
    lr, lt, gr, gt = _ref_loss(case, live, beta, w=1.5)
    assert abs(loss[0].item() - lr.item()) <= 1e-6 * abs(lr.item()), (loss, lr)
    assert abs(loss[1].item() - lt.item()) <= 1e-6 * abs(lt.item()), (loss, lt)
    rest = torch.tensor([r not in (9, 11) for r in range(live)])
    errs = [l2rel(dr[:live][rest], gr[rest]), l2rel(dt[:live][rest], gt[rest]), l2rel(dr[9], gr[9]), l2rel(dt[11], gt[11])]
    assert max(errs) < 1e-6, errs
    assert torch.equal(dr[live:], torch.zeros_like(dr[live:])) and torch.equal(dt[live:], torch.zeros_like(dt[live:]))
    assert bool(torch.isfinite(dr).all() and torch.isfinite(dt).all())
    if beta == 0.0:
        assert torch.equal(dr[7, 2], torch.tensor(0.0))  # |x| at exactly 0: zero subgradient
    loss2, dr2, dt2 = _run_loss(T, case, live, beta, w=1.5)  # bit-reproducible
    assert torch.equal(loss, loss2) and torch.equal(dr, dr2) and torch.equal(dt, dt2)


def test_axis_loss_edge_cases(T):
    case = _loss_case(64, 40, B=3, G=4, seed=5, valid_p=0.0)  # no valid row at all
    loss, dr, dt = _run_loss(T, case, 40, 0.0)
    assert loss.tolist() == [0.0, 0.0] and not dr.any() and not dt.any()
    loss, dr, dt = _run_loss(T, case, 0, 0.0)  # no foreground row (no ground truth): 0, every gradient exactly 0
    assert loss.tolist() == [0.0, 0.0] and not dr.any() and not dt.any()
    case = _loss_case(64, 40, B=3, G=4, seed=6)
    case[2][:] = torch.where(case[2] == 2, torch.zeros_like(case[2]), case[2])  # image 2 has no rows (no GT)
    loss, dr, dt = _run_loss(T, case, 40, 0.0)
    lr, lt, gr, gt = _ref_loss(case, 40, 0.0)
    assert abs(loss[0].item() - lr.item()) <= 1e-6 * abs(lr.item()) and l2rel(dr[:40], gr) < 1e-6 and l2rel(dt[:40], gt) < 1e-6


# ------------------------------------------------------------------------------------------ live-count weight / bias gradients
WG_LIVE = [dict(B=10, H=14, W=14, Cin=256, Cout=256, k=3, s=1, p=1, live=4),  # the axis towers' 3x3 convs on 14x14 ROI maps
           dict(B=96, H=1, W=1, Cin=256 * 196, Cout=1024, k=1, s=1, p=0, live=37),  # the 50176 -> 1024 FC
           dict(B=10, H=14, W=14, Cin=128, Cout=128, k=3, s=2, p=1, live=3)]  # stride 2: the first bf16 form (not the transposed read)


@pytest.mark.parametrize("prec", [0, 1, 2], ids=["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("c", WG_LIVE, ids=["3x3_14x14", "fc50176", "3x3s2"])
def test_wgrad_live_count(T, c, prec):
    torch.manual_seed(7)
    B, H, W, Cin, Cout, k, st, p, live = c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["k"], c["s"], c["p"], c["live"]
    Ho, Wo = (H + 2 * p - k) // st + 1, (W + 2 * p - k) // st + 1
    x = torch.randn(B, H, W, Cin, device="cuda")
    dy = torch.randn(B, Ho, Wo, Cout, device="cuda")
    full = torch.tensor([B * Ho * Wo], dtype=torch.int32, device="cuda")
    part = torch.tensor([live * Ho * Wo], dtype=torch.int32, device="cuda")
    dw0 = torch.empty(Cout, k * k * Cin, device="cuda")
    dw1 = torch.empty_like(dw0)
    T.conv_wgrad(x, dy, dw0, KH=k, KW=k, stride=st, pad=p, precision=prec)
    T.conv_wgrad(x, dy, dw1, KH=k, KW=k, stride=st, pad=p, precision=prec, p_dev=full)
    assert torch.equal(dw0, dw1)  # the full count: the NULL bits
    xn, dyn = x.clone(), dy.clone()
    xn[live:] = float("nan")
    dyn[live:] = float("nan")
    dw2 = torch.empty_like(dw0)
    T.conv_wgrad(xn, dyn, dw2, KH=k, KW=k, stride=st, pad=p, precision=prec, p_dev=part)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dw2).all())
    xr, dr = x[:live].double().cpu(), dy[:live].double().cpu()
    if prec == 1:  # bf16 arithmetic: float64 of the bf16-rounded operands
        xr, dr = x[:live].bfloat16().double().cpu(), dy[:live].bfloat16().double().cpu()
    wd = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr.permute(0, 3, 1, 2), wd, None, st, p).backward(dr.permute(0, 3, 1, 2))
    ref = wd.grad.permute(0, 2, 3, 1).reshape(Cout, -1)
    bound = 2e-6 if prec == 1 else 1e-5
    assert l2rel(dw2, ref) < bound, l2rel(dw2, ref)
    # deferred slice reduction: the bits of the per-launch reduce
    defer = T.DeferredReduces(torch.device("cuda"))
    dw3 = torch.empty_like(dw0)
    T.conv_wgrad(xn, dyn, dw3, KH=k, KW=k, stride=st, pad=p, precision=prec, p_dev=part, defer=defer)
    defer.flush()
    assert torch.equal(dw2, dw3)
    # bias gradient over the live rows
    M = B * Ho * Wo
    db0, db1, db2 = (torch.empty(Cout, device="cuda") for _ in range(3))
    T.colsum(dy, db0)
    T.colsum_rows(dy, db1, full)
    assert torch.equal(db0, db1)
    dyn = dy.clone()
    dyn[live:] = float("nan")
    T.colsum_rows(dyn, db2, part)
    assert l2rel(db2, dy[:live].double().sum((0, 1, 2))) < 1e-6
    db3 = torch.empty_like(db2)
    T.colsum_rows(dyn.bfloat16(), db3, part)
    assert l2rel(db3, dy[:live].bfloat16().double().sum((0, 1, 2))) < 1e-6
    assert M == dy.numel() // Cout


# ------------------------------------------------------------------------------------------ the step
def _axis_targets(tg, seed):
    g = torch.Generator().manual_seed(seed)
    rot, tran = [], []
    for b, _c in tg:
        n = len(b)
        a = torch.rand(n, 2, generator=g) * 2 * math.pi
        v = (torch.arange(n) % 3 != 2).float()  # every third GT without a valid axis
        rot.append(torch.stack((a[:, 0].sin(), a[:, 0].cos(), torch.randn(n, generator=g), v), 1))
        tran.append(torch.stack((a[:, 1].sin(), a[:, 1].cos(), torch.zeros(n), 1.0 - v * (torch.arange(n) % 2 == 1).float()), 1))
    return rot, tran


@pytest.fixture(scope="module")
def batch(oracle):
    from oracle import train_oracle as TO

    frames = torch.from_numpy(oracle.synthetic_frames(2)).cuda()
    tg = TO.synthetic_targets(2)
    rot, tran = _axis_targets(tg, 9)
    return frames, [t[0] for t in tg], [t[1] for t in tg], rot, tran


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_frozen_forward_is_stage_ones_forward_bit_for_bit(hip_model, batch, precision):
    from articulation3d_amd.training import DetectorTrainer
    from articulation3d_amd.training_axis import AxisTrainer

    frames, gb, gc, rot, tran = batch
    t1 = DetectorTrainer(hip_model, seed=13, precision=precision)
    l1, a1 = t1.forward_backward(frames, gb, gc)
    t2 = AxisTrainer(hip_model, seed=13, precision=precision)
    l2, a2 = t2.forward_backward(frames, gb, gc, rot, tran)
    torch.cuda.synchronize()
    assert set(l2) == {"loss_cls", "loss_box_reg", "loss_rot_axis", "loss_tran_axis"}
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
def test_axis_step_matches_float64_autograd(hip_model, oracle, batch, precision, shuffled):
    """shuffled: the samples= hook with the drawn ROI index sets in a random order (foreground rows scattered among the background)."""
    from articulation3d_amd.training_axis import AxisTrainer

    frames, gb, gc, rot, tran = batch
    tr = AxisTrainer(hip_model, seed=21, precision=precision)
    p0 = {k: v.clone() for k, v in tr.export_state_dict().items()}
    samples = None
    if shuffled:
        _, a0 = AxisTrainer(hip_model, seed=21, precision=precision).forward_backward(frames, gb, gc, rot, tran)
        rc, ri = a0["roi_count"].cpu(), a0["roi_index"].cpu()
        g = torch.Generator().manual_seed(4)
        sets = [ri[i, : int(rc[i])].long() for i in range(frames.shape[0])]
        samples = dict(roi_idx=[s_[torch.randperm(len(s_), generator=g)] for s_ in sets])
        del a0
    model_before = {k: v.clone() for k, v in hip_model.state_dict().items()}
    losses, aux = tr.forward_backward(frames, gb, gc, rot, tran, samples=samples)
    torch.cuda.synchronize()
    B = frames.shape[0]
    if shuffled:
        for i in range(B):
            assert torch.equal(aux["roi_index"][i, : len(samples["roi_idx"][i])].cpu().long(), samples["roi_idx"][i])
        cls = aux["roi_cls"].cpu()
        first_bg = [(cls[i, : int(aux["roi_count"][i])] == tr.s.num_classes).nonzero() for i in range(B)]
        assert any(len(f) and bool((cls[i, int(f[0]):int(aux["roi_count"][i])] < tr.s.num_classes).any()) for i, f in enumerate(first_bg)), \
            "the shuffled order should put foreground rows behind background ones"
    fg = aux["fg"]
    rows = _fg_restated(aux, tr.s, B)
    live = int(fg["live"])
    assert live == len(rows) > 0
    assert fg["count"].cpu().tolist() == [sum(1 for r in rows if r[0] == b) for b in range(B)]
    assert fg["row_img"][:live].cpu().tolist() == [r[0] for r in rows] and fg["row_gt"][:live].cpu().tolist() == [r[2] for r in rows]
    # the pooled rows: the oracle's non-aligned ROIAlign of the same proposal boxes on the trainer's pyramid
    feats = {n: aux["feats"][n].permute(0, 3, 1, 2).cpu() for n in ("p2", "p3", "p4", "p5")}
    boxes = [aux["roi_boxes"][b].cpu()[[r[1] for r in rows if r[0] == b]] for b in range(B)]
    pooled_ref = oracle.roi_pool_fpn(feats, boxes, 14, 0, False)
    pooled = aux["pooled"][:live].permute(0, 3, 1, 2).cpu()
    assert l2rel(pooled, pooled_ref) < 1e-6
    # float64 autograd of the reference's axis head + axis loss on the trainer's own pooled rows
    P = {k: v.double().requires_grad_(True) for k, v in p0.items()}
    _, _, raw_rot, raw_tran = oracle.axis_head(pooled.cuda().double(), P, return_raw=True)
    gsel = lambda lst: torch.stack([lst[b][g] for b, _, g in rows]).double().cuda()
    lr, lt = axis_loss_ref(raw_rot, raw_tran, gsel(rot), gsel(tran), beta=tr.beta, loss_weight=tr.loss_weight)
    (lr + lt).backward()
    for got, want in ((losses["loss_rot_axis"], lr), (losses["loss_tran_axis"], lt)):
        assert abs(got.item() - want.item()) <= (1e-5 if precision != "bf16" else 2e-2) * abs(want.item()), (got.item(), want.item())
    g = tr.export_grads()
    assert set(g) == set(P) and len(g) == 26 and sum(v.numel() for v in p0.values()) == 107_488_261
    errs = {k: l2rel(g[k], P[k].grad) for k in g}
    print(precision, "worst relative L2 gradient error:", max((v, k) for k, v in errs.items()))
    bound = 2e-4 if precision != "bf16" else 5e-2
    for k, e in errs.items():
        assert e < bound, (k, e)
    # update: the float64 SGD formula on the axis parameters; every other parameter of the model untouched
    tr.optimizer_step()
    s = tr.s
    from articulation3d_amd.training import lr_at

    lr0 = lr_at(0, s)
    p1 = tr.export_state_dict()
    for k in p0:
        d = g[k].double() + s.weight_decay * p0[k].double()
        want = p0[k].double() - lr0 * d  # first step: the momentum buffer starts as the gradient
        assert l2rel(p1[k], want) < 1e-6, k
    # every parameter and buffer of the model outside the axis head, after the step and after the write-back of leaving training mode
    hip_model.train()
    hip_model._trainer = tr
    hip_model.train(False)
    del hip_model._trainer
    after = hip_model.state_dict()
    for k, v in model_before.items():
        if k.startswith(AH):
            assert torch.equal(after[k].float(), p1[k].float()), k  # (the trained axis head reaches the model)
        else:
            assert torch.equal(after[k], v), k
    hip_model.load_state_dict(model_before)  # (the module-scoped model goes back to the weights the other tests expect)


def test_axis_losses_decrease_on_a_fixed_batch(hip_model, batch):
    from articulation3d_amd.training import SolverCfg
    from articulation3d_amd.training_axis import AxisTrainer

    frames, gb, gc, rot, tran = batch
    tr = AxisTrainer(hip_model, SolverCfg(base_lr=0.001, warmup_iters=0), seed=3)
    hist = []
    for _ in range(30):
        l, _ = tr.step(frames, gb, gc, rot, tran)
        hist.append(torch.stack([l["loss_rot_axis"], l["loss_tran_axis"]]))
    hist = torch.stack(hist).cpu()
    assert bool(torch.isfinite(hist).all())
    first, last = hist[:5].mean(0), hist[-5:].mean(0)
    print("axis losses first / last 5 steps:", first.tolist(), last.tolist(), "ratio", (last / first).tolist())
    # rotation | offset: stage 1's rule (measured ratio 0.03).  Translation: an L1 of the double angle, whose gradient has a fixed size
    # per row -- it falls steadily but slowly (measured ratio 0.80 after 30 steps at learning rates 5e-4 .. 5e-3), so it is held to a fall
    assert last[0] < 0.6 * first[0] and last[1] < 0.9 * first[1], hist.tolist()


def test_tower_stream_keeps_every_bit_of_the_serial_step(hip_model, batch):
    from articulation3d_amd.training_axis import AxisTrainer

    frames, gb, gc, rot, tran = batch
    out = []
    for serial in (False, True):
        tr = AxisTrainer(hip_model, seed=8)
        if serial:
            tr._t_stream = None
        l, _ = tr.step(frames, gb, gc, rot, tran)
        out.append(({k: v.clone() for k, v in l.items()}, tr.grads.clone(), tr.params.clone()))
    assert all(torch.equal(out[0][0][k], out[1][0][k]) for k in out[0][0])
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])


def test_reference_training_loop_is_a_drop_in_for_step2(oracle, oracle_params, batch):
    """model.train(); losses = model(data); sum(losses.values()).backward(); build_optimizer(cfg, model).step(); model.eval(): the
    trained axis weights reach inference."""
    from conftest import ROOT
    from articulation3d_amd.config import get_cfg, get_planercnn_cfg_defaults
    from articulation3d_amd.engine import build_optimizer
    from articulation3d_amd.modeling import build_model
    from articulation3d_amd.structures import Boxes, Instances

    cfg = get_cfg()
    get_planercnn_cfg_defaults(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "step2_axis.yaml"))
    cfg.MODEL.DEVICE = "cuda"
    model = build_model(cfg)
    sd = {k: v for k, v in oracle_params.items() if not k.startswith(("roi_heads.mask", "roi_heads.plane", "depth_head"))}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("num_batches_tracked" in k for k in missing)
    frames, gb, gc, rot, tran = batch
    data = []
    for i in range(frames.shape[0]):
        inst = Instances((480, 640))
        inst.gt_boxes, inst.gt_classes = Boxes(gb[i].cuda()), gc[i].cuda()
        inst.gt_rot_axis, inst.gt_tran_axis = rot[i].cuda(), tran[i].cuda()
        data.append({"image": frames[i].permute(2, 0, 1).cpu(), "instances": inst})
    model.train()
    losses = model(data)
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_rot_axis", "loss_tran_axis"}
    sum(losses.values()).backward()
    optimizer = build_optimizer(cfg, model)
    before = {k: v.clone() for k, v in model.state_dict().items() if k.startswith(AH)}
    optimizer.step()
    model.eval()
    after = {k: v for k, v in model.state_dict().items() if k.startswith(AH)}
    assert any(not torch.equal(before[k], after[k]) for k in before)
    want = model.trainer().export_state_dict()
    for k, v in want.items():
        assert torch.equal(after[k].float(), v.float()), k
    # inference with the trained axis weights: the axis head on a few rows against a float64 forward of the exported weights
    x = torch.randn(6, 256, 14, 14, device="cuda")
    with torch.no_grad():
        r, t = model.roi_heads.axis_head.forward_rows(nhwc(x))
        r64, t64 = oracle.axis_head(x.double(), {k: v.double() for k, v in want.items()})
    assert l2rel(r, r64) < 1e-4 and l2rel(t, t64) < 1e-4, (l2rel(r, r64), l2rel(t, t64))


def test_axis_gradient_segments_equal_the_monolithic_allreduce_two_gloo_ranks():
    """Two ranks (gloo: both on this box's one GPU, different batches): the stage-2 step's exchange in two segments -- the T tower's announced
    from the side stream it ran on, the R tower's from the main stream -- against ONE all-reduce behind the backward pass: parameters,
    momenta, losses and export_grads() after three steps bit-identical for both payloads, and export_grads() at world 2 the mean of the
    two ranks' own gradients."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "tools/train_axis_exchange_check.py", "--steps", "3"], cwd=root, env=env, capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["world"] == 2
    for payload in ("fp32", "bf16"):
        res = d["result"][payload]
        assert res["params_equal"] and res["momentum_equal"] and res["losses_equal"] and res["export_grads_equal"] and res["finite"], (payload, res)
        assert res["segments_per_step"] == [2, 0], res
    fp = d["result"]["fp32"]
    assert fp["ranks_differ"] and fp["export_vs_mean_rel"] < 1e-6, fp
