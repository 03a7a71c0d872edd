"""GPU suite (-m gpu) for the stage-5 training step (configs/step3_depth.yaml, articulation3d_amd/training_depth.py): the kernels of
csrc/depth_train.hip against float64 torch (tests/depth_train_ref.py), the decoder on a small random pyramid and the whole step on two
480 x 640 frames against float64 autograd of the reference's depth head, the frozen detector against stage 1's step bit for bit, the
two-range SGD update, the running statistics, training progress and the reference-style drop-in call."""
import ctypes as C
import os

import pytest
import torch

import depth_train_ref as R

pytestmark = pytest.mark.gpu

DH = R.DH
ACT = {True: 2, False: 1}  # leaky -> A3D_ACT_LEAKY, else A3D_ACT_RELU
BN_SHAPES = [(2, 5, 7, 64), (1, 3, 4, 128), (2, 60, 80, 128)]  # 70 rows; fewer rows than a wave holds; 9600 rows: many workgroups' partials


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


@pytest.fixture(scope="module")
def bn_refs():
    """The float64 reference of every (shape, activation) BN case, computed once."""
    cache = {}

    def get(shape, leaky):
        if (shape, leaky) not in cache:
            case = R.bn_case(shape)
            cache[(shape, leaky)] = (case, R.bn_ref(*case[:5], leaky, case[5]))
        return cache[(shape, leaky)]

    return get


# ------------------------------------------------------------------------------------------ a3d_bn_train_forward / backward
@pytest.mark.parametrize("leaky", [True, False], ids=["leaky", "relu"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_forward_against_float64(T, bn_refs, shape, leaky):
    (z, gamma, beta, rm, rv, _), ref = bn_refs(shape, leaky)
    c = lambda t: t.cuda().contiguous()
    rmd, rvd = c(rm), c(rv)
    y, mean, invstd, var = T.bn_train_forward(c(z), c(gamma), c(beta), act=ACT[leaky], running_mean=rmd, running_var=rvd)
    torch.cuda.synchronize()
    std = ref["var"].sqrt()
    var_err = ((var.double().cpu() - ref["var"]).abs() / ref["var"]).max().item()
    mean_err = ((mean.double().cpu() - ref["mean"]).abs() / std).max().item()
    y_err = l2rel(y, ref["y"])
    print(shape, "leaky" if leaky else "relu", f"variance {var_err:.2e} relative, mean {mean_err:.2e} of a standard deviation, y {y_err:.2e} relative L2")
    assert var_err <= 1e-5 and mean_err <= 1e-5 and y_err <= 5e-6
    assert l2rel(invstd, 1 / (ref["var"] + R.BN_EPS).sqrt()) <= 1e-5
    # the running statistics: momentum 0.01, the variance with N / (N - 1)
    N = z.numel() // shape[-1]
    assert l2rel(rmd, ref["running_mean"]) <= 1e-6 and l2rel(rvd, ref["running_var"]) <= 1e-6
    if N < 100:  # the statistic that went into the running variance is N / (N - 1) times the batch variance (1.4 % and 9 % here)
        step = (rvd.double().cpu() - 0.99 * rv.double()) / 0.01
        assert ((step / ref["var"] - N / (N - 1)).abs().max().item()) <= 1e-3 < 0.1 * (N / (N - 1) - 1)
    # without running buffers nothing else changes
    y2, mean2, _, _ = T.bn_train_forward(c(z), c(gamma), c(beta), act=ACT[leaky])
    assert torch.equal(y2, y) and torch.equal(mean2, mean)


def test_bn_refuses_other_channel_counts_and_a_single_row_without_a_launch(T):
    from articulation3d_amd import _lib

    z = torch.randn(1, 3, 4, 96, device="cuda")
    ones = lambda n: torch.ones(n, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="A3D_ERR_ARG"):
        T.bn_train_forward(z, ones(96), ones(96), act=1)
    with pytest.raises(RuntimeError, match="A3D_ERR_ARG"):
        T.bn_train_forward(torch.randn(1, 1, 1, 64, device="cuda"), ones(64), ones(64), act=1)
    assert _lib.lib().a3d_bn_train_workspace_bytes(12, 96) == 0 and _lib.lib().a3d_bn_train_workspace_bytes(1, 64) == 0
    assert _lib.lib().a3d_bn_train_workspace_bytes(2, 64) > 0
    # malformed descriptors of a good shape: refused as argument errors, nothing written
    zz, y = torch.randn(2, 2, 2, 64, device="cuda"), torch.full((2, 2, 2, 64), 7.0, device="cuda")
    ws = torch.empty(_lib.lib().a3d_bn_train_workspace_bytes(8, 64) // 4, device="cuda")
    keep = [zz, y, ws, ones(64), ones(64), ones(64), ones(64)]

    def desc():
        d = _lib.BnTrainDesc()
        d.z, d.y, d.workspace, d.gamma, d.beta, d.mean, d.invstd = (t.data_ptr() for t in keep)
        d.N, d.C, d.act, d.eps, d.momentum = 8, 64, 1, 1e-3, 0.01
        return d

    st = torch.cuda.current_stream().cuda_stream
    fwd = lambda d: _lib.lib().a3d_bn_train_forward(C.byref(d), st)
    bwd = lambda d: _lib.lib().a3d_bn_train_backward(C.byref(d), st)
    assert _lib.lib().a3d_bn_train_forward(None, st) == -1 and _lib.lib().a3d_bn_train_backward(None, st) == -1
    for edit in (lambda d: setattr(d, "act", 0), lambda d: setattr(d, "z", None), lambda d: setattr(d, "workspace", None),
                 lambda d: setattr(d, "eps", 0.0), lambda d: setattr(d, "running_mean", keep[3].data_ptr()), lambda d: setattr(d, "z", zz.data_ptr() + 4)):
        d = desc()
        edit(d)
        assert fwd(d) == -1
    d = desc()
    assert bwd(d) == -1  # no dy / dz / dgamma / dbeta
    d.dy = d.dz = zz.data_ptr()
    d.dgamma = d.dbeta = keep[3].data_ptr()
    for pitch, off in ((32, 0), (66, 0), (128, 2), (128, 68), (64, -4)):
        d.dy_pitch, d.dy_off = pitch, off
        assert bwd(d) == -1, (pitch, off)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert fwd(desc()) == 0
    torch.cuda.synchronize()
    assert not bool((y == 7.0).all())


@pytest.mark.parametrize("leaky", [True, False], ids=["leaky", "relu"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_backward_against_float64(T, bn_refs, shape, leaky):
    (z, gamma, beta, rm, rv, dy), ref = bn_refs(shape, leaky)
    c = lambda t: t.cuda().contiguous()
    Cc = shape[-1]
    # y, mean and invstd as the float64 forward has them, rounded: the activation's derivative is the reference's own at every element
    y = c(ref["y"].float())
    assert bool(((y > 0) == (ref["y"].cuda() > 0)).all())
    mean, invstd = c(ref["mean"].float()), c((1 / (ref["var"] + R.BN_EPS).sqrt()).float())

    def run(dy_dev, off):
        dg, db = torch.empty(Cc, device="cuda"), torch.empty(Cc, device="cuda")
        dz = T.bn_train_backward(dy_dev, c(z), y, mean, invstd, c(gamma), act=ACT[leaky], dgamma=dg, dbeta=db, dy_off=off)
        return dz, dg, db

    dz, dg, db = run(c(dy), 0)
    torch.cuda.synchronize()
    errs = dict(dz=l2rel(dz, ref["dz"]), dgamma=l2rel(dg, ref["dgamma"]), dbeta=l2rel(db, ref["dbeta"]))
    print(shape, "leaky" if leaky else "relu", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= 1e-5 for v in errs.values()), errs
    # two runs: the same bits
    again = run(c(dy), 0)
    assert all(torch.equal(a, b) for a, b in zip((dz, dg, db), again))
    # dy as the lower / the upper half of a tensor twice as wide (a concatenated gradient read in place): the same bits again
    other = torch.randn(*shape, device="cuda")
    for off, wide in ((0, torch.cat([c(dy), other], -1)), (Cc, torch.cat([other, c(dy)], -1))):
        half = run(wide.contiguous(), off)
        assert all(torch.equal(a, b) for a, b in zip((dz, dg, db), half)), off


def test_bn_halves_of_a_256_channel_gradient(T, bn_refs):
    """The decoder's own shape: the two 128-channel halves of a 256-channel data gradient feed two different norms."""
    shape = (2, 5, 7, 128)
    c = lambda t: t.cuda().contiguous()
    cases = [R.bn_case(shape, seed=s) for s in (21, 22)]
    wide = torch.cat([c(cs[5]) for cs in cases], -1).contiguous()  # [2, 5, 7, 256]
    for i, (z, gamma, beta, rm, rv, dy) in enumerate(cases):
        ref = R.bn_ref(z, gamma, beta, rm, rv, i == 0, dy)
        dg, db = torch.empty(128, device="cuda"), torch.empty(128, device="cuda")
        dz = T.bn_train_backward(wide, c(z), c(ref["y"].float()), c(ref["mean"].float()), c((1 / (ref["var"] + R.BN_EPS).sqrt()).float()), c(gamma),
                                 act=ACT[i == 0], dgamma=dg, dbeta=db, dy_off=128 * i)
        assert l2rel(dz, ref["dz"]) <= 1e-5 and l2rel(dg, ref["dgamma"]) <= 1e-5 and l2rel(db, ref["dbeta"]) <= 1e-5


# ------------------------------------------------------------------------------------------ a3d_depth_loss
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 1, 1), (1, 240, 320)], ids=lambda s: "x".join(map(str, s)))
def test_depth_loss_against_float64(T, shape):
    d, gt = R.loss_case(*shape, holes=shape != (1, 1, 1))
    want, want_grad, res = R.loss_case_ref(d, gt, 0.75)
    out, dd = T.depth_loss(d.cuda(), gt.cuda(), loss_weight=0.75)
    torch.cuda.synchronize()
    valid = int((gt > R.VALID).sum())
    print(shape, "loss", out[0].item(), want.item(), "valid", valid, "gradient", l2rel(dd, want_grad), "exact ties", int((res == 0).sum()))
    assert int(out[1].item()) == valid > 0
    assert abs(out[0].item() - want.item()) <= 1e-6 * abs(want.item())
    assert l2rel(dd, want_grad) <= 1e-5
    again = T.depth_loss(d.cuda(), gt.cuda(), loss_weight=0.75)
    assert torch.equal(again[0], out) and torch.equal(again[1], dd)
    if shape == (2, 5, 7):  # the crafted ties give no gradient: the corner pixel's only valid outputs are ties or pull with a known sign
        assert int((res == 0).sum()) > 0
    # everything masked out: loss 0, gradient 0 (zeros, and values at exactly the threshold)
    for fill in (0.0, R.VALID):
        out0, dd0 = T.depth_loss(d.cuda(), torch.full_like(gt, fill).cuda(), loss_weight=0.75)
        assert out0[0].item() == 0.0 and out0[1].item() == 0.0 and bool((dd0 == 0).all())


# ------------------------------------------------------------------------------------------ the small kernels
def test_depth_pred_backward_against_float64(T):
    g = torch.Generator().manual_seed(2)
    x, up = torch.randn(2, 5, 7, 64, generator=g), torch.randn(2, 5, 7, generator=g)
    w = torch.randn(1, 64, 3, 3, generator=g) * 0.1
    xd, wd, bd = x.double().permute(0, 3, 1, 2).requires_grad_(True), w.double().requires_grad_(True), torch.zeros(1, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(xd, wd, bd, padding=1)[:, 0].backward(up.double())
    w9 = w[0].permute(1, 2, 0).reshape(9, 64).contiguous().cuda()
    out, dx = T.depth_pred_backward(x.cuda(), up.cuda(), w9)
    torch.cuda.synchronize()
    dw = out[:576].view(1, 3, 3, 64).permute(0, 3, 1, 2)
    errs = dict(dw=l2rel(dw, wd.grad), db=abs(out[576].item() - bd.grad.item()) / abs(bd.grad.item()), dx=l2rel(dx, xd.grad.permute(0, 2, 3, 1)))
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= 1e-5 for v in errs.values()), errs
    # ... and it is the adjoint of the forward kernel the trainer runs
    from articulation3d_amd import ops

    y = ops.conv3x3_to1(x.cuda(), w9, 0.0)
    assert abs((y * up.cuda()).sum().item() - (dw.cpu() * w).sum().item()) <= 1e-4 * (y * up.cuda()).abs().sum().item()
    again = T.depth_pred_backward(x.cuda(), up.cuda(), w9)
    assert torch.equal(again[0], out) and torch.equal(again[1], dx)


def test_ups2_concat_is_bit_equal_to_torch(T):
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(2, 3, 4, 128, generator=g).cuda(), torch.randn(2, 3, 4, 128, generator=g).cuda()
    want = torch.cat([a, b], -1).repeat_interleave(2, 1).repeat_interleave(2, 2)
    got = T.ups2_concat(a, b)
    assert got.shape == (2, 6, 8, 256) and torch.equal(got, want)
    assert torch.equal(T.ups2_concat(a), a.repeat_interleave(2, 1).repeat_interleave(2, 2))
    # its adjoint is the 2 x 2 block sum the trainer uses
    up = torch.randn_like(want)
    pooled = T.sumpool2_add(up, torch.zeros(2, 3, 4, 256, device="cuda"))
    assert abs((got * up).sum().item() - (torch.cat([a, b], -1) * pooled).sum().item()) <= 1e-4 * (got * up).abs().sum().item()


@pytest.mark.parametrize("sizes", [((16, 20), (15, 20)), ((6, 6), (5, 6))], ids=["16x20-15x20", "6x6-5x6"])
def test_resize_backward_against_float64(T, sizes):
    from articulation3d_amd import ops

    (H, W), (Ho, Wo) = sizes
    g = torch.Generator().manual_seed(4)
    x, up = torch.randn(2, H, W, 128, generator=g), torch.randn(2, Ho, Wo, 128, generator=g)
    xd = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    yd = torch.nn.functional.interpolate(xd, size=(Ho, Wo), mode="bilinear", align_corners=False)
    yd.backward(up.double().permute(0, 3, 1, 2))
    assert l2rel(ops.resize_bilinear(x.cuda(), Ho, Wo), yd.permute(0, 2, 3, 1)) <= 1e-6  # (the forward kernel it is the backward of)
    dx = T.resize_bilinear_backward(up.cuda(), H, W)
    torch.cuda.synchronize()
    assert dx.shape == x.shape and l2rel(dx, xd.grad.permute(0, 2, 3, 1)) <= 1e-5
    assert torch.equal(T.resize_bilinear_backward(up.cuda(), H, W), dx)


# ------------------------------------------------------------------------------------------ the decoder and the step
def _reference(tr, p0, feats_nhwc, gt, aux, precision):
    """Float64 autograd of the reference's depth head on the trainer's own pyramid, the gates within GATE_MARGIN of a kink taken from the
    trainer's forward pass; asserts the loss and every gradient within the stage's bounds -> (P with .grad, running buffers, keep)."""
    feats = {k: v.permute(0, 3, 1, 2).double() for k, v in feats_nhwc.items()}
    P = {k: v.double().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in p0.items()}
    running = {k: v.clone() for k, v in P.items() if "running" in k}
    gates = {b: aux["depth_acts"][b]["y"].permute(0, 3, 1, 2) > 0 for b in R.BLOCKS}
    ties, keep = [], {}
    want = R.decoder_loss_ref(feats, P, gt.cuda().double(), tr.loss_weight, gates=gates, ties=ties, running=running, keep=keep)
    want.backward()
    total = sum(v.numel() for v in gates.values())
    print(precision, "reference gates within", R.GATE_MARGIN, "of 0 per block:", ties, "of", total)
    assert len(ties) == 10 and sum(ties) <= R.GATE_FRACTION * total, ties
    return P, running, keep, want, feats, gates


def _check_gradients(tr, P, keep, got, want, precision):
    loss_bound, bound = (1e-5, 2e-4) if precision != "bf16" else (2e-2, 5e-2)
    assert abs(got.item() - want.item()) <= loss_bound * abs(want.item()), (got.item(), want.item())
    g = tr.export_grads()
    trainable = {k for k, v in P.items() if v.requires_grad}
    assert set(g) == trainable and len(g) == 42 and sum(v.numel() for v in g.values()) == R.NUM_PARAMS
    front = {R.entries(b)[0] + ".bias": b for b in R.BLOCKS}
    errs, zero = {}, {}
    for k in g:
        assert g[k].shape == P[k].shape, k
        if k in front:  # zero in exact arithmetic: held against the size of what cancels, per channel
            dz_sum = keep[front[k]][0].grad.abs().sum((0, 2, 3))
            zero[k] = ((g[k].double().abs() - 1e-5 * dz_sum).max().item(), dz_sum.max().item())
        else:
            errs[k] = l2rel(g[k], P[k].grad)
    print(precision, "depth_loss", got.item(), want.item(), "relative L2 gradient errors:", {k[len(DH):]: f"{v:.2e}" for k, v in errs.items()})
    print(precision, "biases in front of a norm, max over channels of |db| - 1e-5 sum|dz| (and max sum|dz|):", {k[len(DH):]: (f"{a:.2e}", f"{b:.2e}") for k, (a, b) in zero.items()})
    for k, e in errs.items():
        assert e < bound, (k, e)
    for k, (a, _) in zero.items():
        assert a <= 0, (k, a)
    return g


def _free_running(tr, p0, feats, gt, gates, g, got, precision):
    """Every gate the float64 decoder's own: printed beside the gated comparison, held to the looser 5e-2 of tests/test_gpu_training.py."""
    Pf = {k: v.double().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in p0.items()}
    keep = {}
    free = R.decoder_loss_ref(feats, Pf, gt.cuda().double(), tr.loss_weight, keep=keep)
    free.backward()
    flips = [int((gates[b] != (keep[b][1].detach() > 0)).sum()) for b in R.BLOCKS]
    front = {R.entries(b)[0] + ".bias" for b in R.BLOCKS}
    errs = {k: l2rel(g[k], Pf[k].grad) for k in g if k not in front}
    print(precision, "free-running: gates that differ per block", flips, "loss", free.item(), "worst gradient error", max(errs.values()))
    assert abs(got.item() - free.item()) <= (1e-5 if precision != "bf16" else 2e-2) * abs(free.item())
    assert all(e < 5e-2 for e in errs.values()), errs


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_decoder_matches_float64_autograd_on_a_small_pyramid(hip_model, precision):
    """Two 160 x 192 frames: p2 40 x 48 ... p5 5 x 6, p6 3 x 3; deconv1's 6 x 6 is resized to 5 x 6."""
    from articulation3d_amd.training_depth import DepthTrainer

    tr = DepthTrainer(hip_model, seed=5, precision=precision, loss_weight=0.75)
    p0 = {k: v.clone() for k, v in tr.export_state_dict().items()}
    pyr = R.random_pyramid(2, 160, 192)
    assert tuple(pyr["p5"].shape[-2:]) == (5, 6) and tuple(pyr["p6"].shape[-2:]) == (3, 3)
    feats = {k: nhwc(v).cuda() for k, v in pyr.items()}
    with torch.no_grad():
        pred = R.upsample2(R.decoder_pred({k: v.cuda().double() for k, v in pyr.items()}, {k: v.double() for k, v in p0.items()}))
    gt = R.craft_gt(pred)
    assert tuple(gt.shape) == (2, 160, 192) and 0.3 < float((gt > R.VALID).float().mean()) < 0.9 and int((gt == 0).sum()) > 0
    got, aux = tr.decoder_forward_backward(feats, gt)
    torch.cuda.synchronize()
    assert tuple(aux["depth_acts"]["deconv1"]["y"].shape[1:3]) == (6, 6) and tuple(aux["depth_pred"].shape) == (2, 80, 96)
    assert int(aux["depth_valid"].item()) == int((gt > R.VALID).sum())
    P, running, keep, want, f64, gates = _reference(tr, p0, feats, gt, aux, precision)
    g = _check_gradients(tr, P, keep, got, want, precision)
    _free_running(tr, p0, f64, gt, gates, g, got, precision)
    # the running statistics of the ten norms after one pass, and the batch count
    after = tr.export_state_dict()
    for k, v in running.items():
        assert l2rel(after[k], v) < (1e-5 if precision != "bf16" else 1e-2), k
        assert not torch.equal(after[k], p0[k]), k
    assert all(int(after[R.entries(b)[1] + ".num_batches_tracked"]) == int(p0[R.entries(b)[1] + ".num_batches_tracked"]) + 1 for b in R.BLOCKS)
    # the same call again: the same bits (running buffers aside)
    g2_loss, _ = tr.decoder_forward_backward(feats, gt, update_running=False)
    g2 = tr.export_grads()
    assert torch.equal(g2_loss, got) and all(torch.equal(g[k], g2[k]) for k in g)
    assert all(torch.equal(tr.export_state_dict()[k], after[k]) for k in running)


@pytest.fixture(scope="module")
def batch(oracle):
    from oracle import train_oracle as TO

    frames = torch.from_numpy(oracle.synthetic_frames(2)).cuda()
    tg = TO.synthetic_targets(2)
    yy, xx = torch.meshgrid(torch.arange(480.0), torch.arange(640.0), indexing="ij")
    depth = torch.stack([1.0 + 2.0 * yy / 480 + 0.5 * torch.sin(xx / 40 + i) for i in range(2)])  # a smooth positive depth map per frame
    depth[:, 100:160, 200:420] = 0.0  # ... with a hole
    return frames, [t[0] for t in tg], [t[1] for t in tg], depth


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_frozen_forward_is_stage_ones_forward_bit_for_bit(hip_model, batch, precision):
    from articulation3d_amd.training import DetectorTrainer
    from articulation3d_amd.training_depth import DepthTrainer

    frames, gb, gc, gd = batch
    t1 = DetectorTrainer(hip_model, seed=13, precision=precision)
    l1, a1 = t1.forward_backward(frames, gb, gc)
    t2 = DepthTrainer(hip_model, seed=13, precision=precision)
    l2, a2 = t2.forward_backward(frames, gb, gc, gd)
    torch.cuda.synchronize()
    assert set(l2) == {"loss_cls", "loss_box_reg", "depth_loss"}
    for k in ("loss_cls", "loss_box_reg"):
        assert torch.equal(l1[k], l2[k]), k
    for k in ("roi_index", "roi_count", "roi_cls", "roi_boxes"):
        assert torch.equal(a1[k], a2[k]), k
    assert torch.equal(a1["proposals"][0], a2["proposals"][0]) and torch.equal(a1["proposals"][1], a2["proposals"][1])
    assert bool(torch.isfinite(l2["depth_loss"])) and tuple(a2["depth_pred"].shape) == (2, 240, 320)
    # malformed ground truth: refused before anything runs
    t2.phase_events = []
    for bad in (gd[:, :240], gd[:1].reshape(480, 640), [gd[0], gd[1, :, :320]]):
        with pytest.raises(AssertionError):
            t2.forward_backward(frames, gb, gc, bad)
    assert t2.phase_events == []


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_depth_step_matches_float64_autograd(hip_model, batch, precision):
    from articulation3d_amd.training import SolverCfg, lr_at
    from articulation3d_amd.training_depth import DepthTrainer

    frames, gb, gc, gd = batch
    solver = SolverCfg(base_lr=0.1, warmup_iters=0)  # (a rate at which the two weight decays differ by 1e-5 of a parameter: ten times the bound below)
    # the pyramid of this batch (the frozen detector does not read the depth), the float64 prediction on it, the ground truth made from it
    t0 = DepthTrainer(hip_model, seed=21, precision=precision)
    p0 = {k: v.clone() for k, v in t0.export_state_dict().items()}
    _, a0 = t0.forward_backward(frames, gb, gc, gd)
    feats0 = {k: a0["feats"][k].float().clone() for k in ("p2", "p3", "p4", "p5", "p6")}
    del a0, t0
    with torch.no_grad():
        pred = R.upsample2(R.decoder_pred({k: v.permute(0, 3, 1, 2).double() for k, v in feats0.items()}, {k: v.double() for k, v in p0.items()}))
    gt = R.craft_gt(pred)
    del pred
    assert 0.3 < float((gt > R.VALID).float().mean()) < 0.9
    model_before = {k: v.clone() for k, v in hip_model.state_dict().items()}
    tr = DepthTrainer(hip_model, solver, seed=21, precision=precision)
    losses, aux = tr.forward_backward(frames, gb, gc, gt)
    torch.cuda.synchronize()
    assert set(losses) == {"loss_cls", "loss_box_reg", "depth_loss"}
    feats = {k: aux["feats"][k].float() for k in feats0}
    assert all(torch.equal(feats[k], feats0[k]) for k in feats)
    P, running, keep, want, f64, gates = _reference(tr, p0, feats, gt, aux, precision)
    g = _check_gradients(tr, P, keep, losses["depth_loss"], want, precision)
    del keep, f64, gates
    # update: the float64 SGD formula, weight decay 0 on the norm parameters and 1e-4 elsewhere
    tr.optimizer_step()
    s = tr.s
    assert (s.weight_decay, s.weight_decay_norm) == (1e-4, 0.0) and tr.weight_decays == [1e-4, 0.0]
    lr0 = lr_at(0, s)
    p1 = tr.export_state_dict()
    norm_params = {R.entries(b)[1] + leaf for b in R.BLOCKS for leaf in (".weight", ".bias")}
    for k in g:
        wd = 0.0 if k in norm_params else s.weight_decay
        want_p = p0[k].double() - lr0 * (g[k].double() + wd * p0[k].double())  # first step: the momentum buffer starts as the gradient
        assert l2rel(p1[k], want_p) < 1e-6, k
    assert any(not torch.equal(p0[k], p1[k]) for k in g)
    # with a decay on the norms the result would differ measurably: the check above sees the difference between the two groups
    k = R.entries("deconv5")[1] + ".weight"
    assert lr0 == 0.1 and l2rel(p0[k].double() - lr0 * (g[k].double() + s.weight_decay * p0[k].double()), p0[k].double() - lr0 * g[k].double()) > 5e-6
    # the running statistics and the batch count equal the reference's
    for k, v in running.items():
        assert l2rel(p1[k], v) < (1e-5 if precision != "bf16" else 1e-2), k
    assert all(int(p1[R.entries(b)[1] + ".num_batches_tracked"]) == int(p0[R.entries(b)[1] + ".num_batches_tracked"]) + 1 for b in R.BLOCKS)
    assert set(p1) == {k_ for k_ in model_before if k_.startswith(DH)}
    # nothing of the model changed in the step; leaving training mode writes a complete depth head back
    assert all(torch.equal(v, hip_model.state_dict()[k_]) for k_, v in model_before.items())
    try:
        hip_model.train()
        hip_model._trainer = tr
        hip_model.train(False)
        after = hip_model.state_dict()
        for k_, v in model_before.items():
            if k_.startswith(DH):
                assert torch.equal(after[k_].float(), p1[k_].float()), k_
            else:
                assert torch.equal(after[k_], v), k_
    finally:  # (the session-scoped model goes back to the state the other tests expect, whatever failed above)
        hip_model.__dict__.pop("_trainer", None)
        hip_model.train(False)
        hip_model.load_state_dict(model_before)


def test_depth_loss_decreases_on_a_fixed_batch(hip_model, batch):
    from articulation3d_amd.training import SolverCfg
    from articulation3d_amd.training_depth import DepthTrainer

    frames, gb, gc, gd = batch
    tr = DepthTrainer(hip_model, SolverCfg(base_lr=0.005, warmup_iters=0), seed=3)
    hist = []
    for _ in range(5):
        l, _ = tr.step(frames, gb, gc, gd)
        hist.append(l["depth_loss"])
    hist = torch.stack(hist).cpu()
    print("depth_loss over 5 steps:", hist.tolist())
    assert bool(torch.isfinite(hist).all()) and hist[-1] < hist[0], hist.tolist()
    assert tr.num_batches_tracked == 5 and tr.iter == 5


def test_reference_training_loop_is_a_drop_in_for_the_depth_stage(oracle, oracle_params, batch):
    """model.train(); losses = model(data); sum(losses.values()).backward(); build_optimizer(cfg, model).step(); model.eval(): the
    trained depth head, its running statistics included, reaches inference."""
    from conftest import ROOT
    from articulation3d_amd.config import get_cfg, get_planercnn_cfg_defaults
    from articulation3d_amd.engine import build_optimizer
    from articulation3d_amd.modeling import build_model
    from articulation3d_amd.structures import Boxes, Instances
    from articulation3d_amd.training_depth import DepthTrainer

    cfg = get_cfg()
    get_planercnn_cfg_defaults(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "step3_depth.yaml"))
    cfg.MODEL.DEVICE = "cuda"
    model = build_model(cfg)
    missing, unexpected = model.load_state_dict(oracle_params, strict=False)
    assert not unexpected and all("num_batches_tracked" in k for k in missing)
    assert model.training_stage() == 5
    frames, gb, gc, gd = batch
    data = []
    for i in range(frames.shape[0]):
        inst = Instances((480, 640), gt_boxes=Boxes(gb[i].cuda()), gt_classes=gc[i].cuda())
        data.append({"image": frames[i].permute(2, 0, 1).cpu(), "instances": inst, "depth": gd[i]})
    model.train()
    losses = model(data)
    assert set(losses) == {"loss_cls", "loss_box_reg", "depth_loss"}
    sum(losses.values()).backward()
    optimizer = build_optimizer(cfg, model)
    assert isinstance(model.trainer(), DepthTrainer)
    assert [grp["weight_decay"] for grp in optimizer.param_groups] == [1e-4, 0.0]  # detectron2's two groups: WEIGHT_DECAY, WEIGHT_DECAY_NORM
    before = {k: v.clone() for k, v in model.state_dict().items()}
    optimizer.step()
    model.eval()
    after = model.state_dict()
    want = model.trainer().export_state_dict()
    assert set(want) == {k for k in before if k.startswith(DH)}
    assert any(not torch.equal(before[k], after[k]) for k in want)
    for k, v in before.items():
        if k in want:
            assert torch.equal(after[k].float(), want[k].float()), k
        else:
            assert torch.equal(after[k], v), k
    assert all(int(after[R.entries(b)[1] + ".num_batches_tracked"]) == 1 for b in R.BLOCKS)
    # inference of the trained head on a pyramid: the oracle's depth head on the exported state, within tests/test_gpu_parity.py's 2e-5
    pyr = R.random_pyramid(1, 480, 640, seed=6)
    with torch.no_grad():
        got = model.depth_head.forward_nhwc({k: nhwc(v).cuda() for k, v in pyr.items()})
        ref = oracle.depth_head(pyr, {k: v.float().cpu() for k, v in want.items()})
    assert tuple(got.shape) == (1, 480, 640) and l2rel(got, ref) < 2e-5, l2rel(got, ref)
