"""References of the plane-normal head's training step (tests/test_plane_train_host.py, tests/test_gpu_plane_training.py), all under
float64 autograd: the contract of a3d_plane_loss in plain torch, and the reference plane head's forward pass + plane_rcnn_loss
(pkg/modeling/roi_heads/plane_head.py:71-124) on given pooled rows and parameters.  Not a test module."""
import torch
import torch.nn.functional as F

PH = "roi_heads.plane_head."


def plane_rcnn_loss_ref(pred, gt, loss_weight=1.0, normal_only=True):
    """plane_head.py:96-124 on the rows' matched ground truth gt [R, 3]: smooth_l1_loss(pred, F.normalize(gt), beta 0.0, "sum") -- beta
    below 1e-5 is the plain |x| -- times loss_weight over len(pred): the ROW count, not 3 x rows.  No rows: pred.sum() * 0."""
    if pred.shape[0] == 0:
        return pred.sum() * 0
    if normal_only:
        gt = F.normalize(gt, p=2, dim=1)
    return loss_weight * (pred - gt).abs().sum() / pred.shape[0]


def plane_loss_contract(h, w, b, row_img, row_gt, gt_planes, loss_weight=1.0, normal_only=True):
    """What a3d_plane_loss computes for the live rows h [live, K] (the FC's output after ReLU): w [3, K], b [3], row_img / row_gt [live]
    integers, gt_planes [B, max_gt, 3] -> (loss, raw [live, 3]).  A row whose image or ground-truth index is out of range adds nothing
    and still counts in the divisor.  The gradient of the kernel's dh is this loss's gradient with respect to h, gated by h > 0."""
    raw = h @ w.t() + b
    if h.shape[0] == 0:
        return raw.sum() * 0, raw
    B, G = gt_planes.shape[:2]
    ok = (row_img >= 0) & (row_img < B) & (row_gt >= 0) & (row_gt < G)
    gt = gt_planes[row_img.clamp(0, B - 1).long(), row_gt.clamp(0, G - 1).long()].to(h.dtype)
    pred = raw
    if normal_only:
        pred, gt = F.normalize(raw, p=2, dim=1), F.normalize(gt, p=2, dim=1)
    return loss_weight * ((pred - gt).abs() * ok[:, None].to(h.dtype)).sum() / h.shape[0], raw


GATE_MARGIN = 1e-5    # a ReLU gate of the float64 head may follow the device forward only where its pre-activation is this close to 0
GATE_FRACTION = 2e-5  # ... and at most this share of the gates may lie that close (pre-activations of order 1: about 2 x margin of them)


def plane_head_raw(x, P, gates=None, ties=None):
    """x [R, 256, 14, 14], P: roi_heads.plane_head.* in the reference's layouts -> param_pred's output [R, 3] before F.normalize.
    gates: per 3x3 layer the device forward's (activation > 0) [R, C, 14, 14].  The gradient of a ReLU network jumps where a
    pre-activation crosses 0, and an fp32 forward pass (relative error 1e-6 over K = 2304 sums) lands on the other side of a float64
    one where the pre-activation is within that error of 0: one such gate of 350 000 moves every gradient below it by 1e-3.  Either
    side is the derivative of a forward pass within rounding of this one, so where |pre-activation| <= GATE_MARGIN the gate is taken
    from `gates`; everywhere else it is the float64 one.  ties (a list) receives the count per layer."""
    k = 1
    while PH + f"plane_conv{k}.weight" in P:
        pre = F.conv2d(x, P[PH + f"plane_conv{k}.weight"], P[PH + f"plane_conv{k}.bias"], padding=1)
        if gates is None:
            x = F.relu(pre)
        else:
            near = pre.detach().abs() <= GATE_MARGIN
            x = pre * torch.where(near, gates[k - 1], pre.detach() > 0).to(pre.dtype)
            if ties is not None:
                ties.append(int(near.sum()))
        k += 1
    x = torch.flatten(x, start_dim=1)  # CHW order: the reference's FC columns
    k = 1
    while PH + f"plane_fc{k}.weight" in P:
        x = F.relu(F.linear(x, P[PH + f"plane_fc{k}.weight"], P[PH + f"plane_fc{k}.bias"]))
        k += 1
    return F.linear(x, P[PH + "param_pred.weight"], P[PH + "param_pred.bias"])


@torch.no_grad()
def plane_head_acts(x, P):
    """The outputs of the 3x3 layers [R, C, 14, 14], layer by layer, of the free-running float64 head."""
    out, k = [], 1
    while PH + f"plane_conv{k}.weight" in P:
        x = F.relu(F.conv2d(x, P[PH + f"plane_conv{k}.weight"], P[PH + f"plane_conv{k}.bias"], padding=1))
        out.append(x)
        k += 1
    return out


def plane_head_forward(x, P, normal_only=True, gates=None, ties=None):
    raw = plane_head_raw(x, P, gates, ties)
    return F.normalize(raw, p=2, dim=1) if normal_only else raw


def plane_loss_ref(x, P, gt, loss_weight=1.0, normal_only=True, gates=None, ties=None):
    """The reference plane head in training mode on pooled rows x and their matched ground truth gt [R, 3]."""
    return plane_rcnn_loss_ref(plane_head_forward(x, P, normal_only, gates, ties), gt.to(x.dtype), loss_weight, normal_only)


# ------------------------------------------------------------------------------------------ the shared case of the kernel tests
CRAFTED = dict(eps=0, equal=1, mirrored=2, zero_gt=3, bad_gt=4, bad_img=5)  # rows of loss_case
MIN_RESIDUAL = 1e-4  # outside the crafted rows every |pred - gt| component of the float64 reference exceeds this (the seeds are chosen so)


def loss_case(K=1024, rows=40, live=23, seed=3, B=2, G=5, crafted=True, bad_gt=(), bad_img=()):
    """-> h [rows, K], w [3, K], b [3], row_img [rows], row_gt [rows], gt_planes [B, G, 3] (float32 / int32).  About 5 % exact zeros and as
    many negative entries in h (an FC output after ReLU has neither negatives nor NaNs: the gate must still close on them); rows past
    `live` are NaN with indices that must never be used.  crafted: zero bias and the rows of CRAFTED --
      eps       h row 0 with a zero bias: raw is exactly 0, below F.normalize's eps clamp
      equal     one-hot h on a weight column (0, 3, 4), gt (0, 6, 8): collinear, every residual exactly 0 -> sign 0
      mirrored  the same prediction against gt (0, 6, -8): two residuals exactly 0, the third 1.6
      zero_gt   a zero ground-truth vector (normalises to 0)
      bad_gt / bad_img   row_gt / row_img out of range: nothing but a place in the divisor.
    bad_gt / bad_img (arguments): further live rows whose row_gt / row_img is out of range, with or without the crafted rows."""
    g = torch.Generator().manual_seed(seed)
    h = torch.rand(rows, K, generator=g) * 2
    u = torch.rand(rows, K, generator=g)
    h[u < 0.05] = 0.0
    h[(u >= 0.05) & (u < 0.10)] *= -1.0
    w = torch.randn(3, K, generator=g) * 0.05
    b = torch.zeros(3) if crafted else torch.randn(3, generator=g) * 0.1
    row_img = torch.randint(0, B, (rows,), generator=g, dtype=torch.int32)
    row_gt = torch.randint(0, G, (rows,), generator=g, dtype=torch.int32)
    gt = torch.randn(B, G, 3, generator=g) * 2
    if crafted:
        assert live > max(CRAFTED.values()) and G >= 4
        col = K // 2 + 7
        w[:, col] = torch.tensor([0.0, 3.0, 4.0])
        h[CRAFTED["eps"]] = 0.0
        for name, slot, vec in (("equal", 0, (0.0, 6.0, 8.0)), ("mirrored", 1, (0.0, 6.0, -8.0))):
            h[CRAFTED[name]] = 0.0
            h[CRAFTED[name], col] = 1.0
            row_img[CRAFTED[name]], row_gt[CRAFTED[name]] = 0, slot
            gt[0, slot] = torch.tensor(vec)
        row_img[CRAFTED["zero_gt"]], row_gt[CRAFTED["zero_gt"]] = 1, 2
        gt[1, 2] = 0.0
        for r in range(live):  # (no other row may land on a crafted ground truth)
            if r not in (CRAFTED["equal"], CRAFTED["mirrored"], CRAFTED["zero_gt"]) and (int(row_img[r]), int(row_gt[r])) in ((0, 0), (0, 1), (1, 2)):
                row_gt[r] = 3
        row_gt[CRAFTED["bad_gt"]] = G
        row_img[CRAFTED["bad_img"]] = -1
    for r in bad_gt:
        assert r < live
        row_gt[r] = G + 3
    for r in bad_img:
        assert r < live
        row_img[r] = B
    h[live:] = float("nan")
    row_img[live:] = 10 ** 6
    row_gt[live:] = 10 ** 6
    return h, w, b, row_img, row_gt, gt


def loss_case_ref(h, w, b, row_img, row_gt, gt, live, loss_weight=1.0, normal_only=True):
    """Float64 autograd of the contract on the live rows -> (loss, dh gated, dw, db, raw, residuals [live, 3] with NaN on the rows that
    are out of range)."""
    hd = h[:live].double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    loss, raw = plane_loss_contract(hd, wd, bd, row_img[:live], row_gt[:live], gt.double(), loss_weight, normal_only)
    if live:
        loss.backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    B, G = gt.shape[:2]
    ok = (row_img[:live] >= 0) & (row_img[:live] < B) & (row_gt[:live] >= 0) & (row_gt[:live] < G)
    t = gt.double()[row_img[:live].clamp(0, B - 1).long(), row_gt[:live].clamp(0, G - 1).long()]
    p = raw.detach()
    if normal_only:
        p, t = F.normalize(p, p=2, dim=1), F.normalize(t, p=2, dim=1)
    res = torch.where(ok[:, None], p - t, torch.full_like(p, float("nan")))
    return loss.detach(), z(hd) * (h[:live] > 0), z(wd), z(bd), raw.detach(), res
