"""References of the depth head's training step (tests/test_depth_train_host.py, tests/test_gpu_depth_training.py), all torch itself under
float64 autograd: training-mode batch norm + activation, the masked L1 loss on the x2 bilinear upsampling (l1LossMask restated), and the
reference depth head's forward pass in training mode (pkg/modeling/depth_net/depth_head.py:72-97) on a given pyramid and parameters; plus
the seeded cases the kernel tests share.  Not a test module."""
import torch
import torch.nn.functional as F

DH = "depth_head."
BN_EPS, BN_MOMENTUM = 1e-3, 0.01
LEAKY = 0.01
VALID = 1e-4
NUM_PARAMS = 2658433
BLOCKS = [f"conv{k}" for k in range(1, 6)] + [f"deconv{k}" for k in range(1, 6)]
GATE_MARGIN = 1e-5    # an activation gate of the float64 decoder may follow the device forward only where its pre-activation is this close to 0
GATE_FRACTION = 2e-5  # ... and at most this share of the gates may lie that close (pre-activations of order 1: about 2 x margin of them)


def entries(block):
    """(conv entry, norm entry, leaky?) of a block of the reference's nn.Sequential layout."""
    return (DH + block + ".0", DH + block + ".1", True) if block.startswith("conv") else (DH + block + ".1", DH + block + ".2", False)


def bn_act(z, gamma, beta, leaky, running_mean=None, running_var=None):
    """nn.BatchNorm2d(eps 1e-3, momentum 0.01) in training mode + the block's activation on z [B, C, H, W]; the running buffers (if given)
    are updated in place, with the unbiased variance, as F.batch_norm does."""
    y = F.batch_norm(z, running_mean, running_var, gamma, beta, training=True, momentum=BN_MOMENTUM, eps=BN_EPS)
    return F.leaky_relu(y, LEAKY) if leaky else F.relu(y)


def l1_loss_mask(pred, gt, mask):
    """depth_head.py:19-21."""
    return torch.sum(torch.abs(pred - gt) * mask) / torch.clamp(mask.sum(), min=1)


def upsample2(d):
    """depth_head.py:88 for d [B, h, w]: bilinear to twice the size, align_corners False."""
    return F.interpolate(d[:, None], size=(2 * d.shape[1], 2 * d.shape[2]), mode="bilinear", align_corners=False)[:, 0]


def depth_loss_ref(d, gt, loss_weight=1.0):
    """The contract of a3d_depth_loss: loss_weight * l1LossMask(upsample2(d), gt, gt > 1e-4)."""
    return loss_weight * l1_loss_mask(upsample2(d), gt, (gt > VALID).to(d.dtype))


def decoder_pred(feats, P, gates=None, ties=None, running=None, keep=None):
    """feats {p2..p6: [B, 256, h, w]}, P: depth_head.* in the reference's layouts -> depth_pred's output [B, 4 h_p2 / 2, ...] BEFORE the
    last upsampling, the ten norms in training mode.
    gates: per block the device forward's (activation > 0) [B, C, h, w].  The gradient jumps where a pre-activation crosses 0, and an
    fp32 forward pass lands on the other side of a float64 one where the pre-activation is within its rounding of 0; either side is the
    derivative of a forward pass within rounding of this one, so where |pre-activation| <= GATE_MARGIN the gate is taken from `gates`,
    everywhere else it is the float64 one (tests/plane_train_ref.py's rule).  ties (a list) receives the count per block.
    running: {norm entry + ".running_mean" / ".running_var": tensor} updated in place.  keep (a dict) receives per block the conv's
    output z (with retain_grad) and the activation."""
    def block(name, x):
        conv, norm, leaky = entries(name)
        if not leaky:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        z = F.conv2d(x, P[conv + ".weight"], P[conv + ".bias"], padding=1)
        rm = rv = None
        if running is not None:
            rm, rv = running[norm + ".running_mean"], running[norm + ".running_var"]
        pre = F.batch_norm(z, rm, rv, P[norm + ".weight"], P[norm + ".bias"], training=True, momentum=BN_MOMENTUM, eps=BN_EPS)
        if gates is None:
            y = F.leaky_relu(pre, LEAKY) if leaky else F.relu(pre)
        else:
            near = pre.detach().abs() <= GATE_MARGIN
            opened = torch.where(near, gates[name], pre.detach() > 0)
            one = torch.ones((), dtype=pre.dtype, device=pre.device)
            y = pre * torch.where(opened, one, one * (LEAKY if leaky else 0.0))
            if ties is not None:
                ties.append(int(near.sum()))
        if keep is not None:
            if z.requires_grad:
                z.retain_grad()
            keep[name] = (z, y)
        return y

    x = block("deconv1", block("conv1", feats["p6"]))
    x = F.interpolate(x, size=feats["p5"].shape[-2:], mode="bilinear", align_corners=False)
    for k, lvl in ((2, "p5"), (3, "p4"), (4, "p3"), (5, "p2")):
        x = block(f"deconv{k}", torch.cat([block(f"conv{k}", feats[lvl]), x], 1))
    return F.conv2d(x, P[DH + "depth_pred.weight"], P[DH + "depth_pred.bias"], padding=1)[:, 0]


def decoder_loss_ref(feats, P, gt, loss_weight=1.0, **kw):
    """The reference depth head in training mode: depth_loss = loss_weight * l1LossMask(pred, gt, gt > 1e-4)."""
    return depth_loss_ref(decoder_pred(feats, P, **kw), gt.to(feats["p2"].dtype), loss_weight)


# ------------------------------------------------------------------------------------------ seeded cases of the kernel tests
def bn_case(shape, seed=5, sigmas=20.0):
    """-> z [B, H, W, C] float32 whose every channel has its mean `sigmas` standard deviations from zero (either side), gamma, beta,
    running_mean, running_var, dy."""
    g = torch.Generator().manual_seed(seed)
    C = shape[-1]
    std = 0.5 + 1.5 * torch.rand(C, generator=g)
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    z = (torch.randn(*shape, generator=g) * std + sigmas * std * sign).float()
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.5 * torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    dy = torch.randn(*shape, generator=g)
    return z, gamma, beta, rm, rv, dy


def bn_ref(z, gamma, beta, rm, rv, leaky, dy=None):
    """float64 of a BN case (NHWC in and out) -> dict(mean, var, y, running_mean, running_var[, dz, dgamma, dbeta])."""
    zd = z.double().permute(0, 3, 1, 2).contiguous().requires_grad_(dy is not None)
    gd, bd = gamma.double().requires_grad_(dy is not None), beta.double().requires_grad_(dy is not None)
    rmd, rvd = rm.double().clone(), rv.double().clone()
    y = bn_act(zd, gd, bd, leaky, rmd, rvd)
    out = dict(mean=zd.detach().mean((0, 2, 3)), var=zd.detach().var((0, 2, 3), unbiased=False), y=y.detach().permute(0, 2, 3, 1),
               running_mean=rmd, running_var=rvd)
    if dy is not None:
        y.backward(dy.double().permute(0, 3, 1, 2))
        out.update(dz=zd.grad.permute(0, 2, 3, 1), dgamma=gd.grad, dbeta=bd.grad)
    return out


MIN_RESIDUAL = 0.05  # outside the crafted ties and the masked pixels every |pred - gt| of a loss case exceeds this


def loss_case(B, h, w, seed=9, holes=True, ties=True):
    """-> d [B, h, w], gt [B, 2h, 2w] float32.  gt = the float64 prediction moved by at least MIN_RESIDUAL either way (a wrong sign cannot
    hide behind a tolerance, fp32 rounding cannot flip an honest one); holes: a third of gt is 0 and some values are exactly 1e-4 (masked
    out: the mask is gt > 1e-4); ties: a constant 3 x 3 patch of d whose prediction is exact, met by the same gt (sign 0)."""
    g = torch.Generator().manual_seed(seed)
    d = 0.5 + 2.5 * torch.rand(B, h, w, generator=g)
    if ties and h >= 3 and w >= 3:
        d[0, :3, :3] = 2.0
    pred = upsample2(d.double())
    off = (MIN_RESIDUAL + torch.rand(pred.shape, generator=g).double()) * torch.where(torch.rand(pred.shape, generator=g) < 0.5, -1.0, 1.0)
    gt = (pred + off).float()
    gt = torch.where(gt > 10 * VALID, gt, (pred + off.abs()).float())  # (every unmasked value clearly valid)
    if ties and h >= 3 and w >= 3:
        gt[0, 1:4, 1:4] = 2.0
    if holes:
        u = torch.rand(pred.shape, generator=g)
        gt[u < 1 / 3] = 0.0
        gt[(u >= 1 / 3) & (u < 0.36)] = VALID
    return d.float(), gt


def loss_case_ref(d, gt, loss_weight):
    dd = d.double().requires_grad_(True)
    loss = depth_loss_ref(dd, gt.double(), loss_weight)
    loss.backward()
    res = (upsample2(d.double()) - gt.double())[gt.double() > VALID]
    return loss.detach(), dd.grad, res


def random_pyramid(B=2, H=160, W=192, seed=11, channels=256):
    """A random pyramid of B frames of H x W: p2 (H/4) ... p5 (H/32), p6 = ceil(p5 / 2) as the backbone's stride-2 max pool gives it."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, s in (("p2", 4), ("p3", 8), ("p4", 16), ("p5", 32)):
        out[k] = torch.randn(B, channels, H // s, W // s, generator=g)
    h5, w5 = out["p5"].shape[-2:]
    out["p6"] = torch.randn(B, channels, (h5 + 1) // 2, (w5 + 1) // 2, generator=g)
    return out


def craft_gt(pred_up, seed=13, hole_fraction=0.15):
    """Ground truth for a decoder / step test from the float64 prediction [B, H, W]: pred moved by 0.25 .. 1 of its mean magnitude
    either way (the far way where the near one would not be a positive depth), so that no precision's rounding flips a sign; zero holes
    (a rectangle and scattered pixels)."""
    g = torch.Generator().manual_seed(seed)
    p = pred_up.detach().double().cpu()
    scale = p.abs().mean()
    off = (0.25 + 0.75 * torch.rand(p.shape, generator=g).double()) * scale * torch.where(torch.rand(p.shape, generator=g) < 0.5, -1.0, 1.0)
    gt = p + off
    gt = torch.where(gt > 100 * VALID, gt, p.clamp(min=0) + off.abs()).float()  # (a depth is positive: the far side where the near one is not)
    gt[torch.rand(p.shape, generator=g) < hole_fraction] = 0.0
    H, W = p.shape[-2:]
    gt[:, H // 8: H // 4, W // 8: W // 2] = 0.0
    return gt
