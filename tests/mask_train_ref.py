"""References of the mask head's training step (tests/test_mask_train_host.py, tests/test_gpu_mask_training.py): the mask targets as the
oracle's ROIAlign of the ground-truth bitmask followed by >= 0.5 (detectron2 BitMasks.crop_and_resize), and the mask head's logits and
mean BCE-with-logits under float64 autograd.  Also the shared inputs of the target tests.  Not a test module."""
import math

import torch
import torch.nn.functional as F

MH = "roi_heads.mask_head."
TIE_MARGIN = 1e-4      # a device target may differ from the float64 one only where the float64 ROIAlign value is this close to 0.5
TIE_FRACTION = 1e-3    # ... and at most this share of the live pixels may lie that close


def roi_values(oracle, masks, boxes, gidx, size=28, dtype=torch.float64):
    """masks [N, H, W] (bool / uint8), boxes [K, 4], gidx [K] (the mask of each box) -> the ROIAlign((size, size), 1.0, sampling_ratio 0,
    aligned=True) values [K, size, size] in `dtype` arithmetic (the oracle's C operator: float32 or its float64 yardstick)."""
    feat = (masks != 0).to(dtype)[:, None]
    rois = torch.cat((gidx.to(torch.float32)[:, None], boxes.float()), 1)
    return oracle.roi_align(feat, rois.to(dtype) if dtype == torch.float64 else rois, size, 1.0, 0, True)[:, 0]


def targets_from_values(v):
    return (v >= 0.5).to(torch.uint8)


def check_targets(got, v64, margin=TIE_MARGIN, fraction=TIE_FRACTION):
    """got: uint8 [K, S, S] targets under test; v64: the float64 values.  Returns (mismatches, pixels inside the margin) after asserting
    the margin rule."""
    got = got.cpu()
    assert set(got.unique().tolist()) <= {0, 1}
    want = targets_from_values(v64)
    near = (v64 - 0.5).abs() <= margin
    diff = got != want
    n_diff, n_near = int(diff.sum()), int(near.sum())
    print(f"targets: {n_diff} of {got.numel()} differ from float64, {n_near} within {margin} of 0.5 ({n_near / max(got.numel(), 1):.5%})")
    assert not bool((diff & ~near).any()), f"{int((diff & ~near).sum())} targets differ outside the tie margin"
    assert n_near <= fraction * got.numel(), (n_near, got.numel())
    return n_diff, n_near


# ------------------------------------------------------------------------------------------ inputs of the target tests
def target_masks(H, W, seed):
    """Six masks [6, H, W] uint8: integer-edged rectangle, ellipse, stripes, 3-pixel checkerboard, noise, a thin sliver at the border.
    Also returns the rectangle's own box."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    m = torch.zeros(6, H, W, dtype=torch.uint8)
    x0, y0, x1, y1 = W // 5, H // 6, W // 5 + (3 * W) // 7, H // 6 + (4 * H) // 7
    m[0, y0:y1, x0:x1] = 1
    m[1] = ((((xx + 0.5 - W * 0.55) / (W * 0.31)) ** 2 + ((yy + 0.5 - H * 0.45) / (H * 0.38)) ** 2) <= 1).to(torch.uint8)
    m[2] = ((xx % 13) < 5).to(torch.uint8)  # (5 on, 8 off: a wide bin averages 0.38, not a tie)
    m[3] = (((xx // 3) + (yy // 3)) % 2 == 0).to(torch.uint8)
    m[4] = (torch.rand(H, W, generator=g) < 0.4).to(torch.uint8)
    m[5, :, W - 2:] = 1  # two columns at the right border
    m[5, H - 1, :] = 1   # and the last row
    return m, torch.tensor([x0, y0, x1, y1], dtype=torch.float32)


def target_case(H, W, seed, per_image=120, B=2):
    """-> masks [B, 6, H, W] uint8, boxes [B, per_image, 4], gt [B, per_image] int32: the rectangle's own box, the whole image (on the ellipse), a
    zero-width and a zero-height box, sub-pixel boxes, and log-uniform sizes from 1 to 490 pixels around centres inside the image
    (unclipped: on a small mask most of them cross the borders)."""
    g = torch.Generator().manual_seed(seed + 1)
    masks, boxes, gts = [], [], []
    for b in range(B):
        m, rect = target_masks(H, W, seed + 10 * b)
        masks.append(m)
        bx = [rect, torch.tensor([0.0, 0.0, W, H]), torch.tensor([W / 3, 5.0, W / 3, H - 7.0]), torch.tensor([3.0, H / 2, W - 9.0, H / 2]),
              torch.tensor([W / 2 + 0.2, H / 2 + 0.3, W / 2 + 0.7, H / 2 + 0.9]), torch.tensor([W - 1.25, H - 1.5, W - 0.5, H - 0.25]),
              torch.tensor([0.1, 0.2, 0.35, 2.7])]
        gt = [0, 1, 1, 2, 3, 5, 4]
        n = per_image - len(bx)
        size = torch.exp(torch.rand(n, 2, generator=g) * math.log(490.0))
        ctr = torch.rand(n, 2, generator=g) * torch.tensor([float(W), float(H)])
        rnd = torch.cat((ctr - size / 2, ctr + size / 2), 1)
        if b == 0:  # proposals proper: clipped to the image
            rnd[:, 0::2] = rnd[:, 0::2].clamp(0, W)
            rnd[:, 1::2] = rnd[:, 1::2].clamp(0, H)
        boxes.append(torch.cat((torch.stack(bx), rnd), 0))
        # (a bin that averages many periods of the checkerboard is a tie by construction: the checkerboard goes to the small boxes, whose
        # bins are sub-pixel interpolations, and the ellipse takes its place under the large ones)
        rg = torch.arange(n) % 6
        rg = torch.where((rg == 3) & (size.max(1).values > 30), torch.ones_like(rg), rg)
        gts.append(torch.cat((torch.tensor(gt), rg)).to(torch.int32))
    return torch.stack(masks), torch.stack(boxes), torch.stack(gts)


def target_case_values(oracle, masks, boxes, gt, dtype=torch.float64):
    """The values of every box of a target_case, image after image: [B * per_image, 28, 28]."""
    B, G = masks.shape[:2]
    flat = masks.reshape(B * G, *masks.shape[2:])
    gidx = (torch.arange(B)[:, None] * G + gt.long()).reshape(-1)
    return roi_values(oracle, flat, boxes.reshape(-1, 4), gidx, 28, dtype)


# ------------------------------------------------------------------------------------------ the head under float64 autograd
def mask_head_logits(x, P):
    """x [R, 256, 14, 14], P: roi_heads.mask_head.* in the reference's layouts -> logits [R, 28, 28] (the head without its sigmoid)."""
    k = 1
    while MH + f"mask_fcn{k}.weight" in P:
        x = F.relu(F.conv2d(x, P[MH + f"mask_fcn{k}.weight"], P[MH + f"mask_fcn{k}.bias"], padding=1))
        k += 1
    x = F.relu(F.conv_transpose2d(x, P[MH + "deconv.weight"], P[MH + "deconv.bias"], stride=2))
    return F.conv2d(x, P[MH + "predictor.weight"], P[MH + "predictor.bias"])[:, 0]


def mask_loss_ref(x, P, targets):
    """detectron2 mask_rcnn_loss of a class-agnostic head: the mean BCE-with-logits over all rows and pixels; no rows: logits.sum() * 0."""
    z = mask_head_logits(x, P)
    if z.shape[0] == 0:
        return z.sum() * 0
    return F.binary_cross_entropy_with_logits(z, targets.to(z.dtype), reduction="mean")


def unshuffle(x):
    """[R, C, 2P, 2P] -> [R, P, P, (dy, dx, c)]: the layout the deconv leaves as a plain 1x1 layer."""
    R, C, S, _ = x.shape
    return x.reshape(R, C, S // 2, 2, S // 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(R, S // 2, S // 2, 4 * C)


def shuffle(yu):
    """[R, P, P, (dy, dx, c)] -> [R, C, 2P, 2P]: the inverse of unshuffle."""
    R, P, _, C4 = yu.shape
    C = C4 // 4
    return yu.reshape(R, P, P, 2, 2, C).permute(0, 5, 1, 3, 2, 4).reshape(R, C, 2 * P, 2 * P)
