"""The depth head's TRAINING step on MI355X: the depth share of the reference's third stage, config/step3_plane.yaml.

Replaces what runs when the reference trains that stage with the mask and plane heads frozen (configs/step3_depth.yaml):
  * `PlaneRCNN.forward` with `self.training` (pkg/modeling/meta_arch/planercnn.py:83-123): the frozen detector in training mode, its
    RPN losses dropped, `_forward_box` reporting loss_cls / loss_box_reg without gradient (roi_heads.py:190-204);
  * `PlaneRCNNDepthHead.forward` in training mode (pkg/modeling/depth_net/depth_head.py:72-97): the U-shaped decoder over the whole
    pyramid whose ten nn.BatchNorm2d(eps 1e-3, momentum 0.01) layers normalise with BATCH statistics, the x2 bilinear upsampling and
    l1LossMask against the ground-truth depth where it exceeds 1e-4, and autograd's backward pass through the decoder only;
  * SGD over depth_head.*, the norm parameters with SOLVER.WEIGHT_DECAY_NORM.

Design:
  * The frozen detector, the flat buffers, `flat_layout`, the exchange, the exports and the public shape are `training_head.HeadTrainer`'s.
    The depth decoder has no ROI rows: the ROI prologue (foreground rows, pooling) is replaced, every pixel is live and no launch takes
    a live count.
  * A block is conv (bias, no activation, nothing folded) -> a3d_bn_train_forward.  The convs follow the trainer's `precision` as stage 1's
    do in "fp32" and "bf16x3" (the upsampling / two-source gather form runs the fp32-input MFMA: the one kernel form that has it); in
    "bf16" only the weight gradients take the bf16 arithmetic, as in every HeadTrainer (see `_dconv` for the measurement behind it).
    The batch-norm, loss and depth_pred kernels of csrc/depth_train.hip are fp32 in every precision.  z and y of every block are kept.
  * Backward: a3d_depth_loss -> a3d_depth_pred_backward -> per block a3d_bn_train_backward (the activation's derivative lives there, so
    the data-gradient convs run ungated and LeakyReLU needs nothing of the conv kernel), conv_wgrad (a deconv block's dense input is
    materialised by a3d_ups2_concat, in the backward pass only), the bias gradient as the column sum of dz, the data-gradient conv with
    the transposed filter, sumpool2, and the two channel halves of that sum read in place through a3d_bn_train_backward's row pitch.
    No data gradient flows into the frozen pyramid.  One stream; the exchange leaves in one segment.
  * 2 658 433 parameters: eleven convs, then (a 4-aligned tail range of the flat buffers) gamma / beta of the ten norms.

Data parallelism: the reference wraps the model in DistributedDataParallel(broadcast_buffers=False) around plain nn.BatchNorm2d, so
batch statistics and running buffers are PER RANK and only gradients are exchanged.  This trainer does the same: every rank normalises
with its own batch's statistics and keeps its own running_mean / running_var; `optimizer_step` averages the gradients.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import ops, train_ops as T
from .ops import ACT_LEAKY, ACT_NONE, ACT_RELU
from .training import SolverCfg, _Layer
from .training_head import HeadTrainer

DH = "depth_head."
BN_EPS, BN_MOMENTUM = 1e-3, 0.01
LEVELS = ("p6", "p5", "p4", "p3", "p2")  # conv{k}'s pyramid level, k = 1..5
# block -> (conv entry, norm entry, activation) in the reference's nn.Sequential blocks
BLOCKS = {**{f"conv{k}": (f"{DH}conv{k}.0", f"{DH}conv{k}.1", ACT_LEAKY) for k in range(1, 6)},
          **{f"deconv{k}": (f"{DH}deconv{k}.1", f"{DH}deconv{k}.2", ACT_RELU) for k in range(1, 6)}}


def depth_layer_table() -> dict:
    """The depth head's parameters in flat-buffer order (the arguments of training_head.flat_layout): the ten 3x3 convs in front of a
    norm, then in the tail depth_pred's filter [9, 64] (tap-major) and bias, padding up to a multiple of 4, and gamma / beta of the ten
    norms -- one 4-aligned range (`norm_range`) with its own weight decay.  This order is the checkpoint format."""
    layers = [_Layer(BLOCKS[f"conv{k}"][0], 128, 256, 3, 1, 1, ACT_NONE) for k in range(1, 6)]
    layers += [_Layer(BLOCKS[f"deconv{k}"][0], 64 if k == 5 else 128, 128 if k == 1 else 256, 3, 1, 1, ACT_NONE) for k in range(1, 6)]
    n = sum(ly.rows * 9 * ly.cin + ly.rows for ly in layers) + 9 * 64 + 1
    tail = [("pred_w", 9 * 64), ("pred_b", 1), ("pad", -n % 4)]
    for ly, (_, norm, _) in zip(layers, BLOCKS.values()):
        tail += [(norm + ".weight", ly.rows), (norm + ".bias", ly.rows)]
    return dict(layers=layers, tail=tail)


def norm_range(layout) -> tuple:
    """[begin, end) of the norm parameters in a depth layout: 4-aligned on both sides."""
    offs = [v for k, v in layout.tail.items() if k.startswith(DH)]
    begin, end = offs[0][0], offs[-1][0] + offs[-1][1]
    assert begin % 4 == 0 and end % 4 == 0 and end == layout.total
    return begin, end


def check_gt_depth(gt_depth, hw) -> torch.Tensor:
    """The ground-truth depth of a batch as [B, H, W] float (a [B, H, W] tensor or one [H, W] map per image), H x W the frames' size."""
    if not torch.is_tensor(gt_depth):
        assert len(gt_depth) > 0 and all(torch.is_tensor(d) and d.dim() == 2 for d in gt_depth), "gt_depth: one [H, W] depth map per image"
        assert all(tuple(d.shape) == tuple(gt_depth[0].shape) for d in gt_depth), "gt_depth: one size per batch"
        gt_depth = torch.stack([d.float() for d in gt_depth])
    assert gt_depth.dim() == 3 and tuple(gt_depth.shape[1:]) == tuple(hw), \
        f"gt_depth: [B, H, W] depth maps of the frames' size {tuple(hw)}: got {tuple(gt_depth.shape)}"
    return gt_depth.float()


class DepthTrainer(HeadTrainer):
    """One training step of the configs/step3_depth.yaml configuration (see HeadTrainer and the module docstring): the SGD update of
    depth_head.*.  `forward_backward(frames_u8, gt_boxes, gt_classes, gt_depth)`: gt_depth [B, H, W] (or one [H, W] map per image), 0
    where unknown; the losses gain depth_loss.  Batch statistics and running buffers are per rank (module docstring)."""

    PREFIX = DH

    def __init__(self, model, solver: Optional[SolverCfg] = None, seed: int = 2020, process_group=None, precision: str = "bf16x3",
                 grad_payload: Optional[str] = None, storage: Optional[str] = None, grad_overlap: Optional[str] = None,
                 loss_weight: Optional[float] = None):
        dh = model.depth_head
        self.loss_weight = float(dh._loss_weight if loss_weight is None else loss_weight)
        for blk, (conv, norm, _) in BLOCKS.items():
            seq = getattr(dh, blk)
            bn = seq[int(norm.rsplit(".", 1)[1])]
            assert isinstance(bn, torch.nn.BatchNorm2d) and bn.eps == BN_EPS and bn.momentum == BN_MOMENTUM, "the depth head of the reference"
        self.num_batches_tracked = 0
        super().__init__(model, solver, seed, process_group, precision, grad_payload, storage, grad_overlap)

    @staticmethod
    def batch_extras(batched_inputs) -> tuple:
        """planercnn.py:198-201: x["depth"], [H, W] per image, stacked (refused before a trainer is built when malformed)."""
        assert all("depth" in x for x in batched_inputs), "training the depth head needs x[\"depth\"], an [H, W] depth map per image"
        maps = [torch.as_tensor(x["depth"]) for x in batched_inputs]
        return (check_gt_depth(maps, tuple(batched_inputs[0]["image"].shape[-2:])),)

    # ------------------------------------------------------------------------------------------ parameters
    def _layer_table(self) -> dict:
        return depth_layer_table()

    def _allocate(self, layers, **table):
        super()._allocate(layers, **table)
        lay = self.layout
        self.norm_begin, self.norm_end = norm_range(lay)
        o = lay.tail["pred_w"][0]
        assert o % 4 == 0
        self.pred_w, self.pred_b = self.params[o:o + 576].view(9, 64), self.params[o + 576:o + 577]
        self.pred_grad = self.grads[o:o + 577]  # dw (tap-major) | db: a3d_depth_pred_backward writes it in place
        n_run = sum(ly.rows for ly in layers)
        self.running = torch.zeros(2, n_run, device=self.dev)  # running_mean | running_var of the ten norms, block by block
        self.norms: Dict[str, dict] = {}
        at = 0
        for ly, (blk, (_, norm, act)) in zip(layers, BLOCKS.items()):
            (og, n), (ob, _) = lay.tail[norm + ".weight"], lay.tail[norm + ".bias"]
            self.norms[blk] = dict(name=norm, act=act, gamma=self.params[og:og + n], beta=self.params[ob:ob + n], dgamma=self.grads[og:og + n],
                                   dbeta=self.grads[ob:ob + n], rm=self.running[0, at:at + n], rv=self.running[1, at:at + n])
            at += n

    @property
    def weight_decays(self) -> list:
        """The decay of the two SGD ranges: everything but the norm parameters, the norm parameters."""
        return [self.s.weight_decay, self.s.weight_decay_norm]

    def _views(self, buf):
        o = self.layout.tail["pred_w"][0]
        out = super()._views(buf) + [(DH + "depth_pred.weight", buf[o:o + 576].view(1, 3, 3, 64).permute(0, 3, 1, 2)),
                                     (DH + "depth_pred.bias", buf[o + 576:o + 577])]
        for nm in self.norms.values():
            for leaf in (".weight", ".bias"):
                og, n = self.layout.tail[nm["name"] + leaf]
                out.append((nm["name"] + leaf, buf[og:og + n]))
        return out

    @torch.no_grad()
    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        f = lambda k: sd[DH + k].to(self.dev).float()
        self.pred_w.copy_(f("depth_pred.weight").permute(0, 2, 3, 1).reshape(9, 64))
        self.pred_b.copy_(f("depth_pred.bias").reshape(1))
        for nm in self.norms.values():
            n = nm["name"]
            nm["gamma"].copy_(sd[n + ".weight"].to(self.dev).float())
            nm["beta"].copy_(sd[n + ".bias"].to(self.dev).float())
            nm["rm"].copy_(sd[n + ".running_mean"].to(self.dev).float())
            nm["rv"].copy_(sd[n + ".running_var"].to(self.dev).float())
            if n + ".num_batches_tracked" in sd:
                self.num_batches_tracked = int(sd[n + ".num_batches_tracked"])

    def export_state_dict(self) -> Dict[str, torch.Tensor]:
        """The trainable parameters AND the norms' buffers (running_mean, running_var, num_batches_tracked) under the reference's names:
        with them `model.train(False)` writes a complete depth head back."""
        out = super().export_state_dict()
        for nm in self.norms.values():
            out[nm["name"] + ".running_mean"] = nm["rm"].detach().clone()
            out[nm["name"] + ".running_var"] = nm["rv"].detach().clone()
            out[nm["name"] + ".num_batches_tracked"] = torch.tensor(self.num_batches_tracked, dtype=torch.long, device=self.dev)
        return out

    # ------------------------------------------------------------------------------------------ the decoder
    def _dconv(self, x, pk, **kw):
        """A decoder conv (forward or data gradient).  "fp32" and "bf16x3" run as stage 1's trainable convs do.  "bf16" keeps
        HeadTrainer's rule -- only the weight gradients take the bf16 arithmetic, these launches run the fp32-input MFMA: with the
        plain layers' forward pass in bf16 (measured on the 160 x 192 decoder case) pre-activations move by 4e-3, about 0.3 % of the
        activation gates land on the other side of their kink and every gradient below them is 6e-2 to 8e-2 off float64, past the
        5e-2 the bf16 step is held to."""
        prec = self.det.prec
        return ops.conv2d(x, pk, precision=0 if prec == 1 else prec, **kw)

    def _block(self, blk, x, x2=None, ups=False, train_stats=True):
        ly, nm = self.layers[BLOCKS[blk][0]], self.norms[blk]
        z = self._dconv(x, ly.fwd(), x2=x2, ups=ups)
        y, mean, invstd, _ = T.bn_train_forward(z, nm["gamma"], nm["beta"], act=nm["act"], eps=BN_EPS, momentum=BN_MOMENTUM,
                                                running_mean=nm["rm"] if train_stats else None, running_var=nm["rv"] if train_stats else None)
        return dict(x=x, x2=x2, z=z, y=y, mean=mean, invstd=invstd)

    def _block_backward(self, blk, a, dy, dy_off=0, data_grad=True):
        """Backward of a block given dy, the gradient of its output (the channel slice at dy_off of dy's rows): fills the block's
        gradients -> the gradient of the conv's input [B, H', W', cin] (a deconv block: of the UPSAMPLED concat), or None."""
        ly, nm = self.layers[BLOCKS[blk][0]], self.norms[blk]
        dz = T.bn_train_backward(dy, a["z"], a["y"], a["mean"], a["invstd"], nm["gamma"], act=nm["act"], dgamma=nm["dgamma"], dbeta=nm["dbeta"],
                                 dy_off=dy_off)
        xin = T.ups2_concat(a["x"], a["x2"]) if blk.startswith("deconv") else a["x"]
        T.conv_wgrad(xin, dz, ly.dw, KH=3, KW=3, stride=1, pad=1, precision=self.wgrad_prec)
        T.colsum(dz, ly.db)
        return self._dconv(dz, ly.bwd()) if data_grad else None

    def _decoder(self, feats, gt, train_stats=True):
        """depth_head.py:80-89 in training mode on the pyramid + the loss + the backward pass -> (depth_loss, aux entries)."""
        saved_sk, ops.BF16_SPLITK_AUTO = ops.BF16_SPLITK_AUTO, True
        try:
            f = {n: (feats[n] if feats[n].dtype == torch.float32 else feats[n].float()).contiguous() for n in LEVELS}
            B, hp, wp = f["p2"].shape[:3]
            assert tuple(gt.shape) == (B, 4 * hp, 4 * wp), f"gt_depth {tuple(gt.shape)} against a prediction of {(B, 4 * hp, 4 * wp)}"
            # ---- forward
            A = {"conv1": self._block("conv1", f["p6"], train_stats=train_stats)}
            A["deconv1"] = self._block("deconv1", A["conv1"]["y"], ups=True, train_stats=train_stats)
            x = A["deconv1"]["y"]
            h5, w5 = f["p5"].shape[1:3]
            resized = (x.shape[1], x.shape[2]) != (h5, w5)
            if resized:
                x = ops.resize_bilinear(x, h5, w5)  # depth_head.py:82
            for k in range(2, 6):
                A[f"conv{k}"] = self._block(f"conv{k}", f[LEVELS[k - 1]], train_stats=train_stats)
                A[f"deconv{k}"] = self._block(f"deconv{k}", A[f"conv{k}"]["y"], x2=x, ups=True, train_stats=train_stats)
                x = A[f"deconv{k}"]["y"]
            d = ops.conv3x3_to1(x, self.pred_w, 0.0)
            d += self.pred_b  # (the bias is a device parameter here)
            self._mark("depth_forward")
            # ---- loss and backward
            out, dd = T.depth_loss(d, gt, loss_weight=self.loss_weight)
            _, dx = T.depth_pred_backward(x, dd, self.pred_w, out=self.pred_grad)
            off = 0
            for k in range(5, 1, -1):
                dcat = self._block_backward(f"deconv{k}", A[f"deconv{k}"], dx, off)  # [B, 2h, 2w, 256]
                hk, wk = A[f"conv{k}"]["y"].shape[1:3]
                dx = T.sumpool2_add(dcat, torch.zeros((B, hk, wk, dcat.shape[3]), device=self.dev))  # the upsampling's adjoint
                del dcat
                self._block_backward(f"conv{k}", A[f"conv{k}"], dx, 0, data_grad=False)  # the first 128 channels: conv{k}'s output
                off = 128  # the rest: the previous decoder block's output
            dx = dx[..., 128:].contiguous()  # [B, h5, w5, 128] (small: the p5 level)
            if resized:
                dx = T.resize_bilinear_backward(dx, A["deconv1"]["y"].shape[1], A["deconv1"]["y"].shape[2])
            dcat = self._block_backward("deconv1", A["deconv1"], dx)
            h6, w6 = f["p6"].shape[1:3]
            dx = T.sumpool2_add(dcat, torch.zeros((B, h6, w6, dcat.shape[3]), device=self.dev))
            self._block_backward("conv1", A["conv1"], dx, data_grad=False)
            self._segment_ready(0, torch.cuda.current_stream())
            self._mark("depth_backward")
        finally:
            ops.BF16_SPLITK_AUTO = saved_sk
        return out[0], dict(depth_pred=d, depth_valid=out[1], depth_acts=A, gt_depth=gt)

    @torch.no_grad()
    def decoder_forward_backward(self, feats: Dict[str, torch.Tensor], gt_depth, update_running: bool = True):
        """The decoder alone on a bare pyramid {p2..p6: [B, h, w, 256] NHWC} against gt_depth [B, 16 h_p2 / 4, ...] = 4 x p2's size:
        fills self.grads -> (depth_loss, aux).  What `forward_backward` runs behind the frozen detector; tests drive it at small sizes."""
        hp, wp = feats["p2"].shape[1:3]
        gt = check_gt_depth(gt_depth, (4 * hp, 4 * wp)).to(self.dev).contiguous()
        self._grad_scale = 1.0
        self._begin_head(False)
        if update_running:
            self.num_batches_tracked += 1
        return self._decoder(feats, gt, train_stats=update_running)

    # ------------------------------------------------------------------------------------------ the step
    def _ground_truth(self, frames_u8, gt_boxes, gt_depth):
        return check_gt_depth(gt_depth, tuple(frames_u8.shape[1:3])).to(self.dev, non_blocking=True).contiguous()

    def forward_backward(self, frames_u8: torch.Tensor, gt_boxes: Sequence[torch.Tensor], gt_classes: Sequence[torch.Tensor], gt_depth, *,
                         samples: Optional[dict] = None, exchange: bool = False):
        """HeadTrainer.forward_backward without the ROI prologue: ({loss_cls, loss_box_reg, depth_loss}, aux).  The ground truth is
        checked before anything runs."""
        gt = self._ground_truth(frames_u8, gt_boxes, gt_depth)
        assert gt.shape[0] == frames_u8.shape[0], "one depth map per frame"
        box_l, aux = self._frozen_step(frames_u8, gt_boxes, gt_classes, samples)
        self._mark("frozen_forward")
        self._begin_head(exchange)
        self.num_batches_tracked += 1
        losses = dict(box_l)
        losses["depth_loss"], extra = self._decoder(aux["feats"], gt)
        aux.update(extra)
        return losses, aux

    def _sgd(self, lr: float, scale: float):
        """detectron2's build_optimizer: norm parameters decay with WEIGHT_DECAY_NORM, everything else with WEIGHT_DECAY -- two launches
        over the two 4-aligned ranges of the flat buffers."""
        s, a, b = self.s, self.norm_begin, self.norm_end
        for lo, hi, wd in ((0, a, s.weight_decay), (a, b, s.weight_decay_norm)):
            T.sgd_momentum(self.params[lo:hi], self.grads[lo:hi], self.momentum[lo:hi], lr=lr, momentum=s.momentum, weight_decay=wd,
                           grad_scale=scale, first=self.iter == 0)
