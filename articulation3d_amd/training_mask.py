"""The mask head's TRAINING step on MI355X: the mask share of the reference's third stage, config/step3_plane.yaml.

Replaces what runs when the reference trains that stage with the plane and depth heads frozen (configs/step3_mask.yaml):
  * `PlaneRCNN.forward` with `self.training` (pkg/modeling/meta_arch/planercnn.py:83-123): the frozen detector in training mode, its
    RPN losses dropped, `_forward_box` reporting loss_cls / loss_box_reg without gradient (roi_heads.py:190-204);
  * `select_foreground_proposals` + `_forward_mask` (roi_heads.py:218-238) -> detectron2's MaskRCNNConvUpsampleHead and `mask_rcnn_loss`
    for a class-agnostic head with bitmask ground truth (gt_masks.crop_and_resize(proposal_boxes, 28), BCE-with-logits, mean), and
    autograd's backward pass through the mask head only;  * SGD over roi_heads.mask_head.*.

Design:
  * Frozen detector, foreground rows, flat buffers, exchange, SGD and exports are `training_head.HeadTrainer`'s, shared with the axis
    stage; this module holds the mask head's layer table, the deconv's reference layout, the mask upload and the head's body.
  * The four 3x3 layers run as in the axis towers (precision 0 with a3d_conv_desc.m_dev).  The 2x2 stride-2 deconv runs as a plain 1x1
    convolution with 1024 output channels (dy, dx, co) and ReLU, WITHOUT the pixel shuffle of inference: the predictor is per pixel, and
    the gated transposed-filter data gradient takes the plain layout only.
  * a3d_mask_targets writes the 28 x 28 targets of the live rows; a3d_mask_loss is predictor + loss + backward in one pass over the
    unshuffled activation (csrc/mask_train.hip).
  * 2.6 M parameters (four 3x3 convs, the deconv as [(dy, dx, co), ci] with its 256 biases, the predictor's 256 + 1) in the flat buffers;
    one stream; the gradient exchange leaves in one segment.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import train_ops as T
from .ops import ACT_RELU
from .structures import gt_bitmasks
from .training import SolverCfg, _Layer
from .training_head import HeadTrainer

MH = "roi_heads.mask_head."


def deconv_to_packed(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d(k 2, s 2) weight (or its gradient) [Cin, Cout, 2, 2] -> the 1x1 layer's rows [(dy, dx, co), ci], the order of
    ops.pack_deconv2x2."""
    Cin, Cout = w.shape[:2]
    return w.permute(2, 3, 1, 0).reshape(4 * Cout, Cin)


def deconv_from_packed(p: torch.Tensor) -> torch.Tensor:
    """[(dy, dx, co), ci] -> [Cin, Cout, 2, 2]: the inverse of deconv_to_packed (weights and gradients alike: a permutation)."""
    Cout, Cin = p.shape[0] // 4, p.shape[1]
    return p.reshape(2, 2, Cout, Cin).permute(3, 2, 0, 1)


def deconv_bias_fold(db4: torch.Tensor) -> torch.Tensor:
    """The bias gradient of the four (dy, dx) column groups [(dy, dx, co)] -> [co]: the deconv has ONE bias per output channel."""
    g = db4.reshape(4, -1)
    return (g[0] + g[1]) + (g[2] + g[3])


def mask_layer_table(num_conv: int = 4, dim: int = 256, cin: int = 256) -> dict:
    """The mask head's layers in flat-buffer order (the arguments of training_head.flat_layout): the 3x3 layers, the deconv as a 1x1
    layer of 4 x dim rows with ONE bias per output channel, then the predictor's weights and bias."""
    layers = [_Layer(f"{MH}mask_fcn{k}", dim, cin if k == 1 else dim, 3, 1, 1, ACT_RELU) for k in range(1, num_conv + 1)]
    layers.append(_Layer(MH + "deconv", 4 * dim, dim, 1, 1, 0, ACT_RELU))
    return dict(layers=layers, bias_rows={MH + "deconv": dim}, tail=[("pred_w", dim), ("pred_b", 1)])


class MaskTrainer(HeadTrainer):
    """One training step of the configs/step3_mask.yaml configuration (see HeadTrainer): the SGD update of roi_heads.mask_head.*; the
    target and loss kernels are fp32.  `forward_backward(frames_u8, gt_boxes, gt_classes, gt_masks)`: per image gt_masks [G,H,W] bool /
    uint8 (or a structures.BitMasks); the losses gain loss_mask."""

    PREFIX = MH

    def __init__(self, model, solver: Optional[SolverCfg] = None, seed: int = 2020, process_group=None, precision: str = "bf16x3",
                 grad_payload: Optional[str] = None, storage: Optional[str] = None, grad_overlap: Optional[str] = None):
        rh = model.roi_heads
        mp, mh = rh.mask_pooler, rh.mask_head
        self.pool_size, self.pool_ratio, self.pool_aligned, self.pool_scales = mp.output_size, mp.sampling_ratio, mp.aligned, list(mp.scales)
        self.in_features = list(rh.in_features)
        self.num_conv = len(mh.conv_norm_relus)
        self.dim = mh.predictor.weight.shape[1]
        assert self.num_conv >= 1 and self.dim == 256 and mh.deconv.weight.shape[0] == self.dim, "the mask head of the reference's configs"
        self.fcn = [f"{MH}mask_fcn{k}" for k in range(1, self.num_conv + 1)]
        self.kernel_events = None  # a list: every step appends (start, end) events around a3d_mask_loss (tools/train_mask_bench.py)
        super().__init__(model, solver, seed, process_group, precision, grad_payload, storage, grad_overlap)

    @staticmethod
    def batch_extras(batched_inputs) -> tuple:
        return ([gt_bitmasks(x["instances"].gt_masks) for x in batched_inputs],)  # (polygon ground truth: NotImplementedError)

    def _layer_table(self) -> dict:
        return mask_layer_table(self.num_conv, self.dim, self.model.roi_heads.mask_head.conv_norm_relus[0].weight.shape[1])

    def _allocate(self, layers, **table):
        super()._allocate(layers, **table)
        C, dec = self.dim, self.layers[MH + "deconv"]
        # the deconv's bias is ONE value per output channel: the 1x1 layer reads it repeated over the four (dy, dx) groups, and its
        # gradient is the fold of the four groups' column sums (both scratch, outside the flat buffers)
        self.deconv_b, self.deconv_db = dec.b, dec.db
        dec.b, dec.db = self._b4, self._db4 = torch.zeros(4 * C, device=self.dev), torch.zeros(4 * C, device=self.dev)
        self.pred_off = off = self.layout.tail["pred_w"][0]
        assert off % 4 == 0  # (a3d_mask_loss reads the predictor's weights as 16-byte vectors)
        self.pred_w, self.pred_b = self.params[off:off + C], self.params[off + C:off + C + 1]
        self.pred_grad = self.grads[off:off + C + 1]  # dw | db
        self._loss_out = torch.zeros(C + 2, device=self.dev)  # a3d_mask_loss: dw | db | loss

    # ------------------------------------------------------------------------------------------ reference layout
    def _odd_views(self, ly: _Layer, w, b):
        return [(ly.name + ".weight", deconv_from_packed(w)), (ly.name + ".bias", b)]

    def _load_odd(self, ly: _Layer, sd):
        ly.w.copy_(deconv_to_packed(sd[ly.name + ".weight"].to(self.dev).float()))
        self.deconv_b.copy_(sd[ly.name + ".bias"].to(self.dev))

    def _views(self, buf):
        o, C = self.pred_off, self.dim
        return super()._views(buf) + [(MH + "predictor.weight", buf[o:o + C].view(1, C, 1, 1)), (MH + "predictor.bias", buf[o + C:o + C + 1])]

    @torch.no_grad()
    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self.pred_w.copy_(sd[MH + "predictor.weight"].to(self.dev).float().reshape(self.dim))
        self.pred_b.copy_(sd[MH + "predictor.bias"].to(self.dev).float().reshape(1))

    # ------------------------------------------------------------------------------------------ the head
    def _ground_truth(self, frames_u8, gt_boxes, gt_masks):
        """The bitmasks of a batch as one uint8 [B, G, H, W] on the device (refuses polygons before anything runs)."""
        B, hw = len(gt_masks), tuple(frames_u8.shape[1:3])
        ms = [gt_bitmasks(m) for m in gt_masks]
        for m, b in zip(ms, gt_boxes):
            assert len(m) == len(b), "one gt_masks entry per ground-truth box"
            assert len(m) == 0 or tuple(m.shape[1:]) == hw, f"gt_masks at the image's resolution {hw}, got {tuple(m.shape[1:])}"
        G = max(1, max(len(m) for m in ms))
        out = torch.zeros((B, G, hw[0], hw[1]), device=self.dev, dtype=torch.uint8)
        for i, m in enumerate(ms):
            if len(m):
                out[i, : len(m)] = m.to(self.dev, non_blocking=True).to(torch.uint8)
        return out

    def _head(self, losses, aux, fgd, live, live_px, pooled, masks):
        C, dec = self.dim, self.layers[MH + "deconv"]
        self._b4.copy_(self.deconv_b.repeat(4))
        # ---- forward
        acts = self._tower_forward(self.fcn, pooled, live_px)
        x = acts[-1]
        yu = self._conv(x, dec.fwd(), live_px)  # [M, P, P, (dy, dx, co)]: the deconv's output after ReLU, unshuffled
        targets = T.mask_targets(masks, fgd["boxes"], fgd["count"], fgd["row_offset"], fgd["row_gt"], live, rows=pooled.shape[0],
                                 size=2 * self.pool_size)
        self._mark("mask_forward")
        # ---- predictor + loss + backward of both, then the deconv and the 3x3 layers
        if self.kernel_events is not None:
            k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            k0.record()
        out, dyu = T.mask_loss(yu, targets, self.pred_w, self.pred_b, live, out=self._loss_out)
        if self.kernel_events is not None:
            k1.record()
            self.kernel_events.append((k0, k1))
        self.pred_grad.copy_(out[: C + 1])
        losses["loss_mask"] = out[C + 1].clone()
        self._wgrad(dec, x, dyu, live_px)
        self.deconv_db.copy_(deconv_bias_fold(self._db4))
        self._tower_backward(self.fcn, acts, self._conv(dyu, dec.bwd(), live_px, gate=x), live_px)
        self._segment_ready(0, torch.cuda.current_stream())
        self._mark("mask_backward")
        aux.update(mask_targets=targets, gt_masks=masks)
