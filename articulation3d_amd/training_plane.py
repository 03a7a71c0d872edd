"""The plane-normal head's TRAINING step on MI355X: the plane share of the reference's third stage, config/step3_plane.yaml.

Replaces what runs when the reference trains that stage with the mask and depth heads frozen (configs/step3_planehead.yaml):
  * `PlaneRCNN.forward` with `self.training` (pkg/modeling/meta_arch/planercnn.py:83-123): the frozen detector in training mode, its
    RPN losses dropped, `_forward_box` reporting loss_cls / loss_box_reg without gradient (roi_heads.py:190-204);
  * `select_foreground_proposals` + `_forward_plane` (roi_heads.py:240-255) -> `PlaneRCNNConvFCHead.forward` / `plane_rcnn_loss`
    (plane_head.py:71-124: an L1 sum over the foreground rows' unit normals divided by the row count) and autograd's backward pass
    through the plane head only;  * SGD over roi_heads.plane_head.*.

Design:
  * Frozen detector, foreground rows, flat buffers, exchange, SGD, exports and the 3x3 tower chain are `training_head.HeadTrainer`'s,
    shared with the axis and mask stages; this module holds the plane head's layer table, the FC's and the predictor's reference
    layout, the plane ground truth and the head's body.
  * The four 3x3 layers and the 50176 -> 1024 FC run as the axis head's R tower does (precision 0 with a3d_conv_desc.m_dev, the FC's
    columns in HWC order).  The 1024 -> 3 predictor is NOT a padded 32-row layer here: a3d_plane_loss is predictor + F.normalize + loss
    + the backward pass of all three in one pass over the FC's activation (csrc/plane_train.hip).
  * 53.7 M parameters (four 3x3 convs, the FC, the predictor's 3 x 1024 + 3 behind them) in the flat buffers; one stream; the gradient
    exchange leaves in one segment.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops, train_ops as T
from .ops import ACT_RELU
from .training import SolverCfg, _Layer
from .training_head import HeadTrainer, fc_columns_to_chw, fc_columns_to_hwc

PH = "roi_heads.plane_head."
FC_DIM = 1024


def plane_layer_table(num_conv: int = 4, dim: int = 256, cin: int = 256, size: int = 14) -> dict:
    """The plane head's layers in flat-buffer order (the arguments of training_head.flat_layout): the 3x3 layers, the flattening FC, then
    the predictor's weights [3, 1024] and bias.  This order is the checkpoint format."""
    layers = [_Layer(f"{PH}plane_conv{k}", dim, cin if k == 1 else dim, 3, 1, 1, ACT_RELU) for k in range(1, num_conv + 1)]
    layers.append(_Layer(PH + "plane_fc1", FC_DIM, dim * size * size, 1, 1, 0, ACT_RELU))
    return dict(layers=layers, tail=[("pred_w", 3 * FC_DIM), ("pred_b", 3)])


def check_gt_planes(gt_planes, gt_boxes) -> None:
    """One row of 3 per ground-truth box, image by image."""
    assert len(gt_planes) == len(gt_boxes), "one gt_planes entry per image"
    for p, b in zip(gt_planes, gt_boxes):
        assert p.dim() == 2 and p.shape[1] == 3 and len(p) == len(b), \
            f"one gt_planes row of 3 per ground-truth box: got {tuple(p.shape)} for {len(b)} boxes"


class PlaneTrainer(HeadTrainer):
    """One training step of the configs/step3_planehead.yaml configuration (see HeadTrainer): the SGD update of roi_heads.plane_head.*;
    the loss kernel is fp32.  `forward_backward(frames_u8, gt_boxes, gt_classes, gt_planes)`: per image gt_planes [G, 3] (normal x
    offset; the loss normalises it when ROI_PLANE_HEAD.NORMAL_ONLY); the losses gain loss_plane."""

    PREFIX = PH

    def __init__(self, model, solver: Optional[SolverCfg] = None, seed: int = 2020, process_group=None, precision: str = "bf16x3",
                 grad_payload: Optional[str] = None, storage: Optional[str] = None, grad_overlap: Optional[str] = None,
                 loss_weight: Optional[float] = None):
        rh = model.roi_heads
        pp, ph = rh.plane_pooler, rh.plane_head
        self.pool_size, self.pool_ratio, self.pool_aligned, self.pool_scales = pp.output_size, pp.sampling_ratio, pp.aligned, list(pp.scales)
        self.in_features = list(rh.in_features)
        self.num_conv = len(ph.conv_norm_relus)
        self.dim = ph.conv_norm_relus[-1].weight.shape[0]
        assert self.num_conv >= 1 and len(ph.fcs) == 1 and ph.fcs[0].out_features == FC_DIM and ph.param_pred.out_features == 3 \
            and ph.fcs[0].in_features == self.dim * self.pool_size ** 2, "the plane head of the reference's configs"
        self.loss_weight = float(ph._loss_weight if loss_weight is None else loss_weight)
        self.normal_only = bool(ph._plane_normal_only)
        self.convs = [f"{PH}plane_conv{k}" for k in range(1, self.num_conv + 1)]
        self.kernel_events = None  # a list: every step appends 3 events: before / behind a3d_plane_loss / behind the predictor section (tools/train_plane_bench.py)
        super().__init__(model, solver, seed, process_group, precision, grad_payload, storage, grad_overlap)

    @staticmethod
    def batch_extras(batched_inputs) -> tuple:
        gt = [x["instances"].gt_planes.float() for x in batched_inputs]
        check_gt_planes(gt, [x["instances"].gt_boxes.tensor for x in batched_inputs])  # (refused before a trainer is built)
        return (gt,)

    def _layer_table(self) -> dict:
        return plane_layer_table(self.num_conv, self.dim, self.model.roi_heads.plane_head.conv_norm_relus[0].weight.shape[1], self.pool_size)

    def _allocate(self, layers, **table):
        super()._allocate(layers, **table)
        self.pred_off = off = self.layout.tail["pred_w"][0]
        assert off % 4 == 0  # (a3d_plane_loss reads the predictor's weights as 16-byte vectors)
        n = 3 * FC_DIM
        self.pred_w, self.pred_b = self.params[off:off + n].view(3, FC_DIM), self.params[off + n:off + n + 3]
        self.pred_grad = self.grads[off:off + n + 3]  # dw | db
        self._loss_out = torch.zeros(n + 4, device=self.dev)  # a3d_plane_loss: dw | db | loss

    # ------------------------------------------------------------------------------------------ reference layout
    def _odd_views(self, ly: _Layer, w, b):
        # the FC: columns stored in the HWC order of the NHWC activations, the reference's are CHW
        return [(ly.name + ".weight", fc_columns_to_chw(w, self.dim, self.pool_size)), (ly.name + ".bias", b)]

    def _load_odd(self, ly: _Layer, sd):
        ly.w.copy_(fc_columns_to_hwc(sd[ly.name + ".weight"].to(self.dev).float(), self.dim, self.pool_size))
        ly.b.copy_(sd[ly.name + ".bias"].to(self.dev))

    def _views(self, buf):
        o, n = self.pred_off, 3 * FC_DIM
        return super()._views(buf) + [(PH + "param_pred.weight", buf[o:o + n].view(3, FC_DIM)), (PH + "param_pred.bias", buf[o + n:o + n + 3])]

    @torch.no_grad()
    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self.pred_w.copy_(sd[PH + "param_pred.weight"].to(self.dev).float().reshape(3, FC_DIM))
        self.pred_b.copy_(sd[PH + "param_pred.bias"].to(self.dev).float().reshape(3))

    # ------------------------------------------------------------------------------------------ the head
    def _ground_truth(self, frames_u8, gt_boxes, gt_planes):
        """The plane parameters of a batch as one [B, max_gt, 3] tensor on the device (a malformed batch is refused before anything runs)."""
        check_gt_planes(gt_planes, gt_boxes)
        G = max(self.s.max_gt, max(len(p) for p in gt_planes))
        out = torch.zeros(len(gt_boxes), G, 3)
        for i, p in enumerate(gt_planes):
            out[i, : len(p)] = p.detach().float().cpu()
        return out.to(self.dev, non_blocking=True)

    def _predictor(self, losses, h, live, fgd, gt_planes):
        """The 1024 -> 3 predictor, the normalisation, the loss and the backward pass of all three over h [M, 1024]: fills the predictor's
        gradient and losses["loss_plane"] -> (dh [M, 1024] gated by h > 0, raw [M, 3])."""
        n = 3 * FC_DIM
        raw = torch.empty(h.shape[0], 3, device=self.dev)  # (rows past the live count stay unwritten, like dh)
        ev = self.kernel_events is not None  # (start, behind the launch pair, behind the two small copies that follow it)
        if ev:
            k = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            k[0].record()
        out, dh = T.plane_loss(h, self.pred_w, self.pred_b, live, fgd["row_img"], fgd["row_gt"], gt_planes, loss_weight=self.loss_weight,
                               normal_only=self.normal_only, out=self._loss_out, raw=raw)
        if ev:
            k[1].record()
        self.pred_grad.copy_(out[: n + 3])
        losses["loss_plane"] = out[n + 3].clone()
        if ev:
            k[2].record()
            self.kernel_events.append(tuple(k))
        return dh, raw

    def _head(self, losses, aux, fgd, live, live_px, pooled, gt_planes):
        M, fc = pooled.shape[0], self.layers[PH + "plane_fc1"]
        # ---- forward
        acts = self._tower_forward(self.convs, pooled, live_px)
        xf = acts[-1].view(M, 1, 1, fc.cin)
        h = self._conv(xf, fc.fwd(), live, splitk=ops.choose_splitk(M, FC_DIM, fc.cin))
        self._mark("plane_forward")
        # ---- predictor + normalise + loss + backward of all three, then the FC and the 3x3 layers
        dh, raw = self._predictor(losses, h.view(M, FC_DIM), live, fgd, gt_planes)
        dh = dh.view(M, 1, 1, FC_DIM)
        self._wgrad(fc, xf, dh, live)
        dx = self._conv(dh, fc.bwd(), live, gate=xf).view(M, self.pool_size, self.pool_size, self.dim)
        self._tower_backward(self.convs, acts, dx, live_px)
        self._segment_ready(0, torch.cuda.current_stream())
        self._mark("plane_backward")
        aux.update(raw_plane=raw, gt_planes=gt_planes)
