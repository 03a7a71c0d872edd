"""The articulation-axis head's TRAINING step on MI355X: the reference's second stage, config/step2_axis.yaml.

Replaces what runs when the reference trains that stage (tools/train_net.py -> detectron2 DefaultTrainer with
MODEL.FREEZE = [backbone, proposal_generator, roi_heads.box_head, roi_heads.box_predictor]):
  * `PlaneRCNN.forward` with `self.training` (pkg/modeling/meta_arch/planercnn.py:83-123): the frozen detector runs in training mode
    (training proposal counts, ROI sampling) and its RPN losses are dropped;  `_forward_box` (roi_heads.py:190-204) reports loss_cls /
    loss_box_reg without gradient;
  * `select_foreground_proposals` + `_forward_axis` (roi_heads.py:257-273) + `PlaneRCNNConvFCHead.forward` / `axis_loss`
    (axis_head.py:95-201) and autograd's backward pass through the axis head only;  * SGD over roi_heads.axis_head.*.

Design:
  * The frozen detector is a `DetectorTrainer` driven through `frozen_forward`: the same launches, precision, storage and ROI sampling
    seed as stage 1's step, so the detector this stage sees is exactly the one stage 1 trained.
  * The foreground rows (sampled class < num_classes, in sample order) are compacted on the device into a buffer of B x 128 rows
    (`roi_batch_per_image * roi_positive_fraction`, `training_head.foreground_rows`) -- nothing waits for the host.  Every launch of
    the head takes the live count: the forward and data-gradient convs through a3d_conv_desc.m_dev (the fp32-input MFMA form, the one
    kernel form that honours it), the weight gradients through a3d_wgrad_desc.p_dev (in the step's precision), the bias gradients
    through a3d_colsum_rows.  Dead rows cost nothing and are never read.
  * The 107.5 M trainable parameters (eight 3x3 convs, two 50176 -> 1024 FCs whose columns are permuted CHW -> HWC as the inference
    `Linear(chw=...)` does, rotation | offset fused to one 1024 -> 3 layer, translation) live in `training_head.HeadTrainer`'s flat
    buffers, R tower then T.  The T tower runs beside the R tower on side stream 1; the gradient exchange leaves in two segments, one
    per tower.  This module holds only what is the axis head's own: its layer table, the FC's and the fused layers' reference layout,
    the axis ground truth, and the head's forward / loss / backward body.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import ops, train_ops as T
from .ops import ACT_NONE, ACT_RELU
from .streams import adopt, hop, side as side_stream
from .training import SolverCfg, _Layer
from .training_head import HeadTrainer, fc_columns_to_chw, fc_columns_to_hwc

AXIS_TOWER_STREAM = os.environ.get("A3D_TRAIN_AXIS_STREAM", "1") != "0"  # the T tower on a second stream beside R (same bits)
AH = "roi_heads.axis_head."
P14 = 14
POOLED = 256 * P14 * P14  # 50176
CONVS = {t: [f"{AH}axis_{t}_conv{k}" for k in range(1, 5)] for t in ("R", "T")}
LAST = {"R": AH + "rot", "T": AH + "tran"}


def axis_layer_table() -> dict:
    """The axis head's layers in flat-buffer order (the arguments of training_head.flat_layout): the R tower, then the T tower."""
    layers = []
    for t in ("R", "T"):
        layers += [_Layer(n, 256, 256, 3, 1, 1, ACT_RELU) for n in CONVS[t]]
        layers.append(_Layer(f"{AH}axis_{t}_fc1", 1024, POOLED, 1, 1, 0, ACT_RELU))
        # rotation | offset: one 1024 -> 3 layer, padded to 32 rows like the box predictor;  translation: 1024 -> 2
        src = [(AH + "rotation", 0, 2), (AH + "offset", 2, 1)] if t == "R" else [(AH + "translation", 0, 2)]
        layers.append(_Layer(LAST[t], 32, 1024, 1, 1, 0, ACT_NONE, sources=src))
    return dict(layers=layers, cuts=(CONVS["T"][0],))  # gradient-exchange segments, one per tower


class AxisTrainer(HeadTrainer):
    """One training step of the step2_axis configuration (see HeadTrainer): the SGD update of roi_heads.axis_head.*.
    `forward_backward(frames_u8, gt_boxes, gt_classes, gt_rot_axis, gt_tran_axis)`: per image gt_rot_axis / gt_tran_axis [G,4]
    ([sin, cos, offset, valid]: utils.opt_utils.axis_to_angle_offset); the losses gain loss_rot_axis and loss_tran_axis."""

    PREFIX = AH
    pool_size, pool_ratio, pool_aligned = P14, 0, False
    pool_scales, in_features = [0.25, 0.125, 0.0625, 0.03125], ["p2", "p3", "p4", "p5"]

    def __init__(self, model, solver: Optional[SolverCfg] = None, seed: int = 2020, process_group=None, precision: str = "bf16x3",
                 grad_payload: Optional[str] = None, storage: Optional[str] = None, grad_overlap: Optional[str] = None,
                 beta: Optional[float] = None, loss_weight: Optional[float] = None):
        ah = model.roi_heads.axis_head
        self.beta = float(ah.smooth_l1_beta if beta is None else beta)
        self.loss_weight = float(ah._loss_weight if loss_weight is None else loss_weight)
        super().__init__(model, solver, seed, process_group, precision, grad_payload, storage, grad_overlap)
        self._t_stream = side_stream(1, self.dev) if AXIS_TOWER_STREAM else None

    _layer_table = staticmethod(axis_layer_table)

    @staticmethod
    def batch_extras(batched_inputs) -> tuple:
        return ([x["instances"].gt_rot_axis.float() for x in batched_inputs], [x["instances"].gt_tran_axis.float() for x in batched_inputs])

    # ------------------------------------------------------------------------------------------ reference layout
    def _odd_views(self, ly: _Layer, w, b):
        if ly.sources:
            return [kv for prefix, r0, nr in ly.sources for kv in ((prefix + ".weight", w[r0:r0 + nr]), (prefix + ".bias", b[r0:r0 + nr]))]
        # the FC: columns stored in the HWC order of the NHWC activations, the reference's are CHW
        return [(ly.name + ".weight", fc_columns_to_chw(w, 256, P14)), (ly.name + ".bias", b)]

    def _load_odd(self, ly: _Layer, sd):
        if ly.sources:
            ly.w.zero_()
            ly.b.zero_()
            for prefix, r0, nr in ly.sources:
                ly.w[r0:r0 + nr] = sd[prefix + ".weight"].reshape(nr, -1).to(self.dev)
                ly.b[r0:r0 + nr] = sd[prefix + ".bias"].to(self.dev)
        else:
            ly.w.copy_(fc_columns_to_hwc(sd[ly.name + ".weight"].to(self.dev).float(), 256, P14))
            ly.b.copy_(sd[ly.name + ".bias"].to(self.dev))

    # ------------------------------------------------------------------------------------------ the head
    def _ground_truth(self, frames_u8, gt_boxes, gt_rot_axis, gt_tran_axis):
        gra = torch.zeros(len(gt_boxes), self.s.max_gt, 4)
        gta = torch.zeros(len(gt_boxes), self.s.max_gt, 4)
        for i, (r, t) in enumerate(zip(gt_rot_axis, gt_tran_axis)):
            assert len(r) == len(t) == len(gt_boxes[i]), "one gt_rot_axis / gt_tran_axis row per ground-truth box"
            gra[i, : len(r)] = r.detach().float().cpu()
            gta[i, : len(t)] = t.detach().float().cpu()
        return gra.to(self.dev, non_blocking=True), gta.to(self.dev, non_blocking=True)

    def _axis_forward(self, t, pooled, live, live_px):
        L, M = self.layers, pooled.shape[0]
        acts = self._tower_forward(CONVS[t], pooled, live_px)
        xf = acts[-1].view(M, 1, 1, POOLED)
        h = self._conv(xf, L[f"{AH}axis_{t}_fc1"].fwd(), live, splitk=ops.choose_splitk(M, 1024, POOLED))
        raw = self._conv(h, L[LAST[t]].fwd(), live)
        return acts, xf, h, raw.view(M, 32)

    def _axis_backward(self, t, acts, xf, h, draw, live, live_px):
        L, M = self.layers, xf.shape[0]
        last, fc = L[LAST[t]], L[f"{AH}axis_{t}_fc1"]
        d = draw.view(M, 1, 1, 32)
        self._wgrad(last, h, d, live)
        dh = self._conv(d, last.bwd(), live, gate=h)
        self._wgrad(fc, xf, dh, live)
        dx = self._conv(dh, fc.bwd(), live, gate=xf).view(M, P14, P14, 256)
        self._tower_backward(CONVS[t], acts, dx, live_px)

    def _beside(self, tensors, fn):
        """fn() on the T tower's stream, behind what the main stream holds now (`tensors`: what fn reads of the main stream's).  The
        frozen detector's step has ended on the main stream: its stream cursor and reusable events carry on into the head."""
        return hop(self.det, self._t_stream, tensors, self.det._next_event, fn)

    def _head(self, losses, aux, fgd, live, live_px, pooled, gt):
        main, side = torch.cuda.current_stream(), self._t_stream
        # ---- tower R on the current stream, tower T beside it
        if side is not None:
            t_out = self._beside((pooled, live, live_px), lambda: self._axis_forward("T", pooled, live, live_px))
        r_out = self._axis_forward("R", pooled, live, live_px)
        if side is None:
            t_out = self._axis_forward("T", pooled, live, live_px)
        else:
            main.wait_stream(side)
            adopt(t_out[0] + [t_out[1], t_out[2], t_out[3]], main)
        axl, d_rot, d_tran = T.axis_loss(r_out[3], t_out[3], live, fgd["row_img"], fgd["row_gt"], *gt, beta=self.beta,
                                         loss_weight=self.loss_weight)
        self._mark("axis_forward")
        losses["loss_rot_axis"], losses["loss_tran_axis"] = axl[0], axl[1]
        # ---- backward: T beside R again, each tower's gradient segment leaves when its last launch is enqueued

        def t_backward(stream):
            self._axis_backward("T", *t_out[:3], d_tran, live, live_px)
            self._segment_ready(1, stream)

        if side is not None:
            self._beside((d_tran,), lambda: t_backward(side))
        self._axis_backward("R", *r_out[:3], d_rot, live, live_px)
        self._segment_ready(0, main)
        if side is None:
            t_backward(main)
        else:
            main.wait_stream(side)
        self._mark("axis_backward")
        aux.update(raw_rot=r_out[3][:, :3], raw_tran=t_out[3][:, :2], d_rot=d_rot[:, :3], d_tran=d_tran[:, :2], gt_axes=gt)
