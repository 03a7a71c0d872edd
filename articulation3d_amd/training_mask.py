"""The mask head's TRAINING step on MI355X: the mask share of the reference's third stage, config/step3_plane.yaml.

Replaces what runs when the reference trains that stage with the plane and depth heads frozen (configs/step3_mask.yaml):
  * `PlaneRCNN.forward` with `self.training` (pkg/modeling/meta_arch/planercnn.py:83-123): the frozen detector in training mode, its
    RPN losses dropped, `_forward_box` reporting loss_cls / loss_box_reg without gradient (roi_heads.py:190-204);
  * `select_foreground_proposals` + `_forward_mask` (roi_heads.py:218-238) -> detectron2's MaskRCNNConvUpsampleHead and `mask_rcnn_loss`
    for a class-agnostic head with bitmask ground truth (gt_masks.crop_and_resize(proposal_boxes, 28), BCE-with-logits, mean), and
    autograd's backward pass through the mask head only;  * SGD over roi_heads.mask_head.*.

Design:
  * Frozen detector and foreground rows are the axis stage's (`DetectorTrainer.frozen_forward`, `training_axis.foreground_rows`): compact
    rows, per-image counts, row offsets and the live total stay on the device, and every launch of the head takes the live count.
  * The four 3x3 layers run as in the axis towers (precision 0 with a3d_conv_desc.m_dev).  The 2x2 stride-2 deconv runs as a plain 1x1
    convolution with 1024 output channels (dy, dx, co) and ReLU, WITHOUT the pixel shuffle of inference: the predictor is per pixel, and
    the gated transposed-filter data gradient takes the plain layout only.
  * a3d_mask_targets writes the 28 x 28 targets of the live rows; a3d_mask_loss is predictor + loss + backward in one pass over the
    unshuffled activation (csrc/mask_train.hip).
  * 2.6 M parameters (four 3x3 convs, the deconv as [(dy, dx, co), ci] with its 256 biases, the predictor's 256 + 1) in one flat buffer,
    gradients and momenta beside it; one stream; the gradient exchange leaves in one segment.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import ops, train_ops as T
from .ops import ACT_RELU
from .parallel import GradientExchange, allreduce_gradients
from .structures import gt_bitmasks
from .training import DetectorTrainer, SolverCfg, _Layer, lr_at
from .training_axis import foreground_rows

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


class MaskTrainer:
    """One training step of the configs/step3_mask.yaml configuration: the frozen detector's forward pass, the mask head's forward and
    backward pass over the compacted foreground rows, the mask loss and the SGD update of roi_heads.mask_head.* -- all on the device.

    Precision.  The frozen detector runs in `precision` exactly as DetectorTrainer does.  In the mask head only the weight gradients follow
    it; forward and data-gradient launches run the fp32-input MFMA in every precision (the one conv kernel form that honours a live row
    count), and the target and loss kernels are fp32.

    Public shape of `AxisTrainer`: forward_backward, optimizer_step, step, load_state_dict, export_state_dict, export_grads,
    autograd_anchor, the `samples=` hook and `phase_events`."""

    def __init__(self, model, solver: Optional[SolverCfg] = None, seed: int = 2020, process_group=None, precision: str = "bf16x3",
                 grad_payload: Optional[str] = None, storage: Optional[str] = None, grad_overlap: Optional[str] = None):
        self.det = DetectorTrainer(model, solver, seed=seed, process_group=process_group, precision=precision, storage=storage)
        self.s, self.model, self.dev, self.pg = self.det.s, model, self.det.dev, process_group
        self.precision = precision
        self.wgrad_prec = self.det.wgrad_prec
        self.grad_payload = grad_payload or ("bf16" if precision == "bf16" else "fp32")
        self.grad_overlap = self.det.grad_overlap if grad_overlap is None else str(grad_overlap)
        rh = model.roi_heads
        mp, mh = rh.mask_pooler, rh.mask_head
        self.pool_size, self.pool_ratio, self.pool_aligned, self.pool_scales = mp.output_size, mp.sampling_ratio, mp.aligned, list(mp.scales)
        self.in_features = list(rh.in_features)
        self.num_conv = len(mh.conv_norm_relus)
        self.dim = mh.predictor.weight.shape[1]
        assert self.num_conv >= 1 and self.dim == 256 and mh.deconv.weight.shape[0] == self.dim, "the mask head of the reference's configs"
        self.cap = int(self.s.roi_batch_per_image * self.s.roi_positive_fraction)  # foreground rows per image at most (128)
        self.iter = 0
        self._xchg: Optional[GradientExchange] = None
        self._xchg_live = False
        self._grad_scale = 1.0
        self.phase_events = None  # a list: every step appends (name, event recorded on the main stream) at its phase boundaries
        self.kernel_events = None  # a list: every step appends (start, end) events around a3d_mask_loss (tools/train_mask_bench.py)
        self._build_layers({k: v.detach().float() for k, v in model.state_dict().items() if k.startswith(MH)})

    # ------------------------------------------------------------------------------------------ parameters
    def _build_layers(self, sd):
        C = self.dim
        L: Dict[str, _Layer] = {}
        cin = self.model.roi_heads.mask_head.conv_norm_relus[0].weight.shape[1]
        for k in range(1, self.num_conv + 1):
            n = f"{MH}mask_fcn{k}"
            L[n] = _Layer(n, C, cin if k == 1 else C, 3, 1, 1, ACT_RELU)
        L[MH + "deconv"] = _Layer(MH + "deconv", 4 * C, C, 1, 1, 0, ACT_RELU)
        self.layers = L
        n = sum(ly.rows * ly.k * ly.k * ly.cin for ly in L.values()) + self.num_conv * C + C + C + 1
        n = (n + 3) // 4 * 4
        self.params = torch.zeros(n, device=self.dev)
        self.grads = torch.zeros(n, device=self.dev)
        self.momentum = torch.zeros(n, device=self.dev)
        self._wt = torch.empty(sum(ly.rows * ly.k * ly.k * ly.cin for ly in L.values()), device=self.dev)
        # the deconv's bias is ONE value per output channel: the 1x1 layer reads it repeated over the four (dy, dx) groups, and its
        # gradient is the fold of the four groups' column sums (both scratch, outside the flat buffers)
        self._b4 = torch.zeros(4 * C, device=self.dev)
        self._db4 = torch.zeros(4 * C, device=self.dev)
        off = woff = 0
        for ly in L.values():
            nwl = ly.rows * ly.k * ly.k * ly.cin
            ly.w, ly.dw = self.params[off:off + nwl].view(ly.rows, -1), self.grads[off:off + nwl].view(ly.rows, -1)
            off += nwl
            if ly.k == 3:
                ly.b, ly.db = self.params[off:off + ly.rows], self.grads[off:off + ly.rows]
                off += ly.rows
            else:
                self.deconv_b, self.deconv_db = self.params[off:off + C], self.grads[off:off + C]
                ly.b, ly.db = self._b4, self._db4
                off += C
            ly.wt = self._wt[woff:woff + nwl].view(ly.cin, -1)
            woff += nwl
        assert off % 4 == 0  # (a3d_mask_loss reads the predictor's weights as 16-byte vectors)
        self.pred_off = off
        self.pred_w, self.pred_b = self.params[off:off + C], self.params[off + C:off + C + 1]
        self.pred_grad = self.grads[off:off + C + 1]  # dw | db
        self._loss_out = torch.zeros(C + 2, device=self.dev)  # a3d_mask_loss: dw | db | loss
        self.grad_segments = [(0, n)]
        self._tbatch = None
        self.load_state_dict(sd)

    def _views(self, buf):
        """(name, tensor) of a flat buffer laid out like self.params, under the reference's names and layouts."""
        out, o, C = [], 0, self.dim
        for ly in self.layers.values():
            nwl = ly.rows * ly.k * ly.k * ly.cin
            w = buf[o:o + nwl].view(ly.rows, -1)
            o += nwl
            if ly.k == 3:
                out += [(ly.name + ".weight", w.view(ly.rows, 3, 3, ly.cin).permute(0, 3, 1, 2)), (ly.name + ".bias", buf[o:o + ly.rows])]
                o += ly.rows
            else:
                out += [(ly.name + ".weight", deconv_from_packed(w)), (ly.name + ".bias", buf[o:o + C])]
                o += C
        out += [(MH + "predictor.weight", buf[o:o + C].view(1, C, 1, 1)), (MH + "predictor.bias", buf[o + C:o + C + 1])]
        return out

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Mask-head entries of a state dict (other keys are ignored: the frozen detector keeps the model's weights)."""
        C = self.dim
        for ly in self.layers.values():
            w = sd[ly.name + ".weight"].to(self.dev).float()
            if ly.k == 3:
                ly.w.copy_(w.permute(0, 2, 3, 1).reshape(ly.rows, -1))
                ly.b.copy_(sd[ly.name + ".bias"].to(self.dev))
            else:
                ly.w.copy_(deconv_to_packed(w))
                self.deconv_b.copy_(sd[ly.name + ".bias"].to(self.dev))
        self.pred_w.copy_(sd[MH + "predictor.weight"].to(self.dev).float().reshape(C))
        self.pred_b.copy_(sd[MH + "predictor.bias"].to(self.dev).float().reshape(1))

    def export_state_dict(self) -> Dict[str, torch.Tensor]:
        """The trainable parameters (roi_heads.mask_head.*) under the reference's names and layouts."""
        return {k: v.detach().clone().contiguous() for k, v in self._views(self.params)}

    def export_grads(self) -> Dict[str, torch.Tensor]:
        """The gradients of the last step -- at world > 1 after `optimizer_step`, the exchanged (averaged) ones."""
        g = self.grads * self._grad_scale if self._grad_scale != 1.0 else self.grads
        return {k: v.detach().clone().contiguous() for k, v in self._views(g)}

    def autograd_anchor(self) -> torch.Tensor:
        return self.det.autograd_anchor()

    # ------------------------------------------------------------------------------------------ the head
    def _conv(self, x, pk, m_dev, **kw):
        # precision 0: the fp32-input MFMA form, the one conv kernel form that honours a live row count (a3d_conv_desc.m_dev)
        return ops.conv2d(x, pk, precision=0, m_dev=m_dev, **kw)

    def _mark(self, name):
        if self.phase_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.phase_events.append((name, ev))

    def _upload_masks(self, gt_masks, gt_boxes, hw):
        B = len(gt_masks)
        ms = [gt_bitmasks(m) for m in gt_masks]
        for m, b in zip(ms, gt_boxes):
            assert len(m) == len(b), "one gt_masks entry per ground-truth box"
            assert len(m) == 0 or tuple(m.shape[1:]) == tuple(hw), f"gt_masks at the image's resolution {tuple(hw)}, got {tuple(m.shape[1:])}"
        G = max(1, max(len(m) for m in ms))
        out = torch.zeros((B, G, hw[0], hw[1]), device=self.dev, dtype=torch.uint8)
        for i, m in enumerate(ms):
            if len(m):
                out[i, : len(m)] = m.to(self.dev, non_blocking=True).to(torch.uint8)
        return out

    # ------------------------------------------------------------------------------------------ the step
    def forward_backward(self, frames_u8: torch.Tensor, gt_boxes: Sequence[torch.Tensor], gt_classes: Sequence[torch.Tensor],
                         gt_masks: Sequence[torch.Tensor], samples: Optional[dict] = None,
                         exchange: bool = False) -> Tuple[Dict[str, torch.Tensor], dict]:
        """frames_u8 [B,H,W,3] uint8 BGR on the device; per image gt_boxes [G,4], gt_classes [G], gt_masks [G,H,W] bool / uint8 (or a
        structures.BitMasks).  Fills self.grads; returns ({loss_cls, loss_box_reg, loss_mask}, aux).  exchange=True: the gradient exchange
        leaves behind the backward pass; `optimizer_step` must follow."""
        s, L, C = self.s, self.layers, self.dim
        B, H, W = frames_u8.shape[:3]
        masks = self._upload_masks(gt_masks, gt_boxes, (H, W))  # (refuses polygons before anything runs)
        self._mark("start")
        self._grad_scale = 1.0  # (self.grads is this rank's own gradient until optimizer_step has exchanged it)
        saved_sk, ops.BF16_SPLITK_AUTO = ops.BF16_SPLITK_AUTO, True
        try:
            self.det.iter = self.iter  # (the ROI sampling seed follows the step count, as in stage 1)
            box_l, aux = self.det.frozen_forward(frames_u8, gt_boxes, gt_classes, samples)
        finally:
            ops.BF16_SPLITK_AUTO = saved_sk
        fgd = foreground_rows(s, self.cap, self.dev, aux, B)
        if samples is not None:  # (given index sets: host control flow is allowed here; the cap must hold)
            assert int((aux["roi_cls"][:, :] < s.num_classes).logical_and(
                torch.arange(s.roi_batch_per_image, device=self.dev)[None] < aux["roi_count"][:, None]).sum(1).max()) <= self.cap, \
                f"more than {self.cap} foreground rows in an image"
        self._mark("frozen_forward")
        M, P = B * self.cap, self.pool_size
        live = fgd["live"]
        live_px = (live * (P * P)).to(torch.int32)
        pyr = [aux["feats"][n] for n in self.in_features]
        pooled = ops.roi_align_fpn(pyr, self.pool_scales, fgd["boxes"], fgd["count"], P, self.pool_ratio, self.pool_aligned,
                                   row_offset=fgd["row_offset"], rows=M)
        self._xchg_live = False
        if exchange and self.grad_overlap != "0":
            if self._xchg is None:
                self._xchg = GradientExchange(self.grads, self.grad_segments, self.pg, self.grad_payload,
                                              force=self.grad_overlap.startswith("force"))
            if self._xchg.active:
                self._xchg.begin()
                self._xchg_live = True
        if self._tbatch is None:
            self._tbatch = T.TransposeBatch([(ly.w, None, ly.wt, ly.rows, ly.k, ly.k, ly.cin) for ly in L.values()], self.dev)
        self._tbatch.run()  # the data-gradient filters of the current weights
        self._b4.copy_(self.deconv_b.repeat(4))
        # ---- forward
        acts = [pooled]
        x = pooled
        for k in range(1, self.num_conv + 1):
            x = self._conv(x, L[f"{MH}mask_fcn{k}"].fwd(), live_px)
            acts.append(x)
        dec = L[MH + "deconv"]
        yu = self._conv(x, dec.fwd(), live_px)  # [M, P, P, (dy, dx, co)]: the deconv's output after ReLU, unshuffled
        targets = T.mask_targets(masks, fgd["boxes"], fgd["count"], fgd["row_offset"], fgd["row_gt"], live, rows=M, size=2 * P)
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
        losses = dict(box_l)
        losses["loss_mask"] = out[C + 1].clone()
        T.conv_wgrad(x, dyu, dec.dw, KH=1, KW=1, stride=1, pad=0, precision=self.wgrad_prec, p_dev=live_px)
        T.colsum_rows(dyu, self._db4, live_px)
        self.deconv_db.copy_(deconv_bias_fold(self._db4))
        dx = self._conv(dyu, dec.bwd(), live_px, gate=x)
        for k in range(self.num_conv, 0, -1):
            ly = L[f"{MH}mask_fcn{k}"]
            T.conv_wgrad(acts[k - 1], dx, ly.dw, KH=3, KW=3, stride=1, pad=1, precision=self.wgrad_prec, p_dev=live_px)
            T.colsum_rows(dx, ly.db, live_px)
            if k > 1:  # (no data gradient into the pooled features: conv1's input is frozen)
                dx = self._conv(dx, ly.bwd(), live_px, gate=acts[k - 1])
        if self._xchg_live:
            self._xchg.segment_ready(0, torch.cuda.current_stream())
        self._mark("mask_backward")
        aux.update(fg=fgd, pooled=pooled, mask_targets=targets, gt_masks=masks)
        return losses, aux

    def optimizer_step(self):
        s = self.s
        if self._xchg_live:
            scale, self._xchg_live = self._xchg.finish(), False
        else:
            scale = allreduce_gradients(self.grads, self.pg, payload=self.grad_payload)
        self._grad_scale = scale
        T.sgd_momentum(self.params, self.grads, self.momentum, lr=lr_at(self.iter, s), momentum=s.momentum, weight_decay=s.weight_decay,
                       grad_scale=scale, first=self.iter == 0)
        self._mark("exchange_sgd")
        self.iter += 1

    def step(self, frames_u8, gt_boxes, gt_classes, gt_masks, samples=None):
        losses, aux = self.forward_backward(frames_u8, gt_boxes, gt_classes, gt_masks, samples, exchange=True)
        self.optimizer_step()
        return losses, aux
