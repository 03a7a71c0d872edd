"""The scaffold every head trainer over the frozen detector shares (training_axis.AxisTrainer, training_mask.MaskTrainer,
training_plane.PlaneTrainer; training_depth.DepthTrainer takes everything but the ROI prologue).

`HeadTrainer` owns, once:
  * the frozen detector (a `DetectorTrainer` driven through `frozen_forward`: stage 1's launches, precision, storage and ROI sampling seed)
    and `foreground_rows`, select_foreground_proposals on the device: compact rows, per-image counts, row offsets and the live total stay
    in device tensors, and every launch of a head takes the live count;
  * the flat parameter / gradient / momentum buffers, laid out by the pure `flat_layout` (the layout is the checkpoint format:
    engine.FlatSGD saves the momentum buffer as it lies), the `_Layer` views carved out of them and the transposed data-gradient filters;
  * the step around the head: the shared prologue (ground truth, frozen forward, foreground rows, pooled rows), the lazy gradient exchange
    and filter transposes, the 3x3 tower's forward and backward chain, SGD, and the exports under the reference's names and layouts.

A subclass supplies its state-dict prefix, its layer table (`_layer_table`: the arguments of `flat_layout`), the reference layout of its
layers that are not 3x3 convs (`_odd_views` / `_load_odd`), its ground-truth hooks (`batch_extras`, `_ground_truth`) and `_head`: the
head's forward pass, loss and backward pass.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import ops, train_ops as T
from .parallel import GradientExchange, allreduce_gradients
from .training import DetectorTrainer, FlatLayout, SolverCfg, _Layer, flat_layout, lr_at, open_exchange  # noqa: F401 (FlatLayout: importable from here)


def fc_columns_to_hwc(w: torch.Tensor, channels: int, size: int) -> torch.Tensor:
    """A flattening FC's weight (or its gradient) [rows, channels * size * size] with the reference's CHW column order -> the HWC order of
    the NHWC activations, what the inference `Linear(chw=...)` does."""
    return w.reshape(w.shape[0], channels, size, size).permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def fc_columns_to_chw(w: torch.Tensor, channels: int, size: int) -> torch.Tensor:
    """HWC column order -> the reference's CHW: the inverse of fc_columns_to_hwc (weights and gradients alike: a permutation)."""
    return w.reshape(w.shape[0], size, size, channels).permute(0, 3, 1, 2).reshape(w.shape[0], -1)


def foreground_rows(s: SolverCfg, cap: int, dev, aux, B: int) -> dict:
    """select_foreground_proposals on the device: per-image foreground counts of the sampled rows (class < num_classes, sample order, at
    most `cap` per image), their prefix sum, the live total, and per compact row its proposal box, image and matched ground truth."""
    Rs = s.roi_batch_per_image
    live_slot = torch.arange(Rs, device=dev)[None, :] < aux["roi_count"][:, None]
    fg = live_slot & (aux["roi_cls"] < s.num_classes)
    pos = torch.cumsum(fg.to(torch.int32), 1) - 1
    keep = fg & (pos < cap)
    count = keep.sum(1, dtype=torch.int32)
    row_off = ops.count_offsets(count, cap)  # [B+1]: exclusive prefix sum, total last
    img = torch.arange(B, device=dev, dtype=torch.int32)[:, None].expand(B, Rs)
    trash = B * cap
    slot = torch.where(keep, img * cap + pos, torch.full_like(pos, trash)).reshape(-1).long()  # per-image slot of the pooler's boxes
    row = torch.where(keep, row_off[:-1, None] + pos, torch.full_like(pos, trash)).reshape(-1).long()  # compact row
    boxes = torch.zeros(trash + 1, 4, device=dev)
    boxes[slot] = aux["roi_boxes"].reshape(-1, 4)
    gidx = torch.gather(aux["proposal_match"].long(), 1, aux["roi_index"].clamp(min=0).long()).to(torch.int32)
    row_img = torch.zeros(trash + 1, device=dev, dtype=torch.int32)
    row_gt = torch.zeros(trash + 1, device=dev, dtype=torch.int32)
    row_img[row] = img.reshape(-1)
    row_gt[row] = gidx.reshape(-1)
    return dict(count=count, row_offset=row_off, live=row_off[B:].contiguous(), boxes=boxes[:trash].view(B, cap, 4),
                row_img=row_img[:trash].contiguous(), row_gt=row_gt[:trash].contiguous())


class HeadTrainer:
    """One training step of a head over the frozen detector: the detector's forward pass, the head's forward and backward pass over the
    compacted foreground rows, its loss and the SGD update of its parameters -- all on the device.

    Precision.  The frozen detector runs in `precision` exactly as DetectorTrainer does.  In the head only the weight gradients follow it
    (fp32-input MFMA, bf16 autocast arithmetic or the bf16x3 split); forward and data-gradient launches run the fp32-input MFMA in EVERY
    precision, because that is the one conv kernel form that honours a live row count (a3d_conv_desc.m_dev) -- the bf16 and bf16x3 forms
    refuse it.  So precision="bf16" is not the reference's autocast arithmetic in the head's forward pass: it is more exact, and no
    faster than "fp32" there.

    Public shape of `DetectorTrainer`: forward_backward, optimizer_step, step, load_state_dict, export_state_dict, export_grads,
    autograd_anchor, the `samples=` hook (the ROI index sets to use instead of drawing them), and `phase_events`."""

    PREFIX: str  # the head's state-dict prefix
    # the head's pooler: set by the subclass before HeadTrainer.__init__
    pool_size: int
    pool_ratio: int
    pool_aligned: bool
    pool_scales: list
    in_features: list

    def __init__(self, model, solver: Optional[SolverCfg] = None, seed: int = 2020, process_group=None, precision: str = "bf16x3",
                 grad_payload: Optional[str] = None, storage: Optional[str] = None, grad_overlap: Optional[str] = None):
        self.det = DetectorTrainer(model, solver, seed=seed, process_group=process_group, precision=precision, storage=storage)
        self.s, self.model, self.dev, self.pg = self.det.s, model, self.det.dev, process_group
        self.precision = precision
        self.wgrad_prec = self.det.wgrad_prec
        self.grad_payload = grad_payload or ("bf16" if precision == "bf16" else "fp32")
        self.grad_overlap = self.det.grad_overlap if grad_overlap is None else str(grad_overlap)
        self.cap = int(self.s.roi_batch_per_image * self.s.roi_positive_fraction)  # foreground rows per image at most (128)
        self.iter = 0
        self._xchg: Optional[GradientExchange] = None
        self._xchg_live = False
        self._grad_scale = 1.0
        self._tbatch = None
        self.phase_events = None  # a list: every step appends (name, event recorded on the main stream) at its phase boundaries
        self._allocate(**self._layer_table())
        self.load_state_dict({k: v.detach().float() for k, v in model.state_dict().items() if k.startswith(self.PREFIX)})

    @staticmethod
    def batch_extras(batched_inputs) -> tuple:
        """The head's ground truth in a batch of the reference's training-mode call: what follows gt_classes in `forward_backward`."""
        raise NotImplementedError

    # ------------------------------------------------------------------------------------------ parameters
    def _allocate(self, layers, **table):
        self.layout = lay = flat_layout(layers, **table)
        self.layers: Dict[str, _Layer] = {ly.name: ly for ly in layers}
        self.params = torch.zeros(lay.total, device=self.dev)
        self.grads = torch.zeros(lay.total, device=self.dev)
        self.momentum = torch.zeros(lay.total, device=self.dev)
        self._wt = torch.empty(sum(nw for _, nw, _, _ in lay.layers.values()), device=self.dev)
        self.grad_segments = lay.segments
        woff = 0
        for ly in layers:
            o, nw, ob, nb = lay.layers[ly.name]
            ly.w, ly.dw = self.params[o:o + nw].view(ly.rows, -1), self.grads[o:o + nw].view(ly.rows, -1)
            ly.b, ly.db = self.params[ob:ob + nb], self.grads[ob:ob + nb]
            ly.wt = self._wt[woff:woff + nw].view(ly.cin, -1)
            woff += nw

    def _views(self, buf):
        """(name, tensor) of a flat buffer laid out like self.params, under the reference's names and layouts."""
        out = []
        for ly in self.layers.values():
            o, nw, ob, nb = self.layout.layers[ly.name]
            w, b = buf[o:o + nw].view(ly.rows, -1), buf[ob:ob + nb]
            if ly.k == 3:
                out += [(ly.name + ".weight", w.view(ly.rows, 3, 3, ly.cin).permute(0, 3, 1, 2)), (ly.name + ".bias", b)]
            else:
                out += self._odd_views(ly, w, b)
        return out

    @torch.no_grad()
    def load_state_dict(self, sd):
        """The head's entries of a state dict (other keys are ignored: the frozen detector keeps the model's weights)."""
        for ly in self.layers.values():
            if ly.k == 3:
                ly.w.copy_(sd[ly.name + ".weight"].to(self.dev).float().permute(0, 2, 3, 1).reshape(ly.rows, -1))
                ly.b.copy_(sd[ly.name + ".bias"].to(self.dev))
            else:
                self._load_odd(ly, sd)

    def export_state_dict(self) -> Dict[str, torch.Tensor]:
        """The trainable parameters under the reference's names and layouts."""
        return {k: v.detach().clone().contiguous() for k, v in self._views(self.params)}

    def export_grads(self) -> Dict[str, torch.Tensor]:
        """The gradients of the last step -- at world > 1 after `optimizer_step`, the exchanged (averaged) ones."""
        g = self.grads * self._grad_scale if self._grad_scale != 1.0 else self.grads
        return {k: v.detach().clone().contiguous() for k, v in self._views(g)}

    def autograd_anchor(self) -> torch.Tensor:
        return self.det.autograd_anchor()

    # ------------------------------------------------------------------------------------------ the head's launches
    def _conv(self, x, pk, m_dev, **kw):
        # precision 0: the fp32-input MFMA form, the one conv kernel form that honours a live row count (a3d_conv_desc.m_dev)
        return ops.conv2d(x, pk, precision=0, m_dev=m_dev, **kw)

    def _wgrad(self, ly: _Layer, x, dy, m_dev):
        T.conv_wgrad(x, dy, ly.dw, KH=ly.k, KW=ly.k, stride=1, pad=ly.pad, precision=self.wgrad_prec, p_dev=m_dev)
        T.colsum_rows(dy, ly.db, m_dev)

    def _tower_forward(self, names, x, live_px):
        """The 3x3 layers `names` over x: [x, every layer's output]."""
        acts = [x]
        for n in names:
            acts.append(self._conv(acts[-1], self.layers[n].fwd(), live_px))
        return acts

    def _tower_backward(self, names, acts, dx, live_px):
        """Backward of _tower_forward from dx, the gradient of acts[-1]: per layer weight gradient, bias gradient, gated data gradient."""
        for k in range(len(names), 0, -1):
            ly = self.layers[names[k - 1]]
            self._wgrad(ly, acts[k - 1], dx, live_px)
            if k > 1:  # (no data gradient into the pooled features: the first layer's input is frozen)
                dx = self._conv(dx, ly.bwd(), live_px, gate=acts[k - 1])

    def _mark(self, name):
        if self.phase_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.phase_events.append((name, ev))

    # ------------------------------------------------------------------------------------------ the step
    def forward_backward(self, frames_u8: torch.Tensor, gt_boxes: Sequence[torch.Tensor], gt_classes: Sequence[torch.Tensor], *gt,
                         samples: Optional[dict] = None, exchange: bool = False) -> Tuple[Dict[str, torch.Tensor], dict]:
        """frames_u8 [B,H,W,3] uint8 BGR on the device; per image gt_boxes [G,4], gt_classes [G] and the head's ground truth `gt` (see the
        subclass).  Fills self.grads; returns ({loss_cls, loss_box_reg, the head's losses}, aux).  exchange=True: the gradient exchange
        leaves segment by segment behind the backward pass; `optimizer_step` must follow.  `samples` and `exchange` are keyword-only
        (here and in `step`): the head's ground truth takes the positions behind gt_classes.  The ground truth is checked and uploaded
        (`_ground_truth`) before the `start` mark and the frozen forward pass, so a malformed batch is refused before anything runs."""
        s, B = self.s, frames_u8.shape[0]
        gt = self._ground_truth(frames_u8, gt_boxes, *gt)
        box_l, aux = self._frozen_step(frames_u8, gt_boxes, gt_classes, samples)
        fgd = foreground_rows(s, self.cap, self.dev, aux, B)
        if samples is not None:  # (given index sets: host control flow is allowed here; the cap must hold)
            assert int((aux["roi_cls"][:, :] < s.num_classes).logical_and(
                torch.arange(s.roi_batch_per_image, device=self.dev)[None] < aux["roi_count"][:, None]).sum(1).max()) <= self.cap, \
                f"more than {self.cap} foreground rows in an image"
        self._mark("frozen_forward")
        M, P = B * self.cap, self.pool_size
        live = fgd["live"]
        live_px = (live * (P * P)).to(torch.int32)
        pooled = ops.roi_align_fpn([aux["feats"][n] for n in self.in_features], self.pool_scales, fgd["boxes"], fgd["count"], P,
                                   self.pool_ratio, self.pool_aligned, row_offset=fgd["row_offset"], rows=M)
        self._begin_head(exchange)
        losses = dict(box_l)
        aux.update(fg=fgd, pooled=pooled)
        self._head(losses, aux, fgd, live, live_px, pooled, gt)
        return losses, aux

    def _frozen_step(self, frames_u8, gt_boxes, gt_classes, samples):
        """The `start` mark and the frozen detector's forward pass of a step (the ground truth has been checked and uploaded)."""
        self._mark("start")
        self._grad_scale = 1.0  # (self.grads is this rank's own gradient until optimizer_step has exchanged it)
        self.det.iter = self.iter  # (the ROI sampling seed follows the step count, as in stage 1)
        return self.det.frozen_forward(frames_u8, gt_boxes, gt_classes, samples)

    def _begin_head(self, exchange: bool):
        """In front of the head's launches: the gradient exchange opens (exchange=True) and the data-gradient filters of the current
        weights are made."""
        self._xchg_live = open_exchange(self, exchange)
        if self._tbatch is None:
            self._tbatch = T.TransposeBatch([(ly.w, None, ly.wt, ly.rows, ly.k, ly.k, ly.cin) for ly in self.layers.values()], self.dev)
        self._tbatch.run()

    def _segment_ready(self, i: int, stream):
        if self._xchg_live:
            self._xchg.segment_ready(i, stream)

    def optimizer_step(self):
        s = self.s
        if self._xchg_live:
            scale, self._xchg_live = self._xchg.finish(), False
        else:
            scale = allreduce_gradients(self.grads, self.pg, payload=self.grad_payload)
        self._grad_scale = scale
        self._sgd(lr_at(self.iter, s), scale)
        self._mark("exchange_sgd")
        self.iter += 1

    def _sgd(self, lr: float, scale: float):
        s = self.s
        T.sgd_momentum(self.params, self.grads, self.momentum, lr=lr, momentum=s.momentum, weight_decay=s.weight_decay, grad_scale=scale,
                       first=self.iter == 0)

    def step(self, frames_u8, gt_boxes, gt_classes, *gt, samples=None):
        losses, aux = self.forward_backward(frames_u8, gt_boxes, gt_classes, *gt, samples=samples, exchange=True)
        self.optimizer_step()
        return losses, aux
