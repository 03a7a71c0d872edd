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
    (`roi_batch_per_image * roi_positive_fraction`): per-image counts, their exclusive prefix sum (the pooler's row offsets) and the
    live total stay in device tensors -- nothing waits for the host.  Every launch of the head takes the live count: the forward and
    data-gradient convs through a3d_conv_desc.m_dev (the fp32-input MFMA form, the one kernel form that honours it), the weight
    gradients through a3d_wgrad_desc.p_dev (in the step's precision), the bias gradients through a3d_colsum_rows.  Dead rows cost
    nothing and are never read.
  * The 107.5 M trainable parameters (eight 3x3 convs, two 50176 -> 1024 FCs whose columns are permuted CHW -> HWC as the inference
    `Linear(chw=...)` does, rotation | offset fused to one 1024 -> 3 layer, translation) live in one flat buffer; gradients and momenta
    are two more.  The T tower runs beside the R tower on side stream 1; the gradient exchange leaves in two segments, one per tower.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import ops, train_ops as T
from .ops import ACT_NONE, ACT_RELU
from .parallel import GradientExchange, allreduce_gradients
from .training import DetectorTrainer, SolverCfg, _Layer, lr_at

AXIS_TOWER_STREAM = os.environ.get("A3D_TRAIN_AXIS_STREAM", "1") != "0"  # the T tower on a second stream beside R (same bits)
AH = "roi_heads.axis_head."
P14 = 14
POOLED = 256 * P14 * P14  # 50176


def foreground_rows(s: SolverCfg, cap: int, dev, aux, B: int) -> dict:
    """select_foreground_proposals on the device (shared by the axis and the mask stage): per-image foreground counts of the sampled rows
    (class < num_classes, sample order, at most `cap` per image), their prefix sum, the live total, and per compact row its proposal box,
    image and matched ground truth."""
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


class AxisTrainer:
    """One training step of the step2_axis configuration: the frozen detector's forward pass, the axis head's forward and backward pass
    over the compacted foreground rows, the axis loss and the SGD update of roi_heads.axis_head.* -- all on the device.

    Precision.  The frozen detector runs in `precision` exactly as DetectorTrainer does.  In the axis head only the weight gradients follow
    it (fp32-input MFMA, bf16 autocast arithmetic or the bf16x3 split); its forward and data-gradient launches run the fp32-input MFMA in
    EVERY precision, because that is the one conv kernel form that honours a live row count (a3d_conv_desc.m_dev) -- the bf16 and bf16x3
    forms refuse it.  So precision="bf16" is not the reference's autocast arithmetic in the head's forward pass: it is more exact, and no
    faster than "fp32" there.

    Public shape of `DetectorTrainer`: forward_backward, optimizer_step, step, load_state_dict, export_state_dict, export_grads,
    autograd_anchor, and the `samples=` hook (the ROI index sets to use instead of drawing them)."""

    def __init__(self, model, solver: Optional[SolverCfg] = None, seed: int = 2020, process_group=None, precision: str = "bf16x3",
                 grad_payload: Optional[str] = None, storage: Optional[str] = None, grad_overlap: Optional[str] = None,
                 beta: Optional[float] = None, loss_weight: Optional[float] = None):
        self.det = DetectorTrainer(model, solver, seed=seed, process_group=process_group, precision=precision, storage=storage)
        self.s, self.model, self.dev, self.pg = self.det.s, model, self.det.dev, process_group
        self.precision = precision
        self.wgrad_prec = self.det.wgrad_prec
        self.grad_payload = grad_payload or ("bf16" if precision == "bf16" else "fp32")
        self.grad_overlap = self.det.grad_overlap if grad_overlap is None else str(grad_overlap)
        ah = model.roi_heads.axis_head
        self.beta = float(ah.smooth_l1_beta if beta is None else beta)
        self.loss_weight = float(ah._loss_weight if loss_weight is None else loss_weight)
        self.cap = int(self.s.roi_batch_per_image * self.s.roi_positive_fraction)  # foreground rows per image at most (128)
        self.iter = 0
        self._xchg: Optional[GradientExchange] = None
        self._xchg_live = False
        self._grad_scale = 1.0
        self.phase_events = None  # a list: every step appends (name, event recorded on the main stream) at its phase boundaries
        from .streams import side

        self._t_stream = side(1, self.dev) if AXIS_TOWER_STREAM else None
        self._build_layers({k: v.detach().float() for k, v in model.state_dict().items() if k.startswith(AH)})

    # ------------------------------------------------------------------------------------------ parameters
    def _build_layers(self, sd):
        L: Dict[str, _Layer] = {}
        for t in ("R", "T"):
            for k in range(1, 5):
                n = f"{AH}axis_{t}_conv{k}"
                L[n] = _Layer(n, 256, 256, 3, 1, 1, ACT_RELU)
            n = f"{AH}axis_{t}_fc1"
            L[n] = _Layer(n, 1024, POOLED, 1, 1, 0, ACT_RELU)
            if t == "R":  # rotation | offset: one 1024 -> 3 layer, padded to 32 rows like the box predictor
                L[AH + "rot"] = _Layer(AH + "rot", 32, 1024, 1, 1, 0, ACT_NONE, sources=[(AH + "rotation", 0, 2), (AH + "offset", 2, 1)])
            else:
                L[AH + "tran"] = _Layer(AH + "tran", 32, 1024, 1, 1, 0, ACT_NONE, sources=[(AH + "translation", 0, 2)])
        self.layers = L
        n = sum(ly.rows * ly.k * ly.k * ly.cin + ly.rows for ly in L.values())
        n = (n + 3) // 4 * 4
        self.params = torch.zeros(n, device=self.dev)
        self.grads = torch.zeros(n, device=self.dev)
        self.momentum = torch.zeros(n, device=self.dev)
        self._wt = torch.empty(sum(ly.rows * ly.k * ly.k * ly.cin for ly in L.values()), device=self.dev)
        off = woff = 0
        cut = None
        for ly in L.values():
            if ly.name == f"{AH}axis_T_conv1":
                cut = off
            nwl = ly.rows * ly.k * ly.k * ly.cin
            ly.w, ly.dw = self.params[off:off + nwl].view(ly.rows, -1), self.grads[off:off + nwl].view(ly.rows, -1)
            off += nwl
            ly.b, ly.db = self.params[off:off + ly.rows], self.grads[off:off + ly.rows]
            off += ly.rows
            ly.wt = self._wt[woff:woff + nwl].view(ly.cin, -1)
            woff += nwl
        assert cut % 4 == 0
        # gradient-exchange segments, one per tower: R (the flat buffer's front half) and T
        self.grad_segments = [(0, cut), (cut, n)]
        self._tbatch = None
        self.load_state_dict(sd)

    def _views(self, ly: _Layer, buf_w, buf_b):
        if ly.sources:
            return [kv for prefix, r0, nr in ly.sources for kv in ((prefix + ".weight", buf_w[r0:r0 + nr]), (prefix + ".bias", buf_b[r0:r0 + nr]))]
        if ly.k == 3:
            w = buf_w.view(ly.rows, 3, 3, ly.cin).permute(0, 3, 1, 2)
        else:  # the FC: columns stored in the HWC order of the NHWC activations, the reference's are CHW
            w = buf_w.view(ly.rows, P14, P14, 256).permute(0, 3, 1, 2).reshape(ly.rows, -1)
        return [(ly.name + ".weight", w), (ly.name + ".bias", buf_b)]

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Axis-head entries of a state dict (other keys are ignored: the frozen detector keeps the model's weights)."""
        for ly in self.layers.values():
            if ly.sources:
                ly.w.zero_()
                ly.b.zero_()
                for prefix, r0, nr in ly.sources:
                    ly.w[r0:r0 + nr] = sd[prefix + ".weight"].reshape(nr, -1).to(self.dev)
                    ly.b[r0:r0 + nr] = sd[prefix + ".bias"].to(self.dev)
                continue
            w = sd[ly.name + ".weight"].to(self.dev).float()
            w = w.permute(0, 2, 3, 1) if ly.k == 3 else w.view(ly.rows, 256, P14, P14).permute(0, 2, 3, 1)
            ly.w.copy_(w.reshape(ly.rows, -1))
            ly.b.copy_(sd[ly.name + ".bias"].to(self.dev))

    def export_state_dict(self) -> Dict[str, torch.Tensor]:
        """The trainable parameters (roi_heads.axis_head.*) under the reference's names and layouts."""
        return {k: v.detach().clone().contiguous() for ly in self.layers.values() for k, v in self._views(ly, ly.w, ly.b)}

    def export_grads(self) -> Dict[str, torch.Tensor]:
        """The gradients of the last step -- at world > 1 after `optimizer_step`, the exchanged (averaged) ones."""
        g = self.grads * self._grad_scale if self._grad_scale != 1.0 else self.grads
        out, o = {}, 0
        for ly in self.layers.values():
            nwl = ly.rows * ly.k * ly.k * ly.cin
            w, b = g[o:o + nwl].view(ly.rows, -1), g[o + nwl:o + nwl + ly.rows]
            o += nwl + ly.rows
            out.update({k: v.detach().clone().contiguous() for k, v in self._views(ly, w, b)})
        return out

    def autograd_anchor(self) -> torch.Tensor:
        return self.det.autograd_anchor()

    # ------------------------------------------------------------------------------------------ the head
    def _conv(self, x, pk, m_dev, **kw):
        # precision 0: the fp32-input MFMA form, the one conv kernel form that honours a live row count (a3d_conv_desc.m_dev)
        return ops.conv2d(x, pk, precision=0, m_dev=m_dev, **kw)

    def _wgrad(self, ly: _Layer, x, dy, p_dev, m_dev):
        T.conv_wgrad(x, dy, ly.dw, KH=ly.k, KW=ly.k, stride=1, pad=ly.pad, precision=self.wgrad_prec, p_dev=p_dev)
        T.colsum_rows(dy, ly.db, m_dev)

    def _tower_forward(self, t, pooled, live, live_px):
        L, M = self.layers, pooled.shape[0]
        acts = [pooled]
        x = pooled
        for k in range(1, 5):
            x = self._conv(x, L[f"{AH}axis_{t}_conv{k}"].fwd(), live_px)
            acts.append(x)
        fc = L[f"{AH}axis_{t}_fc1"]
        xf = x.view(M, 1, 1, POOLED)
        h = self._conv(xf, fc.fwd(), live, splitk=ops.choose_splitk(M, 1024, POOLED))
        last = L[AH + ("rot" if t == "R" else "tran")]
        raw = self._conv(h, last.fwd(), live)
        return acts, xf, h, raw.view(M, 32)

    def _tower_backward(self, t, acts, xf, h, draw, live, live_px):
        L, M = self.layers, xf.shape[0]
        last = L[AH + ("rot" if t == "R" else "tran")]
        fc = L[f"{AH}axis_{t}_fc1"]
        d = draw.view(M, 1, 1, 32)
        self._wgrad(last, h, d, live, live)
        dh = self._conv(d, last.bwd(), live, gate=h)
        self._wgrad(fc, xf, dh, live, live)
        dx = self._conv(dh, fc.bwd(), live, gate=xf).view(M, P14, P14, 256)
        for k in (4, 3, 2, 1):
            ly = L[f"{AH}axis_{t}_conv{k}"]
            self._wgrad(ly, acts[k - 1], dx, live_px, live_px)
            if k > 1:  # (no data gradient into the pooled features: conv1's input is frozen)
                dx = self._conv(dx, ly.bwd(), live_px, gate=acts[k - 1])

    def _mark(self, name):
        if self.phase_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.phase_events.append((name, ev))

    # ------------------------------------------------------------------------------------------ the step
    def forward_backward(self, frames_u8: torch.Tensor, gt_boxes: Sequence[torch.Tensor], gt_classes: Sequence[torch.Tensor],
                         gt_rot_axis: Sequence[torch.Tensor], gt_tran_axis: Sequence[torch.Tensor], samples: Optional[dict] = None,
                         exchange: bool = False) -> Tuple[Dict[str, torch.Tensor], dict]:
        """frames_u8 [B,H,W,3] uint8 BGR on the device; per image gt_boxes [G,4], gt_classes [G], gt_rot_axis / gt_tran_axis [G,4]
        ([sin, cos, offset, valid]: utils.opt_utils.axis_to_angle_offset).  Fills self.grads; returns ({loss_cls, loss_box_reg,
        loss_rot_axis, loss_tran_axis}, aux).  exchange=True: the gradient exchange leaves tower by tower; `optimizer_step` must follow."""
        s, L = self.s, self.layers
        B = frames_u8.shape[0]
        self._mark("start")
        self._grad_scale = 1.0  # (self.grads is this rank's own gradient until optimizer_step has exchanged it)
        saved_sk, ops.BF16_SPLITK_AUTO = ops.BF16_SPLITK_AUTO, True
        try:
            self.det.iter = self.iter  # (the ROI sampling seed follows the step count, as in stage 1)
            box_l, aux = self.det.frozen_forward(frames_u8, gt_boxes, gt_classes, samples)
        finally:
            ops.BF16_SPLITK_AUTO = saved_sk
        gra = torch.zeros(B, s.max_gt, 4)
        gta = torch.zeros(B, s.max_gt, 4)
        for i, (r, t) in enumerate(zip(gt_rot_axis, gt_tran_axis)):
            assert len(r) == len(t) == len(gt_boxes[i]), "one gt_rot_axis / gt_tran_axis row per ground-truth box"
            gra[i, : len(r)] = r.detach().float().cpu()
            gta[i, : len(t)] = t.detach().float().cpu()
        gra, gta = gra.to(self.dev, non_blocking=True), gta.to(self.dev, non_blocking=True)
        fgd = foreground_rows(s, self.cap, self.dev, aux, B)
        if samples is not None:  # (given index sets: host control flow is allowed here; the cap must hold)
            assert int((aux["roi_cls"][:, :] < s.num_classes).logical_and(
                torch.arange(s.roi_batch_per_image, device=self.dev)[None] < aux["roi_count"][:, None]).sum(1).max()) <= self.cap, \
                f"more than {self.cap} foreground rows in an image"
        self._mark("frozen_forward")
        M = B * self.cap
        live = fgd["live"]
        live_px = (live * (P14 * P14)).to(torch.int32)
        pyr = [aux["feats"][n] for n in ("p2", "p3", "p4", "p5")]
        pooled = ops.roi_align_fpn(pyr, [0.25, 0.125, 0.0625, 0.03125], fgd["boxes"], fgd["count"], P14, 0, False,
                                   row_offset=fgd["row_offset"], rows=M)
        # ---- tower R on the current stream, tower T beside it
        main, side = torch.cuda.current_stream(), self._t_stream
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
        t_out = None
        if side is not None:
            ev = torch.cuda.Event()
            ev.record(main)
            for ten in (pooled, live, live_px):
                ten.record_stream(side)
            torch.cuda.set_stream(side)
            try:
                side.wait_event(ev)
                t_out = self._tower_forward("T", pooled, live, live_px)
            finally:
                torch.cuda.set_stream(main)
        r_out = self._tower_forward("R", pooled, live, live_px)
        if side is None:
            t_out = self._tower_forward("T", pooled, live, live_px)
        else:
            main.wait_stream(side)
            for ten in t_out[0] + [t_out[1], t_out[2], t_out[3]]:
                ten.record_stream(main)
        axl, d_rot, d_tran = T.axis_loss(r_out[3], t_out[3], live, fgd["row_img"], fgd["row_gt"], gra, gta, beta=self.beta,
                                         loss_weight=self.loss_weight)
        self._mark("axis_forward")
        losses = dict(box_l)
        losses["loss_rot_axis"], losses["loss_tran_axis"] = axl[0], axl[1]
        # ---- backward: T beside R again, each tower's gradient segment leaves when its last launch is enqueued
        if side is not None:
            ev2 = torch.cuda.Event()
            ev2.record(main)
            d_tran.record_stream(side)
            torch.cuda.set_stream(side)
            try:
                side.wait_event(ev2)
                self._tower_backward("T", t_out[0], t_out[1], t_out[2], d_tran, live, live_px)
                if self._xchg_live:
                    self._xchg.segment_ready(1, side)
            finally:
                torch.cuda.set_stream(main)
        self._tower_backward("R", r_out[0], r_out[1], r_out[2], d_rot, live, live_px)
        if self._xchg_live:
            self._xchg.segment_ready(0, main)
        if side is None:
            self._tower_backward("T", t_out[0], t_out[1], t_out[2], d_tran, live, live_px)
            if self._xchg_live:
                self._xchg.segment_ready(1, main)
        else:
            main.wait_stream(side)
        self._mark("axis_backward")
        aux.update(fg=fgd, pooled=pooled, raw_rot=r_out[3][:, :3], raw_tran=t_out[3][:, :2], d_rot=d_rot[:, :3], d_tran=d_tran[:, :2],
                   gt_axes=(gra, gta))
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

    def step(self, frames_u8, gt_boxes, gt_classes, gt_rot_axis, gt_tran_axis, samples=None):
        losses, aux = self.forward_backward(frames_u8, gt_boxes, gt_classes, gt_rot_axis, gt_tran_axis, samples, exchange=True)
        self.optimizer_step()
        return losses, aux
