#!/usr/bin/env python3
"""Throughput of the stage-4 training step (configs/step3_planehead.yaml: the plane-normal head over the frozen detector) on one MI355X.

    python tools/train_plane_bench.py [--steps K --warmup W --batches 2,8 --precisions bf16x3 --unfused]

One step = the frozen detector's forward pass + the plane head's forward and backward pass over the live foreground rows + SGD, on
synthetic 480x640 frames (tools/train_bench.py's boxes, a random unit normal times a random offset per box).  Per (precision, batch):
images/s over K timed steps after W untimed ones, the live foreground rows, the milliseconds of each phase (device events on the main
stream at the phase boundaries of one extra step: frozen forward, plane forward, loss + backward, exchange + SGD), the time of
a3d_plane_loss (`predictor_ms`: both launches, device events around the call, the median of the timed steps; `predictor_with_copies_ms`:
the same plus the two small copies that carry the predictor's gradient and the loss out of the kernel's output), and the peak memory.
The events sit on the stream, so a figure includes whatever host time between two launches the GPU had to wait for.

--unfused adds, per (precision, batch), the same step with the predictor run the axis stage's way: the 1024 -> 3 layer padded to 32
rows through the conv kernel (forward), a one-workgroup loss + gradient launch over the padded rows, the layer's weight gradient, its
column sum and its gated data gradient -- five launches with their host descriptors where the fused route has two.  The loss launch of
that leg is a3d_axis_loss (the in-tree launch of that shape; no plane loss exists outside the fused kernel), so the leg's LOSSES AND
UPDATES ARE NOT THE PLANE HEAD'S: it is a timing of the alternative's launches, nothing else.  Its events enclose the five launches (and, in the second figure, its own two copies).
ONE JSON line on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def synthetic_planes(targets, seed=2020):
    g = torch.Generator().manual_seed(seed)
    out = []
    for t in targets:
        n = torch.randn(len(t[0]), 3, generator=g)
        out.append(n / n.norm(dim=1, keepdim=True) * (0.5 + 3 * torch.rand(len(t[0]), 1, generator=g)))
    return out


def unfused_trainer_class():
    from articulation3d_amd import train_ops as T
    from articulation3d_amd.ops import ACT_NONE
    from articulation3d_amd.training import _Layer
    from articulation3d_amd.training_plane import FC_DIM, PH, PlaneTrainer

    class UnfusedPlaneTrainer(PlaneTrainer):
        """PlaneTrainer with the predictor as a padded 32-row layer: AxisTrainer's route for its `rot` layer (timing only, see above)."""

        def _allocate(self, layers, **table):
            super()._allocate(layers, **table)
            z = lambda *s: torch.zeros(*s, device=self.dev)
            self._last = _Layer(PH + "param_pred32", 32, FC_DIM, 1, 1, 0, ACT_NONE, w=z(32, FC_DIM), dw=z(32, FC_DIM), b=z(32), db=z(32),
                                wt=z(FC_DIM, 32))
            self._axis_gt = z(64, self.s.max_gt, 4)
            self._axis_gt[..., 1] = 1.0
            self._axis_gt[..., 3] = 1.0  # every row valid

        def _predictor(self, losses, h, live, fgd, gt_planes):
            last, M = self._last, h.shape[0]
            last.w[:3].copy_(self.pred_w)
            last.b[:3].copy_(self.pred_b)
            T.weight_transpose(last.w, last.wt, 32, 1, 1, FC_DIM)
            h4 = h.view(M, 1, 1, FC_DIM)
            k0, k1, k2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            k0.record()
            raw = self._conv(h4, last.fwd(), live).view(M, 32)
            gt = self._axis_gt[: gt_planes.shape[0]]
            axl, d_rot, _ = T.axis_loss(raw, raw, live, fgd["row_img"], fgd["row_gt"], gt, gt, beta=0.0, loss_weight=self.loss_weight)
            d = d_rot.view(M, 1, 1, 32)
            self._wgrad(last, h4, d, live)
            dh = self._conv(d, last.bwd(), live, gate=h4)
            k1.record()
            self.pred_grad[: 3 * FC_DIM].copy_(last.dw[:3].reshape(-1))
            self.pred_grad[3 * FC_DIM:].copy_(last.db[:3])
            losses["loss_plane"] = axl[0]
            k2.record()
            if self.kernel_events is not None:
                self.kernel_events.append((k0, k1, k2))
            return dh.view(M, FC_DIM), raw[:, :3]

    return UnfusedPlaneTrainer


def leg(model, dev, precision, batch, steps, warmup, targets, unfused=False):
    from train_head_bench import head_leg
    from articulation3d_amd.training import SolverCfg
    from articulation3d_amd.training_plane import PlaneTrainer
    from articulation3d_amd.utils.synthetic import synthetic_frames

    cls = unfused_trainer_class() if unfused else PlaneTrainer
    frames = torch.from_numpy(synthetic_frames(batch, seed=2020)).to(dev)
    args = (frames, [t[0] for t in targets], [t[1] for t in targets], synthetic_planes(targets))
    kernel_ms = []

    def start_kernel_events(tr):
        tr.kernel_events = []

    def read_kernel_events(tr):  # over the timed steps only: the instrumented step runs without these events
        kernel_ms.append((statistics.median(a.elapsed_time(b) for a, b, _ in tr.kernel_events),
                          statistics.median(a.elapsed_time(c) for a, _, c in tr.kernel_events)))
        tr.kernel_events = None

    out, tr, aux = head_leg(lambda: cls(model, SolverCfg(), seed=2020, precision=precision), args, dev, precision, batch, steps, warmup,
                            start_kernel_events, read_kernel_events)
    out.update(fg_rows=int(aux["fg"]["live"]), route="unfused (timing only)" if unfused else "fused",
               predictor_ms=round(kernel_ms[0][0], 4), predictor_launches=5 if unfused else 2, predictor_with_copies_ms=round(kernel_ms[0][1], 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="2,8")
    ap.add_argument("--precisions", default="bf16x3")
    ap.add_argument("--unfused", action="store_true", help="also time the step with the predictor as the axis stage runs its last layer")
    a = ap.parse_args()
    from bench import build_detector
    from train_bench import synthetic_targets
    from articulation3d_amd.streams import side

    dev = "cuda:0"
    side(0)  # the package's streams first (streams.py)
    model, _cfg = build_detector(0.5, dev)
    legs = []
    for prec in [p for p in a.precisions.split(",") if p]:
        for b in (int(v) for v in a.batches.split(",")):
            for unfused in ([False, True] if a.unfused else [False]):
                legs.append(leg(model, dev, prec, b, a.steps, a.warmup, synthetic_targets(b, 2020), unfused))
                print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"metric": "images/s through the step3_planehead training step", "steps": a.steps, "warmup": a.warmup, "legs": legs}))


if __name__ == "__main__":
    main()
