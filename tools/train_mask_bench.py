#!/usr/bin/env python3
"""Throughput of the stage-3 training step (configs/step3_mask.yaml: the mask head over the frozen detector) on one MI355X.

    python tools/train_mask_bench.py [--steps K --warmup W --batches 2,8 --precisions bf16x3]

One step = the frozen detector's forward pass + the mask head's forward and backward pass over the live foreground rows + SGD, on
synthetic 480x640 frames (tools/train_bench.py's boxes, the ellipse inscribed in each box as its bitmask).  Per (precision, batch):
images/s over K timed steps after W untimed ones, the live foreground rows, the milliseconds of each phase (device events on the main
stream at the phase boundaries of one extra step: frozen forward, mask forward + targets, loss + backward, exchange + SGD), the time of
a3d_mask_loss (both launches, device events around the call, the median of the timed steps) beside the bytes it moves and the share of
the 6.3 TB/s HBM rate (MI355X_MICROARCH: the achievable stream rate) that is, and the peak memory.  ONE JSON line on stdout.
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

HBM_BYTES_PER_S = 6.3e12


def ellipse_masks(boxes, H=480, W=640):
    yy, xx = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    return torch.stack([(((xx - (x1 + x2) / 2) / ((x2 - x1) / 2)) ** 2 + ((yy - (y1 + y2) / 2) / ((y2 - y1) / 2)) ** 2) <= 1
                        for x1, y1, x2, y2 in boxes.tolist()])


def leg(model, dev, precision, batch, steps, warmup, targets):
    from train_head_bench import head_leg
    from articulation3d_amd import train_ops as T
    from articulation3d_amd.training import SolverCfg
    from articulation3d_amd.training_mask import MaskTrainer
    from articulation3d_amd.utils.synthetic import synthetic_frames

    frames = torch.from_numpy(synthetic_frames(batch, seed=2020)).to(dev)
    args = (frames, [t[0] for t in targets], [t[1] for t in targets], [ellipse_masks(t[0]).to(dev) for t in targets])
    kernel_ms = []

    def start_kernel_events(tr):
        tr.kernel_events = []

    def read_kernel_events(tr):  # a3d_mask_loss over the timed steps only: the instrumented step runs without these events
        kernel_ms.append(statistics.median(a.elapsed_time(b) for a, b in tr.kernel_events))
        tr.kernel_events = None

    out, tr, aux = head_leg(lambda: MaskTrainer(model, SolverCfg(), seed=2020, precision=precision), args, dev, precision, batch, steps,
                            warmup, start_kernel_events, read_kernel_events)
    live, ms = int(aux["fg"]["live"]), kernel_ms[0]
    nbytes = T.mask_loss_bytes(live, tr.pool_size, tr.dim)
    out.update(fg_rows=live, mask_loss={"ms": round(ms, 4), "bytes": nbytes, "tb_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3),
                                        "share_of_hbm_rate": round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="2,8")
    ap.add_argument("--precisions", default="bf16x3")
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
            legs.append(leg(model, dev, prec, b, a.steps, a.warmup, synthetic_targets(b, 2020)))
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"metric": "images/s through the step3_mask training step", "steps": a.steps, "warmup": a.warmup, "legs": legs}))


if __name__ == "__main__":
    main()
