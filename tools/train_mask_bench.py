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
import time

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
    from articulation3d_amd import train_ops as T
    from articulation3d_amd.training import SolverCfg
    from articulation3d_amd.training_mask import MaskTrainer
    from articulation3d_amd.utils.synthetic import synthetic_frames

    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    tr = MaskTrainer(model, SolverCfg(), seed=2020, precision=precision)
    frames = torch.from_numpy(synthetic_frames(batch, seed=2020)).to(dev)
    gtb, gtc = [t[0] for t in targets], [t[1] for t in targets]
    gtm = [ellipse_masks(t[0]).to(dev) for t in targets]
    for _ in range(warmup):
        tr.step(frames, gtb, gtc, gtm)
    torch.cuda.synchronize()
    tr.kernel_events = []
    t0 = time.perf_counter()
    for _ in range(steps):
        losses, aux = tr.step(frames, gtb, gtc, gtm)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    kernel_ms = statistics.median(a.elapsed_time(b) for a, b in tr.kernel_events)
    tr.kernel_events = None
    tr.phase_events = []  # one instrumented step
    losses, aux = tr.step(frames, gtb, gtc, gtm)
    torch.cuda.synchronize()
    ev = tr.phase_events
    split = {ev[i][0]: round(ev[i - 1][1].elapsed_time(ev[i][1]), 3) for i in range(1, len(ev))}
    fg = aux["fg"]["count"].float().cpu()
    live = int(aux["fg"]["live"])
    nbytes = T.mask_loss_bytes(live, tr.pool_size, tr.dim)
    out = {"precision": precision, "images_per_gpu": batch, "images_per_s": round(batch * steps / el, 2), "ms_per_step": round(1e3 * el / steps, 3),
           "fg_rows": live, "fg_rows_per_image": round(float(fg.mean()), 2), "ms_split": split,
           "mask_loss": {"ms": round(kernel_ms, 4), "bytes": nbytes, "tb_per_s": round(nbytes / (kernel_ms * 1e-3) / 1e12, 3),
                         "share_of_hbm_rate": round(nbytes / (kernel_ms * 1e-3) / HBM_BYTES_PER_S, 3)},
           "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2),
           "losses": {k: round(float(v), 5) for k, v in losses.items()}}
    del tr
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
