#!/usr/bin/env python3
"""Throughput of the stage-2 training step (config/step2_axis.yaml: the articulation-axis head over the frozen detector) on one MI355X.

    python tools/train_axis_bench.py [--steps K --warmup W --batches 2,16 --precisions bf16x3,fp32,bf16]

One step = the frozen detector's forward pass + the axis head's forward and backward pass over the live foreground rows + SGD, on
synthetic 480x640 frames (tools/train_bench.py's targets plus [sin, cos, offset, valid] axis rows).  Per (precision, batch): images/s over K
timed steps after W untimed ones, the live foreground rows per image, the milliseconds of each phase (device events on the main stream at
the phase boundaries of one extra step: frozen forward, axis forward + loss, axis backward, exchange + SGD) and the peak memory.  The
`cap` leg repeats the 16-image bf16x3 point with targets built so that every image reaches its 128 foreground rows (cap_targets) --
the cost of the step at the cap.  ONE JSON line on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def cap_targets(model, dev, n, g=64):
    """Ground truth that brings every image to its 128 foreground rows: the first `g` proposals the frozen detector itself makes for that
    frame.  Each matches itself (IoU 1) and is appended once more as ground truth, so the sampler finds 2 g >= 128 foreground candidates.
    (64: the matcher's ground-truth limit per image.)"""
    from articulation3d_amd.training import DetectorTrainer, SolverCfg
    from articulation3d_amd.utils.synthetic import synthetic_frames
    from train_bench import synthetic_targets

    det = DetectorTrainer(model, SolverCfg(max_gt=g), seed=2020)
    frames = torch.from_numpy(synthetic_frames(n, seed=2020)).to(dev)
    tg = synthetic_targets(n, 2020)
    _, aux = det.frozen_forward(frames, [t[0] for t in tg], [t[1] for t in tg])
    pb, pc = aux["proposals"]
    assert int(pc.min()) >= g, pc
    out = [(pb[i, :g].cpu().clone(), torch.arange(g) % 2) for i in range(n)]
    del det
    torch.cuda.empty_cache()
    return out


def leg(model, dev, precision, batch, steps, warmup, targets, max_gt=16):
    from train_axis_exchange_check import axis_targets
    from train_head_bench import head_leg
    from articulation3d_amd.training import SolverCfg
    from articulation3d_amd.training_axis import AxisTrainer
    from articulation3d_amd.utils.synthetic import synthetic_frames

    frames = torch.from_numpy(synthetic_frames(batch, seed=2020)).to(dev)
    args = (frames, [t[0] for t in targets], [t[1] for t in targets], *axis_targets(targets, 7))
    out, _tr, aux = head_leg(lambda: AxisTrainer(model, SolverCfg(max_gt=max_gt), seed=2020, precision=precision), args, dev, precision,
                             batch, steps, warmup)
    fg = aux["fg"]["count"]
    out.update(fg_rows_min=int(fg.min()), fg_rows_max=int(fg.max()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="2,16")
    ap.add_argument("--precisions", default="bf16x3,fp32,bf16")
    ap.add_argument("--no-cap", action="store_true")
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
    cap = None
    if not a.no_cap:
        cap = leg(model, dev, "bf16x3", 16, a.steps, a.warmup, cap_targets(model, dev, 16), max_gt=64)
    print(json.dumps({"metric": "images/s through the step2_axis training step", "steps": a.steps, "warmup": a.warmup, "legs": legs, "cap": cap}))


if __name__ == "__main__":
    main()
