#!/usr/bin/env python3
"""Throughput of the stage-5 training step (configs/step3_depth.yaml: the depth head over the frozen detector) on one MI355X.

    python tools/train_depth_bench.py [--steps K --warmup W --batches 2,8 --precisions bf16x3 --kernel-batch 8 --kernel-reps 20]

One step = the frozen detector's forward pass + the depth decoder's forward and backward pass (ten training-mode batch norms, the masked
L1 loss at 480 x 640) + the two-range SGD, on synthetic 480x640 frames (tools/train_bench.py's boxes, a smooth synthetic depth map with a
hole).  Per (precision, batch): images/s over K timed steps after W untimed ones, the milliseconds of each phase (device events on the
main stream at the phase boundaries of one extra step: frozen forward, depth forward, loss + backward, exchange + SGD) and the peak memory.
`kernels`: every launch group of csrc/depth_train.hip alone at the shapes of a --kernel-batch image step, device events around
--kernel-reps back-to-back calls after 3 untimed ones: the milliseconds per call and the achieved GB/s = the bytes the call must move
(computed from the shapes, below) over that time.  ONE JSON line on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def synthetic_depth(batch, h=480, w=640):
    yy, xx = torch.meshgrid(torch.arange(float(h)), torch.arange(float(w)), indexing="ij")
    d = torch.stack([1.0 + 2.0 * yy / h + 0.5 * torch.sin(xx / 40 + i) for i in range(batch)])
    d[:, h // 5: h // 3, w // 3: 2 * w // 3] = 0.0
    return d


def leg(model, dev, precision, batch, steps, warmup, targets):
    from articulation3d_amd.training import SolverCfg
    from articulation3d_amd.training_depth import DepthTrainer
    from articulation3d_amd.utils.synthetic import synthetic_frames

    frames = torch.from_numpy(synthetic_frames(batch, seed=2020)).to(dev)
    args = (frames, [t[0] for t in targets], [t[1] for t in targets], synthetic_depth(batch).to(dev))
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    tr = DepthTrainer(model, SolverCfg(), seed=2020, precision=precision)
    for _ in range(warmup):
        tr.step(*args)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        losses, aux = tr.step(*args)  # (held until the next step returns, as a training loop holds them)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    tr.phase_events = []  # one instrumented step
    losses, aux = tr.step(*args)
    torch.cuda.synchronize()
    ev = tr.phase_events
    split = {ev[i][0]: round(ev[i - 1][1].elapsed_time(ev[i][1]), 3) for i in range(1, len(ev))}
    return {"precision": precision, "images_per_gpu": batch, "images_per_s": round(batch * steps / el, 2), "ms_per_step": round(1e3 * el / steps, 3),
            "ms_split": split, "valid_pixels": int(aux["depth_valid"]), "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2),
            "losses": {k: round(float(v), 5) for k, v in losses.items()}}


def kernel_legs(dev, batch, reps):
    """Each launch group alone at the shapes of a `batch`-image step -> [{kernel, shape, launches, bytes, ms, gb_per_s}]."""
    from articulation3d_amd import train_ops as T

    out = []

    def timed(name, shape, launches, nbytes, fn):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / reps
        out.append({"kernel": name, "shape": shape, "launches": launches, "bytes": int(nbytes), "ms": round(ms, 4), "gb_per_s": round(nbytes / ms / 1e6, 1)})

    rn = lambda *s: torch.randn(*s, device=dev)
    for (h, w, c), what in (((240, 320, 64), "deconv5"), ((120, 160, 128), "conv5 / deconv4")):
        z, dy, g, bt = rn(batch, h, w, c), rn(batch, h, w, c), torch.rand(c, device=dev) + 0.5, rn(c)
        y, mean, invstd, _ = T.bn_train_forward(z, g, bt, act=1)
        fb, bb = T.bn_train_bytes(batch * h * w, c)
        rm, rv, dz, dg, db = torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.empty_like(z), torch.empty(c, device=dev), torch.empty(c, device=dev)
        shape = f"{batch}x{h}x{w}x{c} ({what})"
        timed("a3d_bn_train_forward", shape, 3, fb, lambda: T.bn_train_forward(z, g, bt, act=1, running_mean=rm, running_var=rv, y=y))
        timed("a3d_bn_train_backward", shape, 3, bb, lambda: T.bn_train_backward(dy, z, y, mean, invstd, g, act=1, dgamma=dg, dbeta=db, dz=dz))
        del z, dy, y, dz
    h, w = 240, 320
    d, gt = rn(batch, h, w), torch.rand(batch, 2 * h, 2 * w, device=dev) * 3
    gt[:, :100] = 0.0
    # d read, gt read, dd written, then dd read and written again by the scaling launch
    timed("a3d_depth_loss", f"{batch}x{h}x{w} -> {2 * h}x{2 * w}", 2, batch * h * w * 4 * (1 + 4 + 1 + 2), lambda: T.depth_loss(d, gt, loss_weight=1.0))
    x, wp = rn(batch, h, w, 64), rn(9, 64)
    timed("a3d_depth_pred_backward", f"{batch}x{h}x{w}x64", 2, batch * h * w * 4 * (64 + 64 + 1), lambda: T.depth_pred_backward(x, d, wp))
    del x
    a, b2 = rn(batch, 120, 160, 128), rn(batch, 120, 160, 128)
    timed("a3d_ups2_concat", f"{batch}x120x160x(128+128) -> {batch}x240x320x256", 1, batch * 120 * 160 * 256 * 4 * (1 + 4), lambda: T.ups2_concat(a, b2))
    del a, b2
    up = rn(batch, 15, 20, 128)
    timed("a3d_resize_bilinear_backward_nhwc", f"{batch}x15x20x128 -> 16x20", 1, batch * 128 * 4 * (15 * 20 + 16 * 20), lambda: T.resize_bilinear_backward(up, 16, 20))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="2,8")
    ap.add_argument("--precisions", default="bf16x3")
    ap.add_argument("--kernel-batch", type=int, default=8)
    ap.add_argument("--kernel-reps", type=int, default=20)
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
    kernels = kernel_legs(dev, a.kernel_batch, a.kernel_reps) if a.kernel_batch > 0 else []
    print(json.dumps({"metric": "images/s through the step3_depth training step", "steps": a.steps, "warmup": a.warmup, "legs": legs,
                      "kernel_batch": a.kernel_batch, "kernels": kernels}))


if __name__ == "__main__":
    main()
