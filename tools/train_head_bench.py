"""The leg that tools/train_axis_bench.py and tools/train_mask_bench.py share: one head trainer over the frozen detector (a
training_head.HeadTrainer) through W untimed steps, K timed steps and one instrumented step."""
from __future__ import annotations

import time

import torch


def head_leg(make_trainer, args, dev, precision, batch, steps, warmup, before_timed=None, after_timed=None):
    """-> (the leg's JSON fields, the trainer, the instrumented step's aux).  `args`: what tr.step takes.  before_timed(tr) / after_timed(tr)
    run around the timed steps, outside the clock."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    tr = make_trainer()
    for _ in range(warmup):
        tr.step(*args)
    torch.cuda.synchronize()
    if before_timed is not None:
        before_timed(tr)
    t0 = time.perf_counter()
    for _ in range(steps):
        losses, aux = tr.step(*args)  # (held until the next step returns, as a training loop holds them)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if after_timed is not None:
        after_timed(tr)
    tr.phase_events = []  # one instrumented step
    losses, aux = tr.step(*args)
    torch.cuda.synchronize()
    ev = tr.phase_events
    split = {ev[i][0]: round(ev[i - 1][1].elapsed_time(ev[i][1]), 3) for i in range(1, len(ev))}
    out = {"precision": precision, "images_per_gpu": batch, "images_per_s": round(batch * steps / el, 2), "ms_per_step": round(1e3 * el / steps, 3),
           "fg_rows_per_image": round(float(aux["fg"]["count"].float().mean()), 2), "ms_split": split,
           "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2),
           "losses": {k: round(float(v), 5) for k, v in losses.items()}}
    return out, tr, aux
