#!/usr/bin/env python3
"""Equality check of the stage-2 step's gradient exchange (training_axis.AxisTrainer; tests/test_gpu_axis_training.py runs it as a child
process, because it initialises a process group).

    python tools/train_axis_exchange_check.py [--backend gloo] [--steps 3]

Two ranks (gloo: both on this box's one GPU), each with its own batch.  For each gradient payload (fp32, bf16) two trainers start from the
same weights and run `--steps` optimiser steps: the segmented exchange ("1": the T tower's segment announced from the side stream it was
computed on, the R tower's from the main stream) against ONE all-reduce behind the backward pass ("0").  Parameters, momenta, losses and
`export_grads()` after the last step must be bit-identical; with the fp32 payload `export_grads()` must also equal the mean of the two
ranks' own gradients of that step (gathered separately).  One JSON line on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def axis_targets(tg, seed):
    """[sin, cos, offset, valid] rows per ground-truth box (every third without a valid axis)."""
    g = torch.Generator().manual_seed(seed)
    rot, tran = [], []
    for b, _c in tg:
        n = len(b)
        a = torch.rand(n, 2, generator=g) * 6.283185307179586
        v = (torch.arange(n) % 3 != 2).float()
        rot.append(torch.stack((a[:, 0].sin(), a[:, 0].cos(), torch.randn(n, generator=g), v), 1))
        tran.append(torch.stack((a[:, 1].sin(), a[:, 1].cos(), torch.zeros(n), torch.ones(n)), 1))
    return rot, tran


def run(rank, world, backend, port, steps, batch, precision, out):
    import torch.distributed as dist

    from train_bench import synthetic_targets
    from bench import build_detector
    from articulation3d_amd.streams import side
    from articulation3d_amd.training_axis import AxisTrainer
    from articulation3d_amd.utils.synthetic import synthetic_frames
    from articulation3d_amd import parallel

    torch.cuda.set_device(0)
    dev = "cuda:0"
    side(0)  # the package's streams first (streams.py)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group(backend, rank=rank, world_size=world)
    model, _cfg = build_detector(0.5, dev)
    frames = torch.from_numpy(synthetic_frames(batch, seed=2020 + rank)).to(dev)  # (rank-dependent data)
    tg = synthetic_targets(batch, 2020 + rank)
    gtb, gtc = [t[0] for t in tg], [t[1] for t in tg]
    rot, tran = axis_targets(tg, 31 + rank)
    res = {}
    for payload in ("fp32", "bf16"):
        ends, mean_rel, own_differs = [], None, None
        for form in ("1", "0"):
            tr = AxisTrainer(model, seed=5, precision=precision, grad_payload=payload, grad_overlap=form)
            parallel.GRAD_STATS.update(steps=0, segments=0, bytes=0, host_s=0.0)
            own = None
            for it in range(steps):
                if it == steps - 1 and form == "0" and payload == "fp32":  # this rank's own gradient of the last step: no exchange, no update
                    tr.forward_backward(frames, gtb, gtc, rot, tran)
                    own = tr.grads.cpu().clone()
                losses, _ = tr.step(frames, gtb, gtc, rot, tran)
            torch.cuda.synchronize()
            exp = {k: v.cpu() for k, v in tr.export_grads().items()}
            if own is not None:  # export_grads at world 2 = the mean of the ranks' own gradients
                both = [torch.zeros_like(own) for _ in range(world)]
                dist.all_gather(both, own)
                own_differs = not torch.equal(both[0], both[1])
                tr.grads.copy_(((both[0].double() + both[1].double()) / world).float().to(dev))
                tr._grad_scale = 1.0
                want = {k: v.cpu() for k, v in tr.export_grads().items()}
                mean_rel = max(float((exp[k].double() - want[k].double()).norm() / (want[k].double().norm() + 1e-30)) for k in want)
            ends.append((tr.params.clone(), tr.momentum.clone(), {k: float(v) for k, v in losses.items()}, exp, dict(parallel.GRAD_STATS)))
            del tr
            torch.cuda.empty_cache()
        (p0, m0, l0, e0, s0), (p1, m1, l1, e1, s1) = ends
        res[payload] = {"params_equal": bool(torch.equal(p0, p1)), "momentum_equal": bool(torch.equal(m0, m1)), "losses_equal": l0 == l1,
                        "export_grads_equal": all(torch.equal(e0[k], e1[k]) for k in e0), "finite": bool(torch.isfinite(p0).all()),
                        "segments_per_step": [s0["segments"] // max(steps, 1), s1["segments"] // max(steps, 1)],
                        "export_vs_mean_rel": mean_rel, "ranks_differ": own_differs}
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        line = json.dumps({"world": world, "backend": backend, "steps": steps, "batch": batch, "precision": precision, "result": res})
        if out is None:
            print(line)
        else:
            out.put(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default="gloo")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    port = _free_port()
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")  # (this parent never touches the GPU)
    q = ctx.Queue()
    procs = [ctx.Process(target=run, args=(r, 2, a.backend, port, a.steps, a.batch, a.precision, q)) for r in range(2)]
    for p in procs:
        p.start()
    line = q.get(timeout=1500)
    for p in procs:
        p.join(timeout=120)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    print(line)


if __name__ == "__main__":
    main()
