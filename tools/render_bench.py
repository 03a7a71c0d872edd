#!/usr/bin/env python3
"""Timing of the visualisation panels (articulation3d_amd/render.py, csrc/render.hip) -> one JSON line.

    python tools/render_bench.py [--frames 32] [--instances 4 16] [--iters 200]

Per instance count, on a seeded clip of `--frames` 480x640 frames with hand-made detections (tests/render_ref.make_instances):
  * launch_us / gbps: one a3d_render_panels launch over tables already on the device (device events around `--iters` back-to-back
    launches after a warm-up), and the bytes it must move over that time: per frame one frame read, two panels written, one mask
    word per instance per 32 pixels, plus the tables;
  * clip_fps: render_clip end to end -- build_layers on the host, mask packing, both launches per chunk and the D2H copy of the
    four-panel rows through its pinned ring -- frames over wall time, ended by the last chunk's arrival;
  * host_ref_fps: tests/render_ref.py (numpy) on the first frames of the same clip, the only available stand-in for a host path;
  * png_fps: PIL's PNG encoder on one four-panel row (what bounds --vis png), d2h_gbps: the pinned copy alone.
Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 480, 640


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--instances", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--ref-frames", type=int, default=2, help="frames of the clip the numpy reference renders")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_bench needs a GPU")
    import render_ref as R
    from PIL import Image

    from articulation3d_amd import opt_ops, render

    dev = torch.device("cuda")
    F = args.frames
    rows = []
    for n_inst in args.instances:
        rng = np.random.default_rng(100 + n_inst)
        frames = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
        preds = [R.make_instances(rng, H, W, n_inst) for _ in range(F)]
        tables = render.build_layers(preds, H, W)
        normals = render.unit_normals(preds, tables)
        masks = torch.cat([(p.pred_masks > 0.5).to(torch.uint8) for p in preds]).to(dev)
        bits = opt_ops.pack_masks(masks)
        dframes = torch.from_numpy(frames).to(dev)
        out = torch.empty((F, H, 4 * W, 3), dtype=torch.uint8, device=dev)
        up = [render._dev_bytes(a, dev) for a in (tables.layer_off, tables.layers, tables.pieces, tables.inst_off, tables.inst_row)]
        dn = normals.to(dev)
        call = lambda: opt_ops.render_panels_tables(dframes, *up, dn, bits, out, col=0)
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        launch_us = e0.elapsed_time(e1) * 1e3 / args.iters
        words = opt_ops.words_per_mask(H, W)
        table_bytes = sum(a.nbytes for a in (tables.layer_off, tables.layers, tables.pieces, tables.inst_off, tables.inst_row)) + normals.numel() * 4
        must_move = F * H * W * 3 * 3 + len(tables.inst_row) * words * 4 + table_bytes

        # end to end, host table building and D2H included (two passes: the first also pins the buffers and warms the pool)
        clip_s = None
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = 0
            for chunk in render.render_clip(dframes, preds, preds, chunk=8):
                got += len(chunk)
            clip_s = time.perf_counter() - t0
            assert got == F
        t0 = time.perf_counter()
        tb = render.build_layers(preds, H, W)
        render.unit_normals(preds, tb)
        build_s = time.perf_counter() - t0

        # the D2H copy alone
        pinned = torch.empty((F, H, 4 * W, 3), dtype=torch.uint8).pin_memory()
        pinned.copy_(out)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(out, non_blocking=True)
        torch.cuda.synchronize()
        d2h_s = time.perf_counter() - t0

        # the numpy reference and the PNG encoder on the host
        k = min(args.ref_frames, F)
        hbits = R.pack_bits(np.concatenate([p.pred_masks.numpy() for p in preds[:k]]))
        tk = render.build_layers(preds[:k], H, W)
        t0 = time.perf_counter()
        ref = R.render_tables(frames[:k], tk, render.unit_normals(preds[:k], tk).numpy(), hbits, np.zeros((k, H, 2 * W, 3), np.uint8))
        ref_s = time.perf_counter() - t0
        assert np.array_equal(ref, out[:k, :, :2 * W].cpu().numpy()), "kernel and reference disagree"
        row = pinned[0].numpy()
        t0 = time.perf_counter()
        for _ in range(3):
            Image.fromarray(row).save(io.BytesIO(), format="PNG")
        png_s = (time.perf_counter() - t0) / 3
        rows.append({"instances_per_frame": n_inst, "frames": F, "layers": int(len(tables.layers)), "pieces": int(len(tables.pieces)),
                     "launch_us": round(launch_us, 2), "must_move_MB": round(must_move / 1e6, 2), "gbps": round(must_move / launch_us / 1e3, 1),
                     "clip_fps": round(F / clip_s, 1), "build_layers_ms_per_frame": round(build_s / F * 1e3, 3),
                     "d2h_gbps": round(pinned.numel() / d2h_s / 1e9, 2), "d2h_fps": round(F / d2h_s, 1),
                     "host_ref_fps": round(k / ref_s, 2), "png_fps": round(1 / png_s, 2)})
    print(json.dumps({"bench": "render_panels", "device": torch.cuda.get_device_name(0), "HxW": [H, W], "iters": args.iters, "rows": rows}))


if __name__ == "__main__":
    main()
