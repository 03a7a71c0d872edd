#!/usr/bin/env python3
"""Timing of the Motion-JPEG path (articulation3d_amd/video.py, csrc/jpeg.hip) -> one JSON line.

    python tools/video_bench.py [--frames 32] [--instances 4] [--quality 90] [--iters 1000]

Two seeded clips of `--frames` 480x640 frames with hand-made detections (tests/render_ref.make_instances): `noise`, the clip of
tools/render_bench.py (uniform noise frames: the worst case for an encoder), and `smooth` (tests/mjpeg_ref.smooth_frames: what a
camera frame costs).  Before anything is timed, the first row's file is compared with tests/mjpeg_ref.py byte for byte.  Per clip:
  * encode_us / pack_us: the two library calls on a chunk of 8 rendered rows [8,480,2560,3] already on the device, from device events
    around `--iters` back-to-back calls after a warm-up -- a3d_jpeg_encode is three launches (transform, entropy, offsets), a3d_jpeg_pack
    one -- with the bytes each must move (encode: the pixels read, the coefficients written and read, the stream written; pack: the
    stream read and written) and the rate that makes;
  * jpeg_fps: render_clip_jpeg end to end -- host tables, both render launches and the encoder per chunk, lengths, pack and the copy
    of the used bytes -- frames over wall time, the median of three passes after a warm-up pass and their range; bytes_per_frame: the
    files it yields;
  * png_fps / pil_jpeg_fps: render_clip (raw rows over PCIe) + PIL's PNG / JPEG encoder (same quality, 4:4:4) on the host, per row.
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


def _events(call, iters):
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--instances", type=int, default=4)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--host-frames", type=int, default=4, help="rows the PIL encoders are timed on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_bench needs a GPU")
    import mjpeg_ref as M
    import render_ref as R
    from PIL import Image

    from articulation3d_amd import opt_ops, render, video

    dev = torch.device("cuda")
    F, q = args.frames, args.quality
    rows_out = []
    for name in ("noise", "smooth"):
        rng = np.random.default_rng(100 + args.instances)
        frames = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8) if name == "noise" else M.smooth_frames(F, H, W)
        preds = [R.make_instances(rng, H, W, args.instances) for _ in range(F)]
        dframes = torch.from_numpy(frames).to(dev)

        # correctness first: the first row's file against the law
        first = next(render.render_clip(dframes[:1], preds[:1], preds[:1], chunk=1))[0].copy()
        mine = next(video.render_clip_jpeg(dframes[:1], preds[:1], preds[:1], quality=q, chunk=1))[0]
        assert mine == M.encode_frame(first, q), "kernel and reference disagree"

        # the two library calls on one chunk of 8 rows
        n = min(8, F)
        stage = torch.empty((n, H, 4 * W, 3), dtype=torch.uint8, device=dev)
        render.render_panels(dframes[:n], preds[:n], out=stage, col=0)
        render.render_panels(dframes[:n], preds[:n], out=stage, col=2 * W)
        enc = video._Encoder(n, H, 4 * W, dev)
        enc.encode(stage, q)
        torch.cuda.synchronize()
        total = int(enc.frame_off[n].item())
        packed = torch.empty(total, dtype=torch.uint8, device=dev)
        encode_us = _events(lambda: opt_ops.jpeg_encode_into(stage, q, enc.coef, enc.slots, enc.seg_len, enc.seg_off, enc.frame_off), args.iters)
        pack_us = _events(lambda: opt_ops.jpeg_pack_into(enc.slots, enc.seg_off, enc.seg_len, n, H, 4 * W, packed), args.iters)
        coef_bytes = n * enc.rows * enc.mcus * 384
        encode_move, pack_move = stage.numel() + 2 * coef_bytes + total, 2 * total

        # end to end (four passes: the first also pins the buffers and warms the pool; the other three give the figure and its spread)
        jpeg_runs = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sizes = [len(j) for chunk in video.render_clip_jpeg(dframes, preds, preds, quality=q, chunk=8) for j in chunk]
            jpeg_runs.append(time.perf_counter() - t0)
        assert len(sizes) == F
        jpeg_runs = sorted(jpeg_runs[1:])
        jpeg_s = jpeg_runs[1]

        # the host paths: render_clip's rows through PIL
        k = min(args.host_frames, F)
        host_rows = [r.copy() for chunk in render.render_clip(dframes[:k], preds[:k], preds[:k], chunk=8) for r in chunk]
        clip_runs = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for chunk in render.render_clip(dframes, preds, preds, chunk=8):
                pass
            clip_runs.append(time.perf_counter() - t0)
        clip_s = sorted(clip_runs[1:])[1]
        t0 = time.perf_counter()
        for r in host_rows:
            Image.fromarray(r).save(io.BytesIO(), format="PNG")
        png_s = (time.perf_counter() - t0) / k
        t0 = time.perf_counter()
        pil_sizes = []
        for r in host_rows:
            buf = io.BytesIO()
            Image.fromarray(r).save(buf, format="JPEG", quality=q, subsampling=0)
            pil_sizes.append(buf.tell())
        pil_s = (time.perf_counter() - t0) / k
        rows_out.append({"clip": name, "frames": F, "instances_per_frame": args.instances, "quality": q,
                         "encode_us": round(encode_us, 1), "encode_must_move_MB": round(encode_move / 1e6, 2), "encode_gbps": round(encode_move / encode_us / 1e3, 1),
                         "pack_us": round(pack_us, 1), "pack_must_move_MB": round(pack_move / 1e6, 2), "pack_gbps": round(pack_move / pack_us / 1e3, 1),
                         "chunk_frames": n, "encode_fps_device": round(n / (encode_us + pack_us) * 1e6, 1),
                         "jpeg_fps": round(F / jpeg_s, 1), "jpeg_fps_range": [round(F / jpeg_runs[2], 1), round(F / jpeg_runs[0], 1)], "bytes_per_frame": int(np.mean(sizes)), "raw_bytes_per_frame": H * 4 * W * 3,
                         "render_clip_fps": round(F / clip_s, 1),
                         "png_fps": round(1 / (clip_s / F + png_s), 2), "png_encode_ms": round(png_s * 1e3, 1),
                         "pil_jpeg_fps": round(1 / (clip_s / F + pil_s), 2), "pil_jpeg_encode_ms": round(pil_s * 1e3, 1), "pil_jpeg_bytes_per_frame": int(np.mean(pil_sizes))})
    print(json.dumps({"bench": "video_mjpeg", "device": torch.cuda.get_device_name(0), "HxW": [H, 4 * W], "iters": args.iters, "rows": rows_out}))


if __name__ == "__main__":
    main()
