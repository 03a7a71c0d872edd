#!/usr/bin/env python3
"""Timing and size of the PNG path (articulation3d_amd/png.py, csrc/png.hip) against render_clip + PIL -> one JSON line.

    python tools/png_bench.py [--frames 32] [--instances 4] [--iters 50] [--check-law]

The workload of tools/video_bench.py: two seeded clips of `--frames` 480x640 frames with hand-made detections, `noise` (uniform noise
frames: nothing to compress but the panels' flat parts) and `smooth` (tests/mjpeg_ref.smooth_frames: what a camera frame costs), rendered
to rows of 480 x 2560.  Before anything is timed every file of a pass is opened with PIL and compared with render_clip's row, exactly;
`--check-law` also compares the first row's file with tests/png_ref.py byte for byte (tens of seconds of Python per clip).  Per clip, in
one run:
  * pil_png_fps: what `--png-encoder pil` does -- render_clip (raw rows over PCIe) and PIL's default save(format="PNG") of every row --
    frames over wall time, the median of three passes after a warm-up pass;
  * gpu_png_fps: render_clip_png end to end -- both render launches, scan, the histograms to the host, the Huffman codes, emit, pack, the
    copy of the used bytes, Adler fold, CRCs and file assembly -- the same way; speedup = gpu_png_fps / pil_png_fps;
  * scan_us / emit_us / pack_us: the three library calls on a chunk of 8 rendered rows already on the device, from device events around
    `--iters` back-to-back calls after a warm-up;
  * host_ms_per_frame: the host's shares of the end-to-end pass -- huffman (316 counts -> code, header, table, per frame) and
    crc_and_files (Adler fold, zlib.crc32 over the IDAT, joining the file) -- and crc_ms_per_frame, zlib.crc32 alone over the same bytes;
  * bytes_per_frame against pil_bytes_per_frame (PIL's default zlib level) and their ratio; kinds: how many segments took the stored,
    fixed and dynamic coding; source_frame_size_ratio: the same ratio on the clip's first 8 source frames [480,640,3] alone, which do not
    repeat themselves within a row as the four-panel rows do.
Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 480, 640


def _events(call, iters):
    for _ in range(3):
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--check-law", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_bench needs a GPU")
    import mjpeg_ref as M
    import render_ref as R
    from PIL import Image

    from articulation3d_amd import opt_ops, png, render

    dev = torch.device("cuda")
    F = args.frames
    rows_out = []
    for name in ("noise", "smooth"):
        rng = np.random.default_rng(100 + args.instances)
        frames = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8) if name == "noise" else M.smooth_frames(F, H, W)
        preds = [R.make_instances(rng, H, W, args.instances) for _ in range(F)]
        dframes = torch.from_numpy(frames).to(dev)

        # correctness first: every file opens to exactly render_clip's row
        rows = [r.copy() for chunk in render.render_clip(dframes, preds, preds, chunk=8) for r in chunk]
        files = [f for chunk in png.render_clip_png(dframes, preds, preds, chunk=8) for f in chunk]
        assert len(files) == F
        for row, f in zip(rows, files):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), row), "a file does not decode to its row"
        if args.check_law:
            import png_ref

            assert files[0] == png_ref.encode_frame(rows[0]), "kernel and reference disagree"

        # the three library calls on one chunk of 8 rows
        n = min(8, F)
        stage = torch.from_numpy(np.stack(rows[:n])).to(dev)
        enc = png._Encoder(n, H, 4 * W, dev)
        enc.scan(stage)
        enc.emit()
        torch.cuda.synchronize()
        total = int(enc.frame_off[n].item())
        kinds = np.bincount(enc.kind.cpu().numpy(), minlength=3).tolist()
        packed = torch.empty(total, dtype=torch.uint8, device=dev)
        scan_us = _events(lambda: opt_ops.png_scan_into(stage, enc.filt, enc.tok, enc.hist, enc.s1, enc.s2), args.iters)
        emit_us = _events(lambda: opt_ops.png_emit_into(enc.filt, enc.tok, enc.tab, n, H, 4 * W, enc.slots, enc.seg_len, enc.seg_off, enc.frame_off,
                                                        enc.kind), args.iters)
        pack_us = _events(lambda: opt_ops.png_pack_into(enc.slots, enc.seg_off, enc.seg_len, n, H, 4 * W, packed), args.iters)

        # end to end, both encoders (four passes each: the first pins the buffers and warms the pool)
        gpu_runs, seconds = [], {}
        for k in range(4):
            torch.cuda.synchronize()
            seconds = {}
            t0 = time.perf_counter()
            sizes = [len(f) for chunk in png.render_clip_png(dframes, preds, preds, chunk=8, seconds=seconds) for f in chunk]
            gpu_runs.append(time.perf_counter() - t0)
        gpu_runs = sorted(gpu_runs[1:])
        pil_runs = []
        for k in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pil_sizes = []
            for chunk in render.render_clip(dframes, preds, preds, chunk=8):
                for row in chunk:
                    buf = io.BytesIO()
                    Image.fromarray(row).save(buf, format="PNG")
                    pil_sizes.append(buf.tell())
            pil_runs.append(time.perf_counter() - t0)
        pil_runs = sorted(pil_runs[1:])
        t0 = time.perf_counter()
        for f in files:
            zlib.crc32(f)
        crc_s = (time.perf_counter() - t0) / F
        # size without the row's own repetition: the source frames alone (a row shows the frame twice, 3840 bytes apart)
        k = min(8, F)
        frame_sizes = [len(f) for f in png.png_encode(dframes[:k])]
        frame_pil = []
        for fr in frames[:k]:
            buf = io.BytesIO()
            Image.fromarray(fr).save(buf, format="PNG")
            frame_pil.append(buf.tell())
        gpu_fps, pil_fps = F / gpu_runs[1], F / pil_runs[1]
        rows_out.append({"clip": name, "frames": F, "instances_per_frame": args.instances, "chunk_frames": n,
                         "scan_us": round(scan_us, 1), "emit_us": round(emit_us, 1), "pack_us": round(pack_us, 1),
                         "device_fps": round(n / (scan_us + emit_us + pack_us) * 1e6, 1), "segment_kinds_stored_fixed_dynamic": kinds,
                         "gpu_png_fps": round(gpu_fps, 1), "gpu_png_fps_range": [round(F / gpu_runs[2], 1), round(F / gpu_runs[0], 1)],
                         "pil_png_fps": round(pil_fps, 2), "pil_png_fps_range": [round(F / pil_runs[2], 2), round(F / pil_runs[0], 2)],
                         "speedup": round(gpu_fps / pil_fps, 2),
                         "host_ms_per_frame": {k: round(v / F * 1e3, 3) for k, v in seconds.items()}, "crc_ms_per_frame": round(crc_s * 1e3, 3),
                         "bytes_per_frame": int(np.mean(sizes)), "pil_bytes_per_frame": int(np.mean(pil_sizes)),
                         "size_ratio": round(float(np.sum(sizes)) / float(np.sum(pil_sizes)), 4), "raw_bytes_per_frame": H * 4 * W * 3,
                         "source_frame_size_ratio": round(float(np.sum(frame_sizes)) / float(np.sum(frame_pil)), 4)})
    print(json.dumps({"bench": "png", "device": torch.cuda.get_device_name(0), "HxW": [H, 4 * W], "iters": args.iters, "rows": rows_out}))


if __name__ == "__main__":
    main()
