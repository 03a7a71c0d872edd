#!/usr/bin/env python3
"""Measures the PNG decode path end to end, from file bytes in host memory to pixels, against what the package does without it: PIL on
one host thread.  The numbers decide what `--decoder auto` does with PNG input (tools/inference.py: PNG_AUTO_ON_GPU) and the default
`chunk` of png.png_decode.

    python tools/png_decode_bench.py [--frames 90] [--repeats 3] [--chunks 8,32,90] [--kernels]

Five classes of 480 x 640 file (MEASUREMENTS.md, "PNG decode"): PIL-written smooth frames, camera-like frames (smooth + sigma 3 noise),
noise frames, the package's own files (png.png_encode of the camera-like frames), and PIL's compress_level 0 (stored blocks).
Per class and frames per call, `--repeats` times, the two sides alternating behind one untimed call of each:
  to_host    frames/s from file bytes to a host array of pixels -- what decode_images returns: png_decode + the copy back, against
             PIL alone;
  to_device  frames/s from file bytes to uint8 RGB on the device: png_decode, against PIL + the upload.
Every timing ends in a synchronise.  `gpu_wins` is true when the slowest GPU repetition beats the fastest PIL repetition, to the host,
at that chunk.  `--kernels` adds the device time of every launch of one call, from torch.profiler's kernel records, in a run of its
own.  One JSON object per line."""
from __future__ import annotations

import argparse
import io
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def smooth(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ph = rng.uniform(0, 2 * np.pi, (3, 2))
    return np.stack([np.clip(np.rint(128 + 70 * np.sin(xx / (40.0 + 25 * c) + ph[c, 0]) + 50 * np.cos(yy / (55.0 - 10 * c) + ph[c, 1])), 0, 255)
                     for c in range(3)], axis=2).astype(np.uint8)


def pil_files(frames, **options):
    from PIL import Image

    out = []
    for fr in frames:
        buf = io.BytesIO()
        Image.fromarray(fr).save(buf, "PNG", **options)
        out.append(buf.getvalue())
    return out


def classes(n, H=480, W=640, distinct=6):
    import png_ref
    from articulation3d_amd import png

    cam = [png_ref.camera(H, W, seed=k) for k in range(distinct)]
    sets = {"pil_smooth": pil_files([smooth(H, W, k) for k in range(distinct)]), "pil_camera": pil_files(cam),
            "pil_noise": pil_files([png_ref.noise(H, W, k) for k in range(distinct)]),
            "own_camera": png.png_encode(torch.from_numpy(np.stack(cam)).cuda()), "pil_level0_camera": pil_files(cam, compress_level=0)}
    return {name: [files[k % distinct] for k in range(n)] for name, files in sets.items()}


def time_gpu(pngs, chunk, to_host):
    from articulation3d_amd import png

    torch.cuda.synchronize()
    t = time.perf_counter()
    out = png.png_decode(pngs, chunk=chunk)
    if to_host:
        out = out.cpu().numpy()
    torch.cuda.synchronize()
    return len(pngs) / (time.perf_counter() - t), out


def time_pil(pngs, to_host):
    from PIL import Image

    torch.cuda.synchronize()
    t = time.perf_counter()
    out = np.stack([np.asarray(Image.open(io.BytesIO(p)).convert("RGB")) for p in pngs])
    if not to_host:
        out = torch.from_numpy(out).cuda()
    torch.cuda.synchronize()
    return len(pngs) / (time.perf_counter() - t), out


def kernel_times(pngs, chunk):
    """Device time per launch of one a3d_png_decode call, from torch.profiler: {kernel name: [microseconds]}."""
    from torch.profiler import ProfilerActivity, profile

    from articulation3d_amd import png

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        png.png_decode(pngs[:chunk], chunk=chunk)
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        name = re.search(r"png_\w+_kernel|Memset", e.name)
        if name and e.device_time > 0:
            out.setdefault(name.group(0), []).append(round(e.device_time, 1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", default=90, type=int)
    ap.add_argument("--repeats", default=3, type=int)
    ap.add_argument("--chunks", default="8,32,90")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    chunks = [int(c) for c in args.chunks.split(",")]
    for name, pngs in classes(args.frames).items():
        row = {"class": name, "frames": len(pngs), "file_bytes": round(sum(map(len, pngs)) / len(pngs))}
        want = time_pil(pngs[:4], True)[1]
        assert np.array_equal(time_gpu(pngs[:4], 4, True)[1], want), "the GPU decoder and PIL disagree"
        for to_host in (True, False):
            key = "to_host" if to_host else "to_device"
            for chunk in chunks:
                time_gpu(pngs, chunk, to_host)  # untimed: the scratch and the output of this chunk size come from the allocator's blocks afterwards
                gpu, pil = [], []
                for _ in range(args.repeats):
                    pil.append(round(time_pil(pngs, to_host)[0], 1))
                    gpu.append(round(time_gpu(pngs, chunk, to_host)[0], 1))
                row[f"{key}_chunk{chunk}"] = {"pil_fps": pil, "gpu_fps": gpu, "gpu_wins": min(gpu) > max(pil)}
        if args.kernels:
            for chunk in chunks:
                try:
                    row[f"gpu_kernel_us_chunk{chunk}"] = kernel_times(pngs, chunk)
                except Exception as e:  # a profiler that is not there is not a failed measurement
                    row[f"gpu_kernel_us_chunk{chunk}"] = f"unavailable: {type(e).__name__}: {e}"
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
