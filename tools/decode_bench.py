#!/usr/bin/env python3
"""Measures the JPEG decode path end to end, from file bytes in host memory to uint8 RGB on the device, against what the package did
before it had a decoder: PIL on one host thread plus the upload.

    python tools/decode_bench.py [--frames 90] [--repeats 3] [--chunks 8,32] [--kernels] [--splits 32,64,128,256]
    python tools/decode_bench.py --rounds [--splits 32,64,128,256]      (no GPU: the host model's convergence figures)

Four classes of stream (MEASUREMENTS.md, "JPEG decode"):
  (a) the package's own files, video.jpeg_encode at quality 90: 480 x 2560 visualisation rows and 480 x 640 frames (4:4:4, one MCU row
      per restart interval);
  (b) PIL 480 x 640 quality-90 4:2:0 files without restart intervals;
  (c) the same with restart_marker_rows=1;
  (d) the same with restart_marker_blocks=1 and =5: units of one or a few subsequences, 1 200 and 240 of them per frame.
Per class and chunk: frames/s of video.jpeg_decode (parse + upload + kernels, synchronised at the end), `--repeats` times behind one
untimed call; frames/s of PIL + upload, as often; the bytes that cross PCIe and the bytes the kernels move; then the same call at
every subsequence size of `--splits` for the largest chunk.  `--kernels` adds the device time of every launch of one call, from
torch.profiler's kernel records.
`--rounds` runs nowhere near a GPU: per class it prints the subsequences and the synchronisation rounds of the longest unit of the
first file under tests/jpeg_split_ref.py, the scheme's host model (class (a) is then written by tests/mjpeg_ref.py, the encoder's law,
whose bytes are the package's own).  One JSON object per line."""
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


def smooth_frames(n, H, W, seed=5):
    """Drifting low-frequency colour fields with mild noise: what a camera frame costs a JPEG codec (tests/mjpeg_ref.py has the same)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W, 3), np.uint8)
    for f in range(n):
        for c in range(3):
            ph = rng.uniform(0, 2 * np.pi, 3)
            v = 128 + 60 * np.sin(xx / (40.0 + 25 * c) + ph[0] + 0.1 * f) + 50 * np.cos(yy / (55.0 - 10 * c) + ph[1]) + 15 * np.sin((xx + yy) / 9.0 + ph[2])
            out[f, :, :, c] = np.clip(np.rint(v + rng.normal(0, 2.0, (H, W))), 0, 255).astype(np.uint8)
    return out


def pil_files(frames, **options):
    from PIL import Image

    out = []
    for fr in frames:
        buf = io.BytesIO()
        Image.fromarray(fr).save(buf, "JPEG", quality=90, subsampling=2, **options)
        out.append(buf.getvalue())
    return out


def classes(n, host_only=False):
    base = smooth_frames(min(n, 6), 480, 640)
    frames = base[np.arange(n) % len(base)]
    if host_only:
        import mjpeg_ref

        own, rows = [mjpeg_ref.encode_frame(base[0], 90)], [mjpeg_ref.encode_frame(np.concatenate([base[0]] * 4, 1), 90)]
    else:
        from articulation3d_amd import video

        own = video.jpeg_encode(torch.from_numpy(base).cuda(), 90)
        rows = video.jpeg_encode(torch.from_numpy(np.concatenate([base[:3]] * 4, 2)).cuda(), 90)
    return {"a_rows_480x2560": [rows[k % len(rows)] for k in range(n)], "a_frames_480x640": [own[k % len(own)] for k in range(n)],
            "b_pil_420_no_restart": pil_files(frames), "c_pil_420_restart_rows": pil_files(frames, restart_marker_rows=1),
            "d_pil_420_restart_1_mcu": pil_files(frames, restart_marker_blocks=1),
            "d_pil_420_restart_5_mcus": pil_files(frames, restart_marker_blocks=5)}


def time_gpu(jpegs, chunk, **how):
    from articulation3d_amd import video

    torch.cuda.synchronize()
    t = time.perf_counter()
    out = video.jpeg_decode(jpegs, chunk=chunk, **how)
    torch.cuda.synchronize()
    return len(jpegs) / (time.perf_counter() - t), out


def time_pil(jpegs):
    from PIL import Image

    torch.cuda.synchronize()
    t = time.perf_counter()
    host = np.stack([np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs])
    out = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return len(jpegs) / (time.perf_counter() - t), out


def kernel_times(jpegs, chunk, **how):
    """Device time per launch of the first a3d_jpeg_decode (or _split) call of a run, from torch.profiler: {kernel name: microseconds}."""
    from torch.profiler import ProfilerActivity, profile

    from articulation3d_amd import video

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        video.jpeg_decode(jpegs[:chunk], chunk=chunk, **how)
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        name = re.search(r"jpeg_decode_\w+_kernel|Memset", e.name)
        if name and e.device_time > 0:
            out.setdefault(name.group(0), []).append(round(e.device_time, 1))
    return out


def rounds(splits):
    """Per class the longest unit of the first file: its bytes and, per subsequence size, (subsequences, rounds) of the host model."""
    import jpeg_decode_ref
    import jpeg_split_ref

    for name, jpegs in classes(1, host_only=True).items():
        p = jpeg_decode_ref.parse(jpegs[0])
        scan = jpeg_split_ref.Scan(p)
        unit = jpeg_split_ref.Unit(max(scan.units, key=len))
        row = {"class": name, "units_per_frame": scan.n_units, "longest_unit_bytes": unit.n}
        for split in splits:
            n_rounds, subs = jpeg_split_ref.synchronise(scan, unit, split)
            row[f"split{split}"] = {"bytes": jpeg_split_ref.split_size(unit.n, split), "subsequences": len(subs), "rounds": n_rounds}
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", default=90, type=int)
    ap.add_argument("--repeats", default=3, type=int)
    ap.add_argument("--chunks", default="8,32")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--splits", default="32,64,128,256", help="subsequence sizes of the split path to sweep at the largest chunk")
    ap.add_argument("--rounds", action="store_true", help="no GPU: subsequences and rounds per class from the host model")
    args = ap.parse_args()
    splits = [int(v) for v in args.splits.split(",") if v]
    if args.rounds:
        return rounds(splits)
    from articulation3d_amd import opt_ops, video

    for name, jpegs in classes(args.frames).items():
        info = video.jpeg_parse(jpegs[0])
        ce, pe = opt_ops.jpeg_decode_scratch(*info.geometry)
        scan = sum(video.jpeg_parse(j).scan[1] - video.jpeg_parse(j).scan[0] for j in jpegs) / len(jpegs)
        rgb = info.height * info.width * 3
        time_pil(jpegs[:4]), time_gpu(jpegs[:4], 4)  # warm-up: the library, the allocator, PIL's tables
        pil = [time_pil(jpegs)[0] for _ in range(args.repeats)]
        want = time_pil(jpegs[:4])[1]
        row = {"class": name, "frames": len(jpegs), "size": [info.height, info.width], "units_per_frame": info.n_units,
               "file_bytes": round(sum(map(len, jpegs)) / len(jpegs)), "pil_fps": [round(v, 1) for v in pil],
               # per frame: uploaded scan bytes; memset + coefficient writes and reads (int16), planes written and read, RGB written
               "bytes_per_frame": {"h2d": round(scan), "coef_memset": 2 * ce, "coef_read": 2 * ce, "planes_write_read": 2 * pe, "rgb_write": rgb,
                                   "pil_path_h2d": rgb}}
        chunks = [int(c) for c in args.chunks.split(",")]
        for chunk in chunks:
            # an untimed call first: the scratch and the output of this chunk size come from the allocator's blocks afterwards
            assert torch.equal(time_gpu(jpegs, chunk)[1][:4], want), "the GPU decoder and PIL disagree"
            row[f"gpu_fps_chunk{chunk}"] = [round(time_gpu(jpegs, chunk)[0], 1) for _ in range(args.repeats)]
            if args.kernels:
                try:
                    row[f"gpu_kernel_us_chunk{chunk}"] = kernel_times(jpegs, chunk)
                except Exception as e:  # a profiler that is not there is not a failed measurement
                    row[f"gpu_kernel_us_chunk{chunk}"] = f"unavailable: {type(e).__name__}: {e}"
        for split in splits:  # the sweep the default subsequence size is taken from, at the largest chunk
            how = {"split_bytes": split}
            runs = [time_gpu(jpegs, max(chunks), **how) for _ in range(args.repeats)]
            assert torch.equal(runs[0][1][:4], want), f"the GPU decoder (split {split}) and PIL disagree"
            row[f"split{split}_fps_chunk{max(chunks)}"] = [round(r[0], 1) for r in runs]
            if args.kernels:
                try:
                    row[f"split{split}_kernel_us_chunk{max(chunks)}"] = kernel_times(jpegs, max(chunks), **how).get("jpeg_decode_split_kernel")
                except Exception as e:
                    row[f"split{split}_kernel_us_chunk{max(chunks)}"] = f"unavailable: {type(e).__name__}: {e}"
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
