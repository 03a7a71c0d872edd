#!/usr/bin/env python3
"""The reference's tools/inference.py on this package: per-clip articulation prediction.

    python tools/inference.py --config configs/planercnn_inference.yaml --input <frames> --output out/ [--conf-threshold 0.7]

Same stages as the reference script (tools/inference.py:171-250): build the model from the YAML, detect every frame,
build the `create_instances` records, `track_planes`, `optimize_planes(preds, planes, '3dc')` -- but the frame loop is the
batched, frame-sharded `pipeline.detect_clip` (one RCCL all-gather per clip when launched with torchrun) and the
optimiser's sweeps run on the GPU.  `random.seed(2020)` / `np.random.seed(2020)` as in the reference (:172-173).

Input (this image has no H.264 decoder: cv2 / imageio are absent, so .mp4 / .mov are refused with a clear message):
  * a .npy / .npz file with uint8 frames [F,H,W,3] in RGB order (what imageio would hand over), or
  * a Motion-JPEG .avi (what `--vis avi` writes, and what cameras and ffmpeg -c:v mjpeg write): the frames are baseline JPEG, decoded
    on the GPU (articulation3d_amd/video.py: MJPEGReader + jpeg_decode) to the bytes PIL's libjpeg gives; `--fps` defaults to the
    container's rate, or
  * a directory of .png / .jpg frames, sorted by name: baseline JPEG files of one size go through the same GPU decoder, 8-bit grey,
    grey + alpha, RGB and RGBA PNG files of one size through the GPU PNG decoder (articulation3d_amd/png.py: png_decode -- inflate,
    Adler-32, unfiltering and the conversion in HIP), everything else (palette, 16-bit, interlaced, progressive or otherwise refused
    files, frames a decoder flags) through PIL -- `--decoder auto|gpu|pil`, the frames are the same bytes under all three: `gpu`
    sends every stream a decoder accepts to the GPU, `pil` none; `auto` sends every baseline JPEG stream, with restart intervals or
    without (a scan without them is split among many lanes that synchronise themselves), and keeps PNG on PIL: one wave inflates one
    frame, and at 8 - 90 frames per call that is slower than PIL on one host thread (MEASUREMENTS.md, "PNG decode"), or
  * `synthetic:N` / `synthetic:NxHxW` -- N seeded random frames (plumbing check), optionally at a source size H x W.
The frames go to the GPU as they come from the reader (uint8 RGB, any size): the reference's `cv2.resize(im, (640, 480))` and
BGR flip (:216-218) run on the device, fused with the normalisation in front of the stem (a3d_preprocess_resize_u8).
Output: <output>/predictions.json -- per frame the optimised detections (bbox xyxy, score, class, plane, rotation /
translation axis, RLE mask) and <output>/tracks.json (tracked planes, has_rot, consensus axis).
`--vis png|npy|avi` also writes the reference's 2-D visualisation, the four panels per frame of its output.mp4
(`[opt seg | opt normal | raw seg | raw normal]`, [480, 2560, 3] uint8 RGB), rendered on the GPU (articulation3d_amd/render.py):
<output>/vis/frame_%05d.png, one <output>/vis.npy, or the video <output>/output.avi.  The video is Motion-JPEG in an AVI container,
not the reference's H.264 .mp4: every frame is a baseline JPEG (4:4:4, `--vis-quality`), encoded on the GPU
(articulation3d_amd/video.py), played at `--fps` (a .npy or an image directory carries no frame rate; the reference takes its reader's).
The .png files are lossless either way: `--png-encoder gpu` filters, matches and Huffman-codes the rows on the GPU
(articulation3d_amd/png.py) and only compressed bytes come to the host, `pil` brings the rows to the host for PIL's zlib, `auto` (the
default) takes the faster one, the GPU; the two write different bytes that decode to the same pixels.
`--save-obj` writes the reference's 3-D model (its save_obj_model, :44-168) for the frames of `--obj-frames`:
<output>/frame_%04d/arti_pred.obj + .mtl + uv_maps/*.png -- the most confident articulated plane in its opened poses, two axis
markers and the background, as dense meshes built on the GPU (articulation3d_amd/mesh.py states the departures).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def count_frames(path: str) -> int:
    """Number of frames of a clip without decoding it (npy header / directory listing)."""
    if path.startswith("synthetic:"):
        return int(path.split(":")[1].split("x")[0])
    if path.endswith(".npy"):
        return int(np.load(path, mmap_mode="r").shape[0])
    if path.endswith(".npz"):
        z = np.load(path)
        return int(z[list(z.keys())[0]].shape[0])
    if os.path.isdir(path):
        return len([n for n in os.listdir(path) if n.lower().endswith((".png", ".jpg", ".jpeg"))])
    if path.lower().endswith(".avi"):
        from articulation3d_amd.video import MJPEGReader

        with MJPEGReader(path) as reader:
            return len(reader)
    return 1


def gpu_decodes(info, decoder: str) -> bool:
    """Whether a stream that jpeg_parse accepts goes to the GPU.  `gpu`: always.  `auto`: the classes that MEASUREMENTS.md ("JPEG decode")
    found faster there than PIL on one host thread -- since the entropy launch that splits a unit among many lanes, every class:
    streams with restart intervals, and scans without them (nine times PIL's rate at 32 frames per call)."""
    return decoder in ("gpu", "auto")


PNG_AUTO_ON_GPU = False  # MEASUREMENTS.md, "PNG decode": the GPU path was not faster than PIL in every repetition of every class


def gpu_decodes_png(info, decoder: str) -> bool:
    """Whether a file that png_parse accepts goes to the GPU.  `pil`: never.  `gpu`: always.  `auto`: only where tools/png_decode_bench.py
    found the GPU path faster than PIL in every repetition of every class of file (PNG_AUTO_ON_GPU; it did not: MEASUREMENTS.md, "PNG
    decode"), and only on a machine with a GPU."""
    if decoder == "gpu":
        return True
    return decoder == "auto" and PNG_AUTO_ON_GPU and torch.cuda.is_available()


def _decode_pngs(blobs, frames, decoder: str) -> None:
    """The PNG half of decode_images: the files png_parse accepts that share the first one's geometry, in one png_decode call."""
    from articulation3d_amd.png import SIGNATURE, png_decode, png_parse

    chosen, geometry = [], None
    for k, blob in enumerate(blobs):
        if blob[:8] != SIGNATURE:
            continue
        try:
            info = png_parse(blob)
        except ValueError:
            continue
        if gpu_decodes_png(info, decoder) and geometry in (None, info.geometry):
            geometry = info.geometry
            chosen.append(k)
    if chosen:
        out, status = png_decode([blobs[k] for k in chosen], strict=False)
        out = out.cpu().numpy()
        for i, k in enumerate(chosen):
            if int(status[i]) == 0:
                frames[k] = out[i]


def decode_images(blobs, decoder: str = "auto") -> np.ndarray:
    """Encoded images (the bytes of .jpg / .png files or of an AVI's chunks) -> uint8 [n,H,W,3] RGB.  Baseline JPEG streams that share the
    size and sampling of the first such stream are decoded on the GPU in one jpeg_decode call, PNG files that share the first one's
    geometry in one png_decode call (gpu_decodes / gpu_decodes_png say which), the rest by PIL -- as is every frame a GPU decoder
    flags (a damaged or out-of-domain stream), so the result is PIL's under every setting of `decoder`."""
    import io

    from PIL import Image

    frames = [None] * len(blobs)
    if decoder != "pil":
        _decode_pngs(blobs, frames, decoder)
        from articulation3d_amd.video import jpeg_decode, jpeg_parse

        chosen, geometry = [], None
        for k, blob in enumerate(blobs):
            if blob[:2] != b"\xff\xd8":
                continue
            try:
                info = jpeg_parse(blob)
            except ValueError:
                continue
            if gpu_decodes(info, decoder) and geometry in (None, info.geometry):
                geometry = info.geometry
                chosen.append(k)
        if chosen:
            out, status = jpeg_decode([blobs[k] for k in chosen], chunk=32, strict=False)
            out = out.cpu().numpy()
            for i, k in enumerate(chosen):
                if int(status[i]) == 0:
                    frames[k] = out[i]
    for k, blob in enumerate(blobs):
        if frames[k] is None:
            frames[k] = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))
    return np.stack(frames)


def read_frames(path: str, lo: int = 0, hi: int = None, decoder: str = "auto") -> np.ndarray:
    """-> uint8 [hi-lo,Hs,Ws,3] RGB at the SOURCE size (no host-side resize): frames lo .. hi-1 of the clip (default: all).  Under
    torchrun every rank reads only its own block (memory-mapped .npy, the AVI's index, per-file image decode).  `decoder`: who decodes
    JPEG streams (decode_images)."""
    from PIL import Image

    sl = slice(lo, hi)

    if path.startswith("synthetic:"):
        from articulation3d_amd.utils.synthetic import synthetic_frames

        spec = path.split(":")[1].split("x")
        n, h, w = int(spec[0]), (int(spec[1]) if len(spec) == 3 else 480), (int(spec[2]) if len(spec) == 3 else 640)
        return synthetic_frames(n, h=h, w=w)[sl][..., ::-1].copy()  # generated BGR -> RGB, flipped back on the device
    if path.endswith((".mp4", ".mov")):
        raise SystemExit("no video decoder in this environment (cv2 / imageio absent): pass a .npy of RGB frames or a directory of images")
    if path.lower().endswith(".avi"):
        from articulation3d_amd.video import MJPEGReader

        try:
            with MJPEGReader(path) as reader:
                blobs, size = reader[sl], (reader.height, reader.width)
        except ValueError as e:
            raise SystemExit(f"{path}: {e} (only Motion-JPEG .avi files are read)")
        return decode_images(blobs, decoder) if blobs else np.zeros((0, *size, 3), np.uint8)
    if path.endswith(".npy"):
        frames = np.load(path, mmap_mode="r")[sl]
    elif path.endswith(".npz"):
        z = np.load(path)
        frames = z[list(z.keys())[0]][sl]
    elif os.path.isdir(path):
        every = sorted(n for n in os.listdir(path) if n.lower().endswith((".png", ".jpg", ".jpeg")))
        names = every[sl]
        if names:
            blobs = []
            for n in names:
                with open(os.path.join(path, n), "rb") as f:
                    blobs.append(f.read())
            frames = decode_images(blobs, decoder)
        else:  # an empty block (trailing ranks when F <= ceil(F / world) * (world - 1)): zero frames at the clip's size
            if not every:
                raise SystemExit(f"{path}: no .png / .jpg frames")
            w, h = Image.open(os.path.join(path, every[0])).size
            frames = np.zeros((0, h, w, 3), np.uint8)
    else:
        frames = np.asarray(Image.open(path).convert("RGB"))[None]
    assert frames.ndim == 4 and frames.shape[3] == 3 and frames.dtype == np.uint8, "frames must be uint8 [F,H,W,3]"
    return np.ascontiguousarray(frames)


def snapshot_predictions(preds):
    """The raw predictions as they are before the optimiser, for the visualisation's raw panels.  optimize_planes re-weights the
    scores on copies and clones pred_rot_axis / pred_planes before it writes a track's consensus into them, but a translation
    track's consensus axis is written into pred_tran_axis in place: the small per-detection fields are copied here, boxes and
    masks (never written) are shared."""
    from articulation3d_amd.structures import Instances

    out = []
    for p in preds:
        q = Instances(p.image_size)
        for f in ("scores", "pred_planes", "pred_rot_axis", "pred_tran_axis", "pred_classes"):
            v = getattr(p, f)
            setattr(q, f, v.clone() if isinstance(v, torch.Tensor) else np.copy(v))
        q.pred_boxes, q.pred_masks = p.pred_boxes, p.pred_masks
        out.append(q)
    return out


PNG_AUTO_GPU = True  # MEASUREMENTS.md, "PNG encode": render_clip_png against render_clip + PIL, end to end


def png_on_gpu(choice: str, device, width: int) -> bool:
    """Whether `--vis png` rows of `width` pixels are encoded on the GPU (articulation3d_amd/png.py).  `gpu`: always (a row the encoder
    refuses is an error); `pil`: never; `auto`: on a CUDA device, for rows the encoder takes, if it was measured faster end to end."""
    from articulation3d_amd.png import MAX_W

    if choice == "auto":
        return PNG_AUTO_GPU and torch.device(device).type == "cuda" and width <= MAX_W
    return choice == "gpu"


def write_visualisation(args, device, frames_rgb, raw_preds, opt_preds, chunk: int = 32):
    """--vis: resize the clip's frames on the device in chunks of `chunk` source frames (the detector's own front end, uint8
    output, 0.9 MB per resized frame kept on the device), then ONE render_clip over the whole clip: its buffers are pinned and
    allocated once, and the four-panel rows are written as they come off the copy pipeline.  render_clip works in chunks of 8
    frames: 3.7 MB per row, so 88 MB of pinned memory in its three host buffers.  `--vis avi` goes through render_clip_jpeg instead:
    the rows are encoded on the device and only the JPEG bytes come to the host, straight into <output>/output.avi."""
    from articulation3d_amd import ops
    from articulation3d_amd.render import render_clip

    n = len(frames_rgb)
    u8 = torch.empty((n, 480, 640, 3), dtype=torch.uint8, device=device)
    for lo in range(0, n, chunk):
        src = torch.from_numpy(np.ascontiguousarray(frames_rgb[lo:lo + chunk])).to(device)
        u8[lo:lo + chunk] = ops.preprocess_resize_u8(src, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), want_u8=True)[1]  # resized, still RGB
    if args.vis == "png":
        from PIL import Image

        os.makedirs(os.path.join(args.output, "vis"), exist_ok=True)
        if png_on_gpu(args.png_encoder, device, 4 * 640):
            from articulation3d_amd.png import render_clip_png

            at = 0
            for pngs in render_clip_png(u8, raw_preds, opt_preds, chunk=8, mask_alpha=args.mask_alpha, conf_threshold=args.conf_threshold):
                for png in pngs:
                    with open(os.path.join(args.output, "vis", "frame_%05d.png" % at), "wb") as f:
                        f.write(png)
                    at += 1
            return
    elif args.vis == "npy":
        whole = np.lib.format.open_memmap(os.path.join(args.output, "vis.npy"), mode="w+", dtype=np.uint8, shape=(n, 480, 4 * 640, 3))
    if args.vis == "avi":
        from articulation3d_amd.video import MJPEGWriter, render_clip_jpeg

        with MJPEGWriter(os.path.join(args.output, "output.avi"), 4 * 640, 480, args.fps) as video:
            for jpegs in render_clip_jpeg(u8, raw_preds, opt_preds, quality=args.vis_quality, chunk=8, mask_alpha=args.mask_alpha,
                                          conf_threshold=args.conf_threshold):
                for jpeg in jpegs:
                    video.write(jpeg)
        return
    at = 0
    for rows in render_clip(u8, raw_preds, opt_preds, chunk=8, mask_alpha=args.mask_alpha, conf_threshold=args.conf_threshold):
        if args.vis == "png":
            for k, row in enumerate(rows):
                Image.fromarray(row).save(os.path.join(args.output, "vis", "frame_%05d.png" % (at + k)))
        else:
            whole[at:at + len(rows)] = rows
        at += len(rows)
    if args.vis == "npy":
        whole.flush()


def write_obj_models(args, device, frames_rgb, opt_preds):
    """--save-obj: one articulated model per requested frame (indices past the clip are dropped, as are frames without a usable
    detection -- each with a line on stdout).  The frames are resized on the device as write_visualisation resizes them."""
    from articulation3d_amd import ops
    from articulation3d_amd.mesh import articulated_model, save_obj

    wanted = [i for i in args.obj_frames if 0 <= i < len(opt_preds)]
    written = 0
    if wanted:
        src = torch.from_numpy(np.ascontiguousarray(frames_rgb[wanted])).to(device)
        u8 = ops.preprocess_resize_u8(src, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), want_u8=True)[1].cpu().numpy()  # resized, still RGB
    for k, i in enumerate(wanted):
        model = articulated_model(opt_preds[i], u8[k], axis_dir=args.axis_dir, stride=args.obj_stride, bkgd_stride=args.obj_bkgd_stride,
                                  webvis=args.webvis, device=device)
        if model is None:
            print(f"save-obj: frame {i} has no articulated plane to export")
            continue
        folder = os.path.join(args.output, "frame_%04d" % i)
        os.makedirs(folder, exist_ok=True)
        save_obj(folder, "arti_pred", model)
        written += 1
    print(f"save-obj: {written} of {len(wanted)} requested frames exported" if written else "save-obj: no model exported (no frame with a detection)")


def _frame_list(text: str):
    return [int(v) for v in text.split(",") if v.strip()]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Articulation prediction on a clip (MI355X).")
    ap.add_argument("--config", required=True)
    ap.add_argument("--input", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--conf-threshold", default=0.7, type=float)
    ap.add_argument("--batch", default=32, type=int, help="frames per detector batch per GPU")
    ap.add_argument("--calibrate-bn", action="store_true", help="random-init weights only: estimate batch-norm statistics on the clip")
    ap.add_argument("--random-init", action="store_true",
                    help="do NOT load cfg.MODEL.WEIGHTS: explicit random initialisation (plumbing runs; a missing checkpoint is otherwise an error)")
    ap.add_argument("--dist-backend", default="nccl", help="torchrun only: nccl (= RCCL over xGMI) or gloo")
    ap.add_argument("--no-precision-audit", action="store_true",
                    help="skip the load-time audit of the default arithmetic (PlaneRCNN.audit_precision: every fp16x2 layer checked against its "
                         "bf16x3 evaluation on the clip's first frames; layers that leave the format's window are pinned to bf16x3)")
    ap.add_argument("--vis", choices=("none", "png", "npy", "avi"), default="none",
                    help="write the reference's four-panel visualisation row per frame (opt seg | opt normal | raw seg | raw normal), rendered on "
                         "the GPU: png = <output>/vis/frame_%%05d.png, npy = one <output>/vis.npy [F,480,2560,3], avi = the video "
                         "<output>/output.avi, Motion-JPEG (baseline JPEG frames encoded on the GPU) in an AVI container -- not the reference's "
                         "H.264 .mp4, which needs an encoder this package does not have")
    ap.add_argument("--vis-quality", default=90, type=int, help="--vis avi: JPEG quality, 1 .. 100")
    ap.add_argument("--fps", default=None,
                    help="--vis avi: frames per second, an integer or a ratio such as 30000/1001 (default: the rate of an .avi input, else 30)")
    ap.add_argument("--decoder", choices=("auto", "gpu", "pil"), default="auto",
                    help="who decodes JPEG and PNG input (.avi chunks, .jpg and .png files): gpu = every baseline JPEG stream and every 8-bit "
                         "non-interlaced grey / RGB (with or without alpha) PNG on the GPU, pil = PIL on the host, auto = the GPU for the streams it was "
                         "measured to decode faster (every baseline JPEG stream; PNG stays on PIL: MEASUREMENTS.md, 'PNG decode'); the frames are the same bytes")
    ap.add_argument("--png-encoder", choices=("auto", "gpu", "pil"), default="auto",
                    help="who writes the --vis png files: gpu = filtering, LZ77 and Huffman coding on the GPU, only compressed bytes come to the "
                         "host; pil = the rows come to the host and PIL's zlib compresses them; auto = the GPU where it was measured faster "
                         "(MEASUREMENTS.md, 'PNG encode').  The files differ in bytes and decode to the same pixels")
    ap.add_argument("--mask-alpha", default=0.0, type=float,
                    help="--vis: opacity of the instance masks on the seg panels (0 = none, as the reference draws them)")
    ap.add_argument("--save-obj", action="store_true",
                    help="write <output>/frame_%%04d/arti_pred.obj (+ .mtl, uv_maps/*.png) for the frames of --obj-frames: the most confident "
                         "articulated plane in its opened poses, axis markers and background, meshes built on the GPU")
    ap.add_argument("--obj-frames", default=[0, 30, 60, 89], type=_frame_list, help="--save-obj: comma list of frame indices (past the clip: dropped)")
    ap.add_argument("--webvis", action="store_true", help="--save-obj: flip y and z for web model viewers")
    ap.add_argument("--axis-dir", choices=("l", "r"), default="l", help="--save-obj: the side the plane opens to")
    ap.add_argument("--obj-stride", default=2, type=int, help="--save-obj: pixel lattice of the object's mesh")
    ap.add_argument("--obj-bkgd-stride", default=8, type=int, help="--save-obj: pixel lattice of the background's mesh")
    ap.add_argument("opts", nargs=argparse.REMAINDER, default=[], help="KEY VALUE config overrides, e.g. MODEL.DEVICE cuda:0")
    return ap


def main():
    random.seed(2020)
    np.random.seed(2020)
    args = build_parser().parse_args()
    if args.fps is None:
        args.fps = "30"
        if args.input.lower().endswith(".avi") and os.path.isfile(args.input):
            from articulation3d_amd.video import MJPEGReader

            with MJPEGReader(args.input) as reader:
                args.fps = str(reader.fps)

    # one process per GPU under torchrun (frames sharded by pipeline.detect_clip, ONE all-gather of the records per clip):
    # rank / device / process group are set up before anything touches the GPU; rank 0 alone tracks, optimises and writes
    world, rank, local_rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    if rank == 0:
        os.makedirs(args.output, exist_ok=True)

    from articulation3d_amd.config import get_cfg, get_planercnn_cfg_defaults
    from articulation3d_amd.pipeline import detect_clip
    from articulation3d_amd.utils import rle
    from articulation3d_amd.utils.arti_vis import PlaneRCNN_Branch
    from articulation3d_amd.utils.opt_utils import optimize_planes, track_planes

    cfg = get_cfg()
    get_planercnn_cfg_defaults(cfg)
    cfg.merge_from_file(args.config)
    if args.opts:
        cfg.merge_from_list(args.opts)
    if not str(cfg.MODEL.DEVICE).startswith("cuda"):
        raise SystemExit(f"MODEL.DEVICE={cfg.MODEL.DEVICE!r}: this package is the MI355X (HIP) implementation of the detection path and has "
                         "no CPU fallback; the CPU statement of the same graph lives in oracle/ as the test checker")
    if world > 1:
        import torch.distributed as dist

        n_dev = torch.cuda.device_count()  # (does not initialise HIP)
        cfg.MODEL.DEVICE = f"cuda:{local_rank % max(n_dev, 1)}"
        torch.cuda.set_device(local_rank % max(n_dev, 1))
        from articulation3d_amd.streams import side

        side(0)  # the package's side streams take their hardware queues now, in front of the collective library's (articulation3d_amd/streams.py)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dist_backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device(cfg.MODEL.DEVICE))
        else:
            dist.init_process_group(backend=args.dist_backend)
    if args.random_init:
        torch.manual_seed(2020)  # every rank (and every run) draws the same initialisation
    branch = PlaneRCNN_Branch(cfg, load_weights=not args.random_init)
    model = branch.predictor.model
    from articulation3d_amd.parallel import shard_range

    n_frames = count_frames(args.input)
    lo, hi = shard_range(n_frames, rank, world)
    frames_rgb = read_frames(args.input, lo, hi, args.decoder)  # this rank's block only (rank 0 reads the rest later, for the optimiser)
    if args.calibrate_bn:
        # the statistics come from the FIRST two frames of the clip on EVERY rank (rank 0's own block may hold only one of them)
        n_head = min(2, n_frames)
        frames_rgb_head = frames_rgb[:n_head] if lo == 0 and hi - lo >= n_head else read_frames(args.input, 0, n_head, args.decoder)
        from articulation3d_amd import ops
        from articulation3d_amd.utils.synthetic import calibrate_batchnorm

        _x4, head = ops.preprocess_resize_u8(torch.from_numpy(np.ascontiguousarray(frames_rgb_head)).to(model.device), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), want_u8=True)
        calibrate_batchnorm(model, head.flip(-1).contiguous())  # resized RGB -> BGR uint8
    if not args.no_precision_audit:
        # once per loaded checkpoint, on the FIRST two frames of the clip on every rank (every rank must pin the same layers: a frame's
        # result may not depend on the rank that detects it)
        n_head = min(2, n_frames)
        head_rgb = frames_rgb[:n_head] if lo == 0 and hi - lo >= n_head else read_frames(args.input, 0, n_head, args.decoder)
        audit = model.audit_precision(torch.from_numpy(np.ascontiguousarray(head_rgb)).to(model.device), source_rgb=True)
        if rank == 0:
            worst = max((r["max_ratio"] for r in audit.rows), default=0.0)
            print(f"precision audit: {len(audit.rows)} fp16x2 layer launches checked against bf16x3 on {n_head} frame(s), worst err / bound {worst:.3f}; "
                  f"pinned to bf16x3: {model.pinned_layers() or 'none'}")
    preds = detect_clip(model, frames_rgb, batch=args.batch, conf_threshold=args.conf_threshold, source_rgb=True, num_frames=n_frames)
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
        if rank != 0:  # every rank holds the gathered detections; the temporal stage and the files are rank 0's
            return
        frames_rgb = read_frames(args.input, decoder=args.decoder)  # the optimiser's sweeps look at the whole clip
    planes = track_planes(preds)
    raw_preds = snapshot_predictions(preds) if args.vis != "none" else None
    opt_preds = optimize_planes(preds, planes, "3dc", frames=frames_rgb)

    out = []
    for i, p in enumerate(opt_preds):
        n = len(p.pred_boxes)
        out.append({"frame": i, "instances": [{
            "bbox": [float(v) for v in p.pred_boxes.tensor[k]], "score": float(p.scores[k]), "category_id": int(p.pred_classes[k]),
            "pred_plane": [float(v) for v in p.pred_planes[k]], "pred_rot_axis": [float(v) for v in p.pred_rot_axis[k]],
            "pred_tran_axis": [float(v) for v in p.pred_tran_axis[k]],
            "segmentation": rle.encode(np.asfortranarray(p.pred_masks[k].numpy().astype(np.uint8)))} for k in range(n)]})
    with open(os.path.join(args.output, "predictions.json"), "w") as f:
        json.dump(out, f)
    tracks = {cat: [{"frames": sorted(t["ids"]), "has_motion": bool(t.get("has_rot", False)),
                     "consensus_axis": (np.asarray(t["std_axis"]).tolist() if "std_axis" in t else None)} for t in ts]
              for cat, ts in planes.items()}
    with open(os.path.join(args.output, "tracks.json"), "w") as f:
        json.dump(tracks, f)
    if args.vis != "none":
        write_visualisation(args, model.device, frames_rgb, raw_preds, opt_preds)
    if args.save_obj:
        write_obj_models(args, model.device, frames_rgb, opt_preds)
    kept = sum(len(p.pred_boxes) for p in opt_preds)
    print(f"{len(frames_rgb)} frames, {kept} detections above {args.conf_threshold}, "
          f"{len(planes['rot'])} rotation / {len(planes['trans'])} translation tracks -> {args.output}")


if __name__ == "__main__":
    main()
