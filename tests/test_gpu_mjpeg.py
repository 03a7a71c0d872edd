"""GPU suite: the Motion-JPEG kernels (a3d_jpeg_encode / a3d_jpeg_pack, csrc/jpeg.hip) against tests/mjpeg_ref.py, the law in numpy --
byte for byte, every frame of a call -- then the host path over them (jpeg_encode, render_clip_jpeg, MJPEGWriter) and one run of
tools/inference.py --vis avi.  Sizes are H x W."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mjpeg_ref as M
import render_ref as R
from test_mjpeg_host import PSNR_MARGIN_DB, decode, psnr_deficit, walk_avi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _encode(frames: np.ndarray, quality: int, **kw):
    from articulation3d_amd import video

    return video.jpeg_encode(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), quality, **kw)


def _segments(jpeg: bytes, H: int, W: int, quality: int):
    """The entropy-coded segments of a file of this package: stuffing leaves FF D0 .. FF D7 to the RST markers alone."""
    head = M.headers(H, W, quality)
    assert jpeg[:len(head)] == head and jpeg[-2:] == b"\xff\xd9"
    return re.split(b"\xff[\xd0-\xd7]", jpeg[len(head):-2])


def test_three_noise_frames_in_one_call_and_one_per_call():
    """77 x 45 at q 100: ragged edges in both directions, 10 segments (the RST counter wraps), dense codes, stuffing, per-frame offsets."""
    frames = np.stack([M.noise(77, 45, seed) for seed in (1, 2, 3)])
    want = [M.encode_frame(f, 100) for f in frames]
    assert len({len(w) for w in want}) == 3 and all(b"\xff\x00" in w for w in want)
    got = _encode(frames, 100)
    assert got == want
    assert [_encode(frames[i:i + 1], 100)[0] for i in range(3)] == want          # F does not matter
    assert _encode(frames, 100, chunk=2) == want                                   # nor does the chunking
    for g in got:
        assert decode(g, 77, 45).shape == (77, 45, 3)


@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (8, 8), (16, 24)])
def test_single_blocks_padding_only_and_exact_multiples(H, W):
    frames = np.stack([M.noise(H, W, 10 + H), M.structured(H, W)])
    assert _encode(frames, 50) == [M.encode_frame(f, 50) for f in frames]


def test_a_segment_of_four_tiles():
    """24 x 2056 noise at q 100: 257 MCUs = 771 blocks per segment.  The entropy kernel codes 256 blocks per tile (one per lane of its
    workgroup), so a segment is three full tiles and one of 3 blocks: the bit cursor and the unfinished byte are carried three times,
    and every tile's image exceeds one 1024-byte pass of the stuffing loop."""
    img = M.noise(24, 2056, 3)
    want = M.encode_frame(img, 100)
    assert (len(want) - 700) // 3 > 60000  # ~264 bytes per MCU
    assert _encode(img[None], 100)[0] == want


@pytest.mark.parametrize("quality", [1, 50, 90])
def test_structured_image_zero_runs(quality):
    """Gradients, a saturated rectangle, a one-pixel line: long zero runs, ZRL, EOB, a block without EOB (tests/test_mjpeg_host.py proves
    which symbols these cases reach)."""
    img = M.structured()
    assert _encode(img[None], quality)[0] == M.encode_frame(img, quality)


def test_largest_coefficients():
    """Black and white blocks in the sign patterns of DCT basis functions at q 100: AC category 10, the longest codes there are."""
    img = M.extreme()
    assert _encode(img[None], 100)[0] == M.encode_frame(img, 100)


@pytest.mark.parametrize("H,W", [(77, 45), (16, 48)])
def test_a_pitched_view_gives_the_bytes_of_a_contiguous_copy(H, W):
    """The frames are the right half of a wider device buffer.  77 x 45: the view starts off any boundary (byte loads); 16 x 48: it starts
    on an 8-byte boundary with an 8-byte row pitch (the vector loads, on rows that are not dense)."""
    from articulation3d_amd import video

    frames = np.stack([M.noise(H, W, 21), M.noise(H, W, 22)])
    wide = torch.full((2, H, 2 * W, 3), 0x5A, dtype=torch.uint8, device="cuda")
    wide[:, :, W:] = torch.from_numpy(frames).cuda()
    view = wide[:, :, W:]
    assert not view.is_contiguous()
    got = video.jpeg_encode(view, 90)
    assert got == video.jpeg_encode(view.contiguous(), 90) == [M.encode_frame(f, 90) for f in frames]
    with pytest.raises(ValueError):
        video.jpeg_encode(wide.transpose(1, 2), 90)  # not rows of pixels
    with pytest.raises(ValueError):
        video.jpeg_encode(wide.float(), 90)
    with pytest.raises(RuntimeError):
        video.jpeg_encode(view, 101)
    assert video.jpeg_encode(wide[:0], 90) == []


def test_one_rendered_row_at_the_panel_shape():
    """480 x 2560 at q 90, the shape --vis avi encodes: segments 0, 29 and 59 equal the law byte for byte (60 segments of 960 blocks);
    the whole frame decodes and meets the PSNR rule of tests/test_mjpeg_host.py against PIL's own encode."""
    row = M.rendered_row()
    jpeg = _encode(row[None], 90)[0]
    segs = _segments(jpeg, 480, 2560, 90)
    assert len(segs) == 60
    for r in (0, 29, 59):
        assert segs[r] == M.encode_segment(row, r, 90), r
    d = psnr_deficit(jpeg, row, 90)
    print(f"rendered row q 90: deficit {d:+.4f} dB")
    assert d <= PSNR_MARGIN_DB


def test_render_clip_jpeg_in_chunks_and_the_container(tmp_path):
    """3 frames, chunks of 2 (2 + 1 through the two staging buffers): every file is the law's encoding of render_clip's row for the same
    inputs, decodes to it within the PSNR rule, and an MJPEGWriter file of them passes the RIFF walker."""
    from articulation3d_amd import render, video

    H, W = 24, 40
    rng = np.random.default_rng(61)
    frames = M.smooth_frames(3, H, W)
    raw = [R.make_instances(rng, H, W, n) for n in (2, 0, 3)]
    opt = [R.make_instances(rng, H, W, n) for n in (1, 2, 2)]
    dframes = torch.from_numpy(frames).cuda()
    rows = np.concatenate([c.copy() for c in render.render_clip(dframes, raw, opt, chunk=2, mask_alpha=0.4)])
    chunks = list(video.render_clip_jpeg(dframes, raw, opt, quality=90, chunk=2, mask_alpha=0.4))
    assert [len(c) for c in chunks] == [2, 1]
    jpegs = [j for c in chunks for j in c]
    for row, jpeg in zip(rows, jpegs):
        assert jpeg == M.encode_frame(row, 90)
        d = psnr_deficit(jpeg, row, 90)
        print(f"render_clip_jpeg row: deficit {d:+.4f} dB")
        assert d <= PSNR_MARGIN_DB
    assert [j for c in video.render_clip_jpeg(dframes, raw, opt, quality=90, chunk=8, mask_alpha=0.4) for j in c] == jpegs
    with video.MJPEGWriter(tmp_path / "clip.avi", 4 * W, H, (30000, 1001)) as w:
        for j in jpegs:
            w.write(j)
    avi = walk_avi((tmp_path / "clip.avi").read_bytes())
    assert avi["frames"] == jpegs and (avi["total_frames"], avi["width"], avi["height"], avi["rate"], avi["scale"]) == (3, 4 * W, H, 30000, 1001)


def test_inference_script_writes_the_video(tmp_path):
    """tools/inference.py --vis avi with the flags of test_gpu_render's --vis npy run: output.avi holds one 480 x 2560 frame per input
    frame, and predictions.json is what the same run without the flag writes."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    outs = {}
    for name, extra in (("avi", ["--vis", "avi", "--vis-quality", "85", "--fps", "24"]), ("none", [])):
        outs[name] = tmp_path / name
        r = subprocess.run([sys.executable, "tools/inference.py", "--config", "configs/planercnn_inference.yaml", "--input", "synthetic:3", "--output",
                            str(outs[name]), "--random-init", "--calibrate-bn", "--conf-threshold", "0.3", "--batch", "2", *extra,
                            "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.3"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
    avi = walk_avi((outs["avi"] / "output.avi").read_bytes())
    assert (avi["total_frames"], avi["width"], avi["height"], avi["rate"], avi["scale"]) == (3, 2560, 480, 24, 1) and len(avi["frames"]) == 3
    head = M.headers(480, 2560, 85)
    for j in avi["frames"]:
        assert j[:len(head)] == head and decode(j, 480, 2560).shape == (480, 2560, 3)
    assert not (outs["none"] / "output.avi").exists()
    written = json.load(open(outs["avi"] / "predictions.json"))
    assert written == json.load(open(outs["none"] / "predictions.json")) and sum(len(p["instances"]) for p in written) > 0
