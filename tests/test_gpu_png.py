"""GPU suite: the PNG kernels (a3d_png_scan / a3d_png_emit / a3d_png_pack, csrc/png.hip) and articulation3d_amd/png.py against
tests/png_ref.py, the law in numpy -- byte for byte -- on the smallest shapes where the kernels can go wrong, and against PIL: every file
opens to exactly the input."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import png_ref as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _encode(frames: np.ndarray, **kw):
    from articulation3d_amd import png

    return png.png_encode(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), **kw)


def _open(data: bytes) -> np.ndarray:
    im = Image.open(io.BytesIO(data))
    assert im.mode == "RGB"
    return np.asarray(im)


def _content(H, W):
    """Black: one run of zeros through every type byte, so matches are cut at segment ends and continue from the segment before."""
    return np.stack([P.flat(H, W), P.flat(H, W, (0, 0, 0)), P.mixed(H, W), P.camera(H, W), P.noise(H, W, H + W)])


@pytest.mark.parametrize("H,W", [(1, 1), (2, 1), (1, 2), (3, 86), (40, 86), (9, 640), (5, 2731), (3, 5461)])
def test_bytes_of_the_law(H, W):
    """(1,1), (2,1), (1,2): the degenerate geometries.  (3,86): stride 259, a filter byte and a run of 258.  (40,86): two segments of 32
    and 8 rows, sources in the segment before, matches cut at the boundary.  (9,640): 5 rows per segment.  (5,2731): stride 8194, one
    row per segment, a distance with 12 extra bits.  (3,5461): the widest row, a segment of 16384 bytes.  Flat, black, mixed, camera-like
    and noise frames in one call: stored, fixed and dynamic segments."""
    frames = _content(H, W)
    stages = [P.encode_stages(f) for f in frames]
    want = [s["file"] for s in stages]
    if H * W > 2:  # what the shape is there for, as conditions on the law's own stages
        assert {k for s in stages for k in s["kinds"]} >= {0, 2}
        assert any(L == 258 for s in stages for toks in s["tokens"] for _i, L, _d in toks)
        assert any(d == 1 + 3 * W for s in stages for toks in s["tokens"] for _i, _L, d in toks)
    if (H, W) == (40, 86):
        assert {k for s in stages for k in s["kinds"]} == {0, 1, 2}
        assert any(i < d for s in stages for toks in s["tokens"][1:] for i, _L, d in toks)  # a source in the segment before
    got = _encode(frames)
    for g, w, f in zip(got, want, frames):
        assert g == w
        assert np.array_equal(_open(g), f)


def test_the_stages_of_a_scan():
    """(40,86) mixed content: the filtered bytes, the token words, the histogram and the Adler sums, each against the law."""
    from articulation3d_amd import opt_ops, png

    H, W = 40, 86
    frames = np.stack([P.mixed(H, W), P.flat(H, W)])
    enc = png._Encoder(2, H, W, torch.device("cuda"))
    enc.scan(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    stride, R, S, segs = P.geometry(H, W)
    assert (stride, R, S, P.slot_bytes(W)) == opt_ops.png_geometry(H, W)
    filt = enc.filt.cpu().numpy().reshape(2, -1)
    tok = enc.tok.cpu().numpy().view(np.uint16).reshape(2, -1)
    hist = enc.hist.cpu().numpy().reshape(2, -1)
    s1 = enc.s1.cpu().numpy().view(np.uint32).reshape(2, S)
    s2 = enc.s2.cpu().numpy().view(np.uint64).reshape(2, S)
    for f in range(2):
        st = P.encode_stages(frames[f])
        assert np.array_equal(filt[f], st["filt"])
        want = np.zeros(H * stride, np.uint16)
        for (a, _n), toks in zip(segs, st["tokens"]):
            for i, L, d in toks:
                want[a + i] = 1 if d == 0 else L | (1, 3, stride).index(d) << 9
        assert np.array_equal(tok[f], want)
        assert np.array_equal(hist[f], st["hist"])
        for s, (a, n) in enumerate(segs):
            b = st["filt"][a:a + n].astype(np.uint64)
            assert int(s1[f, s]) == int(b.sum()) and int(s2[f, s]) == int((b * np.arange(n, 0, -1, dtype=np.uint64)).sum())


def test_a_pitched_view_and_independence_of_the_call():
    """Three frames of different content as the right part of a wider device buffer: the bytes of a contiguous copy, of one frame per
    call and of any chunking."""
    from articulation3d_amd import png

    H, W = 40, 86
    frames = np.stack([P.camera(H, W), P.mixed(H, W), P.noise(H, W, 4)])
    wide = torch.full((3, H, W + 37, 3), 0x5A, dtype=torch.uint8, device="cuda")
    wide[:, :, 37:] = torch.from_numpy(frames).cuda()
    view = wide[:, :, 37:]
    assert not view.is_contiguous()
    want = [P.encode_frame(f) for f in frames]
    assert len({len(w) for w in want}) == 3
    assert png.png_encode(view) == want
    assert [_encode(frames[i:i + 1])[0] for i in range(3)] == want
    assert _encode(frames, chunk=2) == want and _encode(frames[::-1].copy(), chunk=1) == want[::-1]
    with pytest.raises(ValueError):
        png.png_encode(wide.transpose(1, 2))
    with pytest.raises(ValueError):
        png.png_encode(wide.float())
    assert png.png_encode(wide[:0]) == []


def test_the_width_cap():
    from articulation3d_amd import _lib, opt_ops, png

    assert _lib.lib().a3d_png_slot_bytes(5461) == 16400 and _lib.lib().a3d_png_slot_bytes(5462) == 0 and _lib.lib().a3d_png_slot_bytes(0) == 0
    with pytest.raises(ValueError):
        png.png_encode(torch.zeros((1, 1, 5462, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        opt_ops.png_geometry(65536, 4)


def test_a_small_destination_keeps_its_guard_bytes():
    """packed_bytes one short of the stream: the last segment is left out, everything in front of it is in place, nothing behind is
    touched."""
    from articulation3d_amd import opt_ops, png

    H, W = 40, 86
    frames = np.stack([P.mixed(H, W), P.camera(H, W)])
    enc = png._Encoder(2, H, W, torch.device("cuda"))
    enc.scan(torch.from_numpy(frames).cuda())
    enc.emit()
    torch.cuda.synchronize()
    seg_len, seg_off = enc.seg_len.cpu().numpy(), enc.seg_off.cpu().numpy()
    total = int(enc.frame_off[2])
    want = b"".join(P.encode_stages(f)["deflate"] for f in frames)
    assert total == len(want) and len(seg_len) == 4
    buf = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    opt_ops.png_pack_into(enc.slots, enc.seg_off, enc.seg_len, 2, H, W, buf[:total - 1])
    got = buf.cpu().numpy().tobytes()
    assert got[:seg_off[3]] == want[:seg_off[3]] and set(got[seg_off[3]:]) == {0xA5}
    opt_ops.png_pack_into(enc.slots, enc.seg_off, enc.seg_len, 2, H, W, buf[:total])
    got = buf.cpu().numpy().tobytes()
    assert got[:total] == want and set(got[total:]) == {0xA5}


def test_argument_refusals():
    """A3D_ERR_ARG (-1) before any launch: null pointers, H outside 1 .. 65535, W outside 1 .. 5461, pitch < W, int32 overflow."""
    from articulation3d_amd import _lib

    lib = _lib.lib()
    t = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p, s = t.data_ptr(), torch.cuda.current_stream().cuda_stream
    scan = lambda fr, F, H, W, pitch, out=p: lib.a3d_png_scan(fr, F, H, W, pitch, out, p, p, p, p, s)  # noqa: E731
    for bad in ((None, 1, 4, 4, 4), (p, 1, 4, 4, 4, None), (p, -1, 4, 4, 4), (p, 1, 0, 4, 4), (p, 1, 65536, 4, 4), (p, 1, 4, 0, 4), (p, 1, 4, 5462, 5462),
                (p, 1, 4, 4, 3), (p, 3, 65535, 5461, 5461)):
        assert scan(*bad) == -1, bad
    emit = lambda F, H, W, tab=p, fo=p: lib.a3d_png_emit(p, p, tab, F, H, W, p, p, p, fo, p, s)  # noqa: E731
    for bad in ((1, 4, 4, None), (1, 4, 4, p, None), (1, 0, 4), (1, 4, 5462), (3, 65535, 5461)):
        assert emit(*bad) == -1, bad
    pack = lambda F, H, W, n, dst=p: lib.a3d_png_pack(p, p, p, F, H, W, dst, n, s)  # noqa: E731
    for bad in ((1, 4, 4, -1), (1, 4, 4, 8, None), (1, 65536, 4, 8), (1, 4, 5462, 8), (3, 65535, 5461, 8)):
        assert pack(*bad) == -1, bad
    assert pack(0, 4, 4, 0, None) == 0
    torch.cuda.synchronize()


def test_render_clip_png_is_render_clip_exactly():
    """2 frames with hand-made detections, chunks of 1 (both staging buffers) and of 8: every file is the law's encoding of render_clip's
    row and opens to exactly that row."""
    import mjpeg_ref as M
    import render_ref as R
    from articulation3d_amd import png, render

    H, W = 24, 40
    rng = np.random.default_rng(62)
    frames = M.smooth_frames(2, H, W)
    raw = [R.make_instances(rng, H, W, n) for n in (2, 1)]
    opt = [R.make_instances(rng, H, W, n) for n in (1, 2)]
    dframes = torch.from_numpy(frames).cuda()
    rows = np.concatenate([c.copy() for c in render.render_clip(dframes, raw, opt, chunk=2, mask_alpha=0.4)])
    seconds = {}
    chunks = list(png.render_clip_png(dframes, raw, opt, chunk=1, mask_alpha=0.4, seconds=seconds))
    assert [len(c) for c in chunks] == [1, 1] and set(seconds) == {"huffman", "crc_and_files"}
    files = [f for c in chunks for f in c]
    for row, f in zip(rows, files):
        assert row.shape == (H, 4 * W, 3) and np.array_equal(_open(f), row)
        assert f == P.encode_frame(row)
    assert [f for c in png.render_clip_png(dframes, raw, opt, chunk=8, mask_alpha=0.4) for f in c] == files


def test_inference_script_writes_the_same_pixels_with_both_encoders(tmp_path):
    """tools/inference.py --vis png with --png-encoder gpu and pil: the same file names, files that decode identically, the GPU's ones
    one IDAT of this package's stream, and the same predictions."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    outs = {}
    for name in ("gpu", "pil"):
        outs[name] = tmp_path / name
        r = subprocess.run([sys.executable, "tools/inference.py", "--config", "configs/planercnn_inference.yaml", "--input", "synthetic:2", "--output",
                            str(outs[name]), "--random-init", "--calibrate-bn", "--conf-threshold", "0.3", "--batch", "2", "--vis", "png",
                            "--png-encoder", name, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.3"], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(outs["gpu"] / "vis"))
    assert names == sorted(os.listdir(outs["pil"] / "vis")) == ["frame_00000.png", "frame_00001.png"]
    for n in names:
        g = (outs["gpu"] / "vis" / n).read_bytes()
        a, b = _open(g), _open((outs["pil"] / "vis" / n).read_bytes())
        assert a.shape == (480, 2560, 3) and np.array_equal(a, b)
        kinds = [c[0] for c in P.chunks(g)]
        assert kinds == [b"IHDR", b"IDAT", b"IEND"] and all(c[2] for c in P.chunks(g)) and P.chunks(g)[1][1][:2] == b"\x78\x01"
    assert json.load(open(outs["gpu"] / "predictions.json")) == json.load(open(outs["pil"] / "predictions.json"))
