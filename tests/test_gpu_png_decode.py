"""GPU suite: the PNG decode kernels (a3d_png_decode, csrc/png_decode.hip) against tests/png_decode_ref.py, the law in numpy -- byte for
byte with the status equal, every frame of a call -- then the host path over them (png.png_decode) and tools/inference.py reading a
directory.  The streams are those of tests/test_png_decode_host.py (tests/png_decode_streams.py).  Sizes are H x W."""
import ctypes as C
import importlib.util
import io
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import png_decode_ref as R
import png_decode_streams as S
import png_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 7), (5, 1), (17, 33), (64, 9), (65, 9), (130, 40), (70, 200)]
_REF = {}


def ref(data: bytes):
    """(pixels, status) of the law, computed once per file."""
    if data not in _REF:
        _REF[data] = R.decode(data)
    return _REF[data]


def gpu(pngs, **kw):
    from articulation3d_amd import png

    frames, status = png.png_decode(pngs, strict=False, **kw)
    return frames.cpu().numpy(), status.tolist()


def check(pngs, **kw):
    """Every frame of one call: the law's status, and the law's pixels where the law has any (status 0)."""
    frames, status = gpu(pngs, **kw)
    for k, data in enumerate(pngs):
        want, st = ref(data)
        assert status[k] == st, (k, status[k], st)
        if st == 0:
            assert np.array_equal(frames[k], want), k
    return frames, status


@pytest.mark.parametrize("ch", (1, 2, 3, 4))
@pytest.mark.parametrize("H,W", SIZES)
def test_sizes_and_channels(H, W, ch):
    """One pixel, one row, one column, ragged sizes, the band edge of the wavefront (64 and 65 rows), three bands, and 70 x 200 whose
    raw bytes pass the 32 768-byte window: PIL's file and hand-filtered rows with a random type per row, in one call."""
    img = S.image(H, W, ch, seed=H + W)
    frames, status = check([S.pil_png(img), S.hand_built(H, W, ch, seed=H + W)["mixed"][1], S.pil_png(S.image(H, W, ch, kind="noise"), compress_level=1)])
    assert status == [0, 0, 0] and np.array_equal(frames[0], R.to_rgb(img))


@pytest.mark.parametrize("ch", (1, 2, 3, 4))
@pytest.mark.parametrize("H,W", [(17, 33), (65, 9), (130, 40)])
def test_each_filter_type_alone_and_mixed(H, W, ch):
    built = S.hand_built(H, W, ch, seed=ch)
    frames, status = check([data for _img, data in built.values()])
    assert status == [0] * 6
    for k, (img, _data) in enumerate(built.values()):
        assert np.array_equal(frames[k], R.to_rgb(img))


@pytest.mark.parametrize("ch", (1, 2, 3, 4))
def test_pil_and_zlib_settings(ch):
    """PIL's writer at every level, zlib.compressobj at every window size and strategy, flushed in the middle, and stored."""
    H, W = 17, 33
    img = S.image(H, W, ch, seed=20 + ch)
    raw = S.filter_rows(img, np.arange(H) % 5)
    pngs = [S.pil_png(img, compress_level=l) for l in (0, 1, 6, 9)] + [S.pil_png(img, optimize=True)]
    pngs += [S.png_of_raw(H, W, ch, raw, d) for d in S.zlib_settings(raw).values()]
    frames, status = check(pngs)
    assert status == [0] * len(pngs) and all(np.array_equal(f, R.to_rgb(img)) for f in frames)


def test_own_files_and_large_zlib_streams():
    """The package's own encoder, and zlib streams of 70 x 200 frames: several blocks, distances past the LDS ring's first lap."""
    for img in (png_ref.mixed(40, 50), png_ref.camera(65, 9)):
        frames, status = check([png_ref.encode_frame(img)])
        assert status == [0] and np.array_equal(frames[0], img)
    H, W = 70, 200
    img = png_ref.mixed(H, W)
    raw = S.filter_rows(img, np.arange(H) % 5)
    pngs = [S.png_of_raw(H, W, 3, raw, S.zlib_deflate(raw, level=l, flush_at=cut)) for l, cut in ((9, ()), (1, (20000,)), (0, ()))]
    frames, status = check(pngs)
    assert status == [0, 0, 0] and all(np.array_equal(f, img) for f in frames)


@pytest.mark.parametrize("name", sorted(S.special_streams()))
def test_token_list_streams(name):
    """What zlib never emits: 258 bytes from exactly 32 768 back, distance 1 and other overlapping copies, empty and full stored blocks,
    one distance code and none, 15-bit codes, a repeat across the two sets of lengths."""
    H, W, ch, data = S.special_streams()[name]
    frames, status = check([data])
    assert status == [0] and np.array_equal(frames[0], S.pil_rgb(data))


def flagged_streams():
    """name -> (PNG file of 5 x 4 RGB, the status the law gives it): one per code."""
    H, W, ch = 5, 4, 3
    img = S.image(H, W, ch, seed=9)
    raw = S.filter_rows(img, [0, 1, 2, 3, 4])
    good = S.zlib_deflate(raw, strategy=zlib.Z_FIXED)
    adler = struct.pack(">I", zlib.adler32(raw))
    far = S.Bits()
    far.put(1, 1)
    far.put(1, 2)
    S.put_tokens(far, [0, 7, (3, 5)], *png_ref.fixed_lengths())
    bad_filter = bytearray(raw)
    bad_filter[2 * (1 + W * ch)] = 7
    big = S.filter_rows(S.image(H + 1, W, ch, seed=9), [0] * (H + 1))
    bodies = {
        "short": (good[:len(good) // 2], R.SHORT),
        "no_trailer": (good + adler[:3], R.SHORT),
        "bad_code": (b"\x07" + good, R.BAD_CODE),
        "far": (far.tobytes() + adler, R.FAR),
        "long": (S.zlib_deflate(big) + struct.pack(">I", zlib.adler32(big)), R.LONG),
        "filter": (S.zlib_deflate(bytes(bad_filter)) + struct.pack(">I", zlib.adler32(bytes(bad_filter))), R.FILTER),
        "adler": (good + bytes([adler[0] ^ 1]) + adler[1:], R.ADLER),
    }
    return {name: (S.png_of_body(H, W, ch, body), st) for name, (body, st) in bodies.items()}, S.png_of_body(H, W, ch, good + adler)


def test_flagged_streams_end_as_their_status():
    """One stream per status code (two for SHORT), between two sound frames: each ends as the law's status and nothing else changes."""
    flagged, good = flagged_streams()
    for name, (data, st) in flagged.items():
        assert ref(data)[1] == st, name
    pngs = [good] + [data for data, _st in flagged.values()] + [good]
    frames, status = check(pngs)
    assert status == [0] + [st for _data, st in flagged.values()] + [0]
    assert np.array_equal(frames[0], frames[-1])


@pytest.mark.parametrize("chunk", (1, 2, 8))
def test_frames_do_not_depend_on_their_neighbours(chunk):
    """Five frames of different content and stream class with a damaged one in the middle: the call gives what each frame gives alone,
    and the damaged frame's neighbours are exact."""
    H, W, ch = 17, 33, 3
    imgs = [S.image(H, W, ch, seed=k, kind="noise" if k == 1 else "camera") for k in range(5)]
    pngs = [S.pil_png(imgs[0]), S.pil_png(imgs[1], compress_level=0), None, S.hand_built(H, W, ch, seed=3)["mixed"][1], png_ref.encode_frame(imgs[4])]
    body = bytearray(R.body_of(S.pil_png(imgs[2])))
    body[len(body) // 2] ^= 0x10
    pngs[2] = S.png_of_body(H, W, ch, bytes(body))
    assert ref(pngs[2])[1] != 0
    frames, status = check(pngs, chunk=chunk)
    for k in (0, 1, 3, 4):
        alone, st = gpu([pngs[k]])
        assert st == [0] and status[k] == 0 and np.array_equal(alone[0], frames[k])
    assert gpu([pngs[2]])[1] == [status[2]]
    assert np.array_equal(frames[1], R.to_rgb(imgs[1])) and np.array_equal(frames[3], ref(pngs[3])[0])


def _call(rgb, status, body, offsets, n_channels, raw, over=None):
    """a3d_png_decode on one uploaded body, straight through the C interface -> its return code."""
    from articulation3d_amd import _lib
    from articulation3d_amd.ops import _p, _stream

    blob = torch.from_numpy(np.frombuffer(body + bytes(-len(body) % 4 + 4), np.uint8).copy()).cuda()
    off = np.array(offsets, np.int32)
    off_dev = torch.from_numpy(off).cuda()
    d = _lib.PngDecodeDesc()
    d.F, d.H, d.W, d.pitch, d.channels, d.data_bytes = rgb.shape[0], rgb.shape[1], rgb.shape[2], rgb.shape[2], n_channels, len(body)
    d.frame_off = C.cast(off.ctypes.data, C.POINTER(C.c_int))
    d.d_data, d.d_frame_off, d.raw, d.rgb, d.status = _p(blob), _p(off_dev), _p(raw), _p(rgb), _p(status)
    for k, v in (over or {}).items():
        setattr(d, k, v)
    rc = _lib.lib().a3d_png_decode(C.byref(d), _stream())
    torch.cuda.synchronize()
    return rc


def test_arguments_outside_the_law_are_refused_before_any_launch():
    from articulation3d_amd import opt_ops

    H, W, ch = 5, 4, 3
    data = flagged_streams()[1]
    body = R.body_of(data)
    rgb = torch.full((1, H, W, 3), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    raw = torch.empty(opt_ops.png_decode_scratch(H, W, ch) + 16, dtype=torch.uint8, device="cuda")
    n = len(body)
    bad = [dict(channels=0), dict(channels=5), dict(H=0), dict(W=0), dict(pitch=W - 1), dict(F=-1), dict(F=65536), dict(data_bytes=n + 1), dict(data_bytes=-1),
           dict(d_data=None), dict(d_frame_off=None), dict(raw=None), dict(rgb=None), dict(status=None), dict(frame_off=None),
           dict(raw=raw.data_ptr() + 8), dict(d_data=raw.data_ptr() + 2), dict(status=raw.data_ptr() + 2), dict(d_frame_off=raw.data_ptr() + 2),
           dict(H=65536, W=16384, pitch=16384, channels=4)]
    for over in bad:
        assert _call(rgb, status, body, [0, n], ch, raw, over) == -1, over
    for offsets in ([1, n], [0, n - 1], [0, n + 1]):
        assert _call(rgb, status, body, offsets, ch, raw) == -1, offsets
    two = torch.empty((2, H, W, 3), dtype=torch.uint8, device="cuda")
    raw2 = torch.empty(2 * opt_ops.png_decode_scratch(H, W, ch), dtype=torch.uint8, device="cuda")
    assert _call(two, torch.empty(2, dtype=torch.int32, device="cuda"), body, [0, n + 4, n], ch, raw2) == -1
    with pytest.raises(ValueError):
        opt_ops.png_decode_scratch(65536, 16384, 4)
    assert (rgb == 0x5A).all() and status.tolist() == [-7]
    assert _call(rgb, status, body, [0, n], ch, raw) == 0
    assert status.tolist() == [0] and np.array_equal(rgb[0].cpu().numpy(), ref(data)[0])
    assert _call(rgb[:0], status[:0], b"", [0], ch, raw) == 0  # F == 0: a no-op


def test_pitch_wider_than_the_frame_leaves_the_padding_alone():
    from articulation3d_amd import opt_ops

    H, W, ch = 17, 33, 4
    pngs = [S.pil_png(S.image(H, W, ch, seed=k)) for k in range(2)]
    wide = torch.full((2, H, W + 11, 3), 0x5A, dtype=torch.uint8, device="cuda")
    bodies = [R.body_of(p) for p in pngs]
    blob = b"".join(bodies)
    off = np.array([0, len(bodies[0]), len(blob)], np.int32)
    status = torch.empty(2, dtype=torch.int32, device="cuda")
    raw = torch.empty(2 * opt_ops.png_decode_scratch(H, W, ch), dtype=torch.uint8, device="cuda")
    data = torch.from_numpy(np.frombuffer(blob + bytes(-len(blob) % 4 + 4), np.uint8).copy()).cuda()
    opt_ops.png_decode_into(wide[:, :, 5:5 + W], status, data, off, torch.from_numpy(off).cuda(), ch, raw)
    got = wide.cpu().numpy()
    assert status.tolist() == [0, 0]
    for k in range(2):
        assert np.array_equal(got[k, :, 5:5 + W], ref(pngs[k])[0])
    assert (got[:, :, :5] == 0x5A).all() and (got[:, :, 5 + W:] == 0x5A).all()


def test_strict_and_mixed_geometries():
    from articulation3d_amd import png

    flagged, good = flagged_streams()
    assert np.array_equal(png.png_decode([good]).cpu().numpy()[0], ref(good)[0])
    with pytest.raises(ValueError, match="frame 1: status ADLER"):
        png.png_decode([good, flagged["adler"][0]])
    with pytest.raises(ValueError, match="frame 1 is"):
        png.png_decode([good, S.pil_png(S.image(5, 4, 4))])
    with pytest.raises(ValueError, match="frame 0: palette"):
        png.png_decode([S.container(5, 4, 1, [zlib.compress(bytes(25))], colour=3)])


def test_round_trip_through_the_encoder():
    """480 x 640: what png.png_encode writes, png_decode reads back exactly."""
    from articulation3d_amd import png

    frames = np.stack([png_ref.camera(480, 640), png_ref.mixed(480, 640)])
    files = png.png_encode(torch.from_numpy(frames).cuda())
    assert np.array_equal(png.png_decode(files).cpu().numpy(), frames)


def _inference():
    spec = importlib.util.spec_from_file_location("a3d_tools_inference_png", os.path.join(ROOT, "tools", "inference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_read_frames_of_a_directory_under_every_decoder(tmp_path):
    """PNG files of every channel count, one flagged, one palette file and one JPEG: the same arrays under pil, gpu and auto."""
    from PIL import Image

    H, W = 48, 64
    tool = _inference()
    rgb = [S.image(H, W, 3, seed=k) for k in range(3)]
    blobs = {"0.png": S.pil_png(rgb[0]), "1.png": S.pil_png(rgb[1], compress_level=0), "2.png": S.pil_png(S.image(H, W, 4, seed=7)),
             "3.png": S.pil_png(S.image(H, W, 1, seed=8)), "6.png": S.hand_built(H, W, 3, seed=2)["mixed"][1]}
    body = R.body_of(blobs["0.png"])
    blobs["4.png"] = S.png_of_body(H, W, 3, body[:-1])  # a checksum cut short: SHORT on the GPU, PIL has every row and reads the pixels
    b = io.BytesIO()
    Image.fromarray(rgb[2]).convert("P").save(b, "PNG")
    blobs["5.png"] = b.getvalue()
    b = io.BytesIO()
    Image.fromarray(rgb[2]).save(b, "JPEG", quality=90)
    blobs["7.jpg"] = b.getvalue()
    for name, data in blobs.items():
        (tmp_path / name).write_bytes(data)
    want = np.stack([S.pil_rgb(blobs[name]) for name in sorted(blobs)])
    assert np.array_equal(want[0], rgb[0]) and np.array_equal(want[4], rgb[0])
    assert tool.gpu_decodes_png(None, "gpu") and not tool.gpu_decodes_png(None, "pil")
    for decoder in ("pil", "gpu", "auto"):
        got = tool.read_frames(str(tmp_path), decoder=decoder)
        assert got.dtype == np.uint8 and np.array_equal(got, want), decoder
