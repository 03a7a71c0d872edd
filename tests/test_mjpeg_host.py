"""Host suite of the Motion-JPEG path: tests/mjpeg_ref.py (the law the kernels of csrc/jpeg.hip reproduce byte for byte) is held to an
independent implementation, PIL's libjpeg -- headers and flat images byte for byte, everything else by decoding -- and the AVI
container of articulation3d_amd/video.py to a RIFF walker written here from the format.  Sizes are H x W."""
import io
import os
import struct
import sys
from fractions import Fraction

import numpy as np
import pytest
from PIL import Image

import mjpeg_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The PSNR rule: psnr(decoded law stream, source) >= psnr(PIL's own 4:4:4 encode at the same quality, decoded, source) - margin.
# The law and libjpeg differ only in the rounding of two integer DCTs (13-bit matrix here, jfdctint there) and in nothing else (the
# colour conversion and the quantiser's rounding are libjpeg's), so they trade hundredths of a decibel in both directions; a real
# defect (a wrong table entry, a transposed block, a lost coefficient) costs whole decibels.  Measured deficits of the law against
# PIL over exactly the cases of quality_cases() (dB, positive = the law is worse):
#   noise 77 x 45      q 50 +0.0001   q 90 +0.0159   q 100 -0.0666
#   structured 77 x 45 q 50 -0.0043   q 90 +0.0746   q 100 -0.1129
#   rendered row 480 x 2560, q 90  +0.0532
# The largest is 0.0746 dB; rounded up to the next 0.05 dB that is the margin.
PSNR_MARGIN_DB = 0.10
FLAT_COLOURS = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (255, 0, 0), (0, 255, 0), (0, 0, 255), (12, 200, 77), (1, 2, 3), (254, 253, 252)]


def pil_jpeg(img: np.ndarray, quality: int) -> bytes:
    """PIL's own file of the same structure: 4:4:4, standard tables, one restart interval per MCU row."""
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=0, restart_marker_rows=1, optimize=False)
    return buf.getvalue()


def through_sos(jpeg: bytes) -> bytes:
    """Everything up to and including the SOS header, found by walking the marker segments."""
    assert jpeg[:2] == b"\xff\xd8"
    at = 2
    while True:
        assert jpeg[at] == 0xFF, at
        marker, n = jpeg[at + 1], int.from_bytes(jpeg[at + 2:at + 4], "big")
        at += 2 + n
        if marker == 0xDA:
            return jpeg[:at]


def decode(jpeg: bytes, H: int, W: int) -> np.ndarray:
    im = Image.open(io.BytesIO(jpeg))
    assert im.size == (W, H) and im.mode == "RGB" and im.format == "JPEG"
    return np.asarray(im)


def psnr_deficit(jpeg: bytes, img: np.ndarray, quality: int) -> float:
    """PIL's PSNR minus this stream's, both against the source (positive = this stream is worse)."""
    H, W, _ = img.shape
    return M.psnr(decode(pil_jpeg(img, quality), H, W), img) - M.psnr(decode(jpeg, H, W), img)


def quality_cases():
    return [("noise", M.noise(77, 45, 1), (50, 90, 100)), ("structured", M.structured(), (50, 90, 100)), ("rendered row", M.rendered_row(), (90,))]


def walk_avi(data: bytes):
    """A RIFF walker written from the AVI format (not from the writer): -> dict with avih / strh / strf fields, the 00dc payloads in
    file order and the idx1 entries.  Checks the nesting and that the sizes of RIFF / hdrl / strl / movi / idx1 are consistent."""
    def chunks(lo, hi):
        out = []
        while lo < hi:
            assert lo % 2 == 0, f"chunk at odd offset {lo}"
            cc, n = data[lo:lo + 4], struct.unpack_from("<I", data, lo + 4)[0]
            assert lo + 8 + n <= hi, (cc, lo, n, hi)
            out.append((cc, lo + 8, n))
            lo += 8 + n + (n & 1)
        assert lo == hi or lo == hi + 1
        return out

    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack_from("<I", data, 4)[0] == len(data) - 8
    top = chunks(12, len(data))
    assert [(c, data[o:o + 4]) for c, o, _n in top[:2]] == [(b"LIST", b"hdrl"), (b"LIST", b"movi")] and top[2][0] == b"idx1" and len(top) == 3
    (_c, hdrl_at, hdrl_n), (_c, movi_at, movi_n), (_c, idx_at, idx_n) = top
    hd = chunks(hdrl_at + 4, hdrl_at + hdrl_n)
    assert [c for c, _o, _n in hd] == [b"avih", b"LIST"] and hd[0][2] == 56 and data[hd[1][1]:hd[1][1] + 4] == b"strl"
    sl = chunks(hd[1][1] + 4, hd[1][1] + hd[1][2])
    assert [(c, n) for c, _o, n in sl] == [(b"strh", 56), (b"strf", 40)]
    avih = struct.unpack_from("<14I", data, hd[0][1])
    strh = struct.unpack_from("<4s4sIHHIIIIIIII4H", data, sl[0][1])
    strf = struct.unpack_from("<IiiHH4sIiiII", data, sl[1][1])
    frames = [(o, n) for c, o, n in chunks(movi_at + 4, movi_at + movi_n) if c == b"00dc"]
    assert len(frames) == len(chunks(movi_at + 4, movi_at + movi_n)), "a chunk of movi is not 00dc"
    assert idx_n % 16 == 0
    index = [struct.unpack_from("<4sIII", data, idx_at + 16 * i) for i in range(idx_n // 16)]
    for (cc, flags, off, n), (o, fn) in zip(index, frames):  # offsets count from the 'movi' fourcc and point at the chunk header
        assert cc == b"00dc" and flags & 0x10 and movi_at + off + 8 == o and n == fn and data[movi_at + off:movi_at + off + 4] == b"00dc"
        assert struct.unpack_from("<I", data, movi_at + off + 4)[0] == n
    assert len(index) == len(frames)
    return {"usec_per_frame": avih[0], "flags": avih[3], "total_frames": avih[4], "streams": avih[6], "width": avih[8], "height": avih[9],
            "type": strh[0], "handler": strh[1], "scale": strh[6], "rate": strh[7], "length": strh[9],
            "bi_width": strf[1], "bi_height": strf[2], "bi_planes": strf[3], "bi_bits": strf[4], "bi_compression": strf[5],
            "frames": [data[o:o + n] for o, n in frames], "frame_offsets": [o for o, _n in frames]}


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", [1, 50, 75, 90, 100])
@pytest.mark.parametrize("H,W", [(1, 1), (16, 24), (77, 45)])
def test_headers_equal_libjpegs(H, W, quality):
    """SOI .. SOS of the law and of the product's host code (its tables come out of the kernel library) equal PIL's byte for byte: the
    segment order, JFIF 1.01, both DQT, SOF0 at 4:4:4, the four Annex K DHT, DRI = MCUs per row, the scan header."""
    from articulation3d_amd import video

    want = through_sos(pil_jpeg(np.zeros((H, W, 3), np.uint8), quality))
    assert M.headers(H, W, quality) == want
    assert video.jpeg_headers(H, W, quality) == want
    assert struct.pack(">BBHH", 0xFF, 0xDD, 4, (W + 7) // 8) in want


def test_tables_are_typed_in_not_read_from_pil():
    """The DQT / DHT segments written equal those of a PIL file with optimize=False at the same quality, and nothing of the product's
    encoder imports PIL."""
    src = open(os.path.join(ROOT, "articulation3d_amd", "video.py")).read()
    assert "PIL" not in src and "Image" not in src

    def tables(jpeg):
        out, at = [], 2
        while jpeg[at + 1] != 0xDA:
            n = int.from_bytes(jpeg[at + 2:at + 4], "big")
            if jpeg[at + 1] in (0xDB, 0xC4):
                out.append(jpeg[at:at + 2 + n])
            at += 2 + n
        return out

    for quality in (1, 50, 90, 100):
        ours, theirs = tables(M.headers(8, 8, quality)), tables(pil_jpeg(np.zeros((8, 8, 3), np.uint8), quality))
        assert len(ours) == 6 and ours == theirs
    assert np.array_equal(M.C13, np.rint(8192 * np.array([[(np.sqrt(1 / 8) if k == 0 else 0.5) * np.cos((2 * n + 1) * k * np.pi / 16) for n in range(8)]
                                                        for k in range(8)])).astype(np.int64))


@pytest.mark.parametrize("quality", [50, 90, 100])
def test_flat_images_equal_libjpegs_byte_for_byte(quality):
    """77 x 45: 10 segments, so the RST counter wraps.  The whole file: headers, Huffman coding, padding, RST numbering, EOI."""
    for colour in FLAT_COLOURS:
        img = np.empty((77, 45, 3), np.uint8)
        img[:] = colour
        assert M.encode_frame(img, quality) == pil_jpeg(img, quality), colour
    for H, W in ((16, 24), (1, 1)):
        img = np.full((H, W, 3), 200, np.uint8)
        assert M.encode_frame(img, quality) == pil_jpeg(img, quality), (H, W)


def test_streams_decode_and_hold_the_psnr_rule():
    """Noise and the structured image at 77 x 45, one rendered four-panel row at 480 x 2560: PIL opens every stream at the right size
    as RGB, and the law is within PSNR_MARGIN_DB of PIL's own encode (never compared with the kernel)."""
    worst = -1e9
    for name, img, qualities in quality_cases():
        for quality in qualities:
            d = psnr_deficit(M.encode_frame(img, quality), img, quality)
            print(f"{name} {img.shape[0]} x {img.shape[1]} q {quality}: deficit {d:+.4f} dB")
            worst = max(worst, d)
            assert d <= PSNR_MARGIN_DB, (name, quality, d)
    assert 0.05 * np.ceil(worst / 0.05) <= PSNR_MARGIN_DB + 1e-9  # the margin is the measured worst case rounded up to 0.05 dB


def test_the_cases_exercise_the_whole_law():
    """What the GPU suite compares byte for byte (three noise frames at q 100, the structured image at q 1 / 50 / 90, the extreme blocks
    at q 100) reaches every branch of the entropy coder."""
    noise, low, mid, ext = M.Report(), M.Report(), M.Report(), M.Report()
    streams = [M.encode_frame(M.noise(77, 45, seed), 100, noise) for seed in (1, 2, 3)]
    M.encode_frame(M.structured(), 1, low)
    M.encode_frame(M.structured(), 50, mid)
    M.encode_frame(M.structured(), 90, mid)
    M.encode_frame(M.extreme(), 100, ext)
    assert {(0, 0xF0), (1, 0xF0)} <= low.ac_symbols and (1, 0xF0) in mid.ac_symbols and low.zrl and mid.zrl   # ZRL, both classes
    assert mid.eob > 0 and (0, 0x00) in mid.ac_symbols and (1, 0x00) in mid.ac_symbols        # EOB, both classes
    assert noise.blocks_without_eob > 0                                                       # a block whose 63rd coefficient is non-zero
    assert noise.negative_dc_diffs > 0 and mid.negative_dc_diffs > 0
    assert ext.max_ac_category == 10 and noise.max_ac_category >= 8                           # the largest AC category there is
    assert noise.max_dc_category >= 9
    assert noise.stuffed_bytes > 0 and any(b"\xff\x00" in s for s in streams)                 # byte stuffing
    assert noise.segments_padded_to_ff > 0                                                    # a filled last byte that is 0xFF itself
    assert noise.segments == 30 and all(s.count(b"\xff\xd7") >= 1 and b"\xff\xd0" in s[s.index(b"\xff\xd7"):] for s in streams)  # RST wraps
    for rep in (noise, low, mid, ext):
        assert 0 < rep.max_block_bits <= M.BLOCK_BITS_MAX
    assert M.BLOCK_BITS_MAX == 1658


def test_a_segment_stands_alone():
    """encode_segment of one MCU row is that row's bytes in the whole file: the unit the GPU suite compares on large frames."""
    img = M.noise(24, 2056, 3)
    whole = M.encode_frame(img, 100)
    body = whole[len(M.headers(24, 2056, 100)):-2]
    segs = [M.encode_segment(img, r, 100) for r in range(3)]
    assert body == segs[0] + b"\xff\xd0" + segs[1] + b"\xff\xd1" + segs[2]
    assert M.coefficients(img, 1, 100).shape == (257, 3, 64)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fps,rate_scale", [(30, (30, 1)), (Fraction(30000, 1001), (30000, 1001)), ((30000, 1001), (30000, 1001)), ("24", (24, 1))])
def test_avi_container(tmp_path, fps, rate_scale):
    jpegs = [M.encode_frame(M.noise(16, 24, seed), q) for seed, q in ((1, 50), (2, 90), (3, 100))]
    assert any(len(j) % 2 for j in jpegs) and any(len(j) % 2 == 0 for j in jpegs)  # odd and even lengths
    path = tmp_path / "clip.avi"
    M.write_avi(path, jpegs, 24, 16, fps)
    avi = walk_avi(path.read_bytes())
    assert avi["frames"] == jpegs and all(o % 2 == 0 for o in avi["frame_offsets"])
    assert (avi["total_frames"], avi["length"], avi["streams"]) == (3, 3, 1) and avi["flags"] & 0x10
    assert (avi["width"], avi["height"], avi["bi_width"], avi["bi_height"]) == (24, 16, 24, 16)
    assert (avi["type"], avi["handler"], avi["bi_compression"], avi["bi_bits"], avi["bi_planes"]) == (b"vids", b"MJPG", b"MJPG", 24, 1)
    assert Fraction(avi["rate"], avi["scale"]) == Fraction(*rate_scale) and (avi["rate"], avi["scale"]) == rate_scale
    assert avi["usec_per_frame"] == round(1e6 * rate_scale[1] / rate_scale[0])
    for j in avi["frames"]:
        assert decode(j, 16, 24).shape == (16, 24, 3)


def test_avi_writer_is_a_context_manager_and_refuses_a_gigabyte(tmp_path):
    from articulation3d_amd.video import MJPEGWriter

    class Huge(bytes):  # a frame that claims a length without holding it
        def __len__(self):
            return (1 << 30) - 100

    jpeg = M.encode_frame(M.noise(8, 8, 1), 50)
    with MJPEGWriter(tmp_path / "a.avi", 8, 8, 30) as w:
        w.write(jpeg)
        with pytest.raises(ValueError, match="1 GiB"):
            w.write(Huge(jpeg))
        w.write(jpeg)
        assert w.frames == 2
    avi = walk_avi((tmp_path / "a.avi").read_bytes())  # the refused frame left nothing behind
    assert avi["frames"] == [jpeg, jpeg] and avi["total_frames"] == 2
    with pytest.raises(ValueError):
        w.write(jpeg)
    empty = tmp_path / "empty.avi"
    MJPEGWriter(empty, 8, 8, 30).close()
    assert walk_avi(empty.read_bytes())["frames"] == []
    with pytest.raises(ValueError):
        MJPEGWriter(tmp_path / "b.avi", 8, 8, 0)


def test_inference_script_offers_avi():
    import subprocess

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import inference
    finally:
        sys.path.pop(0)
    args = inference.build_parser().parse_args(["--config", "c", "--input", "i", "--output", "o", "--vis", "avi", "--vis-quality", "80", "--fps", "24"])
    assert (args.vis, args.vis_quality, str(args.fps)) == ("avi", 80, "24")
    assert inference.build_parser().parse_args(["--config", "c", "--input", "i", "--output", "o"]).vis_quality == 90
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "inference.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "avi" in r.stdout and "Motion-JPEG" in r.stdout and "--vis-quality" in r.stdout and "--fps" in r.stdout
