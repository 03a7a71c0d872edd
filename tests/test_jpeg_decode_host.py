"""Host suite of the JPEG decode path: tests/jpeg_decode_ref.py (the law the kernels of csrc/jpeg_decode.hip reproduce byte for byte) is
held to PIL's libjpeg byte for byte, the package's pure-Python parser to the same refusals, and MJPEGReader to the RIFF walker of
tests/test_mjpeg_host.py.  Sizes are H x W."""
import os
from fractions import Fraction

import numpy as np
import pytest

import jpeg_decode_ref as D
import mjpeg_ref as M
from test_mjpeg_host import walk_avi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")


def _equal_pil(data: bytes):
    got, status = D.decode(data)
    want = D.pil_decode(data)
    assert status == D.OK and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("H,W", D.SIZES)
def test_stream_matrix_equals_pil(H, W):
    """Three images x 4:4:4 / 4:2:2 / 4:2:0 x quality 30 / 90 / 100 x (default, optimised tables, an interval of one MCU row, an
    interval of 3 blocks): 108 streams per size, every one byte for byte PIL's pixels."""
    for img in D.images(H, W):
        for sub in (0, 1, 2):
            for quality in (30, 90, 100):
                for options in D.PIL_OPTIONS:
                    _equal_pil(D.pil_jpeg(img, quality, sub, **options))


def test_grey():
    for quality in (30, 90, 100):
        for options in D.PIL_OPTIONS:
            data = D.pil_jpeg(D.grey_image(), quality, **options)
            assert len(D.parse(data).comps) == 1
            _equal_pil(data)


def test_a_frame_of_the_encoders_law():
    """77 x 45 at quality 100 from mjpeg_ref.encode_frame: ten intervals, so the restart counter wraps."""
    data = M.encode_frame(M.noise(77, 45, 1), 100)
    p = D.parse(data)
    assert len(p.units) == 10 and p.restart == 6 and [m[1] for m in D._RST.findall(data)] == [0xD0 + k % 8 for k in range(9)]
    _equal_pil(data)


def test_a_file_without_dht_uses_annex_k():
    img = D.images(45, 77)[0]
    for sub in (0, 2):
        data = D.pil_jpeg(img, 90, sub)
        bare = D.without_dht(data)
        assert b"\xff\xc4" in data[:700] and len(bare) == len(data) - 432
        assert 0xC4 not in [m for m, _lo, _hi in D.segments(bare)]
        got, status = D.decode(bare)
        assert status == D.OK and np.array_equal(got, D.pil_decode(data)) and np.array_equal(D.pil_decode(bare), got)


def test_domain():
    """Grey 80 x 160 graded noise at quality 75 / 90 / 100 with every DQT value multiplied by 6, 8, 10, 14 (capped at 255): every block the law
    puts inside its domain equals PIL, every frame with a block outside reports RANGE, and both kinds occur."""
    img = D.graded_noise()
    kinds = set()
    for quality in (75, 90, 100):
        base = D.pil_jpeg(img, quality)
        for factor in (6, 8, 10, 14):
            data = D.scaled_dqt(base, factor)
            got, status, inside = D.decode(data, detail=True)
            want = D.pil_decode(data)
            assert status == (D.OK if inside.all() else D.RANGE)
            kinds.add(status)
            same = (got == want).all(2).reshape(10, 8, 20, 8).all((1, 3))
            print(f"q {quality} x {factor}: {int(inside.sum())} of {inside.size} blocks inside, {int((inside & same).sum())} of them equal PIL")
            assert same[inside].all()
    assert kinds == {D.OK, D.RANGE}


@pytest.mark.parametrize("parse", ["ref", "package"])
def test_refusals(parse):
    import io

    from PIL import Image

    if parse == "package":
        from articulation3d_amd.video import jpeg_parse
    else:
        jpeg_parse = D.parse
    img = D.images(17, 33)[0]
    base = D.pil_jpeg(img, 90, 2)
    jpeg_parse(base)
    buf = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(buf, "JPEG")
    for data, message in ((D.pil_jpeg(img, 90, 2, progressive=True), "progressive"), (buf.getvalue(), "4 components"),
                          (D.patched_sampling(base, 0x12), "sampling factors 1x2"), (D.patched_sampling(base, 0x41), "sampling factors 4x1"),
                          (D.cut_before_sos(base), "no SOS"), (base[2:], "SOI")):
        with pytest.raises(ValueError, match=message):
            jpeg_parse(data)


def test_a_file_cut_in_its_scan_is_short():
    for options in ({}, {"restart_marker_rows": 1}):
        data = D.cut_in_scan(D.pil_jpeg(D.images(45, 77)[0], 90, 2, **options))
        assert D.decode(data)[1] == D.SHORT


def test_the_package_parser_agrees_with_the_reference_parser():
    from articulation3d_amd.video import jpeg_parse

    for sub in (0, 1, 2):
        for options in D.PIL_OPTIONS:
            data = D.pil_jpeg(D.images(45, 77)[1], 90, sub, **options)
            info, p = jpeg_parse(data), D.parse(data)
            assert info.geometry == (p.height, p.width, 3, p.hmax, p.vmax) and info.restart == p.restart
            assert [data[a:b] for a, b in info.units] == p.units and info.n_units == len(p.units) and info.scan[1] == len(data) - 2
            for c in range(3):
                assert list(info.quant[c]) == list(p.comps[c][2])
                assert [list(t) for t in info.huff[c]] == [list(p.comps[c][3][0]), list(p.comps[c][3][1]), list(p.comps[c][4][0]), list(p.comps[c][4][1])]
    bare = jpeg_parse(D.without_dht(D.pil_jpeg(D.images(16, 16)[0], 90, 0)))
    assert [list(t) for t in bare.huff[1]] == [M.DC_CHROMA_BITS, M.DC_VALS, M.AC_CHROMA_BITS, M.AC_CHROMA_VALS]


def test_reader_returns_what_the_writer_wrote(tmp_path):
    from articulation3d_amd.video import MJPEGReader, MJPEGWriter

    jpegs = [D.pil_jpeg(M.noise(24, 40, s), 90, 2) for s in (1, 2, 3)]
    assert len(jpegs[0]) % 2 or len(jpegs[1]) % 2 or len(jpegs[2]) % 2  # a padded chunk is among them
    path = tmp_path / "clip.avi"
    with MJPEGWriter(path, 40, 24, "30000/1001") as w:
        for j in jpegs:
            w.write(j)
    avi = walk_avi(path.read_bytes())
    with MJPEGReader(path) as r:
        assert (len(r), r.width, r.height, r.fps) == (3, 40, 24, Fraction(30000, 1001)) == (avi["total_frames"], avi["width"], avi["height"],
                                                                                        Fraction(avi["rate"], avi["scale"]))
        assert list(r) == jpegs == avi["frames"] and r[1:] == jpegs[1:] and r[-1] == jpegs[2] and r[0:3:2] == jpegs[0:3:2]
        assert [off for off, _n in r._frames] == avi["frame_offsets"]
        assert r._walk(avi["frame_offsets"][0] - 8, avi["frame_offsets"][2] + len(jpegs[2])) == r._frames  # a file without idx1 is walked
        with pytest.raises(IndexError):
            r[3]
    with pytest.raises(ValueError):
        r[0]
    data = bytearray(path.read_bytes())
    at = data.index(b"strh") + 12
    data[at:at + 4] = b"H264"
    (tmp_path / "other.avi").write_bytes(data)
    with pytest.raises(ValueError, match="MJPG"):
        MJPEGReader(tmp_path / "other.avi")
    (tmp_path / "dml.avi").write_bytes(path.read_bytes() + b"RIFF\x04\0\0\0AVIX")
    with pytest.raises(ValueError, match="OpenDML"):
        MJPEGReader(tmp_path / "dml.avi")


@pytest.mark.parametrize("name", ["420_optimize", "422_restart3", "444_q100", "grey"])
def test_golden_files(name):
    """Four small PIL files with the pixels PIL decoded them to when they were made: the pin survives another PIL build."""
    data = open(os.path.join(GOLDEN, name + ".jpg"), "rb").read()
    want = np.load(os.path.join(GOLDEN, name + ".npy"))
    assert len(data) <= 4096
    got, status = D.decode(data)
    assert status == D.OK and np.array_equal(got, want)
    assert np.array_equal(D.pil_decode(data), want)
