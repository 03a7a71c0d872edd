"""CPU-only: holds the PNG decoding law (tests/png_decode_ref.py, stated in include/a3d.h under "PNG decode") to zlib's inflate and to PIL,
and png.png_parse to its list of refusals.

Streams decoded and compared (counted by test_stream_count): 20 PIL-written files (five settings x four channel counts), 24 hand-filtered
ones (six filter plans x four channel counts), 60 zlib.compressobj settings (fifteen x four channel counts), 4 of the package's own files,
8 token-list streams zlib never emits, and 78 ways of cutting one file's IDAT payload into chunks: 194 accepted streams; then every
truncation and every bit flip of two small bodies, 1 620 damaged streams, each classified exactly as zlib classifies it.
"""
import struct
import zlib

import numpy as np
import pytest

import png_decode_ref as R
import png_decode_streams as S
import png_ref
from articulation3d_amd import png as P

CHANNELS = (1, 2, 3, 4)
N_STREAMS = {"pil": 20, "hand": 24, "zlib": 60, "own": 4, "special": 8, "splits": 78, "damaged": 1620}


def check_accepted(data, want_rgb=None):
    """The reference against zlib (raw bytes) and PIL (pixels) on a file the law accepts."""
    info = P.png_parse(data)
    body = R.body_of(data, info)
    raw, status, stored = R.inflate(body, info.raw_size)
    assert status == 0
    assert raw.tobytes() == zlib.decompressobj(-15).decompress(body)
    rgb, status = R.decode(data)
    assert status == 0
    assert np.array_equal(rgb, S.pil_rgb(data))
    if want_rgb is not None:
        assert np.array_equal(rgb, want_rgb)


def as_rgb(img):
    return R.to_rgb(img)


@pytest.mark.parametrize("ch", CHANNELS)
def test_pil_writer(ch):
    img = S.image(17, 33, ch, seed=ch)
    files = [S.pil_png(img, compress_level=l) for l in (0, 1, 6, 9)] + [S.pil_png(img, optimize=True)]
    assert len(files) * len(CHANNELS) == N_STREAMS["pil"]
    for data in files:
        check_accepted(data, as_rgb(img))


@pytest.mark.parametrize("ch", CHANNELS)
def test_hand_filtered_rows(ch):
    built = S.hand_built(17, 33, ch, seed=10 + ch)
    assert len(built) * len(CHANNELS) == N_STREAMS["hand"]
    for name, (img, data) in built.items():
        check_accepted(data, as_rgb(img))


@pytest.mark.parametrize("ch", CHANNELS)
def test_zlib_settings(ch):
    H, W = 17, 33
    img = S.image(H, W, ch, seed=20 + ch)
    raw = S.filter_rows(img, np.arange(H) % 5)
    streams = S.zlib_settings(raw)
    assert len(streams) * len(CHANNELS) == N_STREAMS["zlib"]
    for name, deflate in streams.items():
        check_accepted(S.png_of_raw(H, W, ch, raw, deflate), as_rgb(img))


def test_own_files():
    imgs = [png_ref.mixed(40, 50), png_ref.noise(17, 33, 3), png_ref.flat(5, 1), png_ref.camera(65, 9)]
    assert len(imgs) == N_STREAMS["own"]
    for img in imgs:
        check_accepted(png_ref.encode_frame(img), img)


def test_token_list_streams():
    streams = S.special_streams()
    assert len(streams) == N_STREAMS["special"]
    for name, (H, W, ch, data) in streams.items():
        assert P.png_parse(data).geometry == (H, W, ch), name
        check_accepted(data)


def test_idat_splits():
    """The payload of one small file cut into two chunks at every byte position, into single bytes, and left whole."""
    img = S.image(5, 4, 3, seed=3)
    raw = S.filter_rows(img, [0, 1, 2, 3, 4])  # one stored block of 65 bytes: the payload is 2 + 5 + 65 + 4 bytes whatever zlib is installed
    payload = b"\x78\x9c" + S.write_blocks([("stored", raw)]) + struct.pack(">I", zlib.adler32(raw))
    cuts = [[payload], [payload[i:i + 1] for i in range(len(payload))], [b"", payload, b""]]
    cuts += [[payload[:i], payload[i:]] for i in range(1, len(payload))]
    assert len(cuts) == N_STREAMS["splits"], len(cuts)
    for parts in cuts:
        data = S.container(5, 4, 3, parts)
        assert R.body_of(data) == payload[2:]
        check_accepted(data, img)


def test_ancillary_chunks_and_trns_are_ignored():
    img = S.image(5, 4, 3, seed=4)
    payload = zlib.compress(S.filter_rows(img, [4] * 5))
    extra = [S.chunk(b"gAMA", struct.pack(">I", 45455)), S.chunk(b"tRNS", bytes(6)), S.chunk(b"tEXt", b"k\0v")]
    check_accepted(S.container(5, 4, 3, [payload], extra=extra), img)
    grey = S.image(5, 4, 1, seed=5)
    check_accepted(S.container(5, 4, 1, [zlib.compress(S.filter_rows(grey, [1] * 5))], extra=[S.chunk(b"tRNS", b"\0\x10")]), as_rgb(grey))


def test_stream_count():
    """The docstring's and the README's numbers are the ones the tests above assert."""
    bases = S.damaged_bases()
    assert sum(len(S.damaged_variants(body)) for _, _, _, body in bases) == N_STREAMS["damaged"]
    assert sum(v for k, v in N_STREAMS.items() if k != "damaged") == 194


@pytest.mark.parametrize("which", (0, 1))
def test_damaged_streams_classified_as_zlib_does(which):
    """Every truncation and every bit flip of a small body.  The reference reports an inflate error (BAD_CODE or FAR) exactly when zlib
    raises, SHORT exactly when zlib neither raises nor finishes the frame, LONG exactly when zlib would write past the raw size (zlib is
    stopped one byte past it, where the law's walk stops), and FILTER / ADLER / 0 only on streams zlib inflates to the end.  The reference
    asserts every index it forms, so this is also the proof that the law's checks keep a decoder inside its buffers."""
    H, W, ch, body = S.damaged_bases()[which]
    raw_size = H * (1 + W * ch)
    assert R.decode_body(body, H, W, ch)[1] == 0
    seen = set()
    for bad in S.damaged_variants(body):
        want = S.expected_status(bad, raw_size)
        raw, status, stored = R.inflate(bad, raw_size)
        got = R.decode_body(bad, H, W, ch)[1]
        if isinstance(want, set):
            assert got in want
        elif want is not None:
            assert got == want
        else:
            assert status == 0 and raw.tobytes() == zlib.decompressobj(-15).decompress(bad)
            rows = raw.reshape(H, -1)
            want = R.FILTER if (rows[:, 0] > 4).any() else R.ADLER if stored != zlib.adler32(raw.tobytes()) else 0
            assert got == want
        seen.add(got)
    assert {R.SHORT, R.BAD_CODE, R.ADLER} <= seen


# ---- the parser ----------------------------------------------------------------------------------------------------------------------
def _good():
    img = S.image(5, 4, 3, seed=6)
    return S.filter_rows(img, [0] * 5), img


def _refused(data, word):
    with pytest.raises(ValueError, match=word):
        P.png_parse(data)


def test_parser_accepts_and_reports():
    raw, img = _good()
    info = P.png_parse(S.container(5, 4, 3, [zlib.compress(raw)]))
    assert info.geometry == (5, 4, 3) and info.raw_size == len(raw)
    for ch in CHANNELS:
        assert P.png_parse(S.pil_png(S.image(3, 2, ch))).channels == ch


def test_parser_refuses_palette():
    _refused(S.container(5, 4, 1, [zlib.compress(bytes(25))], colour=3, extra=[S.chunk(b"PLTE", bytes(3))]), "palette")


@pytest.mark.parametrize("depth", (1, 2, 4, 16))
def test_parser_refuses_bit_depths(depth):
    _refused(S.container(5, 8, 1, [zlib.compress(bytes(10))], depth=depth), "bit depth")


def test_parser_refuses_adam7():
    _refused(S.container(5, 4, 3, [zlib.compress(_good()[0])], interlace=1), "Adam7")


def test_parser_refuses_bad_signature():
    data = S.container(5, 4, 3, [zlib.compress(_good()[0])])
    _refused(b"\x89PNG\r\n\x1a\r" + data[8:], "signature")
    _refused(data[:7], "signature")


def test_parser_refuses_bad_crc():
    data = bytearray(S.container(5, 4, 3, [zlib.compress(_good()[0])]))
    data[45] ^= 1  # a byte of the IDAT payload
    _refused(bytes(data), "CRC")


def test_parser_refuses_missing_chunks():
    payload = zlib.compress(_good()[0])
    ihdr = S.chunk(b"IHDR", struct.pack(">IIBBBBB", 4, 5, 8, 2, 0, 0, 0))
    _refused(P.SIGNATURE + S.chunk(b"IDAT", payload) + S.chunk(b"IEND", b""), "IHDR")
    _refused(P.SIGNATURE + ihdr + S.chunk(b"IEND", b""), "IDAT")
    _refused(P.SIGNATURE + ihdr + S.chunk(b"IDAT", payload), "IEND")
    _refused(P.SIGNATURE + ihdr + S.chunk(b"IDAT", payload)[:-3], "cut short")


def test_parser_refuses_idat_that_is_not_consecutive():
    payload = zlib.compress(_good()[0])
    ihdr = S.chunk(b"IHDR", struct.pack(">IIBBBBB", 4, 5, 8, 2, 0, 0, 0))
    data = P.SIGNATURE + ihdr + S.chunk(b"IDAT", payload[:9]) + S.chunk(b"tEXt", b"k\0v") + S.chunk(b"IDAT", payload[9:]) + S.chunk(b"IEND", b"")
    _refused(data, "consecutive")


@pytest.mark.parametrize("header", (b"\x79\x9c", b"\x88\x1c", b"\x78\xbb", b"\x78\x9d", b"\x78"))
def test_parser_refuses_zlib_headers(header):
    """CM = 9; CINFO = 8; FDICT set (with a valid FCHECK); a wrong FCHECK; a payload of one byte."""
    if len(header) == 2 and header not in (b"\x78\x9d",):
        cmf, flg = header
        flg = flg & 0xE0
        flg += 31 - (cmf << 8 | flg) % 31
        header = bytes([cmf, flg])
    _refused(S.container(5, 4, 3, [header + zlib.compress(_good()[0])[2:]] if len(header) == 2 else [header]), "zlib header")


def test_parser_refuses_empty_and_oversized_images():
    _refused(S.container(0, 4, 3, [zlib.compress(b"")]), "empty")
    _refused(S.container(5, 0, 3, [zlib.compress(b"")]), "empty")
    _refused(S.container(65536, 16384, 4, [zlib.compress(b"")]), "2\\^31")
    assert P.png_parse(S.container(1, (2 ** 31 - 2) // 4, 4, [zlib.compress(b"")])).raw_size == 2 ** 31 - 3
