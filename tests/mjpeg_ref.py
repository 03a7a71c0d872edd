"""The law of the Motion-JPEG encoder (articulation3d_amd/video.py, csrc/jpeg.hip), in numpy, integers only.  The kernels
reproduce `encode_frame` byte for byte; tests/test_mjpeg_host.py pins this file to PIL's libjpeg (headers and flat images byte
for byte, everything else by decoding), so it depends on nothing of the package but the AVI writer it forwards to.

A frame is a baseline JFIF 1.01 image, 8-bit, Y / Cb / Cr at 4:4:4, with a restart interval of one MCU row: every MCU row is
an independent entropy-coded segment, which is the unit of this file (`encode_segment`).  The tables below are typed in from
ITU-T T.81 Annex K (K.1, K.2 quantisation; K.3 - K.6 Huffman).

  colour    Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
            Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
            Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16      (libjpeg's jccolor.c constants and rounding)
  edges     pixel (y, x) of a block past the image is pixel (min(y, H-1), min(x, W-1))
  DCT       X = component - 128;  T = (X @ C13.T + 512) >> 10  (rows);  F = (C13 @ T + 32768) >> 16  (columns), C13 the 8 x 8
            DCT-II matrix in 13-bit fixed point, >> arithmetic.  Worst case: |X| <= 128 and a row of C13 sums to at most 23168 in
            magnitude (rows 0 and 4: 8 * 2896), so |X @ C13.T| <= 2 965 504 and |T| <= 2896; |C13 @ T| <= 23168 * 2896 =
            67 094 528 < 2^31.  |F[0,0]| <= 1024 (reached by X = -128 alone), so a DC difference is within +-2040: category 11.
            An AC basis function has both signs, X is at most +127 on one of them, so |F| < 1024 there: category 10.
  quantise  q = sign(F) * ((|F| + (Q >> 1)) // Q), Q the Annex K table scaled as libjpeg's jpeg_set_quality scales it
  entropy   the DC predictors start at 0 in every segment; AC runs over 15 emit ZRL, a block that ends in zeros emits EOB;
            negative amplitudes in one's complement; the segment's last byte is filled with 1-bits; every 0xFF byte of a
            segment (the filled one included) is followed by 0x00.
  bound     a block is at most 9 + 11 bits of DC and 63 * (16 + 10) bits of AC = 1658 bits (BLOCK_BITS_MAX); stuffing at most
            doubles the bytes of a segment.
"""
from __future__ import annotations

import struct

import numpy as np

QUANT_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int64)
QUANT_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], np.int64)
ZIGZAG = np.array([  # ZIGZAG[i] = natural (row-major) index of the i-th coefficient in zigzag order
    0, 1, 8, 16, 9, 2, 3, 10,
    17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34,
    27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36,
    29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46,
    53, 60, 61, 54, 47, 55, 62, 63], np.int64)

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7,
    0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5,
    0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0,
    0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
    0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA]

# 13-bit DCT-II: C13[k][n] = rint(8192 * a(k) * cos((2n + 1) k pi / 16)), a(0) = sqrt(1/8), a(k > 0) = 1/2
_C = {1: 4017, 2: 3784, 3: 3406, 4: 2896, 5: 2276, 6: 1567, 7: 799}  # rint(4096 cos(j pi / 16)); 2896 is also rint(8192 / sqrt(8))


def _c13():
    m = np.zeros((8, 8), np.int64)
    for k in range(8):
        for n in range(8):
            j = ((2 * n + 1) * k) % 32  # cos(j pi / 16), folded into the first quadrant
            j = 32 - j if j > 16 else j
            m[k, n] = 2896 if k == 0 else (_C[j] if j < 8 else -_C[16 - j])
    return m


C13 = _c13()
BLOCK_BITS_MAX = 9 + 11 + 63 * (16 + 10)


def huffman_codes(bits, vals):
    """Annex C: symbol -> (code, length) of a table given as its 16 counts and its symbols."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    assert k == len(vals)
    return out


DC_CODES = (huffman_codes(DC_LUMA_BITS, DC_VALS), huffman_codes(DC_CHROMA_BITS, DC_VALS))
AC_CODES = (huffman_codes(AC_LUMA_BITS, AC_LUMA_VALS), huffman_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))


def quant_tables(quality: int):
    """(luma, chroma) int64 [64] in natural order: jpeg_set_quality with force_baseline."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality {quality}: want 1 .. 100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (QUANT_LUMA, QUANT_CHROMA))


def ycc(rgb: np.ndarray) -> np.ndarray:
    """uint8 [...,3] RGB -> int64 [...,3] Y, Cb, Cr in 0 .. 255."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr], -1)


def coefficients(frame: np.ndarray, mcu_row: int, quality: int) -> np.ndarray:
    """The quantised coefficients of one MCU row: int64 [mcus, 3, 64], zigzag order."""
    H, W, _ = frame.shape
    mcus = (W + 7) // 8
    ys = np.minimum(np.arange(8 * mcu_row, 8 * mcu_row + 8), H - 1)
    xs = np.minimum(np.arange(8 * mcus), W - 1)
    x = ycc(frame[ys][:, xs]) - 128                                   # [8, 8*mcus, 3]
    x = x.reshape(8, mcus, 8, 3).transpose(1, 3, 0, 2)                # [mcus, 3, row, col]
    t = (x @ C13.T + (1 << 9)) >> 10
    f = (C13 @ t + (1 << 15)) >> 16
    assert np.abs(x @ C13.T).max(initial=0) < 2 ** 31 and np.abs(C13 @ t).max(initial=0) < 2 ** 31
    ql, qc = quant_tables(quality)
    q = np.stack([ql, qc, qc]).reshape(1, 3, 8, 8)
    v = np.sign(f) * ((np.abs(f) + (q >> 1)) // q)
    return v.reshape(mcus, 3, 64)[:, :, ZIGZAG]


class Report:
    """What a stream used: tests prove with it that a case was exercised."""

    def __init__(self):
        self.dc_symbols, self.ac_symbols = set(), set()  # (table, symbol)
        self.zrl = self.eob = self.blocks_without_eob = self.negative_dc_diffs = 0
        self.max_ac_category = self.max_dc_category = self.max_block_bits = 0
        self.stuffed_bytes = self.segments = self.segments_padded_to_ff = 0


def _category(v: int) -> int:
    return int(abs(v)).bit_length()


def encode_segment(frame: np.ndarray, mcu_row: int, quality: int, report: Report = None) -> bytes:
    """The entropy-coded bytes of MCU row `mcu_row` of uint8 [H,W,3] `frame`: filled to a byte with 1-bits and stuffed, without
    the RST marker that follows it in the file."""
    rep = report if report is not None else Report()
    coef = coefficients(frame, mcu_row, quality)
    out = bytearray()
    acc = n = 0
    pred = [0, 0, 0]

    def put(code, length):
        nonlocal acc, n
        acc, n = (acc << length) | code, n + length
        while n >= 8:
            out.append((acc >> (n - 8)) & 0xFF)
            n -= 8
        acc &= (1 << n) - 1

    def amplitude(v, cat):
        return v if v >= 0 else v + (1 << cat) - 1

    for mcu in range(coef.shape[0]):
        for c in range(3):
            tbl, z = (0 if c == 0 else 1), [int(v) for v in coef[mcu, c]]
            start = len(out) * 8 + n
            diff, pred[c] = z[0] - pred[c], z[0]
            cat = _category(diff)
            assert cat <= 11, "DC difference category above 11"
            rep.dc_symbols.add((tbl, cat))
            rep.negative_dc_diffs += diff < 0
            rep.max_dc_category = max(rep.max_dc_category, cat)
            put(*DC_CODES[tbl][cat])
            put(amplitude(diff, cat), cat)
            run = 0
            for v in z[1:]:
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    put(*AC_CODES[tbl][0xF0])
                    rep.ac_symbols.add((tbl, 0xF0))
                    rep.zrl += 1
                    run -= 16
                cat = _category(v)
                assert cat <= 10, "AC category above 10"
                rep.ac_symbols.add((tbl, run << 4 | cat))
                rep.max_ac_category = max(rep.max_ac_category, cat)
                put(*AC_CODES[tbl][run << 4 | cat])
                put(amplitude(v, cat), cat)
                run = 0
            if run:
                put(*AC_CODES[tbl][0x00])
                rep.ac_symbols.add((tbl, 0x00))
                rep.eob += 1
            else:
                rep.blocks_without_eob += 1
            bits = len(out) * 8 + n - start
            assert bits <= BLOCK_BITS_MAX
            rep.max_block_bits = max(rep.max_block_bits, bits)
    if n:
        put((1 << (8 - n)) - 1, 8 - n)
        rep.segments_padded_to_ff += out[-1] == 0xFF
    rep.segments += 1
    rep.stuffed_bytes += out.count(0xFF)
    return bytes(out).replace(b"\xff", b"\xff\x00")


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def headers(H: int, W: int, quality: int) -> bytes:
    """SOI .. SOS header, in libjpeg's order."""
    if H < 1 or W < 1 or H > 65535 or W > 65535:
        raise ValueError(f"{H} x {W}: a JPEG is 1 .. 65535 pixels a side")
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, t in enumerate((ql, qc)):
        out += _segment(0xDB, bytes([i]) + bytes(int(v) for v in t[ZIGZAG]))
    out += _segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, struct.pack(">H", (W + 7) // 8))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode_frame(frame: np.ndarray, quality: int, report: Report = None) -> bytes:
    """uint8 [H,W,3] RGB -> one complete JFIF file."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    H, W, _ = frame.shape
    rows = (H + 7) // 8
    out = [headers(H, W, quality)]
    for r in range(rows):
        out.append(encode_segment(frame, r, quality, report))
        if r + 1 < rows:
            out.append(bytes([0xFF, 0xD0 + r % 8]))
    return b"".join(out) + b"\xff\xd9"


def write_avi(path, jpegs, width: int, height: int, fps) -> None:
    """A RIFF `AVI ` file of Motion-JPEG frames: articulation3d_amd.video.MJPEGWriter is the one writer of the container
    (tests/test_mjpeg_host.py walks its files with a parser of its own)."""
    from articulation3d_amd.video import MJPEGWriter

    with MJPEGWriter(path, width, height, fps) as w:
        for j in jpegs:
            w.write(j)


# ---------------------------------------------------------------------------------------------------------------------
# seeded cases shared by the host and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def noise(H: int, W: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def structured(H: int = 77, W: int = 45) -> np.ndarray:
    """Gradients in both directions, a saturated rectangle, a one-pixel line and (from 16 x 8 up) one grey block in the sign pattern of
    the highest DCT basis function: its last coefficient is non-zero (no EOB) behind long zero runs (ZRL in the luminance class at low
    quality; the chrominance class reaches ZRL on the rectangle's edges)."""
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), (xx + yy) * 255 // max(H + W - 2, 1)], -1).astype(np.uint8)
    img[H // 4:H // 2, W // 3:2 * W // 3] = (255, 0, 255)
    img[2 * H // 3, :] = (0, 255, 0)
    if H >= 16 and W >= 8:
        img[8:16, 0:8] = np.where(np.outer(C13[7], C13[7]) > 0, 188, 68)[:, :, None]
    return img


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def extreme(pairs=((0, 1), (1, 0), (1, 1), (4, 4), (7, 7), (0, 4))) -> np.ndarray:
    """[8, 8 * len(pairs), 3]: block i is black and white in the sign pattern of the DCT basis function pairs[i], the input that drives
    that coefficient to its largest magnitude (AC category 10 at quality 100)."""
    blocks = [np.where(np.outer(C13[k], C13[l]) > 0, 255, 0) for k, l in pairs]
    return np.repeat(np.concatenate(blocks, 1)[:, :, None], 3, 2).astype(np.uint8)


def smooth_frames(n: int, H: int = 480, W: int = 640, seed: int = 5) -> np.ndarray:
    """uint8 [n,H,W,3]: drifting low-frequency colour fields with mild sensor-like noise -- what a camera frame costs a JPEG encoder,
    which the uniform noise of the synthetic clips is not."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W, 3), np.uint8)
    for f in range(n):
        for c in range(3):
            ph = rng.uniform(0, 2 * np.pi, 3)
            v = 128 + 60 * np.sin(xx / (40.0 + 25 * c) + ph[0] + 0.1 * f) + 50 * np.cos(yy / (55.0 - 10 * c) + ph[1]) + 15 * np.sin((xx + yy) / 9.0 + ph[2])
            out[f, :, :, c] = np.clip(np.rint(v + rng.normal(0, 2.0, (H, W))), 0, 255).astype(np.uint8)
    return out


_ROW = []


def rendered_row() -> np.ndarray:
    """One four-panel row [480, 2560, 3] of the visualisation, rendered by tests/render_ref.py: a smooth frame, 4 optimised and 5 raw
    detections.  Computed once per process."""
    if not _ROW:
        import render_ref as R
        from articulation3d_amd import render

        H, W = 480, 640
        rng = np.random.default_rng(77)
        frame = smooth_frames(1, H, W)
        row = np.zeros((1, H, 4 * W, 3), np.uint8)
        for col, n in ((0, 4), (2 * W, 5)):
            preds = [R.make_instances(rng, H, W, n)]
            tables = render.build_layers(preds, H, W, mask_alpha=0.4)
            R.render_tables(frame, tables, render.unit_normals(preds, tables).numpy(), R.pack_bits(preds[0].pred_masks.numpy()), row, col)
        _ROW.append(row[0])
    return _ROW[0]
