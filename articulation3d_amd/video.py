"""The clip's visualisation as a video: Motion-JPEG in an AVI container, the frames encoded on the GPU (a3d_jpeg_encode /
a3d_jpeg_pack, csrc/jpeg.hip; the law is stated in include/a3d.h and, in numpy, in tests/mjpeg_ref.py).

The reference ends in an H.264 output.mp4 written by imageio; H.264 needs an encoder this package does not have, Motion-JPEG needs
none.  Every frame is a baseline JFIF image (8-bit, Y / Cb / Cr at 4:4:4 so that one-pixel outlines stay sharp, Annex K tables) with
a restart interval of one MCU row, which makes every MCU row an independent piece of work for the device.  The host writes the
headers (once per size and quality) and the container; only the compressed bytes cross PCIe.

    jpeg_encode(frames_u8, quality)                      -> list[bytes], complete JFIF files
    render_clip_jpeg(frames_u8, preds_raw, preds_opt)    -> yields list[bytes] per chunk: render_clip's rows, encoded
    MJPEGWriter(path, width, height, fps)                -> .write(jpeg), .close(); a context manager

The container is a plain RIFF `AVI ` file (hdrl: avih + one strl of type vids / MJPG with a BITMAPINFOHEADER; a movi list of 00dc
chunks; idx1), which ends at 2 GiB: the writer refuses a clip that would pass 1 GiB.  OpenDML is not written.
"""
from __future__ import annotations

import functools
import struct
from fractions import Fraction
from typing import Iterator, List, Sequence

import torch

from . import _lib, opt_ops

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
MAX_AVI_BYTES = 1 << 30


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


@functools.lru_cache(maxsize=32)
def jpeg_headers(H: int, W: int, quality: int) -> bytes:
    """SOI, APP0 (JFIF 1.01, no units, density 1 x 1), two DQT, SOF0, four DHT (DC0, AC0, DC1, AC1), DRI (one MCU row), SOS: libjpeg's
    order and contents.  The tables are the kernel library's own, so a stream cannot state other tables than it was coded with."""
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"{H} x {W}: a JPEG is 1 .. 65535 pixels a side")
    quant = opt_ops.jpeg_quant(quality)
    bits, vals = opt_ops.jpeg_tables()
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2):
        out += _segment(0xDB, bytes([t]) + bytes(quant[64 * t + n] for n in ZIGZAG))
    out += _segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for t, tc_th in enumerate((0x00, 0x10, 0x01, 0x11)):
        counts = bits[16 * t:16 * t + 16]
        out += _segment(0xC4, bytes([tc_th]) + counts + vals[_lib.JPEG_HUFF_VALS * t:_lib.JPEG_HUFF_VALS * t + sum(counts)])
    out += _segment(0xDD, struct.pack(">H", (W + 7) // 8))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


class _Encoder:
    """The device and pinned buffers of one (frames per call, H, W), allocated once: worst-case slots (opt_ops.jpeg_geometry), so no
    input can overrun them.  encode() launches on the current stream; fetch() learns the lengths from one small copy, then packs and
    brings only the used bytes to the host on streams.side(2), the pool's copy role."""

    def __init__(self, cap_frames: int, H: int, W: int, device):
        self.rows, self.mcus, self.slot = opt_ops.jpeg_geometry(H, W)
        while cap_frames > 1 and cap_frames * self.rows * (self.slot + 2) > 0x7FFFFFFF:  # the library's int32 offsets
            cap_frames = (cap_frames + 1) // 2
        self.cap, self.H, self.W, self.dev = cap_frames, H, W, device
        n_seg = cap_frames * self.rows
        self.coef = torch.empty(n_seg * self.mcus * 192, dtype=torch.int16, device=device)
        self.slots = torch.empty(n_seg * self.slot, dtype=torch.uint8, device=device)
        self.meta = torch.empty(2 * n_seg + cap_frames + 1, dtype=torch.int32, device=device)  # seg_len | seg_off | frame_off
        self.seg_len, self.seg_off, self.frame_off = self.meta[:n_seg], self.meta[n_seg:2 * n_seg], self.meta[2 * n_seg:]
        self.host_off = torch.empty(cap_frames + 1, dtype=torch.int32).pin_memory()
        self.packed = torch.empty(0, dtype=torch.uint8, device=device)
        self.host = torch.empty(0, dtype=torch.uint8).pin_memory()

    def encode(self, frames_u8: torch.Tensor, quality: int) -> int:
        """Transform, entropy-code and measure n <= cap frames on the current stream; the per-frame offsets start for the host behind them."""
        n = frames_u8.shape[0]
        assert n <= self.cap and tuple(frames_u8.shape[1:3]) == (self.H, self.W)
        opt_ops.jpeg_encode_into(frames_u8, quality, self.coef, self.slots, self.seg_len, self.seg_off, self.frame_off)
        self.host_off[:n + 1].copy_(self.frame_off[:n + 1], non_blocking=True)  # the one small copy: the host learns the lengths
        self.done = torch.cuda.Event()
        self.done.record(torch.cuda.current_stream(self.dev))
        return n

    def fetch(self, n: int, head: bytes) -> List[bytes]:
        """The n frames of the last encode() as complete files.  Waits for that call alone: the pack and the copy of the used bytes run on
        the copy stream, beside whatever the caller has queued on its own stream since."""
        from . import streams

        self.done.synchronize()
        off = self.host_off[:n + 1].tolist()
        total = off[n]
        copy_stream = streams.side(2, self.dev)
        with torch.cuda.stream(copy_stream):
            if total > self.packed.numel():  # grown geometrically, kept for the next chunk
                size = max(total, 2 * self.packed.numel(), 1 << 16)
                self.packed = torch.empty(size, dtype=torch.uint8, device=self.dev)
                self.host = torch.empty(size, dtype=torch.uint8).pin_memory()
            opt_ops.jpeg_pack_into(self.slots, self.seg_off, self.seg_len, n, self.H, self.W, self.packed)
            self.host[:total].copy_(self.packed[:total], non_blocking=True)
        copy_stream.synchronize()
        data = self.host.numpy()
        return [head + data[off[f]:off[f + 1]].tobytes() + b"\xff\xd9" for f in range(n)]


def jpeg_encode(frames_u8: torch.Tensor, quality: int = 90, chunk: int = 8) -> List[bytes]:
    """uint8 [F,H,W,3] RGB on the device (dense, or a column range of wider rows) -> F complete JFIF files.  The bytes of a frame
    do not depend on F, on `chunk` or on the frames beside it."""
    F, H, W, _pitch = opt_ops._pitched_frames(frames_u8)
    head = jpeg_headers(H, W, int(quality))
    out: List[bytes] = []
    if F == 0:
        return out
    enc = _Encoder(min(max(int(chunk), 1), F), H, W, frames_u8.device)
    for lo in range(0, F, enc.cap):
        out += enc.fetch(enc.encode(frames_u8[lo:lo + enc.cap], int(quality)), head)
    return out


def render_clip_jpeg(frames_u8: torch.Tensor, preds_raw: Sequence, preds_opt: Sequence, quality: int = 90, chunk: int = 8, mask_alpha: float = 0.0,
                     conf_threshold: float = 0.7) -> Iterator[List[bytes]]:
    """Yields, `chunk` frames at a time, the clip's rows `[opt seg | opt normal | raw seg | raw normal]` as JFIF files [H, 4W]: the
    rows are rendered exactly as render.render_clip renders them (the same two render_panels calls per chunk into a device staging
    buffer) and encoded where they are; decoded, they are render_clip's rows up to the loss of JPEG at `quality`.  Raw rows never
    leave the device.  While the host waits for chunk k's bytes, chunk k+1 is already rendered and encoded behind it."""
    from .render import render_panels

    F, H, W, _ = frames_u8.shape
    assert len(preds_raw) == F and len(preds_opt) == F
    dev = frames_u8.device if frames_u8.is_cuda else torch.device("cuda", torch.cuda.current_device())
    chunk = max(1, min(int(chunk), max(F, 1)))
    head = jpeg_headers(H, 4 * W, int(quality))
    stage = [torch.empty((chunk, H, 4 * W, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
    enc = [_Encoder(chunk, H, 4 * W, dev) for _ in range(2)]
    if enc[0].cap < chunk:
        raise ValueError(f"chunk {chunk} of {H} x {4 * W} rows is more than one encoder call holds ({enc[0].cap}): pass a smaller chunk")
    pending = None
    for k, lo in enumerate(range(0, F, chunk)):
        hi, b = min(lo + chunk, F), k % 2
        fr = frames_u8[lo:hi].to(dev, non_blocking=True).contiguous()
        out = stage[b][:hi - lo]
        render_panels(fr, preds_opt[lo:hi], out=out, col=0, mask_alpha=mask_alpha, conf_threshold=conf_threshold)
        render_panels(fr, preds_raw[lo:hi], out=out, col=2 * W, mask_alpha=mask_alpha, conf_threshold=conf_threshold)
        n = enc[b].encode(out, int(quality))
        if pending is not None:  # the previous chunk's lengths, pack and copy: this chunk's launches are queued behind them
            yield pending[0].fetch(pending[1], head)
        pending = (enc[b], n)
    if pending is not None:
        yield pending[0].fetch(pending[1], head)


def _rational(fps):
    """fps as (rate, scale): an int, a Fraction, a (numerator, denominator) pair, a string such as '30000/1001', or a float."""
    if isinstance(fps, (tuple, list)):
        fr = Fraction(int(fps[0]), int(fps[1]))
    elif isinstance(fps, float):
        fr = Fraction(fps).limit_denominator(1001)
    else:
        fr = Fraction(fps)
    if fr <= 0 or fr.numerator >= 1 << 31 or fr.denominator >= 1 << 31:
        raise ValueError(f"fps {fps!r}: want a positive rational")
    return fr.numerator, fr.denominator


class MJPEGWriter:
    """Motion-JPEG frames into a RIFF `AVI ` file: write(jpeg_bytes) per frame, close() writes idx1 and patches the sizes and the
    frame count into the headers.  fps is a rational: dwRate / dwScale hold it exactly, dwMicroSecPerFrame is rounded from it."""

    _HDRL = 4 + (8 + 56) + (12 + (8 + 56) + (8 + 40))  # 'hdrl' + avih + LIST strl (strh, strf)

    def __init__(self, path, width: int, height: int, fps=30):
        if not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
            raise ValueError(f"{width} x {height}: a JPEG is 1 .. 65535 pixels a side")
        self.width, self.height = int(width), int(height)
        self.rate, self.scale = _rational(fps)
        self._index: List[tuple] = []  # (offset of the chunk from the 'movi' fourcc, length)
        self._movi = 4                 # bytes of the movi list so far, its fourcc included
        self._max = 0
        self._f = open(path, "wb")
        self._f.write(self._headers())

    def _headers(self) -> bytes:
        n, usec = len(self._index), (1000000 * self.scale + self.rate // 2) // self.rate
        avih = struct.pack("<14I", usec, (self._max * self.rate + self.scale - 1) // self.scale if n else 0, 0, 0x10, n, 0, 1, self._max,
                           self.width, self.height, 0, 0, 0, 0)  # 0x10 = AVIF_HASINDEX
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, n, self._max, 0xFFFFFFFF, 0,
                           0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + \
            b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"LIST" + struct.pack("<I", self._HDRL) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        assert len(hdrl) == 8 + self._HDRL
        riff = 4 + len(hdrl) + 8 + self._movi + 8 + 16 * n
        return b"RIFF" + struct.pack("<I", riff) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", self._movi) + b"movi"

    def _size_with(self, nbytes: int) -> int:
        """The finished file's size if a frame of `nbytes` were added now."""
        return 12 + 8 + self._HDRL + 8 + self._movi + 8 + nbytes + (nbytes & 1) + 8 + 16 * (len(self._index) + 1)

    def write(self, jpeg: bytes) -> None:
        if self._f is None:
            raise ValueError("write to a closed MJPEGWriter")
        n = len(jpeg)
        if self._size_with(n) > MAX_AVI_BYTES:
            raise ValueError(f"frame {len(self._index)} would take the file past 1 GiB ({self._size_with(n)} bytes): a plain AVI ends at 2 GiB and "
                             "OpenDML is not written -- split the clip or lower the quality")
        self._f.write(b"00dc" + struct.pack("<I", n))
        self._f.write(jpeg)
        if n & 1:
            self._f.write(b"\0")  # chunks start on even offsets
        self._index.append((self._movi, n))
        self._movi += 8 + n + (n & 1)
        self._max = max(self._max, n)

    def close(self) -> None:
        if self._f is None:
            return
        f, self._f = self._f, None
        try:
            f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
            f.write(b"".join(b"00dc" + struct.pack("<III", 0x10, off, n) for off, n in self._index))  # 0x10 = AVIIF_KEYFRAME
            f.seek(0)
            f.write(self._headers())
        finally:
            f.close()

    @property
    def frames(self) -> int:
        return len(self._index)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
