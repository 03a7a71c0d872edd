"""The clip's visualisation as a video: Motion-JPEG in an AVI container, the frames encoded on the GPU (a3d_jpeg_encode /
a3d_jpeg_pack, csrc/jpeg.hip; the law is stated in include/a3d.h and, in numpy, in tests/mjpeg_ref.py).

The reference ends in an H.264 output.mp4 written by imageio; H.264 needs an encoder this package does not have, Motion-JPEG needs
none.  Every frame is a baseline JFIF image (8-bit, Y / Cb / Cr at 4:4:4 so that one-pixel outlines stay sharp, Annex K tables) with
a restart interval of one MCU row, which makes every MCU row an independent piece of work for the device.  The host writes the
headers (once per size and quality) and the container; only the compressed bytes cross PCIe.

    jpeg_encode(frames_u8, quality)                      -> list[bytes], complete JFIF files
    render_clip_jpeg(frames_u8, preds_raw, preds_opt)    -> yields list[bytes] per chunk: render_clip's rows, encoded
    MJPEGWriter(path, width, height, fps)                -> .write(jpeg), .close(); a context manager

and the way back, for clips and JPEG frames as input (a3d_jpeg_decode, csrc/jpeg_decode.hip; the law in include/a3d.h and
tests/jpeg_decode_ref.py): baseline JPEG, grey or 4:4:4 / 4:2:2 / 4:2:0, any tables, any restart interval, decoded on the GPU to the
bytes libjpeg's default decoder gives.

    jpeg_parse(data)                                     -> JPEGInfo (pure Python); ValueError for what the decoder's law leaves out
    jpeg_decode(jpegs, device, chunk, strict)            -> uint8 [F,H,W,3] RGB on the device; a restart interval, or a whole scan
                                                            without them, is decoded by many lanes at once
    MJPEGReader(path)                                    -> .width, .height, .fps, len(), reader[i], reader[a:b]; a context manager

The container is a plain RIFF `AVI ` file (hdrl: avih + one strl of type vids / MJPG with a BITMAPINFOHEADER; a movi list of 00dc
chunks; idx1), which ends at 2 GiB: the writer refuses a clip that would pass 1 GiB.  OpenDML is not written.
"""
from __future__ import annotations

import dataclasses
import functools
import re
import struct
from fractions import Fraction
from typing import Iterator, List, Sequence

import numpy as np
import torch

from . import _lib, opt_ops

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_UNZIG = tuple(ZIGZAG.index(n) for n in range(64))  # place in zigzag order of the coefficient at natural index n
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


# ---------------------------------------------------------------------------------------------------------------------
# reading: baseline JPEG files and Motion-JPEG clips, decoded on the GPU (a3d_jpeg_decode, csrc/jpeg_decode.hip; the law is stated
# in include/a3d.h and, in numpy, in tests/jpeg_decode_ref.py)
# ---------------------------------------------------------------------------------------------------------------------
_NOT_DATA = re.compile(b"\xff[^\x00\xd0-\xd7]")  # in entropy-coded data FF is followed by 00 or, as a restart marker, by D0 .. D7
_RST = re.compile(b"\xff[\xd0-\xd7]")
JPEG_SPLIT_BYTES = _lib.JPEG_SPLIT_BYTES  # bytes of a subsequence of jpeg_decode by default: a3d_jpeg_decode's own (include/a3d.h)
JPEG_STATUS = {_lib.JPEG_RANGE: "RANGE", _lib.JPEG_BAD_CODE: "BAD_CODE", _lib.JPEG_SHORT: "SHORT"}


@dataclasses.dataclass(frozen=True)
class JPEGInfo:
    """What jpeg_parse learns from a file's headers.  quant: per component 64 bytes in natural order; huff: per component (DC bits[16],
    DC vals, AC bits[16], AC vals); restart: MCUs per restart interval, 0 = none; scan: the byte range of the entropy-coded data;
    units: the byte range of every unit (a restart interval, or the whole scan), markers excluded."""
    height: int
    width: int
    ncomp: int
    hs: int
    vs: int
    quant: tuple
    huff: tuple
    restart: int
    scan: tuple
    units: tuple

    @property
    def geometry(self):
        return self.height, self.width, self.ncomp, self.hs, self.vs

    @property
    def mcus(self) -> int:
        return -(-self.width // (8 * self.hs)) * -(-self.height // (8 * self.vs))

    @property
    def n_units(self) -> int:
        """Units the geometry asks for (a damaged stream may hold fewer or more)."""
        return -(-self.mcus // self.restart) if self.restart else 1

    def table_set(self) -> bytes:
        """One table set of a3d_jpeg_decode: _lib.JPEG_TABSET_BYTES bytes."""
        out = b"".join(self.quant) + bytes(64 * (3 - self.ncomp))
        for dc_bits, dc_vals, ac_bits, ac_vals in self.huff:
            out += dc_bits + dc_vals.ljust(256, b"\0") + ac_bits + ac_vals.ljust(256, b"\0")
        return out.ljust(_lib.JPEG_TABSET_BYTES, b"\0")


@functools.lru_cache(maxsize=1)
def _annex_k():
    bits, vals = opt_ops.jpeg_tables()
    n = _lib.JPEG_HUFF_VALS
    return {key: (bits[16 * t:16 * t + 16], vals[n * t:n * t + sum(bits[16 * t:16 * t + 16])])
            for t, key in enumerate(((0, 0), (1, 0), (0, 1), (1, 1)))}  # (class, id): DC0, AC0, DC1, AC1


def jpeg_parse(data: bytes) -> JPEGInfo:
    """The headers of one JPEG file.  Pure Python, one pass over the marker segments and one search over the scan.  Raises ValueError,
    naming the cause, for everything a3d_jpeg_decode's law leaves out: progressive (SOF2), arithmetic coding, 12-bit, 16-bit
    quantisation tables, sampling factors other than 4:4:4 / 4:2:2 / 4:2:0, more than one scan, 2 or 4 components, H or W outside
    1 .. 65535, a missing SOI, SOF or SOS.  A file without any DHT segment gets the Annex K tables (the AVI "MJPG" convention)."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file: it does not start with SOI")
    quant, huff, sof, restart, sos, adobe = {}, {}, None, 0, None, None
    at, n_data = 2, len(data)
    while at + 4 <= n_data:
        if data[at] != 0xFF:
            raise ValueError(f"byte {at}: expected a marker")
        m = data[at + 1]
        if m == 0xFF:  # fill byte
            at += 1
            continue
        if m == 0xD9:
            break
        size = (data[at + 2] << 8) | data[at + 3]
        body = data[at + 4:at + 2 + size]
        at += 2 + size
        if m == 0xDB:
            while body:
                if body[0] >> 4:
                    raise ValueError("16-bit quantisation table")
                if len(body) < 65:
                    raise ValueError("DQT segment cut short")
                quant[body[0] & 15] = bytes(body[1 + z] for z in _UNZIG)  # zigzag in the file, natural order here
                body = body[65:]
        elif m == 0xC4:
            while body:
                if len(body) < 17 or len(body) < 17 + sum(body[1:17]) or sum(body[1:17]) > 256:
                    raise ValueError("DHT segment cut short")
                n = sum(body[1:17])
                huff[(body[0] >> 4, body[0] & 15)] = (body[1:17], body[17:17 + n])
                body = body[17 + n:]
        elif m == 0xDD:
            restart = int.from_bytes(body[:2], "big")
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xC0:
            if sof is not None:
                raise ValueError("more than one frame header")
            sof = body
        elif m == 0xC2:
            raise ValueError("progressive JPEG (SOF2)")
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise ValueError(f"SOF{m - 0xC0}: arithmetic coding" if m >= 0xC9 else f"SOF{m - 0xC0}: not baseline (12-bit, lossless or hierarchical)")
        elif m == 0xDA:
            if sof is None:
                raise ValueError("no SOF marker in front of SOS")
            sos = (body, at)
            break
    if sof is None:
        raise ValueError("no SOF marker")
    if sos is None:
        raise ValueError("no SOS marker")
    if len(sof) < 6 or len(sof) < 6 + 3 * sof[5]:
        raise ValueError("SOF segment cut short")
    precision, height, width, ncomp = sof[0], (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4], sof[5]
    if precision != 8:
        raise ValueError(f"{precision}-bit samples")
    if ncomp not in (1, 3):
        raise ValueError(f"{ncomp} components: grey or Y / Cb / Cr only")
    if not (1 <= height <= 65535 and 1 <= width <= 65535):
        raise ValueError(f"{height} x {width}: a JPEG is 1 .. 65535 pixels a side")
    if ncomp == 3 and adobe == 0:
        raise ValueError("Adobe transform 0: RGB, not Y / Cb / Cr")
    body, lo = sos
    if not body or body[0] != ncomp or len(body) < 4 + 2 * ncomp:
        raise ValueError("more than one scan (the first one does not hold every component)")
    selectors = {body[1 + 2 * i]: body[2 + 2 * i] for i in range(ncomp)}
    if tuple(body[1 + 2 * ncomp:4 + 2 * ncomp]) != (0, 63, 0):
        raise ValueError("not a sequential scan")
    sampling, q_out, h_out = [], [], []
    for i in range(ncomp):
        cid, hv, tq = sof[6 + 3 * i:9 + 3 * i]
        if cid not in selectors:
            raise ValueError("more than one scan (the first one does not hold every component)")
        if tq not in quant:
            raise ValueError(f"quantisation table {tq} is missing")
        tabs = ()
        for cls, tid in ((0, selectors[cid] >> 4), (1, selectors[cid] & 15)):
            if (cls, tid) in huff:
                tabs += huff[(cls, tid)]
            elif not huff and tid < 2:
                tabs += _annex_k()[(cls, tid)]
            else:
                raise ValueError(f"Huffman table {cls}/{tid} is missing")
        sampling.append((hv >> 4, hv & 15))
        q_out.append(quant[tq])
        h_out.append(tabs)
    if ncomp == 1:
        sampling = [(1, 1)]  # a scan of one component is never interleaved: its MCU is one block
    elif sampling[1:] != [(1, 1), (1, 1)] or sampling[0] not in ((1, 1), (2, 1), (2, 2)):
        raise ValueError("sampling factors " + ", ".join(f"{h}x{v}" for h, v in sampling) + ": 4:4:4, 4:2:2 and 4:2:0 only")
    end = _NOT_DATA.search(data, lo)
    hi = end.start() if end else n_data
    if end and data[hi + 1] != 0xD9 and data.find(b"\xff\xda", hi) >= 0:
        raise ValueError("more than one scan")
    units, start = [], lo
    if restart:
        for m in _RST.finditer(data, lo, hi):
            units.append((start, m.start()))
            start = m.end()
    units.append((start, hi))
    return JPEGInfo(height, width, ncomp, sampling[0][0], sampling[0][1], tuple(q_out), tuple(h_out), restart, (lo, hi), tuple(units))


def jpeg_decode(jpegs: Sequence[bytes], device="cuda", chunk: int = 8, strict: bool = True, split_bytes: int = None):
    """F baseline JPEG files of one size and one sampling -> uint8 [F,H,W,3] RGB on the device, byte for byte what libjpeg's
    default decoder returns (include/a3d.h states the law).  The host parses the headers and uploads the entropy-coded bytes and one table set per
    distinct set of tables of the call; `chunk` frames are decoded per a3d_jpeg_decode call, and the host prepares a chunk while the
    device decodes the one before.  A frame's pixels do not depend on the frames beside it or on `chunk`.  With `strict` a frame
    whose status is not 0 raises ValueError with its index and the code (SHORT, BAD_CODE, RANGE); without, -> (frames, status
    int32 [F] on the host).  A unit (a restart interval, the whole scan without them) is cut into subsequences of `split_bytes`
    (None: JPEG_SPLIT_BYTES, the library's default) that synchronise themselves; bytes and status do not depend on the size."""
    split = None if split_bytes is None else int(split_bytes)
    if split is not None and split < 1:
        raise ValueError(f"split_bytes {split_bytes!r}: at least 1")
    infos = []
    for i, j in enumerate(jpegs):
        try:
            infos.append(jpeg_parse(j))
        except ValueError as e:
            raise ValueError(f"frame {i}: {e}") from None
    if not infos:
        raise ValueError("jpeg_decode: no frames")
    for i, info in enumerate(infos):
        if info.geometry != infos[0].geometry:
            raise ValueError(f"frame {i} is {info.geometry} (H, W, components, luma sampling), frame 0 is {infos[0].geometry}: one call decodes one geometry")
    H, W, ncomp, hs, vs = infos[0].geometry
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"device {device!r}: the decoder runs on the GPU")
    F = len(infos)
    chunk = max(1, min(int(chunk), F))
    set_index, set_of = {}, []
    for info in infos:
        set_of.append(set_index.setdefault(info.table_set(), len(set_index)))
    sets = np.frombuffer(b"".join(set_index), np.uint8).reshape(len(set_index), _lib.JPEG_TABSET_BYTES)
    ce, pe = opt_ops.jpeg_decode_scratch(H, W, ncomp, hs, vs)
    with torch.cuda.device(dev):
        sets_dev = torch.from_numpy(sets.copy()).to(dev)
        coef = torch.empty(chunk * ce, dtype=torch.int16, device=dev)
        planes = torch.empty(chunk * pe, dtype=torch.uint8, device=dev)
        out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        status = torch.empty(F, dtype=torch.int32, device=dev)
        for lo in range(0, F, chunk):
            hi = min(lo + chunk, F)
            pieces, unit_off, frame_unit = [], [0], [0]
            for k in range(lo, hi):
                info, data = infos[k], jpegs[k]
                ranges = (list(info.units) + [(0, 0)] * info.n_units)[:info.n_units]  # a damaged stream: empty units for the missing ones
                for a, b in ranges:
                    pieces.append(data[a:b])
                    unit_off.append(unit_off[-1] + b - a)
                frame_unit.append(len(unit_off) - 1)
            total = unit_off[-1]
            if total > 0x7FFFFFFF:
                raise ValueError(f"frames {lo} .. {hi - 1} hold {total} bytes: more than one call takes, pass a smaller chunk")
            blob = np.frombuffer(b"".join(pieces) + bytes(-total % 4 + 4), np.uint8)
            meta = np.array(unit_off + frame_unit + [i.restart for i in infos[lo:hi]] + set_of[lo:hi], np.int32)
            opt_ops.jpeg_decode_into(out[lo:hi], status[lo:hi], torch.from_numpy(blob.copy()).to(dev), total, meta, torch.from_numpy(meta).to(dev), sets,
                                     sets_dev, len(unit_off) - 1, ncomp, hs, vs, coef, planes, split)
        st = status.cpu()
    if not strict:
        return out, st
    bad = torch.nonzero(st).flatten().tolist()
    if bad:
        raise ValueError(f"frame {bad[0]}: status {JPEG_STATUS.get(int(st[bad[0]]), int(st[bad[0]]))}" +
                         (f" (and {len(bad) - 1} more frames)" if len(bad) > 1 else ""))
    return out


class MJPEGReader:
    """The frames of a Motion-JPEG RIFF `AVI ` file, as bytes: reader[i], reader[a:b], len(reader), iteration; .width, .height, .fps (a
    Fraction, dwRate / dwScale of the stream header).  Opening reads hdrl and idx1 (or, without an index, the eight-byte headers of
    the movi list); a frame's bytes are read when it is asked for.  The first stream must be video with the handler MJPG; OpenDML
    files (a second RIFF chunk of type AVIX) are refused, as the writer refuses to write them."""

    def __init__(self, path):
        self._f = open(path, "rb")
        try:
            self._open()
        except Exception:
            self._f.close()
            raise

    def _open(self):
        f = self._f
        size = f.seek(0, 2)
        f.seek(0)
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            raise ValueError("not a RIFF AVI file")
        riff_end = min(8 + struct.unpack("<I", head[4:8])[0], size)
        if riff_end + 12 <= size:
            f.seek(riff_end + (riff_end & 1))
            more = f.read(12)
            if more[:4] == b"RIFF" and more[8:12] == b"AVIX":
                raise ValueError("OpenDML AVI (an AVIX chunk follows the first RIFF chunk): not read")
        hdrl = movi = idx1 = None
        at = 12
        while at + 8 <= riff_end:
            f.seek(at)
            cc, n = struct.unpack("<4sI", f.read(8))
            if cc == b"LIST":
                kind = f.read(4)
                if kind == b"hdrl":
                    hdrl = f.read(n - 4)
                elif kind == b"movi":
                    movi = (at + 8, n)  # offset of the 'movi' fourcc, bytes from there
            elif cc == b"idx1":
                idx1 = f.read(n)
            at += 8 + n + (n & 1)
        if hdrl is None or movi is None:
            raise ValueError("AVI file without a hdrl or a movi list")
        self._parse_hdrl(hdrl)
        self._frames = self._from_index(idx1, movi) if idx1 else None
        if self._frames is None:
            self._frames = self._walk(movi[0] + 4, min(movi[0] + movi[1], size))

    def _parse_hdrl(self, hdrl: bytes):
        at, strh, strf, avih = 0, None, None, None
        while at + 8 <= len(hdrl):
            cc, n = struct.unpack_from("<4sI", hdrl, at)
            if cc == b"avih":
                avih = struct.unpack_from("<14I", hdrl, at + 8)
            elif cc == b"LIST" and hdrl[at + 8:at + 12] == b"strl" and strh is None:  # the first stream
                sub, end = at + 12, at + 8 + n
                while sub + 8 <= end:
                    scc, sn = struct.unpack_from("<4sI", hdrl, sub)
                    if scc == b"strh":
                        strh = hdrl[sub + 8:sub + 8 + sn]
                    elif scc == b"strf":
                        strf = hdrl[sub + 8:sub + 8 + sn]
                    sub += 8 + sn + (sn & 1)
            at += 8 + n + (n & 1)
        if avih is None or strh is None or len(strh) < 36 or strf is None or len(strf) < 20:
            raise ValueError("AVI file without avih, strh or strf")
        if strh[:4] != b"vids":
            raise ValueError(f"the first stream is {strh[:4]!r}, not video")
        handler, compression = strh[4:8], strf[16:20]
        if handler.upper() != b"MJPG" or compression.upper() != b"MJPG":
            raise ValueError(f"stream handler {handler!r} / compression {compression!r}: only MJPG (Motion-JPEG) is read")
        scale, rate = struct.unpack_from("<II", strh, 20)
        if not scale or not rate:
            raise ValueError("stream header without a frame rate")
        self.fps = Fraction(rate, scale)
        self.width, self.height = struct.unpack_from("<ii", strf, 4)
        self.height = abs(self.height)

    def _from_index(self, idx1: bytes, movi):
        """idx1 entries of the first stream -> [(offset of the data, length)].  Offsets count from the 'movi' fourcc (the format) or from
        the start of the file (some writers): whichever makes the first entry point at its chunk header.  None if neither does."""
        entries = [struct.unpack_from("<4sIII", idx1, 16 * i) for i in range(len(idx1) // 16)]
        entries = [(off, n) for cc, _flags, off, n in entries if cc in (b"00dc", b"00db")]
        if not entries:
            return []
        for base in (movi[0], 0):
            self._f.seek(base + entries[0][0])
            if self._f.read(8) == b"00dc" + struct.pack("<I", entries[0][1]):
                return [(base + off + 8, n) for off, n in entries]
        return None

    def _walk(self, lo: int, hi: int):
        out, at = [], lo
        while at + 8 <= hi:
            self._f.seek(at)
            cc, n = struct.unpack("<4sI", self._f.read(8))
            if cc == b"LIST":  # 'rec ' groups: step inside
                at += 12
                continue
            if cc in (b"00dc", b"00db"):
                out.append((at + 8, n))
            at += 8 + n + (n & 1)
        return out

    def __len__(self) -> int:
        return len(self._frames)

    def _read(self, k: int) -> bytes:
        off, n = self._frames[k]
        self._f.seek(off)
        return self._f.read(n)

    def __getitem__(self, key):
        if self._f is None:
            raise ValueError("read from a closed MJPEGReader")
        if isinstance(key, slice):
            return [self._read(k) for k in range(*key.indices(len(self)))]
        k = key + len(self) if key < 0 else key
        if not 0 <= k < len(self):
            raise IndexError(key)
        return self._read(k)

    def __iter__(self):
        return (self[k] for k in range(len(self)))

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
