"""The PNG decoding law of include/a3d.h ("PNG decode") in plain Python / numpy: what a3d_png_decode and articulation3d_amd/png.py's
png_decode must produce byte for byte, status included.  tests/test_png_decode_host.py holds this file to zlib's inflate and to PIL;
tests/test_gpu_png_decode.py holds the kernels to this file.  The stages are exposed one by one: inflate, unfilter, to_rgb, decode.

Every index this file forms is asserted to lie inside its buffer (_Stream.bits, _Out): the walk below is the proof that the law's
checks (SHORT, FAR, LONG) are enough to keep a decoder inside the buffers of the call whatever the stream holds.
"""
import zlib

import numpy as np

from articulation3d_amd import png as P

SHORT, BAD_CODE, FAR, LONG, FILTER, ADLER = 1, 2, 3, 4, 5, 6
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _Stream:
    """The deflate body as a string of bits, LSB first.  Nothing is readable past its last bit."""

    def __init__(self, data: bytes):
        self.data, self.pos, self.n = data, 0, 8 * len(data)

    def bits(self, k: int) -> int:
        if self.pos + k > self.n:
            raise _Stop(SHORT)
        assert 0 <= self.pos and self.pos + k <= self.n  # every bit taken lies inside the stream
        at = self.pos >> 3  # k <= 16: four bytes hold the field; a slice stops at the data's end
        v = (int.from_bytes(self.data[at:at + 4], "little") >> (self.pos & 7)) & ((1 << k) - 1)
        self.pos += k
        return v

    def symbol(self, code):
        """One symbol of a canonical code, a bit at a time: SHORT when the bits run out before a code is complete; BAD_CODE once as
        many bits as the longest code has (at least one) match none: only an incomplete set has such patterns."""
        counts, symbols = code
        top = max([l for l in range(1, 16) if counts[l]] + [1])
        v = first = index = 0
        for l in range(1, top + 1):
            v |= self.bits(1)
            if v - first < counts[l]:
                return symbols[index + v - first]
            index += counts[l]
            first = (first + counts[l]) << 1
            v <<= 1
        raise _Stop(BAD_CODE)


def code_of(lengths):
    """(counts per length, symbols sorted by (length, symbol)) of a set of code lengths, or None if the set is illegal by zlib's rule:
    over-subscribed, or incomplete with a code longer than one bit (one code of one bit, or none at all, is let through)."""
    counts = [0] * 16
    for l in lengths:
        counts[l] += 1
    counts[0] = 0
    left = 1
    for l in range(1, 16):
        left = 2 * left - counts[l]
        if left < 0:
            return None
    if left > 0 and any(counts[2:]):
        return None
    return counts, [s for l in range(1, 16) for s, ls in enumerate(lengths) if ls == l]


FIXED = (code_of([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), code_of([5] * 32))


class _Out:
    def __init__(self, size: int):
        self.buf, self.n, self.size = np.zeros(size, np.uint8), 0, size

    def put(self, b: int):
        if self.n >= self.size:
            raise _Stop(LONG)
        assert 0 <= self.n < self.buf.size
        self.buf[self.n] = b
        self.n += 1


def _dynamic(s: _Stream):
    hlit, hdist, hclen = s.bits(5) + 257, s.bits(5) + 1, s.bits(4) + 4
    if hlit > 286 or hdist > 30:
        raise _Stop(BAD_CODE)
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = s.bits(3)
    cl_code = code_of(cl)
    if cl_code is None or _incomplete(cl_code[0]):  # the code-length code must be complete: no exception for short sets here
        raise _Stop(BAD_CODE)
    lengths = []
    while len(lengths) < hlit + hdist:
        sym = s.symbol(cl_code)
        if sym < 16:
            lengths.append(sym)
            continue
        rep = s.bits((2, 3, 7)[sym - 16]) + (3, 3, 11)[sym - 16]
        if sym == 16 and not lengths:
            raise _Stop(BAD_CODE)
        if len(lengths) + rep > hlit + hdist:
            raise _Stop(BAD_CODE)
        lengths += [lengths[-1] if sym == 16 else 0] * rep
    if lengths[256] == 0:
        raise _Stop(BAD_CODE)
    lit, dist = code_of(lengths[:hlit]), code_of(lengths[hlit:])
    if lit is None or dist is None:
        raise _Stop(BAD_CODE)
    return lit, dist


def _incomplete(counts) -> bool:
    left = 1
    for l in range(1, 16):
        left = 2 * left - counts[l]
    return left > 0


def inflate(body: bytes, raw_size: int):
    """The deflate body of a frame (the zlib stream without its two header bytes, Adler-32 included) -> (raw uint8 [raw_size], status of
    the walk, the four bytes behind the final block as an integer or None).  The bytes of `raw` a flagged walk did not reach are 0."""
    s, out = _Stream(body), _Out(raw_size)
    try:
        final = 0
        while not final:
            final, btype = s.bits(1), s.bits(2)
            if btype == 3:
                raise _Stop(BAD_CODE)
            if btype == 0:
                s.bits(-s.pos % 8)
                n, inv = s.bits(16), s.bits(16)
                if n != inv ^ 0xFFFF:
                    raise _Stop(BAD_CODE)
                at, have = s.pos >> 3, len(body) - (s.pos >> 3)
                if out.n + min(n, have) > raw_size:
                    raise _Stop(LONG)
                if have < n:
                    raise _Stop(SHORT)
                for k in range(n):
                    assert 0 <= at + k < len(body)
                    out.put(body[at + k])
                s.pos += 8 * n
                continue
            lit, dist = FIXED if btype == 1 else _dynamic(s)
            while True:
                sym = s.symbol(lit)
                if sym < 256:
                    out.put(sym)
                elif sym == 256:
                    break
                elif sym >= 286:
                    raise _Stop(BAD_CODE)
                else:
                    length = LEN_BASE[sym - 257] + s.bits(LEN_EXTRA[sym - 257])
                    ds = s.symbol(dist)
                    if ds >= 30:
                        raise _Stop(BAD_CODE)
                    d = DIST_BASE[ds] + s.bits(DIST_EXTRA[ds])
                    if d > out.n:
                        raise _Stop(FAR)
                    if out.n + length > raw_size:
                        raise _Stop(LONG)
                    p = out.n
                    for k in range(length):
                        src = p - d + (k % d if d < length else k)
                        assert 0 <= src < p
                        out.put(int(out.buf[src]))
        if out.n < raw_size:
            raise _Stop(SHORT)
        s.bits(-s.pos % 8)
        if len(body) - (s.pos >> 3) < 4:
            raise _Stop(SHORT)
        return out.buf, 0, int.from_bytes(body[s.pos >> 3:(s.pos >> 3) + 4], "big")
    except _Stop as e:
        return out.buf, e.status, None


def unfilter(raw: np.ndarray, H: int, W: int, channels: int):
    """raw [H * (1 + W * channels)] -> (samples uint8 [H, W, channels], True if a filter byte is above 4: such a row counts as type 0)."""
    stride, bpp = 1 + W * channels, channels
    assert raw.size == H * stride
    out = np.zeros((H, W * channels), np.int32)
    prev, bad = np.zeros(W * channels, np.int32), False
    for y in range(H):
        t, row = int(raw[y * stride]), raw[y * stride + 1:(y + 1) * stride].astype(np.int32)
        if t > 4:
            bad, t = True, 0
        if t == 0:
            cur = row
        elif t == 2:
            cur = (row + prev) & 255
        else:
            cur = np.zeros(W * channels, np.int32)
            for i in range(W * channels):
                a = int(cur[i - bpp]) if i >= bpp else 0
                b = int(prev[i])
                c = int(prev[i - bpp]) if i >= bpp else 0
                if t == 1:
                    pred = a
                elif t == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[i] = (int(row[i]) + pred) & 255
        out[y] = prev = cur
    return out.astype(np.uint8).reshape(H, W, channels), bad


def to_rgb(samples: np.ndarray) -> np.ndarray:
    """[H,W,channels] -> [H,W,3]: grey replicated, alpha dropped."""
    ch = samples.shape[2]
    return np.repeat(samples[:, :, :1], 3, axis=2) if ch <= 2 else np.ascontiguousarray(samples[:, :, :3])


def decode_body(body: bytes, H: int, W: int, channels: int):
    """-> (rgb uint8 [H,W,3], status): the first thing that went wrong in stream order, then the filter bytes, then the checksum."""
    raw_size = H * (1 + W * channels)
    raw, status, stored = inflate(body, raw_size)
    samples, bad = unfilter(raw, H, W, channels)
    if status == 0 and bad:
        status = FILTER
    if status == 0 and stored != zlib.adler32(raw.tobytes()):
        status = ADLER
    return to_rgb(samples), status


def body_of(data: bytes, info=None) -> bytes:
    info = info or P.png_parse(data)
    return b"".join(data[a:b] for a, b in info.ranges)


def decode(data: bytes):
    """A PNG file that png_parse accepts -> (rgb uint8 [H,W,3], status)."""
    info = P.png_parse(data)
    return decode_body(body_of(data, info), *info.geometry)
