"""The PNG law of include/a3d.h ("PNG") in numpy: what a3d_png_scan / a3d_png_emit / a3d_png_pack and articulation3d_amd/png.py must
produce byte for byte.  tests/test_png_host.py holds this file to zlib's inflate and to PIL; tests/test_gpu_png.py holds the kernels to
this file.  The stages are exposed one by one: filter_frame, candidates, tokens, histogram, code_segment, encode_frame.

Everything about pixels, tokens and bits is stated here on its own; the frame's Huffman code and its block header come from the host
half of the encoder itself (png.huffman_lengths / png.dynamic_header), which is pure Python and which the host tests hold to zlib
directly.  The Adler-32 and the CRCs are zlib's own, so png.adler_fold is checked against them, not against itself.
"""
import struct
import zlib

import numpy as np

from articulation3d_amd import png as P

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
MAX_W, SEG_BYTES = 5461, 8192


def geometry(H, W):
    """(stride, rows per segment, segments per frame, [(first byte, bytes) of every segment])."""
    assert 1 <= H <= 65535 and 1 <= W <= MAX_W
    stride = 1 + 3 * W
    R = max(1, -(-SEG_BYTES // stride))
    S = -(-H // R)
    return stride, R, S, [(s * R * stride, min(R, H - s * R) * stride) for s in range(S)]


def slot_bytes(W):
    stride, R, _, _ = geometry(1, W)
    return (R * stride + 5 + 15) // 16 * 16


def length_symbol(L):
    """(symbol - 257, extra bits, extra value) of a match length 3 .. 258."""
    s = max(k for k in range(29) if LEN_BASE[k] <= L) if L < 258 else 28
    return s, LEN_EXTRA[s], L - LEN_BASE[s]


def distance_symbol(d):
    s = max(k for k in range(30) if DIST_BASE[k] <= d)
    return s, DIST_EXTRA[s], d - DIST_BASE[s]


def fixed_lengths():
    return [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30  # 288 literal / length codes (286, 287 never occur), 30 distance codes


# ---- filtering ---------------------------------------------------------------------------------------------------------------------
def filter_frame(img):
    """uint8 [H,W,3] -> (types [H], filtered bytes [H * stride])."""
    H, W, _ = img.shape
    x = img.reshape(H, 3 * W).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255  # [5,H,3W]
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)               # [5,H]
    types = np.argmin(cost, axis=0)                                          # the first minimum: the lowest type
    rows = cand[types, np.arange(H)]
    filt = np.concatenate([types[:, None], rows], axis=1).astype(np.uint8)
    return types.astype(np.uint8), filt.reshape(-1)


def unfilter(filt, H, W):
    """The inverse, row by row (the standard's reconstruction): for the tests."""
    stride = 1 + 3 * W
    out = np.zeros((H, 3 * W), np.int32)
    prev = np.zeros(3 * W, np.int32)
    for y in range(H):
        t, row = int(filt[y * stride]), filt[y * stride + 1:(y + 1) * stride].astype(np.int32)
        cur = np.zeros(3 * W, np.int32)
        if t in (0, 2):
            cur = (row + (prev if t == 2 else 0)) & 255
        else:
            for i in range(3 * W):
                a = cur[i - 3] if i >= 3 else 0
                b = prev[i]
                c = prev[i - 3] if i >= 3 else 0
                if t == 1:
                    pred = a
                elif t == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[i] = (row[i] + pred) & 255
        out[y] = prev = cur
    return out.astype(np.uint8).reshape(H, W, 3)


# ---- tokens ------------------------------------------------------------------------------------------------------------------------
def candidates(filt, H, W):
    """Per byte of the frame: (L, d) of the winning candidate, L capped at 258 and at its segment's end (L < 3: a literal)."""
    stride, _, _, segs = geometry(H, W)
    N = filt.size
    idx = np.arange(N)
    seg_end = np.empty(N, np.int64)
    for a, n in segs:
        seg_end[a:a + n] = a + n
    dists = (1, 3, stride)
    runs = []
    for d in dists:
        eq = np.zeros(N, bool)
        eq[d:] = filt[d:] == filt[:-d]
        fail = np.where(eq, N, idx)                                    # index of a failure, N where the bytes agree
        first_fail = np.minimum.accumulate(fail[::-1])[::-1]           # the first failure at or after g
        runs.append(np.minimum(np.minimum(first_fail - idx, 258), seg_end - idx))
    runs = np.stack(runs)
    sel = np.argmax(runs, axis=0)                                      # the first maximum: the smallest distance
    return runs[sel, idx], np.array(dists)[sel]


def tokens(filt, H, W):
    """Per segment the greedy parse: a list of (byte within the segment, L, d); L = 1, d = 0 is a literal."""
    L, D = candidates(filt, H, W)
    L, D = L.tolist(), D.tolist()
    out = []
    for a, n in geometry(H, W)[3]:
        toks, i = [], 0
        while i < n:
            if L[a + i] >= 3:
                toks.append((i, L[a + i], D[a + i]))
                i += L[a + i]
            else:
                toks.append((i, 1, 0))
                i += 1
        out.append(toks)
    return out


def histogram(filt, H, W, seg_tokens):
    hist = np.zeros(316, np.int64)
    for (a, _n), toks in zip(geometry(H, W)[3], seg_tokens):
        for i, L, d in toks:
            if d == 0:
                hist[filt[a + i]] += 1
            else:
                hist[257 + length_symbol(L)[0]] += 1
                hist[286 + distance_symbol(d)[0]] += 1
        hist[256] += 1
    return hist


# ---- coding ------------------------------------------------------------------------------------------------------------------------
def _huffman_body(fseg, toks, litlen, dist, bits):
    """Appends the tokens and the end of block in the code (litlen, dist lengths) to `bits`."""
    lcode, dcode = P.canonical_codes(litlen), P.canonical_codes(dist)
    for i, L, d in toks:
        if d == 0:
            v = int(fseg[i])
            bits.put_code(lcode[v], litlen[v])
        else:
            s, nx, x = length_symbol(L)
            bits.put_code(lcode[257 + s], litlen[257 + s])
            bits.put(x, nx)
            s, nx, x = distance_symbol(d)
            bits.put_code(dcode[s], dist[s])
            bits.put(x, nx)
    bits.put_code(lcode[256], litlen[256])


def _finish(bits):
    """The empty stored block behind a Huffman block: 000, zeros to a byte boundary, 00 00 FF FF."""
    bits.put(0, 3)
    nbytes = (bits.n + 7) // 8
    return bits.value.to_bytes(nbytes, "little") + b"\x00\x00\xff\xff"


def code_segment(fseg, toks, litlen, dist):
    """One segment -> (kind, bytes): the cheapest of stored, fixed and dynamic; ties go to the lowest number."""
    n = len(fseg)
    stored = b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + bytes(fseg)
    fl, fd = fixed_lengths()
    b1 = P._Bits()
    b1.put(0, 1)
    b1.put(1, 2)
    _huffman_body(fseg, toks, fl, fd, b1)
    b2 = P._Bits()
    b2.put(*P.dynamic_header(litlen, dist))
    _huffman_body(fseg, toks, litlen, dist, b2)
    options = [stored, _finish(b1), _finish(b2)]
    kind = min(range(3), key=lambda k: (len(options[k]), k))
    return kind, options[kind]


def encode_stages(img):
    """Every stage of one frame: a dict with types, filt, tokens, hist, litlen, dist, kinds, segments (bytes each), deflate, file."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W, _ = img.shape
    types, filt = filter_frame(img)
    toks = tokens(filt, H, W)
    hist = histogram(filt, H, W, toks)
    litlen, dist = P.frame_code(hist)
    coded = [code_segment(filt[a:a + n], t, litlen, dist) for (a, n), t in zip(geometry(H, W)[3], toks)]
    deflate = b"".join(c for _k, c in coded)
    idat = b"\x78\x01" + deflate + b"\x03\x00" + struct.pack(">I", zlib.adler32(filt.tobytes()))

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))

    file = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")
    return dict(types=types, filt=filt, tokens=toks, hist=hist, litlen=litlen, dist=dist, kinds=[k for k, _c in coded],
                segments=[c for _k, c in coded], deflate=deflate, file=file)


def encode_frame(img):
    return encode_stages(img)["file"]


def chunks(png):
    """[(type, data, crc ok)] of a PNG file."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(png):
        n, kind = struct.unpack(">I4s", png[at:at + 8])
        data = png[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", png[at + 8 + n:at + 12 + n])
        out.append((kind, data, crc == zlib.crc32(kind + data)))
        at += 12 + n
    return out


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def flat(H, W, colour=(200, 30, 30)):
    return np.broadcast_to(np.array(colour, np.uint8), (H, W, 3)).copy()


def hramp(H, W):
    x = (np.arange(W) * 5 % 256).astype(np.uint8)
    return np.broadcast_to(np.stack([x, x // 2, 255 - x], axis=1)[None], (H, W, 3)).copy()


def vramp(H, W):
    y = (np.arange(H) * 3 % 256).astype(np.uint8)
    return np.broadcast_to(np.stack([y, 255 - y, y // 3], axis=1)[:, None], (H, W, 3)).copy()


def repeated_rows(H, W, seed=5):
    return np.broadcast_to(noise(1, W, seed), (H, W, 3)).copy()


def period3(H, W, seed=6):
    """A 3-pixel-period pattern along each row, another phase every row."""
    base = noise(1, 3, seed)[0]
    x = np.arange(W)[None, :] + np.arange(H)[:, None]
    return base[x % 3]


def camera(H, W, seed=7):
    """Smooth content plus sigma = 3 noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    smooth = np.stack([128 + 90 * np.sin(x / 37.0 + y / 53.0), 128 + 80 * np.cos(x / 29.0 - y / 41.0), 100 + 0.4 * x + 0.3 * y], axis=2)
    return np.clip(np.rint(smooth + rng.normal(0, 3, (H, W, 3))), 0, 255).astype(np.uint8)


def mixed(H, W, seed=8):
    """Bands of every kind of content in one frame: all filters, codings and distances in a few segments."""
    parts = [flat, hramp, vramp, repeated_rows, period3, camera]
    edges = np.linspace(0, H, len(parts) + 2).astype(int)
    out = noise(H, W, seed)
    for k, fn in enumerate(parts):
        lo, hi = edges[k], edges[k + 1]
        if hi > lo:
            out[lo:hi] = fn(hi - lo, W)
    return out
