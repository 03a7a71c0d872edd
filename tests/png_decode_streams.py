"""The PNG files and deflate streams that tests/test_png_decode_host.py and tests/test_gpu_png_decode.py decode: PIL's and zlib's writers
at every setting, hand-filtered rows, the package's own encoder, and a small token-list writer for the streams zlib never emits.
Nothing here decodes: the host test holds tests/png_decode_ref.py to zlib and PIL on these, the GPU test holds the kernels to it."""
import io
import struct
import zlib

import numpy as np
from PIL import Image

import png_decode_ref as R
import png_ref
from articulation3d_amd import png as P

MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
COLOUR = {1: 0, 2: 4, 3: 2, 4: 6}


def image(H, W, ch, seed=0, kind="camera"):
    """uint8 [H,W,ch]: smooth content with noise (every filter pays somewhere), or plain noise."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 90 * np.sin(x / 7.0 + y / 5.0 + c) + 20 * c for c in range(ch)], axis=2)
    return np.clip(np.rint(base + rng.normal(0, 3, (H, W, ch))), 0, 255).astype(np.uint8)


def filter_rows(img, types):
    """uint8 [H,W,ch] and a filter type per row -> the raw bytes of the PNG's rows (the forward filters of the standard)."""
    H, W, ch = img.shape
    x = img.reshape(H, W * ch).astype(np.int32)
    a = np.zeros_like(x)
    a[:, ch:] = x[:, :-ch]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, ch:] = x[:-1, :-ch]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255
    types = np.asarray(types)
    rows = cand[types, np.arange(H)]
    return np.concatenate([types[:, None], rows], axis=1).astype(np.uint8).tobytes()


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def container(H, W, ch, idat_payloads, extra=(), depth=8, colour=None, interlace=0):
    """A PNG file round ready-made IDAT payloads; `extra` chunks go between IHDR and the first IDAT."""
    ihdr = struct.pack(">IIBBBBB", W, H, depth, COLOUR[ch] if colour is None else colour, 0, 0, interlace)
    return P.SIGNATURE + chunk(b"IHDR", ihdr) + b"".join(extra) + b"".join(chunk(b"IDAT", d) for d in idat_payloads) + chunk(b"IEND", b"")


def png_of_body(H, W, ch, body, header=b"\x78\x9c"):
    """A PNG file whose zlib stream is `header` + `body` (deflate blocks and the Adler-32, as the decoder takes them)."""
    return container(H, W, ch, [header + body])


def png_of_raw(H, W, ch, raw, deflate):
    return png_of_body(H, W, ch, deflate + struct.pack(">I", zlib.adler32(raw)))


def zlib_deflate(raw, level=6, wbits=15, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush=zlib.Z_SYNC_FLUSH):
    """Raw deflate by zlib.compressobj, optionally flushed in the middle."""
    c = zlib.compressobj(level, zlib.DEFLATED, -wbits, 9, strategy)
    out, at = [], 0
    for cut in flush_at:
        out += [c.compress(raw[at:cut]), c.flush(flush)]
        at = cut
    return b"".join(out) + c.compress(raw[at:]) + c.flush()


def pil_png(img, **kw):
    b = io.BytesIO()
    Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img, MODES[img.shape[2]]).save(b, "PNG", **kw)
    return b.getvalue()


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


# ---- the token-list writer -----------------------------------------------------------------------------------------------------------
class Bits(P._Bits):
    def align(self):
        self.put(0, -self.n % 8)

    def tobytes(self):
        return self.value.to_bytes((self.n + 7) // 8, "little")


def put_tokens(bits, tokens, litlen, dist):
    """Literals (ints) and copies ((length, distance)) in the code of these lengths, then the end of block."""
    lcode, dcode = P.canonical_codes(litlen), P.canonical_codes(dist)
    for t in tokens:
        if isinstance(t, int):
            assert litlen[t]
            bits.put_code(lcode[t], litlen[t])
        else:
            s, nx, x = png_ref.length_symbol(t[0])
            assert litlen[257 + s]
            bits.put_code(lcode[257 + s], litlen[257 + s])
            bits.put(x, nx)
            s, nx, x = png_ref.distance_symbol(t[1])
            assert dist[s]
            bits.put_code(dcode[s], dist[s])
            bits.put(x, nx)
    bits.put_code(lcode[256], litlen[256])


def write_blocks(blocks):
    """[("stored", bytes) | ("fixed", tokens) | ("dynamic", tokens, litlen, dist)] -> deflate bytes; the last block is final."""
    bits = Bits()
    for k, blk in enumerate(blocks):
        final = int(k == len(blocks) - 1)
        if blk[0] == "stored":
            bits.put(final, 1)
            bits.put(0, 2)
            bits.align()
            bits.put(len(blk[1]), 16)
            bits.put(len(blk[1]) ^ 0xFFFF, 16)
            for byte in blk[1]:
                bits.put(byte, 8)
        elif blk[0] == "fixed":
            bits.put(final, 1)
            bits.put(1, 2)
            put_tokens(bits, blk[1], *png_ref.fixed_lengths())
        else:
            header, n = P.dynamic_header(blk[2], blk[3])
            bits.put(header >> 1 << 1 | final, n)
            put_tokens(bits, blk[1], blk[2], blk[3])
    return bits.tobytes()


def tokens_of(raw, copies=None, lo=0, hi=None):
    """raw[lo:hi] as tokens: the copies {position: (length, distance)} where the plan says (each checked against raw), literals elsewhere."""
    copies, hi, out, p = copies or {}, len(raw) if hi is None else hi, [], lo
    while p < hi:
        if p in copies:
            n, d = copies[p]
            assert p + n <= hi and d <= p and all(raw[p + k] == raw[p - d + k % d] for k in range(n)), (p, n, d)
            out.append((n, d))
            p += n
        else:
            out.append(int(raw[p]))
            p += 1
    return out


def raw_noise(H, W, ch, seed, alphabet=256):
    """Raw rows with a valid filter type in front of each and random sample bytes: any bytes decode."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, alphabet, (H, 1 + W * ch), dtype=np.uint8)
    raw[:, 0] = rng.integers(0, 5, H)
    return bytearray(raw.tobytes())


def lengths_for(tokens):
    """(literal / length code lengths, distance COUNTS) that hold every symbol of these tokens: the encoder's own Huffman construction."""
    lit, dist = [0] * 286, [0] * 30
    lit[256] = 1
    for t in tokens:
        if isinstance(t, int):
            lit[t] += 1
        else:
            lit[257 + png_ref.length_symbol(t[0])[0]] += 1
            dist[png_ref.distance_symbol(t[1])[0]] += 1
    return P.huffman_lengths(lit, 15), dist


def special_streams():
    """name -> (H, W, channels, PNG file): the streams of the issue that zlib never emits, built with the token-list writer."""
    out = {}
    # a length-258 copy at distance exactly 32 768: 70 x 200 RGB is 42 070 raw bytes
    H, W, ch = 70, 200, 3
    stride = 1 + W * ch
    raw = raw_noise(H, W, ch, 1)
    for k in range(258):
        dst, src = 32768 + k, k
        if dst % stride == 0:
            raw[src] = raw[dst]
        else:
            raw[dst] = raw[src]
    toks = tokens_of(raw, {32768: (258, 32768)})
    out["far_copy_fixed"] = (H, W, ch, png_of_raw(H, W, ch, bytes(raw), write_blocks([("fixed", toks)])))
    lit, dc = lengths_for(toks)
    out["far_copy_dynamic"] = (H, W, ch, png_of_raw(H, W, ch, bytes(raw), write_blocks([("dynamic", toks, lit, P.distance_lengths(dc))])))
    # distance 1 with length 258, and the overlapping copies beside it (d = 2, 3, 7 shorter than the length)
    H, W, ch = 17, 33, 3
    raw = raw_noise(H, W, ch, 2)
    raw[150:150 + 259] = bytes([2]) * 259  # filter bytes inside the runs are their values: all of them are filter types
    plan = {151: (258, 1)}
    for at, n, period in ((500, 40, (3, 0)), (600, 258, (1, 4, 2)), (900, 100, (0, 1, 2, 3, 4, 3, 2))):
        d = len(period)
        raw[at - d:at + n] = bytes(period[k % d] for k in range(n + d))
        plan[at] = (n, d)
    toks = tokens_of(raw, plan)
    out["run_copy_fixed"] = (H, W, ch, png_of_raw(H, W, ch, bytes(raw), write_blocks([("fixed", toks)])))
    # an empty stored block and a stored block of 65 535 bytes: 70 x 320 RGB is 67 270 raw bytes
    H, W, ch = 70, 320, 3
    raw = bytes(raw_noise(H, W, ch, 3))
    blocks = [("stored", b""), ("stored", raw[:65535]), ("stored", b""), ("fixed", tokens_of(raw, lo=65535))]
    out["stored_blocks"] = (H, W, ch, png_of_raw(H, W, ch, raw, write_blocks(blocks)))
    # dynamic blocks with one distance code, and with none
    H, W, ch = 5, 9, 2
    raw = raw_noise(H, W, ch, 4, alphabet=16)
    raw[40:48] = raw[32:40]
    if any((40 + k) % (1 + W * ch) == 0 for k in range(8)):
        raw[40:48] = raw[32:40] = bytes([1]) * 8
    toks = tokens_of(raw, {40: (8, 8)})
    lit, dc = lengths_for(toks)
    assert sum(1 for c in dc if c) == 1
    out["one_distance_code"] = (H, W, ch, png_of_raw(H, W, ch, bytes(raw), write_blocks([("dynamic", toks, lit, P.distance_lengths(dc))])))
    toks = tokens_of(raw)
    lit, dc = lengths_for(toks)
    out["no_distance_code"] = (H, W, ch, png_of_raw(H, W, ch, bytes(raw), write_blocks([("dynamic", toks, lit, [0] * 30)])))
    # codes of 15 bits: a chain of lengths 1 .. 10 for the ten commonest bytes, then twelve codes of 14 and eight of 15 bits (Kraft sum 1)
    H, W, ch = 17, 33, 1
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    order = list(range(28, 4, -1)) + [0, 1, 2, 3, 4, 256]  # the bytes 28 .. 5 by falling frequency, the filter types, the end of block
    lit = [0] * 286
    for sym, l in zip(order, list(range(1, 11)) + [14] * 12 + [15] * 8):
        lit[sym] = l
    assert R.code_of(lit) is not None and not R._incomplete(R.code_of(lit)[0])
    rng = np.random.default_rng(5)
    raw = bytearray(rng.choice(np.arange(5, 29), H * (1 + W * ch), p=np.array(fib) / sum(fib)).astype(np.uint8).tobytes())
    raw[1:25] = bytes(range(5, 29))  # every symbol at least once, the 15-bit ones included
    for y in range(H):
        raw[y * (1 + W * ch)] = y % 5
    out["codes_of_15_bits"] = (H, W, ch, png_of_raw(H, W, ch, bytes(raw), write_blocks([("dynamic", tokens_of(raw), lit, [0] * 30)])))
    # a code-16 repeat that crosses from the literal / length lengths into the distance lengths: litlen ends in sixty 9s, the distance
    # lengths begin with two; the greedy run-length pass sends the 9 at 226 as itself and repeats of 6 from 227 on: the tenth covers 281 .. 286
    H, W, ch = 5, 9, 4
    raw = raw_noise(H, W, ch, 6)
    raw[100:110] = raw[90:100]
    if any((100 + k) % (1 + W * ch) == 0 for k in range(10)):
        raw[100:110] = raw[90:100] = bytes([3]) * 10
    lit, dc = [8] * 226 + [9] * 60, [9, 9, 8, 7, 6, 5, 4, 3, 2, 1] + [0] * 20
    out["repeat_across_codes"] = (H, W, ch, png_of_raw(H, W, ch, bytes(raw), write_blocks([("dynamic", tokens_of(raw, {100: (10, 10)}), lit, dc)])))
    return out


def hand_built(H, W, ch, seed=0):
    """name -> PNG file: rows filtered here, each of the five types alone and a random type per row, compressed by zlib.compressobj."""
    img = image(H, W, ch, seed)
    rng = np.random.default_rng(seed + 100)
    plans = {f"type{t}": [t] * H for t in range(5)}
    plans["mixed"] = rng.integers(0, 5, H).tolist()
    return {name: (img, png_of_raw(H, W, ch, filter_rows(img, types), zlib_deflate(filter_rows(img, types)))) for name, types in plans.items()}


def zlib_settings(raw):
    """name -> deflate bytes of `raw` under every window size, strategy and mid-stream flush."""
    out = {f"wbits{w}": zlib_deflate(raw, wbits=w) for w in range(9, 16)}
    for name in ("Z_FIXED", "Z_RLE", "Z_HUFFMAN_ONLY", "Z_FILTERED", "Z_DEFAULT_STRATEGY"):
        out[name] = zlib_deflate(raw, strategy=getattr(zlib, name))
    out["sync_flush"] = zlib_deflate(raw, flush_at=(len(raw) // 3, 2 * len(raw) // 3))
    out["full_flush"] = zlib_deflate(raw, flush_at=(len(raw) // 2,), flush=zlib.Z_FULL_FLUSH)
    out["level0"] = zlib_deflate(raw, level=0)
    return out


def damaged_bases():
    """Two small streams whose every bit flip and truncation the tests classify: (H, W, channels, body) -- a fixed block with copies,
    and a dynamic block."""
    H, W, ch = 5, 4, 3
    img = image(H, W, ch, 9)
    img[2:4] = img[0:2]
    raw = filter_rows(img, [0, 1, 2, 3, 4])
    a = zlib_deflate(raw, strategy=zlib.Z_FIXED) + struct.pack(">I", zlib.adler32(raw))
    H2, W2, ch2 = 6, 9, 2
    raw2 = bytes(raw_noise(H2, W2, ch2, 10, alphabet=12))
    toks = tokens_of(raw2)
    lit, _ = lengths_for(toks)
    b = write_blocks([("dynamic", toks[:60], lit, [0] * 30), ("stored", b""), ("fixed", toks[60:])]) + struct.pack(">I", zlib.adler32(raw2))
    return [(H, W, ch, a), (H2, W2, ch2, b)]


def damaged_variants(body):
    """Every bit flip and every truncation of a body."""
    out = [body[:n] for n in range(len(body))]
    for bit in range(8 * len(body)):
        out.append(body[:bit >> 3] + bytes([body[bit >> 3] ^ 1 << (bit & 7)]) + body[(bit >> 3) + 1:])
    return out


def expected_status(body, raw_size):
    """What the law makes of a body, from zlib alone: zlib inflates until it has one byte more than the raw size (where the law's walk
    stops), raises, runs out of input or reaches the end; then the trailer, the filter bytes and the checksum are looked at.
    -> a status, or the set {BAD_CODE, FAR} where zlib raises (its message is not part of the comparison)."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(body, raw_size + 1)
    except zlib.error:
        return {R.BAD_CODE, R.FAR}
    if len(out) > raw_size:
        return R.LONG
    if not d.eof or len(out) < raw_size or len(d.unused_data) < 4:
        return R.SHORT
    return None  # zlib inflated it to the end: 0, FILTER or ADLER, decided by the raw bytes
