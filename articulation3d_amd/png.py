"""PNG files written on the GPU: filtering, LZ77 and Huffman coding in HIP (a3d_png_scan / a3d_png_emit / a3d_png_pack, csrc/png.hip;
the law is stated in include/a3d.h and, in numpy, in tests/png_ref.py).  The lossless sibling of video.py's Motion-JPEG writer.

Every frame is an 8-bit truecolour PNG without interlace whose one IDAT holds a zlib stream of independent pieces: the frame's filtered
bytes are cut into segments of 8 .. 16 KB, one workgroup codes each segment as a stored, a fixed-Huffman or a dynamic-Huffman block
(the cheapest; the dynamic code is the frame's own) and ends it with an empty stored block, so segments concatenate as bytes.  What is
serial and branchy stays on the host, in this file, where the CPU tests hold it to zlib itself: the Huffman code of a frame from the
histogram the device leaves (huffman_lengths), its block header (dynamic_header), the Adler-32 from per-segment sums (adler_fold), the
chunk CRCs and the container.  Only compressed bytes, 316 counts per frame and two sums per segment cross PCIe.

    png_encode(frames_u8)                               -> list[bytes], complete PNG files
    render_clip_png(frames_u8, preds_raw, preds_opt)    -> yields list[bytes] per chunk: render_clip's rows, encoded losslessly
"""
from __future__ import annotations

import dataclasses
import heapq
import struct
import time
import zlib
from typing import Iterator, List, Sequence

import numpy as np

from . import _lib

MAX_W, SEG_BYTES, SYMS, HDR_AT, TAB_WORDS = _lib.PNG_MAX_W, _lib.PNG_SEG_BYTES, _lib.PNG_SYMS, _lib.PNG_HDR_AT, _lib.PNG_TAB_WORDS
N_LITLEN, N_DIST = 286, 30
SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def geometry(H: int, W: int):
    """(bytes of a filtered row, rows per segment, segments per frame) of H x W frames: pure arithmetic, the library's own rule."""
    if not (1 <= H <= 65535 and 1 <= W <= MAX_W):
        raise ValueError(f"{H} x {W}: the PNG encoder takes 1 .. 65535 rows of 1 .. {MAX_W} pixels")
    stride = 1 + 3 * W
    R = max(1, -(-SEG_BYTES // stride))
    return stride, R, -(-H // R)


def huffman_lengths(counts: Sequence[int], max_bits: int = 15) -> List[int]:
    """Code lengths of a Huffman code for `counts` (symbols with count 0 get length 0).  Plain two-smallest merging: the heap is
    ordered by (weight, id), a leaf's id is its symbol, the k-th merged node's id is len(counts) + k, so ties go to the lower symbol
    and to leaves before merged nodes.  If the longest code passes `max_bits`, every used weight becomes (w + 1) >> 1 and the code is
    built again (weights of 1 stay 1, so this ends with a balanced tree).  One used symbol gets length 1; none, all zeros."""
    n = len(counts)
    weights = [int(c) for c in counts]
    used = [s for s in range(n) if weights[s] > 0]
    if len(used) <= 1:
        return [1 if s in used else 0 for s in range(n)]
    if len(used) > 1 << max_bits:
        raise ValueError(f"{len(used)} symbols do not fit {max_bits} bits")
    while True:
        heap = [(weights[s], s) for s in used]
        heapq.heapify(heap)
        parent, next_id = {}, n
        while len(heap) > 1:
            wa, a = heapq.heappop(heap)
            wb, b = heapq.heappop(heap)
            parent[a] = parent[b] = next_id
            heapq.heappush(heap, (wa + wb, next_id))
            next_id += 1
        depth = {heap[0][1]: 0}
        for node in range(next_id - 2, n - 1, -1):  # merged nodes, children after parents
            depth[node] = depth[parent[node]] + 1
        lengths = [0] * n
        for s in used:
            lengths[s] = depth[parent[s]] + 1
        if max(lengths) <= max_bits:
            return lengths
        for s in used:
            weights[s] = (weights[s] + 1) >> 1


def distance_lengths(counts: Sequence[int]) -> List[int]:
    """huffman_lengths for the 30 distance symbols; a frame that used no distance gives distance 0 a 1-bit code (a single used distance
    gets 1 bit as well): the incomplete codes zlib accepts."""
    if not any(counts):
        return [1] + [0] * (len(counts) - 1)
    return huffman_lengths(counts, 15)


def canonical_codes(lengths: Sequence[int]) -> List[int]:
    """RFC 1951, 3.2.2: codes of one length are consecutive in symbol order, shorter codes come first."""
    max_len = max(lengths) if len(lengths) else 0
    count = [0] * (max_len + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * (max_len + 2)
    for bits in range(1, max_len + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        out.append(nxt[l] if l else 0)
        nxt[l] += 1 if l else 0
    return out


def bit_reverse(code: int, length: int) -> int:
    return int(format(code, f"0{length}b")[::-1], 2) if length else 0


class _Bits:
    """A bit string packed as deflate packs it: LSB first."""

    def __init__(self):
        self.value, self.n = 0, 0

    def put(self, v: int, nbits: int) -> None:  # an integer, least significant bit first
        self.value |= v << self.n
        self.n += nbits

    def put_code(self, code: int, nbits: int) -> None:  # a Huffman code, most significant bit first
        self.put(bit_reverse(code, nbits), nbits)


def dynamic_header(litlen: Sequence[int], dist: Sequence[int]):
    """The header of a dynamic block for these code lengths, BFINAL = 0 and BTYPE = 10 included -> (bits as an integer, LSB first; number of
    bits).  HLIT / HDIST trim the unused tails; the lengths are run-length-coded by one greedy pass: at a zero, a run of 3 or more zeros
    becomes symbol 17 (3 .. 10) or 18 (11 .. 138, the longest that fits); at a non-zero length equal to the one before it, a run of 3 or
    more becomes symbol 16 (3 .. 6); anything else is sent as itself.  The code-length code is huffman_lengths at 7 bits."""
    hlit = max(257, max(s for s in range(len(litlen)) if litlen[s]) + 1)
    hdist = max([s for s in range(len(dist)) if dist[s]] + [0]) + 1
    seq = list(litlen[:hlit]) + list(dist[:hdist])
    syms, p = [], 0  # (symbol, extra bits, extra value)
    while p < len(seq):
        v, r = seq[p], 1
        while p + r < len(seq) and seq[p + r] == v:
            r += 1
        if v == 0 and r >= 3:
            m = min(r, 138)
            syms.append((18, 7, m - 11) if m >= 11 else (17, 3, m - 3))
        elif v != 0 and p > 0 and seq[p - 1] == v and r >= 3:
            m = min(r, 6)
            syms.append((16, 2, m - 3))
        else:
            m = 1
            syms.append((v, 0, 0))
        p += m
    cl_counts = [0] * 19
    for s, _, _ in syms:
        cl_counts[s] += 1
    if sum(1 for c in cl_counts if c) == 1:  # zlib refuses an incomplete code-length code: a second, unused symbol completes it
        cl_counts[1 if cl_counts[0] else 0] = 1
    cl_len = huffman_lengths(cl_counts, 7)
    cl_code = canonical_codes(cl_len)
    hclen = max(4, max(i for i, s in enumerate(_CL_ORDER) if cl_len[s]) + 1)
    b = _Bits()
    b.put(0, 1)
    b.put(2, 2)
    b.put(hlit - 257, 5)
    b.put(hdist - 1, 5)
    b.put(hclen - 4, 4)
    for s in _CL_ORDER[:hclen]:
        b.put(cl_len[s], 3)
    for s, nx, x in syms:
        b.put_code(cl_code[s], cl_len[s])
        if nx:
            b.put(x, nx)
    return b.value, b.n


def frame_code(hist: Sequence[int]):
    """A frame's histogram (286 literal / length counts, then 30 distance counts) -> (litlen lengths, distance lengths)."""
    hist = [int(c) for c in hist]
    return huffman_lengths(hist[:N_LITLEN], 15), distance_lengths(hist[N_LITLEN:SYMS])


def frame_table(hist: Sequence[int]) -> np.ndarray:
    """What a3d_png_emit reads per frame: uint32 [TAB_WORDS]; words 0 .. 315 bit-reversed code | length << 16, word 316 the header's
    bits, from word HDR_AT the header, LSB first."""
    litlen, dist = frame_code(hist)
    tab = np.zeros(TAB_WORDS, np.uint32)
    for base, lengths in ((0, litlen), (N_LITLEN, dist)):
        for s, (c, l) in enumerate(zip(canonical_codes(lengths), lengths)):
            tab[base + s] = bit_reverse(c, l) | l << 16
    bits, n = dynamic_header(litlen, dist)
    assert n <= 32 * (TAB_WORDS - HDR_AT)
    tab[SYMS] = n
    raw = bits.to_bytes(4 * (TAB_WORDS - HDR_AT), "little")
    tab[HDR_AT:] = np.frombuffer(raw, "<u4")
    return tab


def adler_fold(s1: Sequence[int], s2: Sequence[int], n: Sequence[int]) -> int:
    """Adler-32 of the concatenation of pieces of n[k] bytes from their sums s1 = sum b_j and s2 = sum (n - j) b_j."""
    a, b = 1, 0
    for p1, p2, nk in zip(s1, s2, n):
        b = (b + int(nk) * a + int(p2)) % 65521
        a = (a + int(p1)) % 65521
    return b << 16 | a


def _chunk(kind: bytes, *parts: bytes) -> List[bytes]:
    crc = zlib.crc32(kind)
    for p in parts:
        crc = zlib.crc32(p, crc)
    return [struct.pack(">I", sum(len(p) for p in parts)), kind, *parts, struct.pack(">I", crc)]


def png_file(H: int, W: int, deflate: bytes, adler: int) -> bytes:
    """The container round a frame's packed segments: signature, IHDR, one IDAT (78 01 | segments | 03 00 | Adler-32), IEND."""
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    return b"".join([SIGNATURE, *_chunk(b"IHDR", ihdr), *_chunk(b"IDAT", b"\x78\x01", deflate, b"\x03\x00" + struct.pack(">I", adler)),
                     *_chunk(b"IEND")])


class _Encoder:
    """The device and pinned buffers of one (frames per call, H, W), allocated once; slots are worst-case (opt_ops.png_geometry), so no
    input can overrun them.  scan() launches on the current stream and starts the histograms for the host; emit() waits for them alone,
    builds every frame's code and launches the coding; fetch() learns the lengths, then packs and brings only the used bytes to the
    host on streams.side(2), the pool's copy role.  `seconds` collects the host's shares (tools/png_bench.py reports them)."""

    def __init__(self, cap_frames: int, H: int, W: int, device):
        import torch

        from . import opt_ops

        self.stride, self.R, self.S, self.slot = opt_ops.png_geometry(H, W)
        while cap_frames > 1 and cap_frames * max(H * self.stride, self.S * self.slot) > 0x7FFFFFFF:  # the library's int32 offsets
            cap_frames = (cap_frames + 1) // 2
        self.cap, self.H, self.W, self.dev = cap_frames, H, W, device
        n_seg, n_byte = cap_frames * self.S, cap_frames * H * self.stride
        self.filt = torch.empty(n_byte, dtype=torch.uint8, device=device)
        self.tok = torch.empty(n_byte, dtype=torch.int16, device=device)
        self.hist = torch.empty(cap_frames * SYMS, dtype=torch.int32, device=device)
        self.tab = torch.empty(cap_frames * TAB_WORDS, dtype=torch.int32, device=device)
        self.s1 = torch.empty(n_seg, dtype=torch.int32, device=device)
        self.s2 = torch.empty(n_seg, dtype=torch.int64, device=device)
        self.slots = torch.empty(n_seg * self.slot, dtype=torch.uint8, device=device)
        self.meta = torch.empty(3 * n_seg + cap_frames + 1, dtype=torch.int32, device=device)  # seg_len | seg_off | kind | frame_off
        self.seg_len, self.seg_off, self.kind = self.meta[:n_seg], self.meta[n_seg:2 * n_seg], self.meta[2 * n_seg:3 * n_seg]
        self.frame_off = self.meta[3 * n_seg:]
        self.host_hist = torch.empty(cap_frames * SYMS, dtype=torch.int32).pin_memory()
        self.host_tab = torch.empty(cap_frames * TAB_WORDS, dtype=torch.int32).pin_memory()
        self.host_off = torch.empty(cap_frames + 1, dtype=torch.int32).pin_memory()
        self.host_s1 = torch.empty(n_seg, dtype=torch.int32).pin_memory()
        self.host_s2 = torch.empty(n_seg, dtype=torch.int64).pin_memory()
        self.packed = torch.empty(0, dtype=torch.uint8, device=device)
        self.host = torch.empty(0, dtype=torch.uint8).pin_memory()
        rows = [min(self.R, H - s * self.R) for s in range(self.S)]
        self.seg_bytes = [r * self.stride for r in rows]
        self.seconds = {"huffman": 0.0, "crc_and_files": 0.0}
        self.n = 0

    def scan(self, frames_u8) -> None:
        """Filter, find the tokens and count the symbols of n <= cap frames on the current stream."""
        import torch

        from . import opt_ops

        self.n = n = frames_u8.shape[0]
        assert n <= self.cap and tuple(frames_u8.shape[1:3]) == (self.H, self.W)
        opt_ops.png_scan_into(frames_u8, self.filt, self.tok, self.hist, self.s1, self.s2)
        self.host_hist[:n * SYMS].copy_(self.hist[:n * SYMS], non_blocking=True)  # the first small copy: the host learns the histograms
        self.scanned = torch.cuda.Event()
        self.scanned.record(torch.cuda.current_stream(self.dev))

    def emit(self) -> None:
        """The frames' codes, on the host, and their coding, queued on the current stream behind whatever the caller has queued since."""
        import torch

        from . import opt_ops

        n = self.n
        self.scanned.synchronize()
        t0 = time.perf_counter()
        hist, tab = self.host_hist.numpy().reshape(-1, SYMS), self.host_tab.numpy().view(np.uint32).reshape(-1, TAB_WORDS)
        for f in range(n):
            tab[f] = frame_table(hist[f])
        self.seconds["huffman"] += time.perf_counter() - t0
        self.tab[:n * TAB_WORDS].copy_(self.host_tab[:n * TAB_WORDS], non_blocking=True)
        opt_ops.png_emit_into(self.filt, self.tok, self.tab, n, self.H, self.W, self.slots, self.seg_len, self.seg_off, self.frame_off, self.kind)
        self.host_off[:n + 1].copy_(self.frame_off[:n + 1], non_blocking=True)  # the second: the lengths and the Adler sums
        self.host_s1[:n * self.S].copy_(self.s1[:n * self.S], non_blocking=True)
        self.host_s2[:n * self.S].copy_(self.s2[:n * self.S], non_blocking=True)
        self.done = torch.cuda.Event()
        self.done.record(torch.cuda.current_stream(self.dev))

    def fetch(self) -> List[bytes]:
        """The frames of the last scan() + emit() as complete files."""
        import torch

        from . import opt_ops, streams

        n = self.n
        self.done.synchronize()
        off = self.host_off[:n + 1].tolist()
        total = off[n]
        copy_stream = streams.side(2, self.dev)
        with torch.cuda.stream(copy_stream):
            if total > self.packed.numel():  # grown geometrically, kept for the next chunk
                size = max(total, 2 * self.packed.numel(), 1 << 16)
                self.packed = torch.empty(size, dtype=torch.uint8, device=self.dev)
                self.host = torch.empty(size, dtype=torch.uint8).pin_memory()
            opt_ops.png_pack_into(self.slots, self.seg_off, self.seg_len, n, self.H, self.W, self.packed)
            self.host[:total].copy_(self.packed[:total], non_blocking=True)
        copy_stream.synchronize()
        t0 = time.perf_counter()
        data = self.host.numpy()
        s1 = self.host_s1.numpy().view(np.uint32).reshape(-1, self.S)
        s2 = self.host_s2.numpy().view(np.uint64).reshape(-1, self.S)
        out = [png_file(self.H, self.W, data[off[f]:off[f + 1]].tobytes(), adler_fold(s1[f], s2[f], self.seg_bytes)) for f in range(n)]
        self.seconds["crc_and_files"] += time.perf_counter() - t0
        return out


def png_encode(frames_u8, chunk: int = 8) -> List[bytes]:
    """uint8 [F,H,W,3] RGB on the device (dense, or a column range of wider rows) -> F complete PNG files that decode to exactly the
    input.  The bytes of a frame do not depend on F, on `chunk` or on the frames beside it."""
    from . import opt_ops

    F, H, W, _pitch = opt_ops._pitched_frames(frames_u8)
    opt_ops.png_geometry(H, W)
    out: List[bytes] = []
    if F == 0:
        return out
    enc = _Encoder(min(max(int(chunk), 1), F), H, W, frames_u8.device)
    for lo in range(0, F, enc.cap):
        enc.scan(frames_u8[lo:lo + enc.cap])
        enc.emit()
        out += enc.fetch()
    return out


def render_clip_png(frames_u8, preds_raw: Sequence, preds_opt: Sequence, chunk: int = 8, mask_alpha: float = 0.0, conf_threshold: float = 0.7,
                    seconds: dict = None) -> Iterator[List[bytes]]:
    """Yields, `chunk` frames at a time, the clip's rows `[opt seg | opt normal | raw seg | raw normal]` as PNG files [H, 4W]: the rows
    are rendered exactly as render.render_clip renders them (the same two render_panels calls per chunk into a device staging buffer)
    and encoded where they are; decoded, they are render_clip's rows exactly.  Raw rows never leave the device.  While the host builds
    chunk k's Huffman codes, chunk k+1 is being rendered and scanned: its launches are queued first.  `seconds`, if given, receives the
    host's shares."""
    import torch

    from .render import render_panels

    F, H, W, _ = frames_u8.shape
    assert len(preds_raw) == F and len(preds_opt) == F
    dev = frames_u8.device if frames_u8.is_cuda else torch.device("cuda", torch.cuda.current_device())
    chunk = max(1, min(int(chunk), max(F, 1)))
    stage = [torch.empty((chunk, H, 4 * W, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
    enc = [_Encoder(chunk, H, 4 * W, dev) for _ in range(2)]
    if enc[0].cap < chunk:
        raise ValueError(f"chunk {chunk} of {H} x {4 * W} rows is more than one encoder call holds ({enc[0].cap}): pass a smaller chunk")

    def finish(e):
        e.emit()
        files = e.fetch()
        if seconds is not None:
            for k, v in e.seconds.items():
                seconds[k] = seconds.get(k, 0.0) + v
                e.seconds[k] = 0.0
        return files

    pending = None
    for k, lo in enumerate(range(0, F, chunk)):
        hi, b = min(lo + chunk, F), k % 2
        fr = frames_u8[lo:hi].to(dev, non_blocking=True).contiguous()
        out = stage[b][:hi - lo]
        render_panels(fr, preds_opt[lo:hi], out=out, col=0, mask_alpha=mask_alpha, conf_threshold=conf_threshold)
        render_panels(fr, preds_raw[lo:hi], out=out, col=2 * W, mask_alpha=mask_alpha, conf_threshold=conf_threshold)
        enc[b].scan(out)
        if pending is not None:  # the previous chunk's codes, coding, pack and copy: this chunk's launches are queued in front of them
            yield finish(pending)
        pending = enc[b]
    if pending is not None:
        yield finish(pending)


# ---- reading ---------------------------------------------------------------------------------------------------------------------
PNGD_STATUS = {_lib.PNGD_SHORT: "SHORT", _lib.PNGD_BAD_CODE: "BAD_CODE", _lib.PNGD_FAR: "FAR", _lib.PNGD_LONG: "LONG",
               _lib.PNGD_FILTER: "FILTER", _lib.PNGD_ADLER: "ADLER"}
_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}
DECODE_CHUNK = 90  # frames per a3d_png_decode call: the fastest of 8, 32 and 90 for four of five classes of file (MEASUREMENTS.md, "PNG decode")


@dataclasses.dataclass(frozen=True)
class PNGInfo:
    """What png_parse finds: the geometry and where the deflate body lies -- the byte ranges (lo, hi) of the file whose concatenation
    is the IDAT payload without the two bytes of the zlib header (the Adler-32 at its end included)."""
    height: int
    width: int
    channels: int
    ranges: tuple

    @property
    def geometry(self):
        return self.height, self.width, self.channels

    @property
    def raw_size(self) -> int:
        return self.height * (1 + self.width * self.channels)


def png_parse(data: bytes) -> PNGInfo:
    """The container of one PNG file, on the host: the chunk walk, every chunk's CRC, IHDR and the zlib header.  ValueError names
    what puts a file outside the law of include/a3d.h ("PNG decode"): palette, bit depths other than 8, Adam7, a damaged container.
    Ancillary chunks (tRNS included) are skipped."""
    if data[:8] != SIGNATURE:
        raise ValueError("not a PNG file (bad signature)")
    at, n_data = 8, len(data)
    ihdr, ranges, seen_idat, closed, ended = None, [], False, False, False
    while at < n_data:
        if at + 12 > n_data:
            raise ValueError("chunk cut short")
        n, kind = struct.unpack_from(">I4s", data, at)
        if at + 12 + n > n_data:
            raise ValueError(f"chunk {kind!r} cut short")
        if zlib.crc32(data[at + 4:at + 8 + n]) != struct.unpack_from(">I", data, at + 8 + n)[0]:
            raise ValueError(f"chunk {kind!r}: CRC does not match")
        if ihdr is None and kind != b"IHDR":
            raise ValueError("no IHDR chunk in front")
        if kind == b"IHDR":
            if ihdr is not None or n != 13:
                raise ValueError("more than one IHDR chunk, or one of the wrong size")
            ihdr = struct.unpack_from(">IIBBBBB", data, at + 8)
        elif kind == b"IDAT":
            if closed:
                raise ValueError("IDAT chunks are not consecutive")
            seen_idat = True
            ranges.append((at + 8, at + 8 + n))
        elif kind == b"IEND":
            ended = True
            break
        if seen_idat and kind != b"IDAT":
            closed = True
        at += 12 + n
    if ihdr is None:
        raise ValueError("no IHDR chunk")
    if not seen_idat:
        raise ValueError("no IDAT chunk")
    if not ended:
        raise ValueError("no IEND chunk")
    width, height, depth, colour, compression, filt, interlace = ihdr
    if colour == 3:
        raise ValueError("palette image (colour type 3)")
    if colour not in _CHANNELS:
        raise ValueError(f"colour type {colour}")
    if depth != 8:
        raise ValueError(f"bit depth {depth}: 8 only")
    if interlace:
        raise ValueError("interlaced (Adam7)")
    if compression or filt:
        raise ValueError(f"compression method {compression} / filter method {filt}")
    if width == 0 or height == 0:
        raise ValueError(f"{height} x {width}: an empty image")
    channels = _CHANNELS[colour]
    if height * (1 + width * channels) > 0x7FFFFFFF:
        raise ValueError(f"{height} x {width} x {channels}: more than 2^31 - 1 bytes of rows")
    head, body = [], []
    for lo, hi in ranges:  # the zlib header may lie across chunks
        take = min(2 - len(head), hi - lo)
        head += data[lo:lo + take]
        if hi > lo + take:
            body.append((lo + take, hi))
    if len(head) < 2:
        raise ValueError("zlib header cut short")
    cmf, flg = head
    if cmf & 15 != 8 or cmf >> 4 > 7 or flg & 32 or (cmf << 8 | flg) % 31:
        raise ValueError(f"zlib header {cmf:02x} {flg:02x}: want CM = 8, CINFO <= 7, FDICT = 0 and a valid FCHECK")
    return PNGInfo(height, width, channels, tuple(body))


def png_decode(pngs: Sequence[bytes], device="cuda", chunk: int = DECODE_CHUNK, strict: bool = True):
    """F PNG files of one size and one colour type (8-bit grey, grey + alpha, RGB or RGBA, no interlace) -> uint8 [F,H,W,3] RGB on the
    device, byte for byte PIL's Image.open(f).convert("RGB") (include/a3d.h states the law: grey is replicated, alpha dropped).  The host
    walks the chunks and uploads the deflate bodies; inflate, Adler-32, unfiltering and the conversion run on the device, `chunk`
    frames per a3d_png_decode call, and the host prepares a chunk while the device decodes the one before.  A frame's pixels do not
    depend on the frames beside it or on `chunk`.  With `strict` a frame whose status is not 0 raises ValueError with its index and the
    code (PNGD_STATUS); without, -> (frames, status int32 [F] on the host): the pixels of a flagged frame mean nothing."""
    import torch

    from . import opt_ops

    infos = []
    for i, blob in enumerate(pngs):
        try:
            infos.append(png_parse(blob))
        except ValueError as e:
            raise ValueError(f"frame {i}: {e}") from None
    if not infos:
        raise ValueError("png_decode: no frames")
    for i, info in enumerate(infos):
        if info.geometry != infos[0].geometry:
            raise ValueError(f"frame {i} is {info.geometry} (H, W, channels), frame 0 is {infos[0].geometry}: one call decodes one geometry")
    H, W, channels = infos[0].geometry
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"device {device!r}: the decoder runs on the GPU")
    F = len(infos)
    chunk = max(1, min(int(chunk), F))
    per = opt_ops.png_decode_scratch(H, W, channels)
    while chunk > 1 and chunk * per > 1 << 32:  # scratch of at most 4 GB
        chunk = (chunk + 1) // 2
    with torch.cuda.device(dev):
        raw = torch.empty(chunk * per, dtype=torch.uint8, device=dev)
        out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        status = torch.empty(F, dtype=torch.int32, device=dev)
        for lo in range(0, F, chunk):
            hi = min(lo + chunk, F)
            pieces, off = [], [0]
            for k in range(lo, hi):
                pieces += [pngs[k][a:b] for a, b in infos[k].ranges]
                off.append(off[-1] + sum(b - a for a, b in infos[k].ranges))
            total = off[-1]
            if total > 0x7FFFFFFF:
                raise ValueError(f"frames {lo} .. {hi - 1} hold {total} bytes: more than one call takes, pass a smaller chunk")
            blob = np.frombuffer(b"".join(pieces) + bytes(-total % 4 + 4), np.uint8)
            off = np.array(off, np.int32)
            opt_ops.png_decode_into(out[lo:hi], status[lo:hi], torch.from_numpy(blob.copy()).to(dev), off, torch.from_numpy(off).to(dev), channels, raw)
        st = status.cpu()
    if not strict:
        return out, st
    bad = torch.nonzero(st).flatten().tolist()
    if bad:
        raise ValueError(f"frame {bad[0]}: status {PNGD_STATUS.get(int(st[bad[0]]), int(st[bad[0]]))}" +
                         (f" (and {len(bad) - 1} more frames)" if len(bad) > 1 else ""))
    return out
