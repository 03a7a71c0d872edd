"""The law of the baseline-JPEG decoder (articulation3d_amd/video.py, csrc/jpeg_decode.hip; stated in include/a3d.h), in numpy,
integers only.  The kernels reproduce `decode` byte for byte; tests/test_jpeg_decode_host.py holds this file to PIL's libjpeg byte
for byte.  It depends on nothing of the package: the parser below is written from ITU-T T.81, not from video.jpeg_parse.

  accepted  SOF0, 8-bit, one interleaved scan; one component (grey, R = G = B) or Y / Cb / Cr with chroma 1x1 and luma 1x1, 2x1 or
            2x2; 8-bit quantisation tables; any Huffman tables (none at all: the Annex K tables, the AVI "MJPG" convention); any
            restart interval.  Everything else is a ValueError naming the cause.
  geometry  an MCU is 8 hmax x 8 vmax pixels, ceil(W / 8 hmax) x ceil(H / 8 vmax) of them in raster order, each component giving its
            v x h blocks in raster order.  A unit is one restart interval (the whole scan without one): the DC predictors start
            at 0 in every unit.  A stream with fewer units than its geometry asks for is continued with empty units; units past
            the geometry are ignored.
  entropy   FF 00 is the data byte FF.  Symbol, run / size, ZRL, EOB and one's-complement extension as in the standard; a DC value
            accumulates modulo 2^16.  Bits past the unit's bytes read as 0 and make the frame SHORT.  A bit pattern that matches no
            code of at most 16 bits, a DC symbol above 15, or a run that passes coefficient 63 (a ZRL that ends past 64 included)
            makes it BAD_CODE and ends the unit: its remaining blocks stay zero.
  IDCT      libjpeg's jidctint ("islow"): dequantise, pass 1 over columns (descale 11), pass 2 over rows (descale 18),
            sample = clamp(v + 128, 0, 255).  The law holds where every dequantised coefficient and every pass-1 output is within
            +-16383 (every intermediate then fits int32); a frame with a block outside is RANGE and its pixels are unspecified
            (this file clamps both to [-16384, 16383] and carries on).
  upsample  libjpeg's "fancy" filters on the component's true size dw = ceil(W/2), dh = ceil(H/2) (4:2:2: dh = H), neighbours clamped
            to the plane; a chroma plane at most 2 samples wide is replicated instead, in both directions.
  colour    R = Y + ((91881 Cr' + 32768) >> 16), G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16), B = Y + ((116130 Cb' + 32768) >> 16),
            Cb' = Cb - 128, Cr' = Cr - 128, >> arithmetic, clamped to 0 .. 255.
  status    the frame's status is the largest of 0 < RANGE < BAD_CODE < SHORT that occurred: the cause, not its consequences.
"""
from __future__ import annotations

import re

import numpy as np

import mjpeg_ref as M

OK, RANGE, BAD_CODE, SHORT = 0, 1, 2, 3
DOMAIN = 16383
ANNEX_K = {  # (class, id) -> (bits, vals): class 0 DC, 1 AC; id 0 luminance, 1 chrominance
    (0, 0): (M.DC_LUMA_BITS, M.DC_VALS), (1, 0): (M.AC_LUMA_BITS, M.AC_LUMA_VALS),
    (0, 1): (M.DC_CHROMA_BITS, M.DC_VALS), (1, 1): (M.AC_CHROMA_BITS, M.AC_CHROMA_VALS)}
_NOT_DATA = re.compile(b"\xff[^\x00\xd0-\xd7]")
_RST = re.compile(b"\xff[\xd0-\xd7]")


class Parsed:
    """height, width, comps [(h, v, quant int64 [64] natural, (dc_bits, dc_vals), (ac_bits, ac_vals))], hmax, vmax, restart, units
    [bytes]: the entropy-coded bytes of every unit, still stuffed, without the markers between them."""


def parse(data: bytes) -> Parsed:
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG: no SOI marker")
    quant, huff, frame, restart, scan, adobe = {}, {}, None, 0, None, None
    at = 2
    while at + 4 <= len(data):
        if data[at] != 0xFF:
            raise ValueError(f"byte {at}: a marker was expected")
        m = data[at + 1]
        if m == 0xFF:
            at += 1
            continue
        if m == 0xD9:
            break
        n = int.from_bytes(data[at + 2:at + 4], "big")
        body = data[at + 4:at + 2 + n]
        at += 2 + n
        if m == 0xDB:
            while body:
                if body[0] >> 4:
                    raise ValueError("16-bit quantisation table")
                q = np.zeros(64, np.int64)
                q[M.ZIGZAG] = list(body[1:65])
                quant[body[0] & 15], body = q, body[65:]
        elif m == 0xC4:
            while body:
                bits = list(body[1:17])
                huff[(body[0] >> 4, body[0] & 15)] = (bits, list(body[17:17 + sum(bits)]))
                body = body[17 + sum(bits):]
        elif m == 0xDD:
            restart = int.from_bytes(body[:2], "big")
        elif m == 0xEE and body[:5] == b"Adobe":
            adobe = body[11]
        elif m == 0xC0:
            if frame is not None:
                raise ValueError("more than one frame header")
            frame = body
        elif m == 0xC2:
            raise ValueError("progressive JPEG (SOF2)")
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise ValueError(f"SOF{m - 0xC0}: arithmetic coding" if m >= 0xC9 else f"SOF{m - 0xC0}: not baseline (12-bit, lossless or hierarchical)")
        elif m == 0xDA:
            if frame is None:
                raise ValueError("SOS without a frame header: no SOF")
            scan = (body, at)
            break
    if frame is None:
        raise ValueError("no SOF marker")
    if scan is None:
        raise ValueError("no SOS marker")
    out = Parsed()
    precision, out.height, out.width, ncomp = frame[0], int.from_bytes(frame[1:3], "big"), int.from_bytes(frame[3:5], "big"), frame[5]
    if precision != 8:
        raise ValueError(f"{precision}-bit samples")
    if ncomp not in (1, 3):
        raise ValueError(f"{ncomp} components: grey or Y / Cb / Cr only")
    if not (1 <= out.height <= 65535 and 1 <= out.width <= 65535):
        raise ValueError(f"{out.height} x {out.width}: a JPEG is 1 .. 65535 pixels a side")
    if ncomp == 3 and adobe == 0:
        raise ValueError("Adobe transform 0: RGB, not Y / Cb / Cr")
    body, lo = scan
    if body[0] != ncomp:
        raise ValueError("more than one scan")
    ids = {body[1 + 2 * i]: body[2 + 2 * i] for i in range(ncomp)}
    out.comps = []
    for i in range(ncomp):
        cid, hv, tq = frame[6 + 3 * i:9 + 3 * i]
        if cid not in ids:
            raise ValueError("more than one scan")
        if tq not in quant:
            raise ValueError(f"quantisation table {tq} is missing")
        tabs = []
        for cls, tid in ((0, ids[cid] >> 4), (1, ids[cid] & 15)):
            if (cls, tid) in huff:
                tabs.append(huff[(cls, tid)])
            elif not huff and (cls, tid) in ANNEX_K:
                tabs.append(ANNEX_K[(cls, tid)])
            else:
                raise ValueError(f"Huffman table {cls}/{tid} is missing")
        out.comps.append((hv >> 4, hv & 15, quant[tq], tabs[0], tabs[1]))
    if ncomp == 1:
        out.comps[0] = (1, 1) + out.comps[0][2:]
    elif [c[:2] for c in out.comps[1:]] != [(1, 1), (1, 1)] or out.comps[0][:2] not in ((1, 1), (2, 1), (2, 2)):
        raise ValueError("sampling factors " + ", ".join(f"{c[0]}x{c[1]}" for c in out.comps) + ": 4:4:4, 4:2:2 or 4:2:0 only")
    if tuple(body[1 + 2 * ncomp:4 + 2 * ncomp]) != (0, 63, 0):
        raise ValueError("not a sequential scan")
    out.hmax, out.vmax = out.comps[0][:2]
    end = _NOT_DATA.search(data, lo)
    hi = end.start() if end else len(data)
    if end and _NOT_DATA.search(data, hi + 2) is not None and b"\xff\xda" in data[hi:]:
        raise ValueError("more than one scan")
    out.restart = restart
    out.units = _RST.split(data[lo:hi]) if restart else [data[lo:hi]]
    return out


def _codes(bits, vals):
    """(length, code) -> symbol, Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(length, code)] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return out


class _Bits:
    def __init__(self, unit: bytes):
        raw = unit.replace(b"\xff\x00", b"\xff")
        self.n = 8 * len(raw)
        self.v = int.from_bytes(raw, "big") if raw else 0
        self.at = 0
        self.short = False

    def get(self, k: int) -> int:
        """The next k bits; those past the unit's end are 0 and mark it short."""
        if k == 0:
            return 0
        end = self.at + k
        real = max(min(end, self.n) - self.at, 0)  # the bits that exist
        v = ((self.v >> (self.n - self.at - real)) & ((1 << real) - 1)) << (k - real) if real else 0
        self.short |= end > self.n
        self.at = end
        return v

    def symbol(self, codes):
        """The next Huffman symbol, or None.  A code is found from the bits that exist plus zeros; only the bits it takes are consumed."""
        code = 0
        start = self.at
        for length in range(1, 17):
            self.at = start
            code = self.get(length)
            if (length, code) in codes:
                return codes[(length, code)]
        return None


def _extend(v: int, s: int) -> int:
    return v if s == 0 or v >> (s - 1) else v - (1 << s) + 1


def _wrap16(v: int) -> int:
    return ((v + 32768) & 0xFFFF) - 32768


def coefficients(p: Parsed):
    """-> ([per component int64 [bh, bw, 64] natural order, quantised], status)."""
    mx, my = -(-p.width // (8 * p.hmax)), -(-p.height // (8 * p.vmax))
    total = mx * my
    planes = [np.zeros((my * v, mx * h, 64), np.int64) for h, v, *_ in p.comps]
    tabs = [(_codes(*c[3]), _codes(*c[4])) for c in p.comps]
    ri = p.restart if p.restart else total
    n_units = -(-total // ri)
    units = (list(p.units) + [b""] * n_units)[:n_units]
    status = OK
    for k, unit in enumerate(units):
        rd = _Bits(unit)
        pred = [0] * len(p.comps)
        bad = False
        for m in range(k * ri, min((k + 1) * ri, total)):
            for c, (h, v, *_r) in enumerate(p.comps):
                for j in range(v * h):
                    blk = planes[c][(m // mx) * v + j // h, (m % mx) * h + j % h]
                    s = rd.symbol(tabs[c][0])
                    if s is None or s > 15:
                        bad = True
                        break
                    pred[c] = _wrap16(pred[c] + _extend(rd.get(s), s))
                    blk[0] = pred[c]
                    i = 1
                    while i < 64:
                        rs = rd.symbol(tabs[c][1])
                        if rs is None:
                            bad = True
                            break
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            i += 16
                            if i > 64:
                                bad = True
                                break
                            continue
                        i += r
                        if i > 63:
                            bad = True
                            break
                        blk[M.ZIGZAG[i]] = _extend(rd.get(s), s)
                        i += 1
                    if bad:
                        break
                if bad:
                    break
            if bad:
                break
        status = max(status, SHORT if rd.short else BAD_CODE if bad else OK)
    return planes, status


_F = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137, c1961=16069, c2053=16819,
          c2562=20995, c3072=25172)


def _pass(x: np.ndarray, shift: int) -> np.ndarray:
    """One jidctint pass over the LAST axis of int64 [..., 8]."""
    c = _F
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * c["c0541"]
    t2, t3 = z1 - z3 * c["c1847"], z1 + z2 * c["c0765"]
    t0, t1 = (x[..., 0] + x[..., 4]) << 13, (x[..., 0] - x[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * c["c1175"]
    t0, t1, t2, t3 = t0 * c["c0298"], t1 * c["c2053"], t2 * c["c3072"], t3 * c["c1501"]
    z1, z2, z3, z4 = -z1 * c["c0899"], -z2 * c["c2562"], -z3 * c["c1961"] + z5, -z4 * c["c0390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct(coef: np.ndarray, quant: np.ndarray):
    """int64 [bh, bw, 64] quantised, natural order -> (uint8 [8 bh, 8 bw] samples, bool [bh, bw]: the block is inside the domain)."""
    bh, bw, _ = coef.shape
    d = (coef * quant).reshape(bh, bw, 8, 8)
    inside = (np.abs(d) <= DOMAIN).all((2, 3))
    d = np.clip(d, -DOMAIN - 1, DOMAIN)
    w = _pass(d.transpose(0, 1, 3, 2), 11).transpose(0, 1, 3, 2)   # columns
    inside &= (np.abs(w) <= DOMAIN).all((2, 3))
    w = np.clip(w, -DOMAIN - 1, DOMAIN)
    s = np.clip(_pass(w, 18) + 128, 0, 255)                          # rows
    return s.transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw).astype(np.uint8), inside


def upsample(plane: np.ndarray, h: int, v: int, H: int, W: int) -> np.ndarray:
    """The component's samples -> int64 [H, W]: h, v = hmax / h_c, vmax / v_c in {1, 2}."""
    dw, dh = -(-W // h), -(-H // v)
    p = plane[:dh, :dw].astype(np.int64)
    if h == 1:
        return p[:H, :W]
    if dw <= 2:
        return np.repeat(np.repeat(p, v, 0), 2, 1)[:H, :W]
    if v == 2:
        up, dn = p[np.maximum(np.arange(dh) - 1, 0)], p[np.minimum(np.arange(dh) + 1, dh - 1)]
        s = np.empty((2 * dh, dw), np.int64)
        s[0::2], s[1::2] = 3 * p + up, 3 * p + dn
        r0, r1, sh = 8, 7, 4
    else:
        s, r0, r1, sh = p, 1, 2, 2
    left, right = s[:, np.maximum(np.arange(dw) - 1, 0)], s[:, np.minimum(np.arange(dw) + 1, dw - 1)]
    out = np.empty((s.shape[0], 2 * dw), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + r0) >> sh, (3 * s + right + r1) >> sh
    return out[:H, :W]


def colour(y, cb, cr) -> np.ndarray:
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data: bytes, detail: bool = False):
    """One file -> (uint8 [H, W, 3] RGB, status); with `detail` also bool [bh, bw]: which blocks of component 0 are inside the domain."""
    p = parse(data)
    coef, status = coefficients(p)
    planes, inside = zip(*(idct(c, comp[2]) for c, comp in zip(coef, p.comps)))
    if not all(i.all() for i in inside):
        status = max(status, RANGE)
    H, W = p.height, p.width
    if len(planes) == 1:
        rgb = np.repeat(planes[0][:H, :W, None], 3, 2)
    else:
        rgb = colour(planes[0][:H, :W].astype(np.int64), upsample(planes[1], p.hmax, p.vmax, H, W), upsample(planes[2], p.hmax, p.vmax, H, W))
    return (rgb, status, inside[0]) if detail else (rgb, status)


# ---------------------------------------------------------------------------------------------------------------------
# seeded cases shared by the host and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (45, 77), (31, 2), (5, 3), (9, 4), (6, 5), (3, 6), (40, 24)]  # H x W
PIL_OPTIONS = [{}, {"optimize": True}, {"restart_marker_rows": 1}, {"restart_marker_blocks": 3}]


def images(H: int, W: int):
    """Uniform noise, a smooth ramp, a saturated magenta / green checker: uint8 [H, W, 3] each."""
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), (xx + yy) * 255 // max(H + W - 2, 1)], -1).astype(np.uint8)
    checker = np.where(((yy + xx) & 1)[..., None] > 0, np.array([255, 0, 255]), np.array([0, 255, 0])).astype(np.uint8)
    return [M.noise(H, W, 100 * H + W), ramp, checker]


def grey_image(H: int = 19, W: int = 23, seed: int = 7) -> np.ndarray:
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy * 9 + xx * 5) % 256 ^ np.random.default_rng(seed).integers(0, 32, (H, W))).astype(np.uint8)


def graded_noise(H: int = 80, W: int = 160, seed: int = 11) -> np.ndarray:
    """Grey noise whose amplitude grows from a quarter at the left edge to six sevenths at the right: blocks of every strength, so
    that scaled quantisation tables put some of them outside the IDCT's domain and leave others inside."""
    _yy, xx = np.mgrid[0:H, 0:W]
    n = np.random.default_rng(seed).integers(-128, 128, (H, W))
    return np.clip(128 + n * (xx + 32) // (W + 64), 0, 255).astype(np.uint8)


def pil_jpeg(img: np.ndarray, quality: int, subsampling: int = None, **options) -> bytes:
    import io

    from PIL import Image

    buf = io.BytesIO()
    if subsampling is not None:
        options["subsampling"] = subsampling
    Image.fromarray(img).save(buf, "JPEG", quality=quality, **options)
    return buf.getvalue()


def pil_decode(data: bytes) -> np.ndarray:
    import io

    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def segments(data: bytes):
    """[(marker, offset of its FF, offset behind the segment)] up to and including SOS."""
    out, at = [], 2
    while True:
        m, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        out.append((m, at, at + 2 + n))
        at += 2 + n
        if m == 0xDA:
            return out


def without_dht(data: bytes) -> bytes:
    """The file with its DHT segments cut out: the AVI "MJPG" convention."""
    keep, at = bytearray(data[:2]), 2
    for m, lo, hi in segments(data):
        if m != 0xC4:
            keep += data[lo:hi]
        at = hi
    return bytes(keep) + data[at:]


def scaled_dqt(data: bytes, factor: int) -> bytes:
    """Every DQT value multiplied by `factor`, capped at 255 (8-bit tables)."""
    out = bytearray(data)
    for m, lo, hi in segments(data):
        if m == 0xDB:
            for at in range(lo + 4, hi, 65):
                for i in range(at + 1, at + 65):
                    out[i] = min(out[i] * factor, 255)
    return bytes(out)


def patched_sampling(data: bytes, hv: int) -> bytes:
    """The first component's sampling byte in SOF0 replaced."""
    out = bytearray(data)
    (lo,) = [lo for m, lo, _hi in segments(data) if m == 0xC0]
    out[lo + 4 + 6 + 1] = hv
    return bytes(out)


def with_scan(data: bytes, blocks) -> bytes:
    """The one-component file `data` with its scan replaced by one assembled from syntax elements: per block a list of ('dc', v) (the
    DC difference v), ('ac', run, v), 'ZRL', 'EOB', or ('dc_symbol', s) (the DC code of symbol s, no value bits behind it).  Codes
    are the file's own tables'; the last byte is padded with 1-bits and every FF is stuffed."""
    (_h, _v, _q, dc, ac), = parse(data).comps
    dc, ac = ({sym: key for key, sym in _codes(*t).items()} for t in (dc, ac))  # symbol -> (length, code)
    bits = ""

    def put(table, symbol, v=0):
        nonlocal bits
        length, code = table[symbol]
        size = abs(v).bit_length()
        bits += format(code, f"0{length}b") + (format(v if v > 0 else v + (1 << size) - 1, f"0{size}b") if size else "")

    for block in blocks:
        for e in block:
            if e == "ZRL":
                put(ac, 0xF0)
            elif e == "EOB":
                put(ac, 0x00)
            elif e[0] == "dc":
                put(dc, abs(e[1]).bit_length(), e[1])
            elif e[0] == "ac":
                put(ac, e[1] << 4 | abs(e[2]).bit_length(), e[2])
            else:
                put(dc, e[1])
    bits += "1" * (-len(bits) % 8)
    scan = int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00")
    return data[:segments(data)[-1][2]] + scan + b"\xff\xd9"


def patched_dc_symbol(data: bytes, old: int, new: int) -> bytes:
    """The symbol `old` of every DC Huffman table replaced by `new`: the same codes, another alphabet."""
    out = bytearray(data)
    for m, lo, hi in segments(data):
        at = lo + 4
        while m == 0xC4 and at < hi:
            n = sum(data[at + 1:at + 17])
            if data[at] >> 4 == 0:
                out[at + 17 + data[at + 17:at + 17 + n].index(old)] = new
            at += 17 + n
    return bytes(out)


# A block's grammar at its edges (the law's status beside each), every one in front of an ordinary block that comes out wrong unless
# the state behind the edge is right: the last coefficient without an EOB, a ZRL that lands on 64 exactly, a ZRL past 64, a run past 63.
EDGE_TAIL = [("dc", 3), ("ac", 0, 4), ("ac", 2, -9), "EOB"]
EDGE_BLOCKS = {
    "coefficient_63_no_eob": ([("dc", 5), "ZRL", "ZRL", "ZRL", ("ac", 14, -3)], OK),
    "zrl_lands_on_64": ([("dc", 5), ("ac", 14, 2), ("ac", 15, 1), ("ac", 15, -1), "ZRL"], OK),
    "zrl_to_65": ([("dc", 5), "ZRL", "ZRL", "ZRL", "ZRL"], BAD_CODE),
    "run_past_63": ([("dc", 5), "ZRL", "ZRL", "ZRL", ("ac", 15, 1)], BAD_CODE),
    "dc_symbol_16": ([("dc_symbol", 16), "EOB"], BAD_CODE),
}


def edge_stream(name: str) -> bytes:
    """EDGE_BLOCKS[name] and EDGE_TAIL as the two blocks of an 8 x 16 grey file (dc_symbol_16: category 11 of its DC table, which no
    8-bit image needs, is renamed 16: category > 15)."""
    base = pil_jpeg(grey_image(8, 16), 90)
    if name == "dc_symbol_16":
        base = patched_dc_symbol(base, 11, 16)
    return with_scan(base, [EDGE_BLOCKS[name][0], EDGE_TAIL])


def cut_before_sos(data: bytes) -> bytes:
    return data[:[lo for m, lo, _hi in segments(data) if m == 0xDA][0]]


def cut_in_scan(data: bytes) -> bytes:
    hi = segments(data)[-1][2]
    return data[:hi + (len(data) - hi) // 2]
