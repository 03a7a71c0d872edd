"""CPU suite: the PNG law of tests/png_ref.py and the host half of the encoder (articulation3d_amd/png.py: huffman_lengths,
dynamic_header, adler_fold, the container) against independent decoders -- zlib's inflate, zlib's checksums and PIL -- on fixtures of at
most ~100 KB.  The fixture set has to reach every branch of the law; the test checks that it does."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import png_ref as R
from articulation3d_amd import png as P

FIXTURES = {
    "flat": lambda: R.flat(40, 86),
    "black": lambda: R.flat(40, 86, (0, 0, 0)),  # filter None, so the zeros run through the type bytes and across the segment boundary
    "one_pixel": lambda: R.noise(1, 1, 1),
    "hramp": lambda: R.hramp(50, 200),
    "vramp": lambda: R.vramp(60, 120),
    "repeated_rows": lambda: R.repeated_rows(70, 100),
    "period3": lambda: R.period3(40, 150),
    "camera": lambda: R.camera(64, 256),
    "noise": lambda: R.noise(48, 180, 3),
    "mixed": lambda: R.mixed(90, 160),
    "one_row_per_segment": lambda: R.mixed(5, 2731),
}
_STAGES = {}


def stages(name):
    """Computed once per fixture and shared, never changed."""
    if name not in _STAGES:
        img = FIXTURES[name]()
        assert img.nbytes <= 160 * 1024
        _STAGES[name] = (img, R.encode_stages(img))
    return _STAGES[name]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_independent_decoders_read_the_law(name):
    img, st = stages(name)
    H, W, _ = img.shape
    decoded = Image.open(io.BytesIO(st["file"]))
    assert decoded.mode == "RGB" and np.array_equal(np.asarray(decoded), img)          # lossless, by PIL
    chunks = R.chunks(st["file"])
    assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"] and all(ok for _k, _d, ok in chunks)
    idat = chunks[1][1]
    filt = st["filt"].tobytes()
    assert zlib.decompress(idat) == filt                                               # zlib checks the Adler-32 itself
    assert idat[:2] == b"\x78\x01" and idat[-6:-4] == b"\x03\x00" and int.from_bytes(idat[-4:], "big") == zlib.adler32(filt)
    assert np.array_equal(R.unfilter(st["filt"], H, W), img)                           # the filtered bytes, by the standard's reconstruction
    stride, _R, S, segs = R.geometry(H, W)
    assert len(st["segments"]) == S
    from articulation3d_amd import _lib

    for (a, n), seg, toks in zip(segs, st["segments"], st["tokens"]):
        assert len(seg) <= n + 5 and len(seg) <= R.slot_bytes(W) == _lib.lib().a3d_png_slot_bytes(W)
        assert sum(L for _i, L, _d in toks) == n
        # every segment stands alone behind the window: inflate it with the frame's bytes before it as the dictionary
        d = zlib.decompressobj(-15, zdict=filt[max(0, a - 32768):a]) if a else zlib.decompressobj(-15)
        assert d.decompress(seg + b"\x03\x00") == filt[a:a + n] and d.eof
    # the host's fold of the per-segment sums is zlib's Adler-32
    s1 = [int(st["filt"][a:a + n].astype(np.uint64).sum()) for a, n in segs]
    s2 = [int((st["filt"][a:a + n].astype(np.uint64) * np.arange(n, 0, -1, dtype=np.uint64)).sum()) for a, n in segs]
    assert P.adler_fold(s1, s2, [n for _a, n in segs]) == zlib.adler32(filt)
    assert P.png_file(H, W, st["deflate"], zlib.adler32(filt)) == st["file"]          # the package's container is the law's


def test_the_fixtures_reach_every_branch_of_the_law():
    types, kinds, dists = set(), set(), set()
    exact_258 = cut = previous = False
    for name in FIXTURES:
        img, st = stages(name)
        H, W, _ = img.shape
        filt = st["filt"]
        stride, _R, _S, segs = R.geometry(H, W)
        types |= set(st["types"].tolist())
        kinds |= set(st["kinds"])
        for (a, n), toks in zip(segs, st["tokens"]):
            for i, L, d in toks:
                if d == 0:
                    continue
                dists.add(1 if d == 1 else 3 if d == 3 else "stride")
                assert d in (1, 3, stride) and 3 <= L <= 258 and a + i - d >= 0
                exact_258 |= L == 258
                cut |= i + L == n and L < 258 and a + n < filt.size and filt[a + n] == filt[a + n - d]
                previous |= i - d < 0
    assert types == {0, 1, 2, 3, 4}
    assert kinds == {0, 1, 2}
    assert dists == {1, 3, "stride"}
    assert exact_258 and cut and previous


def test_noise_is_stored_and_camera_content_takes_the_frames_code():
    assert set(stages("noise")[1]["kinds"]) == {0}
    assert set(stages("camera")[1]["kinds"]) == {2}


def _kraft(lengths):
    return sum(2.0 ** -l for l in lengths if l)


def _inflate_header_only(litlen, dist):
    """A dynamic block that holds nothing but its header and the end of block, then the final empty fixed block: zlib must take it."""
    bits, n = P.dynamic_header(litlen, dist)
    b = P._Bits()
    b.put(bits, n)
    b.put_code(P.canonical_codes(litlen)[256], litlen[256])
    b.put(3, 3)   # BFINAL 1, BTYPE 01
    b.put(0, 7)   # the fixed code's end of block
    return zlib.decompress(b.value.to_bytes((b.n + 7) // 8, "little"), -15)


def test_huffman_lengths_kraft_and_limits():
    rng = np.random.default_rng(11)
    for trial in range(20):
        counts = rng.integers(0, 1000, 286) * (rng.random(286) < rng.random())
        counts[256] = 1
        counts[int(rng.integers(0, 256))] += 1
        lengths = P.huffman_lengths(counts)
        assert all((l > 0) == (c > 0) for l, c in zip(lengths, counts)) and max(lengths) <= 15 and _kraft(lengths) == 1.0
    # Fibonacci weights: the plain tree is 39 deep; the halving brings it inside 15 bits with Kraft equality intact
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    skew = [0] * 286
    skew[100:140] = fib
    skew[256] = 1
    assert max(P.huffman_lengths(skew, 64)) > 15
    limited = P.huffman_lengths(skew, 15)
    assert max(limited) == 15 and _kraft(limited) == 1.0 and all((l > 0) == (c > 0) for l, c in zip(limited, skew))
    assert _inflate_header_only(limited, P.distance_lengths([0] * 30)) == b""
    # ties: equal weights give a balanced code, lower symbols never longer than higher ones
    assert P.huffman_lengths([1] * 8) == [3] * 8 and P.huffman_lengths([1, 1, 1]) == [2, 2, 1] and P.huffman_lengths([5, 0, 0]) == [1, 0, 0]
    # the code-length code's own limit
    assert max(P.huffman_lengths(fib[:19], 7)) == 7 and _kraft(P.huffman_lengths(fib[:19], 7)) == 1.0


def test_distance_codes_zlib_accepts():
    lit = [0] * 286
    lit[65], lit[256], lit[260] = 5, 1, 2
    litlen = P.huffman_lengths(lit)
    none = P.distance_lengths([0] * 30)
    assert none == [1] + [0] * 29 and _inflate_header_only(litlen, none) == b""
    one = [0] * 30
    one[27] = 9
    assert P.distance_lengths(one)[27] == 1 and sum(P.distance_lengths(one)) == 1 and _inflate_header_only(litlen, P.distance_lengths(one)) == b""
    three = [0] * 30
    three[0], three[2], three[26] = 7, 2, 2
    assert _kraft(P.distance_lengths(three)) == 1.0 and _inflate_header_only(litlen, P.distance_lengths(three)) == b""


def test_every_header_of_the_fixtures_and_of_random_histograms_is_accepted_by_zlib():
    for name in FIXTURES:
        st = stages(name)[1]
        assert _inflate_header_only(st["litlen"], st["dist"]) == b""
        tab = P.frame_table(st["hist"])
        bits, n = P.dynamic_header(st["litlen"], st["dist"])
        assert tab.dtype == np.uint32 and tab.size == P.TAB_WORDS and int(tab[P.SYMS]) == n <= 32 * (P.TAB_WORDS - P.HDR_AT)
        assert int.from_bytes(tab[P.HDR_AT:].tobytes(), "little") == bits
        codes = P.canonical_codes(st["litlen"]) + P.canonical_codes(st["dist"])
        for s, l in enumerate(st["litlen"] + st["dist"]):
            assert int(tab[s]) >> 16 == l and (int(tab[s]) & 0xFFFF) == P.bit_reverse(codes[s], l)
    rng = np.random.default_rng(12)
    for trial in range(30):
        hist = (rng.integers(0, 5000, 316) * (rng.random(316) < rng.random())).astype(np.int64)
        hist[256] = 1 + trial
        hist[int(rng.integers(0, 256))] += 1
        hist[286:] *= np.isin(np.arange(30), (0, 2, int(rng.integers(3, 28))))  # the encoder's three distances
        litlen, dist = P.frame_code(hist)
        assert _inflate_header_only(litlen, dist) == b""


def test_adler_fold_is_zlibs():
    rng = np.random.default_rng(13)
    data = rng.integers(0, 256, 70000, dtype=np.uint8)
    data[:20000] = 255  # the sums' largest terms
    cuts = [0, 1, 16385, 16385, 32769, 49153, 70000]  # an empty piece included
    pieces = [data[a:b].astype(np.uint64) for a, b in zip(cuts, cuts[1:])]
    s1 = [int(p.sum()) for p in pieces]
    s2 = [int((p * np.arange(p.size, 0, -1, dtype=np.uint64)).sum()) for p in pieces]
    assert P.adler_fold(s1, s2, [p.size for p in pieces]) == zlib.adler32(data.tobytes())
    assert P.adler_fold([], [], []) == 1


def test_geometry_is_the_stated_rule():
    for H, W in ((1, 1), (3, 86), (40, 86), (9, 640), (5, 2731), (3, 5461), (480, 2560)):
        stride, Rr, S, segs = R.geometry(H, W)
        assert P.geometry(H, W) == (stride, Rr, S) and stride <= 16384
        assert all(n <= 16384 for _a, n in segs) and all(n >= 8192 for _a, n in segs[:-1]) and sum(n for _a, n in segs) == H * stride
    for bad in ((0, 4), (65536, 4), (4, 0), (4, 5462)):
        with pytest.raises(ValueError):
            P.geometry(*bad)


def test_the_tool_chooses_the_encoder():
    """--png-encoder: `gpu` and `pil` as told; `auto` the GPU on a CUDA device for rows the encoder takes (MEASUREMENTS.md, "PNG encode")."""
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("a3d_tools_inference_png", os.path.join(root, "tools", "inference.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--config", "c.yaml", "--input", "synthetic:3", "--output", "o"]
    assert cli.build_parser().parse_args(base).png_encoder == "auto"
    assert cli.build_parser().parse_args(base + ["--vis", "png", "--png-encoder", "pil"]).png_encoder == "pil"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--png-encoder", "zlib"])
    assert cli.PNG_AUTO_GPU is True
    assert cli.png_on_gpu("auto", "cuda:0", 2560) and not cli.png_on_gpu("auto", "cpu", 2560) and not cli.png_on_gpu("auto", "cuda", 5462)
    assert cli.png_on_gpu("gpu", "cpu", 9999) and not cli.png_on_gpu("pil", "cuda", 2560)
