"""Host suite of the self-synchronising entropy stage: tests/jpeg_split_ref.py (the scheme a3d_jpeg_decode_split's entropy kernel runs,
as a host model) is held to tests/jpeg_decode_ref.coefficients, the law's sequential walk -- coefficient planes and status, exactly, for
every subsequence size -- and the fixtures the GPU tests lean on are shown to stress what they are named for.  Sizes are H x W."""
import numpy as np
import pytest

import jpeg_decode_ref as D
import jpeg_split_ref as R
import mjpeg_ref as M

SPLITS = (2, 4, 8, 64, 1 << 20)  # the last one is longer than every stream here: one subsequence, the sequential walk
_LAW = {}


def law(data: bytes):
    if data not in _LAW:
        _LAW[data] = D.coefficients(D.parse(data))
    return _LAW[data]


def hold(data: bytes, splits=SPLITS, status=None):
    """The model equals the law on this stream at every subsequence size; -> {split: (rounds, per unit its subsequences)}."""
    want, want_status = law(data)
    assert status is None or want_status == status
    out = {}
    for split in splits:
        got, got_status, rounds, record = R.decode(D.parse(data), split)
        assert got_status == want_status, (split, got_status, want_status)
        for c, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), (split, c)
        out[split] = (rounds, record)
    return out


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("H,W", [(1, 1), (8, 8), (16, 16), (17, 33), (45, 77)])
def test_every_sampling_size_and_quality(H, W, sub):
    for img in D.images(H, W):
        for quality in (30, 90, 100):
            hold(D.pil_jpeg(img, quality, sub), (1,) + SPLITS if H == 1 else SPLITS)


def test_grey():
    for quality in (30, 90, 100):
        data = D.pil_jpeg(D.grey_image(), quality)
        assert len(D.parse(data).comps) == 1
        hold(data, (1,) + SPLITS)


def test_optimised_tables_and_no_tables():
    img = D.images(45, 77)[0]
    for sub in (0, 2):
        hold(D.pil_jpeg(img, 90, sub, optimize=True))
        bare = D.without_dht(D.pil_jpeg(img, 90, sub))
        assert 0xC4 not in [m for m, _lo, _hi in D.segments(bare)]
        hold(bare)


@pytest.mark.parametrize("sub,mcus", [(0, 60), (1, 30), (2, 15)])
def test_restart_intervals(sub, mcus):
    """3 MCUs, one MCU row, 7 MCUs (a short last interval): units shorter than a subsequence give one each, longer ones several."""
    img = D.images(45, 77)[0]
    for options, units in (({"restart_marker_blocks": 3}, mcus // 3), ({"restart_marker_rows": 1}, 6 if sub < 2 else 3), ({"restart_marker_blocks": 7}, -(-mcus // 7))):
        data = D.pil_jpeg(img, 90, sub, **options)
        assert len(D.parse(data).units) == units
        seen = hold(data)
        assert max(len(u) for u in seen[4][1]) > 1 and all(len(u) == 1 for u in seen[1 << 20][1])


def garbage(data: bytes, unit: int, seed: int, n: int = 24) -> bytes:
    """The file with the first n bytes of a unit replaced by FF-free noise."""
    lo = D.segments(data)[-1][2]
    for k, m in enumerate(D._RST.finditer(data, lo)):
        if k + 1 == unit:
            lo = m.end()
    noise = bytes(int(v) for v in np.random.default_rng(seed).integers(0, 255, n))
    return data[:lo] + noise + data[lo + n:]


def garbage_scan(seed: int = 4) -> bytes:
    """A 45 x 77 4:2:0 scan without restart intervals with 24 bytes of noise a quarter of the way in (most such noise decodes to
    something: the law answers seed 4 with BAD_CODE and seeds 2, 3 and 10 with 0, which the callers assert)."""
    data = D.pil_jpeg(D.images(45, 77)[0], 90, 2)
    lo = D.segments(data)[-1][2]
    at = lo + (len(data) - lo) // 4
    noise = bytes(int(v) for v in np.random.default_rng(seed).integers(0, 255, 24))
    return data[:at] + noise + data[at + 24:]


def test_damaged_streams():
    base = D.pil_jpeg(D.graded_noise(), 90, restart_marker_blocks=5)
    hold(D.cut_in_scan(base), status=D.SHORT)
    hold(garbage(base, 2, 2), status=D.BAD_CODE)                      # test_gpu_jpeg_decode.garbage_unit: the third unit
    hold(D.cut_in_scan(D.pil_jpeg(D.images(45, 77)[0], 90, 2)), status=D.SHORT)
    assert D.parse(garbage_scan()).restart == 0
    hold(garbage_scan(), status=D.BAD_CODE)
    hold(garbage_scan(2), (4, 64), status=D.OK)  # noise the law decodes to the end: wrong pixels, no inconsistency
    for seed in range(5, 9):  # whatever the law makes of other noise, the model makes the same
        hold(garbage_scan(seed), (4, 64))


@pytest.mark.parametrize("name", list(D.EDGE_BLOCKS))
def test_grammar_edges(name):
    """Scans assembled from syntax elements (D.with_scan): the law's status at every edge of a block's grammar, PIL's bytes where it is
    0, and the model equal to the law at sizes that cut the 8 .. 17 bytes of these units.  video.jpeg_parse and the library accept a DC
    table that lists the symbol 16, so dc_symbol_16 runs like the others."""
    data = D.edge_stream(name)
    p = D.parse(data)
    assert (p.height, p.width, len(p.comps), len(p.units)) == (8, 16, 1, 1) and 8 <= len(p.units[0]) <= 17
    rgb, status = D.decode(data)
    assert status == D.EDGE_BLOCKS[name][1]
    if status == D.OK:
        assert np.array_equal(rgb, D.pil_decode(data))
        first, second = law(data)[0][0][0]
        assert first[63] == (-3 if name == "coefficient_63_no_eob" else 0) and list(second[[0, 1, 9]]) == [8, 4, -9]
    hold(data, (1, 2, 4, 64), status=D.EDGE_BLOCKS[name][1])


def test_the_fixtures_stress_what_they_are_named_for():
    worst = D.pil_jpeg(D.images(17, 33)[2], 100, 2)
    seen = hold(worst, (2, 4))
    rounds, (subs,) = seen[4]
    assert len(subs) > 50 and rounds >= len(subs) - 3                    # the worst case: one subsequence comes true per round
    assert any(s["ff_last"] for s in subs)                                # an FF as the last byte of a subsequence
    assert any(s["entry_past_end"] for s in seen[2][1][0])               # an element that straddles a whole subsequence
    assert any(s["ff_last"] for img in D.images(17, 33) for s in hold(D.pil_jpeg(img, 100, 0), (4,))[4][1][0])


def test_a_real_frame_synchronises_in_a_few_rounds():
    """480 x 640 at 4:2:0, quality 90, no restart intervals: the rounds and every subsequence's entry state are held to ONE continuing
    walk of the same model (the law's own walk takes minutes at this size; the GPU test holds the pixels to PIL)."""
    p = D.parse(D.pil_jpeg(M.smooth_frames(1)[0], 90, 2))
    scan, unit = R.Scan(p), R.Unit(p.units[0])
    rounds, subs = R.synchronise(scan, unit, 128)
    assert len(subs) > 100 and rounds <= 10
    assert [s["entry"] for s in subs] == R.sequential(scan, unit, 128)
    assert all(s["bad_at"] is None for s in subs[:-1])
