"""GPU suite: a3d_jpeg_decode_split (csrc/jpeg_decode.hip), the entropy launch that cuts a unit into subsequences which synchronise
themselves, at explicit subsequence sizes through video.jpeg_decode(..., split_bytes=S, strict=False): byte for byte
tests/jpeg_decode_ref.py with status 0, for every subsequence size, and the law's status for damaged streams.  tests/jpeg_split_ref.py
(held to the law by tests/test_jpeg_split_host.py) says which fixture stresses what.  Sizes are H x W."""
import numpy as np
import pytest
import torch

import jpeg_decode_ref as D
import jpeg_split_ref as R
import mjpeg_ref as M
from test_gpu_jpeg_decode import _inference, garbage_unit, ref  # one reference per stream for both files
from test_jpeg_split_host import garbage_scan

pytestmark = pytest.mark.gpu


def gpu(jpegs, split, **kw):
    from articulation3d_amd import video

    frames, status = video.jpeg_decode(jpegs, strict=False, split_bytes=split, **kw)
    return frames.cpu().numpy(), status.tolist()


def check(jpegs, splits, **kw):
    for split in splits:
        frames, status = gpu(jpegs, split, **kw)
        for k, data in enumerate(jpegs):
            want, st = ref(data)
            assert st == D.OK and status[k] == 0 and np.array_equal(frames[k], want), (split, k)


@pytest.mark.parametrize("H,W,sub", [(1, 1, 0), (1, 1, 2), (8, 8, 0), (8, 8, 2), (16, 16, 0), (16, 16, 2)])
def test_one_pixel_one_block_one_mcu(H, W, sub):
    """The last size is above every stream's length: one subsequence, the sequential walk."""
    check([D.pil_jpeg(img, 90, sub) for img in D.images(H, W)], (1, 4, 1 << 20))


@pytest.mark.parametrize("quality", [30, 100])
@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("H,W", [(17, 33), (45, 77)])
def test_ragged_sizes_at_every_sampling(H, W, sub, quality):
    check([D.pil_jpeg(img, quality, sub) for img in D.images(H, W)], (2, 4, 8, 64))


def test_grey():
    data = D.pil_jpeg(D.grey_image(), 90)
    assert len(D.parse(data).comps) == 1
    check([data], (1, 2, 4, 8, 64))


def test_the_named_fixtures():
    """The worst case (one subsequence comes true per round, so the loop runs to its bound), an FF as the last byte of a subsequence,
    and an element that straddles a whole subsequence (an entry at or past the lane's own end)."""
    worst = D.pil_jpeg(D.images(17, 33)[2], 100, 2)
    p = D.parse(worst)
    scan, unit = R.Scan(p), R.Unit(p.units[0])
    rounds, subs = R.synchronise(scan, unit, 4)
    assert rounds >= len(subs) - 3 > 50 and any(s["ff_last"] for s in subs)
    assert any(s["entry_past_end"] for s in R.synchronise(scan, unit, 2)[1])
    check([worst], (2, 4))
    ff = D.pil_jpeg(D.images(17, 33)[0], 100, 0)
    p = D.parse(ff)
    assert any(s["ff_last"] for s in R.synchronise(R.Scan(p), R.Unit(p.units[0]), 4)[1])
    check([ff], (4,))


@pytest.mark.parametrize("sub,mcus,rows", [(0, 60, 6), (1, 30, 6), (2, 15, 3)])
def test_restart_intervals(sub, mcus, rows):
    """The four streams of test_gpu_jpeg_decode.test_restart_intervals: units shorter than a subsequence give one each, longer ones several."""
    img = D.images(45, 77)[0]
    jpegs = []
    for options, units in (({}, 1), ({"restart_marker_blocks": 3}, mcus // 3), ({"restart_marker_rows": 1}, rows), ({"restart_marker_blocks": 7}, -(-mcus // 7))):
        jpegs.append(D.pil_jpeg(img, 90, sub, **options))
        assert len(D.parse(jpegs[-1]).units) == units
    check(jpegs, (4, 64))


def test_three_frames_in_one_call_one_per_call_and_in_chunks():
    jpegs = [D.pil_jpeg(M.noise(45, 77, seed), quality, 2) for seed, quality in ((1, 90), (2, 60), (3, 98))]
    assert len({len(j) for j in jpegs}) == 3
    for split in (4, 64):
        whole, status = gpu(jpegs, split)
        assert status == [0, 0, 0]
        for k in range(3):
            assert np.array_equal(whole[k], ref(jpegs[k])[0])
            assert np.array_equal(gpu(jpegs[k:k + 1], split)[0][0], whole[k])      # F does not matter
        assert np.array_equal(gpu(jpegs, split, chunk=2)[0], whole)                # nor does the chunking


def test_different_tables_in_one_call():
    from articulation3d_amd import video

    a, b = D.pil_jpeg(M.noise(45, 77, 4), 90, 2, optimize=True), D.pil_jpeg(D.images(45, 77)[1], 90, 2, optimize=True)
    c = D.without_dht(D.pil_jpeg(M.noise(45, 77, 5), 90, 2))
    assert len({video.jpeg_parse(j).table_set() for j in (a, b, c)}) == 3
    check([a, b, c], (4, 64))


def test_status_codes_and_their_neighbours():
    """The seven-frame call of test_gpu_jpeg_decode plus a cut scan and a garbage scan without restart intervals: the law's status for
    each, nothing asked of the damaged frames' pixels, the good frames beside them exact."""
    good = [D.pil_jpeg(D.graded_noise(seed=s), 90, restart_marker_blocks=5) for s in (1, 2)]
    base = D.pil_jpeg(D.graded_noise(), 90, restart_marker_blocks=5)
    cases = {D.SHORT: D.cut_in_scan(base), D.RANGE: D.scaled_dqt(base, 14), D.BAD_CODE: garbage_unit(base)}
    for code, data in cases.items():
        assert ref(data)[1] == code
    jpegs = [good[0], cases[D.SHORT], good[1], cases[D.RANGE], good[0], cases[D.BAD_CODE], good[1]]
    plain = D.pil_jpeg(D.images(45, 77)[0], 90, 2)
    loose = [plain, D.cut_in_scan(plain), garbage_scan(), plain, garbage_scan(2)]  # no restart intervals
    assert [ref(j)[1] for j in loose] == [0, D.SHORT, D.BAD_CODE, 0, 0]
    for split in (4, 64):
        frames, status = gpu(jpegs, split, chunk=8)
        assert status == [0, D.SHORT, 0, D.RANGE, 0, D.BAD_CODE, 0]
        for k in (0, 2, 4, 6):
            assert np.array_equal(frames[k], ref(jpegs[k])[0])
        frames, status = gpu(loose, split, chunk=8)
        assert status == [0, D.SHORT, D.BAD_CODE, 0, 0]
        for k in (0, 3, 4):  # the last one is noise the law decodes to the end without an inconsistency: its pixels are the law's too
            assert np.array_equal(frames[k], ref(loose[k])[0])


def test_real_sizes_equal_pil():
    """480 x 640 at 4:2:0 and 480 x 2560 at 4:4:4, quality 90, no restart intervals, at the default subsequence size (the second
    scan is long enough for the size to be raised above it).  The law in numpy takes minutes here; tests/test_jpeg_decode_host.py
    holds it to PIL byte for byte, so PIL stands for it."""
    from articulation3d_amd import _lib, video

    assert video.JPEG_SPLIT_BYTES == _lib.JPEG_SPLIT_BYTES == 32
    for H, W, sub in ((480, 640, 2), (480, 2560, 0)):
        data = D.pil_jpeg(M.smooth_frames(1, H, W)[0], 90, sub)
        info = video.jpeg_parse(data)
        assert info.restart == 0 and (sub == 2 or info.scan[1] - info.scan[0] > 1024 * video.JPEG_SPLIT_BYTES)
        got, status = video.jpeg_decode([data], strict=False)
        assert status.tolist() == [0] and np.array_equal(got[0].cpu().numpy(), D.pil_decode(data))


@pytest.mark.parametrize("name", list(D.EDGE_BLOCKS))
def test_grammar_edges(name):
    """Scans assembled from syntax elements (tests/test_jpeg_split_host.py holds the law's status and the model on them): the kernel
    equals the law, status and, where that is 0, bytes, at sizes that cut these 8 .. 17 byte units, above them, and at the default."""
    data = D.edge_stream(name)
    want, want_status = ref(data)
    assert want_status == D.EDGE_BLOCKS[name][1]
    for split in (1, 2, 4, 64, None):
        frames, status = gpu([data], split)
        assert status == [want_status], split
        assert want_status != D.OK or np.array_equal(frames[0], want), split


def test_bad_split_sizes_are_refused_before_any_launch():
    from articulation3d_amd import opt_ops, video

    data = D.pil_jpeg(M.noise(16, 16, 1), 90, 2)
    info = video.jpeg_parse(data)
    piece = data[info.scan[0]:info.scan[1]]
    n = len(piece)
    sets = np.frombuffer(info.table_set(), np.uint8)[None].copy()
    dev_data = torch.from_numpy(np.frombuffer(piece + bytes(-n % 4 + 4), np.uint8).copy()).cuda()
    ce, pe = opt_ops.jpeg_decode_scratch(16, 16, 3, 2, 2)
    coef, planes = torch.empty(ce, dtype=torch.int16, device="cuda"), torch.empty(pe, dtype=torch.uint8, device="cuda")
    rgb = torch.full((1, 16, 16, 3), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    meta = np.array([0, n, 0, 1, 0, 0], np.int32)

    def call(split, nbytes=n):
        opt_ops.jpeg_decode_into(rgb, status, dev_data, nbytes, meta, torch.from_numpy(meta).cuda(), sets, torch.from_numpy(sets).cuda(), 1, 3, 2, 2, coef,
                                 planes, split)

    with pytest.raises(RuntimeError, match="a3d_jpeg_decode_split failed with A3D_ERR_ARG"):
        call(-1)
    with pytest.raises(RuntimeError, match="a3d_jpeg_decode_split failed with A3D_ERR_ARG"):
        call(4, nbytes=n - 1)  # the descriptor's own cases hold here too: offsets that do not end at data_bytes
    with pytest.raises(RuntimeError, match="a3d_jpeg_decode_split failed with A3D_ERR_ARG"):
        call(0)
    with pytest.raises(ValueError, match="split_bytes"):
        video.jpeg_decode([data], split_bytes=0)
    torch.cuda.synchronize()
    assert (rgb == 0x5A).all() and status.tolist() == [-7]
    call(4)
    assert status.tolist() == [0] and np.array_equal(rgb[0].cpu().numpy(), ref(data)[0])


def test_the_tool_decodes_a_folder_of_plain_files_on_the_gpu(monkeypatch):
    """PIL's default output (no restart intervals) through tools/inference.py's decode_images under --decoder gpu: PIL's bytes, by
    one GPU call."""
    frames = M.smooth_frames(3, 96, 128)
    blobs = [D.pil_jpeg(fr, 90) for fr in frames]
    from articulation3d_amd import video

    assert all(video.jpeg_parse(b).restart == 0 for b in blobs)
    real, calls = video.jpeg_decode, []
    monkeypatch.setattr(video, "jpeg_decode", lambda *a, **kw: calls.append(real(*a, **kw)) or calls[-1])
    got = _inference().decode_images(blobs, "gpu")
    (frames, status), = calls
    assert status.tolist() == [0, 0, 0] and np.array_equal(frames.cpu().numpy(), got)
    assert got.dtype == np.uint8 and np.array_equal(got, np.stack([D.pil_decode(b) for b in blobs]))
