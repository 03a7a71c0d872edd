"""GPU suite: the JPEG decode kernels (a3d_jpeg_decode, csrc/jpeg_decode.hip) against tests/jpeg_decode_ref.py, the law in numpy -- byte
for byte, every frame of a call -- then the host path over them (jpeg_decode, MJPEGReader) and tools/inference.py reading an .avi.
Sizes are H x W."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_decode_ref as D
import mjpeg_ref as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def ref(data: bytes):
    """(pixels, status) of the law, computed once per stream."""
    if data not in _REF:
        _REF[data] = D.decode(data)
    return _REF[data]


def gpu(jpegs, **kw):
    from articulation3d_amd import video

    frames, status = video.jpeg_decode(jpegs, strict=False, **kw)
    return frames.cpu().numpy(), status.tolist()


def check(jpegs, **kw):
    frames, status = gpu(jpegs, **kw)
    for k, data in enumerate(jpegs):
        want, st = ref(data)
        assert st == D.OK and status[k] == 0 and np.array_equal(frames[k], want), k


@pytest.mark.parametrize("H,W,sub", [(1, 1, 0), (1, 1, 2), (8, 8, 0), (16, 16, 2)])
def test_one_pixel_one_block_one_mcu(H, W, sub):
    for img in D.images(H, W):
        check([D.pil_jpeg(img, 90, sub)])


@pytest.mark.parametrize("quality", [30, 100])
@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("H,W", [(17, 33), (45, 77)])
def test_ragged_sizes_at_every_sampling(H, W, sub, quality):
    """Quality 100 on noise reaches 16-bit codes and stuffed FF bytes; the checker saturates the colour conversion."""
    jpegs = [D.pil_jpeg(img, quality, sub) for img in D.images(H, W)]
    if quality == 100:
        assert b"\xff\x00" in jpegs[0][600:]
    check(jpegs)


@pytest.mark.parametrize("sub", [1, 2])
@pytest.mark.parametrize("H,W", [(31, 2), (5, 3), (9, 4)])
def test_narrow_chroma_and_odd_heights(H, W, sub):
    check([D.pil_jpeg(img, 90, sub) for img in D.images(H, W)])


def test_grey():
    data = D.pil_jpeg(D.grey_image(), 90)
    assert len(D.parse(data).comps) == 1
    check([data])


@pytest.mark.parametrize("sub,mcus,rows", [(0, 60, 6), (1, 30, 6), (2, 15, 3)])
def test_restart_intervals(sub, mcus, rows):
    """45 x 77 is 10 x 6, 5 x 6 or 5 x 3 MCUs: no interval; 3 MCUs (not aligned with the rows; at 4:4:4 the 20 units make the marker
    counter wrap); one MCU row; 7 MCUs (a short last interval)."""
    img = D.images(45, 77)[0]
    jpegs = []
    for options, units in (({}, 1), ({"restart_marker_blocks": 3}, mcus // 3), ({"restart_marker_rows": 1}, rows), ({"restart_marker_blocks": 7}, -(-mcus // 7))):
        jpegs.append(D.pil_jpeg(img, 90, sub, **options))
        assert len(D.parse(jpegs[-1]).units) == units and mcus % 7
    check(jpegs)


def test_a_frame_of_the_encoders_law():
    check([M.encode_frame(M.noise(77, 45, 1), 100)])


def test_three_frames_in_one_call_one_per_call_and_in_chunks():
    jpegs = [D.pil_jpeg(M.noise(45, 77, seed), 90, 2, restart_marker_rows=1) for seed in (1, 2, 3)]
    whole, status = gpu(jpegs)
    assert status == [0, 0, 0]
    for k in range(3):
        assert np.array_equal(whole[k], ref(jpegs[k])[0])
        assert np.array_equal(gpu(jpegs[k:k + 1])[0][0], whole[k])           # F does not matter
    assert np.array_equal(gpu(jpegs, chunk=2)[0], whole)                      # nor does the chunking


def test_different_tables_in_one_call():
    """Two frames with their own optimised Huffman tables and one without any DHT segment: three table sets in one call."""
    from articulation3d_amd import video

    a, b = D.pil_jpeg(M.noise(45, 77, 4), 90, 2, optimize=True), D.pil_jpeg(D.images(45, 77)[1], 90, 2, optimize=True)
    c = D.without_dht(D.pil_jpeg(M.noise(45, 77, 5), 90, 2))
    assert len({video.jpeg_parse(j).table_set() for j in (a, b, c)}) == 3
    check([a, b, c])


def test_a_pitched_destination_keeps_the_bytes_beside_it():
    """The frames land in the right part of wider rows: 77 columns behind 19 (byte stores), and 64 columns behind 16 (the 16-byte
    stores, on rows that are not dense); the columns in front keep their bytes."""
    from articulation3d_amd import opt_ops, video

    for W, pad in ((77, 19), (64, 16)):
        jpegs = [D.pil_jpeg(M.noise(45, W, s), 90, 2) for s in (1, 2)]
        infos = [video.jpeg_parse(j) for j in jpegs]
        wide = torch.full((2, 45, pad + W, 3), 0x5A, dtype=torch.uint8, device="cuda")
        status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        pieces = [j[i.scan[0]:i.scan[1]] for j, i in zip(jpegs, infos)]
        off = [0, len(pieces[0]), len(pieces[0]) + len(pieces[1])]
        meta = np.array(off + [0, 1, 2] + [0, 0] + [0, 0], np.int32)
        sets = np.frombuffer(infos[0].table_set(), np.uint8)[None].copy()
        assert infos[1].table_set() == infos[0].table_set()
        data = np.frombuffer(b"".join(pieces) + bytes(-off[2] % 4 + 4), np.uint8).copy()
        ce, pe = opt_ops.jpeg_decode_scratch(45, W, 3, 2, 2)
        coef, planes = torch.empty(2 * ce, dtype=torch.int16, device="cuda"), torch.empty(2 * pe, dtype=torch.uint8, device="cuda")
        opt_ops.jpeg_decode_into(wide[:, :, pad:], status, torch.from_numpy(data).cuda(), off[2], meta, torch.from_numpy(meta).cuda(), sets,
                                 torch.from_numpy(sets).cuda(), 2, 3, 2, 2, coef, planes)
        got = wide.cpu().numpy()
        assert status.tolist() == [0, 0] and (got[:, :, :pad] == 0x5A).all()
        for k in range(2):
            assert np.array_equal(got[k, :, pad:], ref(jpegs[k])[0])


def garbage_unit(data: bytes) -> bytes:
    """The file with the first 24 bytes of its third unit replaced by FF-free noise (most such noise decodes to something; this seed is
    one the law answers with BAD_CODE, which the caller asserts)."""
    from articulation3d_amd import video

    lo, hi = video.jpeg_parse(data).units[2]
    assert hi - lo > 24
    noise = bytes(int(v) for v in np.random.default_rng(2).integers(0, 255, 24))
    return data[:lo] + noise + data[lo + 24:]


def test_status_codes_and_their_neighbours():
    """A file cut in its scan is SHORT, one with scaled quantisation tables RANGE, one with a unit of garbage BAD_CODE (the law says so
    for each); nothing is asked of their pixels, and the frames beside them in the same call stay exact."""
    good = [D.pil_jpeg(D.graded_noise(seed=s), 90, restart_marker_blocks=5) for s in (1, 2)]
    base = D.pil_jpeg(D.graded_noise(), 90, restart_marker_blocks=5)
    cases = {D.SHORT: D.cut_in_scan(base), D.RANGE: D.scaled_dqt(base, 14), D.BAD_CODE: garbage_unit(base)}
    for code, data in cases.items():
        assert ref(data)[1] == code
    jpegs = [good[0], cases[D.SHORT], good[1], cases[D.RANGE], good[0], cases[D.BAD_CODE], good[1]]
    frames, status = gpu(jpegs, chunk=8)
    assert status == [0, D.SHORT, 0, D.RANGE, 0, D.BAD_CODE, 0]
    for k in (0, 2, 4, 6):
        assert np.array_equal(frames[k], ref(jpegs[k])[0])
    from articulation3d_amd import video

    with pytest.raises(ValueError, match="frame 1: status SHORT"):
        video.jpeg_decode(jpegs)
    colour = D.cut_in_scan(D.pil_jpeg(D.images(45, 77)[0], 90, 2))  # a scan without restart intervals, cut
    assert ref(colour)[1] == D.SHORT and gpu([colour])[1] == [D.SHORT]


def test_bad_descriptors_are_refused_before_any_launch():
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

    def call(meta, sets=sets, nbytes=n, hs=2, vs=2, n_units=1):
        meta = np.array(meta, np.int32)
        opt_ops.jpeg_decode_into(rgb, status, dev_data, nbytes, meta, torch.from_numpy(meta).cuda(), sets, torch.from_numpy(sets).cuda(), n_units, 3, hs,
                                 vs, coef, planes)

    oversubscribed = sets.copy()
    oversubscribed[0, 192] = 3  # three codes of one bit
    for kw in (dict(meta=[0, n, 0, 1, 0, 1]),                       # table index out of range
               dict(meta=[0, n, 0, 1, -1, 0]),                      # negative restart interval
               dict(meta=[0, n, n, 0, 2, 0, 0], n_units=2),         # two units where the geometry asks for one
               dict(meta=[4, n, 0, 1, 0, 0]),                       # offsets do not start at 0
               dict(meta=[0, n + 4, n, 0, 2, 0, 0], n_units=2),     # not monotonic
               dict(meta=[0, n, 0, 1, 0, 0], nbytes=n - 1),         # offsets do not end at data_bytes
               dict(meta=[0, n, 0, 1, 0, 0], sets=oversubscribed)):
        with pytest.raises(RuntimeError, match="A3D_ERR_ARG"):
            call(**kw)
    with pytest.raises(ValueError):
        call([0, n, 0, 1, 0, 0], hs=1, vs=2)
    with pytest.raises(ValueError):
        opt_ops.jpeg_decode_scratch(16, 70000, 3, 1, 1)
    torch.cuda.synchronize()
    assert (rgb == 0x5A).all() and status.tolist() == [-7]
    call([0, n, 0, 1, 0, 0])
    assert status.tolist() == [0] and np.array_equal(rgb[0].cpu().numpy(), ref(data)[0])
    with pytest.raises(ValueError, match="frame 1 is"):
        video.jpeg_decode([data, D.pil_jpeg(M.noise(16, 16, 1), 90, 0)])
    with pytest.raises(ValueError, match="frame 0: progressive"):
        video.jpeg_decode([D.pil_jpeg(M.noise(16, 16, 1), 90, 0, progressive=True)])


def test_round_trip_through_the_encoder():
    from articulation3d_amd import video

    frames = np.stack([M.noise(77, 45, 8), M.structured()])
    jpegs = video.jpeg_encode(torch.from_numpy(frames).cuda(), 90)
    got = video.jpeg_decode(jpegs).cpu().numpy()
    for k in range(2):
        want, status = ref(jpegs[k])
        assert status == D.OK and np.array_equal(got[k], want)
        assert M.psnr(got[k], frames[k]) > (25 if k == 0 else 30)


def _clip(tmp_path, H=96, W=128):
    from articulation3d_amd.video import MJPEGWriter

    frames = M.smooth_frames(4, H, W)
    jpegs = [D.pil_jpeg(frames[0], 90, 2), D.pil_jpeg(frames[1], 90, 2, restart_marker_rows=1), D.without_dht(D.pil_jpeg(frames[2], 90, 2)),
             D.pil_jpeg(frames[3], 90, 2, optimize=True)]
    path = str(tmp_path / "clip.avi")
    with MJPEGWriter(path, W, H, "30000/1001") as w:
        for j in jpegs:
            w.write(j)
    return path, jpegs


def _inference():
    spec = importlib.util.spec_from_file_location("a3d_tools_inference", os.path.join(ROOT, "tools", "inference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_read_frames_of_an_avi_under_every_decoder(tmp_path):
    path, jpegs = _clip(tmp_path)
    tool = _inference()
    want = np.stack([D.pil_decode(j) for j in jpegs])
    assert tool.count_frames(path) == 4
    for decoder in ("gpu", "pil", "auto"):
        got = tool.read_frames(path, decoder=decoder)
        assert got.dtype == np.uint8 and np.array_equal(got, want), decoder
    assert np.array_equal(tool.read_frames(path, 1, 3, decoder="gpu"), want[1:3])
    assert tool.read_frames(path, 4, 4).shape == (0, 96, 128, 3)
    folder = tmp_path / "frames"
    folder.mkdir()
    from PIL import Image

    for k, j in enumerate(jpegs[:2]):
        (folder / f"{k}.jpg").write_bytes(j)
    (folder / "2.jpg").write_bytes(D.pil_jpeg(M.smooth_frames(4, 96, 128)[2], 90, 2, progressive=True))  # refused by the parser: PIL
    Image.fromarray(want[3]).save(folder / "3.png")
    for decoder in ("gpu", "pil", "auto"):
        got = tool.read_frames(str(folder), decoder=decoder)
        assert np.array_equal(got[[0, 1, 3]], want[[0, 1, 3]]) and np.array_equal(got[2], D.pil_decode((folder / "2.jpg").read_bytes()))


def test_inference_script_reads_an_avi(tmp_path):
    path, _jpegs = _clip(tmp_path)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "tools/inference.py", "--config", "configs/planercnn_inference.yaml", "--input", path, "--output", str(out),
                        "--random-init", "--calibrate-bn", "--conf-threshold", "0.3", "--batch", "2", "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.3"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(json.load(open(out / "predictions.json"))) == 4
