"""GPU suite: a3d_render_panels (csrc/render.hip) against tests/render_ref.py, the law in numpy -- bit for bit -- then the host
path over it (render_panels, render_clip's double-buffered copies) and one run of tools/inference.py --vis npy."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


def _case(H, W, counts, seed, mask_alpha=0.5):
    """Seeded frames + hand-made Instances (counts[f] detections in frame f) + their tables, normals and bit masks on the host."""
    from articulation3d_amd import render

    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (len(counts), H, W, 3), dtype=np.uint8)
    preds = [R.make_instances(rng, H, W, n) for n in counts]
    tables = render.build_layers(preds, H, W, mask_alpha=mask_alpha)
    normals = render.unit_normals(preds, tables).numpy()
    bits = R.pack_bits(np.concatenate([p.pred_masks.numpy() for p in preds]))
    return frames, preds, tables, normals, bits


def _gpu(frames, tables, normals, bits, pitch=None, col=0, out=None):
    from articulation3d_amd import render

    F, H, W, _ = frames.shape
    if out is None:
        out = torch.full((F, H, pitch or 2 * W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    dbits = torch.from_numpy(bits.view(np.int32)).cuda() if len(bits) else None
    render.launch(torch.from_numpy(frames).cuda(), tables, torch.from_numpy(np.asarray(normals, np.float32)), dbits, out, col=col)
    return out


def _ref(frames, tables, normals, bits, pitch=None, col=0, out=None):
    F, H, W, _ = frames.shape
    if out is None:
        out = np.full((F, H, pitch or 2 * W, 3), SENTINEL, np.uint8)
    return R.render_tables(frames, tables, normals, bits, out, col)


@pytest.mark.parametrize("H,W,counts", [(7, 37, (0, 1, 4)), (24, 40, (0, 1, 4)), (480, 640, (5,)), (1, 1, (1,)), (5, 3, (2, 0))])
@pytest.mark.parametrize("mask_alpha", [0.0, 0.5])
def test_kernel_equals_the_law(H, W, counts, mask_alpha):
    """7x37: the tail path, mask words straddling rows; 24x40 and 480x640: the dword path; frame ranges of 0, 1 and 4 instances."""
    frames, _preds, tables, normals, bits = _case(H, W, counts, seed=H * 1000 + W, mask_alpha=mask_alpha)
    assert (tables.layers["kind"] == 0).any() == (mask_alpha > 0)
    got = _gpu(frames, tables, normals, bits).cpu().numpy()
    want = _ref(frames, tables, normals, bits)
    assert np.array_equal(got, want), f"{(got != want).sum()} bytes differ"
    if H * W > 100:  # the case draws something
        assert len(np.unique(want[..., W:, :])) > 3 and (want[..., :W, :] != frames).any()


@pytest.mark.parametrize("H,W", [(7, 37), (24, 40)])
def test_alphas_0_128_256_and_a_widened_cull_box(H, W):
    """Every alpha of the blend on every kind of layer, and culling: cull boxes (the layers' and the pieces') widened to the whole image give the same bytes."""
    frames, _preds, tables, normals, bits = _case(H, W, (3, 4), seed=11)
    tables.layers["alpha"] = np.resize([0, 128, 256, 77], len(tables.layers))
    want = _ref(frames, tables, normals, bits)
    got = _gpu(frames, tables, normals, bits).cpu().numpy()
    assert np.array_equal(got, want)
    wide = tables.layers.copy()
    wide["x0"], wide["y0"], wide["x1"], wide["y1"] = 0, 0, W, H
    assert (wide != tables.layers).any()
    tables.layers = wide
    tables.pieces = tables.pieces.copy()
    tables.pieces["x0"], tables.pieces["y0"], tables.pieces["x1"], tables.pieces["y1"] = 0, 0, W, H
    assert np.array_equal(_gpu(frames, tables, normals, bits).cpu().numpy(), want)


@pytest.mark.parametrize("H,W", [(7, 37), (24, 40)])
def test_three_overlapping_masks_hold_the_sum_order_and_the_wrap(H, W):
    """Three masks over one region: the fp32 sum in ascending order (normals of very different magnitude, so another order rounds
    differently) and the stated wrap for v outside [0, 256)."""
    from articulation3d_amd import render

    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    masks = np.zeros((3, H, W), np.uint8)
    masks[0, 1:H - 1, 2:W - 3] = 1
    masks[1, 0:H - 2, 5:W - 1] = 1
    masks[2, 2:H, 0:W - 6] = 1
    assert (masks.sum(0) == 3).any()
    bits = R.pack_bits(masks)
    empty = render.LayerTables(H=H, W=W, layer_off=np.zeros(2, np.int32), layers=np.zeros(0, render.LAYER_DTYPE), pieces=np.zeros(0, render.PIECE_DTYPE),
                               inst_off=np.array([0, 3], np.int32), inst_row=np.array([2, 0, 1], np.int32), mask_keys=[])
    unit = np.array([[0.6, 0.64, 0.48], [0.8, 0.6, 0.0], [0.36, 0.48, 0.8]], np.float32)      # sums up to 1.76: wraps past 255
    neg = -unit                                                                               # negative v: int32 & 0xff
    # instance order 0.75, s, -0.75 with s just above 1/255: ascending, (0.75 + s) loses s's last bits and v falls below 128; an order
    # that cancels +-0.75 first keeps s and gives 128
    f32 = np.float32
    s_ = f32(0.00392158)
    uneven = np.array([[0.75, 0.1, 0.2], [s_, 0.1, 0.2], [-0.75, 0.1, 0.2]], np.float32)
    byte = lambda n: int((n + f32(1)) / f32(2) * f32(255)) & 255
    assert byte((f32(0.75) + s_) + f32(-0.75)) == 127 and byte((f32(0.75) + f32(-0.75)) + s_) == 128
    for normals in (unit, neg, uneven):
        want = _ref(frames, empty, normals, bits)
        v = R.normal_value(empty.inst_row, normals, bits, H, W)
        if normals is not uneven:
            assert ((v < 0) | (v >= 256)).any()
        got = _gpu(frames, empty, normals, bits).cpu().numpy()
        assert np.array_equal(got, want)
        assert np.array_equal(got[:, :, :W], frames)  # no layers: the seg panel is the frame


def test_two_calls_fill_disjoint_halves_and_leave_the_rest_alone():
    H, W = 7, 37
    frames, _p, t_a, n_a, bits_a = _case(H, W, (2, 0, 3), seed=21)
    _f, _p, t_b, n_b, bits_b = _case(H, W, (1, 4, 0), seed=22)
    pitch = 4 * W + 5
    out = torch.full((3, H, pitch, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    _gpu(frames, t_a, n_a, bits_a, out=out, col=1)
    first = out.cpu().numpy().copy()
    assert (first[:, :, :1] == SENTINEL).all() and (first[:, :, 1 + 2 * W:] == SENTINEL).all()
    _gpu(frames, t_b, n_b, bits_b, out=out, col=1 + 2 * W)
    want = np.full((3, H, pitch, 3), SENTINEL, np.uint8)
    _ref(frames, t_a, n_a, bits_a, out=want, col=1)
    _ref(frames, t_b, n_b, bits_b, out=want, col=1 + 2 * W)
    got = out.cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(got[:, :, 1:1 + 2 * W], first[:, :, 1:1 + 2 * W])
    assert (got[:, :, 1 + 4 * W:] == SENTINEL).all() and (got[:, :, 0] == SENTINEL).all()
    # the aligned form of the same placement (dword stores): pitch = 4W, col = 0 and 2W
    H, W = 24, 40
    frames, _p, t_a, n_a, bits_a = _case(H, W, (2, 3), seed=23)
    out = torch.full((2, H, 4 * W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    _gpu(frames, t_a, n_a, bits_a, out=out, col=2 * W)
    got = out.cpu().numpy()
    assert (got[:, :, :2 * W] == SENTINEL).all() and np.array_equal(got[:, :, 2 * W:], _ref(frames, t_a, n_a, bits_a))


def test_inconsistent_arguments_are_refused_before_any_launch():
    """A3D_ERR_ARG (-1), and the output keeps its sentinel.  Every pointer is a real allocation large enough for the widest reading
    of the arguments, so a call that was wrongly accepted would still stay inside it."""
    from articulation3d_amd import _lib

    lib = _lib.lib()
    F, H, W = 2, 4, 8
    big = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")
    frames, out = big(F * H * W * 3 * 4, torch.uint8), torch.full((F * H * 8 * W * 3,), SENTINEL, dtype=torch.uint8, device="cuda")
    off, tab, f32, bits = big(16, torch.int32), big(4096, torch.uint8), big(64, torch.float32), big(64, torch.int32)

    def desc(**kw):
        d = _lib.RenderDesc()
        d.frames, d.out, d.layer_off, d.inst_off = frames.data_ptr(), out.data_ptr(), off.data_ptr(), off.data_ptr()
        d.layers, d.pieces, d.inst_row, d.normals, d.bits = tab.data_ptr(), tab.data_ptr(), off.data_ptr(), f32.data_ptr(), bits.data_ptr()
        d.F, d.H, d.W, d.pitch, d.col = F, H, W, 2 * W, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    stream = torch.cuda.current_stream().cuda_stream
    bad = [dict(col=1), dict(pitch=2 * W - 1), dict(col=-1), dict(F=-1), dict(H=0), dict(W=0), dict(frames=None), dict(out=None),
           dict(layer_off=None), dict(inst_off=None), dict(n_layers=1, layers=None), dict(n_pieces=1, pieces=None),
           dict(n_inst=1, inst_row=None), dict(n_inst=1, normals=None), dict(n_masks=1, bits=None), dict(n_layers=-1), dict(n_masks=-2)]
    for kw in bad:
        assert lib.a3d_render_panels(ctypes.byref(desc(**kw)), stream) == -1, kw
    assert lib.a3d_render_panels(None, stream) == -1
    assert lib.a3d_render_panels(ctypes.byref(desc(F=0, frames=None, out=None, layer_off=None, inst_off=None)), stream) == 0  # nothing to do
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert lib.a3d_render_panels(ctypes.byref(desc()), stream) == 0  # the consistent call: no layers, no instances
    torch.cuda.synchronize()
    got = out.cpu().numpy()[:F * H * 2 * W * 3].reshape(F, H, 2 * W, 3)
    assert (got[:, :, :W] == 0).all() and (got[:, :, W:] == 127).all() and bool((out[F * H * 2 * W * 3:] == SENTINEL).all())


def test_render_panels_on_instances_equals_build_layers_and_the_law():
    from articulation3d_amd import render
    from articulation3d_amd.utils.opt_utils import _MaskBank

    H, W = 24, 40
    frames, preds, _t, _n, bits = _case(H, W, (0, 1, 4), seed=31)
    preds[2].scores = np.array([0.9, 0.5, 0.8, 0.71], np.float32)  # one instance below the threshold: no layers, still in the normal panel
    dframes = torch.from_numpy(frames).cuda()
    for mask_alpha in (0.0, 0.5):
        tables = render.build_layers(preds, H, W, mask_alpha=mask_alpha)
        want = _ref(frames, tables, render.unit_normals(preds, tables).numpy(), bits)
        got = render.render_panels(dframes, preds, mask_alpha=mask_alpha)
        assert got.shape == (3, H, 2 * W, 3) and np.array_equal(got.cpu().numpy(), want)
        # a bank that holds the clip's masks in another row order gives the same bytes
        bank = _MaskBank(preds, "cuda")
        assert np.array_equal(render.render_panels(dframes, preds, mask_alpha=mask_alpha, bank=bank).cpu().numpy(), want)
    with pytest.raises(KeyError):
        render.render_panels(dframes, preds, bank=_MaskBank(preds, "cuda", wanted={(2, 0)}))


def test_render_clip_in_chunks_equals_the_one_shot_result():
    """5 frames, chunks of 2: three chunks through the two device staging buffers (the third reuses the first)."""
    from articulation3d_amd import render

    H, W = 24, 40
    frames, raw, _t, _n, _b = _case(H, W, (2, 0, 3, 1, 4), seed=41)
    rng = np.random.default_rng(42)
    opt = [R.make_instances(rng, H, W, n) for n in (1, 2, 0, 3, 2)]
    dframes = torch.from_numpy(frames).cuda()
    whole = torch.empty((5, H, 4 * W, 3), dtype=torch.uint8, device="cuda")
    render.render_panels(dframes, opt, out=whole, col=0)
    render.render_panels(dframes, raw, out=whole, col=2 * W)
    whole = whole.cpu().numpy()
    chunks = [c.copy() for c in render.render_clip(dframes, raw, opt, chunk=2)]
    assert [len(c) for c in chunks] == [2, 2, 1] and np.array_equal(np.concatenate(chunks), whole)
    assert np.array_equal(np.concatenate([c.copy() for c in render.render_clip(dframes, raw, opt, chunk=8)]), whole)
    t_opt, t_raw = render.build_layers(opt, H, W), render.build_layers(raw, H, W)
    want = np.zeros_like(whole)
    _ref(frames, t_opt, render.unit_normals(opt, t_opt).numpy(), R.pack_bits(np.concatenate([p.pred_masks.numpy() for p in opt])), out=want, col=0)
    _ref(frames, t_raw, render.unit_normals(raw, t_raw).numpy(), R.pack_bits(np.concatenate([p.pred_masks.numpy() for p in raw])), out=want, col=2 * W)
    assert np.array_equal(whole, want)


def test_render_clip_chunk_stays_valid_across_the_next_request():
    """The documented lifetime: a yielded array (no copy taken) still holds its chunk after the NEXT chunk has been requested and every
    copy that request started has landed -- the host side is a ring of three buffers, the copy of chunk k+2 must not land in chunk k."""
    from articulation3d_amd import render

    H, W = 24, 40
    frames, raw, _t, _n, _b = _case(H, W, (2, 0, 3, 1, 4, 2, 1), seed=51)
    rng = np.random.default_rng(52)
    opt = [R.make_instances(rng, H, W, n) for n in (1, 2, 0, 3, 2, 0, 4)]
    dframes = torch.from_numpy(frames).cuda()
    whole = torch.empty((7, H, 4 * W, 3), dtype=torch.uint8, device="cuda")
    render.render_panels(dframes, opt, out=whole, col=0)
    render.render_panels(dframes, raw, out=whole, col=2 * W)
    whole = whole.cpu().numpy()
    assert len({whole[k].tobytes() for k in range(7)}) == 7  # every row differs: a chunk in the wrong buffer shows
    for chunk in (1, 2):
        held, at, seen = None, 0, 0
        for cur in render.render_clip(dframes, raw, opt, chunk=chunk):
            torch.cuda.synchronize()  # whatever asking for `cur` put in flight is now in host memory
            if held is not None:
                assert np.array_equal(held, whole[at - len(held):at]), f"chunk ending at frame {at} was overwritten by the next request"
            assert np.array_equal(cur, whole[at:at + len(cur)])
            held, at, seen = cur, at + len(cur), seen + 1
        assert at == 7 and seen == -(-7 // chunk) and np.array_equal(held, whole[7 - len(held):])


def _instances_from_json(frame, hw=(480, 640)):
    from articulation3d_amd.structures import Boxes, Instances
    from articulation3d_amd.utils import rle

    rows = frame["instances"]
    inst = Instances(hw)
    inst.pred_boxes = Boxes(torch.tensor([r["bbox"] for r in rows], dtype=torch.float32).reshape(-1, 4))
    inst.scores = np.array([r["score"] for r in rows], np.float64)
    inst.pred_classes = np.array([r["category_id"] for r in rows], np.int64)
    inst.pred_planes = torch.tensor([r["pred_plane"] for r in rows], dtype=torch.float32).reshape(-1, 3)
    inst.pred_rot_axis = torch.tensor([r["pred_rot_axis"] for r in rows], dtype=torch.float32).reshape(-1, 3)
    inst.pred_tran_axis = torch.tensor([r["pred_tran_axis"] for r in rows], dtype=torch.float32).reshape(-1, 2)
    masks = [rle.decode(r["segmentation"]) for r in rows]
    inst.pred_masks = torch.from_numpy(np.stack(masks).astype(np.float32)) if masks else torch.zeros((0,) + hw)
    return inst


def test_inference_script_writes_the_four_panel_rows(tmp_path):
    """tools/inference.py --vis npy on a 3-frame synthetic clip (the flags of test_inference_script_on_synthetic_clip): vis.npy is
    [3,480,2560,3]; its opt half equals the law on the written predictions.json and the resized frames.  Three frames are too few for
    a track, so the optimiser only re-weights scores (x 0.6): the raw half shows the same geometry with every detection drawn."""
    from articulation3d_amd import ops, render
    from articulation3d_amd.utils.synthetic import synthetic_frames

    out = tmp_path / "out"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "tools/inference.py", "--config", "configs/planercnn_inference.yaml", "--input", "synthetic:3", "--output", str(out),
                        "--random-init", "--calibrate-bn", "--conf-threshold", "0.3", "--batch", "2", "--vis", "npy",
                        "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.3"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    vis = np.load(out / "vis.npy")
    assert vis.shape == (3, 480, 2560, 3) and vis.dtype == np.uint8
    written = json.load(open(out / "predictions.json"))
    tracks = json.load(open(out / "tracks.json"))
    assert tracks == {"rot": [], "trans": []} and sum(len(p["instances"]) for p in written) > 0
    preds = [_instances_from_json(p) for p in written]
    src = torch.from_numpy(np.ascontiguousarray(synthetic_frames(3)[..., ::-1])).cuda()
    _x4, u8 = ops.preprocess_resize_u8(src, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), want_u8=True)
    frames = u8.cpu().numpy()
    bits = R.pack_bits(np.concatenate([p.pred_masks.numpy() for p in preds]))
    want = np.zeros_like(vis)
    for col, thr in ((0, 0.3), (1280, -1.0)):
        tables = render.build_layers(preds, 480, 640, conf_threshold=thr)
        _ref(frames, tables, render.unit_normals(preds, tables).numpy(), bits, out=want, col=col)
    assert np.array_equal(vis[:, :, :1280], want[:, :, :1280])
    assert np.array_equal(vis[:, :, 1280:], want[:, :, 1280:])
    assert (vis[:, :, :640] != frames).any()  # something was drawn
