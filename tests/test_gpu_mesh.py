"""GPU suite: a3d_mesh_build (csrc/mesh.hip) against tests/mesh_ref.py, the law in numpy -- counts, verts, uvs and faces byte for
byte -- then the model assembly of articulation3d_amd/mesh.py over it and one run of tools/inference.py --save-obj."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_ref as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = lambda H, W: dict(focal=M.FOCAL, cx=W / 2, cy=H / 2)


def _gpu(mask, A, *, stride=1, invert=False, flip_yz=False, tail_ones=False):
    from articulation3d_amd import opt_ops

    H, W = mask.shape
    normal, offset, pivot, xf = M.plane_and_poses(A, H, W)
    row = torch.from_numpy(M.pack_bits(mask, tail_ones=tail_ones)).cuda()
    got = opt_ops.build_mesh(row, H, W, normal.tolist(), float(offset), pivot.tolist(), torch.from_numpy(xf).cuda(), stride=stride, invert=invert,
                             flip_yz=flip_yz, **CAM(H, W))
    return tuple(t.cpu().numpy() for t in got)


def _ref(mask, A, fast=True, **kw):
    H, W = mask.shape
    normal, offset, pivot, xf = M.plane_and_poses(A, H, W)
    return (M.build_mesh_fast if fast else M.build_mesh_loop)(mask, normal, offset, pivot, xf, **kw)


def _assert_same(got, want, what):
    for name, g, w in zip(("verts", "uvs", "faces"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {name}: {g.dtype}{g.shape} != {w.dtype}{w.shape}"
        assert g.tobytes() == w.tobytes(), f"{what} {name}: {(g != w).sum()} of {g.size} elements differ"


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (5, 7), (33, 65), (24, 40)])
@pytest.mark.parametrize("name", sorted(M.MASKS))
def test_kernel_equals_the_law(H, W, name):
    """5x7: two words, tail bits, rows straddling words; 33x65: several words per row, stride 3 divides neither side; 24x40: whole
    words.  Strides 1 / 2 / 3, both inversions, 1 and 5 poses about a non-trivial pivot, flip_yz."""
    mask = M.MASKS[name](H, W)
    for stride, invert, A, flip in ((1, False, 5, False), (1, True, 1, True), (2, False, 1, False), (2, True, 5, True), (3, False, 5, True), (3, True, 1, False)):
        kw = dict(stride=stride, invert=invert, flip_yz=flip)
        _assert_same(_gpu(mask, A, **kw), _ref(mask, A, fast=H * W > 100, **kw), f"{name} {H}x{W} {kw}")


@pytest.mark.parametrize("stride,invert", [(1, False), (2, True)])
def test_kernel_equals_the_law_at_480x640(stride, invert):
    """More than one block of the count kernel (9 600 words at stride 1), block offsets and ranks that cross blocks."""
    mask = M.mask_blobs(480, 640, 5) & M.mask_random(480, 640, 6) | M.mask_blobs(480, 640, 7, n=1)
    got, want = _gpu(mask, 5, stride=stride, invert=invert), _ref(mask, 5, stride=stride, invert=invert)
    assert len(want[1]) > 10000 and len(want[2]) > 10000
    _assert_same(got, want, f"480x640 stride {stride}")


@pytest.mark.parametrize("H,W", [(5, 7), (33, 65)])
@pytest.mark.parametrize("invert", [False, True])
def test_tail_bits_past_the_mask_stay_dead(H, W, invert):
    mask = M.mask_random(H, W, 11)
    assert (H * W) % 32 != 0
    for stride in (1, 2):
        _assert_same(_gpu(mask, 1, stride=stride, invert=invert, tail_ones=True), _ref(mask, 1, fast=False, stride=stride, invert=invert), f"tail {H}x{W}")


def test_full_mask_counts():
    for stride in (1, 2, 3):
        Lh, Lw = -(-33 // stride), -(-65 // stride)
        verts, uvs, faces = _gpu(M.mask_full(33, 65), 1, stride=stride)
        assert len(uvs) == Lh * Lw and len(faces) == 2 * (Lh - 1) * (Lw - 1)  # the worst case exactly fills the capacities


def test_capacity_cut_short_keeps_true_counts_and_sentinels():
    from articulation3d_amd import opt_ops

    H, W, A = 33, 65, 5
    mask = M.mask_blobs(H, W, 2)
    want = _ref(mask, A)
    n, m = len(want[1]), len(want[2])
    assert n > 2 and m > 2
    normal, offset, pivot, xf = M.plane_and_poses(A, H, W)
    row = torch.from_numpy(M.pack_bits(mask)).cuda()
    S = -7.0
    # allocations one row longer than the capacities n-1 / m-1 handed to the kernel
    vbuf = torch.full((A * (n - 1) + 1, 3), S, device="cuda")
    cut_v = vbuf[:A * (n - 1)].view(A, n - 1, 3)
    uvs = torch.full((n, 2), S, device="cuda")
    faces = torch.full((m, 3), -7, dtype=torch.int32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    opt_ops.mesh_build_into(row, H, W, normal.tolist(), float(offset), pivot.tolist(), torch.from_numpy(xf).cuda(), cut_v, uvs[:n - 1], faces[:m - 1], counts,
                            **CAM(H, W))
    assert counts.tolist() == [n, m]
    assert uvs[n - 1].tolist() == [S, S] and faces[m - 1].tolist() == [-7, -7, -7] and vbuf[-1].tolist() == [S, S, S]
    assert cut_v.cpu().numpy().tobytes() == want[0][:, :n - 1].tobytes()
    assert uvs[:n - 1].cpu().numpy().tobytes() == want[1][:n - 1].tobytes() and faces[:m - 1].cpu().numpy().tobytes() == want[2][:m - 1].tobytes()
    # capacities LARGER than the counts: rows past the counts are left untouched
    big_u = torch.full((n + 3, 2), S, device="cuda")
    big_v = torch.full((A, n + 3, 3), S, device="cuda")
    big_f = torch.full((m + 3, 3), -7, dtype=torch.int32, device="cuda")
    opt_ops.mesh_build_into(row, H, W, normal.tolist(), float(offset), pivot.tolist(), torch.from_numpy(xf).cuda(), big_v, big_u, big_f, counts, **CAM(H, W))
    assert (big_u[n:] == S).all() and (big_v[:, n:] == S).all() and (big_f[m:] == -7).all()
    assert big_v[:, :n].cpu().numpy().tobytes() == want[0].tobytes()


def test_bad_arguments_return_err_arg_without_a_launch():
    from articulation3d_amd import _lib

    lib = _lib.lib()
    H, W = 5, 7
    keep = [torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros((1, 12), device="cuda"), torch.full((1, 35, 3), 3.0, device="cuda"),
            torch.full((35, 2), 3.0, device="cuda"), torch.full((48, 3), 3, dtype=torch.int32, device="cuda"), torch.full((2,), 9, dtype=torch.int32, device="cuda"),
            torch.zeros(max(lib.a3d_mesh_workspace_bytes(H, W, 1), 4) // 4 + 1, dtype=torch.int32, device="cuda")]

    def desc(**over):
        d = _lib.MeshDesc()
        d.bits, d.xforms, d.verts, d.uvs, d.faces, d.counts, d.workspace = (t.data_ptr() for t in keep)
        d.H, d.W, d.stride, d.invert, d.A, d.cap_v, d.cap_f = H, W, 1, 0, 1, 35, 48
        d.normal[2], d.offset, d.focal, d.cx, d.cy = 1.0, 1.0, M.FOCAL, W / 2, H / 2
        for k, v in over.items():
            setattr(d, k, v)
        return d

    stream = torch.cuda.current_stream().cuda_stream
    assert lib.a3d_mesh_build(ctypes.byref(desc()), stream) == 0
    torch.cuda.synchronize()
    assert keep[5].tolist() == [0, 0]
    keep[5].fill_(9)
    bad = [dict(bits=None), dict(xforms=None), dict(counts=None), dict(workspace=None), dict(verts=None), dict(uvs=None), dict(faces=None),
           dict(H=0), dict(W=0), dict(H=-3), dict(stride=0), dict(stride=-1), dict(A=0), dict(A=17), dict(cap_v=-1), dict(cap_f=-1)]
    for over in bad:
        assert lib.a3d_mesh_build(ctypes.byref(desc(**over)), stream) == -1, over
    assert lib.a3d_mesh_build(None, stream) == -1
    torch.cuda.synchronize()
    assert keep[5].tolist() == [9, 9]  # nothing ran
    assert lib.a3d_mesh_build(ctypes.byref(desc(verts=None, uvs=None, cap_v=0, faces=None, cap_f=0)), stream) == 0  # null with zero extent is fine
    torch.cuda.synchronize()
    assert keep[5].tolist() == [0, 0] and (keep[2] == 3.0).all() and (keep[4] == 3).all()
    assert lib.a3d_mesh_workspace_bytes(0, 7, 1) == 0 and lib.a3d_mesh_workspace_bytes(5, 7, 0) == 0 and lib.a3d_mesh_workspace_bytes(480, 640, 1) > 0
    with pytest.raises(ValueError):
        _gpu(M.mask_full(5, 7), 17)


def test_articulated_model_equals_the_host_assembly():
    """mesh.articulated_model on the device == the same call with its two device steps replaced by the numpy law."""
    from articulation3d_amd import mesh

    for scores, webvis in (((0.4, 0.9, 0.7), False), ((0.95, 0.9, 0.7), True)):
        inst, frame = M.handmade_instances(scores=scores)
        got = mesh.articulated_model(inst, frame, stride=2, bkgd_stride=3, webvis=webvis, device="cuda")
        with pytest.MonkeyPatch.context() as mp:
            M.patch_mesh_to_reference(mp)
            want = mesh.articulated_model(inst, frame, stride=2, bkgd_stride=3, webvis=webvis, device="cpu")
        assert got.kind == want.kind and got.box_id == want.box_id and len(got.meshes) == len(want.meshes) == 8
        for g, w in zip(got.meshes, want.meshes):
            assert g.material == w.material
            _assert_same((g.verts, g.uvs, g.faces), (w.verts, w.uvs, w.faces), g.material)
        assert list(got.textures) == list(want.textures) and all(np.array_equal(got.textures[k], want.textures[k]) for k in got.textures)


def test_articulated_model_reads_a_mask_bank():
    from articulation3d_amd import mesh
    from articulation3d_amd.utils.opt_utils import _MaskBank

    inst, frame = M.handmade_instances()
    bank = _MaskBank([inst], "cuda")
    a = mesh.articulated_model(inst, frame, bank=bank, frame_idx=0, device="cuda")
    b = mesh.articulated_model(inst, frame, device="cuda")
    for g, w in zip(a.meshes, b.meshes):
        _assert_same((g.verts, g.uvs, g.faces), (w.verts, w.uvs, w.faces), g.material)


def test_inference_script_saves_obj_models(tmp_path):
    """tools/inference.py --save-obj on a 3-frame synthetic clip (the flags of test_gpu_render's script test).  A frame with a detection
    gets a parseable arti_pred.obj whose face indices are in range, plus its textures; a frame without one gets a line on stdout; frame
    index 7 is past the clip and dropped; the run exits 0 either way."""
    import json

    from PIL import Image

    out = tmp_path / "out"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "tools/inference.py", "--config", "configs/planercnn_inference.yaml", "--input", "synthetic:3", "--output", str(out),
                        "--random-init", "--calibrate-bn", "--conf-threshold", "0.3", "--batch", "2", "--save-obj", "--obj-frames", "0,2,7",
                        "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.3"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    written = json.load(open(out / "predictions.json"))
    assert "save-obj:" in r.stdout and not (out / "frame_0007").exists() and not (out / "frame_0001").exists()
    exported = 0
    for i in (0, 2):
        folder = out / ("frame_%04d" % i)
        if not folder.exists():
            assert f"save-obj: frame {i} has no articulated plane to export" in r.stdout
            continue
        assert len(written[i]["instances"]) > 0
        exported += 1
        nv, nf = M.parse_obj(folder / "arti_pred.obj")
        assert nv >= 24 and nf >= 80  # the two markers at least
        mtl = open(folder / "arti_pred.mtl").read()
        maps = [line.split()[1] for line in mtl.splitlines() if line.startswith("map_Kd ")]
        assert len(maps) >= 6 and len(maps) == mtl.count("newmtl ")
        for rel in maps:
            img = Image.open(folder / rel)
            assert img.size == ((4, 4) if rel.endswith("axis.png") else (640, 480))
    if exported == 0:
        assert "save-obj: no model exported" in r.stdout
    else:
        assert f"save-obj: {exported} of 2 requested frames exported" in r.stdout
