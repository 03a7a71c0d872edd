"""Host suite of the 3-D model export: tests/mesh_ref.py's two statements of a3d_mesh_build's law against each other, the model
assembly of articulation3d_amd/mesh.py over that law (no device), save_obj's file layout, and the CLI flags."""
import importlib.util
import os

import numpy as np
import pytest

import mesh_ref as M
from articulation3d_amd import mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (2, 2), (5, 7), (33, 65), (24, 40)]


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("name", sorted(M.MASKS))
def test_loop_and_fast_agree_byte_for_byte(H, W, name):
    mask = M.MASKS[name](H, W)
    for stride, invert, A, flip in ((1, False, 5, False), (2, True, 1, True), (3, False, 5, True), (3, True, 1, False)):
        normal, offset, pivot, xf = M.plane_and_poses(A, H, W)
        kw = dict(stride=stride, invert=invert, flip_yz=flip)
        loop, fast = M.build_mesh_loop(mask, normal, offset, pivot, xf, **kw), M.build_mesh_fast(mask, normal, offset, pivot, xf, **kw)
        assert _same(loop, fast), (name, stride, invert)
        verts, uvs, faces = fast
        assert verts.shape == (A, len(uvs), 3) and np.isfinite(verts).all()
        assert faces.size == 0 or (faces.min() >= 0 and faces.max() < len(uvs))
        live = ((mask != 0) != invert)[::stride, ::stride]
        assert len(uvs) == live.sum()
        if name == "checkerboard" and not invert:
            assert len(faces) == 0 or stride == 2  # stride 2 samples one colour of the board: a full lattice
        if name == "last_row_col" and stride == 1 and not invert:
            assert len(faces) == 0 and len(uvs) == H + W - 1


def test_two_by_two_full_mask_by_hand():
    normal, offset, pivot, xf = [0.0, 0.0, 1.0], 2.0, [0.0, 0.0, 0.0], np.concatenate([np.eye(3).ravel(), np.zeros(3)])[None].astype(np.float32)
    verts, uvs, faces = M.build_mesh_loop(M.mask_full(2, 2), normal, offset, pivot, xf, focal=2.0, cx=1.0, cy=1.0)
    assert faces.tolist() == [[0, 3, 1], [0, 2, 3]]
    # depth 2 everywhere; rays ((x-1)/2, (y-1)/2): row-major (0,0) (0,1) (1,0) (1,1)
    assert verts[0].tolist() == [[-1.0, -1.0, 2.0], [0.0, -1.0, 2.0], [-1.0, 0.0, 2.0], [0.0, 0.0, 2.0]]
    assert uvs.tolist() == [[0.0, 1.0], [0.5, 1.0], [0.0, 0.5], [0.5, 0.5]]
    flipped = M.build_mesh_fast(M.mask_full(2, 2), normal, offset, pivot, xf, focal=2.0, cx=1.0, cy=1.0, flip_yz=True)[0]
    assert np.array_equal(flipped[0], verts[0] * np.float32([1, -1, -1]))


def test_pack_bits_round_trip_and_tail():
    m = M.mask_random(5, 7, 1)
    assert np.array_equal(M.unpack_bits(M.pack_bits(m), 5, 7), m)
    tail = M.pack_bits(m, tail_ones=True).view(np.uint32)
    assert tail[1] >> 3 == (1 << 29) - 1 and np.array_equal(M.unpack_bits(tail, 5, 7), m)


def test_pose_angles():
    assert mesh.POSE_ANGLES.dtype == np.float32 and mesh.POSE_ANGLES.tolist() == np.float32([-1.8, -1.35, -0.9, -0.45]).tolist()
    assert mesh.POSE_ANGLES_R.tolist() == np.float32([0.45, 0.9, 1.35]).tolist()
    d = np.array([0.0, 1.0, 0.0])
    xf, pivot = mesh.pose_table("rot", d, np.array([1.0, 2.0, 3.0]), "l")
    assert xf.shape == (5, 12) and xf.dtype == np.float32 and pivot.tolist() == [1.0, 2.0, 3.0]
    assert xf[0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    # column-vector rotation about +y by angle a is [[c,0,s],[0,1,0],[-s,0,c]]; the table holds its TRANSPOSE (row-vector convention)
    a = float(mesh.POSE_ANGLES[0])
    np.testing.assert_allclose(xf[1, :9].reshape(3, 3), np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]]), atol=1e-6)
    assert mesh.pose_table("rot", d, np.zeros(3), "r")[0].shape == (4, 12)
    xt, pt = mesh.pose_table("tran", d, np.array([1.0, 2.0, 3.0]))
    assert pt.tolist() == [0, 0, 0] and np.array_equal(xt[:, :9], np.tile(np.eye(3, dtype=np.float32).ravel(), (5, 1)))
    assert xt[:, 10].tolist() == np.float32([0.0, 0.1, 0.2, 0.3, 0.4]).tolist() and not xt[:, [9, 11]].any()
    with pytest.raises(ValueError):
        mesh.pose_table("rot", d, np.zeros(3), "x")


def test_model_assembly_over_the_reference(monkeypatch):
    M.patch_mesh_to_reference(monkeypatch)
    inst, frame = M.handmade_instances()
    H, W = frame.shape[:2]
    model = mesh.articulated_model(inst, frame, stride=1, bkgd_stride=2, device="cpu")
    assert model is not None and model.box_id == 1 and model.kind == "tran"  # the top score is the class-1 detection
    assert [m.material for m in model.meshes] == ["obj_pose0", "obj_pose1", "obj_pose2", "obj_pose3", "obj_pose4", "axis", "axis", "bkgd"]
    assert list(model.textures) == ["obj_pose0", "obj_pose1", "obj_pose2", "obj_pose3", "obj_pose4", "axis", "bkgd"]
    obj = model.meshes[:5]
    mask = (inst.pred_masks[1].numpy() > 0.5)
    assert len(obj[0].verts) == mask.sum() and all(m.faces is obj[0].faces or np.array_equal(m.faces, obj[0].faces) for m in obj)
    # class 1: every pose is the detected one moved along ONE direction, by 0.1 .. 0.4
    for i in range(1, 5):
        step = obj[i].verts.astype(np.float64) - obj[0].verts
        np.testing.assert_allclose(np.linalg.norm(step, axis=1), 0.1 * i, atol=1e-5)
        assert np.abs(step - step[0]).max() < 1e-5
    bk = model.meshes[-1]
    assert len(bk.verts) == (~mask)[::2, ::2].sum() and np.array_equal(model.textures["bkgd"], frame)
    for marker in model.meshes[5:7]:
        assert marker.verts.shape == (12, 3) and marker.faces.shape == (20, 3) and (marker.uvs == 0.5).all()
        np.testing.assert_allclose(np.linalg.norm(marker.verts - marker.verts.mean(0), axis=1), 0.1, atol=1e-6)
    assert model.textures["axis"].reshape(-1, 3).tolist() == [[56, 207, 252]] * 16
    # the markers sit on the plane the object lies on: the first one is the (zero) pivot's axis point, inside the object's depth range
    z = obj[0].verts[:, 2]
    assert z.min() - 1 < model.meshes[5].verts[:, 2].mean() < z.max() + 1

    # class 0 on top: rotations about the axis -- the pivot-to-vertex distance is kept, the axis points stay put
    inst0, _ = M.handmade_instances(scores=(0.95, 0.9, 0.7))
    rot = mesh.articulated_model(inst0, frame, stride=1, bkgd_stride=2, device="cpu")
    assert rot.box_id == 0 and rot.kind == "rot" and len(rot.meshes) == 8
    p0 = rot.meshes[5].verts.mean(0).astype(np.float64)
    r0 = np.linalg.norm(rot.meshes[0].verts - p0, axis=1)
    for i in range(1, 5):
        np.testing.assert_allclose(np.linalg.norm(rot.meshes[i].verts - p0, axis=1), r0, atol=1e-4)
        assert np.abs(rot.meshes[i].verts - rot.meshes[0].verts).max() > 1e-2
    right = mesh.articulated_model(inst0, frame, stride=1, bkgd_stride=2, axis_dir="r", device="cpu")
    assert len(right.meshes) == 4 + 2 + 1
    assert np.abs(right.meshes[1].verts - rot.meshes[4].verts).max() > 1e-2  # the other side

    web = mesh.articulated_model(inst0, frame, stride=1, bkgd_stride=2, webvis=True, device="cpu")
    for a, b in zip(web.meshes, rot.meshes):
        if a.material == "axis":  # the marker's CENTRE is flipped; the icosahedron about it is the same table
            np.testing.assert_allclose(a.verts.mean(0), b.verts.mean(0) * np.float32([1, -1, -1]), atol=1e-6)
            np.testing.assert_allclose(a.verts - a.verts.mean(0), b.verts - b.verts.mean(0), atol=1e-6)
        else:
            assert np.array_equal(a.verts, b.verts * np.float32([1, -1, -1]))


def test_model_none_cases(monkeypatch):
    import torch

    from articulation3d_amd.structures import Boxes, Instances

    M.patch_mesh_to_reference(monkeypatch)
    inst, frame = M.handmade_instances()
    empty = Instances(frame.shape[:2])
    empty.scores = np.zeros(0, np.float32)
    empty.pred_boxes = Boxes(torch.zeros((0, 4)))
    assert mesh.articulated_model(empty, frame, device="cpu") is None
    inst.pred_planes[1] = 0.0  # the top detection's plane has zero length
    assert mesh.articulated_model(inst, frame, device="cpu") is None
    inst2, _ = M.handmade_instances()
    monkeypatch.setattr(mesh, "angle_offset_to_axis", lambda ao, c, H, W: torch.tensor([[3, 4, 3, 4]] * len(ao)))
    assert mesh.articulated_model(inst2, frame, device="cpu") is None  # coinciding axis end points


def test_object_texture_formula():
    frame = np.full((3, 4, 3), 100, np.uint8)
    want = [int((100 / 255 + c / 255 * (2 / 10 + 1 / 2)) / 2 * 255) for c in (252, 116, 81)]
    got = mesh.object_texture(frame, 2)
    assert got.dtype == np.uint8 and got.shape == frame.shape and got[1, 2].tolist() == want == [138, 90, 78]


EXPECTED_OBJ = """mtllib arti_pred.mtl

# mesh 0
v 0.0000000000 0.0000000000 1.0000000000
v 1.0000000000 0.0000000000 1.5000000000
v 0.0000000000 -2.2500000000 0.3333333433
vt 0.0000000000 1.0000000000
vt 0.5000000000 1.0000000000
vt 0.0000000000 0.2500000000
usemtl first
f 1/1 2/2 3/3
f 3/3 2/2 1/1
# mesh 1
v 5.0000000000 5.0000000000 5.0000000000
v 6.0000000000 5.0000000000 5.0000000000
v 5.0000000000 6.0000000000 5.0000000000
v 6.0000000000 6.0000000000 5.0000000000
vt 0.5000000000 0.5000000000
vt 0.5000000000 0.5000000000
vt 0.5000000000 0.5000000000
vt 0.5000000000 0.5000000000
usemtl second
f 4/4 7/7 5/5
f 5/5 7/7 4/4
f 4/4 6/6 7/7
f 7/7 6/6 4/4
"""
EXPECTED_MTL = """newmtl first
map_Kd uv_maps/first.png
# Test colors
Ka 1.000 1.000 1.000  # white
Kd 1.000 1.000 1.000  # white
Ks 0.000 0.000 0.000  # black
Ns 10.0
newmtl second
map_Kd uv_maps/second.png
# Test colors
Ka 1.000 1.000 1.000  # white
Kd 1.000 1.000 1.000  # white
Ks 0.000 0.000 0.000  # black
Ns 10.0
"""


def _two_mesh_model():
    tri = mesh.Mesh(np.float32([[0, 0, 1], [1, 0, 1.5], [0, -2.25, 1 / 3]]), np.float32([[0, 1], [0.5, 1], [0, 0.25]]), np.int32([[0, 1, 2]]), "first")
    quad = mesh.Mesh(np.float32([[5, 5, 5], [6, 5, 5], [5, 6, 5], [6, 6, 5]]), np.full((4, 2), 0.5, np.float32), np.int32([[0, 3, 1], [0, 2, 3]]), "second")
    return mesh.ArticulatedModel([tri, quad], {"first": np.full((6, 8, 3), 7, np.uint8), "second": np.full((2, 3, 3), 200, np.uint8)})


def test_save_obj_matches_the_literal_files(tmp_path):
    from PIL import Image

    path = mesh.save_obj(str(tmp_path / "frame_0000"), "arti_pred", _two_mesh_model())
    assert open(path).read() == EXPECTED_OBJ
    assert open(tmp_path / "frame_0000" / "arti_pred.mtl").read() == EXPECTED_MTL
    for line in EXPECTED_MTL.splitlines():
        if line.startswith("map_Kd "):
            img = Image.open(tmp_path / "frame_0000" / line.split()[1])
            assert img.size == ((8, 6) if "first" in line else (3, 2)) and img.mode == "RGB"
    one_sided = open(mesh.save_obj(str(tmp_path / "one"), "m", _two_mesh_model(), decimal_places=2, double_sided=False)).read()
    assert one_sided.startswith("mtllib m.mtl\n\n# mesh 0\nv 0.00 0.00 1.00\n") and one_sided.endswith("f 4/4 7/7 5/5\nf 4/4 6/6 7/7\n")
    bad = _two_mesh_model()
    bad.meshes[1].material = "missing"
    with pytest.raises(ValueError):
        mesh.save_obj(str(tmp_path / "bad"), "m", bad)


def test_save_obj_of_an_assembled_model(tmp_path, monkeypatch):
    from PIL import Image

    M.patch_mesh_to_reference(monkeypatch)
    inst, frame = M.handmade_instances()
    model = mesh.articulated_model(inst, frame, stride=1, bkgd_stride=2, device="cpu")
    path = mesh.save_obj(str(tmp_path), "arti_pred", model)
    nv, nf = M.parse_obj(path)
    assert nv == sum(len(m.verts) for m in model.meshes) and nf == 2 * sum(len(m.faces) for m in model.meshes)
    for name in model.textures:
        img = Image.open(tmp_path / "uv_maps" / (name + ".png"))
        assert img.size == ((4, 4) if name == "axis" else (frame.shape[1], frame.shape[0]))
    assert np.array_equal(np.asarray(Image.open(tmp_path / "uv_maps" / "obj_pose2.png")), mesh.object_texture(frame, 2))


def _cli():
    spec = importlib.util.spec_from_file_location("a3d_tools_inference", os.path.join(ROOT, "tools", "inference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags():
    ap = _cli().build_parser()
    base = ["--config", "c.yaml", "--input", "synthetic:3", "--output", "o"]
    off = ap.parse_args(base)
    assert off.save_obj is False and off.obj_frames == [0, 30, 60, 89] and off.axis_dir == "l" and not off.webvis
    assert off.obj_stride == 2 and off.obj_bkgd_stride == 8 and off.opts == []
    on = ap.parse_args(base + ["--save-obj", "MODEL.DEVICE", "cuda:0"])
    assert on.save_obj is True and on.opts == ["MODEL.DEVICE", "cuda:0"]
    full = ap.parse_args(base + ["--save-obj", "--obj-frames", "0,2", "--webvis", "--axis-dir", "r", "--obj-stride", "1", "--obj-bkgd-stride", "4",
                                 "MODEL.DEVICE", "cuda:0"])
    assert full.obj_frames == [0, 2] and full.webvis and full.axis_dir == "r" and (full.obj_stride, full.obj_bkgd_stride) == (1, 4)
    assert full.opts == ["MODEL.DEVICE", "cuda:0"]
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--axis-dir", "up"])
