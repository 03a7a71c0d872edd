"""The articulated 3-D model of a frame as a textured OBJ: what the reference's `--save-obj` block exports
(tools/inference.py:44-168 + pkg/utils/mesh_utils.py:126-266) -- the most confident articulated plane of the frame in several opened
poses about its predicted axis, two markers at the axis end points, and the rest of the image on the same plane as background.

The meshes are built on the GPU (csrc/mesh.hip through opt_ops.build_mesh) from the detection's bit-packed mask: all poses of the
object come from ONE read of the mask.  Textures and the OBJ / MTL text are host work (PIL, vectorised formatting).

DEPARTURES from the reference, on purpose:
  * The mesh is the DENSE one of get_single_image_mesh's reduce_size=False branch (pkg/utils/vis.py:579-600: a vertex per set pixel,
    up to two triangles per pixel, UVs into the frame itself) on a pixel lattice of `stride`, not get_single_image_mesh_arti's polygon
    mesh (skimage contours + Douglas-Peucker + earcut + a cv2.warpPerspective texture: none of those libraries is here, the route is
    sequential host code, and its get_pcd call passes the focal length where the image height belongs).  The reference's script asks
    for reduce_size = False, which get_single_image_mesh_arti ignores; this is what it asked for.  No rectified texture is needed:
    the texture of every mesh is the frame (tinted per pose).
  * The lift uses the optimiser's intrinsics (opt_utils.FOCAL, the image centre), as the sweeps do.
  * The reference's five rotations include angle 0 for axis_dir 'l' (np.arange(-1.8, 0.1, 0.45) ends at 0) and start at 0 for 'r':
    that copy coincides with the detected pose, which is exported anyway, and is dropped.  'l' gives 1 + 4 poses, 'r' 1 + 3.
  * A translation-class detection (class 1) is opened by four TRANSLATIONS along its axis (steps 0.1 .. 0.4); the reference rotates
    it about a rotation axis it does not have.
  * --webvis' matrix diag(1,-1,-1) is applied to the finished vertices (a3d_mesh_build's flip_yz).  It is a proper rotation, so
    turning the flipped points about the flipped axis, as the reference does, is the same model.
  * The axis markers get one flat (56, 207, 252) texture; the reference blends that colour into a copy of the object's texture and
    gives the markers UVs that do not address it.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from .utils.opt_utils import FOCAL, _axis_angle_to_matrix, _get_pcd, angle_offset_to_axis

POSE_ANGLES = np.float32(np.arange(-1.8, 0.1, 1.8 / 4))[:4]    # axis_dir 'l' (tools/inference.py:116 without its copy at 0)
POSE_ANGLES_R = np.float32(np.arange(0.0, 1.8, 1.8 / 4))[1:]    # axis_dir 'r' (:118 without its copy at 0)
TRAN_STEPS = (0.1, 0.2, 0.3, 0.4)
OBJ_TINT = (252, 116, 81)      # tools/inference.py:153
AXIS_COLOR = (56, 207, 252)    # :157
MARKER_RADIUS = 0.1            # :75

# the icosahedron (pytorch3d's ico_sphere(0) is one): 12 unit vertices on three golden rectangles, 20 faces
_T = (1.0 + 5.0 ** 0.5) / 2.0
ICO_VERTS = np.array([[-1, _T, 0], [1, _T, 0], [-1, -_T, 0], [1, -_T, 0], [0, -1, _T], [0, 1, _T], [0, -1, -_T], [0, 1, -_T],
                      [_T, 0, -1], [_T, 0, 1], [-_T, 0, -1], [-_T, 0, 1]], np.float64) / (1.0 + _T * _T) ** 0.5
ICO_FACES = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                      [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int32)


@dataclass
class Mesh:
    verts: np.ndarray   # [n,3] fp32
    uvs: np.ndarray     # [n,2] fp32
    faces: np.ndarray   # [m,3] int32, 0-based, local to the mesh
    material: str       # a key of ArticulatedModel.textures


@dataclass
class ArticulatedModel:
    meshes: List[Mesh]
    textures: Dict[str, np.ndarray] = field(default_factory=dict)  # material -> uint8 [h,w,3] RGB, in the order of first use
    box_id: int = 0
    kind: str = "rot"   # 'rot' (class 0) | 'tran' (class 1)


def _pack_row(mask_u8: np.ndarray, device):
    """One [H,W] uint8 mask -> its bit row on the device."""
    from . import opt_ops

    return opt_ops.pack_masks(torch.from_numpy(np.ascontiguousarray(mask_u8[None])).to(device))[0]


def _build_mesh(row, H, W, normal, offset, pivot, xforms: np.ndarray, **kw):
    """opt_ops.build_mesh with host arrays out (the one device -> host copy of the mesh)."""
    from . import opt_ops

    v, u, f = opt_ops.build_mesh(row, H, W, normal, offset, pivot, torch.from_numpy(np.ascontiguousarray(xforms, dtype=np.float32)).to(row.device), **kw)
    return v.cpu().numpy(), u.cpu().numpy(), f.cpu().numpy()


def pose_table(kind: str, direction: np.ndarray, pivot3d: np.ndarray, axis_dir: str = "l"):
    """-> (xforms [A,12] fp32 with the identity first, pivot [3] fp32), in sweep_hypotheses' convention: pytorch3d's Rotate multiplies
    row vectors, so the column-vector rotation is the transpose."""
    if axis_dir not in ("l", "r"):
        raise ValueError(f"axis_dir {axis_dir!r}: 'l' or 'r'")
    eye = np.eye(3, dtype=np.float32).reshape(1, 9)
    if kind == "rot":
        angles = POSE_ANGLES if axis_dir == "l" else POSE_ANGLES_R
        R = _axis_angle_to_matrix(angles.astype(np.float64)[:, None] * direction[None, :]).astype(np.float32)
        rot = np.concatenate([np.transpose(R, (0, 2, 1)).reshape(-1, 9), np.zeros((len(R), 3), np.float32)], 1)
        return np.concatenate([np.concatenate([eye, np.zeros((1, 3), np.float32)], 1), rot]), pivot3d.astype(np.float32)
    t = (np.asarray((0.0,) + TRAN_STEPS, np.float64)[:, None] * direction[None, :]).astype(np.float32)
    return np.concatenate([np.tile(eye, (len(t), 1)), t], 1), np.zeros(3, np.float32)


def object_texture(frame_rgb_u8: np.ndarray, i: int) -> np.ndarray:
    """Pose i's tint, blended in float64 as the reference does (tools/inference.py:152-155)."""
    color = np.array([[OBJ_TINT]], np.float64) / 255 * (i / 10 + 1 / 2)
    return ((frame_rgb_u8 / 255.0 + color) / 2 * 255.0).astype(np.uint8)


def articulated_model(pred, frame_rgb_u8: np.ndarray, *, bank=None, frame_idx: int = 0, axis_dir: str = "l", stride: int = 2, bkgd_stride: int = 8,
                      webvis: bool = False, device="cuda") -> Optional[ArticulatedModel]:
    """The model of one frame: `pred` its Instances (host fields, as optimize_planes returns them), frame_rgb_u8 [H,W,3] the frame at
    the masks' size.  `bank` (an opt_utils._MaskBank of the clip) supplies the packed mask of (frame_idx, box) when it holds it.
    None when the frame has no instance, the top one's plane has zero length or its axis end points coincide."""
    scores = np.asarray(pred.scores.cpu() if isinstance(pred.scores, torch.Tensor) else pred.scores)
    if len(scores) == 0:
        return None
    box = int(scores.argmax())
    H, W = frame_rgb_u8.shape[:2]
    plane = pred.pred_planes[box].clone().float()
    plane = torch.stack((plane[0], -plane[2], plane[1]))  # (a, b, c) -> (a, -c, b)
    offset = torch.norm(plane, p=2)
    if not float(offset) > 0.0:
        return None
    normal = torch.nn.functional.normalize(plane[None], p=2)[0]
    kind = "tran" if int(pred.pred_classes[box]) == 1 else "rot"
    centers = pred.pred_boxes.get_centers()
    if kind == "rot":
        pts = angle_offset_to_axis(pred.pred_rot_axis, centers, H, W)
    else:
        at = pred.pred_tran_axis
        pts = angle_offset_to_axis(torch.cat((at, torch.zeros(len(at), 1)), 1), centers, H, W)
    ends = pts[box].reshape(2, 2).numpy()
    if (ends[0] == ends[1]).all():
        return None
    axis3d = _get_pcd(ends, normal.numpy(), offset.item(), h=H, w=W)
    d = axis3d[1] - axis3d[0]
    length = np.linalg.norm(d)
    if not (np.isfinite(length) and length > 0):
        return None
    xforms, pivot = pose_table(kind, d / length, axis3d[0], axis_dir)

    mask = (pred.pred_masks[box] > 0.5).to(torch.uint8).cpu().numpy()
    if bank is not None and (frame_idx, box) in bank.index and (bank.H, bank.W) == (H, W):
        row = bank.bits[bank.index[(frame_idx, box)]]
    else:
        row = _pack_row(mask, device)
    cam = dict(focal=FOCAL, cx=W / 2, cy=H / 2, flip_yz=bool(webvis))
    n3, off = normal.tolist(), offset.item()
    verts, uvs, faces = _build_mesh(row, H, W, n3, off, pivot.tolist(), xforms, stride=stride, invert=False, **cam)
    bv, bu, bf = _build_mesh(row, H, W, n3, off, [0.0, 0.0, 0.0], xforms[:1], stride=bkgd_stride, invert=True, **cam)

    model = ArticulatedModel([], {}, box, kind)
    for i in range(len(xforms)):
        model.meshes.append(Mesh(verts[i], uvs, faces, f"obj_pose{i}"))
        model.textures[f"obj_pose{i}"] = object_texture(frame_rgb_u8, i)
    flip = np.array([1.0, -1.0, -1.0]) if webvis else np.ones(3)
    for end in axis3d:
        model.meshes.append(Mesh((ICO_VERTS * MARKER_RADIUS + end * flip).astype(np.float32), np.full((len(ICO_VERTS), 2), 0.5, np.float32), ICO_FACES, "axis"))
    model.textures["axis"] = np.broadcast_to(np.array(AXIS_COLOR, np.uint8), (4, 4, 3)).copy()
    model.meshes.append(Mesh(bv[0], bu, bf, "bkgd"))
    model.textures["bkgd"] = np.ascontiguousarray(frame_rgb_u8)
    return model


_MTL_BLOCK = ("newmtl {name}\nmap_Kd uv_maps/{name}.png\n# Test colors\nKa 1.000 1.000 1.000  # white\nKd 1.000 1.000 1.000  # white\n"
              "Ks 0.000 0.000 0.000  # black\nNs 10.0\n")


def _rows(fmt: str, values: np.ndarray) -> str:
    """One C-level format of every row of `values` with the row template `fmt` (no Python loop per element)."""
    return (fmt * len(values)) % tuple(values.ravel().tolist()) if len(values) else ""


def save_obj(folder: str, prefix: str, model: ArticulatedModel, decimal_places: int = 10, double_sided: bool = True) -> str:
    """<folder>/<prefix>.obj + <prefix>.mtl + uv_maps/<material>.png in the reference's layout (mesh_utils.py:126-266): `mtllib`, a
    blank line, then per mesh `# mesh i`, its `v` lines, its `vt` lines, `usemtl`, and `f a/a b/b c/c` with 1-based indices that run on
    across the meshes, each face followed by its reversed copy when double_sided.  -> the .obj's path."""
    from PIL import Image

    os.makedirs(os.path.join(folder, "uv_maps"), exist_ok=True)
    for name, tex in model.textures.items():
        Image.fromarray(np.ascontiguousarray(tex)).save(os.path.join(folder, "uv_maps", name + ".png"))
    with open(os.path.join(folder, prefix + ".mtl"), "w") as f:
        f.write("".join(_MTL_BLOCK.format(name=name) for name in model.textures))
    num = "%%.%df" % decimal_places
    v_fmt, vt_fmt = f"v {num} {num} {num}\n", f"vt {num} {num}\n"
    f_fmt = "f %d/%d %d/%d %d/%d\n" * (2 if double_sided else 1)
    order = [0, 0, 1, 1, 2, 2] + ([2, 2, 1, 1, 0, 0] if double_sided else [])
    path = os.path.join(folder, prefix + ".obj")
    base = 1
    with open(path, "w") as f:
        f.write(f"mtllib {prefix}.mtl\n\n")
        for i, m in enumerate(model.meshes):
            if m.material not in model.textures:
                raise ValueError(f"mesh {i}: material {m.material!r} has no texture")
            f.write(f"# mesh {i}\n")
            f.write(_rows(v_fmt, np.asarray(m.verts, np.float64)))
            f.write(_rows(vt_fmt, np.asarray(m.uvs, np.float64)))
            f.write(f"usemtl {m.material}\n")
            f.write(_rows(f_fmt, (np.asarray(m.faces, np.int64).reshape(-1, 3) + base)[:, order]))
            base += len(m.verts)
    return path
