"""The law of a3d_render_panels (include/a3d.h) in numpy: fp32 arithmetic for the half-plane value e and the normal value v,
integers for the blend.  Written from the stated law; it shares no rasterising code with the package (it only reads the
tables' fields: layers kind / alpha / color / p0 / p1, pieces n / abc).

    seg     start from the frame; per layer in table order, a covered pixel's channels become
            (old*(256-a) + colour*a + 128) >> 8, once per layer.  MASK: the mask bit.  POLY: OR over the pieces, inside a
            piece iff (A*px + B*py) + C >= 0 for each of its n half-planes, px = x + 0.5f, py = y + 0.5f, fp32.
    normal  n = sum_i bit_i * normal_i in fp32, ascending;  v = (n + 1) / 2 * 255;  byte = int32(trunc v) & 0xff.
The cull box is NOT read: it may never change a byte.
"""
import numpy as np

MASK, POLY = 0, 1
F32 = np.float32


def pack_bits(masks: np.ndarray) -> np.ndarray:
    """[n,H,W] (non-zero = set) -> uint32 [n, ceil(H*W/32)]: bit i of word w = pixel 32w+i, row-major."""
    n = masks.shape[0]
    npix = int(np.prod(masks.shape[1:]))
    words = (npix + 31) // 32
    flat = np.zeros((n, words * 32), np.uint8)
    flat[:, :npix] = masks.reshape(n, npix) != 0
    return np.packbits(flat, axis=1, bitorder="little").view("<u4").reshape(n, words)


def mask_of(bits: np.ndarray, row: int, H: int, W: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(bits[row]).view(np.uint8), bitorder="little")[:H * W].reshape(H, W).astype(bool)


def piece_coverage(piece, H: int, W: int) -> np.ndarray:
    px = np.arange(W, dtype=F32) + F32(0.5)
    py = np.arange(H, dtype=F32) + F32(0.5)
    n = int(piece["n"])
    inside = np.full((H, W), n > 0)
    for h in range(min(n, 4)):
        A, B, C = (F32(t) for t in piece["abc"][h])
        e = ((A * px)[None, :] + (B * py)[:, None]) + C
        assert e.dtype == np.float32
        inside &= e >= 0
    return inside


def layer_coverage(layer, pieces, bits, H: int, W: int) -> np.ndarray:
    if int(layer["kind"]) == MASK:
        return mask_of(bits, int(layer["p0"]), H, W)
    cov = np.zeros((H, W), bool)
    for q in range(int(layer["p0"]), int(layer["p1"])):
        cov |= piece_coverage(pieces[q], H, W)
    return cov


def seg_panel(frame: np.ndarray, layers, pieces, bits) -> np.ndarray:
    H, W, _ = frame.shape
    img = frame.astype(np.int64)
    for layer in layers:
        cov = layer_coverage(layer, pieces, bits, H, W)
        a = int(layer["alpha"])
        col = np.asarray(layer["color"], np.int64)[:3]
        img[cov] = (img[cov] * (256 - a) + col[None, :] * a + 128) >> 8
    return img.astype(np.uint8)


def normal_value(rows, normals: np.ndarray, bits, H: int, W: int) -> np.ndarray:
    """v of the law, fp32 [H,W,3]."""
    n = np.zeros((H, W, 3), F32)
    for row, nrm in zip(rows, np.asarray(normals, F32)):
        n = n + mask_of(bits, int(row), H, W).astype(F32)[..., None] * nrm[None, None, :]
    v = (n + F32(1.0)) / F32(2.0) * F32(255.0)
    assert v.dtype == np.float32
    return v


def normal_panel(rows, normals, bits, H: int, W: int) -> np.ndarray:
    return (normal_value(rows, normals, bits, H, W).astype(np.int32) & 0xFF).astype(np.uint8)


def render(frames: np.ndarray, layer_off, layers, pieces, inst_off, inst_row, normals, bits, out: np.ndarray, col: int = 0) -> np.ndarray:
    """The whole call: fills out[:, :, col : col+2W] and leaves every other byte alone."""
    F, H, W, _ = frames.shape
    assert col >= 0 and col + 2 * W <= out.shape[2]
    for f in range(F):
        out[f, :, col:col + W] = seg_panel(frames[f], layers[int(layer_off[f]):int(layer_off[f + 1])], pieces, bits)
        i0, i1 = int(inst_off[f]), int(inst_off[f + 1])
        out[f, :, col + W:col + 2 * W] = normal_panel(inst_row[i0:i1], np.asarray(normals)[i0:i1], bits, H, W)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# seeded cases shared by the host and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def make_instances(rng: np.random.Generator, H: int, W: int, n: int, scores=None):
    """n hand-made detections on an H x W image: boxes inside the image, blob masks inside the boxes, both classes."""
    import torch

    from articulation3d_amd.structures import Boxes, Instances

    inst = Instances((H, W))
    x0 = rng.uniform(0, W * 0.5, n)
    y0 = rng.uniform(0, H * 0.5, n)
    bw, bh = rng.uniform(W * 0.2, W * 0.5, n), rng.uniform(H * 0.2, H * 0.5, n)
    boxes = np.stack([x0, y0, np.minimum(x0 + bw, W - 1), np.minimum(y0 + bh, H - 1)], 1).astype(np.float32)
    masks = np.zeros((n, H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for i, (bx0, by0, bx1, by1) in enumerate(boxes):
        cx, cy = (bx0 + bx1) / 2, (by0 + by1) / 2
        masks[i] = (((xx - cx) / max((bx1 - bx0) / 2, 1)) ** 2 + ((yy - cy) / max((by1 - by0) / 2, 1)) ** 2 <= 1.0)
    ang = rng.uniform(0, 2 * np.pi, n)
    inst.pred_boxes = Boxes(torch.from_numpy(boxes))
    inst.scores = np.asarray(scores if scores is not None else rng.uniform(0.75, 1.0, n), np.float32)
    inst.pred_classes = torch.from_numpy((np.arange(n) % 2).astype(np.int64))
    inst.pred_planes = torch.from_numpy(rng.normal(size=(n, 3)).astype(np.float32))
    inst.pred_rot_axis = torch.from_numpy(np.stack([np.sin(ang), np.cos(ang), rng.uniform(-0.05, 0.05, n)], 1).astype(np.float32))
    inst.pred_tran_axis = torch.from_numpy(np.stack([np.sin(ang[::-1]), np.cos(ang[::-1])], 1).astype(np.float32))
    inst.pred_masks = torch.from_numpy(masks)
    return inst


def render_tables(frames: np.ndarray, tables, normals, bits, out: np.ndarray, col: int = 0) -> np.ndarray:
    """`render` over a render.LayerTables object."""
    return render(frames, tables.layer_off, tables.layers, tables.pieces, tables.inst_off, tables.inst_row, np.asarray(normals), bits, out, col)
