"""Host-side wrappers over the optimiser-sweep kernels of include/a3d.h: bit-packed masks,
hypothesis projection, IoU matrix.  torch tensors carry device memory only."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from . import _lib
from .ops import _p, _req, _stream

MAX_HYP = 64


def words_per_mask(H: int, W: int) -> int:
    return (H * W + 31) // 32


def pack_masks(masks_u8: torch.Tensor) -> torch.Tensor:
    """[n,H,W] uint8 (non-zero = set) -> [n, words] int32 bit masks."""
    n, H, W = _req(masks_u8, torch.uint8).shape
    bits = torch.empty((n, words_per_mask(H, W)), device=masks_u8.device, dtype=torch.int32)
    _lib.check(_lib.lib().a3d_masks_pack_bits(_p(masks_u8), _p(bits), n, H, W, _stream()), "a3d_masks_pack_bits")
    return bits


def unpack_masks(bits: torch.Tensor, H: int, W: int) -> torch.Tensor:
    n = _req(bits, torch.int32).shape[0]
    out = torch.empty((n, H, W), device=bits.device, dtype=torch.uint8)
    _lib.check(_lib.lib().a3d_masks_unpack_bits(_p(bits), _p(out), n, H, W, _stream()), "a3d_masks_unpack_bits")
    return out


def project_hypotheses(mask_u8: torch.Tensor, normal: Sequence[float], offset: float, pivot: Sequence[float], xforms: torch.Tensor, *,
                       focal: float, cx: float, cy: float) -> torch.Tensor:
    """mask [H,W] uint8 on the device, xforms [A,12] fp32 (R row-major | t) -> bit masks [A, words] of the A re-projections."""
    H, W = _req(mask_u8, torch.uint8).shape
    A = _req(xforms).shape[0]
    assert xforms.shape[1] == 12 and A <= MAX_HYP
    d = _lib.SweepDesc()
    d.mask, d.H, d.W = _p(mask_u8), H, W
    for i in range(3):
        d.normal[i], d.pivot[i] = float(normal[i]), float(pivot[i])
    d.offset, d.focal, d.cx, d.cy = float(offset), float(focal), float(cx), float(cy)
    out = torch.empty((A, words_per_mask(H, W)), device=mask_u8.device, dtype=torch.int32)
    d.xforms, d.A, d.out_bits = _p(xforms), A, _p(out)
    _lib.check(_lib.lib().a3d_project_hypotheses(C.byref(d), _stream()), "a3d_project_hypotheses")
    return out


def mask_iou_matrix(target_bits: torch.Tensor, proj_bits: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """[F,words] x [A,words] -> IoU [F,A] fp32."""
    F_, A = _req(target_bits, torch.int32).shape[0], _req(proj_bits, torch.int32).shape[0]
    iou = torch.empty((F_, A), device=target_bits.device, dtype=torch.float32)
    _lib.check(_lib.lib().a3d_mask_iou_matrix(_p(target_bits), _p(proj_bits), _p(iou), F_, A, H, W, _stream()), "a3d_mask_iou_matrix")
    return iou


def render_panels_tables(frames_u8: torch.Tensor, layer_off: torch.Tensor, layers, pieces, inst_off: torch.Tensor, inst_row, normals, bits, out: torch.Tensor,
                  col: int = 0) -> torch.Tensor:
    """a3d_render_panels over tables that are already on the device (articulation3d_amd/render.py builds and uploads them): frames uint8
    [F,H,W,3]; layer_off / inst_off the [F+1] int32 offsets, layers / pieces the a3d_render_layer / a3d_render_piece records, inst_row
    int32 [n_inst] -- each as a flat uint8 tensor of its bytes (None where empty); normals fp32 [n_inst,3]; bits int32 [n_masks, words].
    Fills out[:, :, col : col+W] (seg panels) and out[:, :, col+W : col+2W] (normal panels) of out uint8 [F,H,pitch,3]."""
    F_, H, W, ch = _req(frames_u8, torch.uint8).shape
    if ch != 3 or _req(out, torch.uint8).dim() != 4 or out.shape[0] != F_ or out.shape[1] != H or out.shape[3] != 3:
        raise ValueError(f"frames {tuple(frames_u8.shape)} / out {tuple(out.shape)}: want [F,H,W,3] and [F,H,pitch,3]")
    nbytes = lambda t: 0 if t is None else _req(t, torch.uint8).numel()
    if nbytes(layer_off) != 4 * (F_ + 1) or nbytes(inst_off) != 4 * (F_ + 1):
        raise ValueError("layer_off / inst_off must hold F + 1 int32 offsets")
    d = _lib.RenderDesc()
    d.frames, d.out, d.layer_off, d.layers, d.pieces, d.inst_off, d.inst_row = (_p(t) for t in (frames_u8, out, layer_off, layers, pieces, inst_off, inst_row))
    d.normals = _p(None if normals is None else _req(normals))
    d.bits = _p(None if bits is None else _req(bits, torch.int32))
    d.F, d.H, d.W, d.pitch, d.col = F_, H, W, out.shape[2], int(col)
    d.n_layers, d.n_pieces = nbytes(layers) // C.sizeof(_lib.RenderLayer), nbytes(pieces) // C.sizeof(_lib.RenderPiece)
    d.n_inst, d.n_masks = nbytes(inst_row) // 4, (0 if bits is None else bits.shape[0])
    if normals is not None and tuple(normals.shape) != (d.n_inst, 3) or normals is None and d.n_inst:
        raise ValueError("normals must be [n_inst,3]")
    if bits is not None and bits.shape[1] != words_per_mask(H, W):
        raise ValueError("bit masks do not have ceil(H*W/32) words per row")
    _lib.check(_lib.lib().a3d_render_panels(C.byref(d), _stream()), "a3d_render_panels")
    return out
