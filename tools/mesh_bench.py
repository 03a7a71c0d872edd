#!/usr/bin/env python3
"""Timing of the dense mesh builder (articulation3d_amd/opt_ops.build_mesh, csrc/mesh.hip) -> one JSON line.

    python tools/mesh_bench.py [--iters 200] [--poses 5]

At 480x640, for a full mask and for a typical detection mask (one blob, ~12 % of the image), at stride 1 and 2, `--poses` poses:
  * build_us / written_MB / gbps: a3d_mesh_build's launches into preallocated worst-case buffers (device events around `--iters`
    back-to-back calls after a warm-up; no count read-back), and the bytes of vertices, UVs and faces it writes over that time;
  * torch_us: the same mesh from stock torch ops on the device (nonzero / cumsum / gathers / stack), what a user would otherwise
    write -- checked against the kernel's output (faces exactly, UVs to 1e-6 and vertices to 1e-4: fp32 throughout is not the law's float64 lift);
  * build_mesh_us: opt_ops.build_mesh end to end (allocation, the launches, the one read-back of the counts), wall time;
  * d2h_ms: the mesh's copy to the host;  save_obj_ms: articulation3d_amd.mesh.save_obj of an articulated model built from that
    mask (object at `stride`, background at stride 8), host time for the OBJ / MTL text and the PNG textures.
Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 480, 640


def torch_mesh(mask_b, normal, offset, pivot, xf, stride):
    """The same mesh from stock torch ops (fp32 throughout)."""
    live = mask_b[::stride, ::stride]
    idx = (torch.cumsum(live.reshape(-1).to(torch.int32), 0, dtype=torch.int32) - 1).reshape(live.shape)
    ly, lx = torch.nonzero(live, as_tuple=True)
    x, y = (lx * stride).float(), (ly * stride).float()
    rx, ry = (x - W / 2) / 517.97, (y - H / 2) / 517.97
    depth = offset / (normal[0] * rx + normal[1] * ry + normal[2])
    q = torch.stack((depth * rx, depth * ry, depth), 1) - pivot
    R, t = xf[:, :9].reshape(-1, 3, 3), xf[:, 9:]
    verts = torch.einsum("aij,nj->ani", R, q) + (pivot + t)[:, None, :]
    uvs = torch.stack((x / W, 1.0 - y / H), 1)
    src, right, below, diag = live[:-1, :-1], live[:-1, 1:], live[1:, :-1], live[1:, 1:]
    k, kr, kb, kd = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    both = torch.stack((torch.stack((k, kd, kr), -1), torch.stack((k, kb, kd), -1)), 2)
    keep = torch.stack((src & right & diag, src & below & diag), 2)
    return verts, uvs, both[keep]


def timed(call, iters):
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--poses", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench needs a GPU")
    import mesh_ref as M

    from articulation3d_amd import mesh, opt_ops

    dev = torch.device("cuda")
    A = args.poses
    normal, offset, pivot, xf = M.plane_and_poses(A, H, W)
    dxf = torch.from_numpy(xf).to(dev)
    cam = dict(focal=M.FOCAL, cx=W / 2, cy=H / 2)
    rows = []
    for name, mask in (("full", M.mask_full(H, W)), ("detection", M.mask_blobs(H, W, 4, n=1))):
        row = torch.from_numpy(M.pack_bits(mask)).to(dev)
        mask_b = torch.from_numpy(mask != 0).to(dev)
        for stride in (1, 2):
            _Lh, _Lw, cap_v, cap_f = opt_ops.mesh_lattice(H, W, stride)
            verts = torch.empty((A, cap_v, 3), device=dev)
            uvs = torch.empty((cap_v, 2), device=dev)
            faces = torch.empty((cap_f, 3), dtype=torch.int32, device=dev)
            counts = torch.empty(2, dtype=torch.int32, device=dev)
            call = lambda: opt_ops.mesh_build_into(row, H, W, normal.tolist(), float(offset), pivot.tolist(), dxf, verts, uvs, faces, counts, stride=stride, **cam)
            build_us = timed(call, args.iters)
            n, m = counts.tolist()
            written = A * n * 12 + n * 8 + m * 12 + 8
            tn, tp = torch.from_numpy(normal).to(dev), torch.from_numpy(pivot).to(dev)
            torch_us = timed(lambda: torch_mesh(mask_b, tn, float(offset), tp, dxf, stride), max(args.iters // 10, 5))
            tv, tu, tf = torch_mesh(mask_b, tn, float(offset), tp, dxf, stride)
            assert torch.equal(tf.to(torch.int32), faces[:m]), "torch ops and kernel disagree on the faces"
            assert n == 0 or (float((tu - uvs[:n]).abs().max()) < 1e-6 and float((tv - verts[:, :n]).abs().max()) < 1e-4)

            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                got = opt_ops.build_mesh(row, H, W, normal.tolist(), float(offset), pivot.tolist(), dxf, stride=stride, **cam)
            build_mesh_us = (time.perf_counter() - t0) / 20 * 1e6
            t0 = time.perf_counter()
            host = [t.cpu() for t in got]
            d2h_ms = (time.perf_counter() - t0) * 1e3
            del host

            # save_obj on an articulated model over this mask
            inst, _ = M.handmade_instances(H, W)
            inst.pred_masks[int(np.argmax(inst.scores))] = torch.from_numpy(mask.astype(np.float32))
            frame = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
            model = mesh.articulated_model(inst, frame, stride=stride, bkgd_stride=8, device=dev)
            with tempfile.TemporaryDirectory() as tmp:
                t0 = time.perf_counter()
                path = mesh.save_obj(tmp, "arti_pred", model)
                save_ms = (time.perf_counter() - t0) * 1e3
                obj_mb = os.path.getsize(path) / 1e6
            rows.append({"mask": name, "stride": stride, "poses": A, "verts": n, "faces": m, "build_us": round(build_us, 2),
                         "written_MB": round(written / 1e6, 2), "gbps": round(written / build_us / 1e3, 1), "torch_us": round(torch_us, 1),
                         "build_mesh_us": round(build_mesh_us, 1), "d2h_ms": round(d2h_ms, 2), "save_obj_ms": round(save_ms, 1), "obj_MB": round(obj_mb, 1)})
    print(json.dumps({"bench": "mesh_build", "device": torch.cuda.get_device_name(0), "HxW": [H, W], "iters": args.iters, "rows": rows}))


if __name__ == "__main__":
    main()
