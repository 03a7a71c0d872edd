#!/usr/bin/env python3
"""Timing of the three evaluation launches (articulation3d_amd/opt_ops eval_match / eval_ap / depth_l1, csrc/eval.hip) on a seeded
synthetic dataset -> one JSON line.

    python tools/eval_bench.py [--images 5000] [--dets 100] [--gts 3] [--iters 200]

  * match_us: a3d_eval_match over every detection of every image, one prebuilt descriptor (device events around `--iters`
    back-to-back calls after a warm-up);  match_call_us: the same through opt_ops.eval_match, which converts and uploads the
    offsets and allocates the outputs per call;
  * ap_us: a3d_eval_ap over the valid detections' sorted true-positive bits, two classes;  sort_us: the three torch.sort calls
    and gathers that put the entries in order, for scale;
  * depth_us: a3d_depth_l1 over `--depth-batch` 480x640 maps, and the GB/s of the two maps it reads;
  * evaluate_ms: ArtiEvaluator.evaluate() end to end on the same detections fed as packed records (wall time, host work included);
  * mask_counts: a3d_eval_mask_counts (csrc/plane_eval.hip) on one detector batch -- `--mask-batch` images of `--dets` pasted
    480x640 masks, `--mask-gts` ground truths each -- and, alternating with it in the same process, the route the library offered
    before for the same numbers: opt_ops.pack_masks on the batch's masks, then mask_iou_matrix per image.  `--mask-rounds` rounds of
    both; the medians, each route's spread over the rounds (max - min) and the new launch's GB/s from N*H*W + N*words*4 bytes.
Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(n_img: int, D: int, G: int, seed: int = 0):
    """Vectorised: G ground truths per image, D detections jittered around them.  -> det [I,D,14], gt_f [I*G,7], gt_i [I*G,12]."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 300, (n_img, G, 2))
    wh = rng.uniform(80, 200, (n_img, G, 2))
    gbox = np.concatenate([xy, xy + wh], 2)
    n = rng.normal(size=(n_img, G, 3))
    gt_f = np.concatenate([gbox, n / np.linalg.norm(n, axis=2, keepdims=True)], 2).astype(np.float32)
    gt_i = np.zeros((n_img, G, 12), np.int32)
    gt_i[..., 0] = gt_i[..., 1] = rng.integers(0, 2, (n_img, G))
    for base in (2, 7):
        gt_i[..., base:base + 4] = rng.integers(0, 480, (n_img, G, 4))
        gt_i[..., base + 4] = 1
    pick = rng.integers(0, G, (n_img, D))
    src = np.take_along_axis(gt_f, pick[..., None], 1)
    det = np.zeros((n_img, D, 14), np.float32)
    det[..., :4] = src[..., :4] + rng.uniform(-1, 1, (n_img, D, 4)) * rng.choice([3.0, 12.0, 40.0], (n_img, D, 1))
    det[..., 4] = rng.uniform(0.05, 1, (n_img, D))
    det[..., 5] = np.take_along_axis(gt_i[..., 0], pick, 1)
    det[..., 6:9] = src[..., [4, 6, 5]] + rng.normal(size=(n_img, D, 3)) * 0.3
    ang = rng.uniform(0, 2 * np.pi, (n_img, D))
    det[..., 9], det[..., 10], det[..., 11] = np.sin(ang), np.cos(ang), rng.uniform(0, 1, (n_img, D))
    det[..., 12], det[..., 13] = np.sin(ang), np.cos(ang)
    return det, gt_f.reshape(-1, 7), gt_i.reshape(-1, 12)


def timed(call, iters):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def bench_mask_counts(B: int, R: int, G: int, rounds: int, iters: int, H: int = 480, W: int = 640):
    """-> dict: the new launch against pack_masks + mask_iou_matrix per image, alternating, on B x R masks with G ground truths each."""
    from articulation3d_amd import opt_ops

    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)

    def boxes(n):
        xy = torch.rand((n, 2), device=dev, generator=gen) * torch.tensor([W - 200.0, H - 160.0], device=dev)
        wh = 60 + torch.rand((n, 2), device=dev, generator=gen) * torch.tensor([140.0, 100.0], device=dev)
        return torch.cat([xy, xy + wh], 1)

    def fill(b):  # [n,4] -> uint8 [n,H,W]: the box's rectangle, 255 inside as a pasted mask has it
        yy, xx = torch.arange(H, device=dev)[None, :, None], torch.arange(W, device=dev)[None, None, :]
        return (((xx >= b[:, 0, None, None]) & (xx < b[:, 2, None, None]) & (yy >= b[:, 1, None, None]) & (yy < b[:, 3, None, None])).to(torch.uint8) * 255).contiguous()

    N, M = B * R, B * G
    gbox = boxes(M)
    src = (torch.arange(B, device=dev)[:, None] * G + torch.randint(0, G, (B, R), device=dev, generator=gen)).reshape(-1)
    dbox = gbox[src] + (torch.rand((N, 4), device=dev, generator=gen) - 0.5) * 40
    det = torch.zeros((N, 14), device=dev)
    det[:, :4] = dbox
    gt = torch.zeros((M, 8), device=dev)
    gt[:, :4] = gbox
    masks = torch.cat([fill(dbox[at:at + 100]) for at in range(0, N, 100)])
    gt_bits = opt_ops.pack_masks(fill(gbox))
    det_off, gt_off = [b * R for b in range(B + 1)], [b * G for b in range(B + 1)]
    slot = torch.arange(N, device=dev, dtype=torch.int32)
    words = opt_ops.words_per_mask(H, W)

    new = lambda: opt_ops.eval_mask_counts(det, det_off, gt, gt_off, masks, slot, gt_bits)

    def old():
        bits = opt_ops.pack_masks(masks)
        return [opt_ops.mask_iou_matrix(bits[b * R:(b + 1) * R], gt_bits[b * G:(b + 1) * G], H, W) for b in range(B)]

    gt_id, inter, uni = new()
    iou = torch.cat(old())  # [N,G] fp32: the column of each detection's ground truth is inter / uni
    mine = torch.where(uni > 0, inter.double() / uni.double().clamp(min=1), torch.zeros((), device=dev, dtype=torch.float64))
    assert float((iou.gather(1, gt_id.long()[:, None])[:, 0].double() - mine).abs().max()) < 1e-6
    t_new, t_old = [], []
    for _ in range(rounds):
        t_new.append(timed(new, iters))
        t_old.append(timed(old, iters))
    med = lambda v: float(np.median(v))
    nbytes = N * H * W + N * words * 4
    return {"batch": B, "dets_per_image": R, "gts_per_image": G, "hw": [H, W], "rounds": rounds, "iters": iters,
            "new_us": round(med(t_new), 1), "new_spread_us": round(max(t_new) - min(t_new), 1),
            "pack_then_iou_us": round(med(t_old), 1), "pack_then_iou_spread_us": round(max(t_old) - min(t_old), 1),
            "new_gbps": round(nbytes / med(t_new) / 1e3, 1), "mean_mask_iou": round(float(mine.mean()), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--gts", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--depth-batch", type=int, default=16)
    ap.add_argument("--mask-batch", type=int, default=16)
    ap.add_argument("--mask-gts", type=int, default=8)
    ap.add_argument("--mask-rounds", type=int, default=7)
    ap.add_argument("--mask-iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a GPU")
    import ctypes as C

    from articulation3d_amd import _lib, evaluation, opt_ops

    dev = torch.device("cuda")
    I, D, G = args.images, args.dets, args.gts
    det, gt_f, gt_i = synthetic(I, D, G)
    d_det = torch.from_numpy(det.reshape(-1, 14)).to(dev)
    d_gt_f, d_gt_i = torch.from_numpy(gt_f).to(dev), torch.from_numpy(gt_i).to(dev)
    det_off, gt_off = (np.arange(I + 1) * D).tolist(), (np.arange(I + 1) * G).tolist()
    d_gt_off = torch.tensor(gt_off, dtype=torch.int32, device=dev)
    match_call_us = timed(lambda: opt_ops.eval_match(d_det, det_off, d_gt_f, d_gt_i, gt_off, gt_off_dev=d_gt_off), args.iters)
    m = opt_ops.eval_match(d_det, det_off, d_gt_f, d_gt_i, gt_off, gt_off_dev=d_gt_off)
    # the launch alone: one descriptor, built once (the wrapper converts and uploads 2 x (I + 1) offsets per call, host work)
    d = _lib.EvalMatchDesc()
    d_det_off = torch.tensor(det_off, dtype=torch.int32, device=dev)
    h_det_off, h_gt_off = (C.c_int * (I + 1))(*det_off), (C.c_int * (I + 1))(*gt_off)
    d.det, d.gt_f, d.gt_i, d.det_off, d.gt_off = d_det.data_ptr(), d_gt_f.data_ptr(), d_gt_i.data_ptr(), d_det_off.data_ptr(), d_gt_off.data_ptr()
    d.det_off_host, d.gt_off_host = h_det_off, h_gt_off
    d.I, d.N, d.M, d.img_h, d.img_w = I, I * D, I * G, 480, 640
    d.filter_iou, d.iou_thresh, d.normal_thresh = 0.7, 0.5, 30.0
    scratch = {k: torch.empty_like(v) for k, v in m.items()}
    d.gt_id, d.iou, d.ea, d.normal_err, d.rank, d.tp = (scratch[k].data_ptr() for k in ("gt_id", "iou", "ea", "normal_err", "rank", "tp"))
    stream = torch.cuda.current_stream().cuda_stream
    match_us = timed(lambda: _lib.check(_lib.lib().a3d_eval_match(C.byref(d), stream), "a3d_eval_match"), args.iters)
    assert all(torch.equal(scratch[k], m[k]) for k in ("gt_id", "rank", "tp", "iou"))
    valid = m["gt_id"] >= 0
    score, cls, tp = d_det[valid, 4], d_det[valid, 5], m["tp"][valid]

    def order():
        o = torch.sort(score, descending=True, stable=True)[1]
        return o[torch.sort(cls[o], stable=True)[1]]

    sort_us = timed(order, args.iters)
    o = order()
    tp_sorted = tp[o].contiguous()
    seg = np.concatenate([[0], np.cumsum(np.bincount(cls[o].long().cpu().numpy(), minlength=2)[:2])]).tolist()
    npos = np.bincount(gt_i[:, 0], minlength=2)[:2].tolist()
    ap_us = timed(lambda: opt_ops.eval_ap(tp_sorted, seg, npos), args.iters)
    ap_table, _ = opt_ops.eval_ap(tp_sorted, seg, npos)

    B = args.depth_batch
    pred, gtd = torch.rand(B, 480, 640, device=dev) * 4, torch.rand(B, 480, 640, device=dev) * 4
    depth_us = timed(lambda: opt_ops.depth_l1(pred, gtd), args.iters)

    mask_counts = bench_mask_counts(args.mask_batch, D, args.mask_gts, args.mask_rounds, args.mask_iters)

    gt = evaluation.ArtiGroundTruth(list(range(I)), gt_f, gt_i, gt_off, npos, ["arti_rot", "arti_tran"], ["arti_rot", "arti_tran"], dev)
    ev = evaluation.ArtiEvaluator(gt)
    step = 64
    rec = torch.from_numpy(det).to(dev)
    cnt = torch.full((I,), D, dtype=torch.int32, device=dev)
    for at in range(0, I, step):
        ev.process_records(list(range(at, min(at + step, I))), rec[at:at + step], cnt[at:at + step])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ev.evaluate()
    evaluate_ms = (time.perf_counter() - t0) * 1e3
    assert all(abs(res[f"{name} - {c}"] - float(ap_table[k, j])) < 1e-12 for k, name in enumerate(evaluation.METRICS) for j, c in enumerate(gt.names))
    print(json.dumps({"bench": "eval", "device": torch.cuda.get_device_name(0), "images": I, "dets_per_image": D, "gts_per_image": G,
                      "iters": args.iters, "valid_detections": int(valid.sum()), "match_us": round(match_us, 1), "match_call_us": round(match_call_us, 1), "sort_us": round(sort_us, 1),
                      "ap_us": round(ap_us, 1), "depth_batch": B, "depth_us": round(depth_us, 1),
                      "depth_gbps": round(2 * B * 480 * 640 * 4 / depth_us / 1e3, 1), "evaluate_ms": round(evaluate_ms, 1), "mask_counts": mask_counts,
                      "ap": {k: round(v, 6) for k, v in res.items()}}))


if __name__ == "__main__":
    main()
