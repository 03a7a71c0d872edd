// The mask head's training step (the mask share of config/step3_plane.yaml): the two launches no other stage has.
//
// Replaces, under autograd, detectron2's mask_rcnn_loss as the reference's ROI heads call it in training (roi_heads.py:_forward_mask ->
// mask_head.py) for a class-agnostic head with bitmask ground truth:
//   a3d_mask_targets  gt_masks.crop_and_resize(proposal_boxes, 28) -- ROIAlign((28, 28), 1.0, sampling_ratio 0, aligned) of the matched
//                     bitmask, >= 0.5 -- once per image on the host side of the step there, here for every live compact row at once;
//   a3d_mask_loss     the 256 -> 1 predictor conv, F.binary_cross_entropy_with_logits(mean) and the backward pass of both, fused so the
//                     28 x 28 x 256 activation (803 KB per ROI, the head's largest) is read once and its gated gradient written once.
// Rows are the compacted foreground ROIs [0, *live).  No atomics anywhere: the same bits on every run.
#include "kernel_prims.h"
#include "../../include/a3d.h"

namespace {
constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / A3D_WAVE;
constexpr int MT_MAX_GRID = 32768;  // samples per bin on a side: a box beyond 28 x this many pixels is not a proposal of any image

// One bilinear sample of a byte mask: the pooler's out-of-range and border rules (samples outside [-1, H] x [-1, W] are 0; coordinates
// clamp to the last row / column, so every read is inside the mask).
__device__ __forceinline__ float mk_bilinear(const uint8_t *__restrict__ p, int H, int W, float y, float x) {
    if (y < -1.0f || y > (float)H || x < -1.0f || x > (float)W) return 0.0f;
    if (y <= 0.0f) y = 0.0f;
    if (x <= 0.0f) x = 0.0f;
    int yl = (int)y, xl = (int)x, yh, xh;
    if (yl >= H - 1) {
        yh = yl = H - 1;
        y = (float)yl;
    } else
        yh = yl + 1;
    if (xl >= W - 1) {
        xh = xl = W - 1;
        x = (float)xl;
    } else
        xh = xl + 1;
    const float ly = y - (float)yl, lx = x - (float)xl, hy = 1.0f - ly, hx = 1.0f - lx;
    const float v1 = p[(size_t)yl * W + xl] ? 1.f : 0.f, v2 = p[(size_t)yl * W + xh] ? 1.f : 0.f;
    const float v3 = p[(size_t)yh * W + xl] ? 1.f : 0.f, v4 = p[(size_t)yh * W + xh] ? 1.f : 0.f;
    return (hy * hx) * v1 + (hy * lx) * v2 + (ly * hx) * v3 + (ly * lx) * v4;
}

// One workgroup per (row, bin row).  Each wave takes every fourth bin; its lanes run over the bin's samples with the sample column
// fastest (neighbouring lanes read neighbouring bytes), each lane sums its samples in sample order, the wave folds the 64 sums.
// The bytes a bin row touches (at most ceil(roi_h / 28) + 2 mask rows) are shared by its 28 bins and by the lanes of a bin through L1.
__global__ __launch_bounds__(MT_THREADS) void mask_targets_kernel(const a3d_mask_targets_desc d) {
    const int S = d.S;
    const int r = blockIdx.x / S, ph = blockIdx.x - r * S;
    if (r >= a3d_live_rows(d.live, d.rows)) return;
    const int wave = threadIdx.x / A3D_WAVE, lane = threadIdx.x % A3D_WAVE;
    int b = 0;
    while (b + 1 < d.B && d.row_offset[b + 1] <= r) ++b;
    const int slot = r - d.row_offset[b], g = d.row_gt[r];
    bool ok = slot >= 0 && slot < d.cap && slot < d.count[b] && (unsigned)g < (unsigned)d.max_gt;
    float x1 = 0.f, y1 = 0.f, bw = 0.f, bh = 0.f;
    int gh = 0, gw = 0;
    if (ok) {
        const float *bx = d.boxes + ((size_t)b * d.cap + slot) * 4;
        x1 = bx[0] - 0.5f;
        y1 = bx[1] - 0.5f;
        const float x2 = bx[2] - 0.5f, y2 = bx[3] - 0.5f;
        const float rw = x2 - x1, rh = y2 - y1;  // (aligned: the box size is not clamped)
        bw = rw / (float)S;
        bh = rh / (float)S;
        ok = fabsf(x1) < 1e30f && fabsf(y1) < 1e30f && rw > 0.f && rh > 0.f && rw < 1e30f && rh < 1e30f;  // (NaN fails every comparison)
        if (ok) {
            gh = (int)ceilf(bh);
            gw = (int)ceilf(bw);
            ok = gh <= MT_MAX_GRID && gw <= MT_MAX_GRID;
        }
    }
    uint8_t *out = d.targets + ((size_t)r * S + ph) * S;
    if (!ok) {  // no area, no ground truth: the empty sum
        for (int pw = threadIdx.x; pw < S; pw += MT_THREADS) out[pw] = 0;
        return;
    }
    const uint8_t *mask = d.masks + ((size_t)b * d.max_gt + g) * ((size_t)d.H * d.W);
    const int n = gh * gw;
    const float cnt = (float)(n > 1 ? n : 1);
    const float ybin = y1 + (float)ph * bh;
    for (int pw = wave; pw < S; pw += MT_WAVES) {
        const float xbin = x1 + (float)pw * bw;
        float acc = 0.f;
        for (int s = lane; s < n; s += A3D_WAVE) {
            const int iy = s / gw, ix = s - iy * gw;
            const float y = ybin + ((float)iy + 0.5f) * bh / (float)gh;
            const float x = xbin + ((float)ix + 0.5f) * bw / (float)gw;
            acc += mk_bilinear(mask, d.H, d.W, y, x);
        }
        acc = a3d_wave_sum(acc);
        if (lane == 0) out[pw] = acc / cnt >= 0.5f ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ predictor + BCE, forward and backward
constexpr int ML_THREADS = 256;
constexpr int ML_WAVES = ML_THREADS / A3D_WAVE;
constexpr int ML_C = 256;            // channels: one wave, four per lane
constexpr int ML_WGS = 1024;         // four workgroups per CU: 16 waves with four 16-byte loads each in flight
constexpr int ML_COLS = ML_C + 4;    // a partial: dw [256] | db | loss | pad
constexpr int ML_STRANDS = ML_THREADS / 4;

// One wave per INPUT pixel (row, iy, ix) = 1024 contiguous floats = the four output pixels (2 iy + dy, 2 ix + dx): four independent
// 16-byte loads per lane, four interleaved dot products, and the lane's 4 x 4 values stay in registers until the gated gradient leaves.
__global__ __launch_bounds__(ML_THREADS) void mask_loss_kernel(const a3d_mask_loss_desc d) {
    __shared__ float part[ML_WAVES][ML_COLS];
    const int live = a3d_live_rows(d.live, d.rows);
    const int P = d.P, PP = P * P, S2 = 2 * P;
    const long long units = (long long)live * PP;
    const float inv = live > 0 ? 1.f / ((float)live * (float)(4 * PP)) : 0.f;
    const int wave = threadIdx.x / A3D_WAVE, lane = threadIdx.x % A3D_WAVE;
    const f32x4 w = a3d_ld4(d.w + lane * 4);
    const float bias = *d.b;
    f32x4 dw = {0.f, 0.f, 0.f, 0.f};
    float db = 0.f, ls = 0.f;
    for (long long u = (long long)blockIdx.x * ML_WAVES + wave; u < units; u += (long long)ML_WGS * ML_WAVES) {
        const size_t at = (size_t)u * (4 * ML_C) + lane * 4;
        f32x4 y[4];
        float p[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) y[q] = a3d_ld4(d.yu + at + q * ML_C);
#pragma unroll
        for (int q = 0; q < 4; ++q) p[q] = __builtin_fmaf(y[q][3], w[3], __builtin_fmaf(y[q][2], w[2], __builtin_fmaf(y[q][1], w[1], y[q][0] * w[0])));
#pragma unroll
        for (int q = 0; q < 4; ++q) p[q] = a3d_wave_sum(p[q]);
        const int r = (int)(u / PP), rem = (int)(u - (long long)r * PP), iy = rem / P, ix = rem - iy * P;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const size_t px = ((size_t)r * S2 + (2 * iy + (q >> 1))) * S2 + (2 * ix + (q & 1));
            const float z = p[q] + bias;
            const float t = d.targets[px] ? 1.f : 0.f;
            const float e = expf(-fabsf(z));  // in (0, 1]: no overflow at any z
            ls += (fmaxf(z, 0.f) - z * t) + log1pf(e);
            const float sg = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
            const float dz = (sg - t) * inv;
            db += dz;
            f32x4 g;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                dw[k] = __builtin_fmaf(dz, y[q][k], dw[k]);
                g[k] = y[q][k] > 0.f ? dz * w[k] : 0.f;  // the deconv's ReLU gate: closed at 0
            }
            a3d_st4(d.dyu + at + q * ML_C, g);
            if (d.z && lane == 0) d.z[px] = z;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) part[wave][lane * 4 + k] = dw[k];
    if (lane == 0) {
        part[wave][ML_C] = db;
        part[wave][ML_C + 1] = ls;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < ML_C + 2; c += ML_THREADS)
        d.workspace[(size_t)blockIdx.x * ML_COLS + c] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
}

// The partials of ML_WGS workgroups, four columns per workgroup: 64 strands sum every 64th partial in order, then a fixed tree.
__global__ __launch_bounds__(ML_THREADS) void mask_loss_reduce_kernel(const a3d_mask_loss_desc d) {
    __shared__ float red[ML_THREADS];
    const int t = threadIdx.x, c = blockIdx.x * 4 + (t & 3), j = t >> 2;
    float s = 0.f;
    if (c < ML_C + 2)
        for (int k = j; k < ML_WGS; k += ML_STRANDS) s += d.workspace[(size_t)k * ML_COLS + c];
    red[t] = s;
    __syncthreads();
    a3d_lds_tree<ML_THREADS, 4>(red);  // (t and t + w hold the same column: w is a multiple of 4)
    if (t < 4 && c < ML_C + 2) {
        float v = red[t];
        if (c == ML_C + 1) {  // the mean's divisor: the device live count
            const int live = a3d_live_rows(d.live, d.rows);
            v = live > 0 ? v * (1.f / ((float)live * (float)(4 * d.P * d.P))) : 0.f;
        }
        d.out[c] = v;
    }
}
}  // namespace

extern "C" int a3d_mask_targets(const a3d_mask_targets_desc *d, void *stream) {
    if (!d || !d->masks || !d->boxes || !d->count || !d->row_offset || !d->row_gt || !d->live || !d->targets) return A3D_ERR_ARG;
    if (d->B <= 0 || d->max_gt <= 0 || d->H <= 0 || d->W <= 0 || d->cap <= 0 || d->rows < 0 || d->S <= 0) return A3D_ERR_ARG;
    if ((long long)d->rows * d->S > 0x7fffffffLL) return A3D_ERR_ARG;
    if (d->rows == 0) return A3D_OK;
    a3d_begin();
    hipLaunchKernelGGL(mask_targets_kernel, dim3(d->rows * d->S), dim3(MT_THREADS), 0, (hipStream_t)stream, *d);
    return a3d_check_launch();
}

extern "C" size_t a3d_mask_loss_workspace_bytes(void) { return (size_t)ML_WGS * ML_COLS * sizeof(float); }

extern "C" int a3d_mask_loss(const a3d_mask_loss_desc *d, void *stream) {
    if (!d || !d->yu || !d->targets || !d->w || !d->b || !d->live || !d->dyu || !d->out || !d->workspace) return A3D_ERR_ARG;
    if (d->rows < 0 || d->P <= 0 || d->P > 16384) return A3D_ERR_ARG;
    if (d->C != ML_C) return A3D_ERR_UNSUPPORTED;
    if (((uintptr_t)d->yu | (uintptr_t)d->dyu | (uintptr_t)d->w) & 15) return A3D_ERR_ARG;
    a3d_begin();
    hipLaunchKernelGGL(mask_loss_kernel, dim3(ML_WGS), dim3(ML_THREADS), 0, (hipStream_t)stream, *d);
    hipLaunchKernelGGL(mask_loss_reduce_kernel, dim3(ML_COLS / 4), dim3(ML_THREADS), 0, (hipStream_t)stream, *d);
    return a3d_check_launch();
}
