// The plane-normal head's training step (the plane share of config/step3_plane.yaml): the one launch pair no other stage has.
//
// Replaces, under autograd, pkg/modeling/roi_heads/plane_head.py:80-82 (param_pred, the 1024 -> 3 layer, and F.normalize) and :96-124
// (plane_rcnn_loss: smooth_l1_loss(pred, F.normalize(gt), beta 0.0, "sum") * loss_weight / len(pred) -- an L1 SUM over the foreground
// rows divided by their number, not by 3 x their number) plus the backward pass of all three, in one pass over the FC's activation:
//   a3d_plane_loss  raw = w . h + b,  pred = raw / max(|raw|, 1e-12),  loss = k sum |pred - gt|,  k = loss_weight / *live,
//                   draw = normalise-backward(k sign(pred - gt)),  dh = (h > 0) ? w^T draw : 0,  dw = sum draw x h,  db = sum draw.
// Rows are the compacted foreground ROIs [0, *live).  *live is known before any row is read, so k needs no first pass.  One wave per row;
// no atomics anywhere: the same bits on every run.
#include "kernel_prims.h"
#include "../../include/a3d.h"

namespace {
constexpr int PL_THREADS = 256;
constexpr int PL_WAVES = PL_THREADS / A3D_WAVE;
constexpr int PL_WGS = 64;                    // a fixed grid: 256 waves, one row each up to 256 live rows (two images' cap)
constexpr int PL_PARTS = PL_WGS * PL_WAVES;   // partials in the workspace, one per wave
constexpr int PL_MAX_NV = 4;                  // 16-byte loads per lane and row: K = 256 NV <= 1024
constexpr int PL_RED_COLS = 16;               // the reduce launch: 16 columns x 16 strands per workgroup
constexpr int PL_RED_STRANDS = PL_THREADS / PL_RED_COLS;
constexpr float PL_EPS = 1e-12f;              // F.normalize's eps

__device__ __forceinline__ float pl_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }  // (abs backward: 0 at 0)

// One wave per row, rows gw, gw + PL_PARTS, ...: the lane holds columns q * 256 + lane * 4 + (0..3), q < NV, of the row and of the three
// weight rows in registers.  NV independent 16-byte loads, three interleaved dot products folded over the wave by a butterfly (a fixed
// order), the row's scalar work in every lane alike, the gated gradient out as 16-byte stores, dw in 3 x NV x 4 register partials.
template <int NV>
__global__ __launch_bounds__(PL_THREADS) void plane_loss_kernel(const a3d_plane_loss_desc d) {
    constexpr int K = NV * 256;
    const int live = a3d_live_rows(d.live, d.rows);
    const int lane = threadIdx.x % A3D_WAVE, gw = blockIdx.x * PL_WAVES + threadIdx.x / A3D_WAVE;
    if (gw >= live) return;  // (wave-uniform; the reduce launch reads the partials of the waves [0, min(live, PL_PARTS)) only)
    const float k = d.loss_weight / (float)live;
    f32x4 w[3][NV], dw[3][NV];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            w[j][q] = a3d_ld4(d.w + (size_t)j * K + q * 256 + lane * 4);
            dw[j][q] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const float bias[3] = {d.b[0], d.b[1], d.b[2]};
    float db[3] = {0.f, 0.f, 0.f}, ls = 0.f;
    for (int r = gw; r < live; r += PL_PARTS) {
        const size_t at = (size_t)r * K + lane * 4;
        f32x4 h[NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) h[q] = a3d_ld4(d.h + at + q * 256);
        float raw[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float acc = h[0][0] * w[j][0][0];
#pragma unroll
            for (int q = 0; q < NV; ++q) {
#pragma unroll
                for (int c = (q == 0 ? 1 : 0); c < 4; ++c) acc = __builtin_fmaf(h[q][c], w[j][q][c], acc);
            }
            raw[j] = acc;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) raw[j] = a3d_wave_sum(raw[j]);
#pragma unroll
        for (int j = 0; j < 3; ++j) raw[j] += bias[j];
        if (d.raw && lane == 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) d.raw[(size_t)r * 3 + j] = raw[j];
        }
        // the row's loss terms and the gradient of its raw vector: every lane computes the same values
        const int img = d.row_img[r], g = d.row_gt[r];
        float dr[3] = {0.f, 0.f, 0.f};
        if ((unsigned)img < (unsigned)d.B && (unsigned)g < (unsigned)d.max_gt) {  // (else: no loss, no gradient, still in the divisor)
            const float *gp = d.gt_planes + ((size_t)img * d.max_gt + g) * 3;
            float t[3] = {gp[0], gp[1], gp[2]}, v[3] = {raw[0], raw[1], raw[2]}, n = 0.f, dn = 1.f, gs[3];
            if (d.normal_only) {
                n = sqrtf((raw[0] * raw[0] + raw[1] * raw[1]) + raw[2] * raw[2]);
                dn = fmaxf(n, PL_EPS);
                const float gdn = fmaxf(sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]), PL_EPS);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    v[j] = raw[j] / dn;
                    t[j] = t[j] / gdn;
                }
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float e = v[j] - t[j];
                ls += fabsf(e);
                gs[j] = k * pl_sign(e);
            }
            if (d.normal_only)
                a3d_norm_bwd<3>(raw, n, dn, PL_EPS, gs, dr);
            else {
#pragma unroll
                for (int j = 0; j < 3; ++j) dr[j] = gs[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) db[j] += dr[j];
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            f32x4 gh;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int j = 0; j < 3; ++j) dw[j][q][c] = __builtin_fmaf(dr[j], h[q][c], dw[j][q][c]);
                const float s = __builtin_fmaf(w[2][q][c], dr[2], __builtin_fmaf(w[1][q][c], dr[1], w[0][q][c] * dr[0]));
                gh[c] = h[q][c] > 0.f ? s : 0.f;  // the FC's ReLU gate: closed at 0
            }
            a3d_st4(d.dh + at + q * 256, gh);
        }
    }
    float *part = d.workspace + (size_t)gw * (3 * K + 4);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int q = 0; q < NV; ++q) a3d_st4(part + (size_t)j * K + q * 256 + lane * 4, dw[j][q]);
    }
    if (lane == 0) a3d_st4(part + 3 * K, f32x4{db[0], db[1], db[2], ls});
}

// The partials of the waves that had a row, 16 columns per workgroup: 16 strands sum every 16th partial in order, then a fixed tree.
__global__ __launch_bounds__(PL_THREADS) void plane_loss_reduce_kernel(const a3d_plane_loss_desc d) {
    __shared__ float red[PL_THREADS];
    const int C = 3 * d.K + 4;
    const int live = a3d_live_rows(d.live, d.rows);
    const int parts = live < PL_PARTS ? live : PL_PARTS;
    const int t = threadIdx.x, c = blockIdx.x * PL_RED_COLS + (t % PL_RED_COLS), j = t / PL_RED_COLS;
    float s = 0.f;
    if (c < C)
        for (int p = j; p < parts; p += PL_RED_STRANDS) s += d.workspace[(size_t)p * C + c];
    red[t] = s;
    __syncthreads();
    // (a3d_lds_tree<PL_THREADS, PL_RED_COLS> written out: through the helper this kernel's exec-mask arithmetic compiles differently)
    for (int w = PL_THREADS / 2; w >= PL_RED_COLS; w >>= 1) {  // (t and t + w hold the same column: w is a multiple of 16)
        if (t < w) red[t] = red[t] + red[t + w];
        __syncthreads();
    }
    if (t < PL_RED_COLS && c < C) {
        float v = red[t];
        if (c == C - 1) v = live > 0 ? d.loss_weight * v / (float)live : 0.f;  // the sum's divisor: the device live count
        d.out[c] = v;
    }
}
}  // namespace

extern "C" size_t a3d_plane_loss_workspace_bytes(int K) {
    if (K <= 0 || K % 256 != 0) return 0;
    return (size_t)PL_PARTS * (3 * (size_t)K + 4) * sizeof(float);
}

extern "C" int a3d_plane_loss(const a3d_plane_loss_desc *d, void *stream) {
    if (!d || !d->h || !d->w || !d->b || !d->live || !d->row_img || !d->row_gt || !d->gt_planes || !d->workspace || !d->out || !d->dh)
        return A3D_ERR_ARG;
    if (d->K <= 0 || d->K % 256 != 0 || d->rows < 0 || d->B <= 0 || d->max_gt <= 0) return A3D_ERR_ARG;
    if (((uintptr_t)d->h | (uintptr_t)d->dh | (uintptr_t)d->w | (uintptr_t)d->workspace) & 15) return A3D_ERR_ARG;
    const int nv = d->K / 256;
    if (nv > PL_MAX_NV) return A3D_ERR_UNSUPPORTED;
    const hipStream_t s = (hipStream_t)stream;
    a3d_begin();
    switch (nv) {
        case 1: hipLaunchKernelGGL(plane_loss_kernel<1>, dim3(PL_WGS), dim3(PL_THREADS), 0, s, *d); break;
        case 2: hipLaunchKernelGGL(plane_loss_kernel<2>, dim3(PL_WGS), dim3(PL_THREADS), 0, s, *d); break;
        case 3: hipLaunchKernelGGL(plane_loss_kernel<3>, dim3(PL_WGS), dim3(PL_THREADS), 0, s, *d); break;
        default: hipLaunchKernelGGL(plane_loss_kernel<4>, dim3(PL_WGS), dim3(PL_THREADS), 0, s, *d); break;
    }
    hipLaunchKernelGGL(plane_loss_reduce_kernel, dim3((3 * d->K + 4 + PL_RED_COLS - 1) / PL_RED_COLS), dim3(PL_THREADS), 0, s, *d);
    return a3d_check_launch();
}
