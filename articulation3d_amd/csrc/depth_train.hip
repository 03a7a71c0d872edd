// The depth head's training step (the depth share of config/step3_plane.yaml): the launches no other stage has.
//
// Replaces, under autograd, what pkg/modeling/depth_net/depth_head.py runs in training mode besides its convolutions: the ten
// nn.BatchNorm2d(eps 1e-3, momentum 0.01) layers with BATCH statistics and their activations (:32-46), depth_pred's backward pass (:68),
// the nearest x2 upsampling + channel concat as a dense tensor (the weight gradient's input), the one bilinear resize's backward pass
// (:82) and the loss: F.interpolate(x2, bilinear) + l1LossMask(pred, gt, gt > 1e-4) (:88-89).
//
// All of these are HBM-bound passes over NHWC fp32 rows of C = 64 or 128 floats: a group of C / 4 lanes reads a row as 16-byte vectors
// and keeps its four channels' sums in registers.  No atomics anywhere: every sum leaves its workgroup as a partial and a later launch
// folds the partials in index order, so every call gives the same bits.  Built with -ffp-contract=off: the bilinear weights and the L1
// tail round like the reference's separate operators.
#include "kernel_prims.h"
#include "../../include/a3d.h"

namespace {
constexpr int DT_THREADS = 256;
constexpr int DT_MAX_PARTS = 1024;  // workgroups (= partials) of a reduction launch at most: four per CU
constexpr int DT_MIN_ROWS = 32;     // rows per workgroup at least
constexpr float DT_LEAKY = 0.01f;   // nn.LeakyReLU's default slope (depth_head.py:36)
constexpr float DT_VALID = 1e-4f;   // l1LossMask: gt > 1e-4
constexpr int DL_MAX_PARTS = 256;   // a3d_depth_loss: workgroups of the gather launch
constexpr int PB_MAX_PARTS = 512;   // a3d_depth_pred_backward
constexpr int PB_C = 64;

__host__ __device__ inline int dt_rows_per_part(int N) {
    const int r = (N + DT_MAX_PARTS - 1) / DT_MAX_PARTS;
    return r < DT_MIN_ROWS ? DT_MIN_ROWS : r;
}

// Sum over the strands of a workgroup: strand s holds acc for channels sub * 4 .. + 3 -> red[s][C]; threads t < C then add the strands
// in order.  (red is reused by the caller: barriers on both sides)
template <int C>
__device__ __forceinline__ float dt_fold_strands(float (*red)[C], const f32x4 acc, int s, int sub) {
    constexpr int S = DT_THREADS / (C / 4);
    __syncthreads();
    a3d_st4(&red[s][sub * 4], acc);
    __syncthreads();
    float a = 0.f;
    if ((int)threadIdx.x < C) {
#pragma unroll
        for (int j = 0; j < S; ++j) a += red[j][threadIdx.x];
    }
    return a;
}

// ---- batch statistics: per workgroup (mean, M2 about that mean) over its rows --------------------------------------------------------
template <int C>
__global__ __launch_bounds__(DT_THREADS) void bn_stats_kernel(const a3d_bn_train_desc d, int R) {
    constexpr int LPR = C / 4, S = DT_THREADS / LPR;
    __shared__ __attribute__((aligned(16))) float red[S][C];
    __shared__ __attribute__((aligned(16))) float mu[C];
    const int sub = threadIdx.x % LPR, s = threadIdx.x / LPR;
    const int r0 = blockIdx.x * R, r1 = min(d.N, r0 + R), n = r1 - r0;
    const float *z = d.z + (size_t)sub * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int r = r0 + s;
    for (; r + 3 * S < r1; r += 4 * S) {  // four independent 16-byte loads in flight per lane
        const f32x4 a = a3d_ld4(z + (size_t)r * C), b = a3d_ld4(z + (size_t)(r + S) * C), c = a3d_ld4(z + (size_t)(r + 2 * S) * C), e = a3d_ld4(z + (size_t)(r + 3 * S) * C);
        acc += (a + b) + (c + e);
    }
    for (; r < r1; r += S) acc += a3d_ld4(z + (size_t)r * C);
    const float sum = dt_fold_strands<C>(red, acc, s, sub);
    if ((int)threadIdx.x < C) mu[threadIdx.x] = sum / (float)n;
    __syncthreads();
    const f32x4 m = a3d_ld4(&mu[sub * 4]);
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
    r = r0 + s;
    for (; r + 3 * S < r1; r += 4 * S) {  // (the workgroup's own rows again: served from L2)
        const f32x4 a = a3d_ld4(z + (size_t)r * C) - m, b = a3d_ld4(z + (size_t)(r + S) * C) - m, c = a3d_ld4(z + (size_t)(r + 2 * S) * C) - m,
                    e = a3d_ld4(z + (size_t)(r + 3 * S) * C) - m;
        acc += (a * a + b * b) + (c * c + e * e);
    }
    for (; r < r1; r += S) {
        const f32x4 a = a3d_ld4(z + (size_t)r * C) - m;
        acc += a * a;
    }
    const float m2 = dt_fold_strands<C>(red, acc, s, sub);
    if ((int)threadIdx.x < C) {
        float *part = d.workspace + (size_t)blockIdx.x * 2 * C;
        part[threadIdx.x] = mu[threadIdx.x];
        part[C + threadIdx.x] = m2;
    }
}

// The partials folded by one workgroup (double): 1024 / C strands per channel add every (1024 / C)-th partial in index order, the strands
// are added in order.  mean = sum n_g mean_g / N, then M2 = sum (M2_g + n_g (mean_g - mean)^2).
constexpr int DT_MERGE_THREADS = 1024;

__device__ __forceinline__ double dt_fold_merge(double *red, double v, int c, int C) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    double a = 0.0;
    if ((int)threadIdx.x < C)
        for (int k = 0; k < DT_MERGE_THREADS / C; ++k) a += red[k * C + c];
    return a;
}

__global__ __launch_bounds__(DT_MERGE_THREADS) void bn_merge_kernel(const a3d_bn_train_desc d, int R, int parts) {
    __shared__ double red[DT_MERGE_THREADS];
    __shared__ double mean_s[128];
    const int C = d.C, c = threadIdx.x % C, j = threadIdx.x / C, J = DT_MERGE_THREADS / C;
    double sm = 0.0;
    for (int g = j; g < parts; g += J) {
        const int n = min(d.N, (g + 1) * R) - g * R;
        sm += (double)n * (double)d.workspace[(size_t)g * 2 * C + c];
    }
    sm = dt_fold_merge(red, sm, c, C);
    if ((int)threadIdx.x < C) mean_s[c] = sm / (double)d.N;
    __syncthreads();
    const double mean = mean_s[c];
    double m2 = 0.0;
    for (int g = j; g < parts; g += J) {
        const int n = min(d.N, (g + 1) * R) - g * R;
        const double dm = (double)d.workspace[(size_t)g * 2 * C + c] - mean;
        m2 += (double)d.workspace[(size_t)g * 2 * C + C + c] + (double)n * dm * dm;
    }
    m2 = dt_fold_merge(red, m2, c, C);
    if ((int)threadIdx.x >= C) return;
    const double var = m2 / (double)d.N;
    d.mean[c] = (float)mean;
    d.invstd[c] = (float)(1.0 / sqrt(var + (double)d.eps));
    if (d.var) d.var[c] = (float)var;
    if (d.running_mean) {  // F.batch_norm(training=True): the running variance takes the UNBIASED estimate
        const float mo = d.momentum, unb = (float)(m2 / (double)(d.N - 1));
        d.running_mean[c] = (1.f - mo) * d.running_mean[c] + mo * (float)mean;
        d.running_var[c] = (1.f - mo) * d.running_var[c] + mo * unb;
    }
}

__device__ __forceinline__ float dt_act(float v, int act) { return v > 0.f ? v : (act == A3D_ACT_LEAKY ? DT_LEAKY * v : 0.f); }
__device__ __forceinline__ float dt_act_grad(float y, int act) { return y > 0.f ? 1.f : (act == A3D_ACT_LEAKY ? DT_LEAKY : 0.f); }

template <int C>
__global__ __launch_bounds__(DT_THREADS) void bn_apply_kernel(const a3d_bn_train_desc d) {
    constexpr int LPR = C / 4;
    const int sub = threadIdx.x % LPR;  // (the grid stride is a multiple of LPR: a thread keeps its channels)
    const f32x4 m = a3d_ld4(d.mean + sub * 4), is = a3d_ld4(d.invstd + sub * 4), ga = a3d_ld4(d.gamma + sub * 4), be = a3d_ld4(d.beta + sub * 4);
    const f32x4 sc = ga * is;
    const size_t total = (size_t)d.N * LPR;
    for (size_t i = (size_t)blockIdx.x * DT_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * DT_THREADS) {
        const f32x4 v = (a3d_ld4(d.z + i * 4) - m) * sc + be;
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = dt_act(v[k], d.act);
        a3d_st4(d.y + i * 4, o);
    }
}

// ---- backward: per workgroup sum g and sum g xh over its rows ------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(DT_THREADS) void bn_bwd_reduce_kernel(const a3d_bn_train_desc d, int R) {
    constexpr int LPR = C / 4, S = DT_THREADS / LPR;
    __shared__ __attribute__((aligned(16))) float red[S][C];
    const int sub = threadIdx.x % LPR, s = threadIdx.x / LPR;
    const int r0 = blockIdx.x * R, r1 = min(d.N, r0 + R);
    const f32x4 m = a3d_ld4(d.mean + sub * 4), is = a3d_ld4(d.invstd + sub * 4);
    f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int r = r0 + s; r < r1; r += S) {
        const size_t at = (size_t)r * C + sub * 4;
        const f32x4 dy = a3d_ld4(d.dy + (size_t)r * d.dy_pitch + d.dy_off + sub * 4), y = a3d_ld4(d.y + at), z = a3d_ld4(d.z + at);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float g = dy[k] * dt_act_grad(y[k], d.act);
            sg[k] += g;
            sx[k] += g * ((z[k] - m[k]) * is[k]);
        }
    }
    const float a = dt_fold_strands<C>(red, sg, s, sub);
    const float b = dt_fold_strands<C>(red, sx, s, sub);
    if ((int)threadIdx.x < C) {
        float *part = d.workspace + (size_t)blockIdx.x * 2 * C;
        part[threadIdx.x] = a;
        part[C + threadIdx.x] = b;
    }
}

__global__ __launch_bounds__(DT_MERGE_THREADS) void bn_bwd_merge_kernel(const a3d_bn_train_desc d, int parts) {
    __shared__ double red[DT_MERGE_THREADS];
    const int C = d.C, c = threadIdx.x % C, j = threadIdx.x / C, J = DT_MERGE_THREADS / C;
    double a = 0.0, b = 0.0;
    for (int g = j; g < parts; g += J) {
        a += (double)d.workspace[(size_t)g * 2 * C + c];
        b += (double)d.workspace[(size_t)g * 2 * C + C + c];
    }
    a = dt_fold_merge(red, a, c, C);
    b = dt_fold_merge(red, b, c, C);
    if ((int)threadIdx.x < C) {
        d.dbeta[c] = (float)a;
        d.dgamma[c] = (float)b;
    }
}

template <int C>
__global__ __launch_bounds__(DT_THREADS) void bn_bwd_apply_kernel(const a3d_bn_train_desc d) {
    constexpr int LPR = C / 4;
    const int sub = threadIdx.x % LPR;
    const f32x4 m = a3d_ld4(d.mean + sub * 4), is = a3d_ld4(d.invstd + sub * 4), ga = a3d_ld4(d.gamma + sub * 4);
    const float inv_n = 1.f / (float)d.N;
    const f32x4 mg = a3d_ld4(d.dbeta + sub * 4) * inv_n, mx = a3d_ld4(d.dgamma + sub * 4) * inv_n, sc = ga * is;
    const size_t total = (size_t)d.N * LPR;
    for (size_t i = (size_t)blockIdx.x * DT_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * DT_THREADS) {
        const size_t r = i / LPR;
        const f32x4 dy = a3d_ld4(d.dy + r * d.dy_pitch + d.dy_off + sub * 4), y = a3d_ld4(d.y + i * 4), z = a3d_ld4(d.z + i * 4);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float g = dy[k] * dt_act_grad(y[k], d.act);
            o[k] = sc[k] * ((g - mg[k]) - ((z[k] - m[k]) * is[k]) * mx[k]);
        }
        a3d_st4(d.dz + i * 4, o);
    }
}

int bn_check(const a3d_bn_train_desc *d, bool backward) {
    if (!d || !d->z || !d->gamma || !d->y || !d->mean || !d->invstd || !d->workspace) return A3D_ERR_ARG;
    if ((d->C != 64 && d->C != 128) || d->N < 2) return A3D_ERR_ARG;
    if (d->act != A3D_ACT_RELU && d->act != A3D_ACT_LEAKY) return A3D_ERR_ARG;
    if (((uintptr_t)d->z | (uintptr_t)d->y | (uintptr_t)d->workspace | (uintptr_t)d->gamma | (uintptr_t)d->mean | (uintptr_t)d->invstd) & 15) return A3D_ERR_ARG;
    if (!backward) {
        if (!d->beta || ((uintptr_t)d->beta & 15) || !(d->eps > 0.f) || (!d->running_mean) != (!d->running_var)) return A3D_ERR_ARG;
    } else {
        if (!d->dy || !d->dz || !d->dgamma || !d->dbeta) return A3D_ERR_ARG;
        if (d->dy_pitch < d->C || (d->dy_pitch & 3) || d->dy_off < 0 || (d->dy_off & 3) || d->dy_off + d->C > d->dy_pitch) return A3D_ERR_ARG;
        if (((uintptr_t)d->dy | (uintptr_t)d->dz | (uintptr_t)d->dgamma | (uintptr_t)d->dbeta) & 15) return A3D_ERR_ARG;
    }
    return A3D_OK;
}

// ---- the loss ---------------------------------------------------------------------------------------------------------------------------
// One thread per low-resolution pixel (grid-stride): it visits the up to 4 x 4 output pixels whose bilinear footprint holds it, forms
// each one's prediction with the resize kernel's arithmetic and collects sign(pred - gt) x its own weight there; the 2 x 2 outputs it
// owns (oy >> 1 == y, ox >> 1 == x) also go into its loss sum and its count, so every output pixel is counted once.
__global__ __launch_bounds__(DT_THREADS) void depth_loss_gather_kernel(const a3d_depth_loss_desc d) {
    __shared__ float red[DT_THREADS];
    __shared__ int redn[DT_THREADS];
    const int h = d.h, w = d.w, H = 2 * h, W = 2 * w;
    const size_t total = (size_t)d.B * h * w;
    float ls = 0.f;
    int cnt = 0;
    for (size_t i = (size_t)blockIdx.x * DT_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * DT_THREADS) {
        const int x = (int)(i % w), y = (int)((i / w) % h);
        const size_t b = i / ((size_t)w * h);
        const float *src = d.d + b * h * w, *gt = d.gt + b * H * W;
        float grad = 0.f;
        for (int oy = max(2 * y - 1, 0); oy <= min(2 * y + 2, H - 1); ++oy) {
            int y0, y1;
            float ly;
            a3d_src_index(oy, 0.5f, h, y0, y1, ly);
            const float hy = 1.f - ly;
            const float wy = (y0 == y ? hy : 0.f) + (y1 == y ? ly : 0.f);
            for (int ox = max(2 * x - 1, 0); ox <= min(2 * x + 2, W - 1); ++ox) {
                const float t = gt[(size_t)oy * W + ox];
                if (!(t > DT_VALID)) continue;
                int x0, x1;
                float lx;
                a3d_src_index(ox, 0.5f, w, x0, x1, lx);
                const float hx = 1.f - lx;
                const float wx = (x0 == x ? hx : 0.f) + (x1 == x ? lx : 0.f);
                const float p = hy * (hx * src[(size_t)y0 * w + x0] + lx * src[(size_t)y0 * w + x1]) +
                                ly * (hx * src[(size_t)y1 * w + x0] + lx * src[(size_t)y1 * w + x1]);
                const float e = p - t;
                grad += (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)) * (wy * wx);  // (torch.sign: 0 at a tie)
                if ((oy >> 1) == y && (ox >> 1) == x) {
                    ls += fabsf(e);
                    ++cnt;
                }
            }
        }
        d.dd[i] = grad;
    }
    red[threadIdx.x] = ls;
    redn[threadIdx.x] = cnt;
    __syncthreads();
    a3d_lds_tree<DT_THREADS>(red, redn);
    if (threadIdx.x == 0) {
        d.workspace[2 * blockIdx.x] = red[0];
        reinterpret_cast<int *>(d.workspace)[2 * blockIdx.x + 1] = redn[0];
    }
}

// Every workgroup folds the partials by the same fixed tree (at most 256 pairs) and scales its share of the gradient by
// loss_weight / max(count, 1); workgroup 0 writes the loss and the count.
__global__ __launch_bounds__(DT_THREADS) void depth_loss_scale_kernel(const a3d_depth_loss_desc d, int parts) {
    __shared__ double red[DT_THREADS];
    __shared__ long long redn[DT_THREADS];
    const int t = threadIdx.x;
    red[t] = t < parts ? (double)d.workspace[2 * t] : 0.0;  // (parts <= DT_THREADS)
    redn[t] = t < parts ? (long long)reinterpret_cast<const int *>(d.workspace)[2 * t + 1] : 0;
    __syncthreads();
    a3d_lds_tree<DT_THREADS>(red, redn);
    const long long n = redn[0] > 0 ? redn[0] : 1;
    if (blockIdx.x == 0 && t == 0) {
        d.out[0] = (float)((double)d.loss_weight * red[0] / (double)n);
        d.out[1] = (float)redn[0];
    }
    const float k = d.loss_weight / (float)n;
    const size_t total = (size_t)d.B * d.h * d.w;
    for (size_t i = (size_t)blockIdx.x * DT_THREADS + t; i < total; i += (size_t)gridDim.x * DT_THREADS) d.dd[i] *= k;
}

// ---- depth_pred's backward pass -------------------------------------------------------------------------------------------------------------
// 16 lanes per pixel (four channels each), 16 pixels per workgroup step.  For the pixel q the lane reads x[q] once and the nine gradients
// around q:  dx[q] = sum_t g[q - off_t] w[t]  and  dw[t] += x[q] g[q - off_t]  (y[p] = sum_t x[p + off_t] w[t], off_t = (ky - 1, kx - 1)).
__global__ __launch_bounds__(DT_THREADS) void pred_bwd_kernel(const a3d_pred_bwd_desc d) {
    constexpr int C = PB_C, LPR = C / 4, S = DT_THREADS / LPR;
    __shared__ __attribute__((aligned(16))) float red[S][C];
    const int sub = threadIdx.x % LPR, s = threadIdx.x / LPR;
    const int H = d.H, W = d.W;
    const size_t total = (size_t)d.B * H * W;
    f32x4 wt[9], dw[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        wt[t] = a3d_ld4(d.w + t * C + sub * 4);
        dw[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float db = 0.f;
    for (size_t q = (size_t)blockIdx.x * S + s; q < total; q += (size_t)gridDim.x * S) {
        const int x = (int)(q % W), y = (int)((q / W) % H);
        const float *gb = d.g + (q - (size_t)y * W - x);  // the image's gradient map
        const f32x4 v = a3d_ld4(d.x + q * C + sub * 4);
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int py = y - (ky - 1), px = x - (kx - 1);
                const float g = ((unsigned)py < (unsigned)H && (unsigned)px < (unsigned)W) ? gb[(size_t)py * W + px] : 0.f;
                o += wt[ky * 3 + kx] * g;
                dw[ky * 3 + kx] += v * g;
            }
        }
        a3d_st4(d.dx + q * C + sub * 4, o);
        db += gb[(size_t)y * W + x];
    }
    float *part = d.workspace + (size_t)blockIdx.x * (9 * C + 4);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const float a = dt_fold_strands<C>(red, dw[t], s, sub);
        if ((int)threadIdx.x < C) part[t * C + threadIdx.x] = a;
    }
    const float b = dt_fold_strands<C>(red, f32x4{db, 0.f, 0.f, 0.f}, s, sub);  // (every lane of a pixel holds the same db: channel 0 of lane group 0 only)
    if (threadIdx.x == 0) part[9 * C] = b;
}

// 16 columns per workgroup: 16 strands add every 16th partial in index order, then the strands in order.
__global__ __launch_bounds__(DT_THREADS) void pred_bwd_fold_kernel(const a3d_pred_bwd_desc d, int parts) {
    __shared__ double red[DT_THREADS];
    const int t = threadIdx.x, c = blockIdx.x * 16 + (t % 16), j = t / 16;
    double a = 0.0;
    if (c <= 9 * PB_C)
        for (int g = j; g < parts; g += 16) a += (double)d.workspace[(size_t)g * (9 * PB_C + 4) + c];
    red[t] = a;
    __syncthreads();
    if (t < 16 && c <= 9 * PB_C) {
        double v = 0.0;
        for (int k = 0; k < 16; ++k) v += red[k * 16 + t];
        d.out[c] = (float)v;
    }
}

inline int pb_parts(size_t pixels) {
    const size_t b = (pixels + 63) / 64;  // 64 pixels per workgroup at least
    return (int)(b < 1 ? 1 : (b > PB_MAX_PARTS ? PB_MAX_PARTS : b));
}

// ---- nearest x2 upsampling of a channel concat, dense --------------------------------------------------------------------------------------
__global__ __launch_bounds__(DT_THREADS) void ups2_concat_kernel(const float *__restrict__ a, const float *__restrict__ b2, float *__restrict__ out,
                                                                 int B, int H, int W, int Ca, int Cb) {
    const int CV = (Ca + Cb) / 4, Wo = 2 * W, Ho = 2 * H;
    const size_t total = (size_t)B * Ho * Wo * CV;
    for (size_t i = (size_t)blockIdx.x * DT_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * DT_THREADS) {
        const int c = (int)(i % CV) * 4;
        size_t p = i / CV;
        const int ox = (int)(p % Wo);
        p /= Wo;
        const int oy = (int)(p % Ho);
        const size_t b = p / Ho;
        const size_t src = (b * H + (oy >> 1)) * W + (ox >> 1);
        a3d_st4(out + i * 4, c < Ca ? a3d_ld4(a + src * Ca + c) : a3d_ld4(b2 + src * Cb + (c - Ca)));
    }
}

// ---- the bilinear resize's backward pass: a gather per input pixel, outputs visited in order ------------------------------------------------
__global__ __launch_bounds__(DT_THREADS) void resize_bilinear_bwd_kernel(const float *__restrict__ dy, float *__restrict__ dx, int B, int H, int W,
                                                                         int C, int Ho, int Wo, float sh, float sw) {
    const int CV = C / 4;
    const size_t total = (size_t)B * H * W * CV;
    for (size_t i = (size_t)blockIdx.x * DT_THREADS + threadIdx.x; i < total; i += (size_t)gridDim.x * DT_THREADS) {
        const int c = (int)(i % CV) * 4;
        size_t p = i / CV;
        const int ix = (int)(p % W);
        p /= W;
        const int iy = (int)(p % H);
        const size_t b = p / H;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int oy = 0; oy < Ho; ++oy) {
            int y0, y1;
            float ly;
            a3d_src_index(oy, sh, H, y0, y1, ly);
            const float wy = (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
            if (y0 != iy && y1 != iy) continue;
            for (int ox = 0; ox < Wo; ++ox) {
                int x0, x1;
                float lx;
                a3d_src_index(ox, sw, W, x0, x1, lx);
                if (x0 != ix && x1 != ix) continue;
                const float wx = (x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f);
                acc += a3d_ld4(dy + ((b * Ho + oy) * Wo + ox) * C + c) * (wy * wx);
            }
        }
        a3d_st4(dx + i * 4, acc);
    }
}
}  // namespace

extern "C" size_t a3d_bn_train_workspace_bytes(int N, int C) {
    if ((C != 64 && C != 128) || N < 2) return 0;
    return (size_t)DT_MAX_PARTS * 2 * C * sizeof(float);
}

extern "C" int a3d_bn_train_forward(const a3d_bn_train_desc *d, void *stream) {
    const int rc = bn_check(d, false);
    if (rc != A3D_OK) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const int R = dt_rows_per_part(d->N), parts = (d->N + R - 1) / R;
    const int grid = a3d_stream_grid((size_t)d->N * (d->C / 4));
    a3d_begin();
    if (d->C == 64) {
        hipLaunchKernelGGL(bn_stats_kernel<64>, dim3(parts), dim3(DT_THREADS), 0, s, *d, R);
        hipLaunchKernelGGL(bn_merge_kernel, dim3(1), dim3(DT_MERGE_THREADS), 0, s, *d, R, parts);
        hipLaunchKernelGGL(bn_apply_kernel<64>, dim3(grid), dim3(DT_THREADS), 0, s, *d);
    } else {
        hipLaunchKernelGGL(bn_stats_kernel<128>, dim3(parts), dim3(DT_THREADS), 0, s, *d, R);
        hipLaunchKernelGGL(bn_merge_kernel, dim3(1), dim3(DT_MERGE_THREADS), 0, s, *d, R, parts);
        hipLaunchKernelGGL(bn_apply_kernel<128>, dim3(grid), dim3(DT_THREADS), 0, s, *d);
    }
    return a3d_check_launch();
}

extern "C" int a3d_bn_train_backward(const a3d_bn_train_desc *d, void *stream) {
    const int rc = bn_check(d, true);
    if (rc != A3D_OK) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const int R = dt_rows_per_part(d->N), parts = (d->N + R - 1) / R;
    const int grid = a3d_stream_grid((size_t)d->N * (d->C / 4));
    a3d_begin();
    if (d->C == 64) {
        hipLaunchKernelGGL(bn_bwd_reduce_kernel<64>, dim3(parts), dim3(DT_THREADS), 0, s, *d, R);
        hipLaunchKernelGGL(bn_bwd_merge_kernel, dim3(1), dim3(DT_MERGE_THREADS), 0, s, *d, parts);
        hipLaunchKernelGGL(bn_bwd_apply_kernel<64>, dim3(grid), dim3(DT_THREADS), 0, s, *d);
    } else {
        hipLaunchKernelGGL(bn_bwd_reduce_kernel<128>, dim3(parts), dim3(DT_THREADS), 0, s, *d, R);
        hipLaunchKernelGGL(bn_bwd_merge_kernel, dim3(1), dim3(DT_MERGE_THREADS), 0, s, *d, parts);
        hipLaunchKernelGGL(bn_bwd_apply_kernel<128>, dim3(grid), dim3(DT_THREADS), 0, s, *d);
    }
    return a3d_check_launch();
}

extern "C" size_t a3d_depth_loss_workspace_bytes(void) { return (size_t)DL_MAX_PARTS * 2 * sizeof(float); }

extern "C" int a3d_depth_loss(const a3d_depth_loss_desc *d, void *stream) {
    if (!d || !d->d || !d->gt || !d->dd || !d->out || !d->workspace) return A3D_ERR_ARG;
    if (d->B <= 0 || d->h <= 0 || d->w <= 0 || d->h > (1 << 14) || d->w > (1 << 14)) return A3D_ERR_ARG;
    const size_t total = (size_t)d->B * d->h * d->w;
    const size_t b = (total + DT_THREADS - 1) / DT_THREADS;
    const int parts = (int)(b > DL_MAX_PARTS ? DL_MAX_PARTS : b);
    const hipStream_t s = (hipStream_t)stream;
    a3d_begin();
    hipLaunchKernelGGL(depth_loss_gather_kernel, dim3(parts), dim3(DT_THREADS), 0, s, *d);
    hipLaunchKernelGGL(depth_loss_scale_kernel, dim3(parts), dim3(DT_THREADS), 0, s, *d, parts);
    return a3d_check_launch();
}

extern "C" size_t a3d_pred_bwd_workspace_bytes(void) { return (size_t)PB_MAX_PARTS * (9 * PB_C + 4) * sizeof(float); }

extern "C" int a3d_depth_pred_backward(const a3d_pred_bwd_desc *d, void *stream) {
    if (!d || !d->x || !d->g || !d->w || !d->dx || !d->out || !d->workspace) return A3D_ERR_ARG;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->C != PB_C) return A3D_ERR_ARG;
    if (((uintptr_t)d->x | (uintptr_t)d->dx | (uintptr_t)d->w | (uintptr_t)d->workspace) & 15) return A3D_ERR_ARG;
    const int parts = pb_parts((size_t)d->B * d->H * d->W);
    const hipStream_t s = (hipStream_t)stream;
    a3d_begin();
    hipLaunchKernelGGL(pred_bwd_kernel, dim3(parts), dim3(DT_THREADS), 0, s, *d);
    hipLaunchKernelGGL(pred_bwd_fold_kernel, dim3((9 * PB_C + 1 + 15) / 16), dim3(DT_THREADS), 0, s, *d, parts);
    return a3d_check_launch();
}

extern "C" int a3d_ups2_concat(const float *a, const float *b2, float *out, int B, int H, int W, int Ca, int Cb, void *stream) {
    if (!a || !out || B <= 0 || H <= 0 || W <= 0 || Ca <= 0 || Cb < 0 || (Ca & 3) || (Cb & 3) || (Cb > 0 && !b2)) return A3D_ERR_ARG;
    if (((uintptr_t)a | (uintptr_t)b2 | (uintptr_t)out) & 15) return A3D_ERR_ARG;
    a3d_begin();
    hipLaunchKernelGGL(ups2_concat_kernel, dim3(a3d_stream_grid((size_t)B * 4 * H * W * ((Ca + Cb) / 4))), dim3(DT_THREADS), 0, (hipStream_t)stream, a, b2,
                       out, B, H, W, Ca, Cb);
    return a3d_check_launch();
}

extern "C" int a3d_resize_bilinear_backward_nhwc(const float *dy, float *dx, int B, int H, int W, int C, int Ho, int Wo, void *stream) {
    if (!dy || !dx || B <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || (C & 3)) return A3D_ERR_ARG;
    if (((uintptr_t)dy | (uintptr_t)dx) & 15) return A3D_ERR_ARG;
    const float sh = (float)H / (float)Ho, sw = (float)W / (float)Wo;
    a3d_begin();
    hipLaunchKernelGGL(resize_bilinear_bwd_kernel, dim3(a3d_stream_grid((size_t)B * H * W * (C / 4))), dim3(DT_THREADS), 0, (hipStream_t)stream, dy, dx, B, H,
                       W, C, Ho, Wo, sh, sw);
    return a3d_check_launch();
}
