// Axis loss of the articulation head's training stage (config/step2_axis.yaml), forward and backward in one launch (a3d_axis_loss).
//
// Replaces, under autograd, pkg/modeling/roi_heads/axis_head.py:104-120 (F.normalize of the rotation / translation outputs),
// :130-131 (axis_loss for both axes) and :147-201 (double_angle, smooth_l1 over the valid rows, masked mean) plus their backward.
// The rows are the compacted foreground ROIs [0, *live) of a batch; the loss is a mean over the valid rows of the WHOLE batch, so
// the launch is one workgroup: pass 1 sums counts and losses (per thread in row order, then a fixed tree), pass 2 writes the gradients
// of (loss_rot + loss_tran) with respect to the raw head outputs.  No atomics: the same bits on every run.
#include "kernel_prims.h"
#include "../../include/a3d.h"

namespace {
constexpr int AX_THREADS = 256;
constexpr float AX_EPS = 1e-12f;  // F.normalize's eps

// fvcore smooth_l1_loss: |x| below beta 1e-5, else the quadratic zone |x| < beta
__device__ __forceinline__ float ax_sl1(float x, float beta) {
    const float n = fabsf(x);
    if (beta < 1e-5f) return n;
    return n < beta ? 0.5f * n * n / beta : n - 0.5f * beta;
}
__device__ __forceinline__ float ax_sl1_grad(float x, float beta) {
    const float sg = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);  // (abs backward: 0 at 0)
    if (beta < 1e-5f) return sg;
    return fabsf(x) < beta ? x / beta : sg;
}

// one row's forward values: normalised vectors, residuals, per-axis validity and loss terms
struct AxRow {
    float a, b, n, dn, s, c, e[3];     // rotation: raw (a, b), |.|, clamped |.|, normalised (s, c), residuals (sin, cos, offset)
    float ta, tb, tn, tdn, ts, tc, f[2];  // translation: raw, |.|, clamped, normalised, double-angle residuals
    float vr, vt;                      // gt valid columns
    bool ok;                           // image / gt index in range
};

__device__ __forceinline__ AxRow ax_row(const a3d_axis_loss_desc &d, int r) {
    AxRow q;
    const int img = d.row_img[r], g = d.row_gt[r];
    q.ok = (unsigned)img < (unsigned)d.B && (unsigned)g < (unsigned)d.max_gt;
    if (!q.ok) return q;
    const float *gr = d.gt_rot_axis + ((size_t)img * d.max_gt + g) * 4;
    const float *gt = d.gt_tran_axis + ((size_t)img * d.max_gt + g) * 4;
    const float *rr = d.raw_rot + (size_t)r * d.rot_pitch;
    const float *rt = d.raw_tran + (size_t)r * d.tran_pitch;
    q.a = rr[0];
    q.b = rr[1];
    q.n = sqrtf(q.a * q.a + q.b * q.b);
    q.dn = fmaxf(q.n, AX_EPS);
    q.s = q.a / q.dn;
    q.c = q.b / q.dn;
    q.e[0] = q.s - gr[0];
    q.e[1] = q.c - gr[1];
    q.e[2] = rr[2] - gr[2];
    q.vr = gr[3];
    q.ta = rt[0];
    q.tb = rt[1];
    q.tn = sqrtf(q.ta * q.ta + q.tb * q.tb);
    q.tdn = fmaxf(q.tn, AX_EPS);
    q.ts = q.ta / q.tdn;
    q.tc = q.tb / q.tdn;
    const float g0 = gt[0], g1 = gt[1];
    q.f[0] = 2.f * q.ts * q.tc - 2.f * g0 * g1;
    q.f[1] = (q.tc * q.tc - q.ts * q.ts) - (g1 * g1 - g0 * g0);
    q.vt = gt[3];
    return q;
}

// the block's sum of v in every thread; `red` is free again on return
template <typename T>
__device__ __forceinline__ T ax_reduce(T v, T *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    a3d_lds_tree<AX_THREADS>(red);
    const T s = red[0];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(AX_THREADS) void axis_loss_kernel(const a3d_axis_loss_desc d) {
    __shared__ float redf[AX_THREADS];
    __shared__ int redi[AX_THREADS];
    const int live = a3d_live_rows(d.live, d.rows);
    // ---- pass 1: valid counts, valid-column sums and loss sums of both axes
    float vsr = 0.f, vst = 0.f, lr = 0.f, lt = 0.f;
    int cr = 0, ct = 0;
    for (int r = threadIdx.x; r < live; r += AX_THREADS) {
        const AxRow q = ax_row(d, r);
        if (!q.ok) continue;
        vsr += q.vr;
        vst += q.vt;
        if (q.vr >= 0.5f) {
            ++cr;
            lr += (ax_sl1(q.e[0], d.beta) + ax_sl1(q.e[1], d.beta)) + ax_sl1(q.e[2], d.beta);
        }
        if (q.vt >= 0.5f) {
            ++ct;
            lt += ax_sl1(q.f[0], d.beta) + ax_sl1(q.f[1], d.beta);
        }
    }
    vsr = ax_reduce(vsr, redf);
    vst = ax_reduce(vst, redf);
    lr = ax_reduce(lr, redf);
    lt = ax_reduce(lt, redf);
    cr = ax_reduce(cr, redi);
    ct = ax_reduce(ct, redi);
    // (the reference returns 0 * pred.sum() when the valid column sums below 1 -- no ground truth at all included; a sum >= 1 made of
    // values under 0.5 would be the mean of nothing there, NaN: 0 here)
    const bool onr = vsr >= 1.f && cr > 0, ont = vst >= 1.f && ct > 0;
    const float kr = onr ? d.loss_weight / (float)(3 * cr) : 0.f, kt = ont ? d.loss_weight / (float)(2 * ct) : 0.f;
    if (threadIdx.x == 0) {
        d.loss[0] = onr ? d.loss_weight * (lr / (float)(3 * cr)) : 0.f;
        d.loss[1] = ont ? d.loss_weight * (lt / (float)(2 * ct)) : 0.f;
    }
    // ---- pass 2: gradients of the raw rows (dead rows and padding columns: zeros)
    for (int r = threadIdx.x; r < d.rows; r += AX_THREADS) {
        float gr[3] = {0.f, 0.f, 0.f}, gt[2] = {0.f, 0.f};
        if (r < live) {
            const AxRow q = ax_row(d, r);
            if (q.ok && onr && q.vr >= 0.5f) {
                const float gn[2] = {kr * ax_sl1_grad(q.e[0], d.beta), kr * ax_sl1_grad(q.e[1], d.beta)}, v[2] = {q.a, q.b};
                a3d_norm_bwd<2>(v, q.n, q.dn, AX_EPS, gn, gr);
                gr[2] = kr * ax_sl1_grad(q.e[2], d.beta);
            }
            if (q.ok && ont && q.vt >= 0.5f) {
                const float g0 = kt * ax_sl1_grad(q.f[0], d.beta), g1 = kt * ax_sl1_grad(q.f[1], d.beta);
                // double_angle backward: d(2sc)/ds = 2c, d(2sc)/dc = 2s, d(c^2 - s^2)/ds = -2s, d(c^2 - s^2)/dc = 2c
                const float gn[2] = {g0 * (2.f * q.tc) - g1 * (2.f * q.ts), g0 * (2.f * q.ts) + g1 * (2.f * q.tc)}, v[2] = {q.ta, q.tb};
                a3d_norm_bwd<2>(v, q.tn, q.tdn, AX_EPS, gn, gt);
            }
        }
        float *dr = d.d_rot + (size_t)r * d.rot_pitch;
        for (int k = 0; k < d.rot_pitch; ++k) dr[k] = k < 3 ? gr[k] : 0.f;
        float *dt = d.d_tran + (size_t)r * d.tran_pitch;
        for (int k = 0; k < d.tran_pitch; ++k) dt[k] = k < 2 ? gt[k] : 0.f;
    }
}
}  // namespace

extern "C" int a3d_axis_loss(const a3d_axis_loss_desc *d, void *stream) {
    if (!d || !d->raw_rot || !d->raw_tran || !d->live || !d->row_img || !d->row_gt || !d->gt_rot_axis || !d->gt_tran_axis || !d->loss ||
        !d->d_rot || !d->d_tran)
        return A3D_ERR_ARG;
    if (d->rows < 0 || d->B <= 0 || d->max_gt <= 0 || d->rot_pitch < 3 || d->tran_pitch < 2 || !(d->beta >= 0.f)) return A3D_ERR_ARG;
    a3d_begin();
    hipLaunchKernelGGL(axis_loss_kernel, dim3(1), dim3(AX_THREADS), 0, (hipStream_t)stream, *d);
    return a3d_check_launch();
}
