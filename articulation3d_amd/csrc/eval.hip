// Evaluation of a checkpoint on the device: the reference's articulation AP (ArtiEvaluator -> evaluate_for_arti_axis,
// pkg/evaluation/arti_evaluation.py:262-665 over pkg/utils/metrics.py and pkg/utils/VOCap.py) and its depth_l1_dist
// (pkg/evaluation/scannet_evaluation.py:241-248).  The reference walks detections and ground truths in Python loops on the host; here
// one launch matches every detection of every image processed so far, one launch turns the sorted true-positive bits into the AP
// table, one launch sums the depth error of a batch.  The law of each is stated in include/a3d.h and, in numpy float64, by
// tests/eval_ref.py.
//
// All three are latency-bound (a few hundred kB in, a few kB out) and do their arithmetic in float64, which on gfx950 runs at a
// fraction of the fp32 rate: neither matters at these sizes, so the launch shapes are the plain ones -- one wave per image, one
// workgroup per (class, metric), one workgroup per depth map.  No atomics on floats and no reduction whose order depends on timing:
// the only atomic is an integer minimum in LDS, so every call gives the same bits.  Built with -ffp-contract=off: every operator
// rounds on its own, as numpy's do.
#include "kernel_prims.h"
#include "eval_common.h"  // the box IoU, a detection's ground truth and rank: shared with csrc/plane_eval.hip

#include <limits.h>

namespace {
constexpr int EV_DET = A3D_EVAL_DET_COLS, EV_GF = A3D_EVAL_GT_FCOLS, EV_GI = A3D_EVAL_GT_ICOLS, EV_MAX_GT = A3D_EVAL_MAX_GT;
constexpr double EV_PI = 3.141592653589793;  // numpy's np.pi
constexpr int AP_THREADS = 1024;  // entries per pass: a pass costs three barriers whatever its width (2 x 177 000 entries: 848 us at 256, 450 us at 1024)
constexpr int DL1_THREADS = 1024;

struct EvLine {
    double x1, y1, x2, y2;
};

// (sin, cos, offset / 100) about the box centre -> the line's two points on the image border (a3d.h: "line")
__device__ EvLine ev_pred_line(const float *box, float s, float c, float off, int H, int W) {
    const float cx = (box[0] + box[2]) / 2.0f, cy = (box[1] + box[3]) / 2.0f;
    const float p = off * 100.0f;
    const float xf = (p * c) + cx, yf = (p * s) + cy;
    const double x = xf, y = yf;
    if (s == 0.0f) return EvLine{trunc(x), 0.0, trunc(x), (double)(H - 1)};
    const double k = -((double)c / (double)s);
    if (k == 0.0) return EvLine{0.0, trunc(y), (double)(W - 1), trunc(y)};
    double px[4], py[4];
    int n = 0;
    double v = y - k * x;
    if (v >= 0.0 && v < (double)H) {
        px[n] = 0.0;
        py[n++] = trunc(v);
    }
    v = (k * (double)(W - 1) + y) - k * x;
    if (v >= 0.0 && v < (double)H) {
        px[n] = (double)(W - 1);
        py[n++] = trunc(v);
    }
    v = x - y / k;
    if (v >= 0.0 && v < (double)W) {
        px[n] = trunc(v);
        py[n++] = 0.0;
    }
    v = (x - y / k) + (double)(H - 1) / k;
    if (v >= 0.0 && v < (double)W) {
        px[n] = trunc(v);
        py[n++] = (double)(H - 1);
    }
    if (n == 0) return EvLine{0.0, 0.0, 1.0, 1.0};
    int second = 0;
    for (int i = n - 1; i >= 1; --i)
        if (px[i] != px[0] || py[i] != py[0]) second = i;  // the FIRST later candidate that differs
    return EvLine{px[0], py[0], px[second], py[second]};
}

__device__ __forceinline__ double ev_angle(const EvLine &l) { return l.x1 == l.x2 ? -EV_PI / 2 : atan((l.y1 - l.y2) / (l.x1 - l.x2)); }

__device__ double ev_ea(const EvLine &p, const EvLine &g, double size) {
    if ((p.x1 == p.x2 && p.y1 == p.y2) || (g.x1 == g.x2 && g.y1 == g.y2)) return 0.0;
    double d = fabs(ev_angle(p) - ev_angle(g));
    const double w = EV_PI - d;
    d = d < w ? d : w;
    d = d * 2 / EV_PI;
    double sa = 1 - d;
    sa = sa > 0.0 ? sa : 0.0;
    sa = sa * sa;
    const double dy = fabs((p.y1 + p.y2) / 2 - (g.y1 + g.y2) / 2), dx = fabs((p.x1 + p.x2) / 2 - (g.x1 + g.x2) / 2);
    const double dc = sqrt(dy * dy + dx * dx) / size;
    double se = 1 - dc;
    se = se > 0.0 ? se : 0.0;
    se = se * se;
    return sa * se;
}

__device__ double ev_normal_err(const float *plane, const float *gn) {
    const double p0 = plane[0], p1 = plane[1], p2 = plane[2], g0 = gn[0], g1 = gn[1], g2 = gn[2];
    const double len = sqrt((p0 * p0 + p1 * p1) + p2 * p2), den = len > 1e-12 ? len : 1e-12;
    const double n0 = p0 / den, n1 = p1 / den, n2 = p2 / den;
    double dot = (n0 * g0 + (-n2) * (-g1)) + n1 * g2;
    dot = dot > 1.0 ? 1.0 : (dot < -1.0 ? -1.0 : dot);
    const double err = acos(dot) / EV_PI * 180.0;
    return sqrt((g0 * g0 + g1 * g1) + g2 * g2) > 1.1 ? 180.0 : err;
}

// One wave per image; its lanes loop over the image's detections.  best[m][g] = the lowest rank among the detections that qualify for
// metric m with ground truth g: ranks are distinct within an image, so the minimum names one detection whatever the order of arrival.
__global__ __launch_bounds__(A3D_WAVE) void eval_match_kernel(const a3d_eval_match_desc a) {
    __shared__ int best[4][EV_MAX_GT];
    const int img = blockIdx.x, lane = threadIdx.x;
    const int d0 = ev_clampi(a.det_off[img], 0, a.N), d1 = ev_clampi(a.det_off[img + 1], d0, a.N);
    const int g0 = ev_clampi(a.gt_off[img], 0, a.M), g1 = ev_clampi(a.gt_off[img + 1], g0, a.M);
    const int G = min(g1 - g0, EV_MAX_GT);
#pragma unroll
    for (int m = 0; m < 4; ++m) best[m][lane] = INT_MAX;
    __syncthreads();
    const double size = (double)max(a.img_w, a.img_h);
    for (int d = d0 + lane; d < d1; d += A3D_WAVE) {
        const float *row = a.det + (size_t)d * EV_DET;
        const int rank = ev_rank(a.det, d0, d1, d);
        double biou;
        const int gid = ev_best_gt(row, a.gt_f + (size_t)g0 * EV_GF, EV_GF, G, &biou);
        const bool valid = G > 0 && biou > a.filter_iou;
        double ea = 0.0, err = 180.0;
        unsigned q = 0;
        if (valid) {
            const float *gf = a.gt_f + (size_t)(g0 + gid) * EV_GF;
            const int *gi = a.gt_i + (size_t)(g0 + gid) * EV_GI;
            const bool tran = gi[1] != 0;
            const int *gl = gi + (tran ? 7 : 2);
            if (gl[4] != 0) {
                const EvLine pl = tran ? ev_pred_line(row, row[12], row[13], 0.0f, a.img_h, a.img_w)
                                       : ev_pred_line(row, row[9], row[10], row[11], a.img_h, a.img_w);
                ea = ev_ea(pl, EvLine{(double)gl[0], (double)gl[1], (double)gl[2], (double)gl[3]}, size);
            }
            err = ev_normal_err(row + 6, gf + 4);
            if ((int)row[5] == gi[0] && biou > a.iou_thresh) {
                const bool ax = ea > a.iou_thresh, nm = err < a.normal_thresh;
                q = 1u | (ax ? 2u : 0u) | (nm ? 4u : 0u) | (ax && nm ? 8u : 0u);
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if ((q >> m) & 1u) atomicMin(&best[m][gid], rank);
        }
        a.gt_id[d] = valid ? gid : -1;
        a.iou[d] = biou;
        a.ea[d] = ea;
        a.normal_err[d] = err;
        a.rank[d] = rank;
        a.tp[d] = (unsigned char)q;  // the qualifying bits; the second pass keeps the first of each ground truth
    }
    __syncthreads();
    for (int d = d0 + lane; d < d1; d += A3D_WAVE) {  // (every lane re-reads what it wrote itself)
        const unsigned q = a.tp[d];
        if (!q) continue;
        const int gid = a.gt_id[d], rank = a.rank[d];
        unsigned t = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (((q >> m) & 1u) && best[m][gid] == rank) t |= 1u << m;
        a.tp[d] = (unsigned char)t;
    }
}

// ---- AP -------------------------------------------------------------------------------------------------------------------------------
struct ApArgs {
    const unsigned char *tp;
    double *ap;
    int *n_entries;
    int C;
    int seg_off[A3D_EVAL_MAX_CLASSES + 1];
    int npos[A3D_EVAL_MAX_CLASSES];
};

// One workgroup per (class, metric).  The segment is walked in passes of AP_THREADS entries from its END: the envelope mpre is a
// running maximum from the end, and the inclusive count of true positives at a pass's last entry is the segment's total minus the
// passes already done, so one backward walk needs no workspace however long the segment is.  Every partial sum has a fixed owner
// and the owners are added in index order.
__global__ __launch_bounds__(AP_THREADS) void eval_ap_kernel(const ApArgs a) {
    __shared__ int wsum[AP_THREADS / A3D_WAVE];
    __shared__ double wmax[AP_THREADS / A3D_WAVE];
    __shared__ double part[AP_THREADS];
    const int c = blockIdx.x, m = blockIdx.y, tid = threadIdx.x, lane = tid & (A3D_WAVE - 1), wv = tid / A3D_WAVE;
    constexpr int NW = AP_THREADS / A3D_WAVE;
    const int s0 = a.seg_off[c], n = a.seg_off[c + 1] - s0, npos = a.npos[c];
    if (m == 0 && tid == 0) a.n_entries[c] = n;
    if (n <= 0 || npos <= 0) {
        if (tid == 0) a.ap[(size_t)m * a.C + c] = 0.0;
        return;
    }
    const unsigned char *tp = a.tp + s0;
    // the segment's number of true positives
    int cnt = 0;
    for (int i = tid; i < n; i += AP_THREADS) cnt += (tp[i] >> m) & 1;
    cnt = a3d_wave_sum(cnt);
    if (lane == 0) wsum[wv] = cnt;
    __syncthreads();
    int end_cum = 0;
    for (int w = 0; w < NW; ++w) end_cum += wsum[w];
    __syncthreads();
    double carry = 0.0, acc = 0.0;  // carry: mpre just past the pass (VOCap.py's closing sentinel 0)
    const double dn = (double)npos;
    for (int i0 = ((n - 1) / AP_THREADS) * AP_THREADS; i0 >= 0; i0 -= AP_THREADS) {
        const int i = i0 + tid;
        const int bit = i < n ? (tp[i] >> m) & 1 : 0;
        int total;
        const int before = a3d_block_exclusive_scan<AP_THREADS>(bit, wsum, total);
        const int cum = end_cum - total + before + bit;  // true positives among entries 0 .. i
        const double prec = i < n ? (double)cum / (double)(i + 1) : 0.0;
        double mx = prec;  // suffix maximum within the wave, then over the later waves and the later passes
        for (int off = 1; off < A3D_WAVE; off <<= 1) {
            const double u = __shfl_down(mx, off, A3D_WAVE);
            if (lane + off < A3D_WAVE) mx = u > mx ? u : mx;
        }
        if (lane == 0) wmax[wv] = mx;
        __syncthreads();
        double later = carry;
        for (int w = NW - 1; w > wv; --w) later = wmax[w] > later ? wmax[w] : later;
        const double mpre = mx > later ? mx : later;
        if (bit) acc += ((double)cum / dn - (double)(cum - 1) / dn) * mpre;
        double all = carry;
        for (int w = 0; w < NW; ++w) all = wmax[w] > all ? wmax[w] : all;
        carry = all;
        end_cum -= total;
        __syncthreads();
    }
    part[tid] = acc;
    __syncthreads();
    a3d_lds_tree<AP_THREADS>(part);
    if (tid == 0) a.ap[(size_t)m * a.C + c] = part[0];
}

// ---- depth L1 -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DL1_THREADS) void depth_l1_kernel(const a3d_depth_l1_desc d) {
    __shared__ double ssum[DL1_THREADS];
    __shared__ int scnt[DL1_THREADS];
    const size_t hw = (size_t)d.H * d.W;
    const float *p = d.pred + (size_t)blockIdx.x * hw, *g = d.gt + (size_t)blockIdx.x * hw;
    double s = 0.0;
    int n = 0;
    for (size_t i = threadIdx.x; i < hw; i += DL1_THREADS) {
        const float gv = g[i];
        if (gv > 1e-4f) {
            s += fabs((double)p[i] - (double)gv);
            ++n;
        }
    }
    ssum[threadIdx.x] = s;
    scnt[threadIdx.x] = n;
    __syncthreads();
    a3d_lds_tree<DL1_THREADS>(ssum, scnt);
    if (threadIdx.x == 0) {
        d.sum[blockIdx.x] = ssum[0];
        d.count[blockIdx.x] = scnt[0];
    }
}

}  // namespace

extern "C" int a3d_eval_match(const a3d_eval_match_desc *d, void *stream) {
    if (!d || d->I < 0 || d->N < 0 || d->M < 0 || d->img_h < 1 || d->img_w < 1) return A3D_ERR_ARG;
    if (d->I == 0) return (d->N == 0 && d->M == 0) ? A3D_OK : A3D_ERR_ARG;
    if (!ev_offsets_ok(d->det_off_host, d->I, d->N, 0) || !ev_offsets_ok(d->gt_off_host, d->I, d->M, EV_MAX_GT)) return A3D_ERR_ARG;
    if (!d->det_off || !d->gt_off) return A3D_ERR_ARG;
    if (d->M > 0 && (!d->gt_f || !d->gt_i)) return A3D_ERR_ARG;
    if (d->N > 0 && (!d->det || !d->gt_id || !d->iou || !d->ea || !d->normal_err || !d->rank || !d->tp)) return A3D_ERR_ARG;
    if (!(d->filter_iou == d->filter_iou) || !(d->iou_thresh == d->iou_thresh) || !(d->normal_thresh == d->normal_thresh)) return A3D_ERR_ARG;
    if (d->N == 0) return A3D_OK;
    a3d_begin();
    hipLaunchKernelGGL(eval_match_kernel, dim3(d->I), dim3(A3D_WAVE), 0, (hipStream_t)stream, *d);
    return a3d_check_launch();
}

extern "C" int a3d_eval_ap(const a3d_eval_ap_desc *d, void *stream) {
    if (!d || d->C < 1 || d->C > A3D_EVAL_MAX_CLASSES || !d->seg_off_host || !d->npos_host || !d->ap || !d->n_entries) return A3D_ERR_ARG;
    if (d->seg_off_host[0] != 0) return A3D_ERR_ARG;
    for (int c = 0; c < d->C; ++c)
        if (d->seg_off_host[c + 1] < d->seg_off_host[c]) return A3D_ERR_ARG;
    if (d->seg_off_host[d->C] > 0 && !d->tp) return A3D_ERR_ARG;
    ApArgs a = {};
    a.tp = d->tp;
    a.ap = d->ap;
    a.n_entries = d->n_entries;
    a.C = d->C;
    for (int c = 0; c <= d->C; ++c) a.seg_off[c] = d->seg_off_host[c];
    for (int c = 0; c < d->C; ++c) a.npos[c] = d->npos_host[c];
    a3d_begin();
    hipLaunchKernelGGL(eval_ap_kernel, dim3(d->C, 4), dim3(AP_THREADS), 0, (hipStream_t)stream, a);
    return a3d_check_launch();
}

extern "C" int a3d_depth_l1(const a3d_depth_l1_desc *d, void *stream) {
    if (!d || d->B < 0 || d->H < 1 || d->W < 1 || (long long)d->H * d->W >= (1ll << 31)) return A3D_ERR_ARG;
    if (d->B == 0) return A3D_OK;
    if (!d->pred || !d->gt || !d->sum || !d->count) return A3D_ERR_ARG;
    a3d_begin();
    hipLaunchKernelGGL(depth_l1_kernel, dim3(d->B), dim3(DL1_THREADS), 0, (hipStream_t)stream, *d);
    return a3d_check_launch();
}
