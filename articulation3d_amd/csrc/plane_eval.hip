// Evaluation of the plane stage on the device: the reference's ScanNet box / mask / plane AP (ScannetEvaluator -> evaluate_for_planes,
// pkg/evaluation/scannet_evaluation.py:254-450 over compare_planes, pkg/utils/metrics.py:6-19).  The reference turns every mask into an
// RLE on the host and calls pycocotools' iou on every (detection, ground truth) pair of an image, then uses one column of that matrix
// per detection.  Here a3d_eval_mask_counts reads the pasted masks where the detector left them, once, and counts each detection
// against the ONE ground truth its box selects; a3d_eval_plane_match then decides the three metrics per image.  The law of both is
// stated in include/a3d.h and, in numpy float64, by tests/plane_eval_ref.py.
//
// a3d_eval_mask_counts is the only launch here with real traffic: 307 KB per detection at 480 x 640, 490 MB for 16 images of 100
// detections, against 38 KB of ground-truth bits per detection that mostly stay in L2 (a few ground truths per image serve all its
// detections).  It is a pure stream, so the shape is (detection, block of PE_BLOCK pixels) -- 1600 x 19 workgroups for that batch,
// far more than the chip holds at once -- with 16 bytes per lane and load, consecutive lanes on consecutive 16-byte groups.  A mask row
// starts at slot * H * W bytes, which is 16-byte aligned only by luck: the wide loads begin at the first aligned ADDRESS of the block
// and the bytes before it and after the last whole group go one by one.  The bits that belong to an aligned group of mask bytes then
// start anywhere in a word; they come out of the (at most two) words that hold them.  Sums are integers, added with integer atomics
// (LDS, then one per workgroup and counter on the global counters a first launch zeroes): no result depends on the order of arrival.
#include "kernel_prims.h"
#include "eval_common.h"

#include <limits.h>

namespace {
constexpr int EV_DET = A3D_EVAL_DET_COLS, PG = A3D_PLANE_GT_COLS, EV_MAX_GT = A3D_EVAL_MAX_GT;
constexpr double EV_PI = 3.141592653589793;  // numpy's np.pi
constexpr int PE_THREADS = 256;
constexpr int PE_LOADS = 4;                             // 16-byte loads per lane and block, all issued before the first is used
constexpr int PE_BLOCK = PE_THREADS * PE_LOADS * 16;    // pixels per workgroup: a multiple of 32, so blocks never share a word of bits

// The image of detection n: the i with off[i] <= n < off[i+1] over the clamped offsets, itself clamped to [0, I).
__device__ __forceinline__ int pe_image_of(const int *off, int I, int N, int n) {
    int lo = 0, hi = I;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ev_clampi(off[mid + 1], 0, N) <= n) lo = mid + 1;
        else hi = mid;
    }
    return lo < I ? lo : I - 1;
}

// One thread per detection: its ground truth, and the two counters set to zero.
__global__ __launch_bounds__(PE_THREADS) void pe_assign_kernel(const a3d_eval_mask_counts_desc a) {
    const int n = blockIdx.x * PE_THREADS + threadIdx.x;
    if (n >= a.N) return;
    const int img = pe_image_of(a.det_off, a.I, a.N, n);
    const int g0 = ev_clampi(a.gt_off[img], 0, a.M), g1 = ev_clampi(a.gt_off[img + 1], g0, a.M);
    const int G = min(g1 - g0, EV_MAX_GT);
    double biou;
    const int gid = ev_best_gt(a.det + (size_t)n * EV_DET, a.gt + (size_t)g0 * PG, PG, G, &biou);
    a.gt_id[n] = G > 0 ? gid : -1;
    a.inter[n] = 0;
    a.uni[n] = 0;
}

// bit k of the result = byte k of v is non-zero (k = 0 .. 3, the lowest address first)
__device__ __forceinline__ unsigned pe_nonzero4(unsigned v) {
    const unsigned t = (((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u;  // bit 7 of every non-zero byte
    return ((t >> 7) * 0x10204080u) >> 28;                                      // bits 0, 8, 16, 24 -> 0, 1, 2, 3 (no two products meet)
}

__global__ __launch_bounds__(PE_THREADS) void pe_counts_kernel(const a3d_eval_mask_counts_desc a, const int hw, const int words) {
    __shared__ int s_row, s_slot, s_cnt[2];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * PE_BLOCK, p1 = p0 + min(hw - p0, PE_BLOCK);  // (the grid has ceil(hw / PE_BLOCK) blocks: p0 < hw < 2^31)
    for (int n = blockIdx.y; n < a.N; n += gridDim.y) {
        if (tid == 0) {
            const int img = pe_image_of(a.det_off, a.I, a.N, n);
            const int g0 = ev_clampi(a.gt_off[img], 0, a.M), g1 = ev_clampi(a.gt_off[img + 1], g0, a.M);
            const int G = min(g1 - g0, EV_MAX_GT), gid = a.gt_id[n];
            s_row = (G > 0 && gid >= 0) ? g0 + min(gid, G - 1) : -1;
            const int slot = a.det_slot[n];
            s_slot = (slot >= 0 && slot < a.S) ? slot : -1;
            s_cnt[0] = s_cnt[1] = 0;
        }
        __syncthreads();
        const unsigned *grow = s_row >= 0 ? a.gt_bits + (size_t)s_row * words : nullptr;
        const unsigned char *mrow = s_slot >= 0 ? a.masks + (size_t)s_slot * hw : nullptr;
        int inter = 0, uni = 0;
        if (grow || mrow) {
            // an empty mask has no address: its block counts as aligned (PE_BLOCK is a multiple of 16)
            const int head = mrow ? min((int)((16u - (unsigned)((uintptr_t)(mrow + p0) & 15u)) & 15u), p1 - p0) : 0;
            const int groups = (p1 - p0 - head) >> 4, b0 = p0 + head, b1 = b0 + (groups << 4);
            uint4 v[PE_LOADS];
#pragma unroll
            for (int k = 0; k < PE_LOADS; ++k) {
                const int j = tid + k * PE_THREADS;
                v[k] = (mrow && j < groups) ? *reinterpret_cast<const uint4 *>(mrow + b0 + (j << 4)) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int k = 0; k < PE_LOADS; ++k) {
                const int j = tid + k * PE_THREADS;
                if (j < groups) {
                    const unsigned m = pe_nonzero4(v[k].x) | (pe_nonzero4(v[k].y) << 4) | (pe_nonzero4(v[k].z) << 8) | (pe_nonzero4(v[k].w) << 12);
                    const unsigned g = grow ? a3d_mask_window<16>(grow, b0 + (j << 4), words) : 0u;
                    inter += __popc(m & g);
                    uni += __popc(m | g);
                }
            }
            const int singles = head + (p1 - b1);  // at most 15 + 15 pixels, one lane each
            if (tid < singles) {
                const int p = tid < head ? p0 + tid : b1 + (tid - head);
                const unsigned m = (mrow && mrow[p]) ? 1u : 0u;
                const unsigned g = grow ? a3d_mask_bit(grow, p) : 0u;
                inter += m & g;
                uni += m | g;
            }
        }
        inter = a3d_wave_sum(inter);
        uni = a3d_wave_sum(uni);
        if ((tid & (A3D_WAVE - 1)) == 0 && (inter | uni)) {
            atomicAdd(&s_cnt[0], inter);
            atomicAdd(&s_cnt[1], uni);
        }
        __syncthreads();
        if (tid == 0) {
            if (s_cnt[0]) atomicAdd(a.inter + n, s_cnt[0]);
            if (s_cnt[1]) atomicAdd(a.uni + n, s_cnt[1]);
        }
        __syncthreads();  // (thread 0 rewrites the shared words at the top of the next detection)
    }
}

// compare_planes for one pair (a3d.h: "planes")
__device__ void pe_compare(const float *p, const float *g, double *normal_err, double *offset_err) {
    const double p0 = p[0], p1 = p[1], p2 = p[2], g0 = g[0], g1 = g[1], g2 = g[2];
    const double op = sqrt((p0 * p0 + p1 * p1) + p2 * p2) + 1e-5, og = sqrt((g0 * g0 + g1 * g1) + g2 * g2) + 1e-5;
    const double dx = p0 / op - g0 / og, dy = p1 / op - g1 / og, dz = p2 / op - g2 / og;
    double d = sqrt((dx * dx + dy * dy) + dz * dz);
    d = d < 0.0 ? 0.0 : (d > 2.0 ? 2.0 : d);
    *normal_err = 2.0 * asin(d / 2.0) / EV_PI * 180.0;
    *offset_err = fabs(op - og);
}

// One wave per image, shaped like eval_match_kernel: best[m][g] = the lowest rank among the detections that qualify for metric m with
// ground truth g (ranks are distinct within an image, so the minimum names one detection whatever the order of arrival).
__global__ __launch_bounds__(A3D_WAVE) void plane_match_kernel(const a3d_eval_plane_match_desc a) {
    __shared__ int best[3][EV_MAX_GT];
    const int img = blockIdx.x, lane = threadIdx.x;
    const int d0 = ev_clampi(a.det_off[img], 0, a.N), d1 = ev_clampi(a.det_off[img + 1], d0, a.N);
    const int g0 = ev_clampi(a.gt_off[img], 0, a.M), g1 = ev_clampi(a.gt_off[img + 1], g0, a.M);
    const int G = min(g1 - g0, EV_MAX_GT);
#pragma unroll
    for (int m = 0; m < 3; ++m) best[m][lane] = INT_MAX;
    __syncthreads();
    for (int d = d0 + lane; d < d1; d += A3D_WAVE) {
        const float *row = a.det + (size_t)d * EV_DET;
        const int rank = ev_rank(a.det, d0, d1, d);
        double biou;
        const int gid = ev_best_gt(row, a.gt + (size_t)g0 * PG, PG, G, &biou);
        double miou = 0.0, nerr = 180.0, oerr = (double)INFINITY;
        unsigned q = 0;
        if (G > 0) {
            const float *g = a.gt + (size_t)(g0 + gid) * PG;
            const int inter = a.inter[d], uni = a.uni[d];
            miou = uni > 0 ? (double)inter / (double)uni : 0.0;
            pe_compare(row + 6, g + 4, &nerr, &oerr);
            if ((int)row[5] == (int)g[7])
                q = (biou > a.iou_thresh ? 1u : 0u) | (miou > a.iou_thresh ? 2u : 0u) | ((nerr < a.normal_thresh && oerr < a.offset_thresh) ? 4u : 0u);
#pragma unroll
            for (int m = 0; m < 3; ++m)
                if ((q >> m) & 1u) atomicMin(&best[m][gid], rank);
        }
        a.gt_id[d] = G > 0 ? gid : -1;
        a.rank[d] = rank;
        a.box_iou[d] = biou;
        a.mask_iou[d] = miou;
        a.normal_err[d] = nerr;
        a.offset_err[d] = oerr;
        a.tp[d] = (unsigned char)q;  // the qualifying bits; the second pass keeps the first of each ground truth
    }
    __syncthreads();
    for (int d = d0 + lane; d < d1; d += A3D_WAVE) {  // (every lane re-reads what it wrote itself)
        const unsigned q = a.tp[d];
        if (!q) continue;
        const int gid = a.gt_id[d], rank = a.rank[d];
        unsigned t = 0;
#pragma unroll
        for (int m = 0; m < 3; ++m)
            if (((q >> m) & 1u) && best[m][gid] == rank) t |= 1u << m;
        a.tp[d] = (unsigned char)t;
    }
}

// what both descriptors share: counts and the two offset tables
bool pe_tables_ok(int I, int N, int M, const int *det_off_host, const int *gt_off_host, const int *det_off, const int *gt_off) {
    if (I < 0 || N < 0 || M < 0) return false;
    if (I == 0) return N == 0 && M == 0;
    return ev_offsets_ok(det_off_host, I, N, 0) && ev_offsets_ok(gt_off_host, I, M, EV_MAX_GT) && det_off && gt_off;
}
}  // namespace

extern "C" int a3d_eval_mask_counts(const a3d_eval_mask_counts_desc *d, void *stream) {
    if (!d || d->S < 0 || d->H < 1 || d->W < 1 || (long long)d->H * d->W >= (1ll << 31)) return A3D_ERR_ARG;
    if (!pe_tables_ok(d->I, d->N, d->M, d->det_off_host, d->gt_off_host, d->det_off, d->gt_off)) return A3D_ERR_ARG;
    if (d->M > 0 && (!d->gt || !d->gt_bits)) return A3D_ERR_ARG;
    if (d->S > 0 && !d->masks) return A3D_ERR_ARG;
    if (d->N > 0 && (!d->det || !d->det_slot || !d->gt_id || !d->inter || !d->uni)) return A3D_ERR_ARG;
    if (d->I == 0 || d->N == 0) return A3D_OK;
    const int hw = d->H * d->W, words = a3d_mask_words((size_t)hw);
    a3d_begin();
    hipLaunchKernelGGL(pe_assign_kernel, dim3((d->N + PE_THREADS - 1) / PE_THREADS), dim3(PE_THREADS), 0, (hipStream_t)stream, *d);
    hipLaunchKernelGGL(pe_counts_kernel, dim3((hw - 1) / PE_BLOCK + 1, d->N < 65535 ? d->N : 65535), dim3(PE_THREADS), 0, (hipStream_t)stream,
                       *d, hw, words);
    return a3d_check_launch();
}

extern "C" int a3d_eval_plane_match(const a3d_eval_plane_match_desc *d, void *stream) {
    if (!d || !pe_tables_ok(d->I, d->N, d->M, d->det_off_host, d->gt_off_host, d->det_off, d->gt_off)) return A3D_ERR_ARG;
    if (d->M > 0 && !d->gt) return A3D_ERR_ARG;
    if (d->N > 0 && (!d->det || !d->inter || !d->uni || !d->gt_id || !d->rank || !d->box_iou || !d->mask_iou || !d->normal_err || !d->offset_err || !d->tp))
        return A3D_ERR_ARG;
    if (!(d->iou_thresh == d->iou_thresh) || !(d->normal_thresh == d->normal_thresh) || !(d->offset_thresh == d->offset_thresh)) return A3D_ERR_ARG;
    if (d->I == 0 || d->N == 0) return A3D_OK;
    a3d_begin();
    hipLaunchKernelGGL(plane_match_kernel, dim3(d->I), dim3(A3D_WAVE), 0, (hipStream_t)stream, *d);
    return a3d_check_launch();
}
