// What the evaluation launches share (csrc/eval.hip: the articulation AP; csrc/plane_eval.hip: the ScanNet box / mask / plane AP): the
// box IoU, a detection's ground truth and its rank, by ONE law (include/a3d.h, a3d_eval_match), and the host check of an offsets table.
// Both translation units are built with -ffp-contract=off: every float64 operator rounds on its own, as numpy's do.
#pragma once
#include "a3d_common.h"
#include "../../include/a3d.h"

__device__ __forceinline__ int ev_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ double ev_iou(const float *a, const float *b) {
    const double ax1 = a[0], ay1 = a[1], ax2 = a[2], ay2 = a[3], bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
    const double area_a = (ax2 - ax1) * (ay2 - ay1), area_b = (bx2 - bx1) * (by2 - by1);
    double w = (ax2 < bx2 ? ax2 : bx2) - (ax1 > bx1 ? ax1 : bx1), h = (ay2 < by2 ? ay2 : by2) - (ay1 > by1 ? ay1 : by1);
    w = w > 0.0 ? w : 0.0;
    h = h > 0.0 ? h : 0.0;
    const double inter = w * h;
    return inter > 0.0 ? inter / ((area_a + area_b) - inter) : 0.0;
}

// The ground truth of a box among G rows of `cols` floats (box xyxy first): the largest IoU, the lowest index on ties.  -> its index
// (0 when G == 0), *best its IoU (0 when G == 0).
__device__ __forceinline__ int ev_best_gt(const float *box, const float *gt_rows, int cols, int G, double *best) {
    int gid = 0;
    double biou = 0.0;
    for (int g = 0; g < G; ++g) {
        const double v = ev_iou(box, gt_rows + (size_t)g * cols);
        if (g == 0 || v > biou) {
            biou = v;
            gid = g;
        }
    }
    *best = biou;
    return gid;
}

// The number of detections j in [d0, d1) with score_j > score_d, or score_j == score_d and j < d.
__device__ __forceinline__ int ev_rank(const float *det, int d0, int d1, int d) {
    const float sc = det[(size_t)d * A3D_EVAL_DET_COLS + 4];
    int rank = 0;
    for (int j = d0; j < d1; ++j) {
        const float sj = det[(size_t)j * A3D_EVAL_DET_COLS + 4];
        rank += (sj > sc || (sj == sc && j < d)) ? 1 : 0;
    }
    return rank;
}

// HOST: 0 = off[0] <= off[1] <= ... <= off[I] = total, no step above max_per (0: any).
static inline bool ev_offsets_ok(const int *off, int I, int total, int max_per) {
    if (!off || off[0] != 0 || off[I] != total) return false;
    for (int i = 0; i < I; ++i) {
        if (off[i + 1] < off[i]) return false;
        if (max_per > 0 && off[i + 1] - off[i] > max_per) return false;
    }
    return true;
}
