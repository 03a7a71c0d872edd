// The device primitives the non-conv kernels share: ONE definition of each collective, index rule and stated law that the training,
// evaluation and export kernels used to restate per file ("Shared primitives").  Every float
// collective states its pairing: results that tests hold bit for bit depend on it.  A call site whose assembly changes behind a helper
// beyond instruction order keeps its local form and says so (MEASUREMENTS.md lists them).
#pragma once
#include "a3d_common.h"

// ---- loads, grids, the live-row count ---------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 a3d_ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }  // p: 16-byte aligned
__device__ __forceinline__ void a3d_st4(float *p, const f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// An HBM-bound element pass of 256-thread workgroups: ceil(n / 256) of them, at least 1 and at most 2048 (grid-stride beyond).
static inline int a3d_stream_grid(size_t n) {
    const size_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// The device-side row count of a compacted batch, clamped to [0, rows] and wave-uniform (a scalar register).
__device__ __forceinline__ int a3d_live_rows(const int *live, int rows) {
    const int nl = __builtin_amdgcn_readfirstlane(*live);
    return nl < 0 ? 0 : (nl < rows ? nl : rows);
}

// ---- wave collectives -------------------------------------------------------------------------------------------------------------
// Butterfly over the wave: partner masks 32, 16, ... 1 in that order, every lane ends with the same value.  The pairing is fixed, so
// a float sum is the same bits on every run and in every caller.
template <typename T>
__device__ __forceinline__ T a3d_wave_sum(T v) {
#pragma unroll
    for (int m = A3D_WAVE / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, A3D_WAVE);
    return v;
}
// Inclusive prefix sum over the wave's lanes (distances 1, 2, ... 32): lane i ends with v_0 + ... + v_i.  Integers: order-free.
template <typename T>
__device__ __forceinline__ T a3d_wave_inclusive_scan(T v) {
    const int lane = threadIdx.x & (A3D_WAVE - 1);
#pragma unroll
    for (int d = 1; d < A3D_WAVE; d <<= 1) {
        const T u = __shfl_up(v, d, A3D_WAVE);
        if (lane >= d) v += u;
    }
    return v;
}

// ---- block collectives ------------------------------------------------------------------------------------------------------------
// Exclusive prefix sum of one integer per thread over a block of N threads: every wave's last lane posts the wave's inclusive total
// in part[wave], a barrier, then every thread adds the totals of the waves before its own; `total` = the block's sum, in every thread.
// `part` is N / A3D_WAVE words of LDS; the caller puts a __syncthreads between two uses of the same array.
template <int N, typename T>
__device__ __forceinline__ T a3d_block_exclusive_scan(const T v, T *part, T &total) {
    const int wave = threadIdx.x / A3D_WAVE;
    const T incl = a3d_wave_inclusive_scan(v);
    if ((threadIdx.x & (A3D_WAVE - 1)) == A3D_WAVE - 1) part[wave] = incl;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int j = 0; j < N / A3D_WAVE; ++j) {
        const T p = part[j];
        if (j < wave) before += p;
        total += p;
    }
    return before + incl - v;
}

// Halving tree over one or more LDS arrays of N elements that the block has filled and synchronised: red[t] = red[t] + red[t + w] for
// w = N/2, N/4, ... STOP, a barrier after each level.  The pairing (t, t + w) is fixed: bit-reproducible.  The sums end in red[0 .. STOP).
template <int N, int STOP = 1, typename... T>
__device__ __forceinline__ void a3d_lds_tree(T *...red) {
    const int t = threadIdx.x;
    for (int w = N / 2; w >= STOP; w >>= 1) {
        if (t < w) ((red[t] = red[t] + red[t + w]), ...);
        __syncthreads();
    }
}

// ---- index rules ------------------------------------------------------------------------------------------------------------------
// aten upsample_bilinear2d's source index, align_corners false: output o reads i0 and i1 with weights 1 - l1 and l1.  (No contraction
// pragma here: the inference resize is built with contraction on, the training loss without, and each keeps its rounding.)
__device__ __forceinline__ void a3d_src_index(int o, float scale, int in_size, int &i0, int &i1, float &l1) {
    float s = scale * ((float)o + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = s - (float)i0;
}

// Bit-packed mask rows: bit i of word w is pixel 32 w + i; a row of npix pixels takes a3d_mask_words(npix) words.
static inline __host__ __device__ int a3d_mask_words(const size_t npix) { return (int)((npix + 31) / 32); }
template <typename I>
__device__ __forceinline__ unsigned int a3d_mask_bit(const unsigned int *__restrict__ row, const I p) {
    return (row[p >> 5] >> (p & 31)) & 1u;
}
// The BITS (< 32) bits of pixels p .. p + BITS - 1 of a row of `words` words, at any alignment; bits past the last word read as 0.
template <int BITS>
__device__ __forceinline__ unsigned int a3d_mask_window(const unsigned int *__restrict__ row, const long long p, const int words) {
    const long long w = p >> 5;
    const int sh = (int)(p & 31);
    unsigned int m = row[w] >> sh;
    if (sh > 32 - BITS && w + 1 < words) m |= row[w + 1] << (32 - sh);
    return m & ((1u << BITS) - 1u);
}

// ---- stated laws ------------------------------------------------------------------------------------------------------------------
// Backward of v / max(|v|, eps) for an N-vector: g = gs / dn, plus the tangential term -(gs . v) / dn^2 * v / n where n = |v| >= eps
// only (clamp_min passes the gradient of |v| there; below eps dn == eps and no such term passes).  The dot product adds left to right.
template <int N>
__device__ __forceinline__ void a3d_norm_bwd(const float *v, float n, float dn, float eps, const float *gs, float *g) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] = gs[j] / dn;
    if (n >= eps) {
        float dot = gs[0] * v[0];
#pragma unroll
        for (int j = 1; j < N; ++j) dot = dot + gs[j] * v[j];
        const float dd = -dot / (dn * dn);
#pragma unroll
        for (int j = 0; j < N; ++j) g[j] += dd * v[j] / n;
    }
}

// The plane lift and the rigid pose (include/a3d.h states both for callers).  Every operation rounds on its own: the bodies (and
// a3d_norm_bwd's above) pin that with clang's fp-contract pragma, so the law holds whatever flag the including file is built with.
//   lift  float64: ray = ((x - cx)/focal, (y - cy)/focal, 1), depth = offset / (normal . ray), p = (float)(depth * ray)
__device__ __forceinline__ void a3d_plane_lift(int x, int y, double focal, double cx, double cy, const float *normal, float offset, float (&p)[3]) {
#pragma clang fp contract(off)
    const double rx = ((double)x - cx) / focal, ry = ((double)y - cy) / focal;
    const double den = (double)normal[0] * rx + (double)normal[1] * ry + (double)normal[2];
    const double depth = (double)offset / den;
    p[0] = (float)(depth * rx);
    p[1] = (float)(depth * ry);
    p[2] = (float)depth;
}
//   pose  fp32, left to right: q = p - pivot, t_i = (m[3i] qx + m[3i+1] qy + m[3i+2] qz) + pivot_i + m[9+i]; m = R (row-major) | t
__device__ __forceinline__ void a3d_pose_apply(const float *m, const float (&p)[3], const float *pivot, float (&t)[3]) {
#pragma clang fp contract(off)
    const float qx = p[0] - pivot[0], qy = p[1] - pivot[1], qz = p[2] - pivot[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = (m[3 * i] * qx + m[3 * i + 1] * qy + m[3 * i + 2] * qz) + pivot[i] + m[9 + i];
}
