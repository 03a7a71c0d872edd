// The dense mesh of one detection mask on its plane, in several rigid poses: what the reference's --save-obj block
// (tools/inference.py:44-168) gets from get_single_image_mesh's reduce_size=False branch (pkg/utils/vis.py:579-600), built on the
// GPU from opt_ops.pack_masks' bit row.  One vertex per live lattice pixel in row-major order, up to two triangles per pixel, UVs into
// the frame itself.  Byte work over a 38 KB mask that fans out to megabytes of vertices: bound by the stores, no MFMA, no atomics.
//
// THE LAW (include/a3d.h states it for callers; tests/mesh_ref.py holds it bit for bit):
//   lattice    pixels (y, x) with y % s == 0 and x % s == 0; Lh = ceil(H/s), Lw = ceil(W/s); lattice index l = (y/s)*Lw + x/s.
//              A lattice pixel is live iff its mask bit XOR invert is 1 (bit i of word w = pixel 32w+i); bits at or past H*W never are.
//   vertices   vertex k = the k-th live lattice pixel in row-major order.
//   position   float64: rx = (x - cx)/focal, ry = (y - cy)/focal, den = n0*rx + n1*ry + n2, depth = offset/den;
//              p = ((float)(depth*rx), (float)(depth*ry), (float)depth); per pose, fp32, left to right, no contraction (this file is
//              built with -ffp-contract=off): q = p - pivot, t_i = (m[3i]*qx + m[3i+1]*qy + m[3i+2]*qz) + pivot_i + m[9+i];
//              flip_yz negates t_y and t_z last.
//   uv         ((float)((double)x / W), (float)(1.0 + (-(double)y) / H))
//   faces      in the row-major order of their first vertex; for a live (y, x) with y+s < H and x+s < W: first
//              [v(y,x), v(y+s,x+s), v(y,x+s)] if (y,x+s) and (y+s,x+s) are live, then [v(y,x), v(y+s,x), v(y+s,x+s)] if (y+s,x) and
//              (y+s,x+s) are live.
//   counts     (n_verts, n_faces), the TRUE numbers even past the capacities; nothing is written at or past a capacity.
//
// Shape: the order is part of the law, so the output slots come from two exclusive prefix sums (live pixels, faces), not from atomics.
//   live    (stride > 1 only) one lattice pixel per lane, one __ballot per wave: the lattice's own bit row, 32 lattice pixels per word.
//           At stride 1 the lattice IS the mask: the other kernels read the mask words directly (XOR invert, tail masked).
//   count   one lattice WORD per thread: the live word, its right / below / below-right neighbour words (funnel shifts of the same
//           bit row) give the word's two face masks; two popcounts; a block-wide exclusive scan of both counts (wave shuffles, the
//           four wave totals through LDS); per-word prefixes, face masks and the block's totals go to the workspace.
//   scan    one block turns the block totals into exclusive offsets and writes `counts`.
//   emit    one lattice pixel per thread, so neighbouring lanes write neighbouring vertices: slot = block offset + word prefix +
//           popcount of the lower bits of the word; the rank of the pixel below comes from the same three numbers of ITS word.
//           The pose table sits in LDS; the mask is read once for all poses.
// No host synchronisation, vector stores only.
#include "kernel_prims.h"
#include "../../include/a3d.h"

namespace {

constexpr int kBlock = 256;  // threads per block; also lattice words per block of the count kernel (boff is indexed by word >> 8)

// the lattice's bit row: at stride 1 the mask words themselves (flip = invert ? ~0 : 0, the last word masked to the bits below H*W),
// else the words the live kernel wrote (flip 0, tail all ones: it never sets a bit at or past the lattice's end)
struct live_row {
    const unsigned int *words;
    unsigned int flip, tail;
    int LW;
};
__device__ __forceinline__ unsigned int live_word(const live_row r, const int w) {
    if (w < 0 || w >= r.LW) return 0u;
    const unsigned int v = r.words[w] ^ r.flip;
    return w == r.LW - 1 ? (v & r.tail) : v;
}
// 32 live bits starting at lattice index l (any alignment); bits past the row's end read as 0
__device__ __forceinline__ unsigned int live_window(const live_row r, const long long l) {
    const int w = (int)(l >> 5), sh = (int)(l & 31);
    const unsigned int lo = live_word(r, w);
    if (sh == 0) return lo;
    return (lo >> sh) | (live_word(r, w + 1) << (32 - sh));
}

struct mesh_dims {
    int H, W, s, Lw, Lh, L, LW, nb;
    int A, flip_yz, cap_v, cap_f;
    float normal[3], offset, pivot[3];
    double focal, cx, cy;
};

__global__ __launch_bounds__(kBlock) void mesh_live_kernel(const unsigned int *__restrict__ bits, unsigned int *__restrict__ live, const int W,
                                                           const int s, const int Lw, const int L, const int LW, const unsigned int invert) {
    const int l = blockIdx.x * kBlock + threadIdx.x;
    bool b = false;
    if (l < L) {
        const int ly = l / Lw, lx = l - ly * Lw;
        const int p = ly * s * W + lx * s;  // < H*W: a bit past the mask is never read
        b = (a3d_mask_bit(bits, p) ^ invert) != 0u;
    }
    const unsigned long long m = __ballot(b);
    const int lane = threadIdx.x & (A3D_WAVE - 1);
    const int w0 = (l - lane) >> 5;  // the wave's 64 lattice pixels are words w0, w0 + 1
    if (lane == 0 && w0 < LW) live[w0] = (unsigned int)m;
    if (lane == 32 && w0 + 1 < LW) live[w0 + 1] = (unsigned int)(m >> 32);
}

// a3d_block_exclusive_scan of the pair (a, b) behind ONE barrier (two calls of the helper would cost a second one); ta / tb = the
// block's totals.  `part` is [2][4] ints of LDS; the caller puts a __syncthreads between two uses of the same array.
__device__ __forceinline__ void block_exclusive_scan2(const int a, const int b, int (*part)[kBlock / A3D_WAVE], int &ea, int &eb, int &ta, int &tb) {
    const int lane = threadIdx.x & (A3D_WAVE - 1), wave = threadIdx.x / A3D_WAVE;
    const int ia = a3d_wave_inclusive_scan(a), ib = a3d_wave_inclusive_scan(b);
    if (lane == A3D_WAVE - 1) {
        part[0][wave] = ia;
        part[1][wave] = ib;
    }
    __syncthreads();
    int ba = 0, bb = 0;
    ta = tb = 0;
#pragma unroll
    for (int j = 0; j < kBlock / A3D_WAVE; ++j) {
        const int pa = part[0][j], pb = part[1][j];
        if (j < wave) {
            ba += pa;
            bb += pb;
        }
        ta += pa;
        tb += pb;
    }
    ea = ba + ia - a;
    eb = bb + ib - b;
}

__global__ __launch_bounds__(kBlock) void mesh_count_kernel(const live_row row, int *__restrict__ vpre, int *__restrict__ fpre,
                                                            unsigned int *__restrict__ upper, unsigned int *__restrict__ lower,
                                                            int *__restrict__ bsum, const int Lw, const int Lh) {
    __shared__ int part[2][kBlock / A3D_WAVE];
    const int w = blockIdx.x * kBlock + threadIdx.x;
    unsigned int lv = 0u, up = 0u, lo = 0u;
    if (w < row.LW) {
        lv = live_word(row, w);
        const long long l0 = (long long)w * 32;
        // bits whose pixel has a right neighbour (x+s < W) and a row below (y+s < H)
        unsigned int ok = 0xFFFFFFFFu;
        for (long long i = (long long)(Lw - 1) - l0 % Lw; i < 32; i += Lw) ok &= ~(1u << i);
        const long long below_end = (long long)(Lh - 1) * Lw - l0;  // lattice indices at or past (Lh-1)*Lw are the last row
        if (below_end < 32) ok &= below_end <= 0 ? 0u : ((1u << below_end) - 1u);
        const unsigned int src = lv & ok;
        if (src) {
            const unsigned int right = live_window(row, l0 + 1), below = live_window(row, l0 + Lw), diag = live_window(row, l0 + Lw + 1);
            up = src & right & diag;
            lo = src & below & diag;
        }
    }
    int ev, ef, tv, tf;
    block_exclusive_scan2(__popc(lv), __popc(up) + __popc(lo), part, ev, ef, tv, tf);
    if (w < row.LW) {
        vpre[w] = ev;
        fpre[w] = ef;
        upper[w] = up;
        lower[w] = lo;
    }
    if (threadIdx.x == 0) {
        bsum[2 * blockIdx.x] = tv;
        bsum[2 * blockIdx.x + 1] = tf;
    }
}

__global__ __launch_bounds__(kBlock) void mesh_scan_kernel(const int *__restrict__ bsum, int *__restrict__ boff, int *__restrict__ counts, const int nb) {
    __shared__ int part[2][kBlock / A3D_WAVE];
    int cv = 0, cf = 0;
    for (int base = 0; base < nb; base += kBlock) {
        const int b = base + threadIdx.x;
        const int v = b < nb ? bsum[2 * b] : 0, f = b < nb ? bsum[2 * b + 1] : 0;
        int ev, ef, tv, tf;
        block_exclusive_scan2(v, f, part, ev, ef, tv, tf);
        if (b < nb) {
            boff[2 * b] = cv + ev;
            boff[2 * b + 1] = cf + ef;
        }
        cv += tv;
        cf += tf;
        __syncthreads();  // `part` is written again by the next round
    }
    if (threadIdx.x == 0) {
        counts[0] = cv;
        counts[1] = cf;
    }
}

__global__ __launch_bounds__(kBlock) void mesh_emit_kernel(const live_row row, const int *__restrict__ vpre, const int *__restrict__ fpre,
                                                           const unsigned int *__restrict__ upper, const unsigned int *__restrict__ lower,
                                                           const int *__restrict__ boff, const float *__restrict__ xforms,
                                                           float *__restrict__ verts, float *__restrict__ uvs, int *__restrict__ faces,
                                                           const mesh_dims g) {
    __shared__ float xf[A3D_MESH_MAX_POSES][12];
    for (int i = threadIdx.x; i < g.A * 12; i += kBlock) xf[i / 12][i % 12] = xforms[i];
    __syncthreads();
    const int l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= g.L) return;
    const int w = l >> 5, i = l & 31;
    const unsigned int lv = live_word(row, w);
    if (!((lv >> i) & 1u)) return;
    const unsigned int below_me = (1u << i) - 1u;
    const int k = boff[2 * (w >> 8)] + vpre[w] + __popc(lv & below_me);
    const int ly = l / g.Lw, lx = l - ly * g.Lw;
    const int y = ly * g.s, x = lx * g.s;

    if (k < g.cap_v) {
        uvs[(size_t)k * 2] = (float)((double)x / (double)g.W);
        uvs[(size_t)k * 2 + 1] = (float)(1.0 + (-(double)y) / (double)g.H);
        float pt[3];
        a3d_plane_lift(x, y, g.focal, g.cx, g.cy, g.normal, g.offset, pt);
        for (int a = 0; a < g.A; ++a) {
            float t[3];
            a3d_pose_apply(xf[a], pt, g.pivot, t);
            float *o = verts + ((size_t)a * g.cap_v + k) * 3;
            o[0] = t[0];
            o[1] = g.flip_yz ? -t[1] : t[1];
            o[2] = g.flip_yz ? -t[2] : t[2];
        }
    }

    const unsigned int up = (upper[w] >> i) & 1u, lo = (lower[w] >> i) & 1u;
    if (!(up | lo)) return;
    // a face mask bit implies y+s < H and x+s < W: lattice indices l + Lw and l + Lw + 1 exist
    const int fb = boff[2 * (w >> 8) + 1] + fpre[w] + __popc(upper[w] & below_me) + __popc(lower[w] & below_me);
    const int l2 = l + g.Lw, w2 = l2 >> 5, i2 = l2 & 31;
    const unsigned int lv2 = live_word(row, w2);
    const int kb = boff[2 * (w2 >> 8)] + vpre[w2] + __popc(lv2 & ((1u << i2) - 1u));  // rank of (y+s, x), live or not
    const int kd = kb + (int)((lv2 >> i2) & 1u);                                        // rank of (y+s, x+s)
    if (up && fb < g.cap_f) {
        int *o = faces + (size_t)fb * 3;
        o[0] = k;
        o[1] = kd;
        o[2] = k + 1;
    }
    const int fl = fb + (int)up;
    if (lo && fl < g.cap_f) {
        int *o = faces + (size_t)fl * 3;
        o[0] = k;
        o[1] = kb;
        o[2] = kd;
    }
}

struct mesh_plan {
    int Lh, Lw, L, LW, nb;
    size_t off_live, off_vpre, off_fpre, off_upper, off_lower, off_bsum, off_boff, bytes;
};

// lattice sizes and the workspace's layout; false when the sizes are out of range (H*W must stay below 2^30 so that 2*H*W faces fit int32)
bool mesh_make_plan(const int H, const int W, const int s, mesh_plan *p) {
    if (H < 1 || W < 1 || s < 1 || (size_t)H * (size_t)W > 0x3FFFFFFFull) return false;
    p->Lh = (int)(((long long)H + s - 1) / s);
    p->Lw = (int)(((long long)W + s - 1) / s);
    p->L = p->Lh * p->Lw;
    p->LW = a3d_mask_words((size_t)p->L);
    p->nb = (p->LW + kBlock - 1) / kBlock;
    size_t at = 0;
    const size_t per_word = (size_t)p->LW * 4, per_block = (size_t)p->nb * 8;
    p->off_live = at, at += per_word;
    p->off_vpre = at, at += per_word;
    p->off_fpre = at, at += per_word;
    p->off_upper = at, at += per_word;
    p->off_lower = at, at += per_word;
    p->off_bsum = at, at += per_block;
    p->off_boff = at, at += per_block;
    p->bytes = at;
    return true;
}

}  // namespace

extern "C" size_t a3d_mesh_workspace_bytes(int H, int W, int stride) {
    mesh_plan p;
    return mesh_make_plan(H, W, stride, &p) ? p.bytes : 0;
}

extern "C" int a3d_mesh_build(const a3d_mesh_desc *d, void *stream) {
    if (!d) return A3D_ERR_ARG;
    mesh_plan p;
    if (!mesh_make_plan(d->H, d->W, d->stride, &p)) return A3D_ERR_ARG;
    if (d->A < 1 || d->A > A3D_MESH_MAX_POSES || d->cap_v < 0 || d->cap_f < 0) return A3D_ERR_ARG;
    if (!d->bits || !d->xforms || !d->counts || !d->workspace) return A3D_ERR_ARG;
    if ((d->cap_v > 0 && (!d->verts || !d->uvs)) || (d->cap_f > 0 && !d->faces)) return A3D_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)d->workspace;
    unsigned int *live = (unsigned int *)(ws + p.off_live), *upper = (unsigned int *)(ws + p.off_upper), *lower = (unsigned int *)(ws + p.off_lower);
    int *vpre = (int *)(ws + p.off_vpre), *fpre = (int *)(ws + p.off_fpre), *bsum = (int *)(ws + p.off_bsum), *boff = (int *)(ws + p.off_boff);
    const unsigned int inv = d->invert ? 1u : 0u;
    live_row row;
    a3d_begin();
    if (d->stride == 1) {
        const int nbits = p.L - (p.LW - 1) * 32;  // 1 .. 32 mask bits in the last word
        row = {d->bits, inv ? 0xFFFFFFFFu : 0u, nbits == 32 ? 0xFFFFFFFFu : ((1u << nbits) - 1u), p.LW};
    } else {
        hipLaunchKernelGGL(mesh_live_kernel, dim3((p.L + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d->bits, live, d->W, d->stride, p.Lw, p.L, p.LW, inv);
        row = {live, 0u, 0xFFFFFFFFu, p.LW};
    }
    mesh_dims g;
    g.H = d->H, g.W = d->W, g.s = d->stride, g.Lw = p.Lw, g.Lh = p.Lh, g.L = p.L, g.LW = p.LW, g.nb = p.nb;
    g.A = d->A, g.flip_yz = d->flip_yz ? 1 : 0, g.cap_v = d->cap_v, g.cap_f = d->cap_f;
    for (int i = 0; i < 3; ++i) g.normal[i] = d->normal[i], g.pivot[i] = d->pivot[i];
    g.offset = d->offset, g.focal = d->focal, g.cx = d->cx, g.cy = d->cy;
    hipLaunchKernelGGL(mesh_count_kernel, dim3(p.nb), dim3(kBlock), 0, s, row, vpre, fpre, upper, lower, bsum, p.Lw, p.Lh);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kBlock), 0, s, bsum, boff, d->counts, p.nb);
    hipLaunchKernelGGL(mesh_emit_kernel, dim3((p.L + kBlock - 1) / kBlock), dim3(kBlock), 0, s, row, vpre, fpre, upper, lower, boff, d->xforms, d->verts,
                       d->uvs, d->faces, g);
    return a3d_check_launch();
}
