// The clip's visualisation panels on the GPU: what the reference's tools/inference.py:230-276 draws per frame with
// matplotlib (draw_pred: box outlines + articulation-axis arrows over the frame; get_normal_map: the surface-normal map),
// here one launch over layer / piece / instance tables that articulation3d_amd/render.py builds on the host once per clip.
// Per-pixel byte work over data that is already on the device (the resized uint8 frames, opt_ops.pack_masks' bit masks):
// HBM-bound, no MFMA, no atomics, no host synchronisation.
//
// THE LAW (include/a3d.h states it for callers; tests/render_ref.py holds it bit for bit):
//   seg panel     start from the frame's pixel; apply the frame's layers [layer_off[f], layer_off[f+1]) in table order.
//                 A layer covers a pixel AT MOST ONCE, however many of its pieces do; where it does, every channel becomes
//                     (old*(256-alpha) + color*alpha + 128) >> 8            (integers; alpha 0 .. 256)
//                 MASK layer: covered = the mask bit (bit i of word w = pixel 32w+i, row-major).
//                 POLY layer: covered = OR over its pieces; a pixel is inside a piece iff e >= 0 for each of the piece's n
//                 half-planes (A,B,C), with px = x + 0.5f, py = y + 0.5f, e = (A*px + B*py) + C in fp32, in exactly that
//                 order, no contraction (this file is built with -ffp-contract=off).  A piece with n = 0 covers nothing.
//                 A cull box (every layer has one, every piece has one) is a SUPERSET of the coverage: it only lets a wave
//                 skip the layer / the piece, it never changes a byte.
//   normal panel  n = sum_i bit_i * normal_i, component-wise in fp32 over the frame's instances in ascending order;
//                 v = (n + 1.0f) / 2.0f * 255.0f, in that order; byte = low 8 bits of v truncated toward zero to int32.
//                 With at most two masks over a pixel and v in [0, 256) this is the reference's get_normal_map exactly
//                 (matmul of the 0/1 masks with F.normalize(plane), then astype(uint8)): a sum of at most two non-zero
//                 fp32 terms does not depend on the order.  The WRAP for v outside [0, 256) (three unit normals that add
//                 up, a negative sum) is this library's stated choice: numpy's float -> uint8 cast is unspecified there.
//                 Normals must be finite (|v| then stays far inside int32).
// Placement: out is [F, H, pitch, 3]; frame f's seg panel is written to columns [col, col+W), its normal panel to
// [col+W, col+2W); nothing else is touched.  Two calls fill the reference's row [opt seg | opt normal | raw seg | raw normal].
//
// Shape: a thread owns 4 horizontally adjacent pixels of both panels -- one mask word per instance (two where a row
// width that is no multiple of 4 makes the 4 pixels straddle a word), 12 bytes per panel as three dwords when the frame
// rows and the output columns are 4-pixel aligned (byte accesses otherwise: any H, W >= 1 works, the tail of a row
// included).  The frame index and the table cursors are wave-uniform, so layer / piece / instance records come through
// scalar loads; a wave whose pixel span misses a layer's cull box (one ballot) never touches its pieces or mask word,
// and one that misses a piece's box skips its half-planes.
#include "kernel_prims.h"
#include "../../include/a3d.h"

namespace {

// A table record as ONE group of scalar loads.  Left to itself the compiler loads each field where it is first used -- behind the
// short-circuit of the box test, behind the branch on the kind -- which costs a wave two or three dependent round trips per record; the
// empty asm pins every dword of the record to a scalar register at this point, so the loads leave together and are waited for once.
template <typename T>
__device__ __forceinline__ T load_record(const T *__restrict__ rec) {
    static_assert(sizeof(T) % 4 == 0, "records are whole dwords");
    union {
        T t;
        int w[sizeof(T) / 4];
    } u;
    const int *__restrict__ src = reinterpret_cast<const int *>(rec);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 4); ++k) u.w[k] = src[k];
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 4); ++k) asm volatile("" : "+s"(u.w[k]));
    return u.t;
}

struct render_dims {
    int F, H, W, pitch, col, n_layers, n_pieces, n_inst, n_masks, groups, words, vec_in, vec_out;
};

// (the tables are separate __restrict__ parameters, not the descriptor by value: only then does the compiler know that the
// stores to `out` cannot change them and reads the wave-uniform records with scalar loads)
__global__ __launch_bounds__(256) void render_panels_kernel(const unsigned char *__restrict__ frames, const int *__restrict__ layer_off,
                                                            const a3d_render_layer *__restrict__ layers,
                                                            const a3d_render_piece *__restrict__ pieces, const int *__restrict__ inst_off,
                                                            const int *__restrict__ inst_row, const float *__restrict__ normals,
                                                            const unsigned int *__restrict__ bits, unsigned char *__restrict__ out,
                                                            const render_dims d) {
    const int groups = d.groups, words = d.words, vec_in = d.vec_in, vec_out = d.vec_out;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= d.H * groups) return;
    const int y = t / groups, x = (t - y * groups) * 4;
    const int nv = min(4, d.W - x);  // valid pixels of this thread (the row's tail)
    const unsigned int live = (1u << nv) - 1u;
    const long long p = (long long)y * d.W + x;
    const float py = (float)y + 0.5f;

    for (int f = blockIdx.y; f < d.F; f += gridDim.y) {
        // ---- the frame's 4 pixels
        int c[12];
        const unsigned char *src = frames + (((size_t)f * d.H + y) * d.W + x) * 3;
        if (vec_in) {
            const unsigned int *s4 = reinterpret_cast<const unsigned int *>(src);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const unsigned int v = s4[q];
#pragma unroll
                for (int b = 0; b < 4; ++b) c[q * 4 + b] = (int)((v >> (8 * b)) & 0xFFu);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) c[j * 3 + k] = j < nv ? (int)src[j * 3 + k] : 0;
        }

        // ---- seg panel: the layers in table order
        const int l0 = max(layer_off[f], 0), l1 = min(layer_off[f + 1], d.n_layers);
        for (int l = l0; l < l1; ++l) {
            const a3d_render_layer L = load_record(layers + l);
            const bool in_box = x < L.x1 && x + 4 > L.x0 && y >= L.y0 && y < L.y1;
            if (__ballot(in_box) == 0ull) continue;  // the wave's pixel span misses the cull box
            unsigned int cov = 0;
            if (L.kind == A3D_RENDER_MASK) {
                if (L.p0 >= 0 && L.p0 < d.n_masks) cov = a3d_mask_window<4>(bits + (size_t)L.p0 * words, p, words);
            } else {
                const int p1 = min(L.p1, d.n_pieces);
                for (int q = max(L.p0, 0); q < p1; ++q) {
                    const a3d_render_piece P = load_record(pieces + q);
                    // (most of a layer's box is empty for an outline or an arrow: the piece's own box lets the wave skip the arithmetic)
                    if (__ballot(x < P.x1 && x + 4 > P.x0 && y >= P.y0 && y < P.y1) == 0ull) continue;
                    const int n = min(P.n, A3D_RENDER_MAX_HALFPLANES);
                    unsigned int in = n > 0 ? 0xFu : 0u;
#pragma unroll
                    for (int h = 0; h < A3D_RENDER_MAX_HALFPLANES; ++h) {
                        if (h < n) {
                            const float A = P.abc[h][0], B = P.abc[h][1], C = P.abc[h][2];
                            const float by = B * py;
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const float px = (float)(x + j) + 0.5f;
                                const float e = (A * px + by) + C;
                                if (!(e >= 0.f)) in &= ~(1u << j);
                            }
                        }
                    }
                    cov |= in;
                }
            }
            cov &= live;
            const int a = L.alpha, ia = 256 - L.alpha;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((cov >> j) & 1u) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) c[j * 3 + k] = (c[j * 3 + k] * ia + (int)L.color[k] * a + 128) >> 8;
                }
        }

        // ---- normal panel: the instances in ascending order
        float nrm[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) nrm[i] = 0.f;
        const int i0 = max(inst_off[f], 0), i1 = min(inst_off[f + 1], d.n_inst);
        for (int i = i0; i < i1; ++i) {
            const int row = inst_row[i];
            if (row < 0 || row >= d.n_masks) continue;
            const float n0 = normals[(size_t)i * 3], n1 = normals[(size_t)i * 3 + 1], n2 = normals[(size_t)i * 3 + 2];
            const unsigned int m = a3d_mask_window<4>(bits + (size_t)row * words, p, words);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float b = (float)((m >> j) & 1u);
                nrm[j * 3] = nrm[j * 3] + b * n0;
                nrm[j * 3 + 1] = nrm[j * 3 + 1] + b * n1;
                nrm[j * 3 + 2] = nrm[j * 3 + 2] + b * n2;
            }
        }
        int g[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const float v = (nrm[i] + 1.0f) / 2.0f * 255.0f;
            g[i] = (int)v & 0xFF;  // (v_cvt_i32_f32: truncation toward zero)
        }

        // ---- both panels out
        unsigned char *dst = out + (((size_t)f * d.H + y) * d.pitch + d.col + x) * 3;
        unsigned char *dst_n = dst + (size_t)d.W * 3;
        if (vec_out) {
            unsigned int *o4 = reinterpret_cast<unsigned int *>(dst), *n4 = reinterpret_cast<unsigned int *>(dst_n);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                o4[q] = (unsigned int)c[q * 4] | ((unsigned int)c[q * 4 + 1] << 8) | ((unsigned int)c[q * 4 + 2] << 16) | ((unsigned int)c[q * 4 + 3] << 24);
                n4[q] = (unsigned int)g[q * 4] | ((unsigned int)g[q * 4 + 1] << 8) | ((unsigned int)g[q * 4 + 2] << 16) | ((unsigned int)g[q * 4 + 3] << 24);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        dst[j * 3 + k] = (unsigned char)c[j * 3 + k];
                        dst_n[j * 3 + k] = (unsigned char)g[j * 3 + k];
                    }
                }
        }
    }
}

}  // namespace

extern "C" int a3d_render_panels(const a3d_render_desc *d, void *stream) {
    if (!d || d->F < 0 || d->H < 1 || d->W < 1 || d->col < 0 || d->pitch < 1 || (long long)d->col + 2ll * d->W > (long long)d->pitch) return A3D_ERR_ARG;
    if (d->n_layers < 0 || d->n_pieces < 0 || d->n_inst < 0 || d->n_masks < 0) return A3D_ERR_ARG;
    if ((size_t)d->H * d->W > 0x7FFFFFFFull - 31) return A3D_ERR_ARG;
    if ((d->n_layers > 0 && !d->layers) || (d->n_pieces > 0 && !d->pieces) || (d->n_inst > 0 && (!d->inst_row || !d->normals)) ||
        (d->n_masks > 0 && !d->bits))
        return A3D_ERR_ARG;
    if (d->F > 0 && (!d->frames || !d->out || !d->layer_off || !d->inst_off)) return A3D_ERR_ARG;
    if (d->F == 0) return A3D_OK;
    const int groups = (d->W + 3) / 4;
    const int words = a3d_mask_words((size_t)d->H * d->W);
    // dword accesses need every row start, the panel's first column and its width on a 4-pixel (12-byte) boundary
    const int vec_in = (d->W % 4 == 0) && ((uintptr_t)d->frames % 4 == 0);
    const int vec_out = (d->W % 4 == 0) && (d->pitch % 4 == 0) && (d->col % 4 == 0) && ((uintptr_t)d->out % 4 == 0);
    const long long threads = (long long)d->H * groups;
    const render_dims dims = {d->F, d->H, d->W, d->pitch, d->col, d->n_layers, d->n_pieces, d->n_inst, d->n_masks, groups, words, vec_in, vec_out};
    a3d_begin();
    hipLaunchKernelGGL(render_panels_kernel, dim3((unsigned int)((threads + 255) / 256), d->F < 65535 ? d->F : 65535), dim3(256), 0,
                       (hipStream_t)stream, d->frames, d->layer_off, d->layers, d->pieces, d->inst_off, d->inst_row, d->normals, d->bits,
                       d->out, dims);
    return a3d_check_launch();
}
