// PNG on the device (include/a3d.h, "PNG"): every frame of a call becomes the deflate blocks of one zlib stream, byte for byte what
// tests/png_ref.py writes.  Integer arithmetic only.
//
//   filter      one workgroup per image row: the five filters' sums of absolute signed bytes in one pass over the row (the lanes stride
//               over its bytes; the row above comes from the input, so rows are independent), a workgroup reduction, the choice, and a
//               second pass that writes the chosen filter's bytes behind the type byte.
//   tokens      one workgroup per segment (n <= 16384 filtered bytes).  Three equality masks f[g] == f[g - d], one bit per byte, built
//               64 bytes at a time by a wave ballot; L_d(i) is then a count of trailing ones from bit i, at most six 64-bit words.
//               next[i] = i + (L >= 3 ? L : 1) goes to LDS and the chain of token starts from byte 0 is found by pointer doubling:
//               round r marks jump[i] for every marked i and squares jump (read everything, barrier, write: in place), so after
//               round r the first 2^(r+1) tokens are marked and the loop ends as soon as jump[0] reaches n.  A racing mark is harmless:
//               whatever a marked byte reaches by any power of next is on the chain.  The marked bytes recompute their token (cheaper
//               than 32 KB more of LDS), count their symbols in an LDS histogram that is added to the frame's, and every byte writes
//               its token word (0: no token starts here).  The Adler partial sums ride along.
//   emit        one workgroup per segment, a contiguous run of bytes per lane.  The lanes measure their tokens in the fixed and in the
//               frame's code, two workgroup scans give both totals and every lane's bit offset, the cheapest coding is chosen, and the
//               lanes OR their codes into a little-endian bit image in LDS (whole words of disjoint bits: the order cannot matter).  A
//               Huffman coding is only chosen when it is shorter than the stored one, so the image never passes n + 4 bytes.
//   pack        one workgroup scans the segment lengths into offsets; once the host has sized the destination, one workgroup per
//               segment copies it to its place.
#include "kernel_prims.h"
#include "../../include/a3d.h"

namespace {

constexpr int MAX_N = 16384;                // bytes of the largest segment
constexpr int MASK_WORDS = MAX_N / 64 + 1;  // one zero word behind the last: a run ends there at the latest
constexpr int IMG_WORDS = (MAX_N + 8) / 4 + 2;
constexpr int HDR_WORDS = A3D_PNG_TAB_WORDS - A3D_PNG_HDR_AT;

// RFC 1951, 3.2.5
constexpr unsigned short K_LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr unsigned char K_LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr unsigned short K_DIST_BASE[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                            193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr unsigned char K_DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

constexpr unsigned int bit_reverse(unsigned int code, int len) {
    unsigned int r = 0;
    for (int i = 0; i < len; ++i) r |= (code >> i & 1u) << (len - 1 - i);
    return r;
}
// length 3 .. 258 -> (symbol - 257) | extra bits << 8 | (length - base) << 16;  symbol -> bit-reversed fixed code | length << 16
struct png_tables {
    unsigned int len[259];
    unsigned int fixed[A3D_PNG_SYMS];
};
constexpr png_tables make_tables() {
    png_tables t = {};
    for (int s = 0; s < 29; ++s) {
        const int hi = s == 28 ? 258 : s == 27 ? 257 : K_LEN_BASE[s + 1] - 1;
        for (int l = K_LEN_BASE[s]; l <= hi; ++l) t.len[l] = (unsigned int)s | (unsigned int)K_LEN_EXTRA[s] << 8 | (unsigned int)(l - K_LEN_BASE[s]) << 16;
    }
    for (int s = 0; s < 286; ++s) {
        const unsigned int code = s < 144 ? 0x30 + s : s < 256 ? 0x190 + (s - 144) : s < 280 ? s - 256 : 0xC0 + (s - 280);
        const int len = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
        t.fixed[s] = bit_reverse(code, len) | (unsigned int)len << 16;
    }
    for (int s = 0; s < 30; ++s) t.fixed[286 + s] = bit_reverse((unsigned int)s, 5) | 5u << 16;
    return t;
}
__device__ const png_tables k_tab = make_tables();

// What the kernels need of a geometry; dsym / dbits / dval: the distance symbol, its number of extra bits and their value for
// the three candidate distances 1, 3, stride.
struct png_geom {
    int H, W, stride, R, S;
    int dsym[3], dbits[3], dval[3];
    size_t cap;
};

bool make_geom(int F, int H, int W, png_geom *g) {
    if (F < 0 || H < 1 || H > 65535 || W < 1 || W > A3D_PNG_MAX_W) return false;
    g->H = H, g->W = W, g->stride = 1 + 3 * W;
    g->R = (A3D_PNG_SEG_BYTES + g->stride - 1) / g->stride;
    if (g->R < 1) g->R = 1;
    g->S = (H + g->R - 1) / g->R;
    const int d[3] = {1, 3, g->stride};
    for (int k = 0; k < 3; ++k) {
        int s = 0;
        while (s + 1 < 30 && K_DIST_BASE[s + 1] <= d[k]) ++s;
        g->dsym[k] = s, g->dbits[k] = K_DIST_EXTRA[s], g->dval[k] = d[k] - K_DIST_BASE[s];
    }
    g->cap = ((size_t)g->R * g->stride + 5 + 15) / 16 * 16;
    return true;
}
// everything the kernels index with an int
bool sizes_ok(int F, const png_geom &g) {
    return (long long)F * g.H * g.stride <= 0x7FFFFFFFll && (long long)F * g.S * (long long)g.cap <= 0x7FFFFFFFll;
}

__device__ __forceinline__ int paeth(const int a, const int b, const int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
__device__ __forceinline__ int filtered(const int t, const int x, const int a, const int b, const int c) {
    const int pred = t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (x - pred) & 255;
}

__global__ __launch_bounds__(256) void png_filter_kernel(const unsigned char *__restrict__ frames, unsigned char *__restrict__ filt, const int H, const int W,
                                                         const int pitch) {
    __shared__ int part[5][4];
    const int tid = threadIdx.x, y = blockIdx.x % H;
    const size_t f = blockIdx.x / H;
    const int n = 3 * W, stride = n + 1;
    const unsigned char *cur = frames + (f * H + y) * (size_t)pitch * 3;
    const unsigned char *up = cur - (size_t)pitch * 3;  // read for y > 0 only
    int s[5] = {0, 0, 0, 0, 0};
    for (int x = tid; x < n; x += 256) {
        const int v = cur[x], a = x >= 3 ? cur[x - 3] : 0, b = y ? up[x] : 0, c = y && x >= 3 ? up[x - 3] : 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int r = filtered(t, v, a, b, c);
            s[t] += r < 128 ? r : 256 - r;
        }
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const int w = a3d_wave_sum(s[t]);
        if ((tid & (A3D_WAVE - 1)) == 0) part[t][tid / A3D_WAVE] = w;
    }
    __syncthreads();
    int best = 0, best_sum = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const int sum = part[t][0] + part[t][1] + part[t][2] + part[t][3];
        if (t == 0 || sum < best_sum) best = t, best_sum = sum;  // ties: the lowest type
    }
    unsigned char *out = filt + (f * H + y) * (size_t)stride;
    if (tid == 0) out[0] = (unsigned char)best;
    for (int x = tid; x < n; x += 256) {
        const int v = cur[x], a = x >= 3 ? cur[x - 3] : 0, b = y ? up[x] : 0, c = y && x >= 3 ? up[x - 3] : 0;
        out[1 + x] = (unsigned char)filtered(best, v, a, b, c);
    }
}

// ones from bit i on, counted to the first zero: at most 258 + 63.  Words behind the segment's last are zero.
__device__ __forceinline__ int run_from(const unsigned long long *m, const int i) {
    int w = i >> 6;
    const int sh = i & 63;
    unsigned long long x = ~m[w] >> sh;
    if (x) return __builtin_ctzll(x);
    int run = 64 - sh;
    while (run < 258 && w + 1 < MASK_WORDS) {
        x = ~m[++w];
        if (x) return run + __builtin_ctzll(x);
        run += 64;
    }
    return run;
}
// the token that starts at byte i: L | candidate << 9, or 1 for a literal
__device__ __forceinline__ int best_token(const unsigned long long (*m)[MASK_WORDS], const int i, const int n) {
    const int cap = min(258, n - i);
    int L = 0, sel = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int l = min(run_from(m[d], i), cap);
        if (l > L) L = l, sel = d;  // ties: the smallest distance
    }
    return L >= 3 ? L | sel << 9 : 1;
}

__global__ __launch_bounds__(256) void png_token_kernel(const unsigned char *__restrict__ filt, unsigned short *__restrict__ tok, int *__restrict__ hist,
                                                        unsigned int *__restrict__ s1_out, unsigned long long *__restrict__ s2_out, const png_geom g) {
    __shared__ unsigned long long mask[3][MASK_WORDS];
    __shared__ unsigned short jump[MAX_N + 2];
    __shared__ unsigned int mark[MAX_N / 32];
    __shared__ int sh[A3D_PNG_SYMS];
    __shared__ unsigned int p1[4];
    __shared__ unsigned long long p2[4];
    const int tid = threadIdx.x, s = blockIdx.x % g.S;
    const size_t f = blockIdx.x / g.S;
    const int a = s * g.R * g.stride, n = min(g.R, g.H - s * g.R) * g.stride;  // 1 <= n <= MAX_N
    const unsigned char *frame = filt + f * (size_t)g.H * g.stride;
    const int kmax = (n + 255) / 256;
    for (int i = tid; i < A3D_PNG_SYMS; i += 256) sh[i] = 0;
    for (int i = tid; i < MAX_N / 32; i += 256) mark[i] = i == 0 ? 1u : 0u;
    for (int i = kmax * 4 + tid; i < MASK_WORDS; i += 256) mask[0][i] = mask[1][i] = mask[2][i] = 0;
    for (int k = 0; k < kmax; ++k) {
        const int i = k * 256 + tid, gi = a + i;
        const bool live = i < n;
        const int v = live ? frame[gi] : 0;
        const unsigned long long e0 = __ballot(live && gi >= 1 && frame[gi - 1] == v);
        const unsigned long long e1 = __ballot(live && gi >= 3 && frame[gi - 3] == v);
        const unsigned long long e2 = __ballot(live && gi >= g.stride && frame[gi - g.stride] == v);
        if ((tid & (A3D_WAVE - 1)) == 0) {
            const int w = i >> 6;
            mask[0][w] = e0, mask[1][w] = e1, mask[2][w] = e2;
        }
    }
    __syncthreads();
    for (int k = 0; k < kmax; ++k) {
        const int i = k * 256 + tid;
        if (i < n) {
            const int t = best_token(mask, i, n);
            jump[i] = (unsigned short)(i + (t == 1 ? 1 : t & 511));  // <= n: L is capped at n - i
        }
    }
    if (tid == 0) jump[n] = (unsigned short)n;
    __syncthreads();
    for (int r = 0; r < 15; ++r) {  // 2^14 tokens at the most
        for (int k = 0; k < kmax; ++k) {
            const int i = k * 256 + tid;
            if (i < n && (mark[i >> 5] >> (i & 31) & 1u)) {
                const int j = jump[i];
                if (j < n) atomicOr(&mark[j >> 5], 1u << (j & 31));
            }
        }
        __syncthreads();
        unsigned short t[MAX_N / 256];
#pragma unroll
        for (int k = 0; k < MAX_N / 256; ++k) {
            const int i = k * 256 + tid;
            if (i < n) t[k] = jump[jump[i]];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MAX_N / 256; ++k) {
            const int i = k * 256 + tid;
            if (i < n) jump[i] = t[k];
        }
        __syncthreads();
        if (jump[0] >= n) break;  // the same word in every lane
    }
    unsigned int s1 = 0;
    unsigned long long s2 = 0;
    unsigned short *tk = tok + f * (size_t)g.H * g.stride + a;
    for (int k = 0; k < kmax; ++k) {
        const int i = k * 256 + tid;
        if (i >= n) break;
        const unsigned int b = frame[a + i];
        s1 += b;
        s2 += (unsigned long long)(n - i) * b;
        int t = 0;
        if (mark[i >> 5] >> (i & 31) & 1u) {
            t = best_token(mask, i, n);
            if (t == 1) {
                atomicAdd(&sh[b], 1);
            } else {
                atomicAdd(&sh[257 + (k_tab.len[t & 511] & 255u)], 1);
                atomicAdd(&sh[286 + g.dsym[t >> 9]], 1);
            }
        }
        tk[i] = (unsigned short)t;
    }
    s1 = a3d_wave_sum(s1);
    s2 = a3d_wave_sum(s2);
    if ((tid & (A3D_WAVE - 1)) == 0) p1[tid / A3D_WAVE] = s1, p2[tid / A3D_WAVE] = s2;
    __syncthreads();
    if (tid == 0) {
        s1_out[blockIdx.x] = p1[0] + p1[1] + p1[2] + p1[3];
        s2_out[blockIdx.x] = p2[0] + p2[1] + p2[2] + p2[3];
        atomicAdd(&hist[f * A3D_PNG_SYMS + 256], 1);  // this segment's end of block
    }
    for (int i = tid; i < A3D_PNG_SYMS; i += 256)
        if (sh[i]) atomicAdd(&hist[f * A3D_PNG_SYMS + i], sh[i]);
}

// Appends `len` (<= 28) bits, LSB first, to a lane's stream.  acc / cnt: the bits not yet in LDS (cnt < 32 between calls); w: their word.
struct bit_writer {
    unsigned long long acc;
    int cnt, w;
    unsigned int *img;
    __device__ __forceinline__ void put(const unsigned int val, const int len) {
        acc |= (unsigned long long)val << cnt;
        cnt += len;
        if (cnt >= 32) {
            if (w < IMG_WORDS) atomicOr(&img[w], (unsigned int)acc);
            acc >>= 32;
            cnt -= 32;
            ++w;
        }
    }
    __device__ __forceinline__ void flush() {
        if (cnt > 0 && w < IMG_WORDS) atomicOr(&img[w], (unsigned int)acc);
    }
};
__device__ __forceinline__ bit_writer writer_at(unsigned int *img, const int bit) { return bit_writer{0ull, bit & 31, bit >> 5, img}; }

// One token in the code `c` (316 words: bit-reversed code | length << 16): its bits, and with EMIT its codes into the writer.
template <bool EMIT>
__device__ __forceinline__ int code_token(const int t, const unsigned int lit, const unsigned int *c, const png_geom &g, bit_writer &bw) {
    if (t == 1) {
        const unsigned int e = c[lit];
        if (EMIT) bw.put(e & 0xFFFFu, e >> 16);
        return e >> 16;
    }
    const int L = min(max(t & 511, 3), 258), sel = min(t >> 9, 2);
    const unsigned int li = k_tab.len[L], el = c[257 + (li & 255u)], ed = c[286 + g.dsym[sel]];
    const int nl = (el >> 16) + (li >> 8 & 255u), nd = (ed >> 16) + g.dbits[sel];
    if (EMIT) {
        bw.put((el & 0xFFFFu) | (li >> 16) << (el >> 16), nl);
        bw.put((ed & 0xFFFFu) | (unsigned int)g.dval[sel] << (ed >> 16), nd);
    }
    return nl + nd;
}

__global__ __launch_bounds__(256) void png_emit_kernel(const unsigned char *__restrict__ filt, const unsigned short *__restrict__ tok,
                                                       const unsigned int *__restrict__ tab, unsigned char *__restrict__ slots, int *__restrict__ seg_len,
                                                       int *__restrict__ kind_out, const png_geom g) {
    __shared__ unsigned int img[IMG_WORDS];
    __shared__ unsigned int code[2][A3D_PNG_SYMS];  // 0 the fixed code, 1 the frame's
    __shared__ int ss[2][4];
    const int tid = threadIdx.x, s = blockIdx.x % g.S;
    const size_t f = blockIdx.x / g.S;
    const int a = s * g.R * g.stride, n = min(g.R, g.H - s * g.R) * g.stride;
    const unsigned char *fs = filt + f * (size_t)g.H * g.stride + a;
    const unsigned short *tk = tok + f * (size_t)g.H * g.stride + a;
    const unsigned int *ft = tab + f * A3D_PNG_TAB_WORDS;
    for (int i = tid; i < A3D_PNG_SYMS; i += 256) {
        const unsigned int e = ft[i];
        code[0][i] = k_tab.fixed[i];
        code[1][i] = (e & 0xFFFFu) | min(e >> 16, 15u) << 16;
    }
    const int hdr_bits = (int)min(ft[A3D_PNG_SYMS], (unsigned int)(HDR_WORDS * 32));
    __syncthreads();
    const int per = (n + 255) / 256, lo = min(tid * per, n), hi = min(lo + per, n);
    bit_writer bw = {0, 0, 0, img};
    int mine[2] = {0, 0};
    for (int i = lo; i < hi; ++i) {
        const int t = tk[i];
        if (!t) continue;
        const unsigned int lit = t == 1 ? fs[i] : 0u;
        mine[0] += code_token<false>(t, lit, code[0], g, bw);
        mine[1] += code_token<false>(t, lit, code[1], g, bw);
    }
    int total[2], off[2];
    off[0] = a3d_block_exclusive_scan<256>(mine[0], ss[0], total[0]);
    off[1] = a3d_block_exclusive_scan<256>(mine[1], ss[1], total[1]);
    // bytes of a Huffman coding: its bits, 3 bits of the empty stored block, up to a byte boundary, LEN and NLEN
    const int body[2] = {3 + total[0] + (int)(code[0][256] >> 16), hdr_bits + total[1] + (int)(code[1][256] >> 16)};
    const int bytes[2] = {((body[0] + 3 + 7) >> 3) + 4, ((body[1] + 3 + 7) >> 3) + 4};
    int kind = 0, len = n + 5;
    if (bytes[0] < len) kind = 1, len = bytes[0];
    if (bytes[1] < len) kind = 2, len = bytes[1];
    unsigned char *out = slots + (size_t)blockIdx.x * g.cap;
    if (kind == 0) {
        if (tid == 0) {
            out[0] = 0;
            out[1] = (unsigned char)(n & 255), out[2] = (unsigned char)(n >> 8);
            out[3] = (unsigned char)(~n & 255), out[4] = (unsigned char)(~n >> 8 & 255);
        }
        for (int i = tid; i < n; i += 256) out[5 + i] = fs[i];
    } else {
        const int c = kind - 1, nwords = (len + 3) >> 2, hdr_words = c ? (hdr_bits + 31) >> 5 : 1;  // len < n + 5: nwords < IMG_WORDS
        for (int i = tid; i < nwords; i += 256) img[i] = i < hdr_words ? (c ? ft[A3D_PNG_HDR_AT + i] : 2u) : 0u;
        __syncthreads();
        const int first = c ? hdr_bits : 3;
        bw = writer_at(img, first + off[c]);
        for (int i = lo; i < hi; ++i) {
            const int t = tk[i];
            if (t) code_token<true>(t, t == 1 ? fs[i] : 0u, code[c], g, bw);
        }
        bw.flush();
        if (tid == 0) {
            bit_writer eob = writer_at(img, first + total[c]);
            eob.put(code[c][256] & 0xFFFFu, code[c][256] >> 16);
            eob.flush();
            for (int b = len - 2; b < len; ++b) atomicOr(&img[b >> 2], 0xFFu << (8 * (b & 3)));  // 00 00 FF FF
        }
        __syncthreads();
        for (int i = tid; i < nwords; i += 256) reinterpret_cast<unsigned int *>(out)[i] = img[i];  // cap is a multiple of 16 and >= n + 5
    }
    if (tid == 0) seg_len[blockIdx.x] = len, kind_out[blockIdx.x] = kind;
}

// seg_off[s] = bytes in front of segment s in the packed stream; frame_off[f] = seg_off[f * S], frame_off[F] = the total.  One workgroup.
__global__ __launch_bounds__(256) void png_offsets_kernel(const int *__restrict__ seg_len, int *__restrict__ seg_off, int *__restrict__ frame_off,
                                                          const int n_seg, const int S) {
    __shared__ int ss[4];
    int base = 0;
    for (int s0 = 0; s0 < n_seg; s0 += 256) {
        const int s = s0 + threadIdx.x;
        const bool live = s < n_seg;
        int total;
        const int off = base + a3d_block_exclusive_scan<256>(live ? seg_len[s] : 0, ss, total);
        __syncthreads();
        if (live) {
            seg_off[s] = off;
            if (s % S == 0) frame_off[s / S] = off;
        }
        base += total;
    }
    if (threadIdx.x == 0) frame_off[n_seg / S] = base;
}

__global__ __launch_bounds__(256) void png_pack_kernel(const unsigned char *__restrict__ slots, const int *__restrict__ seg_off, const int *__restrict__ seg_len,
                                                       unsigned char *__restrict__ packed, const long long packed_bytes, const unsigned int cap) {
    const size_t seg = blockIdx.x;
    const int len = seg_len[seg];
    const long long off = seg_off[seg];
    if (len < 0 || (unsigned int)len > cap || off < 0 || off + len > packed_bytes) return;  // never past the destination
    const unsigned char *src = slots + seg * (size_t)cap;
    for (int i = threadIdx.x; i < len; i += 256) packed[off + i] = src[i];
}

}  // namespace

extern "C" size_t a3d_png_slot_bytes(int W) {
    png_geom g;
    return make_geom(0, 1, W, &g) ? g.cap : 0;
}

extern "C" int a3d_png_scan(const unsigned char *frames, int F, int H, int W, int pitch, unsigned char *filt, unsigned short *tok, int *hist,
                            unsigned int *s1, unsigned long long *s2, void *stream) {
    png_geom g;
    if (!make_geom(F, H, W, &g) || pitch < W || !sizes_ok(F, g)) return A3D_ERR_ARG;
    if (F > 0 && (!frames || !filt || !tok || !hist || !s1 || !s2)) return A3D_ERR_ARG;
    if (F == 0) return A3D_OK;
    a3d_begin();
    if (hipMemsetAsync(hist, 0, (size_t)F * A3D_PNG_SYMS * sizeof(int), (hipStream_t)stream) != hipSuccess) return A3D_ERR_LAUNCH;
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned int)(F * H)), dim3(256), 0, (hipStream_t)stream, frames, filt, H, W, pitch);
    hipLaunchKernelGGL(png_token_kernel, dim3((unsigned int)(F * g.S)), dim3(256), 0, (hipStream_t)stream, filt, tok, hist, s1, s2, g);
    return a3d_check_launch();
}

extern "C" int a3d_png_emit(const unsigned char *filt, const unsigned short *tok, const unsigned int *tab, int F, int H, int W, unsigned char *slots,
                            int *seg_len, int *seg_off, int *frame_off, int *kind, void *stream) {
    png_geom g;
    if (!make_geom(F, H, W, &g) || !sizes_ok(F, g) || !frame_off) return A3D_ERR_ARG;
    if (F > 0 && (!filt || !tok || !tab || !slots || !seg_len || !seg_off || !kind || (uintptr_t)slots % 4 != 0)) return A3D_ERR_ARG;
    a3d_begin();
    if (F > 0)
        hipLaunchKernelGGL(png_emit_kernel, dim3((unsigned int)(F * g.S)), dim3(256), 0, (hipStream_t)stream, filt, tok, tab, slots, seg_len, kind, g);
    hipLaunchKernelGGL(png_offsets_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, seg_len, seg_off, frame_off, F * g.S, g.S);
    return a3d_check_launch();
}

extern "C" int a3d_png_pack(const unsigned char *slots, const int *seg_off, const int *seg_len, int F, int H, int W, unsigned char *packed,
                            long long packed_bytes, void *stream) {
    png_geom g;
    if (!make_geom(F, H, W, &g) || !sizes_ok(F, g) || packed_bytes < 0) return A3D_ERR_ARG;
    if (F == 0) return A3D_OK;
    if (!slots || !seg_off || !seg_len || (!packed && packed_bytes > 0)) return A3D_ERR_ARG;
    a3d_begin();
    hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned int)(F * g.S)), dim3(256), 0, (hipStream_t)stream, slots, seg_off, seg_len, packed, packed_bytes,
                       (unsigned int)g.cap);
    return a3d_check_launch();
}
