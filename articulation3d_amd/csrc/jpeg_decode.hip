// Baseline JPEG decode on the device (include/a3d.h, "JPEG decode"): the entropy-coded bytes of F frames of one geometry become
// uint8 [F,H,pitch,3] RGB, byte for byte what tests/jpeg_decode_ref.py computes.  Integer arithmetic only.  One memset (the
// coefficient scratch, each frame's status word at its tail included) and three launches:
//
//   entropy   one lane per unit (a restart interval, or the whole scan), 16 units per workgroup, the lanes of a workgroup in one frame.
//             The workgroup turns its frame's six Huffman specifications into an 8-bit lookahead table plus the Annex F first-code /
//             count rows for the longer codes, in LDS.  A lane reads its unit by aligned dword loads, one cached word at a time, drops
//             the 00 behind every FF, and writes each non-zero coefficient as int16 at its natural place in the zeroed scratch.  The
//             lanes of a wave walk different streams, so their loops diverge, and a scan without restart intervals keeps one lane of
//             one wave busy per frame: that is the price of the format, and MEASUREMENTS.md says what it costs.
//   idct      32 blocks per workgroup, 8 lanes per block.  Lane r loads row r (one 16-byte load) and dequantises it, lane j transforms
//             column j, lane r transforms row r and stores its 8 samples as one 8-byte word; rows meet columns in LDS (rows padded to 9
//             words).  The domain test of the law is taken here and raised into the frame's status word.
//   colour    one lane per 16 pixels of a row: chroma upsampled as the law states, converted, clamped, and stored as three 16-byte
//             words where the destination allows (bytes otherwise).  The first lane of a frame publishes its status word.
//
// What keeps every access inside the call's buffers, whatever the stream holds: a lane's byte cursor runs over [lo, hi) of its unit,
// both clamped to the data (past hi it reads zeros); a code's symbol index is below the table's symbol count by construction of the
// first-code rows; a coefficient index is tested against 63 before the store; a unit's MCU range is clamped to the frame's MCUs, and
// every block of an MCU inside that range lies inside the component's padded plane.
#include "kernel_prims.h"
#include "../../include/a3d.h"

namespace {

constexpr int SET_QUANT = 192;           // bytes of the three quantisation tables in front of a table set
constexpr int SET_TABLE = 16 + 256;      // one Huffman specification: bits[16], vals[256]
static_assert(A3D_JPEG_TABSET_BYTES == SET_QUANT + 6 * SET_TABLE, "table set layout");
constexpr int DOMAIN = 16383;

__device__ const unsigned char k_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct dec_geom {
    int F, H, W, pitch, ncomp, hs, vs, mx, my;
    int h[3], v[3], bw[3], bh[3];   // sampling factors and padded size in blocks of every component
    long long cblk[4];               // first block of every component within a frame; cblk[ncomp] = blocks per frame
    long long coef_frame, plane_frame, poff[3];
    int n_units, n_sets, data_bytes;
};

bool make_geom(int F, int H, int W, int pitch, int ncomp, int hs, int vs, dec_geom *g) {
    if (F < 0 || H < 1 || W < 1 || H > 65535 || W > 65535 || pitch < W) return false;
    if (!(ncomp == 1 && hs == 1 && vs == 1) && !(ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)))) return false;
    g->F = F, g->H = H, g->W = W, g->pitch = pitch, g->ncomp = ncomp, g->hs = hs, g->vs = vs;
    g->mx = (W + 8 * hs - 1) / (8 * hs), g->my = (H + 8 * vs - 1) / (8 * vs);
    long long blk = 0, pix = 0;
    for (int c = 0; c < 3; ++c) {
        g->h[c] = c == 0 ? hs : 1, g->v[c] = c == 0 ? vs : 1;
        g->bw[c] = c < ncomp ? g->mx * g->h[c] : 0, g->bh[c] = c < ncomp ? g->my * g->v[c] : 0;
        g->cblk[c] = blk, g->poff[c] = pix;
        blk += (long long)g->bw[c] * g->bh[c];
        pix += (long long)g->bw[c] * g->bh[c] * 64;
    }
    g->cblk[3] = blk;
    if (ncomp == 1) g->cblk[1] = g->cblk[2] = blk;
    g->coef_frame = blk * 64 + 8;  // the frame's status word lives in the 16 bytes behind its coefficients
    g->plane_frame = pix;
    return true;
}

// ---- entropy ------------------------------------------------------------------------------------------------------------------------
struct huff_lds {
    unsigned short lut[256];  // 8 leading bits -> length << 8 | symbol of a code of at most 8 bits, else 0
    int first[17];            // first code of every length (Annex C)
    unsigned short cum[17];   // codes shorter than or as long as l
    unsigned short nb[17];    // codes of length l
    unsigned char vals[256];
};

struct bit_reader {
    const unsigned int *words;
    unsigned long long acc;  // the low `cnt` bits are the stream's next bits
    unsigned int w;
    int cnt, pos, end, widx, pad;
    bool ff;
    __device__ __forceinline__ void refill() {
        while (cnt <= 56) {
            unsigned int b;
            for (;;) {
                if (pos >= end) {  // past the unit: zeros, counted (8 or more of them in `acc` mean every bit there is one)
                    b = 0, ff = false;
                    pad = min(pad + 1, 16);
                    break;
                }
                const int wi = pos >> 2;
                if (wi != widx) widx = wi, w = words[wi];
                b = (w >> (8 * (pos & 3))) & 0xFFu;
                ++pos;
                if (ff && b == 0) {  // FF 00 is the data byte FF
                    ff = false;
                    continue;
                }
                ff = b == 0xFFu;
                break;
            }
            acc = acc << 8 | b;
            cnt += 8;
        }
    }
    // The next symbol of table t, or -1 where the next 16 bits start no code (they are consumed).  Leaves at least 16 bits in `acc`.
    __device__ __forceinline__ int symbol(const huff_lds &t) {
        if (cnt < 32) refill();
        const unsigned int p = (unsigned int)(acc >> (cnt - 16)) & 0xFFFFu;
        const unsigned int e = t.lut[p >> 8];
        if (e) {
            cnt -= (int)(e >> 8);
            return (int)(e & 255u);
        }
        for (int l = 9; l <= 16; ++l) {
            const int d = (int)(p >> (16 - l)) - t.first[l];
            if (d >= 0 && d < (int)t.nb[l]) {
                cnt -= l;
                return t.vals[min(t.cum[l - 1] + d, 255)];
            }
        }
        cnt -= 16;
        return -1;
    }
    // s <= 15 bits behind a symbol, extended: the value of a coefficient of category s
    __device__ __forceinline__ int value(const int s) {
        if (s == 0) return 0;
        const int v = (int)(acc >> (cnt - s)) & ((1 << s) - 1);
        cnt -= s;
        return v >> (s - 1) ? v : v - (1 << s) + 1;
    }
    __device__ __forceinline__ bool ran_short() const { return cnt < 8 * pad; }
};

// One block into its 64 zeroed coefficients; false at a bad code.
__device__ __forceinline__ bool decode_block(bit_reader &rd, short *__restrict__ dst, int &pred, const huff_lds &dc, const huff_lds &ac,
                                             const unsigned char *zig) {
    const int s = rd.symbol(dc);
    if (s < 0 || s > 15) return false;
    pred = (short)(pred + rd.value(s));  // modulo 2^16
    if (pred) dst[0] = (short)pred;
    int i = 1;
    while (i < 64) {
        const int rs = rd.symbol(ac);
        if (rs < 0) return false;
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            if (r != 15) break;  // EOB
            i += 16;             // ZRL
            if (i > 64) return false;
            continue;
        }
        i += r;
        if (i > 63) return false;
        dst[zig[i]] = (short)rd.value(sz);
        ++i;
    }
    return true;
}

// Units per workgroup.  A wave runs the distinct paths of its live lanes one after the other, so fewer lanes per wave buy less
// serialisation at the price of more table builds: 16 was measured against 64 (MEASUREMENTS.md, "JPEG decode").
constexpr int EN_LANES = 16;

__global__ __launch_bounds__(EN_LANES) void jpeg_decode_entropy_kernel(const unsigned int *__restrict__ data, const int *__restrict__ meta,
                                                                       const unsigned char *__restrict__ sets, short *__restrict__ coef,
                                                                       const dec_geom g) {
    __shared__ huff_lds T[6];
    __shared__ unsigned char zig[64];
    const int lane = threadIdx.x, f = blockIdx.y;
    const int *unit_off = meta, *frame_unit = meta + g.n_units + 1, *frame_ri = frame_unit + g.F + 1, *frame_set = frame_ri + g.F;
    const int set = min(max(frame_set[f], 0), g.n_sets - 1);
    const unsigned char *spec = sets + (size_t)set * A3D_JPEG_TABSET_BYTES + SET_QUANT;
    const int n_tab = 2 * g.ncomp;
    for (int i = lane; i < 64; i += EN_LANES) zig[i] = k_zigzag[i];
    if (lane < n_tab) {
        const unsigned char *bits = spec + lane * SET_TABLE;
        huff_lds &t = T[lane];
        int code = 0, cum = 0;
        t.first[0] = 0, t.cum[0] = 0, t.nb[0] = 0;
        for (int l = 1; l <= 16; ++l) {
            const int n = bits[l - 1];
            t.first[l] = code, t.nb[l] = (unsigned short)n;
            cum = min(cum + n, 256);
            t.cum[l] = (unsigned short)cum;
            code = (code + n) << 1;
        }
    }
    for (int t = 0; t < n_tab; ++t)
        for (int i = lane; i < 256; i += EN_LANES) T[t].vals[i] = spec[t * SET_TABLE + 16 + i];
    __syncthreads();
    for (int t = 0; t < n_tab; ++t)
        for (int e = lane; e < 256; e += EN_LANES) {
            unsigned short hit = 0;
            for (int l = 8; l >= 1; --l) {  // (a valid specification is prefix-free: at most one length matches)
                const int d = (e >> (8 - l)) - T[t].first[l];
                if (d >= 0 && d < (int)T[t].nb[l]) hit = (unsigned short)(l << 8 | T[t].vals[min(T[t].cum[l - 1] + d, 255)]);
            }
            T[t].lut[e] = hit;
        }
    __syncthreads();

    const int u0 = frame_unit[f], u1 = frame_unit[f + 1];
    const long long k = (long long)blockIdx.x * EN_LANES + lane;  // this lane's unit within the frame
    if (u0 < 0 || u1 > g.n_units || k >= (long long)u1 - u0) return;
    const long long total = (long long)g.mx * g.my;
    const long long ri = frame_ri[f] > 0 ? frame_ri[f] : total;
    const long long m0 = k * ri, m1 = min(m0 + ri, total);
    if (m0 >= total) return;
    const int u = u0 + (int)k;
    bit_reader rd;
    rd.words = data, rd.acc = 0, rd.w = 0, rd.cnt = 0, rd.widx = -1, rd.pad = 0, rd.ff = false;
    rd.pos = min(max(unit_off[u], 0), g.data_bytes);
    rd.end = min(max(unit_off[u + 1], rd.pos), g.data_bytes);
    short *cf = coef + (size_t)f * g.coef_frame;
    int pred[3] = {0, 0, 0};
    int mxi = (int)(m0 % g.mx), myi = (int)(m0 / g.mx);
    bool ok = true;
    for (long long m = m0; m < m1 && ok; ++m) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= g.ncomp || !ok) continue;
            for (int vy = 0; vy < g.v[c] && ok; ++vy)
                for (int vx = 0; vx < g.h[c] && ok; ++vx) {
                    const long long blk = g.cblk[c] + (long long)(myi * g.v[c] + vy) * g.bw[c] + mxi * g.h[c] + vx;
                    ok = decode_block(rd, cf + blk * 64, pred[c], T[2 * c], T[2 * c + 1], zig);
                }
        }
        if (++mxi == g.mx) mxi = 0, ++myi;
    }
    const int st = rd.ran_short() ? A3D_JPEG_SHORT : ok ? 0 : A3D_JPEG_BAD_CODE;
    if (st) atomicMax(reinterpret_cast<int *>(cf + g.cblk[3] * 64), st);
}

// ---- dequantise + IDCT ----------------------------------------------------------------------------------------------------------------
// One jidctint pass ("islow", CONST_BITS 13): x in, y out, descaled by `shift`.  Inside the domain every intermediate fits int32.
__device__ __forceinline__ void idct8(const int (&x)[8], int (&y)[8], const int shift) {
    int z2 = x[2], z3 = x[6];
    int z1 = (z2 + z3) * 4433;
    int t2 = z1 - z3 * 15137, t3 = z1 + z2 * 6270;
    int t0 = (x[0] + x[4]) * 8192, t1 = (x[0] - x[4]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
    z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2;
    int z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;
    t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
    const int r = 1 << (shift - 1);
    y[0] = (t10 + t3 + r) >> shift, y[7] = (t10 - t3 + r) >> shift;
    y[1] = (t11 + t2 + r) >> shift, y[6] = (t11 - t2 + r) >> shift;
    y[2] = (t12 + t1 + r) >> shift, y[5] = (t12 - t1 + r) >> shift;
    y[3] = (t13 + t0 + r) >> shift, y[4] = (t13 - t0 + r) >> shift;
}

constexpr int ID_BLOCKS = 32;  // blocks per workgroup (8 lanes each)
constexpr int ID_LD = 9;

__global__ __launch_bounds__(256) void jpeg_decode_idct_kernel(short *__restrict__ coef, const int *__restrict__ meta, const unsigned char *__restrict__ sets,
                                                               unsigned char *__restrict__ planes, const dec_geom g, const long long n_blocks) {
    __shared__ int sA[ID_BLOCKS * 8 * ID_LD];
    const int tid = threadIdx.x, b = tid >> 3, r = tid & 7;
    const long long gb = (long long)blockIdx.x * ID_BLOCKS + b;
    const bool live = gb < n_blocks;
    const long long f = live ? gb / g.cblk[3] : 0, blk = live ? gb - f * g.cblk[3] : 0;
    const int c = blk >= g.cblk[2] ? 2 : blk >= g.cblk[1] ? 1 : 0;
    int *my = sA + b * 8 * ID_LD;
    bool out = false;
    if (live) {
        const int set = min(max(meta[g.n_units + 1 + g.F + 1 + g.F + f], 0), g.n_sets - 1);
        const uint2 qv = *reinterpret_cast<const uint2 *>(sets + (size_t)set * A3D_JPEG_TABSET_BYTES + c * 64 + r * 8);
        const uint4 cv = *reinterpret_cast<const uint4 *>(coef + (size_t)f * g.coef_frame + blk * 64 + r * 8);
        const unsigned int cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[2] = {qv.x, qv.y};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int d = (int)(short)(cw[k >> 1] >> (16 * (k & 1))) * (int)((qw[k >> 2] >> (8 * (k & 3))) & 0xFFu);
            out |= abs(d) > DOMAIN;
            my[r * ID_LD + k] = min(max(d, -DOMAIN - 1), DOMAIN);
        }
    }
    __syncthreads();
    if (live) {  // column r, in place: no other lane touches it in this phase
        int x[8], y[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = my[k * ID_LD + r];
        idct8(x, y, 11);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            out |= abs(y[k]) > DOMAIN;
            my[k * ID_LD + r] = min(max(y[k], -DOMAIN - 1), DOMAIN);
        }
    }
    __syncthreads();
    if (live) {
        int x[8], y[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = my[r * ID_LD + k];
        idct8(x, y, 18);
        unsigned int lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (unsigned int)min(max(y[k] + 128, 0), 255) << (8 * k);
            hi |= (unsigned int)min(max(y[k + 4] + 128, 0), 255) << (8 * k);
        }
        const long long local = blk - g.cblk[c];
        const int by = (int)(local / g.bw[c]), bx = (int)(local - (long long)by * g.bw[c]);
        unsigned char *dst = planes + (size_t)f * g.plane_frame + g.poff[c] + ((size_t)(by * 8 + r) * g.bw[c] + bx) * 8;
        *reinterpret_cast<uint2 *>(dst) = make_uint2(lo, hi);
        if (out) atomicMax(reinterpret_cast<int *>(coef + (size_t)f * g.coef_frame + g.cblk[3] * 64), A3D_JPEG_RANGE);
    }
}

// ---- upsample + colour ----------------------------------------------------------------------------------------------------------------
// The chroma sample of pixel (x, y): p the component's plane (pw samples a row), dw x dh its true size.
__device__ __forceinline__ int chroma_at(const unsigned char *__restrict__ p, const int pw, const int dw, const int dh, const int x, const int y,
                                         const int hs, const int vs) {
    if (hs == 1) return p[(size_t)y * pw + x];
    if (dw <= 2) return p[(size_t)(y >> (vs - 1)) * pw + (x >> 1)];  // too narrow for the filter: replicated
    const int i = x >> 1, in = (x & 1) ? min(i + 1, dw - 1) : max(i - 1, 0);
    if (vs == 1) return (3 * p[(size_t)y * pw + i] + p[(size_t)y * pw + in] + ((x & 1) ? 2 : 1)) >> 2;
    const int j = y >> 1, jn = (y & 1) ? min(j + 1, dh - 1) : max(j - 1, 0);
    const unsigned char *near = p + (size_t)j * pw, *far = p + (size_t)jn * pw;
    const int si = 3 * near[i] + far[i], sn = 3 * near[in] + far[in];
    return (3 * si + sn + ((x & 1) ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_decode_colour_kernel(const unsigned char *__restrict__ planes, const short *__restrict__ coef,
                                                                 unsigned char *__restrict__ rgb, int *__restrict__ status, const dec_geom g,
                                                                 const long long n_groups, const int groups, const int vec) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= n_groups) return;
    const long long row = gi / groups;
    const int x0 = (int)(gi - row * groups) * 16;
    const long long f = row / g.H;
    const int y = (int)(row - f * g.H);
    if (x0 == 0 && y == 0) status[f] = *reinterpret_cast<const int *>(coef + (size_t)f * g.coef_frame + g.cblk[3] * 64);
    const unsigned char *pl = planes + (size_t)f * g.plane_frame;
    const int pw0 = g.bw[0] * 8, pw1 = g.bw[1] * 8;
    const int dw = (g.W + g.hs - 1) / g.hs, dh = (g.H + g.vs - 1) / g.vs;
    unsigned int w[12] = {};
#pragma unroll
    for (int n = 0; n < 16; ++n) {
        const int x = min(x0 + n, g.W - 1);
        const int Y = pl[(size_t)y * pw0 + x];
        int R = Y, G = Y, B = Y;
        if (g.ncomp == 3) {
            const int cb = chroma_at(pl + g.poff[1], pw1, dw, dh, x, y, g.hs, g.vs) - 128;
            const int cr = chroma_at(pl + g.poff[2], pw1, dw, dh, x, y, g.hs, g.vs) - 128;
            R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
            G = min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
            B = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
        }
        w[(3 * n) >> 2] |= (unsigned int)R << (8 * ((3 * n) & 3));
        w[(3 * n + 1) >> 2] |= (unsigned int)G << (8 * ((3 * n + 1) & 3));
        w[(3 * n + 2) >> 2] |= (unsigned int)B << (8 * ((3 * n + 2) & 3));
    }
    unsigned char *dst = rgb + ((size_t)row * g.pitch + x0) * 3;
    if (vec && x0 + 16 <= g.W) {
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        d4[0] = make_uint4(w[0], w[1], w[2], w[3]);
        d4[1] = make_uint4(w[4], w[5], w[6], w[7]);
        d4[2] = make_uint4(w[8], w[9], w[10], w[11]);
    } else {
        const int nb = 3 * min(16, g.W - x0);
#pragma unroll
        for (int i = 0; i < 48; ++i)
            if (i < nb) dst[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
    }
}

}  // namespace

extern "C" int a3d_jpeg_decode_scratch(int H, int W, int ncomp, int hs, int vs, size_t *coef_elems, size_t *plane_elems) {
    dec_geom g;
    if (!coef_elems || !plane_elems || !make_geom(0, H, W, W, ncomp, hs, vs, &g)) return A3D_ERR_ARG;
    *coef_elems = (size_t)g.coef_frame;
    *plane_elems = (size_t)g.plane_frame;
    return A3D_OK;
}

extern "C" int a3d_jpeg_decode(const a3d_jpeg_decode_desc *d, void *stream) {
    dec_geom g;
    if (!d || !make_geom(d->F, d->H, d->W, d->pitch, d->ncomp, d->hs, d->vs, &g)) return A3D_ERR_ARG;
    if (d->F == 0) return A3D_OK;
    if (d->F > 65535 || d->n_units < 1 || d->n_sets < 1 || d->data_bytes < 0 || d->data_bytes > 0x7FFFFFFFll) return A3D_ERR_ARG;
    if (!d->unit_off || !d->frame_unit || !d->frame_ri || !d->frame_set || !d->sets || !d->d_meta || !d->d_sets || !d->coef || !d->planes || !d->rgb ||
        !d->status || (!d->d_data && d->data_bytes > 0))
        return A3D_ERR_ARG;
    if ((uintptr_t)d->d_data % 4 || (uintptr_t)d->d_sets % 8 || (uintptr_t)d->coef % 16 || (uintptr_t)d->planes % 8) return A3D_ERR_ARG;
    if (d->unit_off[0] != 0 || d->unit_off[d->n_units] != d->data_bytes || d->frame_unit[0] != 0 || d->frame_unit[d->F] != d->n_units) return A3D_ERR_ARG;
    for (int u = 0; u < d->n_units; ++u)
        if (d->unit_off[u + 1] < d->unit_off[u]) return A3D_ERR_ARG;
    const long long total = (long long)g.mx * g.my;
    long long most = 0;
    for (int f = 0; f < d->F; ++f) {
        const long long ri = d->frame_ri[f] > 0 ? d->frame_ri[f] : total, n = (long long)d->frame_unit[f + 1] - d->frame_unit[f];
        if (d->frame_ri[f] < 0 || n != (total + ri - 1) / ri || d->frame_set[f] < 0 || d->frame_set[f] >= d->n_sets) return A3D_ERR_ARG;
        most = n > most ? n : most;
    }
    for (int s = 0; s < d->n_sets; ++s)
        for (int t = 0; t < 2 * d->ncomp; ++t) {  // Annex C: the codes of every length must fit that length
            const unsigned char *bits = d->sets + (size_t)s * A3D_JPEG_TABSET_BYTES + SET_QUANT + t * SET_TABLE;
            int code = 0, n = 0;
            for (int l = 1; l <= 16; ++l) {
                code += bits[l - 1], n += bits[l - 1];
                if (code > (1 << l)) return A3D_ERR_ARG;
                code <<= 1;
            }
            if (n > 256) return A3D_ERR_ARG;
        }
    g.n_units = d->n_units, g.n_sets = d->n_sets, g.data_bytes = (int)d->data_bytes;
    const long long n_blocks = (long long)d->F * g.cblk[3], id_grid = (n_blocks + ID_BLOCKS - 1) / ID_BLOCKS;
    const int groups = (d->W + 15) / 16;
    const long long n_groups = (long long)d->F * d->H * groups, co_grid = (n_groups + 255) / 256, en_grid = (most + EN_LANES - 1) / EN_LANES;
    if (id_grid > 0x7FFFFFFFll || co_grid > 0x7FFFFFFFll || en_grid > 0x7FFFFFFFll) return A3D_ERR_ARG;
    const int vec = (uintptr_t)d->rgb % 16 == 0 && ((size_t)d->pitch * 3) % 16 == 0;
    a3d_begin();
    if (hipMemsetAsync(d->coef, 0, (size_t)d->F * g.coef_frame * sizeof(short), (hipStream_t)stream) != hipSuccess) return A3D_ERR_LAUNCH;
    hipLaunchKernelGGL(jpeg_decode_entropy_kernel, dim3((unsigned int)en_grid, (unsigned int)d->F), dim3(EN_LANES), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned int *>(d->d_data), d->d_meta, d->d_sets, d->coef, g);
    hipLaunchKernelGGL(jpeg_decode_idct_kernel, dim3((unsigned int)id_grid), dim3(256), 0, (hipStream_t)stream, d->coef, d->d_meta, d->d_sets, d->planes,
                       g, n_blocks);
    hipLaunchKernelGGL(jpeg_decode_colour_kernel, dim3((unsigned int)co_grid), dim3(256), 0, (hipStream_t)stream, d->planes, d->coef, d->rgb, d->status, g,
                       n_groups, groups, vec);
    return a3d_check_launch();
}
