// Baseline JPEG decode on the device (include/a3d.h, "JPEG decode"): the entropy-coded bytes of F frames of one geometry become
// uint8 [F,H,pitch,3] RGB, byte for byte what tests/jpeg_decode_ref.py computes.  Integer arithmetic only.  One memset (the
// coefficient scratch, each frame's status word at its tail included) and three launches:
//
//   entropy   a unit (a restart interval, or the whole scan) is cut into subsequences that many lanes walk at once and that synchronise
//             themselves; the lanes of a unit share a workgroup, short units share one, the units of a workgroup are of one frame
//             ("entropy" below states the scheme).  The workgroup turns its frame's six Huffman specifications into an 8-bit
//             lookahead table plus the Annex F first-code / count rows for the longer codes, in LDS.  A lane reads its bytes by
//             aligned dword loads, one cached word at a time, drops the 00 behind every FF, and writes each non-zero coefficient as
//             int16 at its natural place in the zeroed scratch.  The lanes of a wave walk different bytes, so their loops diverge:
//             that is the price of the format, and MEASUREMENTS.md says what it costs.
//   idct      32 blocks per workgroup, 8 lanes per block.  Lane r loads row r (one 16-byte load) and dequantises it, lane j transforms
//             column j, lane r transforms row r and stores its 8 samples as one 8-byte word; rows meet columns in LDS (rows padded to 9
//             words).  The domain test of the law is taken here and raised into the frame's status word.
//   colour    one lane per 16 pixels of a row: chroma upsampled as the law states, converted, clamped, and stored as three 16-byte
//             words where the destination allows (bytes otherwise).  The first lane of a frame publishes its status word.
//
// What keeps every access inside the call's buffers, whatever the stream holds, is stated with the entropy kernel; the dense launches
// index by the geometry alone, and a frame's table index is clamped where it is read.
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
    // Block (vx, vy) of component c in MCU (mxi, myi), counted within a frame
    __device__ __forceinline__ long long block(const int c, const int mxi, const int myi, const int vy, const int vx) const {
        return cblk[c] + (long long)(myi * v[c] + vy) * bw[c] + mxi * h[c] + vx;
    }
};

// d_meta: the descriptor's four host tables back to back.  The per-frame rows, and a frame's table set with its index clamped.
struct dec_meta {
    const int *unit_off, *frame_unit, *frame_ri, *frame_set;
    __device__ __forceinline__ dec_meta(const int *meta, const dec_geom &g)
        : unit_off(meta), frame_unit(meta + g.n_units + 1), frame_ri(frame_unit + g.F + 1), frame_set(frame_ri + g.F) {}
    __device__ __forceinline__ const unsigned char *table_set(const unsigned char *sets, const dec_geom &g, const long long f) const {
        return sets + (size_t)min(max(frame_set[f], 0), g.n_sets - 1) * A3D_JPEG_TABSET_BYTES;
    }
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

// ---- entropy: the tables ----------------------------------------------------------------------------------------------------------------
struct huff_lds {
    unsigned short lut[256];  // 8 leading bits -> length << 8 | symbol of a code of at most 8 bits, else 0
    int first[17];            // first code of every length (Annex C)
    unsigned short cum[17];   // codes shorter than or as long as l
    unsigned short nb[17];    // codes of length l
    unsigned char vals[256];
};

// The workgroup's form of a frame's Huffman specifications (`spec`: n_tab of them, bits[16] + vals[256] each) and the zig-zag order, in
// LDS: every one of the workgroup's `lanes` threads calls it.  It ends behind a barrier.
__device__ __forceinline__ void build_tables(huff_lds *T, unsigned char *zig, const unsigned char *__restrict__ spec, const int n_tab, const int lane,
                                             const int lanes) {
    for (int i = lane; i < 64; i += lanes) zig[i] = k_zigzag[i];
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
        for (int i = lane; i < 256; i += lanes) T[t].vals[i] = spec[t * SET_TABLE + 16 + i];
    __syncthreads();
    for (int t = 0; t < n_tab; ++t)
        for (int e = lane; e < 256; e += lanes) {
            unsigned short hit = 0;
            for (int l = 8; l >= 1; --l) {  // (a valid specification is prefix-free: at most one length matches)
                const int d = (e >> (8 - l)) - T[t].first[l];
                if (d >= 0 && d < (int)T[t].nb[l]) hit = (unsigned short)(l << 8 | T[t].vals[min(T[t].cum[l - 1] + d, 255)]);
            }
            T[t].lut[e] = hit;
        }
    __syncthreads();
}

// ---- entropy: the walk -------------------------------------------------------------------------------------------------------------------
// A unit's stuffed bytes are cut into subsequences of S = max(split_bytes, ceil(unit bytes / lpu)) bytes, one lane each; the lpu lanes
// of a unit (a power of two, 1024 at the most) sit in one workgroup, and a workgroup holds blockDim / lpu units of one frame, so all
// synchronisation is LDS and barriers.  A decoder state between two syntax elements is (position, slot within the MCU, zig-zag index;
// 0: a DC symbol is next), one 64-bit word.  Round 0 walks lane j >= 1 from (its first data bit, 0, 0) and lane 0 from the unit's
// start; in every later round a lane whose left neighbour's exit differs from the entry it last used walks again from there, until a
// round changes nothing (a workgroup vote) or lpu rounds have run: after round r the lanes 0 .. r hold their true states, so the fixed
// point is the sequential walk whatever the stream holds.  A speculative walk carries on past an inconsistency (it consumes what the
// law consumes, ends the block, goes to the next slot) and records the number of blocks it had begun by then.  An exclusive sum of the
// begun-block counts gives every lane the ordinal of its first block; the first flagged lane whose bad block is one of the unit's ends
// the unit.  Then every lane in front of it walks once more from its true entry and stores AC values at their places and the DC
// DIFFERENCE at coefficient 0, the unit's last lane walking on (zeros past the bytes) until the unit's blocks are done; a per-component
// sum of the differences in scan order, modulo 2^16, turns them into DC values behind a barrier.
//
// What keeps every access inside the call's buffers: the reader fetches bytes of [lo, hi) of its unit only, both clamped to the data
// (zeros beyond); a code's symbol index is below the table's symbol count by construction of the first-code rows; a block's ordinal
// is tested against the unit's block count before its address is formed, so it lies in the unit's own MCUs; a coefficient index is
// at most 63 by the tests of `element`; LDS is indexed by the thread and by its unit within the workgroup.  Every loop is bounded: a
// walk by its end bit or by the unit's blocks (an element moves the index forward and a block takes at most 64 of them), the rounds
// by lpu.
constexpr int SP_LANES = 1024;     // threads of a workgroup, and lanes of a unit, at the most
constexpr int SP_SATURATE = 1 << 30;  // above every unit's block count (201 M for 65535 x 65535 at 4:4:4)

struct pos_reader {
    const unsigned int *words;
    unsigned long long acc;  // the low `cnt` bits are the stream's next bits
    unsigned long long skp;  // beside acc: the last bit of a data byte FF that has a stuffed 00 behind it
    long long bp;            // bits from the unit's first byte to the next unread bit, stuffed bytes counted: always on a data byte
    unsigned int w;
    int cnt, pos, end, widx;
    bool ff;
    __device__ __forceinline__ void refill() {
        while (cnt <= 56) {
            unsigned int b = 0;
            for (;;) {
                if (pos >= end) {  // past the unit: zeros
                    b = 0, ff = false;
                    break;
                }
                const int wi = pos >> 2;
                if (wi != widx) widx = wi, w = words[wi];
                b = (w >> (8 * (pos & 3))) & 0xFFu;
                ++pos;
                if (ff && b == 0) {  // FF 00 is the data byte FF: the FF is the newest byte in acc, whose last bit is never taken
                    ff = false;      // before the next refill (an element takes at most 31 of the 32 bits a refill leaves)
                    skp |= 1ull;
                    continue;
                }
                ff = b == 0xFFu;
                break;
            }
            acc = acc << 8 | b;
            skp <<= 8;
            cnt += 8;
        }
    }
    // At bit `at` of the unit [lo, hi) of the data; `at` rests on a data byte (or lies past the unit).
    __device__ __forceinline__ void start(const unsigned int *data, const int lo, const int hi, const long long at) {
        words = data, acc = 0, skp = 0, w = 0, cnt = 0, widx = -1, ff = false, bp = at, end = hi;
        pos = (at >> 3) < (long long)(hi - lo) ? lo + (int)(at >> 3) : hi;
        refill();
        cnt -= (int)(at & 7);
    }
    __device__ __forceinline__ void take(const int n) {  // 1 <= n <= 16 <= cnt
        const unsigned int m = (unsigned int)(skp >> (cnt - n)) & ((1u << n) - 1u);
        bp += n + 8 * __popc(m);
        cnt -= n;
    }
    // The next symbol of table t, or -1 where the next 16 bits start no code (they are consumed).  Leaves at least 16 bits in `acc`.
    __device__ __forceinline__ int symbol(const huff_lds &t) {
        if (cnt < 32) refill();
        const unsigned int p = (unsigned int)(acc >> (cnt - 16)) & 0xFFFFu;
        const unsigned int e = t.lut[p >> 8];
        if (e) {
            take((int)(e >> 8));
            return (int)(e & 255u);
        }
        for (int l = 9; l <= 16; ++l) {
            const int d = (int)(p >> (16 - l)) - t.first[l];
            if (d >= 0 && d < (int)t.nb[l]) {
                take(l);
                return t.vals[min(t.cum[l - 1] + d, 255)];
            }
        }
        take(16);
        return -1;
    }
    __device__ __forceinline__ int value(const int s) {  // s <= 15 bits behind a symbol, extended
        if (s == 0) return 0;
        const int v = (int)(acc >> (cnt - s)) & ((1 << s) - 1);
        take(s);
        return v >> (s - 1) ? v : v - (1 << s) + 1;
    }
};

// One element at zig-zag index idx of a block whose tables are dc / ac; false at an inconsistency (idx is then left as it was).
// k >= 0: coefficient k (zig-zag) has the value val, the DC difference for k = 0.  idx = 64: the block is done.
__device__ __forceinline__ bool element(pos_reader &rd, const huff_lds &dc, const huff_lds &ac, int &idx, int &k, int &val) {
    k = -1;
    if (idx == 0) {
        const int s = rd.symbol(dc);
        if (s < 0 || s > 15) return false;
        k = 0, val = rd.value(s), idx = 1;
        return true;
    }
    const int rs = rd.symbol(ac);
    if (rs < 0) return false;
    const int r = rs >> 4, sz = rs & 15;
    if (sz == 0) {
        if (r != 15) {  // EOB
            idx = 64;
            return true;
        }
        if (idx + 16 > 64) return false;
        idx += 16;  // ZRL
        return true;
    }
    if (idx + r > 63) return false;
    k = idx + r, val = rd.value(sz), idx = k + 1;
    return true;
}

__device__ __forceinline__ unsigned long long pack_state(const long long bp, const int slot, const int idx) {
    return (unsigned long long)bp << 9 | (unsigned int)(slot << 6 | idx);
}

// The other way, and what follows every element: a block that is done gives way to the next slot of the MCU (hv luma blocks, then
// one per chroma component; nslot in all).  (The component of a slot, slot < hv ? 0 : slot - hv + 1, stays at its three sites: as a
// function it changed the kernel's instruction selection; MEASUREMENTS.md, "JPEG decode: one entropy kernel".)
__device__ __forceinline__ void unpack_state(const unsigned long long state, int &slot, int &idx) {
    slot = (int)(state >> 6) & 7, idx = (int)state & 63;
}
__device__ __forceinline__ void next_slot_if_done(int &slot, int &idx, const int nslot) {
    if (idx == 64) idx = 0, slot = slot + 1 == nslot ? 0 : slot + 1;
}

// Inclusive sum over the lpu lanes of a unit (lpu a power of two, segments aligned to it), through s[blockDim]; SAT: saturating at
// SP_SATURATE (the operands are not negative), else modulo 2^32.  Every thread of the workgroup calls it; it ends behind a barrier.
template <bool SAT>
__device__ __forceinline__ unsigned int unit_inclusive_scan(const unsigned int v, unsigned int *s, const int jl, const int lpu) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < lpu; d <<= 1) {
        const unsigned int u = jl >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] = SAT ? min(s[t] + u, (unsigned int)SP_SATURATE) : s[t] + u;
        __syncthreads();
    }
    return s[t];
}

__global__ __launch_bounds__(SP_LANES) void jpeg_decode_split_kernel(const unsigned int *__restrict__ data, const int *__restrict__ meta,
                                                                     const unsigned char *__restrict__ sets, short *__restrict__ coef, const dec_geom g,
                                                                     const int split, const int lpu) {
    __shared__ huff_lds T[6];
    __shared__ unsigned char zig[64];
    __shared__ unsigned long long s_exit[SP_LANES];
    __shared__ unsigned int s_scan[SP_LANES];
    __shared__ int s_bad[SP_LANES], s_lim[SP_LANES];  // per unit of the workgroup: its first flagged lane; the blocks its DC sums cover
    const int t = threadIdx.x, f = blockIdx.y;
    const dec_meta mt(meta, g);
    build_tables(T, zig, mt.table_set(sets, g, f) + SET_QUANT, 2 * g.ncomp, t, (int)blockDim.x);

    const int ul = t / lpu, jl = t - ul * lpu;  // the unit within the workgroup, the lane within the unit
    const int u0 = mt.frame_unit[f], u1 = mt.frame_unit[f + 1];
    const long long k = (long long)blockIdx.x * ((int)blockDim.x / lpu) + ul;  // the unit within the frame
    const long long total = (long long)g.mx * g.my;
    const long long ri = mt.frame_ri[f] > 0 ? mt.frame_ri[f] : total;
    const long long m0 = k * ri;
    const bool unit_ok = u0 >= 0 && u1 <= g.n_units && k < (long long)u1 - u0 && m0 < total;
    const int hv = g.hs * g.vs, nslot = g.ncomp == 1 ? 1 : hv + 2;
    const int n_blocks = unit_ok ? (int)((min(m0 + ri, total) - m0) * nslot) : 0;
    int lo = 0, len = 0;
    if (unit_ok) {
        const int u = u0 + (int)k;
        lo = min(max(mt.unit_off[u], 0), g.data_bytes);
        len = min(max(mt.unit_off[u + 1], lo), g.data_bytes) - lo;
    }
    const int S = max(max(split, (len + lpu - 1) / lpu), 1);
    const int n_sub = max((len + S - 1) / S, 1);
    const bool active = unit_ok && jl < n_sub, last = jl == n_sub - 1;
    const long long end_bit = 8 * min((long long)(jl + 1) * S, (long long)len);
    short *cf = coef + (size_t)f * g.coef_frame;

    // ---- the rounds ----
    unsigned long long entry = 0, exit_state = 0;
    int begun = 0, bad_at = -1;
    if (active && jl > 0) {
        long long q = (long long)jl * S;  // < len
        const int i = lo + (int)q;
        const unsigned int b0 = (data[i >> 2] >> (8 * (i & 3))) & 0xFFu, b1 = (data[(i - 1) >> 2] >> (8 * ((i - 1) & 3))) & 0xFFu;
        if (b0 == 0 && b1 == 0xFFu) ++q;  // the 00 behind an FF is no data
        entry = pack_state(8 * q, 0, 0);
    }
    if (jl == 0) s_bad[ul] = 0x7FFFFFFF, s_lim[ul] = n_blocks;
    bool need = active;
    for (int r = 0;; ++r) {
        if (need) {
            pos_reader rd;
            rd.start(data, lo, lo + len, (long long)(entry >> 9));
            int slot, idx;
            unpack_state(entry, slot, idx);
            begun = 0, bad_at = -1;
            while (rd.bp < end_bit) {
                const int c = slot < hv ? 0 : slot - hv + 1;
                if (idx == 0) ++begun;
                int kk, val;
                if (!element(rd, T[2 * c], T[2 * c + 1], idx, kk, val)) {
                    if (bad_at < 0) bad_at = begun;
                    idx = 64;
                }
                next_slot_if_done(slot, idx, nslot);
            }
            exit_state = pack_state(rd.bp, slot, idx);
        }
        __syncthreads();  // every lane has read its neighbour's exit of the round before
        if (need) s_exit[t] = exit_state;
        const int any = __syncthreads_or(need);
        if ((r > 0 && !any) || r + 1 >= lpu) break;
        need = false;
        if (active && jl > 0 && s_exit[t - 1] != entry) entry = s_exit[t - 1], need = true;
    }

    // ---- positions, and where the unit ends ----
    const int prefix = (int)unit_inclusive_scan<true>(active ? (unsigned int)begun : 0u, s_scan, jl, lpu) - (active ? min(begun, SP_SATURATE) : 0);
    if (active && bad_at >= 0 && (long long)prefix + bad_at - 1 < n_blocks) atomicMin(&s_bad[ul], jl);
    __syncthreads();

    // ---- the write pass ----
    if (active && prefix <= n_blocks && jl <= s_bad[ul]) {
        pos_reader rd;
        rd.start(data, lo, lo + len, (long long)(entry >> 9));
        int slot, idx;
        unpack_state(entry, slot, idx);
        int n = 0, st = 0;  // blocks begun here
        short *dst = nullptr;
        auto block_at = [&](const int ordinal, const int sl) -> short * {
            const long long m = m0 + ordinal / nslot;
            const int mxi = (int)(m % g.mx), myi = (int)(m / g.mx);
            const int c = sl < hv ? 0 : sl - hv + 1, vy = c == 0 ? sl / g.hs : 0, vx = c == 0 ? sl - vy * g.hs : 0;
            return cf + g.block(c, mxi, myi, vy, vx) * 64;
        };
        if (idx > 0 && prefix > 0) dst = block_at(prefix - 1, slot);
        for (;;) {
            if (idx == 0 && prefix + n >= n_blocks) {  // the unit's blocks are done
                if (rd.bp > 8ll * len) st = A3D_JPEG_SHORT;
                break;
            }
            if (!last && rd.bp >= end_bit) break;
            if (idx == 0) dst = block_at(prefix + n, slot), ++n;
            const int c = slot < hv ? 0 : slot - hv + 1;
            const bool was_dc = idx == 0;
            int kk, val;
            if (!element(rd, T[2 * c], T[2 * c + 1], idx, kk, val)) {  // the unit's first inconsistency: the law ends the unit here
                st = rd.bp > 8ll * len ? A3D_JPEG_SHORT : A3D_JPEG_BAD_CODE;
                s_lim[ul] = prefix + n - (was_dc ? 1 : 0);  // the law keeps the DC value of a block whose DC symbol was sound
                break;
            }
            if (kk >= 0 && val != 0 && dst) dst[zig[kk]] = (short)val;
            next_slot_if_done(slot, idx, nslot);
        }
        if (st) atomicMax(reinterpret_cast<int *>(cf + g.cblk[3] * 64), st);
    }
    __syncthreads();  // the differences are in memory, s_lim is final

    // ---- the DC pass ----
    const int lim = unit_ok ? min(max(s_lim[ul], 0), n_blocks) : 0;
    for (int c = 0; c < g.ncomp; ++c) {
        const int hvc = g.h[c] * g.v[c], sb = c == 0 ? 0 : hv + c - 1;
        const long long n_c = (long long)(lim / nslot) * hvc + min(max(lim % nslot - sb, 0), hvc);  // the component's blocks in front of `lim`
        const long long per = (n_c + lpu - 1) / lpu, q0 = min(jl * per, n_c), q1 = min(q0 + per, n_c);
        auto dc_at = [&](const long long q) -> short * {
            const long long m = m0 + q / hvc;
            const int wi = (int)(q % hvc), vy = wi / g.h[c], vx = wi - vy * g.h[c];
            const int mxi = (int)(m % g.mx), myi = (int)(m / g.mx);
            return cf + g.block(c, mxi, myi, vy, vx) * 64;
        };
        unsigned int sum = 0;
        for (long long q = q0; q < q1; ++q) sum += (unsigned int)(int)*dc_at(q);
        unsigned int run = unit_inclusive_scan<false>(sum, s_scan, jl, lpu) - sum;
        for (long long q = q0; q < q1; ++q) {
            short *p = dc_at(q);
            run += (unsigned int)(int)*p;
            *p = (short)run;
        }
    }
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
        const uint2 qv = *reinterpret_cast<const uint2 *>(dec_meta(meta, g).table_set(sets, g, f) + c * 64 + r * 8);
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

extern "C" int a3d_jpeg_decode_split(const a3d_jpeg_decode_desc *d, int split_bytes, void *stream) {
    dec_geom g;
    if (!d || split_bytes < 1 || !make_geom(d->F, d->H, d->W, d->pitch, d->ncomp, d->hs, d->vs, &g)) return A3D_ERR_ARG;
    if (d->F == 0) return A3D_OK;
    if (d->F > 65535 || d->n_units < 1 || d->n_sets < 1 || d->data_bytes < 0 || d->data_bytes > 0x7FFFFFFFll) return A3D_ERR_ARG;
    if (!d->unit_off || !d->frame_unit || !d->frame_ri || !d->frame_set || !d->sets || !d->d_meta || !d->d_sets || !d->coef || !d->planes || !d->rgb ||
        !d->status || (!d->d_data && d->data_bytes > 0))
        return A3D_ERR_ARG;
    if ((uintptr_t)d->d_data % 4 || (uintptr_t)d->d_sets % 8 || (uintptr_t)d->coef % 16 || (uintptr_t)d->planes % 8) return A3D_ERR_ARG;
    if (d->unit_off[0] != 0 || d->unit_off[d->n_units] != d->data_bytes || d->frame_unit[0] != 0 || d->frame_unit[d->F] != d->n_units) return A3D_ERR_ARG;
    int longest = 0;
    for (int u = 0; u < d->n_units; ++u) {
        if (d->unit_off[u + 1] < d->unit_off[u]) return A3D_ERR_ARG;
        longest = d->unit_off[u + 1] - d->unit_off[u] > longest ? d->unit_off[u + 1] - d->unit_off[u] : longest;
    }
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
    const long long n_groups = (long long)d->F * d->H * groups, co_grid = (n_groups + 255) / 256;
    // The lanes of a unit are the power of two that gives the longest unit of the call subsequences of split_bytes, and a workgroup
    // is as many units of `lpu` lanes as the frame with the most units fills, 1024 threads at the most.
    int lpu = 1;
    while (lpu < SP_LANES && (long long)lpu * split_bytes < longest) lpu *= 2;
    const long long step = lpu > 64 ? lpu : 64, want = (most * lpu + step - 1) / step * step;
    const int threads = (int)(want < SP_LANES ? want : SP_LANES);
    const long long per_group = threads / lpu, en_grid = (most + per_group - 1) / per_group;
    if (id_grid > 0x7FFFFFFFll || co_grid > 0x7FFFFFFFll || en_grid > 0x7FFFFFFFll) return A3D_ERR_ARG;
    const int vec = (uintptr_t)d->rgb % 16 == 0 && ((size_t)d->pitch * 3) % 16 == 0;
    a3d_begin();
    if (hipMemsetAsync(d->coef, 0, (size_t)d->F * g.coef_frame * sizeof(short), (hipStream_t)stream) != hipSuccess) return A3D_ERR_LAUNCH;
    hipLaunchKernelGGL(jpeg_decode_split_kernel, dim3((unsigned int)en_grid, (unsigned int)d->F), dim3(threads), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned int *>(d->d_data), d->d_meta, d->d_sets, d->coef, g, split_bytes, lpu);
    hipLaunchKernelGGL(jpeg_decode_idct_kernel, dim3((unsigned int)id_grid), dim3(256), 0, (hipStream_t)stream, d->coef, d->d_meta, d->d_sets, d->planes,
                       g, n_blocks);
    hipLaunchKernelGGL(jpeg_decode_colour_kernel, dim3((unsigned int)co_grid), dim3(256), 0, (hipStream_t)stream, d->planes, d->coef, d->rgb, d->status, g,
                       n_groups, groups, vec);
    return a3d_check_launch();
}

extern "C" int a3d_jpeg_decode(const a3d_jpeg_decode_desc *d, void *stream) { return a3d_jpeg_decode_split(d, A3D_JPEG_SPLIT_BYTES, stream); }
