// PNG decode (include/a3d.h, "PNG decode"): the deflate bodies of F PNG frames of one geometry -> uint8 [F,H,pitch,3] RGB.  Three launches:
//   png_inflate_kernel   one wave per frame.  The decode tables live in LDS (a 10-bit primary lookup per code; a longer code resolves
//                        through the canonical first / count / offset rows of its length), built by all 64 lanes from the block's code
//                        lengths.  Lane 0 walks the Huffman codes -- the serial chain -- and hands tokens over in batches of 64 through
//                        LDS; all lanes then place the literals and run the copies, each copy lane-parallel, the copies of a batch in
//                        order.  The last 32 768 bytes of output live in an LDS ring, so a copy never waits for global memory; every
//                        byte is also stored to `raw`, which this kernel never reads.
//   png_adler_kernel     one workgroup per frame: a = 1 + sum b_j, b = N + sum (N - j) b_j, both mod 65521, summed in any order.
//   png_unfilter_kernel  one wave per frame, bands of 64 rows in sequence: lane r owns row r of the band and reconstructs pixel t - r at
//                        step t; b and c arrive from lane r - 1 through a cross-lane move, a is the lane's own previous pixel.  Only the
//                        row above a band is read back (from `raw`, where the band before left its last row reconstructed).
// Integers only.  Every loop is bounded by the stream's bit count or by the raw size.
#include "kernel_prims.h"
#include "../../include/a3d.h"

namespace {

constexpr int WIN = 32768;   // the LDS ring: deflate's largest distance
constexpr int TB = 10;       // bits of a primary lookup
constexpr int BATCH = 64;    // tokens per hand-over: one per lane
constexpr int N_LIT = 288, N_DIST = 32;  // the fixed code's symbol counts (286, 287 and 30, 31 have codes and no meaning)

// A table entry: bits 0-3 the code's length, 4-7 the number of extra bits, 8-10 the kind, 16-31 the literal or the base value.
enum { K_LIT = 0, K_BASE = 1, K_EOB = 2, K_BAD = 3, K_LONG = 4, K_NONE = 5 };
constexpr unsigned int E_NONE = (K_NONE << 8) | 1u;  // a pattern no code matches (incomplete sets only): one bit, then BAD_CODE
constexpr unsigned int E_LONG = (K_LONG << 8);
// What the walking lane reports with a batch.
enum { EV_MORE = 0, EV_EOB = -1 };
// What the header of a block turns out to be.
enum { H_STORED = 0, H_FIXED = 1, H_DYNAMIC = 2, H_ERROR = 3 };
// ctl[] slots
enum { C_KIND = 0, C_FINAL, C_STATUS, C_SRC, C_N, C_NT, C_EV, C_P0, C_WORDS };

__device__ const unsigned short LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const unsigned char LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const unsigned short DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
                                                 6145, 8193, 12289, 16385, 24577};
__device__ const unsigned char DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__device__ const unsigned char CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct geom {
    int F, H, W, pitch, ch;
    unsigned int stride, raw_size;  // bytes of a filtered row, of a frame's rows
    size_t per;                     // bytes of a frame's scratch: the rows rounded up to 16, then 16 bytes (stored | computed Adler-32)
};

static bool make_geom(int F, int H, int W, int pitch, int ch, geom *g) {
    if (F < 0 || F > 65535 || H < 1 || W < 1 || ch < 1 || ch > 4 || pitch < W) return false;
    const unsigned long long stride = 1ull + (unsigned long long)W * ch, raw = stride * (unsigned long long)H;
    if (raw > 0x7FFFFFFFull) return false;
    *g = geom{F, H, W, pitch, ch, (unsigned int)stride, (unsigned int)raw, (size_t)((raw + 15) / 16 * 16 + 16)};
    return true;
}

// One wave: LDS traffic between its lanes needs the compiler to keep the order, nothing more (DS instructions of a wave run in order).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned int lit_entry(int s) {
    if (s < 256) return (K_LIT << 8) | ((unsigned int)s << 16);
    if (s == 256) return K_EOB << 8;
    if (s < 286) return (K_BASE << 8) | ((unsigned int)LEN_EXTRA[s - 257] << 4) | ((unsigned int)LEN_BASE[s - 257] << 16);
    return K_BAD << 8;
}
__device__ __forceinline__ unsigned int dist_entry(int s) {
    if (s < 30) return (K_BASE << 8) | ((unsigned int)DIST_EXTRA[s] << 4) | ((unsigned int)DIST_BASE[s] << 16);
    return K_BAD << 8;
}

// The tables of one code from its lengths, by all 64 lanes: tab[1 << TB] the primary lookup on the next TB bits of the stream; sorted[]
// the symbols' entries by (length, symbol); meta[l], meta[16 + l], meta[32 + l] the first code, the count and the offset into sorted[]
// of length l.  false: an illegal set by zlib's rule (over-subscribed, or incomplete with a code longer than one bit).
template <bool DIST>
__device__ bool build_code(const unsigned char *lens, unsigned int *tab, unsigned int *sorted, unsigned short *meta, const int lane) {
    constexpr int N = DIST ? N_DIST : N_LIT;
    int cnt[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int g = 0; g < (N + 63) / 64; ++g) {
        const int s = g * 64 + lane, l = s < N ? lens[s] : 0;
#pragma unroll
        for (int L = 1; L < 16; ++L) cnt[L] += __popcll(__ballot(l == L));
    }
    int left = 1, maxl = 0;
    bool over = false;
#pragma unroll
    for (int L = 1; L < 16; ++L) {
        left = 2 * left - cnt[L];
        over |= left < 0;
        if (cnt[L]) maxl = L;
    }
    if (over || (left > 0 && maxl > 1)) return false;
    int first[16], offs[16], code = 0, o = 0;
#pragma unroll
    for (int L = 1; L < 16; ++L) {
        code = (code + cnt[L - 1]) << 1;
        first[L] = code;
        offs[L] = o;
        o += cnt[L];
        if (lane == 0) {
            meta[L] = (unsigned short)code;
            meta[16 + L] = (unsigned short)cnt[L];
            meta[32 + L] = (unsigned short)offs[L];
        }
    }
    for (int i = lane; i < (1 << TB); i += 64) tab[i] = E_NONE;
    wave_sync();
    int run[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) run[l] = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int g = 0; g < (N + 63) / 64; ++g) {
        const int s = g * 64 + lane, l = s < N ? lens[s] : 0;
        int rank = 0, f = 0, at = 0;
#pragma unroll
        for (int L = 1; L < 16; ++L) {
            const unsigned long long m = __ballot(l == L);
            if (l == L) {
                rank = run[L] + __popcll(m & below);
                f = first[L];
                at = offs[L];
            }
            run[L] += __popcll(m);
        }
        if (l > 0) {
            const unsigned int e = (DIST ? dist_entry(s) : lit_entry(s)) | (unsigned int)l;
            sorted[at + rank] = e;
            const unsigned int rev = __brev((unsigned int)(f + rank)) >> (32 - l);
            if (l <= TB) {
                for (unsigned int k = rev; k < (1u << TB); k += 1u << l) tab[k] = e;
            } else {
                tab[rev & ((1u << TB) - 1u)] = E_LONG;
            }
        }
    }
    wave_sync();
    return true;
}

// A code longer than TB bits, from the next 15 bits of the stream: the canonical walk over the lengths TB + 1 .. 15.
__device__ __forceinline__ unsigned int long_lookup(const unsigned int b15, const unsigned short *meta, const unsigned int *sorted) {
    const unsigned int r = __brev(b15) >> 17;  // the 15 bits, the first of the stream on top
    for (int len = TB + 1; len <= 15; ++len) {
        const unsigned int d = (r >> (15 - len)) - meta[len];
        if (d < meta[16 + len]) return sorted[meta[32 + len] + d];
    }
    return E_NONE;
}

// The walking lane's view of a frame's bytes [start, end) of the blob: a 64-bit window refilled by aligned words, the next word always
// in flight.  Bytes outside the frame read as zero and are never consumed: every consumer checks rem() first.
struct bit_reader {
    const unsigned int *words;
    unsigned int start, end;  // byte offsets in the blob
    unsigned long long buf, pos, nbits;
    int cnt;
    unsigned int wi, nxt;

    __device__ __forceinline__ unsigned int fetch(const unsigned int w) const {
        const unsigned long long a = 4ull * w;
        if (a >= end) return 0u;
        unsigned int v = words[w];
        if (end - a < 4) v &= (1u << (8 * (unsigned int)(end - a))) - 1u;
        return v;
    }
    __device__ __forceinline__ void seek(const unsigned long long byte) {  // byte <= end - start
        const unsigned long long at = start + byte;
        wi = (unsigned int)(at >> 2);
        const int sh = 8 * (int)(at & 3);
        buf = (unsigned long long)(fetch(wi) >> sh);
        cnt = 32 - sh;
        nxt = fetch(++wi);
        pos = 8 * byte;
    }
    __device__ __forceinline__ void refill() {  // afterwards at least 33 bits are in the window
        if (cnt <= 32) {
            buf |= (unsigned long long)nxt << cnt;
            cnt += 32;
            nxt = fetch(++wi);
        }
    }
    __device__ __forceinline__ unsigned long long rem() const { return nbits - pos; }
    __device__ __forceinline__ unsigned int peek(const int n) const { return (unsigned int)buf & ((1u << n) - 1u); }
    __device__ __forceinline__ void drop(const int n) {
        buf >>= n;
        cnt -= n;
        pos += n;
    }
};

struct inflate_lds {
    unsigned char win[WIN];
    unsigned int lit_tab[1 << TB], dist_tab[1 << TB];
    unsigned int lit_sorted[N_LIT], dist_sorted[N_DIST];
    unsigned short lit_meta[48], dist_meta[48];
    unsigned int tok[BATCH];
    int ctl[C_WORDS];
    unsigned char lens[N_LIT + N_DIST];
    unsigned char cl_tab[128];  // the code-length code: symbol | length << 5 on the next 7 bits
    unsigned char cl_len[19];
    unsigned short cl_cnt[8], cl_first[8];  // the walking lane's, in LDS: indexed by a length
};

// Lane 0: the header of a dynamic block after its three first bits -> lens[] (zero-filled by the caller).  0 or the status.
__device__ int dynamic_header(bit_reader &rd, inflate_lds &s) {
    rd.refill();
    if (rd.rem() < 14) return A3D_PNGD_SHORT;
    const int hlit = (int)rd.peek(5) + 257;
    rd.drop(5);
    const int hdist = (int)rd.peek(5) + 1;
    rd.drop(5);
    const int hclen = (int)rd.peek(4) + 4;
    rd.drop(4);
    if (hlit > 286 || hdist > 30) return A3D_PNGD_BAD_CODE;
    for (int i = 0; i < 19; ++i) s.cl_len[i] = 0;
    for (int i = 0; i < hclen; ++i) {
        rd.refill();
        if (rd.rem() < 3) return A3D_PNGD_SHORT;
        s.cl_len[CL_ORDER[i]] = (unsigned char)rd.peek(3);
        rd.drop(3);
    }
    for (int l = 0; l < 8; ++l) s.cl_cnt[l] = 0;
    for (int i = 0; i < 19; ++i) s.cl_cnt[s.cl_len[i]] += 1;
    s.cl_cnt[0] = 0;
    int left = 1, code = 0;
    for (int l = 1; l < 8; ++l) {
        left = 2 * left - s.cl_cnt[l];
        if (left < 0) return A3D_PNGD_BAD_CODE;
        code = (code + s.cl_cnt[l - 1]) << 1;
        s.cl_first[l] = (unsigned short)code;
    }
    if (left != 0) return A3D_PNGD_BAD_CODE;  // the code-length code is complete or illegal
    for (int sym = 0; sym < 19; ++sym) {
        const int l = s.cl_len[sym];
        if (!l) continue;
        const unsigned int rev = __brev((unsigned int)s.cl_first[l]) >> (32 - l);
        s.cl_first[l] += 1;
        for (unsigned int k = rev; k < 128u; k += 1u << l) s.cl_tab[k] = (unsigned char)(sym | l << 5);
    }
    int have = 0, prev = 0;
    const int want = hlit + hdist;
    while (have < want) {
        rd.refill();
        const unsigned int e = s.cl_tab[rd.peek(7)];
        const int l = (int)(e >> 5), sym = (int)(e & 31);
        if ((unsigned long long)l > rd.rem()) return A3D_PNGD_SHORT;
        rd.drop(l);
        int rep = 1, val = sym;
        if (sym >= 16) {
            const int x = sym == 16 ? 2 : (sym == 17 ? 3 : 7);
            if ((unsigned long long)x > rd.rem()) return A3D_PNGD_SHORT;
            rep = (int)rd.peek(x) + (sym == 18 ? 11 : 3);
            rd.drop(x);
            if (sym == 16 && have == 0) return A3D_PNGD_BAD_CODE;
            if (have + rep > want) return A3D_PNGD_BAD_CODE;
            val = sym == 16 ? prev : 0;
        }
        for (int k = 0; k < rep; ++k, ++have) s.lens[have < hlit ? have : N_LIT + have - hlit] = (unsigned char)val;
        prev = val;
    }
    return s.lens[256] ? 0 : A3D_PNGD_BAD_CODE;
}

__global__ void __launch_bounds__(64) png_inflate_kernel(const unsigned char *__restrict__ data, const int *__restrict__ frame_off, const long long data_bytes,
                                                         unsigned char *__restrict__ raw_all, int *__restrict__ status, const geom g) {
    __shared__ inflate_lds s;
    const int f = blockIdx.x, lane = threadIdx.x;
    unsigned char *raw = raw_all + (size_t)f * g.per;
    // whatever the device copy of the offsets holds, the frame's bytes lie inside the blob
    long long lo = frame_off[f], hi = frame_off[f + 1];
    lo = lo < 0 ? 0 : (lo > data_bytes ? data_bytes : lo);
    hi = hi < lo ? lo : (hi > data_bytes ? data_bytes : hi);
    bit_reader rd;
    rd.words = reinterpret_cast<const unsigned int *>(data);
    rd.start = (unsigned int)lo;
    rd.end = (unsigned int)hi;
    rd.nbits = 8ull * (unsigned long long)(hi - lo);
    rd.seek(0);
    const unsigned int raw_size = g.raw_size;
    unsigned int opos = 0;  // bytes of output so far (the walking lane's count)
    int st = 0;
    for (bool final = false; !final;) {
        if (lane == 0) {
            int kind = H_ERROR, err = 0;
            rd.refill();
            if (rd.rem() < 3) {
                err = A3D_PNGD_SHORT;
            } else {
                s.ctl[C_FINAL] = (int)rd.peek(1);
                rd.drop(1);
                const int btype = (int)rd.peek(2);
                rd.drop(2);
                if (btype == 3) {
                    err = A3D_PNGD_BAD_CODE;
                } else if (btype == 0) {
                    rd.drop((int)(-(long long)rd.pos & 7));
                    rd.refill();
                    if (rd.rem() < 32) {
                        err = A3D_PNGD_SHORT;
                    } else {
                        const unsigned int n = rd.peek(16), inv = (unsigned int)(rd.buf >> 16) & 0xFFFFu;
                        rd.drop(32);
                        const unsigned long long at = rd.pos >> 3, have = (rd.nbits >> 3) - at;
                        const unsigned int fits = have < n ? (unsigned int)have : n;
                        if (n != (inv ^ 0xFFFFu)) err = A3D_PNGD_BAD_CODE;
                        else if (opos + fits > raw_size) err = A3D_PNGD_LONG;
                        else if (have < n) err = A3D_PNGD_SHORT;
                        else {
                            kind = H_STORED;
                            s.ctl[C_SRC] = (int)at;
                            s.ctl[C_N] = (int)n;
                            s.ctl[C_P0] = (int)opos;
                            opos += n;
                            rd.seek(at + n);
                        }
                    }
                } else {
                    kind = btype;
                }
            }
            s.ctl[C_KIND] = kind;
            s.ctl[C_STATUS] = err;
        }
        wave_sync();
        int kind = __builtin_amdgcn_readfirstlane(s.ctl[C_KIND]);
        final = __builtin_amdgcn_readfirstlane(s.ctl[C_FINAL]) != 0;
        if (kind == H_ERROR) {
            st = __builtin_amdgcn_readfirstlane(s.ctl[C_STATUS]);
            break;
        }
        if (kind == H_STORED) {  // a cooperative copy: [src, src + n) lies inside the frame's bytes, [p0, p0 + n) inside raw
            const unsigned int src = rd.start + (unsigned int)s.ctl[C_SRC], n = (unsigned int)s.ctl[C_N], p0 = (unsigned int)s.ctl[C_P0];
            for (unsigned int k = lane; k < n; k += 64) {
                const unsigned char b = data[src + k];
                s.win[(p0 + k) & (WIN - 1)] = b;
                raw[p0 + k] = b;
            }
            wave_sync();
            continue;
        }
        for (int i = lane; i < N_LIT + N_DIST; i += 64) s.lens[i] = kind == H_FIXED ? (i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < N_LIT ? 8 : 5) : 0;
        wave_sync();
        if (kind == H_DYNAMIC) {
            if (lane == 0) s.ctl[C_STATUS] = dynamic_header(rd, s);
            wave_sync();
            st = __builtin_amdgcn_readfirstlane(s.ctl[C_STATUS]);
            if (st) break;
        }
        const bool ok_lit = build_code<false>(s.lens, s.lit_tab, s.lit_sorted, s.lit_meta, lane);
        const bool ok_dist = build_code<true>(s.lens + N_LIT, s.dist_tab, s.dist_sorted, s.dist_meta, lane);
        if (!ok_lit || !ok_dist) {
            st = A3D_PNGD_BAD_CODE;
            break;
        }
        int ev = EV_MORE;
        while (ev == EV_MORE) {
            if (lane == 0) {  // the serial chain: up to BATCH tokens, each checked against the stream's end and the output's
                int nt = 0, e_out = EV_MORE;
                s.ctl[C_P0] = (int)opos;
                while (nt < BATCH) {
                    rd.refill();
                    unsigned int e = s.lit_tab[rd.peek(TB)];
                    if (((e >> 8) & 7) == K_LONG) e = long_lookup(rd.peek(15), s.lit_meta, s.lit_sorted);
                    int l = (int)(e & 15), k = (int)((e >> 8) & 7);
                    if ((unsigned long long)l > rd.rem()) { e_out = A3D_PNGD_SHORT; break; }
                    if (k == K_NONE) { e_out = A3D_PNGD_BAD_CODE; break; }
                    rd.drop(l);
                    if (k == K_LIT) {
                        if (opos >= raw_size) { e_out = A3D_PNGD_LONG; break; }
                        s.tok[nt++] = e >> 16;
                        opos += 1;
                        continue;
                    }
                    if (k == K_EOB) { e_out = EV_EOB; break; }
                    if (k == K_BAD) { e_out = A3D_PNGD_BAD_CODE; break; }
                    int x = (int)((e >> 4) & 15);
                    if ((unsigned long long)x > rd.rem()) { e_out = A3D_PNGD_SHORT; break; }
                    const unsigned int len = (e >> 16) + rd.peek(x);
                    rd.drop(x);
                    rd.refill();
                    e = s.dist_tab[rd.peek(TB)];
                    if (((e >> 8) & 7) == K_LONG) e = long_lookup(rd.peek(15), s.dist_meta, s.dist_sorted);
                    l = (int)(e & 15), k = (int)((e >> 8) & 7);
                    if ((unsigned long long)l > rd.rem()) { e_out = A3D_PNGD_SHORT; break; }
                    if (k != K_BASE) { e_out = A3D_PNGD_BAD_CODE; break; }
                    rd.drop(l);
                    x = (int)((e >> 4) & 15);
                    if ((unsigned long long)x > rd.rem()) { e_out = A3D_PNGD_SHORT; break; }
                    const unsigned int d = (e >> 16) + rd.peek(x);
                    rd.drop(x);
                    if (d > opos) { e_out = A3D_PNGD_FAR; break; }
                    if (opos + len > raw_size) { e_out = A3D_PNGD_LONG; break; }
                    s.tok[nt++] = len | d << 9;
                    opos += len;
                }
                s.ctl[C_NT] = nt;
                s.ctl[C_EV] = e_out;
            }
            wave_sync();
            const int nt = __builtin_amdgcn_readfirstlane(s.ctl[C_NT]);
            ev = __builtin_amdgcn_readfirstlane(s.ctl[C_EV]);
            const unsigned int p0 = (unsigned int)__builtin_amdgcn_readfirstlane(s.ctl[C_P0]);
            // all lanes: lane i takes token i.  1 <= d <= pos and pos + len <= raw_size hold for every token (the walking lane checked).
            const unsigned int t = lane < nt ? s.tok[lane] : 0u;
            const bool is_copy = lane < nt && (t >> 9) != 0u;
            const unsigned int mylen = lane < nt ? (is_copy ? (t & 511u) : 1u) : 0u;
            const unsigned int pos = p0 + a3d_wave_inclusive_scan(mylen) - mylen;
            bool lit_waits = lane < nt && !is_copy;
            for (unsigned long long m = __ballot(is_copy); m; m &= m - 1) {
                const int i = __ffsll((long long)m) - 1;
                if (lit_waits && lane < i) {  // the literals in front of this copy: a later one may land on a ring slot this copy still reads
                    s.win[pos & (WIN - 1)] = (unsigned char)t;
                    raw[pos] = (unsigned char)t;
                    lit_waits = false;
                }
                const unsigned int tt = __shfl(t, i), p = __shfl(pos, i), len = tt & 511u, d = tt >> 9;
                for (unsigned int k = lane; k < len; k += 64) {  // ascending passes, a pass reads before it writes
                    const unsigned int src = p - d + (d < len ? k % d : k);
                    const unsigned char b = s.win[src & (WIN - 1)];
                    s.win[(p + k) & (WIN - 1)] = b;
                    raw[p + k] = b;
                }
            }
            if (lit_waits) {
                s.win[pos & (WIN - 1)] = (unsigned char)t;
                raw[pos] = (unsigned char)t;
            }
            wave_sync();
        }
        if (ev > 0) {
            st = ev;
            break;
        }
    }
    if (lane == 0) {
        unsigned int stored = 0;
        if (st == 0) {
            if (opos < raw_size) {
                st = A3D_PNGD_SHORT;
            } else {
                rd.refill();
                rd.drop((int)(-(long long)rd.pos & 7));
                rd.refill();
                if (rd.rem() < 32) st = A3D_PNGD_SHORT;
                else stored = __builtin_bswap32(rd.peek(16) | ((unsigned int)(rd.buf >> 16) & 0xFFFFu) << 16);
            }
        }
        reinterpret_cast<unsigned int *>(raw + (g.per - 16))[0] = stored;
        status[f] = st;
    }
}

// Adler-32 of a frame's raw bytes -> word 1 of the frame's 16-byte tail.  Thread-strided 16-byte loads; a vector at byte j0 adds
// sum b_i to s1 and ((N - j0) mod 65521 + 65521) sum b_i - sum i b_i to s2, which is sum (N - j0 - i) b_i mod 65521 and never negative.
__global__ void __launch_bounds__(1024) png_adler_kernel(unsigned char *__restrict__ raw_all, const geom g) {
    __shared__ unsigned long long r1[1024], r2[1024];
    unsigned char *raw = raw_all + (size_t)blockIdx.x * g.per;
    const unsigned int N = g.raw_size, nvec = (N + 15) / 16;
    unsigned long long s1 = 0, s2 = 0;
    for (unsigned int v = threadIdx.x; v < nvec; v += 1024) {
        const uint4 q = reinterpret_cast<const uint4 *>(raw)[v];
        const unsigned int w[4] = {q.x, q.y, q.z, q.w}, j0 = 16 * v;
        unsigned int sum = 0, wsum = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const unsigned int b = j0 + i < N ? (w[i >> 2] >> (8 * (i & 3))) & 255u : 0u;
            sum += b;
            wsum += i * b;
        }
        s1 += sum;
        s2 += (unsigned long long)((N - j0) % 65521u + 65521u) * sum - wsum;
    }
    r1[threadIdx.x] = s1;
    r2[threadIdx.x] = s2;
    __syncthreads();
    a3d_lds_tree<1024>(r1, r2);
    if (threadIdx.x == 0) {
        const unsigned int a = (unsigned int)((1ull + r1[0]) % 65521ull), b = (unsigned int)((N % 65521u + r2[0] % 65521ull) % 65521ull);
        reinterpret_cast<unsigned int *>(raw + (g.per - 16))[1] = b << 16 | a;
    }
}

// A lane's window on one row of raw: aligned 16-byte blocks staged through 64 bytes of LDS, the next block always in flight.
struct row_queue {
    unsigned char *lds;  // this lane's 64 bytes, 16-byte aligned
    const uint4 *blk;
    unsigned int last, pq;  // the last block that may be read; the block `pend` holds
    uint4 pend;
    __device__ __forceinline__ uint4 ld(const unsigned int q) const { return blk[q < last ? q : last]; }
    __device__ __forceinline__ void st(const unsigned int q, const uint4 v) { *reinterpret_cast<uint4 *>(lds + 16 * (q & 3)) = v; }
    __device__ __forceinline__ void init(const unsigned int o) {
        const unsigned int q = o >> 4;
        st(q, ld(q));
        st(q + 1, ld(q + 1));
        pq = q + 2;
        pend = ld(pq);
    }
    __device__ __forceinline__ void reach(const unsigned int o_last) {  // called with offsets that grow by at most 16 a call
        if (((o_last + 16) >> 4) >= pq) {
            st(pq, pend);
            pq += 1;
            pend = ld(pq);
        }
    }
    template <int CH>
    __device__ __forceinline__ unsigned int pixel(const unsigned int o) const {
        unsigned int v = 0;
#pragma unroll
        for (int i = 0; i < CH; ++i) v |= (unsigned int)lds[(o + i) & 63] << (8 * i);
        return v;
    }
};

__device__ __forceinline__ unsigned int paeth(const int a, const int b, const int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (unsigned int)(pa <= pb && pa <= pc ? a : (pb <= pc ? b : c));
}

template <int CH>
__global__ void __launch_bounds__(64) png_unfilter_kernel(unsigned char *__restrict__ raw_all, unsigned char *__restrict__ rgb, int *__restrict__ status,
                                                          const geom g) {
    __shared__ __attribute__((aligned(16))) unsigned char rows[64 * 64];
    __shared__ __attribute__((aligned(16))) unsigned char above_row[64];
    const int f = blockIdx.x, lane = threadIdx.x, H = g.H, W = g.W;
    unsigned char *raw = raw_all + (size_t)f * g.per;
    row_queue own, above;
    own.lds = rows + 64 * lane;
    above.lds = above_row;
    own.blk = above.blk = reinterpret_cast<const uint4 *>(raw);
    own.last = above.last = (g.raw_size + 15) / 16 - 1;
    bool bad = false;
    for (int y0 = 0; y0 < H; y0 += 64) {
        const int y = y0 + lane;
        const bool row_ok = y < H, from_above = lane == 0 && y0 > 0, keep = lane == 63 && y + 1 < H;
        const unsigned int o_row = row_ok ? (unsigned int)y * g.stride + 1u : 0u;  // the row's first sample
        int type = 0;
        if (row_ok) {
            type = raw[o_row - 1];
            if (type > 4) bad = true, type = 0;
            own.init(o_row);
        }
        if (from_above) above.init(o_row - g.stride);
        unsigned int outp = 0, bprev = 0;
        const int steps = W + (H - y0 < 64 ? H - y0 : 64) - 1;
        for (int t = 0; t < steps; ++t) {
            unsigned int up = __shfl_up(outp, 1);
            const int x = t - lane;
            if (row_ok && x >= 0 && x < W) {
                const unsigned int o = o_row + (unsigned int)x * CH;
                if (from_above) {
                    above.reach(o - g.stride + CH - 1);
                    up = above.pixel<CH>(o - g.stride);
                } else if (lane == 0) {
                    up = 0;
                }
                own.reach(o + CH - 1);
                const unsigned int px = own.pixel<CH>(o), a = x > 0 ? outp : 0u, c = x > 0 ? bprev : 0u;
                unsigned int out = 0;
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int ai = (a >> (8 * i)) & 255, bi = (up >> (8 * i)) & 255, ci = (c >> (8 * i)) & 255;
                    const unsigned int pred = type == 0 ? 0u : type == 1 ? (unsigned int)ai : type == 2 ? (unsigned int)bi : type == 3 ? (unsigned int)((ai + bi) >> 1) : paeth(ai, bi, ci);
                    out |= ((((px >> (8 * i)) & 255u) + pred) & 255u) << (8 * i);
                }
                unsigned char *dst = rgb + (((size_t)f * H + y) * g.pitch + x) * 3;
                dst[0] = (unsigned char)out;
                dst[1] = (unsigned char)(CH <= 2 ? out : out >> 8);
                dst[2] = (unsigned char)(CH <= 2 ? out : out >> 16);
                if (keep) {  // the band's last row, reconstructed, for the band below
#pragma unroll
                    for (int i = 0; i < CH; ++i) raw[o + i] = (unsigned char)(out >> (8 * i));
                }
                bprev = up;
                outp = out;
            }
        }
        __threadfence_block();
        __syncthreads();
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0 && status[f] == 0) {
        const unsigned int *tail = reinterpret_cast<const unsigned int *>(raw + (g.per - 16));
        status[f] = any_bad ? A3D_PNGD_FILTER : (tail[0] != tail[1] ? A3D_PNGD_ADLER : 0);
    }
}

}  // namespace

extern "C" int a3d_png_decode_scratch(int H, int W, int channels, size_t *raw_bytes) {
    geom g;
    if (!raw_bytes || !make_geom(0, H, W, W, channels, &g)) return A3D_ERR_ARG;
    *raw_bytes = g.per;
    return A3D_OK;
}

extern "C" int a3d_png_decode(const a3d_png_decode_desc *d, void *stream) {
    geom g;
    if (!d || !make_geom(d->F, d->H, d->W, d->pitch, d->channels, &g)) return A3D_ERR_ARG;
    if (d->F == 0) return A3D_OK;
    if (!d->frame_off || !d->d_data || !d->d_frame_off || !d->raw || !d->rgb || !d->status) return A3D_ERR_ARG;
    if (((uintptr_t)d->d_data & 3) || ((uintptr_t)d->d_frame_off & 3) || ((uintptr_t)d->raw & 15) || ((uintptr_t)d->status & 3)) return A3D_ERR_ARG;
    if (d->data_bytes < 0 || d->data_bytes > 0x7FFFFFFFll || d->frame_off[0] != 0 || d->frame_off[d->F] != d->data_bytes) return A3D_ERR_ARG;
    for (int f = 0; f < d->F; ++f)
        if (d->frame_off[f + 1] < d->frame_off[f]) return A3D_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    a3d_begin();
    if (hipMemsetAsync(d->status, 0, sizeof(int) * (size_t)d->F, s) != hipSuccess) return A3D_ERR_LAUNCH;
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned int)d->F), dim3(64), 0, s, d->d_data, d->d_frame_off, d->data_bytes, d->raw, d->status, g);
    hipLaunchKernelGGL(png_adler_kernel, dim3((unsigned int)d->F), dim3(1024), 0, s, d->raw, g);
    const dim3 grid((unsigned int)d->F), block(64);
    switch (g.ch) {
    case 1: hipLaunchKernelGGL(png_unfilter_kernel<1>, grid, block, 0, s, d->raw, d->rgb, d->status, g); break;
    case 2: hipLaunchKernelGGL(png_unfilter_kernel<2>, grid, block, 0, s, d->raw, d->rgb, d->status, g); break;
    case 3: hipLaunchKernelGGL(png_unfilter_kernel<3>, grid, block, 0, s, d->raw, d->rgb, d->status, g); break;
    default: hipLaunchKernelGGL(png_unfilter_kernel<4>, grid, block, 0, s, d->raw, d->rgb, d->status, g); break;
    }
    return a3d_check_launch();
}
