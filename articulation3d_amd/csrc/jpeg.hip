// Baseline JPEG on the device (include/a3d.h, "Motion-JPEG"): every frame of a call becomes the entropy-coded data of a JFIF image
// with a restart interval of one MCU row, byte for byte what tests/mjpeg_ref.py writes.  Integer arithmetic only.
//
//   transform   32 MCUs per workgroup, 8 lanes per MCU.  Lane r loads row r of the MCU's 8 x 8 pixels once (edge replication is a
//               clamp of the pixel index), converts the colour and transforms the row of all three components; the rows meet the
//               columns through LDS (rows padded to 9 words: both the row-wise stores and the column-wise loads touch 32 distinct
//               banks per half wave); lane j then transforms column j, quantises, and drops the result at its zigzag place in an
//               LDS image of the workgroup's 32 x 3 blocks, which leaves for global memory as 16-byte stores.
//   entropy     one workgroup per segment (frame, MCU row), one lane per 8 x 8 block, 256 blocks per tile.  Per tile: the lanes
//               measure their blocks, a workgroup scan turns the lengths into bit offsets, the lanes OR their codes into a
//               big-endian bit image in LDS (whole words, so the OR is of disjoint bits and its order cannot matter), and the
//               image is read back four bytes per lane, a second scan over "bytes + 0xFF bytes" placing the stuffed output.
//               The bit cursor and the unfinished byte are carried from tile to tile.  A block's DC predictor is the DC
//               coefficient three blocks back, read directly: no scan.
//   pack        one workgroup scans the segment lengths (plus 2 bytes per RST marker) into offsets; once the host has sized the
//               destination, one workgroup per segment copies it to its place and appends its marker.
//
// The bound everything is sized by: a block is at most 9 + 11 bits of DC and 63 x (16 + 10) bits of AC = 1658 bits
// (A3D_JPEG_BLOCK_BITS).  The categories 11 / 10 follow from the transform: |X| <= 128, a row of C13 sums to at most 23168 in
// magnitude, so |T| <= 2896 and |F| <= 1024, reached by the DC term alone (an AC basis function has both signs and X <= +127 on one
// of them); the transform clamps to those ranges all the same, so the bound holds whatever the arithmetic above it does.  A tile
// of 256 blocks is therefore at most 7 carried bits + 256 * 1658 bits = 13265 words of LDS, and a segment of M MCUs at most
// ceil(3 M * 1658 / 8) bytes before and twice that after stuffing (the filled last byte included): a3d_jpeg_slot_bytes.
#include "kernel_prims.h"
#include "../../include/a3d.h"

namespace {

// ITU-T T.81 Annex K: K.1 / K.2 quantisation (natural order), K.3 - K.6 Huffman specifications in the order DC0, AC0, DC1, AC1
constexpr unsigned char K_QUANT[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr unsigned char K_BITS[4][16] = {
    {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr int K_NVALS[4] = {12, 162, 12, 162};
constexpr unsigned char K_VALS[4][A3D_JPEG_HUFF_VALS] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
     0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A,
     0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53,
     0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
     0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
     0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9,
     0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2,
     0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
     0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17,
     0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A,
     0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
     0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
     0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7,
     0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2,
     0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}};
// symbol -> code << 5 | length.  Per class (0 luma, 1 chroma): 16 DC entries, then 256 AC entries.  Unused symbols stay 0.
constexpr int LUT_CLASS = 16 + 256;
struct huff_lut {
    unsigned int e[2 * LUT_CLASS];
};
constexpr huff_lut make_lut() {
    huff_lut l = {};
    for (int t = 0; t < 4; ++t) {  // Annex C: codes of one length are consecutive, the next length starts at twice the next code
        const int base = (t >> 1) * LUT_CLASS + (t & 1) * 16;
        unsigned int code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < K_BITS[t][len - 1]; ++i) l.e[base + K_VALS[t][k++]] = code++ << 5 | (unsigned int)len;
            code <<= 1;
        }
    }
    return l;
}
__device__ const huff_lut k_lut = make_lut();
// k_unzig[n] = place in zigzag order of the coefficient at natural (row-major) index n
__device__ const unsigned char k_unzig[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                              10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

struct quant_arg {
    unsigned char q[2][64];  // natural order, 1 .. 255
};

int scaled_quant(int quality, quant_arg *out) {
    if (quality < 1 || quality > 100) return A3D_ERR_ARG;
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = (K_QUANT[t][i] * s + 50) / 100;
            out->q[t][i] = (unsigned char)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
    return A3D_OK;
}

// y = C13 x, the 8-point DCT-II in 13-bit fixed point, through its even / odd halves: exact integers, so the same numbers as the matrix
__device__ __forceinline__ void dct8(const int (&x)[8], int (&y)[8]) {
    const int s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const int d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    y[0] = 2896 * (s0 + s1 + s2 + s3);
    y[4] = 2896 * (s0 - s1 - s2 + s3);
    y[2] = 3784 * (s0 - s3) + 1567 * (s1 - s2);
    y[6] = 1567 * (s0 - s3) - 3784 * (s1 - s2);
    y[1] = 4017 * d0 + 3406 * d1 + 2276 * d2 + 799 * d3;
    y[3] = 3406 * d0 - 799 * d1 - 4017 * d2 - 2276 * d3;
    y[5] = 2276 * d0 - 4017 * d1 + 799 * d2 + 3406 * d3;
    y[7] = 799 * d0 - 2276 * d1 + 3406 * d2 - 4017 * d3;
}

constexpr int TR_MCUS = 32;  // MCUs per transform workgroup (8 lanes each)
constexpr int T_LD = 9;      // words per transformed row in LDS

__global__ __launch_bounds__(256) void jpeg_transform_kernel(const unsigned char *__restrict__ frames, short *__restrict__ coef, const quant_arg qa,
                                                             const long long n_mcus, const int H, const int W, const int pitch, const int rows,
                                                             const int mcus, const int vec) {
    __shared__ int sT[TR_MCUS * 3 * 8 * T_LD];
    __shared__ __attribute__((aligned(16))) short sQ[TR_MCUS * 3 * 64];
    __shared__ unsigned char sq[2][64];
    const int tid = threadIdx.x, m = tid >> 3, r = tid & 7;
    if (tid < 128) sq[tid >> 6][tid & 63] = qa.q[tid >> 6][tid & 63];
    const long long g0 = (long long)blockIdx.x * TR_MCUS, g = g0 + m;
    const bool live = g < n_mcus;
    if (live) {
        const long long seg = g / mcus;
        const int mcu = (int)(g - seg * mcus), row = (int)(seg % rows);
        const long long f = seg / rows;
        const int y = min(row * 8 + r, H - 1);
        const unsigned char *src = frames + ((size_t)f * H + y) * (size_t)pitch * 3;
        unsigned char px[24];
        if (vec && mcu * 8 + 8 <= W) {  // 24 bytes on an 8-byte boundary (the host checked the base and the row pitch)
            const uint2 *p = reinterpret_cast<const uint2 *>(src + (size_t)mcu * 24);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint2 v = p[i];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    px[i * 8 + b] = (unsigned char)(v.x >> (8 * b));
                    px[i * 8 + 4 + b] = (unsigned char)(v.y >> (8 * b));
                }
            }
        } else {
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const unsigned char *p = src + (size_t)min(mcu * 8 + n, W - 1) * 3;
                px[n * 3] = p[0], px[n * 3 + 1] = p[1], px[n * 3 + 2] = p[2];
            }
        }
        int x[3][8];
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int R = px[n * 3], G = px[n * 3 + 1], B = px[n * 3 + 2];
            x[0][n] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
            x[1][n] = ((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16) - 128;
            x[2][n] = ((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16) - 128;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int t[8];
            dct8(x[c], t);
#pragma unroll
            for (int k = 0; k < 8; ++k) sT[((m * 3 + c) * 8 + r) * T_LD + k] = (t[k] + (1 << 9)) >> 10;
        }
    }
    __syncthreads();
    if (live) {
        const int j = r;  // this lane's column
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int t[8], f[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) t[n] = sT[((m * 3 + c) * 8 + n) * T_LD + j];
            dct8(t, f);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int v = (f[k] + (1 << 15)) >> 16, nat = k * 8 + j;
                const int q = sq[c ? 1 : 0][nat];
                int a = (abs(v) + (q >> 1)) / q;
                a = min(a, nat == 0 && v < 0 ? 1024 : 1023);  // never taken (header comment); it makes the categories 11 / 10 unconditional
                sQ[(m * 3 + c) * 64 + k_unzig[nat]] = (short)(v < 0 ? -a : a);
            }
        }
    }
    __syncthreads();
    const long long left = n_mcus - g0;
    const int n16 = (int)(left < TR_MCUS ? left : TR_MCUS) * 24;  // 384 bytes per MCU
    uint4 *dst = reinterpret_cast<uint4 *>(coef + (size_t)g0 * 192);
    for (int i = tid; i < n16; i += 256) dst[i] = reinterpret_cast<const uint4 *>(sQ)[i];
}

// exclusive scan of one int per lane over the 256-lane workgroup; `total` is the same in every lane.  s: 4 words of LDS, free again
// on return.
__device__ __forceinline__ int scan256(const int v, int *s, int &total) {
    const int excl = a3d_block_exclusive_scan<256>(v, s, total);
    __syncthreads();
    return excl;
}

constexpr int EN_TILE = 256;  // blocks per tile = lanes per workgroup
constexpr int EN_WORDS = (7 + EN_TILE * A3D_JPEG_BLOCK_BITS + 31) / 32 + 1;

// Appends `len` (<= 26) bits to a lane's stream.  acc / cnt: the bits not yet in LDS (cnt < 32 between calls); w: the word they go to.
struct bit_writer {
    unsigned long long acc;
    int cnt, w;
    unsigned int *img;
    __device__ __forceinline__ void put(const unsigned int code, const int len) {
        acc = acc << len | code;
        cnt += len;
        if (cnt >= 32) {
            cnt -= 32;
            if (w < EN_WORDS) atomicOr(&img[w], (unsigned int)(acc >> cnt));
            ++w;
        }
    }
    __device__ __forceinline__ void flush() {
        if (cnt > 0 && w < EN_WORDS) atomicOr(&img[w], (unsigned int)(acc << (32 - cnt)));
    }
};

// One block: its length in bits (EMIT = false) or its codes into the writer.  z: 64 coefficients in zigzag order, 16-byte aligned.
template <bool EMIT>
__device__ __forceinline__ int code_block(const short *__restrict__ z, const int pred, const unsigned int *lut, bit_writer &bw) {
    int bits = 0, run = 0;
    const uint4 *p = reinterpret_cast<const uint4 *>(z);
#pragma unroll 1
    for (int i = 0; i < 8; ++i) {
        const uint4 q = p[i];
        const unsigned int wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int v = (short)(wd[j >> 1] >> (16 * (j & 1)));
            const bool dc = i == 0 && j == 0;
            if (dc) v -= pred;
            if (v == 0 && !dc) {
                ++run;
                continue;
            }
            while (run > 15) {  // ZRL
                const unsigned int e = lut[16 + 0xF0];
                if (EMIT) bw.put(e >> 5, e & 31);
                bits += e & 31;
                run -= 16;
            }
            const int a = abs(v), cat = 32 - __clz(a);  // __clz(0) = 32
            const unsigned int e = dc ? lut[cat] : lut[16 + (run << 4 | cat)];
            const int len = (e & 31) + cat;
            if (EMIT) bw.put((e >> 5) << cat | (unsigned int)(v < 0 ? v + (1 << cat) - 1 : v), len);
            bits += len;
            run = 0;
        }
    }
    if (run) {  // EOB
        const unsigned int e = lut[16];
        if (EMIT) bw.put(e >> 5, e & 31);
        bits += e & 31;
    }
    return bits;
}

__global__ __launch_bounds__(256) void jpeg_entropy_kernel(const short *__restrict__ coef, unsigned char *__restrict__ slots, int *__restrict__ seg_len,
                                                           const int blocks, const unsigned int cap) {
    __shared__ unsigned int img[EN_WORDS];
    __shared__ unsigned int lut[2 * LUT_CLASS];
    __shared__ int ss[4];
    const int tid = threadIdx.x;
    const size_t seg = blockIdx.x;
    for (int i = tid; i < 2 * LUT_CLASS; i += 256) lut[i] = k_lut.e[i];
    __syncthreads();
    const short *zseg = coef + seg * (size_t)blocks * 64;
    unsigned char *out = slots + seg * (size_t)cap;
    unsigned int out_pos = 0, carry_val = 0;
    int carry_bits = 0;
    for (int t0 = 0; t0 < blocks; t0 += EN_TILE) {
        const int b = t0 + tid;
        const bool live = b < blocks;
        const unsigned int *my_lut = lut + (b % 3 ? LUT_CLASS : 0);
        const short *z = zseg + (size_t)b * 64;
        const int pred = live && b >= 3 ? z[-192] : 0;
        bit_writer bw = {0, 0, 0, img};
        const int len = live ? code_block<false>(z, pred, my_lut, bw) : 0;
        int tile_bits;
        const int off = carry_bits + scan256(len, ss, tile_bits);
        const int end_bits = carry_bits + tile_bits;  // <= 7 + 256 * 1658
        const int nwords = min((end_bits + 31) >> 5, EN_WORDS);
        for (int i = tid; i < nwords; i += 256) img[i] = i == 0 ? carry_val << 24 : 0u;
        __syncthreads();
        if (live) {
            bw.w = off >> 5, bw.cnt = off & 31;
            code_block<true>(z, pred, my_lut, bw);
            bw.flush();
        }
        __syncthreads();
        int nbytes = end_bits >> 3;
        const int rem = end_bits & 7;
        if (t0 + EN_TILE >= blocks) {  // the segment ends here: fill its last byte with 1-bits
            if (rem) {
                if (tid == 0) atomicOr(&img[nbytes >> 2], ((1u << (8 - rem)) - 1u) << (8 * (3 - (nbytes & 3))));
                ++nbytes;
                __syncthreads();
            }
        } else {  // the unfinished byte goes in front of the next tile
            carry_val = rem ? img[nbytes >> 2] >> (8 * (3 - (nbytes & 3))) & 0xFFu : 0u;
            carry_bits = rem;
        }
        for (int base = 0; base < nbytes; base += 1024) {  // four bytes per lane; every 0xFF takes a 0x00 behind it
            const int first = base + 4 * tid;
            const int nv = min(max(nbytes - first, 0), 4);
            const unsigned int w = nv > 0 ? img[first >> 2] : 0u;
            int need = nv;
#pragma unroll
            for (int k = 0; k < 4; ++k) need += k < nv && (w >> (24 - 8 * k) & 0xFFu) == 0xFFu;
            int total;
            unsigned int pos = out_pos + (unsigned int)scan256(need, ss, total);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) {
                    const unsigned int byte = w >> (24 - 8 * k) & 0xFFu;
                    if (pos < cap) out[pos] = (unsigned char)byte;
                    ++pos;
                    if (byte == 0xFFu) {
                        if (pos < cap) out[pos] = 0;
                        ++pos;
                    }
                }
            out_pos += (unsigned int)total;
        }
        __syncthreads();  // the image is rewritten by the next tile
    }
    if (tid == 0) seg_len[seg] = (int)min(out_pos, cap);
}

// seg_off[s] = bytes in front of segment s in the packed stream: every segment before it, plus 2 per RST marker (none after a frame's last
// segment).  frame_off[f] = seg_off[f * rows], frame_off[F] = the total.  One workgroup.
__global__ __launch_bounds__(256) void jpeg_offsets_kernel(const int *__restrict__ seg_len, int *__restrict__ seg_off, int *__restrict__ frame_off,
                                                           const int n_seg, const int rows) {
    __shared__ int ss[4];
    int base = 0;
    for (int s0 = 0; s0 < n_seg; s0 += 256) {
        const int s = s0 + threadIdx.x;
        const bool live = s < n_seg;
        const int need = live ? seg_len[s] + (s % rows == rows - 1 ? 0 : 2) : 0;
        int total;
        const int off = base + scan256(need, ss, total);
        if (live) {
            seg_off[s] = off;
            if (s % rows == 0) frame_off[s / rows] = off;
        }
        base += total;
    }
    if (threadIdx.x == 0) frame_off[n_seg / rows] = base;
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const unsigned char *__restrict__ slots, const int *__restrict__ seg_off, const int *__restrict__ seg_len,
                                                        unsigned char *__restrict__ packed, const long long packed_bytes, const int rows,
                                                        const unsigned int cap) {
    const size_t seg = blockIdx.x;
    const int row = (int)(seg % rows), len = seg_len[seg];
    const long long off = seg_off[seg];
    if (len < 0 || (unsigned int)len > cap || off < 0 || off + len + (row == rows - 1 ? 0 : 2) > packed_bytes) return;  // never past the destination
    const unsigned char *src = slots + seg * (size_t)cap;
    for (int i = threadIdx.x; i < len; i += 256) packed[off + i] = src[i];
    if (threadIdx.x == 0 && row != rows - 1) {
        packed[off + len] = 0xFF;
        packed[off + len + 1] = (unsigned char)(0xD0 + (row & 7));
    }
}

bool geometry_ok(int F, int H, int W) { return F >= 0 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535; }

}  // namespace

extern "C" int a3d_jpeg_tables(unsigned char *bits, unsigned char *vals) {
    if (!bits || !vals) return A3D_ERR_ARG;
    for (int t = 0; t < 4; ++t) {
        for (int i = 0; i < 16; ++i) bits[t * 16 + i] = K_BITS[t][i];
        for (int i = 0; i < A3D_JPEG_HUFF_VALS; ++i) vals[t * A3D_JPEG_HUFF_VALS + i] = i < K_NVALS[t] ? K_VALS[t][i] : 0;
    }
    return A3D_OK;
}

extern "C" int a3d_jpeg_quant(int quality, unsigned char *out) {
    quant_arg qa;
    if (!out || scaled_quant(quality, &qa) != A3D_OK) return A3D_ERR_ARG;
    for (int i = 0; i < 128; ++i) out[i] = qa.q[i >> 6][i & 63];
    return A3D_OK;
}

extern "C" size_t a3d_jpeg_slot_bytes(int W) {
    if (W < 1 || W > 65535) return 0;
    const size_t bits = (size_t)((W + 7) / 8) * 3 * A3D_JPEG_BLOCK_BITS;
    return (2 * ((bits + 7) / 8) + 15) / 16 * 16;
}

extern "C" int a3d_jpeg_encode(const unsigned char *frames, int F, int H, int W, int pitch, int quality, short *coef, unsigned char *slots,
                               int *seg_len, int *seg_off, int *frame_off, void *stream) {
    quant_arg qa;
    if (!geometry_ok(F, H, W) || pitch < W || scaled_quant(quality, &qa) != A3D_OK) return A3D_ERR_ARG;
    if (!frame_off || (F > 0 && (!frames || !coef || !slots || !seg_len || !seg_off)) || (uintptr_t)coef % 16 != 0) return A3D_ERR_ARG;
    const int rows = (H + 7) / 8, mcus = (W + 7) / 8;
    const size_t cap = a3d_jpeg_slot_bytes(W);
    const long long n_seg = (long long)F * rows;
    if (n_seg * (long long)(cap + 2) > 0x7FFFFFFFll) return A3D_ERR_ARG;  // offsets are int32: encode fewer frames per call
    a3d_begin();
    if (F > 0) {
        const long long n_mcus = n_seg * mcus;
        const int vec = (uintptr_t)frames % 8 == 0 && ((size_t)pitch * 3) % 8 == 0;
        hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned int)((n_mcus + TR_MCUS - 1) / TR_MCUS)), dim3(256), 0, (hipStream_t)stream, frames, coef,
                           qa, n_mcus, H, W, pitch, rows, mcus, vec);
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned int)n_seg), dim3(256), 0, (hipStream_t)stream, coef, slots, seg_len, mcus * 3,
                           (unsigned int)cap);
    }
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, seg_len, seg_off, frame_off, (int)n_seg, rows);
    return a3d_check_launch();
}

extern "C" int a3d_jpeg_pack(const unsigned char *slots, const int *seg_off, const int *seg_len, int F, int H, int W, unsigned char *packed,
                             long long packed_bytes, void *stream) {
    if (!geometry_ok(F, H, W) || packed_bytes < 0) return A3D_ERR_ARG;
    if (F == 0) return A3D_OK;
    if (!slots || !seg_off || !seg_len || (!packed && packed_bytes > 0)) return A3D_ERR_ARG;
    const int rows = (H + 7) / 8;
    const long long n_seg = (long long)F * rows;
    if (n_seg > 0x7FFFFFFFll) return A3D_ERR_ARG;
    a3d_begin();
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned int)n_seg), dim3(256), 0, (hipStream_t)stream, slots, seg_off, seg_len, packed, packed_bytes,
                       rows, (unsigned int)a3d_jpeg_slot_bytes(W));
    return a3d_check_launch();
}
