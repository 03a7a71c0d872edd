// The device primitives the conv kernels share: ONE definition of each piece of arithmetic and addressing that the bit-identity
// links between kernel forms (DESIGN.md sections 3 and 4) rest on.
#pragma once
#include "a3d_common.h"

typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

// ---- buffer addressing -------------------------------------------------------------------------------------------
__device__ __forceinline__ __amdgpu_buffer_rsrc_t a3d_rsrc(const void *p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}
// (base pointer and size pass through v_readfirstlane: they ARE wave-uniform, and saying so keeps the descriptor in SGPRs --
// otherwise hipcc wraps every buffer load of the unrolled loop in a waterfall loop)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t a3d_rsrc_uniform(const void *p, unsigned bytes) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    void *q = reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(q, 0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
__device__ __forceinline__ f32x4 a3d_load4(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ void a3d_dma16(__amdgpu_buffer_rsrc_t r, void *lds_dst, int voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void *)lds_dst, 16, voff, soff, 0, 0);
}
template <int N>
__device__ __forceinline__ void a3d_wait_vm() {
    __asm__ volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- operand splits (F = f32x4 / f32x8 with the matching 16-bit vector) ------------------------------------------------------
// An fp32 number is EXACTLY the sum of three bf16 numbers (x = hi + mid + lo: each split rounds to nearest even and the sign
// carries one bit, so 3 x 8 significand bits cover the 24 of fp32), and a bf16 x bf16 product is exact in fp32.
template <typename F, typename B>
__device__ __forceinline__ void a3d_split3(const F v, B &h, B &m, B &l) {
    h = __builtin_convertvector(v, B);
    const F r1 = v - __builtin_convertvector(h, F);
    m = __builtin_convertvector(r1, B);
    const F r2 = r1 - __builtin_convertvector(m, F);
    l = __builtin_convertvector(r2, B);
}
// fp16x2 mode (a3d_conv_desc.precision == 3): x * s = h + l with h, l fp16 and s a power of two that puts the tensor's largest
// magnitude in [2^14, 2^15): h carries 11 significant bits, l the next 11 (2^-22 relative wherever |x| >= max / 2^18, 2^-40 of the
// maximum below); h.h + h.l + l.h with fp32 accumulation drops only l.l (<= 2^-22 relative).  THREE MFMAs per k step.
template <typename F, typename H>
__device__ __forceinline__ void a3d_split2h(const F v, const float s, H &h, H &l) {
    const F xs = v * s;
    h = __builtin_convertvector(xs, H);
    const F r = xs - __builtin_convertvector(h, F);
    l = __builtin_convertvector(r, H);
}

// ---- row-major epilogue: the 32 x 32 tile turn ------------------------------------------------------------------------------------
// The MFMA leaves a lane with ONE pixel and register quads of 4 channels: stored as they are, a wave instruction touches 32 rows x
// 32 bytes (64 separate 16-byte requests, and the same again for the residual).  Each 32 x 32 tile therefore goes through 4 KiB of
// LDS (quad index XOR-swizzled with the row: conflict-free both ways) and comes back with 8 lanes per row: a wave instruction then
// covers 8 rows x 128 contiguous bytes (res2 1x1 64 -> 256 + residual: 0.79 -> 0.61 ms).  Same values, same operations per element:
// the stored bits do not change.
__device__ __forceinline__ void a3d_turn_put(float *T, const int row, const int quad, const f32x4 v) {
    *reinterpret_cast<f32x4 *>(T + row * 32 + ((quad ^ (row & 7)) << 2)) = v;
}
__device__ __forceinline__ f32x4 a3d_turn_get(const float *T, const int row, const int quad) {
    return *reinterpret_cast<const f32x4 *>(T + row * 32 + ((quad ^ (row & 7)) << 2));
}

// ---- per-image output maxima ------------------------------------------------------------------------------------------------------
// y_amax[b] = max(y_amax[b], v) for the lanes with `valid`; v >= 0.  One atomic per wave when the wave's valid lanes share b (the
// rule: 32 consecutive pixels of one image), and none at all once the slot already holds a larger value.
__device__ __forceinline__ void a3d_note_amax(float *y_amax, const int b, float v, const bool valid) {
    if (!valid) v = 0.f;
    const unsigned long long live = __ballot(valid);
    if (!live) return;
    const int b0 = __shfl(b, __ffsll((long long)live) - 1, 64);
    const bool uniform = __all(!valid || b == b0);
    if (uniform) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
        if ((threadIdx.x & 63) == 0 && v > y_amax[b0]) atomicMax(reinterpret_cast<int *>(y_amax + b0), __float_as_int(v));
    } else if (valid && v > y_amax[b]) {
        atomicMax(reinterpret_cast<int *>(y_amax + b), __float_as_int(v));
    }
}
// Maximum over the 8 lanes that share a row of a turned tile.
__device__ __forceinline__ float a3d_max8(float v) {
    v = fmaxf(v, __shfl_xor(v, 1, 64));
    v = fmaxf(v, __shfl_xor(v, 2, 64));
    v = fmaxf(v, __shfl_xor(v, 4, 64));
    return v;
}
// The maxima of a wave's 32 turned rows mb .. mb + 31 (vm[j]: the lane's maximum over row mb + qr + 8 j).  They go out ONCE per wave,
// behind its last store: an atomic on an image's slot queues behind every other workgroup's at the L2, and a wave that goes on to
// another N step would wait for it at its next counted vmcnt (measured: 0.97 -> 0.43 ms on the res2 64 -> 256 layer).  Rows of
// several images, e.g. the FC layers where every ROI is one: the 8 lanes of a row reduce first, so a row costs one pre-checked atomic
// per wave instead of eight.
__device__ __forceinline__ void a3d_note_rows(float *y_amax, const float (&vm)[4], const bool one_image, const int mb, const int M, const int hwo,
                                              const int qr, const int qc) {
    if (!y_amax) return;
    if (one_image) {
        a3d_note_amax(y_amax, mb / hwo, fmaxf(fmaxf(vm[0], vm[1]), fmaxf(vm[2], vm[3])), true);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = mb + qr + 8 * j;
            const float v = a3d_max8(vm[j]);
            a3d_note_amax(y_amax, m < M ? m / hwo : 0, v, m < M && qc == 0);
        }
    }
}
