// mfma_dev.h -- what the dense-layer kernels share besides the GEMM parameters: vector types, the counted vector-memory wait, bf16 packing and
// the exact three-term split, the bf16 MFMA, the transposing LDS read and the bank swizzle of the 128-wide layers' LDS images (layer_*.hip,
// head_bf16.hip, narrow_stream.hip, gemm_split.hip, gemm_bf16.hip include this file in gemm_common.h's place).
// Everything here is static and force-inlined: moving a helper with an unchanged body into this file leaves every object's device listing
// (.isa/<name>.s) byte-identical, which is how such a move is checked ("Shared layer helpers").
#pragma once
#include "gemm_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// At most N of this wave's vector-memory instructions (loads, LDS-DMA, stores: they complete in order) may still be outstanding.  The kernels
// that issue their memory instructions by hand count them, so that a wait publishes one tile without draining the younger prefetches; the
// run-time "at most n" ladders on top of this stay in their files (each kernel has its own set of steps).
template <int N>
static __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Two fp32 -> one dword of packed bf16 (RNE), `lo` in the low half.  The two spellings are arithmetically the same, but they do not compile
// the same: swapping one for the other moves register allocation through the whole calling kernel (about 2,800 changed lines in
// layer_nb16's listing).  So both stay, and a caller keeps the one it was tuned and measured with.
static __device__ __forceinline__ unsigned pack_bf16_cast(float lo, float hi) {
    bf16x2 p;
    p[0] = (__bf16)lo; p[1] = (__bf16)hi;
    return __builtin_bit_cast(unsigned, p);
}
static __device__ __forceinline__ unsigned pack_bf16_bits(float lo, float hi) {
    return (unsigned)float_to_bf16_bits(lo) | ((unsigned)float_to_bf16_bits(hi) << 16);
}
// the halves of such a dword, widened back to fp32 (exact)
static __device__ __forceinline__ float bf16_lo(unsigned p) { return __uint_as_float(p << 16); }
static __device__ __forceinline__ float bf16_hi(unsigned p) { return __uint_as_float(p & 0xffff0000u); }
static __device__ __forceinline__ float bf16_pair_sum(unsigned u) { return __uint_as_float(u << 16) + __uint_as_float(u & 0xffff0000u); }

// exact three-way split of a pair (x = h + m + l, each term a bf16: 8 significant bits apiece, 24 together): h, m, l receive the packed
// (a, b) terms of the leading, middle and trailing plane -- the arithmetic of every fp32x6 kernel (layer_x6.hip has the derivation)
static __device__ __forceinline__ void split3_pair(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    h = pack_bf16_cast(a, b);
    const float ra = a - bf16_lo(h), rb = b - bf16_hi(h);
    m = pack_bf16_cast(ra, rb);
    const float sa = ra - bf16_lo(m), sb = rb - bf16_hi(m);
    l = pack_bf16_cast(sa, sb);
}

// one v_mfma_f32_32x32x16_bf16 on fragments held as four dwords; the kernels put the weight fragment first (swapped operands: a lane then
// owns one output row)
static __device__ __forceinline__ f32x16 mfma_bf16(const u32x4& w, const u32x4& a, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, a), c, 0, 0, 0);
}

static __device__ __forceinline__ bf16x8 cvt8(const float4 a, const float4 b) {
    bf16x8 r;
    r[0] = (__bf16)a.x; r[1] = (__bf16)a.y; r[2] = (__bf16)a.z; r[3] = (__bf16)a.w;
    r[4] = (__bf16)b.x; r[5] = (__bf16)b.y; r[6] = (__bf16)b.z; r[7] = (__bf16)b.w;
    return r;
}
static __device__ __forceinline__ unsigned keep_positive(unsigned v, unsigned mk) {      // per 16-bit half: v where the mask half is > 0
    const unsigned lo = bf16_bits_positive((unsigned short)(mk & 0xffffu)) ? 0x0000ffffu : 0u;
    const unsigned hi = bf16_bits_positive((unsigned short)(mk >> 16)) ? 0xffff0000u : 0u;
    return v & (lo | hi);
}

// Transposing LDS read: a 16-lane group reads a [4 m][16 col] block of bf16, lane q receives column q (two of these make the 8-m fragment of
// a weight-gradient MFMA).  Two forms, because they are different assembly text: the address in a register, or with its constant part in the
// instruction's offset field.
static __device__ __forceinline__ uint2 tr_read(unsigned addr) {
    uint2 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(addr) : "memory");
    return r;
}
template <int OFF>
static __device__ __forceinline__ uint2 tr_read_off(unsigned addr) {
    static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
    uint2 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
    return r;
}

// Bank swizzle of the 128-wide layers' bf16 LDS images (layer_nb16.hip, layer_n6.hip): 16-byte chunk c of row r sits in slot c ^ bank_sw<KCH>(r),
// KCH = chunks per row: 16 (256-byte rows) or 20 (320-byte rows; consecutive rows already start 16 banks apart)
template <int KCH>
static __device__ __forceinline__ int bank_sw(int r) { return KCH == 16 ? (r & 15) : ((r >> 2) & 3); }
