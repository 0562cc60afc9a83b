// Device-side vocabulary of the kernel files: the vector types, the 16-bit MFMA operand policy, the compile-time autocast
// rounding and the MFMA fragment order of a weight matrix.  Each of these is one decision; the kernel files include it from
// here.  Host-side helpers are in common.h, the functions one file defines for another in kernels.h.
#pragma once
#include "common.h"

namespace vqae {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// autocast rounding with the dtype compiled in: fp32 value -> nearest DT (RNE) -> fp32; the identity for fp32
// (round_dt in common.h is the run-time form)
template <int DT> __device__ __forceinline__ float round_to(float v) {
    if (DT == VQAE_DT_BF16) return (float)(__bf16)v;
    if (DT == VQAE_DT_F16) return (float)(_Float16)v;
    return v;
}

// 16-bit MFMA operands of dtype DT (bf16 / f16): element and fragment types, v_mfma_f32_32x32x16_{bf16,f16} (one k-step:
// lane (i = l & 31, h = l >> 5) holds the 8 consecutive k at 8 h of row / column i), and the rounding fp32 -> DT -> fp32
template <int DT> struct Mfma16;
template <> struct Mfma16<VQAE_DT_BF16> {
    using elem = __bf16; using x8 = bf16x8; using x4 = bf16x4;
    static __device__ __forceinline__ f32x16 mma(const x8& a, const x8& b, const f32x16& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ float rnd(float v) { return round_to<VQAE_DT_BF16>(v); }
};
template <> struct Mfma16<VQAE_DT_F16> {
    using elem = _Float16; using x8 = f16x8; using x4 = f16x4;
    static __device__ __forceinline__ f32x16 mma(const x8& a, const x8& b, const f32x16& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ float rnd(float v) { return round_to<VQAE_DT_F16>(v); }
};

// fp32 fragment order of a [n][K] matrix: element (n, k) of the 32-row tile n >> 5 and sk-wide k-slice k / sk goes to
// lane (k / (sk / 2) & 1) * 32 + (n & 31), component k % (sk / 2).  sk = 8: what lane (li = n & 31, hh) feeds to fp32 MFMA
// number k & 3 of the slice; sk = 16: the lane's half of a 16-bit MFMA's k-step, still as fp32.
__device__ __forceinline__ int frag_offset(int n, int k, int K, int sk = 8) {
    const int h = sk / 2;
    return (((n >> 5) * (K / sk) + k / sk) * 64 + ((k / h) & 1) * 32 + (n & 31)) * h + k % h;
}

}  // namespace vqae

namespace {

// per-channel normalisation of a uint8 RGB input, passed by value to the kernels that read one (file-local, as they are)
struct Norm3 { float mean[4]; float inv[4]; };

}  // namespace
