// The element type of one tensor of a mixed-precision training node (fixup_train_io.hip, mbconv_train_io.hip) and its 1- /
// 4-element accesses: up-cast on load (exact), ONE rounding on store; and the host-side dtype-code helpers that go with it.
#pragma once
#include <initializer_list>
#include <type_traits>
#include <utility>

#include "mfma.h"

namespace vqae {

// ---- one tensor's element type and its 1- / 4-element accesses (up-cast on load, one rounding on store) ------------------
template <int DT> struct Io {
    using elem = float;
    static __device__ __forceinline__ float ld(const elem* p, int64_t i) { return p[i]; }
    static __device__ __forceinline__ void st(elem* p, int64_t i, float v) { p[i] = v; }
    static __device__ __forceinline__ f32x4 ld4(const elem* p, int64_t i4) { return reinterpret_cast<const f32x4*>(p)[i4]; }
    static __device__ __forceinline__ void st4(elem* p, int64_t i4, const f32x4& v) { reinterpret_cast<f32x4*>(p)[i4] = v; }
};
template <int DT> struct Io16 {
    using elem = typename Mfma16<DT>::elem;
    using x4 = typename Mfma16<DT>::x4;
    // The one rounding of a result.  The empty asm pins the fp32 value in a register first: left alone, hipcc folds a product
    // and its conversion into v_fma_mixlo_f16 a, b, 0 -- ONE rounding of the exact product where torch's cast rounds the fp32
    // product, and +0 where the product is -0.
    static __device__ __forceinline__ elem rnd(float v) {
        asm("" : "+v"(v));
        return (elem)round_to<DT>(v);
    }
    static __device__ __forceinline__ float ld(const elem* p, int64_t i) { return (float)p[i]; }
    static __device__ __forceinline__ void st(elem* p, int64_t i, float v) { p[i] = rnd(v); }
    static __device__ __forceinline__ f32x4 ld4(const elem* p, int64_t i4) {
        const x4 r = reinterpret_cast<const x4*>(p)[i4];
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)r[e];
        return v;
    }
    static __device__ __forceinline__ void st4(elem* p, int64_t i4, const f32x4& v) {
        x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = rnd(v[e]);
        reinterpret_cast<x4*>(p)[i4] = r;
    }
};
template <> struct Io<VQAE_DT_BF16> : Io16<VQAE_DT_BF16> {};
template <> struct Io<VQAE_DT_F16> : Io16<VQAE_DT_F16> {};

template <int V> using DtC = std::integral_constant<int, V>;

static inline bool dt_ok(int dt) { return dt == VQAE_DT_F32 || dt == VQAE_DT_BF16 || dt == VQAE_DT_F16; }
static inline bool dt_16(int dt) { return dt == VQAE_DT_BF16 || dt == VQAE_DT_F16; }

// the 4-element access of a tensor: 16 bytes (fp32) or 8 (16-bit)
static inline bool aligned_vec(std::initializer_list<std::pair<const void*, int>> ps) {
    for (const auto& p : ps)
        if ((uintptr_t)p.first & (dt_16(p.second) ? 7 : 15)) return false;
    return true;
}

}  // namespace vqae
