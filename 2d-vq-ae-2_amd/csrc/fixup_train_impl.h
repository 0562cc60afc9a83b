// Shared by fixup_train.hip and up_train.hip: the bicubic x2 taps and adjoint weights, the 1- / 4-channel pixel pack, and the
// fixed-order fp64 sums (per-workgroup partial rows, one final launch).  Everything here has internal linkage: each file
// that includes it gets its own copy.
#pragma once
#include <algorithm>

#include "kernels.h"
#include "mfma.h"

namespace vqae {
namespace ft {

constexpr int FT_THREADS = 256;
constexpr int FT_SUMS = 2;               // sums per op

// The workgroup's FT_SUMS sums -> its row of the workspace.  Called by every thread of the workgroup.
__device__ __forceinline__ void ft_block_partials(double s0, double s1, double* __restrict__ partials) {
    __shared__ double red[FT_SUMS][FT_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if (lane == 0) { red[0][wave] = s0; red[1][wave] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[(int64_t)blockIdx.x * FT_SUMS + 0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        partials[(int64_t)blockIdx.x * FT_SUMS + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// One workgroup: thread t adds rows t, t + 256, ... in that order, then the same wave / workgroup order as above.
static __global__ __launch_bounds__(FT_THREADS)
void ft_final(const double* __restrict__ partials, int n_wg, float* __restrict__ o0a, float* __restrict__ o0b,
              float* __restrict__ o1a, float* __restrict__ o1b) {
    __shared__ double red[FT_SUMS][FT_THREADS / 64];
    double s0 = 0.0, s1 = 0.0;
    for (int w = threadIdx.x; w < n_wg; w += FT_THREADS) {
        s0 += partials[(int64_t)w * FT_SUMS + 0];
        s1 += partials[(int64_t)w * FT_SUMS + 1];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if (lane == 0) { red[0][wave] = s0; red[1][wave] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v0 = (float)(((red[0][0] + red[0][1]) + red[0][2]) + red[0][3]);
        const float v1 = (float)(((red[1][0] + red[1][1]) + red[1][2]) + red[1][3]);
        if (o0a) *o0a = v0;
        if (o0b) *o0b = v0;
        if (o1a) *o1a = v1;
        if (o1b) *o1b = v1;
    }
}

static inline int finish_sums(const double* ws, int n_wg, float* o0a, float* o0b, float* o1a, float* o1b, hipStream_t stream) {
    if (!(o0a || o0b || o1a || o1b)) return VQAE_OK;
    ft_final<<<1, FT_THREADS, 0, stream>>>(ws, n_wg, o0a, o0b, o1a, o1b);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

// ---- pixel forms: one thread = one pixel x VEC channels (VEC = 4 where C % 4 == 0 and the pointers allow, else 1) --------
template <int VEC> struct alignas(VEC * 4) Pk { float f[VEC]; };       // VEC = 4: one 16-byte access
template <int VEC> struct Pack { using type = Pk<VEC>; };
template <int VEC> __device__ __forceinline__ float& lane_of(Pk<VEC>& v, int e) { return v.f[e]; }

// Bicubic x2 taps (A = -0.75): even outputs (source offset .75) read inputs m-2 .. m+1, odd outputs (.25) m-1 .. m+2, m = o >> 1
__device__ __forceinline__ float tap75(int k) { return k == 0 ? -0.03515625f : k == 1 ? 0.26171875f : k == 2 ? 0.87890625f : -0.10546875f; }
__device__ __forceinline__ float tap25(int k) { return k == 0 ? -0.10546875f : k == 1 ? 0.87890625f : k == 2 ? 0.26171875f : -0.03515625f; }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Weight of input `i` in output `o` along an axis of n inputs: the sum of o's four taps whose clamped index is i (the taps
// are multiples of 2^-8, so the sum is exact).
__device__ __forceinline__ float axis_weight(int o, int i, int n) {
    const bool odd = o & 1;
    const int base = (o >> 1) - (odd ? 1 : 2);
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (clampi(base + k, n - 1) == i) a += odd ? tap25(k) : tap75(k);
    return a;
}

// dims of a [B][H][W][C] tensor: each >= 1 and the element count (of the LARGEST tensor of the op, `grow` elements per
// input element) below 2^40
static inline int check_dims(const char* who, int B, int H, int W, int C, int grow) {
    VQAE_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1, VQAE_ERR_INVALID, "%s: shape [%d][%d][%d][%d]", who, B, H, W, C);
    VQAE_REQUIRE(H <= (1 << 28) && W <= (1 << 28) && (double)B * (H + 2.0) * (W + 2.0) * C * grow < 1099511627776.0,
                 VQAE_ERR_UNSUPPORTED, "%s: shape [%d][%d][%d][%d] is too large", who, B, H, W, C);
    return VQAE_OK;
}

}  // namespace ft
}  // namespace vqae
