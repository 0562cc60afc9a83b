// Shared by mbconv_train.hip (fp32) and mbconv_train_io.hip (16-bit I/O): the lane layout, the fixed-order fp64 sums (one
// partial row per workgroup, one finishing launch), SiLU and its derivative, and the host-side shape checks.  Everything here
// has internal linkage: each file that includes it gets its own copy.
#pragma once
#include <algorithm>

#include "kernels.h"
#include "mfma.h"

namespace vqae {
namespace mbt {

constexpr int MBT_THREADS = 256;
constexpr int MBT_ROWS = VQAE_MBT_ROWS;            // rows (pixels) one workgroup reduces: one fp64 partial row each
constexpr int MBT_FIN_LANES = VQAE_MBT_FIN_LANES;  // lanes that share one column's partial rows in the finishing launch
static_assert(MBT_ROWS == 256 && MBT_FIN_LANES == 64, "the kernels assume 256 rows per workgroup and one wave per column");

__device__ __forceinline__ float sigmoid1(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ float silu1(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float silu_grad1(float v) {
    const float s = sigmoid1(v);
    return s * (1.0f + v * (1.0f - s));
}

struct Lane {
    int cg, pl, PL;
    bool live;
};
__device__ __forceinline__ Lane lane_of_thread(int C4) {
    Lane l;
    l.PL = MBT_THREADS / C4;
    l.cg = threadIdx.x % C4;
    l.pl = threadIdx.x / C4;
    l.live = l.pl < l.PL;
    return l;
}

// acc[K][4] of every thread -> row[k * C + 4 cg + e], the pixel lanes added in index order.  Called by all 256 threads.
template <int K>
__device__ __forceinline__ void block_rows(const double (&acc)[K][4], const Lane& l, int C4, double* __restrict__ row) {
    __shared__ double red[MBT_THREADS][4];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) red[threadIdx.x][e] = acc[k][e];
        __syncthreads();
        if (l.pl == 0) {
            double s[4] = {red[l.cg][0], red[l.cg][1], red[l.cg][2], red[l.cg][3]};
            for (int q = 1; q < l.PL; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] += red[q * C4 + l.cg][e];
#pragma unroll
            for (int e = 0; e < 4; ++e) row[(int64_t)k * C4 * 4 + l.cg * 4 + e] = s[e];
        }
        __syncthreads();
    }
}

// lane `l` of a wave adds rows l, l + 64, ... of column `col` in order, then the lanes by shuffle: lane 0 has the sum
__device__ __forceinline__ double column_sum(const double* __restrict__ partials, int n_rows, int n_cols, int col, int lane) {
    double s = 0.0;
    for (int r = lane; r < n_rows; r += MBT_FIN_LANES) s += partials[(int64_t)r * n_cols + col];
    return wave_sum(s);
}

// partials [n_batches][n_rows][n_cols] -> out [n_batches][n_cols]; taps > 0: the column (t, c) of a [taps][C] row goes to
// out[c * taps + t], the layout of a [C][1][k][k] weight.  out64 (or NULL): the same sums unrounded, column order kept.
// grid (ceil(n_cols / 4), n_batches), one wave per column.
static __global__ __launch_bounds__(MBT_THREADS)
void mbt_finish(const double* __restrict__ partials, int n_rows, int n_cols, int taps, float* __restrict__ out,
                double* __restrict__ out64) {
    const int lane = threadIdx.x & 63, col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= n_cols) return;                                   // wave-uniform
    const double s = column_sum(partials + (int64_t)blockIdx.y * n_rows * n_cols, n_rows, n_cols, col, lane);
    if (lane != 0) return;
    int o = col;
    if (taps > 0) {
        const int C = n_cols / taps, t = col / C, c = col - t * C;
        o = c * taps + t;
    }
    out[(int64_t)blockIdx.y * n_cols + o] = (float)s;
    if (out64) out64[(int64_t)blockIdx.y * n_cols + col] = s;
}

static __global__ void bn_eval_stats_kernel(const float* __restrict__ running_mean, const float* __restrict__ running_var,
                                            double eps, int C, double* __restrict__ mean, double* __restrict__ invstd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    mean[c] = (double)running_mean[c];
    invstd[c] = 1.0 / sqrt((double)running_var[c] + eps);
}

__device__ __forceinline__ int wrap_m(int i, int n) { return i == 0 ? n - 1 : i - 1; }
__device__ __forceinline__ int wrap_p(int i, int n) { return i == n - 1 ? 0 : i + 1; }

// a b + c with one rounding per element (the stock depthwise convs accumulate with fused multiply-adds too)
__device__ __forceinline__ f32x4 fma4(const f32x4& a, const f32x4& b, const f32x4& c) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = fmaf(a[e], b[e], c[e]);
    return r;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
static inline bool channels_ok(int c) { return c >= 4 && c % 4 == 0 && c <= 1024; }
static inline int64_t strips_of(int64_t hw) { return ceil_div(hw, MBT_ROWS); }

// batch x hw rows of c channels: the shape checks every entry shares (who: the entry's name for the message)
static inline int check_rows(const char* who, int64_t batch, int64_t hw, int c) {
    VQAE_REQUIRE(batch >= 1 && hw >= 1 && c >= 1, VQAE_ERR_INVALID, "%s: shape [%lld][%lld][%d]", who, (long long)batch,
                 (long long)hw, c);
    VQAE_REQUIRE(channels_ok(c), VQAE_ERR_UNSUPPORTED, "%s: channels %d must be a multiple of 4, at most 1024", who, c);
    VQAE_REQUIRE(batch <= 65535, VQAE_ERR_UNSUPPORTED, "%s: batch %lld > 65535", who, (long long)batch);
    VQAE_REQUIRE(hw < (1ll << 31) && (double)batch * (double)hw * c < 1099511627776.0, VQAE_ERR_UNSUPPORTED,
                 "%s: shape [%lld][%lld][%d] is too large", who, (long long)batch, (long long)hw, c);
    return VQAE_OK;
}

static inline int finish(const double* partials, int n_batches, int64_t n_rows, int n_cols, int taps, float* out,
                         hipStream_t stream, double* out64 = nullptr) {
    mbt_finish<<<dim3((unsigned)ceil_div(n_cols, 4), (unsigned)n_batches), MBT_THREADS, 0, stream>>>(partials, (int)n_rows, n_cols,
                                                                                                    taps, out, out64);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

static inline void dw_out_dims(int mode, int h, int w, int* ho, int* wo) {
    *ho = mode == VQAE_DW_DOWN ? h / 2 : (mode == VQAE_DW_UP ? 2 * h : h);
    *wo = mode == VQAE_DW_DOWN ? w / 2 : (mode == VQAE_DW_UP ? 2 * w : w);
}

static inline int dw_check(const char* who, int batch, int h, int w, int c, int mode) {
    VQAE_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && c >= 1, VQAE_ERR_INVALID, "%s: shape [%d][%d][%d][%d]", who, batch, h, w, c);
    VQAE_REQUIRE(mode >= VQAE_DW_SAME && mode <= VQAE_DW_UP, VQAE_ERR_INVALID, "%s: mode %d", who, mode);
    VQAE_REQUIRE(vqae_dwconv_train_supported(c, h, w, mode), VQAE_ERR_UNSUPPORTED,
                 "%s: channels %d must be a multiple of 4, at most 1024; h %d, w %d even and at most 16384 (mode %d)", who, c, h, w,
                 mode);
    VQAE_REQUIRE(batch <= 65535, VQAE_ERR_UNSUPPORTED, "%s: batch %d > 65535", who, batch);
    return VQAE_OK;
}

}  // namespace mbt
}  // namespace vqae
