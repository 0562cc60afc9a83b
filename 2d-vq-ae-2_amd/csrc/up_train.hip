// Training forms of the two full-resolution ops of an 'up' Fixup block in the commuted order (conv_block.py:196-216 with the
// bicubic x2 of conv.py:4-11 moved behind the 1x1 convs it commutes with), forward and backward, fp32, NHWC:
//
//   up2_act       y = ELU(up2(t_low) + a) + b                       t_low [B][H][W][C] -> y [B][2H][2W][C]
//   fixup_out_up  y = (t * scale + bias4) + (up2(s_low) + bias1d)   t, y [B][2H][2W][C], s_low [B][H][W][C]
//
// up2 is the bicubic x2 of fixup_train.hip: per output the sums of ft_bicubic_fwd (columns left to right per row, then rows
// top to bottom, unfused, clamped taps), and up2^T the gather of ft_bicubic_bwd (output rows 2i-3 .. 2i+4 outer, columns
// inner, zero-weight outputs skipped).  Same expressions, same order, -ffp-contract=off: up2_act is bit for bit
// fixup_act(bicubic_up2_bias(t_low)), its g_t_low bit for bit bicubic_up2_backward(fixup_act_backward(...)), and likewise
// for fixup_out_up.  What the fusion removes is memory: neither up2(t_low), nor g_v = g * ELU'(up2(t_low) + a), nor
// up2(s_low) is ever written; the backward recomputes up2(t_low) from the saved low-resolution tensor.
//
// A workgroup owns UT_T x UT_T low-resolution pixels x UT_K channels, i.e. a 2 UT_T x 2 UT_T tile of outputs.
//   forward   stages the (UT_T + 4)^2 clamped input window once (each input pixel is read once per workgroup, not once
//             per output that uses it); a thread owns one output column x 4 output rows and keeps the 6 row sums
//             they share in registers.
//   backward  stages the (UT_T + 6)^2 clamped window of t_low, forms g_v for the (2 UT_T + 6)^2 outputs the tile's pixels
//             gather from (its own outputs and a 3-pixel halo) into LDS, reading g once per tile, and gathers from LDS.
//             fixup_out_up's backward is the same gather with g_v = g; it writes g_t = g * scale from the staged tile's own
//             outputs in the same pass.  Both passes are separable (row sums, then column sums) with the sums shared through
//             LDS; the order of every sum is ft_bicubic_fwd's / ft_bicubic_bwd's.
// The g_v tile is stored [row][column parity][column / 2][channel]: the lanes of a wave walk low-resolution columns, whose
// outputs of one window position lie two columns apart; split by parity they are contiguous, so the 16-byte LDS reads of
// every 16-lane group cover one contiguous 256-byte row of banks.
// LDS per workgroup: forward 9 KiB; backward 41.25 KiB (fixup_out_up) and 49.5 KiB (up2_act), regions reused as they die.
//
// Sums (g_a = sum g_v, g_b = sum g; g_scale = sum g t, g_bias4 = g_bias1d = sum g) count a tile's own outputs only, per thread
// in fp64 in index order, then fixup_train.hip's scheme: wave shuffle, the four waves in order, one fp64 row per workgroup,
// one final launch and one rounding.  The grid is a function of the shape alone; no floating-point atomics.
#include "fixup_train_impl.h"

namespace {

using namespace vqae;
using namespace vqae::ft;

constexpr int UT_T = 8;                          // low-resolution pixels per tile axis
constexpr int UT_K = 16;                         // channels per tile
constexpr int UT_MAX_WG = 2048;                  // workgroups (rows of fp64 partials); a workgroup loops over its tiles
constexpr int UT_FW = UT_T + 4;                  // forward window of inputs:   i0 - 2 .. i0 + T + 1
constexpr int UT_BW = UT_T + 6;                  // backward window of inputs:  i0 - 3 .. i0 + T + 2
constexpr int UT_GW = 2 * UT_T + 6;              // backward window of outputs: 2 i0 - 3 .. 2 i0 + 2 T + 2
constexpr int UT_GH = UT_GW / 2;                 // columns of one parity

struct Tiles {
    int ty, tx, kc;                              // tiles per image along H, W and channel chunks
    int64_t n;
};
inline Tiles ut_tiles(int B, int H, int W, int C) {
    Tiles t;
    t.ty = (int)ceil_div(H, UT_T);
    t.tx = (int)ceil_div(W, UT_T);
    t.kc = (int)ceil_div(C, UT_K);
    t.n = (int64_t)B * t.ty * t.tx * t.kc;
    return t;
}
inline int ut_grid(const Tiles& t) { return (int)std::min<int64_t>(UT_MAX_WG, t.n); }

template <int VEC>
__device__ __forceinline__ Pk<VEC> zero_pk() {
    Pk<VEC> v;
#pragma unroll
    for (int e = 0; e < VEC; ++e) v.f[e] = 0.f;
    return v;
}

// The clamped window [n x n] of low-resolution pixels with origin (i0, j0) (may be negative), channels c0 .. c0 + UT_K, as
// x + 0.f (ft_bicubic_fwd's `x + pre_bias` without a bias) -> tile[pixel][UT_K].  Channels >= C are staged as zeros.
template <int VEC>
__device__ __forceinline__ void stage_low(const float* __restrict__ x, int bb, int H, int W, int C, int i0, int j0, int c0,
                                          int n, float* __restrict__ tile) {
    using P = Pk<VEC>;
    constexpr int KV = UT_K / VEC;
    for (int it = threadIdx.x; it < n * n * KV; it += FT_THREADS) {
        const int q = it % KV, p = it / KV, ch = c0 + q * VEC;
        P v = zero_pk<VEC>();
        if (ch < C) {
            const int iy = clampi(i0 + p / n, H - 1), ix = clampi(j0 + p % n, W - 1);
            v = *reinterpret_cast<const P*>(x + (((int64_t)bb * H + iy) * W + ix) * C + ch);
#pragma unroll
            for (int e = 0; e < VEC; ++e) v.f[e] = v.f[e] + 0.f;
        }
        *reinterpret_cast<P*>(tile + p * UT_K + q * VEC) = v;
    }
}

// One row of an output's sum: the four taps of column window `col` .. col + 3 of a staged row, left to right.
template <int VEC>
__device__ __forceinline__ Pk<VEC> row_sum(const float* __restrict__ row, bool oddx) {
    using P = Pk<VEC>;
    P h;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const P v = *reinterpret_cast<const P*>(row + j * UT_K);
        const float wx = oddx ? tap25(j) : tap75(j);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float q = v.f[e] * wx;
            h.f[e] = j == 0 ? q : h.f[e] + q;
        }
    }
    return h;
}

// ACT:  y = ELU(up2(x) + *p0) + *p1                       (p0 = a, p1 = b)
// !ACT: y = (t * *p0 + *p1) + (up2(x) + *p2)              (p0 = scale, p1 = bias4, p2 = bias1d)
template <int VEC, bool ACT>
__global__ __launch_bounds__(FT_THREADS)
void ut_fwd(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ pp0,
            const float* __restrict__ pp1, const float* __restrict__ pp2, int B, int H, int W, int C, Tiles tiles,
            float* __restrict__ y) {
    using P = Pk<VEC>;
    constexpr int KV = UT_K / VEC;
    __shared__ __attribute__((aligned(16))) float win[UT_FW * UT_FW * UT_K];
    const float p0 = *pp0, p1 = *pp1, p2 = ACT ? 0.f : *pp2;
    const int OH = 2 * H, OW = 2 * W;
    for (int64_t tile = blockIdx.x; tile < tiles.n; tile += gridDim.x) {
        int64_t r = tile;
        const int c0 = (int)(r % tiles.kc) * UT_K; r /= tiles.kc;
        const int j0 = (int)(r % tiles.tx) * UT_T; r /= tiles.tx;
        const int i0 = (int)(r % tiles.ty) * UT_T;
        const int bb = (int)(r / tiles.ty);
        stage_low<VEC>(x, bb, H, W, C, i0 - 2, j0 - 2, c0, UT_FW, win);
        __syncthreads();
        // item = (channel group, output column of the tile, group of 4 output rows = 2 low-resolution rows)
        for (int it = threadIdx.x; it < KV * 2 * UT_T * (UT_T / 2); it += FT_THREADS) {
            const int q = it % KV, oxl = (it / KV) % (2 * UT_T), rg = it / (KV * 2 * UT_T);
            const int ch = c0 + q * VEC, ox = 2 * j0 + oxl;
            if (ch >= C || ox >= OW) continue;
            const bool oddx = oxl & 1;
            const int col = (oxl >> 1) - (oddx ? 1 : 2) + 2;              // window column of the first tap
            // output rows 4 rg + d, d = 0 .. 3, read window rows 2 rg + s(d) .. + 3, s = 0, 1, 1, 2
            P h[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) h[k] = row_sum<VEC>(win + ((2 * rg + k) * UT_FW + col) * UT_K + q * VEC, oddx);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int oy = 2 * i0 + 4 * rg + d;
                if (oy >= OH) continue;
                const bool oddy = d & 1;
                const int s = d == 0 ? 0 : (d == 3 ? 2 : 1);
                P out;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float wy = oddy ? tap25(k) : tap75(k);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const float v = h[s + k].f[e] * wy;
                        out.f[e] = k == 0 ? v : out.f[e] + v;
                    }
                }
                const int64_t o = (((int64_t)bb * OH + oy) * OW + ox) * C + ch;
                if constexpr (ACT) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) out.f[e] = elu_train(out.f[e] + p0) + p1;
                } else {
                    const P tv = *reinterpret_cast<const P*>(t + o);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) out.f[e] = (tv.f[e] * p0 + p1) + (out.f[e] + p2);
                }
                *reinterpret_cast<P*>(y + o) = out;
            }
        }
        __syncthreads();                                                  // the next tile overwrites the window
    }
}

// ACT:  g_v = g * ELU'(up2(x) + *p0) (x = t_low, p0 = a);  g_low = up2^T g_v;  s0 = sum g_v, s1 = sum g
// !ACT: g_v = g;  g_t = g * *p0 (p0 = scale);  g_low = up2^T g;  s0 = sum g * x (x = t, full resolution), s1 = sum g
// Both directions are separable without changing a bit: an output's row sums depend on (input row, output column) only and
// are shared by the output rows that read that input row, and the gather's inner sums depend on (output row, low-resolution
// column) only and are shared by the 4 low-resolution rows that read that output row.  LDS, in floats:
//   r0  the g_v tile [UT_GW][2][UT_GH][UT_K];  before it exists, the t_low window [UT_BW][UT_BW][UT_K] (ACT)
//   r1  ACT: the row sums of up2(t_low) [UT_BW][UT_GW][UT_K];  then the gather's inner sums [UT_GW][UT_T][UT_K]
template <int VEC, bool ACT>
__global__ __launch_bounds__(FT_THREADS)
void ut_bwd(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ pp0, int B, int H, int W, int C,
            Tiles tiles, float* __restrict__ g_low, float* __restrict__ g_t, double* __restrict__ partials) {
    using P = Pk<VEC>;
    constexpr int KV = UT_K / VEC;
    constexpr int R0 = UT_GW * UT_GW * UT_K, R1 = (ACT ? UT_BW : UT_T) * UT_GW * UT_K;
    __shared__ __attribute__((aligned(16))) float lds[R0 + R1];
    float* const gt = lds;                               // [row][parity][column / 2][UT_K]
    float* const win = lds;                              // dead once the row sums exist
    float* const hs = lds + R0;                          // [window row][output column][UT_K]
    float* const hg = lds + R0;                          // [output row][low-resolution column][UT_K]; hs is dead by then
    const float p0 = *pp0;
    const int OH = 2 * H, OW = 2 * W;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t tile = blockIdx.x; tile < tiles.n; tile += gridDim.x) {
        int64_t r = tile;
        const int c0 = (int)(r % tiles.kc) * UT_K; r /= tiles.kc;
        const int j0 = (int)(r % tiles.tx) * UT_T; r /= tiles.tx;
        const int i0 = (int)(r % tiles.ty) * UT_T;
        const int bb = (int)(r / tiles.ty);
        if constexpr (ACT) {
            stage_low<VEC>(x, bb, H, W, C, i0 - 3, j0 - 3, c0, UT_BW, win);
            __syncthreads();
            // row sums of up2(t_low): window row wr x output column 2 j0 - 3 + lc (zeros outside the image: never read)
            for (int it = threadIdx.x; it < UT_BW * UT_GW * KV; it += FT_THREADS) {
                const int q = it % KV, p = it / KV, wr = p / UT_GW, lc = p % UT_GW;
                const int ox = 2 * j0 - 3 + lc;
                P h = zero_pk<VEC>();
                if (ox >= 0 && ox < OW) {
                    const bool oddx = ox & 1;
                    const int wc = (ox >> 1) - (oddx ? 1 : 2) - (j0 - 3);     // first tap, as a window column: 0 .. UT_BW - 4
                    h = row_sum<VEC>(win + (wr * UT_BW + wc) * UT_K + q * VEC, oddx);
                }
                *reinterpret_cast<P*>(hs + p * UT_K + q * VEC) = h;
            }
            __syncthreads();                             // the g_v tile overwrites the window
        }
        // g_v of the outputs 2 i0 - 3 .. 2 i0 + 2 T + 2 (columns likewise); zeros outside the image and past C
        for (int it = threadIdx.x; it < UT_GW * UT_GW * KV; it += FT_THREADS) {
            const int q = it % KV, p = it / KV, lr = p / UT_GW, lc = p % UT_GW;
            const int oy = 2 * i0 - 3 + lr, ox = 2 * j0 - 3 + lc, ch = c0 + q * VEC;
            P val = zero_pk<VEC>();
            if (oy >= 0 && oy < OH && ox >= 0 && ox < OW && ch < C) {
                const int64_t o = (((int64_t)bb * OH + oy) * OW + ox) * C + ch;
                const P gv = *reinterpret_cast<const P*>(g + o);
                const bool own = lr >= 3 && lr < 3 + 2 * UT_T && lc >= 3 && lc < 3 + 2 * UT_T;   // this tile's own outputs
                if constexpr (ACT) {
                    const bool oddy = oy & 1;
                    const int wr = (oy >> 1) - (oddy ? 1 : 2) - (i0 - 3);     // first tap, as a window row: 0 .. UT_BW - 4
                    P v;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const P h = *reinterpret_cast<const P*>(hs + ((wr + k) * UT_GW + lc) * UT_K + q * VEC);
                        const float wy = oddy ? tap25(k) : tap75(k);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const float u = h.f[e] * wy;
                            v.f[e] = k == 0 ? u : v.f[e] + u;
                        }
                    }
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        val.f[e] = gv.f[e] * elu_grad(v.f[e] + p0);
                        if (own) {
                            s0 += (double)val.f[e];
                            s1 += (double)gv.f[e];
                        }
                    }
                } else {
                    val = gv;
                    if (own) {
                        const P tv = *reinterpret_cast<const P*>(x + o);
                        P gs;
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            gs.f[e] = gv.f[e] * p0;
                            s0 += (double)gv.f[e] * (double)tv.f[e];
                            s1 += (double)gv.f[e];
                        }
                        *reinterpret_cast<P*>(g_t + o) = gs;
                    }
                }
            }
            *reinterpret_cast<P*>(gt + ((lr * 2 + (lc & 1)) * UT_GH + (lc >> 1)) * UT_K + q * VEC) = val;
        }
        __syncthreads();                                 // the inner sums overwrite the row sums
        // the gather of ft_bicubic_bwd, inner sums: output row lr x low-resolution column jl reads window columns 2 jl .. 2 jl + 7
        for (int it = threadIdx.x; it < UT_GW * UT_T * KV; it += FT_THREADS) {
            const int q = it % KV, p = it / KV, jl = p % UT_T, lr = p / UT_T;
            const int ix = j0 + jl;
            P h = zero_pk<VEC>();
            if (ix < W) {
                const float* row = gt + lr * 2 * UT_GH * UT_K + q * VEC;
#pragma unroll
                for (int c = 0; c < 8; ++c) {            // outputs 2i-3 .. 2i+4: every output whose clamped taps can reach i
                    const int ox = 2 * ix - 3 + c, lc = 2 * jl + c;
                    const float ax = (ox >= 0 && ox < OW) ? axis_weight(ox, ix, W) : 0.f;
                    if (ax == 0.f) continue;             // outside the grid, or no tap of this output reaches ix
                    const P gv = *reinterpret_cast<const P*>(row + ((lc & 1) * UT_GH + (lc >> 1)) * UT_K);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) h.f[e] = h.f[e] + gv.f[e] * ax;
                }
            }
            *reinterpret_cast<P*>(hg + p * UT_K + q * VEC) = h;
        }
        __syncthreads();
        // outer sums: low-resolution pixel (il, jl) of the tile reads the inner sums of output rows 2 il .. 2 il + 7
        for (int it = threadIdx.x; it < UT_T * UT_T * KV; it += FT_THREADS) {
            const int q = it % KV, p = it / KV, jl = p % UT_T, il = p / UT_T;
            const int iy = i0 + il, ix = j0 + jl, ch = c0 + q * VEC;
            if (iy >= H || ix >= W || ch >= C) continue;
            P acc = zero_pk<VEC>();
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int oy = 2 * iy - 3 + k;
                const float ay = (oy >= 0 && oy < OH) ? axis_weight(oy, iy, H) : 0.f;
                if (ay == 0.f) continue;
                const P h = *reinterpret_cast<const P*>(hg + ((2 * il + k) * UT_T + jl) * UT_K + q * VEC);
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc.f[e] = acc.f[e] + h.f[e] * ay;
            }
            *reinterpret_cast<P*>(g_low + (((int64_t)bb * H + iy) * W + ix) * C + ch) = acc;
        }
        __syncthreads();                                 // the next tile overwrites every region
    }
    ft_block_partials(s0, s1, partials);
}

}  // namespace

extern "C" size_t vqae_up_train_workspace_bytes(int B, int H, int W, int C) {
    const int grid = (B >= 1 && H >= 1 && W >= 1 && C >= 1) ? ut_grid(ut_tiles(B, H, W, C)) : 1;
    return (size_t)grid * FT_SUMS * sizeof(double) + 256;
}

extern "C" int vqae_up2_act_f32(const float* t_low, const float* a, const float* b, int B, int H, int W, int C, float* y,
                                void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_dims("up2_act", B, H, W, C, 4)) return rc;
    VQAE_REQUIRE(t_low && a && b && y, VQAE_ERR_INVALID, "up2_act: null pointer");
    const Tiles tiles = ut_tiles(B, H, W, C);
    if (C % 4 == 0 && aligned16({t_low, y}))
        ut_fwd<4, true><<<ut_grid(tiles), FT_THREADS, 0, stream>>>(t_low, nullptr, a, b, nullptr, B, H, W, C, tiles, y);
    else
        ut_fwd<1, true><<<ut_grid(tiles), FT_THREADS, 0, stream>>>(t_low, nullptr, a, b, nullptr, B, H, W, C, tiles, y);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" int vqae_up2_act_backward_f32(const float* g, const float* t_low, const float* a, int B, int H, int W, int C,
                                         float* g_t_low, float* g_a, float* g_b, void* ws, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_dims("up2_act_backward", B, H, W, C, 4)) return rc;
    VQAE_REQUIRE(g && t_low && a && g_t_low && ws, VQAE_ERR_INVALID, "up2_act_backward: null pointer");
    VQAE_REQUIRE(((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID, "up2_act_backward: workspace must be 8-byte aligned");
    const Tiles tiles = ut_tiles(B, H, W, C);
    const int grid = ut_grid(tiles);
    if (C % 4 == 0 && aligned16({g, t_low, g_t_low}))
        ut_bwd<4, true><<<grid, FT_THREADS, 0, stream>>>(g, t_low, a, B, H, W, C, tiles, g_t_low, nullptr, (double*)ws);
    else
        ut_bwd<1, true><<<grid, FT_THREADS, 0, stream>>>(g, t_low, a, B, H, W, C, tiles, g_t_low, nullptr, (double*)ws);
    VQAE_LAUNCH_CHECK();
    return finish_sums((double*)ws, grid, g_a, nullptr, g_b, nullptr, stream);
}

extern "C" int vqae_fixup_out_up_f32(const float* t, const float* s_low, const float* scale, const float* bias4,
                                     const float* bias1d, int B, int H, int W, int C, float* y, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_dims("fixup_out_up", B, H, W, C, 4)) return rc;
    VQAE_REQUIRE(t && s_low && scale && bias4 && bias1d && y, VQAE_ERR_INVALID, "fixup_out_up: null pointer");
    const Tiles tiles = ut_tiles(B, H, W, C);
    if (C % 4 == 0 && aligned16({t, s_low, y}))
        ut_fwd<4, false><<<ut_grid(tiles), FT_THREADS, 0, stream>>>(s_low, t, scale, bias4, bias1d, B, H, W, C, tiles, y);
    else
        ut_fwd<1, false><<<ut_grid(tiles), FT_THREADS, 0, stream>>>(s_low, t, scale, bias4, bias1d, B, H, W, C, tiles, y);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" int vqae_fixup_out_up_backward_f32(const float* g, const float* t, const float* scale, int B, int H, int W, int C,
                                              float* g_t, float* g_s_low, float* g_scale, float* g_bias4, float* g_bias1d,
                                              void* ws, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_dims("fixup_out_up_backward", B, H, W, C, 4)) return rc;
    VQAE_REQUIRE(g && t && scale && g_t && g_s_low && ws, VQAE_ERR_INVALID, "fixup_out_up_backward: null pointer");
    VQAE_REQUIRE(((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID, "fixup_out_up_backward: workspace must be 8-byte aligned");
    const Tiles tiles = ut_tiles(B, H, W, C);
    const int grid = ut_grid(tiles);
    if (C % 4 == 0 && aligned16({g, t, g_t, g_s_low}))
        ut_bwd<4, false><<<grid, FT_THREADS, 0, stream>>>(g, t, scale, B, H, W, C, tiles, g_s_low, g_t, (double*)ws);
    else
        ut_bwd<1, false><<<grid, FT_THREADS, 0, stream>>>(g, t, scale, B, H, W, C, tiles, g_s_low, g_t, (double*)ws);
    VQAE_LAUNCH_CHECK();
    return finish_sums((double*)ws, grid, g_scale, nullptr, g_bias4, g_bias1d, stream);
}
