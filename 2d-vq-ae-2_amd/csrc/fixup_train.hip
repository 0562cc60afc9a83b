// Training forms of every op of a Fixup block that is not a convolution (conv_block.py:196-216), forward and backward, fp32,
// NHWC.  The convolutions between them stay with the caller (train.py runs them through torch).
//
//   act       y = ELU(x + a) + b                      (three per block: `activation(out + bias_a)` then `+ bias_b`)
//             halo = 1: y is [B][H+2][W+2][C] with the circular wrap written, bit for bit F.pad(y, (1,1,1,1), 'circular'):
//             the 3x3 circular conv that follows runs with padding 0 and no pad copy exists
//   plain     y = x + c                               (`inp + bias1c` of the skip paths)
//   out       y = (t * scale + bias4) + (skip [+ bias1d])
//   bicubic   y = bicubic_x2(x + pre_bias), the arithmetic of vqae_bicubic_up2_f32 with pre_bias read from the device
//
// Every one-element parameter is read from DEVICE memory and every scalar gradient is written to device memory: a training
// step never synchronises the host for them.
//
// Backward, one pass each:
//   act       v = x + a, ELU' = v > 0 ? 1 : exp(v), from the saved INPUT.  (Deriving it from the output, ELU' = (y - b) + 1, loses
//             everything where the ELU saturates: y - b -> -1 leaves ELU' ~ 1e-7 with an absolute error of an ulp of 1.  Norm-wise
//             that is invisible, but Adam divides by the gradient's own size and turns it into full-size steps of dead channels:
//             DESIGN section 16 has both measured distances.)  With a halo the padded gradient is first folded onto the interior
//             in GATHER form: an interior pixel adds its images (itself, and the wrapped copies of border rows / columns: up to
//             4, up to 9 when H or W <= 2);  g_x = fold * ELU',  g_a = sum g_x,  g_b = sum fold
//   plain     g_c = sum g              (g_x is g itself: no launch writes it)
//   out       g_t = g * scale,  g_scale = sum g * t,  g_bias4 = g_bias1d = sum g     (g_skip is g itself)
//   bicubic   the exact adjoint in gather form: input pixel (i, j) walks the fixed window of outputs 2i-3 .. 2i+4 (2j-3 ..
//             2j+4) whose clamped taps can reach it and adds each output's weight onto it -- the sum of that output's taps
//             that clamp to i, which is how border pixels collect the clamped taps;  g_pre_bias = sum g_x
//
// Sums: every thread adds its elements in index order in fp64 (a product of two fp32 is exact there), the 64 lanes of a
// wave by shuffle, the 4 waves in index order, one fp64 row per workgroup in the workspace; ft_final adds the rows in a
// fixed order and rounds to fp32 once.  The grid is a function of the shape alone and there are no floating-point atomics:
// every result is bit-identical run to run.
//
// Everything here is fp32.  The forms of act / plain / out with 16-bit I/O, for training under autocast, are the sibling file
// fixup_train_io.hip (vqae_fixup_*_io): the same arithmetic in the same element order on up-cast values, one rounding on
// store; with every tensor fp32 they forward to the entry points below.
#include "fixup_train_impl.h"

namespace {

using namespace vqae;
using namespace vqae::ft;                // the taps, the pixel pack and the fixed-order sums, shared with up_train.hip

constexpr int FT_MAX_WG = 1024;          // rows of fp64 partials

inline int ft_grid(int64_t items) {
    return (int)std::min<int64_t>(FT_MAX_WG, std::max<int64_t>(1, ceil_div(items, FT_THREADS)));
}

// ---- flat forms (no halo): n4 16-byte groups, then the tail [4 n4, n) ----------------------------------------------------
template <bool ACT>
__global__ __launch_bounds__(FT_THREADS)
void ft_act_fwd_flat(const float* __restrict__ x, const float* __restrict__ pa, const float* __restrict__ pb, int64_t n,
                     int64_t n4, float* __restrict__ y) {
    const float a = ACT ? *pa : 0.f, b = *pb;
    const int64_t stride = (int64_t)gridDim.x * FT_THREADS, t0 = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    for (int64_t i = t0; i < n4; i += stride) {
        f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ACT ? elu_train(v[e] + a) + b : v[e] + b;
        reinterpret_cast<f32x4*>(y)[i] = v;
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) y[i] = ACT ? elu_train(x[i] + a) + b : x[i] + b;
}

// ACT: g_x = g * ELU'(x + a), s0 = sum g_x, s1 = sum g.  Plain: s1 = sum g only (x, pa, g_x unused).
template <bool ACT>
__global__ __launch_bounds__(FT_THREADS)
void ft_act_bwd_flat(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ pa, int64_t n,
                     int64_t n4, float* __restrict__ g_x, double* __restrict__ partials) {
    const float a = ACT ? *pa : 0.f;
    const int64_t stride = (int64_t)gridDim.x * FT_THREADS, t0 = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t i = t0; i < n4; i += stride) {
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        if constexpr (ACT) {
            const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = gv[e] * elu_grad(xv[e] + a);
                s0 += (double)o[e];
                s1 += (double)gv[e];
            }
            reinterpret_cast<f32x4*>(g_x)[i] = o;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) s1 += (double)gv[e];
        }
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) {
        const float gv = g[i];
        if constexpr (ACT) {
            const float o = gv * elu_grad(x[i] + a);
            g_x[i] = o;
            s0 += (double)o;
        }
        s1 += (double)gv;
    }
    ft_block_partials(s0, s1, partials);
}

__global__ __launch_bounds__(FT_THREADS)
void ft_out_fwd(const float* __restrict__ t, const float* __restrict__ skip, const float* __restrict__ pscale,
                const float* __restrict__ pb4, const float* __restrict__ pb1d, int64_t n, int64_t n4, float* __restrict__ y) {
    const float sc = *pscale, b4 = *pb4;
    const bool has_d = pb1d != nullptr;
    const float b1d = has_d ? *pb1d : 0.f;
    const int64_t stride = (int64_t)gridDim.x * FT_THREADS, t0 = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    for (int64_t i = t0; i < n4; i += stride) {
        const f32x4 tv = reinterpret_cast<const f32x4*>(t)[i], sv = reinterpret_cast<const f32x4*>(skip)[i];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (tv[e] * sc + b4) + (has_d ? sv[e] + b1d : sv[e]);
        reinterpret_cast<f32x4*>(y)[i] = o;
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) y[i] = (t[i] * sc + b4) + (has_d ? skip[i] + b1d : skip[i]);
}

// g_t = g * scale, s0 = sum g * t, s1 = sum g
__global__ __launch_bounds__(FT_THREADS)
void ft_out_bwd(const float* __restrict__ g, const float* __restrict__ t, const float* __restrict__ pscale, int64_t n,
                int64_t n4, float* __restrict__ g_t, double* __restrict__ partials) {
    const float sc = *pscale;
    const int64_t stride = (int64_t)gridDim.x * FT_THREADS, t0 = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t i = t0; i < n4; i += stride) {
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i], tv = reinterpret_cast<const f32x4*>(t)[i];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = gv[e] * sc;
            s0 += (double)gv[e] * (double)tv[e];
            s1 += (double)gv[e];
        }
        reinterpret_cast<f32x4*>(g_t)[i] = o;
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) {
        const float gv = g[i];
        g_t[i] = gv * sc;
        s0 += (double)gv * (double)t[i];
        s1 += (double)gv;
    }
    ft_block_partials(s0, s1, partials);
}

// x [B][H][W][C] -> y [B][H+2][W+2][C], padded pixel (py, px) = ELU(x[(py-1) mod H][(px-1) mod W] + a) + b
template <int VEC>
__global__ __launch_bounds__(FT_THREADS)
void ft_act_fwd_halo(const float* __restrict__ x, const float* __restrict__ pa, const float* __restrict__ pb, int B, int H,
                     int W, int C, float* __restrict__ y) {
    using P = typename Pack<VEC>::type;
    const float a = *pa, b = *pb;
    const int CV = C / VEC, PH = H + 2, PW = W + 2;
    const int64_t total = (int64_t)B * PH * PW * CV;
    for (int64_t i = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * FT_THREADS) {
        const int cv = (int)(i % CV);
        int64_t p = i / CV;
        const int px = (int)(p % PW); p /= PW;
        const int py = (int)(p % PH);
        const int bb = (int)(p / PH);
        const int ix = (px + W - 1) % W, iy = (py + H - 1) % H;       // px - 1 >= -1
        P v = *reinterpret_cast<const P*>(x + (((int64_t)bb * H + iy) * W + ix) * C + (int64_t)cv * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) lane_of<VEC>(v, e) = elu_train(lane_of<VEC>(v, e) + a) + b;
        *reinterpret_cast<P*>(y + i * VEC) = v;
    }
}

// g [B][H+2][W+2][C], x [B][H][W][C] -> g_x [B][H][W][C]; s0 = sum g_x, s1 = sum of the folded g (= the sum of all of g)
template <int VEC>
__global__ __launch_bounds__(FT_THREADS)
void ft_act_bwd_halo(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ pa, int B, int H,
                     int W, int C, float* __restrict__ g_x, double* __restrict__ partials) {
    using P = typename Pack<VEC>::type;
    const float a = *pa;
    const int CV = C / VEC, PW = W + 2;
    const int64_t total = (int64_t)B * H * W * CV;
    const int64_t prow = (int64_t)PW * C, pimg = (int64_t)(H + 2) * prow;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * FT_THREADS) {
        const int cv = (int)(i % CV);
        int64_t p = i / CV;
        const int ix = (int)(p % W); p /= W;
        const int iy = (int)(p % H);
        const int bb = (int)(p / H);
        const int64_t base = (int64_t)bb * pimg + (int64_t)cv * VEC;
        P fold;
#pragma unroll
        for (int e = 0; e < VEC; ++e) lane_of<VEC>(fold, e) = 0.f;
        // images of (iy, ix) in the padded grid: row iy + 1, row 0 if iy == H - 1, row H + 1 if iy == 0 (columns likewise)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const bool vy = dy == 0 || (dy == 1 && iy == H - 1) || (dy == 2 && iy == 0);
            const int py = dy == 0 ? iy + 1 : (dy == 1 ? 0 : H + 1);
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const bool vx = dx == 0 || (dx == 1 && ix == W - 1) || (dx == 2 && ix == 0);
                const int px = dx == 0 ? ix + 1 : (dx == 1 ? 0 : W + 1);
                if (vy && vx) {
                    P gv = *reinterpret_cast<const P*>(g + base + py * prow + (int64_t)px * C);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) lane_of<VEC>(fold, e) = lane_of<VEC>(fold, e) + lane_of<VEC>(gv, e);
                }
            }
        }
        P xv = *reinterpret_cast<const P*>(x + i * VEC);
        P o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float f = lane_of<VEC>(fold, e);
            const float r = f * elu_grad(lane_of<VEC>(xv, e) + a);
            lane_of<VEC>(o, e) = r;
            s0 += (double)r;
            s1 += (double)f;
        }
        *reinterpret_cast<P*>(g_x + i * VEC) = o;
    }
    ft_block_partials(s0, s1, partials);
}

// x [B][H][W][C] -> y [B][2H][2W][C]: per output the sums of vqae_bicubic_up2_f32 in its order (columns left to right per
// row, then rows top to bottom, unfused)
template <int VEC>
__global__ __launch_bounds__(FT_THREADS)
void ft_bicubic_fwd(const float* __restrict__ x, const float* __restrict__ ppb, int B, int H, int W, int C,
                    float* __restrict__ y) {
    using P = typename Pack<VEC>::type;
    const float pb = ppb ? *ppb : 0.f;
    const int CV = C / VEC, OH = 2 * H, OW = 2 * W;
    const int64_t total = (int64_t)B * OH * OW * CV;
    for (int64_t i = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * FT_THREADS) {
        const int cv = (int)(i % CV);
        int64_t p = i / CV;
        const int ox = (int)(p % OW); p /= OW;
        const int oy = (int)(p % OH);
        const int bb = (int)(p / OH);
        const bool oddx = ox & 1, oddy = oy & 1;
        const int bx = (ox >> 1) - (oddx ? 1 : 2), by = (oy >> 1) - (oddy ? 1 : 2);
        P out;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* row = x + (((int64_t)bb * H + clampi(by + r, H - 1)) * W) * C + (int64_t)cv * VEC;
            P h;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                P v = *reinterpret_cast<const P*>(row + (int64_t)clampi(bx + j, W - 1) * C);
                const float wx = oddx ? tap25(j) : tap75(j);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float q = (lane_of<VEC>(v, e) + pb) * wx;
                    lane_of<VEC>(h, e) = j == 0 ? q : lane_of<VEC>(h, e) + q;
                }
            }
            const float wy = oddy ? tap25(r) : tap75(r);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float q = lane_of<VEC>(h, e) * wy;
                lane_of<VEC>(out, e) = r == 0 ? q : lane_of<VEC>(out, e) + q;
            }
        }
        *reinterpret_cast<P*>(y + i * VEC) = out;
    }
}

// g [B][2H][2W][C] -> g_x [B][H][W][C] = up^T g; s0 = sum g_x
template <int VEC>
__global__ __launch_bounds__(FT_THREADS)
void ft_bicubic_bwd(const float* __restrict__ g, int B, int H, int W, int C, float* __restrict__ g_x,
                    double* __restrict__ partials) {
    using P = typename Pack<VEC>::type;
    const int CV = C / VEC, OH = 2 * H, OW = 2 * W;
    const int64_t total = (int64_t)B * H * W * CV;
    double s0 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * FT_THREADS) {
        const int cv = (int)(i % CV);
        int64_t p = i / CV;
        const int ix = (int)(p % W); p /= W;
        const int iy = (int)(p % H);
        const int bb = (int)(p / H);
        float ax[8], ay[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {                    // outputs 2i-3 .. 2i+4: every output whose clamped taps can reach i
            const int oy = 2 * iy - 3 + r, ox = 2 * ix - 3 + r;
            ay[r] = (oy >= 0 && oy < OH) ? axis_weight(oy, iy, H) : 0.f;
            ax[r] = (ox >= 0 && ox < OW) ? axis_weight(ox, ix, W) : 0.f;
        }
        P acc;
#pragma unroll
        for (int e = 0; e < VEC; ++e) lane_of<VEC>(acc, e) = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (ay[r] == 0.f) continue;                  // outside the grid, or no tap of this output reaches iy
            const float* row = g + (((int64_t)bb * OH + (2 * iy - 3 + r)) * OW) * C + (int64_t)cv * VEC;
            P h;
#pragma unroll
            for (int e = 0; e < VEC; ++e) lane_of<VEC>(h, e) = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                if (ax[c] == 0.f) continue;
                P gv = *reinterpret_cast<const P*>(row + (int64_t)(2 * ix - 3 + c) * C);
#pragma unroll
                for (int e = 0; e < VEC; ++e) lane_of<VEC>(h, e) = lane_of<VEC>(h, e) + lane_of<VEC>(gv, e) * ax[c];
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) lane_of<VEC>(acc, e) = lane_of<VEC>(acc, e) + lane_of<VEC>(h, e) * ay[r];
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) s0 += (double)lane_of<VEC>(acc, e);
        *reinterpret_cast<P*>(g_x + i * VEC) = acc;
    }
    ft_block_partials(s0, 0.0, partials);
}

}  // namespace

extern "C" size_t vqae_fixup_train_workspace_bytes(int64_t n_elems) {
    return (size_t)ft_grid(n_elems > 0 ? n_elems : 1) * FT_SUMS * sizeof(double) + 256;
}

extern "C" int vqae_fixup_act_f32(const float* x, const float* a, const float* b, int act, int halo, int B, int H, int W, int C,
                                  float* y, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_dims("fixup_act", B, H, W, C, 1)) return rc;
    VQAE_REQUIRE(x && y && b && (a || !act), VQAE_ERR_INVALID, "fixup_act: null pointer");
    VQAE_REQUIRE((halo == 0 || halo == 1) && (act == 0 || act == 1), VQAE_ERR_INVALID, "fixup_act: act %d halo %d", act, halo);
    VQAE_REQUIRE(act || !halo, VQAE_ERR_UNSUPPORTED, "fixup_act: the plain mode (y = x + c) has no halo form");
    if (halo) {
        const bool vec = C % 4 == 0 && aligned16({x, y});
        const int64_t items = (int64_t)B * (H + 2) * (W + 2) * (vec ? C / 4 : C);
        if (vec) ft_act_fwd_halo<4><<<ft_grid(items), FT_THREADS, 0, stream>>>(x, a, b, B, H, W, C, y);
        else ft_act_fwd_halo<1><<<ft_grid(items), FT_THREADS, 0, stream>>>(x, a, b, B, H, W, C, y);
    } else {
        const int64_t n = (int64_t)B * H * W * C, n4 = aligned16({x, y}) ? n / 4 : 0;
        const int grid = ft_grid(n4 > 0 ? n4 : n);
        if (act) ft_act_fwd_flat<true><<<grid, FT_THREADS, 0, stream>>>(x, a, b, n, n4, y);
        else ft_act_fwd_flat<false><<<grid, FT_THREADS, 0, stream>>>(x, nullptr, b, n, n4, y);
    }
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" int vqae_fixup_act_backward_f32(const float* g, const float* x, const float* a, int act, int halo, int B, int H, int W,
                                           int C, float* g_x, float* g_a, float* g_b, void* ws, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_dims("fixup_act_backward", B, H, W, C, 1)) return rc;
    VQAE_REQUIRE((halo == 0 || halo == 1) && (act == 0 || act == 1), VQAE_ERR_INVALID, "fixup_act_backward: act %d halo %d", act,
                 halo);
    VQAE_REQUIRE(act || !halo, VQAE_ERR_UNSUPPORTED, "fixup_act_backward: the plain mode (y = x + c) has no halo form");
    VQAE_REQUIRE(g && ws && (!act || (x && a && g_x)), VQAE_ERR_INVALID, "fixup_act_backward: null pointer");
    VQAE_REQUIRE(((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID, "fixup_act_backward: workspace must be 8-byte aligned");
    double* partials = (double*)ws;
    int grid;
    if (halo) {
        const bool vec = C % 4 == 0 && aligned16({g, x, g_x});
        grid = ft_grid((int64_t)B * H * W * (vec ? C / 4 : C));
        if (vec) ft_act_bwd_halo<4><<<grid, FT_THREADS, 0, stream>>>(g, x, a, B, H, W, C, g_x, partials);
        else ft_act_bwd_halo<1><<<grid, FT_THREADS, 0, stream>>>(g, x, a, B, H, W, C, g_x, partials);
    } else {
        const int64_t n = (int64_t)B * H * W * C, n4 = aligned16({g, x, g_x}) ? n / 4 : 0;
        grid = ft_grid(n4 > 0 ? n4 : n);
        if (act) ft_act_bwd_flat<true><<<grid, FT_THREADS, 0, stream>>>(g, x, a, n, n4, g_x, partials);
        else ft_act_bwd_flat<false><<<grid, FT_THREADS, 0, stream>>>(g, nullptr, nullptr, n, n4, nullptr, partials);
    }
    VQAE_LAUNCH_CHECK();
    return finish_sums(partials, grid, act ? g_a : nullptr, nullptr, g_b, nullptr, stream);
}

extern "C" int vqae_fixup_out_f32(const float* t, const float* skip, const float* scale, const float* bias4, const float* bias1d,
                                  int64_t n, float* y, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VQAE_REQUIRE(n >= 1 && n < (1ll << 40), VQAE_ERR_INVALID, "fixup_out: %lld elements", (long long)n);
    VQAE_REQUIRE(t && skip && scale && bias4 && y, VQAE_ERR_INVALID, "fixup_out: null pointer");
    const int64_t n4 = aligned16({t, skip, y}) ? n / 4 : 0;
    ft_out_fwd<<<ft_grid(n4 > 0 ? n4 : n), FT_THREADS, 0, stream>>>(t, skip, scale, bias4, bias1d, n, n4, y);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" int vqae_fixup_out_backward_f32(const float* g, const float* t, const float* scale, int64_t n, float* g_t,
                                           float* g_scale, float* g_bias4, float* g_bias1d, void* ws, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VQAE_REQUIRE(n >= 1 && n < (1ll << 40), VQAE_ERR_INVALID, "fixup_out_backward: %lld elements", (long long)n);
    VQAE_REQUIRE(g && t && scale && g_t && ws, VQAE_ERR_INVALID, "fixup_out_backward: null pointer");
    VQAE_REQUIRE(((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID, "fixup_out_backward: workspace must be 8-byte aligned");
    const int64_t n4 = aligned16({g, t, g_t}) ? n / 4 : 0;
    const int grid = ft_grid(n4 > 0 ? n4 : n);
    ft_out_bwd<<<grid, FT_THREADS, 0, stream>>>(g, t, scale, n, n4, g_t, (double*)ws);
    VQAE_LAUNCH_CHECK();
    return finish_sums((double*)ws, grid, g_scale, nullptr, g_bias4, g_bias1d, stream);
}

extern "C" int vqae_bicubic_up2_bias_f32(const float* x, int B, int H, int W, int C, const float* pre_bias, float* y,
                                         void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_dims("bicubic_up2_bias", B, H, W, C, 4)) return rc;
    VQAE_REQUIRE(x && y, VQAE_ERR_INVALID, "bicubic_up2_bias: null pointer");
    const bool vec = C % 4 == 0 && aligned16({x, y});
    const int64_t items = (int64_t)B * 4 * H * W * (vec ? C / 4 : C);
    if (vec) ft_bicubic_fwd<4><<<ft_grid(items), FT_THREADS, 0, stream>>>(x, pre_bias, B, H, W, C, y);
    else ft_bicubic_fwd<1><<<ft_grid(items), FT_THREADS, 0, stream>>>(x, pre_bias, B, H, W, C, y);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" int vqae_bicubic_up2_backward_f32(const float* g, int B, int H, int W, int C, float* g_x, float* g_pre_bias, void* ws,
                                             void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_dims("bicubic_up2_backward", B, H, W, C, 4)) return rc;
    VQAE_REQUIRE(g && g_x && ws, VQAE_ERR_INVALID, "bicubic_up2_backward: null pointer");
    VQAE_REQUIRE(((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID, "bicubic_up2_backward: workspace must be 8-byte aligned");
    const bool vec = C % 4 == 0 && aligned16({g, g_x});
    const int grid = ft_grid((int64_t)B * H * W * (vec ? C / 4 : C));
    if (vec) ft_bicubic_bwd<4><<<grid, FT_THREADS, 0, stream>>>(g, B, H, W, C, g_x, (double*)ws);
    else ft_bicubic_bwd<1><<<grid, FT_THREADS, 0, stream>>>(g, B, H, W, C, g_x, (double*)ws);
    VQAE_LAUNCH_CHECK();
    return finish_sums((double*)ws, grid, g_pre_bias, nullptr, nullptr, nullptr, stream);
}
