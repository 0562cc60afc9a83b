// Mixed-precision forms of the three element-wise nodes of fixup_train.hip (act / plain, out), forward and backward, for
// training under 16-bit autocast: every tensor of a call is fp32 or ONE 16-bit type (bf16 or f16), stated per tensor by a
// VQAE_DT_* code.  A node that reads a conv output (16-bit under autocast) and feeds a conv (which rounds its input to 16
// bits) reads 2 bytes and writes 2 bytes per element, where the fp32 kernel between two casts moves 20.
//
// Arithmetic: the values are up-cast on load (exact), the fp32 arithmetic is that of fixup_train.hip (elu_train, elu_grad,
// the same operations in the same order), and a 16-bit result is rounded once on store with round_to<DT> (mfma.h): every
// output is bit for bit the fp32 entry point on the up-cast inputs followed by torch's cast.  inf / NaN pass through as
// through torch's ops (a GradScaler's overflow check sees them).
//
// Sums: the UNROUNDED fp32 terms, in fp64, through ft_block_partials / ft_final.  The element-to-thread order is the fp32
// kernels': items of 4 elements (one 16-byte access of an fp32 tensor, one 8-byte access of a 16-bit one), the same grid
// for the same shape, the same tail -- so the sums are the fp32 entry points' bit for bit where both take the vector path.
// The vector path needs every tensor of the call aligned to its 4-element access (16 / 8 bytes); a 16-bit view can start on
// a 2-byte boundary, and then the call takes the scalar path, as the fp32 kernels do.  No atomics, a grid that depends on the
// shape alone: bit-identical run to run.
//
// A call whose tensors are all fp32 is forwarded to the _f32 entry point.
#include "fixup_train_impl.h"
#include "io_dtype.h"

namespace {

using namespace vqae;
using namespace vqae::ft;

constexpr int FT_MAX_WG = 1024;          // rows of fp64 partials, as in fixup_train.hip

inline int ft_grid(int64_t items) {
    return (int)std::min<int64_t>(FT_MAX_WG, std::max<int64_t>(1, ceil_div(items, FT_THREADS)));
}

// VEC consecutive elements at element offset `off` (VEC = 4: off % 4 == 0 and an aligned base) -> the first VEC lanes
template <int DT, int VEC> __device__ __forceinline__ f32x4 ldv(const typename Io<DT>::elem* p, int64_t off) {
    if constexpr (VEC == 4) {
        return Io<DT>::ld4(p, off >> 2);
    } else {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        v[0] = Io<DT>::ld(p, off);
        return v;
    }
}
template <int DT, int VEC> __device__ __forceinline__ void stv(typename Io<DT>::elem* p, int64_t off, const f32x4& v) {
    if constexpr (VEC == 4) Io<DT>::st4(p, off >> 2, v);
    else Io<DT>::st(p, off, v[0]);
}

// ---- flat forms: n4 4-element groups, then the tail [4 n4, n) ---------------------------------------------------------------
template <bool ACT, int DX, int DY>
__global__ __launch_bounds__(FT_THREADS)
void ftio_act_fwd_flat(const typename Io<DX>::elem* __restrict__ x, const float* __restrict__ pa, const float* __restrict__ pb,
                       int64_t n, int64_t n4, typename Io<DY>::elem* __restrict__ y) {
    const float a = ACT ? *pa : 0.f, b = *pb;
    const int64_t stride = (int64_t)gridDim.x * FT_THREADS, t0 = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    for (int64_t i = t0; i < n4; i += stride) {
        f32x4 v = Io<DX>::ld4(x, i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ACT ? elu_train(v[e] + a) + b : v[e] + b;
        Io<DY>::st4(y, i, v);
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) {
        const float v = Io<DX>::ld(x, i);
        Io<DY>::st(y, i, ACT ? elu_train(v + a) + b : v + b);
    }
}

// g has y's dtype DY, x and g_x have DX.  ACT: g_x = g * ELU'(x + a), s0 = sum g_x (unrounded), s1 = sum g.
// Plain: s1 = sum g; g_x = g is written (one rounding) only where WRITE (DX != DY: otherwise it is the incoming tensor).
template <bool ACT, bool WRITE, int DX, int DY>
__global__ __launch_bounds__(FT_THREADS)
void ftio_act_bwd_flat(const typename Io<DY>::elem* __restrict__ g, const typename Io<DX>::elem* __restrict__ x,
                       const float* __restrict__ pa, int64_t n, int64_t n4, typename Io<DX>::elem* __restrict__ g_x,
                       double* __restrict__ partials) {
    const float a = ACT ? *pa : 0.f;
    const int64_t stride = (int64_t)gridDim.x * FT_THREADS, t0 = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t i = t0; i < n4; i += stride) {
        const f32x4 gv = Io<DY>::ld4(g, i);
        if constexpr (ACT) {
            const f32x4 xv = Io<DX>::ld4(x, i);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = gv[e] * elu_grad(xv[e] + a);
                s0 += (double)o[e];
                s1 += (double)gv[e];
            }
            Io<DX>::st4(g_x, i, o);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) s1 += (double)gv[e];
            if constexpr (WRITE) Io<DX>::st4(g_x, i, gv);
        }
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) {
        const float gv = Io<DY>::ld(g, i);
        if constexpr (ACT) {
            const float o = gv * elu_grad(Io<DX>::ld(x, i) + a);
            Io<DX>::st(g_x, i, o);
            s0 += (double)o;
        } else if constexpr (WRITE) {
            Io<DX>::st(g_x, i, gv);
        }
        s1 += (double)gv;
    }
    ft_block_partials(s0, s1, partials);
}

template <int DT, int DS>
__global__ __launch_bounds__(FT_THREADS)
void ftio_out_fwd(const typename Io<DT>::elem* __restrict__ t, const typename Io<DS>::elem* __restrict__ skip,
                  const float* __restrict__ pscale, const float* __restrict__ pb4, const float* __restrict__ pb1d, int64_t n,
                  int64_t n4, float* __restrict__ y) {
    const float sc = *pscale, b4 = *pb4;
    const bool has_d = pb1d != nullptr;
    const float b1d = has_d ? *pb1d : 0.f;
    const int64_t stride = (int64_t)gridDim.x * FT_THREADS, t0 = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    for (int64_t i = t0; i < n4; i += stride) {
        const f32x4 tv = Io<DT>::ld4(t, i), sv = Io<DS>::ld4(skip, i);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (tv[e] * sc + b4) + (has_d ? sv[e] + b1d : sv[e]);
        reinterpret_cast<f32x4*>(y)[i] = o;
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) {
        const float tv = Io<DT>::ld(t, i), sv = Io<DS>::ld(skip, i);
        y[i] = (tv * sc + b4) + (has_d ? sv + b1d : sv);
    }
}

// g fp32.  g_t (DT) = g * scale, s0 = sum g * t, s1 = sum g; a 16-bit skip (DS) gets its copy of g in the same pass.
template <int DT, int DS>
__global__ __launch_bounds__(FT_THREADS)
void ftio_out_bwd(const float* __restrict__ g, const typename Io<DT>::elem* __restrict__ t, const float* __restrict__ pscale,
                  int64_t n, int64_t n4, typename Io<DT>::elem* __restrict__ g_t, typename Io<DS>::elem* __restrict__ g_skip,
                  double* __restrict__ partials) {
    const float sc = *pscale;
    const int64_t stride = (int64_t)gridDim.x * FT_THREADS, t0 = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t i = t0; i < n4; i += stride) {
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i], tv = Io<DT>::ld4(t, i);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = gv[e] * sc;
            s0 += (double)gv[e] * (double)tv[e];
            s1 += (double)gv[e];
        }
        Io<DT>::st4(g_t, i, o);
        if constexpr (DS != VQAE_DT_F32) Io<DS>::st4(g_skip, i, gv);
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) {
        const float gv = g[i];
        Io<DT>::st(g_t, i, gv * sc);
        if constexpr (DS != VQAE_DT_F32) Io<DS>::st(g_skip, i, gv);
        s0 += (double)gv * (double)Io<DT>::ld(t, i);
        s1 += (double)gv;
    }
    ft_block_partials(s0, s1, partials);
}

// ---- halo forms: one thread = one pixel x VEC channels ----------------------------------------------------------------------
// x [B][H][W][C] -> y [B][H+2][W+2][C], padded pixel (py, px) = ELU(x[(py-1) mod H][(px-1) mod W] + a) + b
template <int VEC, int DX, int DY>
__global__ __launch_bounds__(FT_THREADS)
void ftio_act_fwd_halo(const typename Io<DX>::elem* __restrict__ x, const float* __restrict__ pa, const float* __restrict__ pb,
                       int B, int H, int W, int C, typename Io<DY>::elem* __restrict__ y) {
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
        f32x4 v = ldv<DX, VEC>(x, (((int64_t)bb * H + iy) * W + ix) * C + (int64_t)cv * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = elu_train(v[e] + a) + b;
        stv<DY, VEC>(y, i * VEC, v);
    }
}

// g [B][H+2][W+2][C] (DY), x [B][H][W][C] (DX) -> g_x [B][H][W][C] (DX); s0 = sum g_x (unrounded), s1 = sum of the folded g
template <int VEC, int DX, int DY>
__global__ __launch_bounds__(FT_THREADS)
void ftio_act_bwd_halo(const typename Io<DY>::elem* __restrict__ g, const typename Io<DX>::elem* __restrict__ x,
                       const float* __restrict__ pa, int B, int H, int W, int C, typename Io<DX>::elem* __restrict__ g_x,
                       double* __restrict__ partials) {
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
        f32x4 fold = {0.f, 0.f, 0.f, 0.f};
        // images of (iy, ix) in the padded grid, in the order of ft_act_bwd_halo: the fp32 fold adds in that order
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const bool vy = dy == 0 || (dy == 1 && iy == H - 1) || (dy == 2 && iy == 0);
            const int py = dy == 0 ? iy + 1 : (dy == 1 ? 0 : H + 1);
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const bool vx = dx == 0 || (dx == 1 && ix == W - 1) || (dx == 2 && ix == 0);
                const int px = dx == 0 ? ix + 1 : (dx == 1 ? 0 : W + 1);
                if (vy && vx) {
                    const f32x4 gv = ldv<DY, VEC>(g, base + py * prow + (int64_t)px * C);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) fold[e] = fold[e] + gv[e];
                }
            }
        }
        const f32x4 xv = ldv<DX, VEC>(x, i * VEC);
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float r = fold[e] * elu_grad(xv[e] + a);
            o[e] = r;
            s0 += (double)r;
            s1 += (double)fold[e];
        }
        stv<DX, VEC>(g_x, i * VEC, o);
    }
    ft_block_partials(s0, s1, partials);
}

// ---- host: dtype codes -> instantiations ---------------------------------------------------------------------------------------
// f(DtC<d0>, DtC<d1>) for a pair of codes of which at least one is 16-bit and which hold one 16-bit type (checked by the caller)
template <typename F> inline void for_pair(int d0, int d1, F&& f) {
    const int t16 = dt_16(d0) ? d0 : d1;
    if (t16 == VQAE_DT_BF16) {
        if (!dt_16(d0)) f(DtC<VQAE_DT_F32>{}, DtC<VQAE_DT_BF16>{});
        else if (!dt_16(d1)) f(DtC<VQAE_DT_BF16>{}, DtC<VQAE_DT_F32>{});
        else f(DtC<VQAE_DT_BF16>{}, DtC<VQAE_DT_BF16>{});
    } else {
        if (!dt_16(d0)) f(DtC<VQAE_DT_F32>{}, DtC<VQAE_DT_F16>{});
        else if (!dt_16(d1)) f(DtC<VQAE_DT_F16>{}, DtC<VQAE_DT_F32>{});
        else f(DtC<VQAE_DT_F16>{}, DtC<VQAE_DT_F16>{});
    }
}

inline int check_pair(const char* who, const char* n0, int d0, const char* n1, int d1) {
    VQAE_REQUIRE(dt_ok(d0) && dt_ok(d1), VQAE_ERR_INVALID, "%s: dtype codes %s %d, %s %d", who, n0, d0, n1, d1);
    VQAE_REQUIRE(!(dt_16(d0) && dt_16(d1) && d0 != d1), VQAE_ERR_UNSUPPORTED,
                 "%s: %s and %s are two different 16-bit types (%d, %d); a call takes at most one", who, n0, n1, d0, d1);
    return VQAE_OK;
}

}  // namespace

extern "C" int vqae_fixup_act_io(const void* x, int x_dt, const float* a, const float* b, int act, int halo, int B, int H, int W,
                                 int C, void* y, int y_dt, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_pair("fixup_act_io", "x", x_dt, "y", y_dt)) return rc;
    if (x_dt == VQAE_DT_F32 && y_dt == VQAE_DT_F32)
        return vqae_fixup_act_f32((const float*)x, a, b, act, halo, B, H, W, C, (float*)y, stream_);
    if (int rc = check_dims("fixup_act_io", B, H, W, C, 1)) return rc;
    VQAE_REQUIRE(x && y && b && (a || !act), VQAE_ERR_INVALID, "fixup_act_io: null pointer");
    VQAE_REQUIRE((halo == 0 || halo == 1) && (act == 0 || act == 1), VQAE_ERR_INVALID, "fixup_act_io: act %d halo %d", act, halo);
    VQAE_REQUIRE(act || !halo, VQAE_ERR_UNSUPPORTED, "fixup_act_io: the plain mode (y = x + c) has no halo form");
    const bool al = aligned_vec({{x, x_dt}, {y, y_dt}});
    for_pair(x_dt, y_dt, [&](auto dx, auto dy) {
        constexpr int DX = decltype(dx)::value, DY = decltype(dy)::value;
        auto xp = (const typename Io<DX>::elem*)x;
        auto yp = (typename Io<DY>::elem*)y;
        if (halo) {
            const bool vec = C % 4 == 0 && al;
            const int64_t items = (int64_t)B * (H + 2) * (W + 2) * (vec ? C / 4 : C);
            if (vec) ftio_act_fwd_halo<4, DX, DY><<<ft_grid(items), FT_THREADS, 0, stream>>>(xp, a, b, B, H, W, C, yp);
            else ftio_act_fwd_halo<1, DX, DY><<<ft_grid(items), FT_THREADS, 0, stream>>>(xp, a, b, B, H, W, C, yp);
        } else {
            const int64_t n = (int64_t)B * H * W * C, n4 = al ? n / 4 : 0;
            const int grid = ft_grid(n4 > 0 ? n4 : n);
            if (act) ftio_act_fwd_flat<true, DX, DY><<<grid, FT_THREADS, 0, stream>>>(xp, a, b, n, n4, yp);
            else ftio_act_fwd_flat<false, DX, DY><<<grid, FT_THREADS, 0, stream>>>(xp, nullptr, b, n, n4, yp);
        }
    });
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" int vqae_fixup_act_backward_io(const void* g, int g_dt, const void* x, int x_dt, const float* a, int act, int halo,
                                          int B, int H, int W, int C, void* g_x, float* g_a, float* g_b, void* ws,
                                          void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_pair("fixup_act_backward_io", "g", g_dt, "x", x_dt)) return rc;
    if (g_dt == VQAE_DT_F32 && x_dt == VQAE_DT_F32)
        return vqae_fixup_act_backward_f32((const float*)g, (const float*)x, a, act, halo, B, H, W, C, (float*)g_x, g_a, g_b, ws,
                                           stream_);
    if (int rc = check_dims("fixup_act_backward_io", B, H, W, C, 1)) return rc;
    VQAE_REQUIRE((halo == 0 || halo == 1) && (act == 0 || act == 1), VQAE_ERR_INVALID, "fixup_act_backward_io: act %d halo %d",
                 act, halo);
    VQAE_REQUIRE(act || !halo, VQAE_ERR_UNSUPPORTED, "fixup_act_backward_io: the plain mode (y = x + c) has no halo form");
    const bool write = act || g_dt != x_dt;              // plain, equal dtypes: g_x is the incoming tensor itself
    VQAE_REQUIRE(g && ws && (!act || (x && a)) && (!write || g_x), VQAE_ERR_INVALID, "fixup_act_backward_io: null pointer");
    VQAE_REQUIRE(((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID, "fixup_act_backward_io: workspace must be 8-byte aligned");
    double* partials = (double*)ws;
    int grid = 1;
    // pointers a form does not read or write (x of the plain mode, g_x where nothing is written) do not decide the path
    const bool al = aligned_vec({{g, g_dt}, {act ? x : nullptr, x_dt}, {write ? g_x : nullptr, x_dt}});
    for_pair(x_dt, g_dt, [&](auto dx, auto dy) {
        constexpr int DX = decltype(dx)::value, DY = decltype(dy)::value;
        auto gp = (const typename Io<DY>::elem*)g;
        auto xp = (const typename Io<DX>::elem*)x;
        auto gxp = (typename Io<DX>::elem*)g_x;
        if (halo) {
            const bool vec = C % 4 == 0 && al;
            grid = ft_grid((int64_t)B * H * W * (vec ? C / 4 : C));
            if (vec) ftio_act_bwd_halo<4, DX, DY><<<grid, FT_THREADS, 0, stream>>>(gp, xp, a, B, H, W, C, gxp, partials);
            else ftio_act_bwd_halo<1, DX, DY><<<grid, FT_THREADS, 0, stream>>>(gp, xp, a, B, H, W, C, gxp, partials);
        } else {
            const int64_t n = (int64_t)B * H * W * C, n4 = al ? n / 4 : 0;
            grid = ft_grid(n4 > 0 ? n4 : n);
            if (act)
                ftio_act_bwd_flat<true, true, DX, DY><<<grid, FT_THREADS, 0, stream>>>(gp, xp, a, n, n4, gxp, partials);
            else if (write)
                ftio_act_bwd_flat<false, true, DX, DY><<<grid, FT_THREADS, 0, stream>>>(gp, nullptr, nullptr, n, n4, gxp, partials);
            else
                ftio_act_bwd_flat<false, false, DX, DY><<<grid, FT_THREADS, 0, stream>>>(gp, nullptr, nullptr, n, n4, nullptr,
                                                                                        partials);
        }
    });
    VQAE_LAUNCH_CHECK();
    return finish_sums(partials, grid, act ? g_a : nullptr, nullptr, g_b, nullptr, stream);
}

extern "C" int vqae_fixup_out_io(const void* t, int t_dt, const void* skip, int skip_dt, const float* scale, const float* bias4,
                                 const float* bias1d, int64_t n, void* y, int y_dt, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_pair("fixup_out_io", "t", t_dt, "skip", skip_dt)) return rc;
    VQAE_REQUIRE(dt_ok(y_dt), VQAE_ERR_INVALID, "fixup_out_io: dtype code y %d", y_dt);
    VQAE_REQUIRE(y_dt == VQAE_DT_F32, VQAE_ERR_UNSUPPORTED,
                 "fixup_out_io: y is the residual stream and stays fp32 (dtype code %d)", y_dt);
    if (t_dt == VQAE_DT_F32 && skip_dt == VQAE_DT_F32)
        return vqae_fixup_out_f32((const float*)t, (const float*)skip, scale, bias4, bias1d, n, (float*)y, stream_);
    VQAE_REQUIRE(n >= 1 && n < (1ll << 40), VQAE_ERR_INVALID, "fixup_out_io: %lld elements", (long long)n);
    VQAE_REQUIRE(t && skip && scale && bias4 && y, VQAE_ERR_INVALID, "fixup_out_io: null pointer");
    const int64_t n4 = aligned_vec({{t, t_dt}, {skip, skip_dt}, {y, y_dt}}) ? n / 4 : 0;
    const int grid = ft_grid(n4 > 0 ? n4 : n);
    for_pair(t_dt, skip_dt, [&](auto dt, auto ds) {
        constexpr int DT = decltype(dt)::value, DS = decltype(ds)::value;
        ftio_out_fwd<DT, DS><<<grid, FT_THREADS, 0, stream>>>((const typename Io<DT>::elem*)t, (const typename Io<DS>::elem*)skip,
                                                              scale, bias4, bias1d, n, n4, (float*)y);
    });
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" int vqae_fixup_out_backward_io(const float* g, const void* t, int t_dt, const float* scale, int64_t n, void* g_t,
                                          void* g_skip, int skip_dt, float* g_scale, float* g_bias4, float* g_bias1d, void* ws,
                                          void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_pair("fixup_out_backward_io", "t", t_dt, "skip", skip_dt)) return rc;
    if (t_dt == VQAE_DT_F32 && skip_dt == VQAE_DT_F32)
        return vqae_fixup_out_backward_f32(g, (const float*)t, scale, n, (float*)g_t, g_scale, g_bias4, g_bias1d, ws, stream_);
    VQAE_REQUIRE(n >= 1 && n < (1ll << 40), VQAE_ERR_INVALID, "fixup_out_backward_io: %lld elements", (long long)n);
    VQAE_REQUIRE(g && t && scale && g_t && ws && (g_skip || !dt_16(skip_dt)), VQAE_ERR_INVALID,
                 "fixup_out_backward_io: null pointer");
    VQAE_REQUIRE(((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID, "fixup_out_backward_io: workspace must be 8-byte aligned");
    const int64_t n4 = aligned_vec({{g, VQAE_DT_F32}, {t, t_dt}, {g_t, t_dt}, {dt_16(skip_dt) ? g_skip : nullptr, skip_dt}})
                           ? n / 4 : 0;
    const int grid = ft_grid(n4 > 0 ? n4 : n);
    for_pair(t_dt, skip_dt, [&](auto dt, auto ds) {
        constexpr int DT = decltype(dt)::value, DS = decltype(ds)::value;
        ftio_out_bwd<DT, DS><<<grid, FT_THREADS, 0, stream>>>(g, (const typename Io<DT>::elem*)t, scale, n, n4,
                                                              (typename Io<DT>::elem*)g_t, (typename Io<DS>::elem*)g_skip,
                                                              (double*)ws);
    });
    VQAE_LAUNCH_CHECK();
    return finish_sums((double*)ws, grid, g_scale, nullptr, g_bias4, g_bias1d, stream);
}
