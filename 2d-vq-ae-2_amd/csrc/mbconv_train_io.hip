// Mixed-precision forms of the three nodes of mbconv_train.hip (bn_act, dwconv, se_scale), forward and backward, for training
// under 16-bit autocast.  Under autocast every activation tensor of an MBConv block is 16-bit -- the conv outputs, the
// BatchNorm and SiLU outputs, the SE product, the residual stream -- so the [B][H][W][C] tensors of a call (x, y, g, g_x)
// share ONE dtype T (VQAE_DT_BF16 or VQAE_DT_F16; all fp32: the call is forwarded to the _f32 entry).  The small tensors stay
// what they are in mbconv_train.hip: gamma, beta, the running statistics, pool, g_pool, g_gamma, g_beta, g_w fp32; mean,
// invstd and the partial rows fp64.  gate and g_gate have a dtype code of their own, fp32 or T: under autocast the gate leaves
// a Linear as 16-bit.
//
// Layout: the fp32 kernels' element-to-thread order.  One 4-channel item per lane (8 bytes of a 16-bit type where the fp32
// kernels read 16), (pl, cg) = (tid / C4, tid % C4), MBT_ROWS rows per workgroup, the same grids, the same finishing launch.
//
// Arithmetic: values are up-cast on load (exact); the fp32 / fp64 arithmetic is mbconv_train.hip's operation for operation;
// the fp64 sums are taken from the UNROUNDED fp32 terms in the same order, so every sum (mean, invstd, the running
// statistics, pool, g_gamma, g_beta, g_w, g_gate) equals the fp32 entry's on the up-cast inputs bit for bit; a 16-bit result
// is rounded ONCE on store (Io16::rnd, io_dtype.h).  One rounding per node: stock torch rounds z to 16 bits between BatchNorm
// and SiLU and again behind SiLU, the fused node rounds y only, and the backward recomputes z from the saved x in fp32.
//
// dwconv: the module's fp32 weight is read in place and each tap rounded to T in registers (autocast casts the conv weight),
// in the forward and in the gathered data gradient; g_w is the fixed-order fp64 sum, rounded once to fp32, in w's shape.
//
// Alignment: a 16-bit [B][H][W][C] tensor (and a 16-bit gate) on 8 bytes, an fp32 one on 16; anything else is
// VQAE_ERR_INVALID.  Two different 16-bit types in one call: VQAE_ERR_UNSUPPORTED.  inf / NaN pass through as through torch's ops.
#include "mbconv_train_impl.h"
#include "io_dtype.h"

namespace {

using namespace vqae;
using namespace vqae::mbt;

template <int DT> using El = typename Io<DT>::elem;

// ---- BatchNorm --------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(MBT_THREADS)
void bn_stats_io(const El<DT>* __restrict__ x, int64_t M, int C4, double* __restrict__ partials) {
    const Lane l = lane_of_thread(C4);
    const int64_t p0 = (int64_t)blockIdx.x * MBT_ROWS, p_end = min(p0 + MBT_ROWS, M);
    double acc[2][4] = {};
    if (l.live) {
        const f32x4 sh = Io<DT>::ld4(x, l.cg);
        for (int64_t p = p0 + l.pl; p < p_end; p += l.PL) {
            const f32x4 v = Io<DT>::ld4(x, p * C4 + l.cg);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)v[e] - (double)sh[e];
                acc[0][e] += d;
                acc[1][e] += d * d;
            }
        }
    }
    block_rows<2>(acc, l, C4, partials + (int64_t)blockIdx.x * 2 * C4 * 4);
}

template <int DT>
__global__ __launch_bounds__(MBT_THREADS)
void bn_finish_io(const double* __restrict__ partials, int n_rows, const El<DT>* __restrict__ x, int64_t M, int C,
                  double momentum, double eps, float* __restrict__ running_mean, float* __restrict__ running_var,
                  double* __restrict__ mean, double* __restrict__ invstd) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;                                          // wave-uniform
    const double s1 = column_sum(partials, n_rows, 2 * C, c, lane);
    const double s2 = column_sum(partials, n_rows, 2 * C, C + c, lane);
    if (lane != 0) return;
    const double m1 = s1 / (double)M;
    const double mu = (double)Io<DT>::ld(x, c) + m1;
    const double var = fmax(s2 / (double)M - m1 * m1, 0.0);
    mean[c] = mu;
    invstd[c] = 1.0 / sqrt(var + eps);
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mu);
    if (running_var)
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (var * ((double)M / (double)(M - 1))));
}

template <int DT>
__global__ __launch_bounds__(MBT_THREADS)
void bn_apply_io(const El<DT>* __restrict__ x, const double* __restrict__ mean, const double* __restrict__ invstd,
                 const f32x4* __restrict__ gamma, const f32x4* __restrict__ beta, int act, int64_t HW, int C4,
                 El<DT>* __restrict__ y, double* __restrict__ pool_partials) {
    const Lane l = lane_of_thread(C4);
    const int64_t base = (int64_t)blockIdx.y * HW;
    const int64_t p0 = (int64_t)blockIdx.x * MBT_ROWS, p_end = min(p0 + MBT_ROWS, HW);
    double acc[1][4] = {};
    if (l.live) {
        const f32x4 ga = gamma[l.cg], be = beta[l.cg];
        f32x4 mu, is;
#pragma unroll
        for (int e = 0; e < 4; ++e) { mu[e] = (float)mean[l.cg * 4 + e]; is[e] = (float)invstd[l.cg * 4 + e]; }
        for (int64_t p = p0 + l.pl; p < p_end; p += l.PL) {
            const f32x4 v = Io<DT>::ld4(x, (base + p) * C4 + l.cg);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float z = (v[e] - mu[e]) * is[e] * ga[e] + be[e];
                o[e] = act ? silu1(z) : z;
                acc[0][e] += (double)o[e];                       // the unrounded fp32 term
            }
            Io<DT>::st4(y, (base + p) * C4 + l.cg, o);
        }
    }
    if (pool_partials) block_rows<1>(acc, l, C4, pool_partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * C4 * 4);
}

struct BnBwdLane {
    double mu[4], is[4];
    f32x4 ga, be, gp;
};
__device__ __forceinline__ void bn_bwd_d(const BnBwdLane& k, int act, const f32x4& gv, const f32x4& xv, f32x4& d, double (&xh)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        xh[e] = ((double)xv[e] - k.mu[e]) * k.is[e];
        const float gg = gv[e] + k.gp[e];
        d[e] = act ? gg * silu_grad1((float)xh[e] * k.ga[e] + k.be[e]) : gg;
    }
}
__device__ __forceinline__ BnBwdLane bn_bwd_lane(const double* mean, const double* invstd, const f32x4* gamma, const f32x4* beta,
                                                 const f32x4* g_pool, int C4, int cg) {
    BnBwdLane k;
#pragma unroll
    for (int e = 0; e < 4; ++e) { k.mu[e] = mean[cg * 4 + e]; k.is[e] = invstd[cg * 4 + e]; }
    k.ga = gamma[cg]; k.be = beta[cg];
    k.gp = g_pool ? g_pool[(int64_t)blockIdx.y * C4 + cg] : (f32x4)(0.f);
    return k;
}

template <int DT>
__global__ __launch_bounds__(MBT_THREADS)
void bn_bwd_sums_io(const El<DT>* __restrict__ g, const El<DT>* __restrict__ x, const double* __restrict__ mean,
                    const double* __restrict__ invstd, const f32x4* __restrict__ gamma, const f32x4* __restrict__ beta,
                    const f32x4* __restrict__ g_pool, int act, int64_t HW, int C4, double* __restrict__ partials) {
    const Lane l = lane_of_thread(C4);
    const int64_t base = (int64_t)blockIdx.y * HW;
    const int64_t p0 = (int64_t)blockIdx.x * MBT_ROWS, p_end = min(p0 + MBT_ROWS, HW);
    double acc[2][4] = {};
    if (l.live) {
        const BnBwdLane k = bn_bwd_lane(mean, invstd, gamma, beta, g_pool, C4, l.cg);
        for (int64_t p = p0 + l.pl; p < p_end; p += l.PL) {
            f32x4 d;
            double xh[4];
            bn_bwd_d(k, act, Io<DT>::ld4(g, (base + p) * C4 + l.cg), Io<DT>::ld4(x, (base + p) * C4 + l.cg), d, xh);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0][e] += (double)d[e];
                acc[1][e] += (double)d[e] * xh[e];
            }
        }
    }
    block_rows<2>(acc, l, C4, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * C4 * 4);
}

// the fp32 kernel rounds the fp64 combination to fp32 once; the 16-bit store rounds that fp32 value once more, as torch's cast
template <int DT>
__global__ __launch_bounds__(MBT_THREADS)
void bn_bwd_apply_io(const El<DT>* __restrict__ g, const El<DT>* __restrict__ x, const double* __restrict__ mean,
                     const double* __restrict__ invstd, const f32x4* __restrict__ gamma, const f32x4* __restrict__ beta,
                     const f32x4* __restrict__ g_pool, int act, const double* __restrict__ sums64, double inv_m, int training,
                     int64_t HW, int C4, El<DT>* __restrict__ g_x) {
    const Lane l = lane_of_thread(C4);
    if (!l.live) return;
    const int64_t base = (int64_t)blockIdx.y * HW;
    const int64_t p0 = (int64_t)blockIdx.x * MBT_ROWS, p_end = min(p0 + MBT_ROWS, HW);
    const BnBwdLane k = bn_bwd_lane(mean, invstd, gamma, beta, g_pool, C4, l.cg);
    double mb[4], mg[4], sc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        mb[e] = training ? sums64[l.cg * 4 + e] * inv_m : 0.0;
        mg[e] = training ? sums64[(C4 + l.cg) * 4 + e] * inv_m : 0.0;
        sc[e] = (double)k.ga[e] * k.is[e];
    }
    for (int64_t p = p0 + l.pl; p < p_end; p += l.PL) {
        f32x4 d, o;
        double xh[4];
        bn_bwd_d(k, act, Io<DT>::ld4(g, (base + p) * C4 + l.cg), Io<DT>::ld4(x, (base + p) * C4 + l.cg), d, xh);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (float)(sc[e] * (((double)d[e] - mb[e]) - xh[e] * mg[e]));
        Io<DT>::st4(g_x, (base + p) * C4 + l.cg, o);
    }
}

// ---- depthwise conv -------------------------------------------------------------------------------------------------------
// The taps of channel group cg from the fp32 [C][1][k][k] weight, each rounded to DT: autocast's cast of the conv weight
template <int DT, int TAPS>
__device__ __forceinline__ void load_taps(const float* __restrict__ w, int cg, bool flip, f32x4 (&wt)[TAPS]) {
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) wt[t][e] = round_to<DT>(w[(cg * 4 + e) * TAPS + (flip ? TAPS - 1 - t : t)]);
}

// MODE as in mbconv_train.hip: 0 3x3 circular, 1 2x2 stride 2, 2 ConvTranspose 2x2 stride 2.  H, W: of x.
template <int DT, int MODE>
__global__ __launch_bounds__(MBT_THREADS)
void dwt_conv_io(const El<DT>* __restrict__ x, const float* __restrict__ w, int flip, int H, int W, int C4, int Ho, int Wo,
                 El<DT>* __restrict__ y) {
    constexpr int TAPS = MODE == 0 ? 9 : 4;
    const Lane l = lane_of_thread(C4);
    if (!l.live) return;
    const int hw_o = Ho * Wo;
    const int p_end = min((int)(blockIdx.x + 1) * MBT_ROWS, hw_o);
    const int64_t xb = (int64_t)blockIdx.y * H * W * C4, yb = (int64_t)blockIdx.y * hw_o * C4;       // in 4-channel items
    f32x4 wt[TAPS];
    load_taps<DT, TAPS>(w, l.cg, flip != 0, wt);
    for (int p = blockIdx.x * MBT_ROWS + l.pl; p < p_end; p += l.PL) {
        const int oy = p / Wo, ox = p - oy * Wo;
        f32x4 acc;
        if (MODE == 0) {
            const int ys[3] = {wrap_m(oy, H), oy, wrap_p(oy, H)}, xs[3] = {wrap_m(ox, W), ox, wrap_p(ox, W)};
            f32x4 v[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) v[t] = Io<DT>::ld4(x, xb + ((int64_t)ys[t / 3] * W + xs[t % 3]) * C4 + l.cg);
            acc = v[0] * wt[0];
#pragma unroll
            for (int t = 1; t < 9; ++t) acc = fma4(v[t], wt[t], acc);
        } else if (MODE == 1) {
            f32x4 v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = Io<DT>::ld4(x, xb + ((int64_t)(2 * oy + t / 2) * W + 2 * ox + t % 2) * C4 + l.cg);
            acc = v[0] * wt[0];
#pragma unroll
            for (int t = 1; t < 4; ++t) acc = fma4(v[t], wt[t], acc);
        } else {
            const f32x4 v = Io<DT>::ld4(x, xb + ((int64_t)(oy >> 1) * W + (ox >> 1)) * C4 + l.cg);
            const int t = (oy & 1) * 2 + (ox & 1);
            acc = v * (t == 0 ? wt[0] : (t == 1 ? wt[1] : (t == 2 ? wt[2] : wt[3])));
        }
        Io<DT>::st4(y, yb + (int64_t)p * C4 + l.cg, acc);
    }
}

// partials[(b, strip)][t][c] = sum over the strip's pixels of g x at tap t, as dwt_wgrad_kernel of mbconv_train.hip
template <int DT, int MODE>
__global__ __launch_bounds__(MBT_THREADS)
void dwt_wgrad_io(const El<DT>* __restrict__ g, const El<DT>* __restrict__ x, int H, int W, int C4, int Hs, int Ws,
                  double* __restrict__ partials) {
    constexpr int TAPS = MODE == 0 ? 9 : 4;
    const Lane l = lane_of_thread(C4);
    const int hw_s = Hs * Ws;
    const int p_end = min((int)(blockIdx.x + 1) * MBT_ROWS, hw_s);
    const int Hg = MODE == 0 ? H : (MODE == 1 ? H / 2 : 2 * H), Wg = MODE == 0 ? W : (MODE == 1 ? W / 2 : 2 * W);
    const int64_t xb = (int64_t)blockIdx.y * H * W * C4, gb = (int64_t)blockIdx.y * Hg * Wg * C4;
    double acc[TAPS][4] = {};
    if (l.live) {
        for (int p = blockIdx.x * MBT_ROWS + l.pl; p < p_end; p += l.PL) {
            const int py = p / Ws, px = p - py * Ws;
            if (MODE == 0) {
                const f32x4 gv = Io<DT>::ld4(g, gb + (int64_t)p * C4 + l.cg);
                const int ys[3] = {wrap_m(py, H), py, wrap_p(py, H)}, xs[3] = {wrap_m(px, W), px, wrap_p(px, W)};
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const f32x4 v = Io<DT>::ld4(x, xb + ((int64_t)ys[t / 3] * W + xs[t % 3]) * C4 + l.cg);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[t][e] += (double)gv[e] * (double)v[e];
                }
            } else if (MODE == 1) {
                const f32x4 gv = Io<DT>::ld4(g, gb + (int64_t)p * C4 + l.cg);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const f32x4 v = Io<DT>::ld4(x, xb + ((int64_t)(2 * py + t / 2) * W + 2 * px + t % 2) * C4 + l.cg);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[t][e] += (double)gv[e] * (double)v[e];
                }
            } else {
                const f32x4 v = Io<DT>::ld4(x, xb + (int64_t)p * C4 + l.cg);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const f32x4 gv = Io<DT>::ld4(g, gb + ((int64_t)(2 * py + t / 2) * Wg + 2 * px + t % 2) * C4 + l.cg);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[t][e] += (double)gv[e] * (double)v[e];
                }
            }
        }
    }
    block_rows<TAPS>(acc, l, C4, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * TAPS * C4 * 4);
}

// ---- squeeze-excite product -------------------------------------------------------------------------------------------------
// grid (strips, B).  forward (g == NULL): y = x gate.  backward: y = g gate, partials[(b, strip)][c] = sum g x.  The gate is
// DG (fp32 or DT).  Io16::rnd pins the fp32 product before its conversion: -0 and the subnormal products round as torch's.
template <int DT, int DG>
__global__ __launch_bounds__(MBT_THREADS)
void se_scale_io(const El<DT>* __restrict__ g, const El<DT>* __restrict__ x, const El<DG>* __restrict__ gate, int64_t HW, int C4,
                 El<DT>* __restrict__ y, double* __restrict__ partials) {
    const Lane l = lane_of_thread(C4);
    const int64_t base = (int64_t)blockIdx.y * HW;
    const int64_t p0 = (int64_t)blockIdx.x * MBT_ROWS, p_end = min(p0 + MBT_ROWS, HW);
    double acc[1][4] = {};
    if (l.live) {
        const f32x4 gt = Io<DG>::ld4(gate, (int64_t)blockIdx.y * C4 + l.cg);
        for (int64_t p = p0 + l.pl; p < p_end; p += l.PL) {
            if (g) {
                const f32x4 xv = Io<DT>::ld4(x, (base + p) * C4 + l.cg);
                const f32x4 gv = Io<DT>::ld4(g, (base + p) * C4 + l.cg);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[0][e] += (double)gv[e] * (double)xv[e];
                Io<DT>::st4(y, (base + p) * C4 + l.cg, gv * gt);
            } else {
                const f32x4 xv = Io<DT>::ld4(x, (base + p) * C4 + l.cg);
                Io<DT>::st4(y, (base + p) * C4 + l.cg, xv * gt);
            }
        }
    }
    if (partials) block_rows<1>(acc, l, C4, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * C4 * 4);
}

// mbt_finish for a 16-bit g_gate: the column sum rounded to fp32 once, as the fp32 entry's, then to DG once, as torch's cast
template <int DG>
__global__ __launch_bounds__(MBT_THREADS)
void mbt_finish_io(const double* __restrict__ partials, int n_rows, int n_cols, El<DG>* __restrict__ out) {
    const int lane = threadIdx.x & 63, col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= n_cols) return;                                   // wave-uniform
    const double s = column_sum(partials + (int64_t)blockIdx.y * n_rows * n_cols, n_rows, n_cols, col, lane);
    if (lane != 0) return;
    Io<DG>::st(out, (int64_t)blockIdx.y * n_cols + col, (float)s);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// f(DtC<dt>) for a 16-bit code -> f's error code
template <typename F> inline int for_dt16(int dt, F&& f) {
    return dt == VQAE_DT_BF16 ? f(DtC<VQAE_DT_BF16>{}) : f(DtC<VQAE_DT_F16>{});
}

inline int check_io(const char* who, int io_dt) {
    VQAE_REQUIRE(dt_ok(io_dt), VQAE_ERR_INVALID, "%s: dtype code %d", who, io_dt);
    return VQAE_OK;
}

// the gate's code beside the tensors': fp32 or the tensors' own type
inline int check_gate(const char* who, int io_dt, int gate_dt) {
    VQAE_REQUIRE(dt_ok(io_dt) && dt_ok(gate_dt), VQAE_ERR_INVALID, "%s: dtype codes %d, gate %d", who, io_dt, gate_dt);
    VQAE_REQUIRE(!(dt_16(io_dt) && dt_16(gate_dt) && io_dt != gate_dt), VQAE_ERR_UNSUPPORTED,
                 "%s: the tensors and the gate are two different 16-bit types (%d, %d); a call takes at most one", who, io_dt,
                 gate_dt);
    VQAE_REQUIRE(dt_16(io_dt) || !dt_16(gate_dt), VQAE_ERR_UNSUPPORTED,
                 "%s: a 16-bit gate (%d) goes with 16-bit tensors, not fp32 ones", who, gate_dt);
    return VQAE_OK;
}

template <int DT>
inline int dw_launch_io(int mode, const void* x, const float* wgt, int flip, int batch, int h, int w, int c, void* y,
                        hipStream_t stream) {
    int ho, wo;
    dw_out_dims(mode, h, w, &ho, &wo);
    const dim3 grid((unsigned)strips_of((int64_t)ho * wo), (unsigned)batch);
    const int C4 = c / 4;
    auto xp = (const El<DT>*)x;
    auto yp = (El<DT>*)y;
    if (mode == VQAE_DW_SAME) dwt_conv_io<DT, 0><<<grid, MBT_THREADS, 0, stream>>>(xp, wgt, flip, h, w, C4, ho, wo, yp);
    else if (mode == VQAE_DW_DOWN) dwt_conv_io<DT, 1><<<grid, MBT_THREADS, 0, stream>>>(xp, wgt, flip, h, w, C4, ho, wo, yp);
    else dwt_conv_io<DT, 2><<<grid, MBT_THREADS, 0, stream>>>(xp, wgt, flip, h, w, C4, ho, wo, yp);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

}  // namespace

extern "C" int vqae_bn_act_train_forward_io(const void* x, const float* gamma, const float* beta, float* running_mean,
                                            float* running_var, int training, double momentum, double eps, int act, int batch,
                                            int64_t hw, int c, void* y, double* mean, double* invstd, float* pool, void* ws,
                                            int io_dt, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_io("bn_act_train_forward_io", io_dt)) return rc;
    if (io_dt == VQAE_DT_F32)
        return vqae_bn_act_train_forward_f32((const float*)x, gamma, beta, running_mean, running_var, training, momentum, eps, act,
                                             batch, hw, c, (float*)y, mean, invstd, pool, ws, stream_);
    if (int rc = check_rows("bn_act_train_forward_io", batch, hw, c)) return rc;
    VQAE_REQUIRE(x && gamma && beta && y && mean && invstd && ws, VQAE_ERR_INVALID, "bn_act_train_forward_io: null pointer");
    VQAE_REQUIRE(training || (running_mean && running_var), VQAE_ERR_INVALID,
                 "bn_act_train_forward_io: eval mode needs the running statistics");
    VQAE_REQUIRE((act == 0 || act == 1) && eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0, VQAE_ERR_INVALID,
                 "bn_act_train_forward_io: act %d eps %g momentum %g", act, eps, momentum);
    const int64_t M = (int64_t)batch * hw;
    VQAE_REQUIRE(!training || M > 1, VQAE_ERR_VALUE,
                 "Expected more than 1 value per channel when training, got input size [%d, %d, %lld]", batch, c, (long long)hw);
    VQAE_REQUIRE(aligned_vec({{x, io_dt}, {y, io_dt}}) && aligned16({gamma, beta, mean, invstd}) && ((uintptr_t)ws & 7) == 0,
                 VQAE_ERR_INVALID,
                 "bn_act_train_forward_io: 16-bit tensors must be 8-byte, fp32 ones 16-byte, the workspace 8-byte aligned");
    const int C4 = c / 4;
    double* partials = (double*)ws;
    const int64_t n_img = pool ? batch : 1, img = pool ? hw : M;
    const dim3 grid((unsigned)strips_of(img), (unsigned)n_img);
    const f32x4 *ga = (const f32x4*)gamma, *be = (const f32x4*)beta;
    const int rc = for_dt16(io_dt, [&](auto dt) -> int {
        constexpr int DT = decltype(dt)::value;
        auto xp = (const El<DT>*)x;
        if (training) {
            const int64_t n_wg = strips_of(M);
            bn_stats_io<DT><<<(unsigned)n_wg, MBT_THREADS, 0, stream>>>(xp, M, C4, partials);
            VQAE_LAUNCH_CHECK();
            bn_finish_io<DT><<<(unsigned)ceil_div(c, 4), MBT_THREADS, 0, stream>>>(partials, (int)n_wg, xp, M, c, momentum, eps,
                                                                                  running_mean, running_var, mean, invstd);
        } else {
            bn_eval_stats_kernel<<<(unsigned)ceil_div(c, 256), 256, 0, stream>>>(running_mean, running_var, eps, c, mean, invstd);
        }
        VQAE_LAUNCH_CHECK();
        // without the pool the rows are one image: the grid does not depend on how M splits into batch and hw
        bn_apply_io<DT><<<grid, MBT_THREADS, 0, stream>>>(xp, mean, invstd, ga, be, act, img, C4, (El<DT>*)y,
                                                         pool ? partials : nullptr);
        VQAE_LAUNCH_CHECK();
        return VQAE_OK;
    });
    if (rc) return rc;
    if (pool) return finish(partials, batch, strips_of(hw), c, 0, pool, stream);
    return VQAE_OK;
}

extern "C" int vqae_bn_act_train_backward_io(const void* g, const void* x, const double* mean, const double* invstd,
                                             const float* gamma, const float* beta, const float* g_pool, int training, int act,
                                             int batch, int64_t hw, int c, void* g_x, float* g_beta_gamma, void* ws, int io_dt,
                                             void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_io("bn_act_train_backward_io", io_dt)) return rc;
    if (io_dt == VQAE_DT_F32)
        return vqae_bn_act_train_backward_f32((const float*)g, (const float*)x, mean, invstd, gamma, beta, g_pool, training, act,
                                              batch, hw, c, (float*)g_x, g_beta_gamma, ws, stream_);
    if (int rc = check_rows("bn_act_train_backward_io", batch, hw, c)) return rc;
    VQAE_REQUIRE(g && x && mean && invstd && gamma && beta && g_x && g_beta_gamma && ws, VQAE_ERR_INVALID,
                 "bn_act_train_backward_io: null pointer");
    VQAE_REQUIRE(act == 0 || act == 1, VQAE_ERR_INVALID, "bn_act_train_backward_io: act %d", act);
    VQAE_REQUIRE(aligned_vec({{g, io_dt}, {x, io_dt}, {g_x, io_dt}}) &&
                     aligned16({mean, invstd, gamma, beta, g_pool, g_beta_gamma}) && ((uintptr_t)ws & 7) == 0,
                 VQAE_ERR_INVALID,
                 "bn_act_train_backward_io: 16-bit tensors must be 8-byte, fp32 ones 16-byte, the workspace 8-byte aligned");
    const int C4 = c / 4;
    const int64_t M = (int64_t)batch * hw;
    const int64_t n_img = g_pool ? batch : 1, img = g_pool ? hw : M;
    const dim3 grid((unsigned)strips_of(img), (unsigned)n_img);
    double* partials = (double*)ws;
    double* sums64 = partials + (size_t)grid.x * grid.y * 2 * c;
    const f32x4 *ga = (const f32x4*)gamma, *be = (const f32x4*)beta, *gp = (const f32x4*)g_pool;
    if (int rc = for_dt16(io_dt, [&](auto dt) -> int {
        constexpr int DT = decltype(dt)::value;
        bn_bwd_sums_io<DT><<<grid, MBT_THREADS, 0, stream>>>((const El<DT>*)g, (const El<DT>*)x, mean, invstd, ga, be, gp, act, img,
                                                            C4, partials);
        VQAE_LAUNCH_CHECK();
        return VQAE_OK;
    })) return rc;
    if (int rc = finish(partials, 1, (int64_t)grid.x * grid.y, 2 * c, 0, g_beta_gamma, stream, sums64)) return rc;
    return for_dt16(io_dt, [&](auto dt) -> int {
        constexpr int DT = decltype(dt)::value;
        bn_bwd_apply_io<DT><<<grid, MBT_THREADS, 0, stream>>>((const El<DT>*)g, (const El<DT>*)x, mean, invstd, ga, be, gp, act,
                                                             sums64, 1.0 / (double)M, training != 0, img, C4, (El<DT>*)g_x);
        VQAE_LAUNCH_CHECK();
        return VQAE_OK;
    });
}

extern "C" int vqae_dwconv_train_forward_io(const void* x, const float* wgt, int mode, int batch, int h, int w, int c, void* y,
                                            int io_dt, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_io("dwconv_train_forward_io", io_dt)) return rc;
    if (io_dt == VQAE_DT_F32) return vqae_dwconv_train_forward_f32((const float*)x, wgt, mode, batch, h, w, c, (float*)y, stream_);
    if (int rc = dw_check("dwconv_train_forward_io", batch, h, w, c, mode)) return rc;
    VQAE_REQUIRE(x && wgt && y, VQAE_ERR_INVALID, "dwconv_train_forward_io: null pointer");
    VQAE_REQUIRE(aligned_vec({{x, io_dt}, {y, io_dt}}), VQAE_ERR_INVALID,
                 "dwconv_train_forward_io: 16-bit tensors must be 8-byte aligned");
    return for_dt16(io_dt, [&](auto dt) -> int {
        return dw_launch_io<decltype(dt)::value>(mode, x, wgt, 0, batch, h, w, c, y, stream);
    });
}

extern "C" int vqae_dwconv_train_backward_io(const void* g, const void* x, const float* wgt, int mode, int batch, int h, int w,
                                             int c, void* g_x, float* g_w, void* ws, int io_dt, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_io("dwconv_train_backward_io", io_dt)) return rc;
    if (io_dt == VQAE_DT_F32)
        return vqae_dwconv_train_backward_f32((const float*)g, (const float*)x, wgt, mode, batch, h, w, c, (float*)g_x, g_w, ws,
                                              stream_);
    if (int rc = dw_check("dwconv_train_backward_io", batch, h, w, c, mode)) return rc;
    VQAE_REQUIRE(g && (!g_x || wgt) && (!g_w || (x && ws)), VQAE_ERR_INVALID, "dwconv_train_backward_io: null pointer");
    VQAE_REQUIRE(aligned_vec({{g, io_dt}, {x, io_dt}, {g_x, io_dt}}) && ((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID,
                 "dwconv_train_backward_io: 16-bit tensors and the workspace must be 8-byte aligned");
    int ho, wo;
    dw_out_dims(mode, h, w, &ho, &wo);
    if (g_x) {       // gathered: the 3x3 over g with flipped taps; the stride-2 modes are each other's adjoints
        const int adj = mode == VQAE_DW_SAME ? VQAE_DW_SAME : (mode == VQAE_DW_DOWN ? VQAE_DW_UP : VQAE_DW_DOWN);
        if (int rc = for_dt16(io_dt, [&](auto dt) -> int {
                return dw_launch_io<decltype(dt)::value>(adj, g, wgt, mode == VQAE_DW_SAME, batch, ho, wo, c, g_x, stream);
            }))
            return rc;
    }
    if (g_w) {
        const int hs = mode == VQAE_DW_DOWN ? ho : h, wsz = mode == VQAE_DW_DOWN ? wo : w;     // the walked (smaller) tensor
        const dim3 grid((unsigned)strips_of((int64_t)hs * wsz), (unsigned)batch);
        const int C4 = c / 4, taps = mode == VQAE_DW_SAME ? 9 : 4;
        double* partials = (double*)ws;
        if (int rc = for_dt16(io_dt, [&](auto dt) -> int {
            constexpr int DT = decltype(dt)::value;
            auto gp = (const El<DT>*)g;
            auto xp = (const El<DT>*)x;
            if (mode == VQAE_DW_SAME) dwt_wgrad_io<DT, 0><<<grid, MBT_THREADS, 0, stream>>>(gp, xp, h, w, C4, hs, wsz, partials);
            else if (mode == VQAE_DW_DOWN) dwt_wgrad_io<DT, 1><<<grid, MBT_THREADS, 0, stream>>>(gp, xp, h, w, C4, hs, wsz, partials);
            else dwt_wgrad_io<DT, 2><<<grid, MBT_THREADS, 0, stream>>>(gp, xp, h, w, C4, hs, wsz, partials);
            VQAE_LAUNCH_CHECK();
            return VQAE_OK;
        })) return rc;
        return finish(partials, 1, (int64_t)grid.x * grid.y, taps * c, taps, g_w, stream);
    }
    return VQAE_OK;
}

namespace {

// se_scale_io<DT, DG> for a 16-bit io_dt and a gate code that is fp32 or io_dt
inline int se_launch(int io_dt, int gate_dt, const dim3& grid, const void* g, const void* x, const void* gate, int64_t hw, int C4,
                      void* y, double* partials, hipStream_t stream) {
    return for_dt16(io_dt, [&](auto dt) -> int {
        constexpr int DT = decltype(dt)::value;
        auto gp = (const El<DT>*)g;
        auto xp = (const El<DT>*)x;
        auto yp = (El<DT>*)y;
        if (gate_dt == VQAE_DT_F32)
            se_scale_io<DT, VQAE_DT_F32><<<grid, MBT_THREADS, 0, stream>>>(gp, xp, (const float*)gate, hw, C4, yp, partials);
        else
            se_scale_io<DT, DT><<<grid, MBT_THREADS, 0, stream>>>(gp, xp, (const El<DT>*)gate, hw, C4, yp, partials);
        VQAE_LAUNCH_CHECK();
        return VQAE_OK;
    });
}

}  // namespace

extern "C" int vqae_se_scale_forward_io(const void* x, const void* gate, int batch, int64_t hw, int c, void* y, int io_dt,
                                        int gate_dt, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_gate("se_scale_forward_io", io_dt, gate_dt)) return rc;
    if (io_dt == VQAE_DT_F32) return vqae_se_scale_forward_f32((const float*)x, (const float*)gate, batch, hw, c, (float*)y, stream_);
    if (int rc = check_rows("se_scale_forward_io", batch, hw, c)) return rc;
    VQAE_REQUIRE(x && gate && y, VQAE_ERR_INVALID, "se_scale_forward_io: null pointer");
    VQAE_REQUIRE(aligned_vec({{x, io_dt}, {y, io_dt}, {gate, gate_dt}}), VQAE_ERR_INVALID,
                 "se_scale_forward_io: 16-bit tensors must be 8-byte, fp32 ones 16-byte aligned");
    return se_launch(io_dt, gate_dt, dim3((unsigned)strips_of(hw), (unsigned)batch), nullptr, x, gate, hw, c / 4, y, nullptr,
                     stream);
}

extern "C" int vqae_se_scale_backward_io(const void* g, const void* x, const void* gate, int batch, int64_t hw, int c, void* g_x,
                                         void* g_gate, void* ws, int io_dt, int gate_dt, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_gate("se_scale_backward_io", io_dt, gate_dt)) return rc;
    if (io_dt == VQAE_DT_F32)
        return vqae_se_scale_backward_f32((const float*)g, (const float*)x, (const float*)gate, batch, hw, c, (float*)g_x,
                                          (float*)g_gate, ws, stream_);
    if (int rc = check_rows("se_scale_backward_io", batch, hw, c)) return rc;
    VQAE_REQUIRE(g && x && gate && g_x && g_gate && ws, VQAE_ERR_INVALID, "se_scale_backward_io: null pointer");
    // g_gate is written element by element: its own type's alignment is enough
    VQAE_REQUIRE(aligned_vec({{g, io_dt}, {x, io_dt}, {g_x, io_dt}, {gate, gate_dt}}) && ((uintptr_t)ws & 7) == 0 &&
                     ((uintptr_t)g_gate & (dt_16(gate_dt) ? 1 : 3)) == 0,
                 VQAE_ERR_INVALID,
                 "se_scale_backward_io: 16-bit tensors must be 8-byte, fp32 ones 16-byte, the workspace 8-byte aligned");
    const dim3 grid((unsigned)strips_of(hw), (unsigned)batch);
    if (int rc = se_launch(io_dt, gate_dt, grid, g, x, gate, hw, c / 4, g_x, (double*)ws, stream)) return rc;
    if (gate_dt == VQAE_DT_F32) return finish((double*)ws, batch, strips_of(hw), c, 0, (float*)g_gate, stream);
    const dim3 fgrid((unsigned)ceil_div(c, 4), (unsigned)batch);
    return for_dt16(gate_dt, [&](auto dt) -> int {
        constexpr int DG = decltype(dt)::value;
        mbt_finish_io<DG><<<fgrid, MBT_THREADS, 0, stream>>>((const double*)ws, (int)strips_of(hw), c, (El<DG>*)g_gate);
        VQAE_LAUNCH_CHECK();
        return VQAE_OK;
    });
}
