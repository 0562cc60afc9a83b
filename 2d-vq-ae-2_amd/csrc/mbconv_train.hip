// Training forms of every op of an MBConv block that is not a dense conv (reference vq_ae/layers/conv_block.py:240-321,
// vq_ae/layers/misc.py:7-30), forward and backward, fp32, NHWC.  mbconv.hip has the inference forms, with the BatchNorms
// folded away; here they are back:
//
//   bn_act    batch-statistic BatchNorm2d (+ SiLU): y = act((x - mean) invstd gamma + beta), the running statistics updated
//             in the launch that finishes the sums; optionally pool[b][c] = sum_hw y, the squeeze of the SE layer
//   dwconv    the depthwise conv of branch[3], the three modes of mbconv.hip (3x3 circular, 2x2 stride 2, ConvTranspose 2x2
//             stride 2), reading the module's own [C][1][k][k] weight in place
//   se_scale  y = x gate[b][c]
//
// Every kernel is a byte mover laid out as mbconv.hip's: one float4 (4 channels) per lane, thread (pl, cg) = (tid / C4,
// tid % C4) on channel group cg and the rows pl, pl + PL, ... (PL = 256 / C4) of its workgroup's MBT_ROWS rows, so every
// wavefront access is a run of contiguous 16-byte words.  C % 4 == 0, C <= 1024.
//
// Sums (BatchNorm statistics and its g_gamma / g_beta, pool, the depthwise weight gradient, g_gate): every thread adds its rows
// in index order in fp64 (a product of two fp32 is exact there), the pixel lanes of a workgroup are added in index order
// through LDS, one fp64 row per workgroup goes to the workspace, and a second launch (one wave per column: lane l adds rows
// l, l + 64, ... in order, then the lanes by shuffle) adds the rows and rounds to fp32 once.  Grids depend on the shape alone
// and there is no floating-point atomic: every result is bit-identical run to run.
//
// Backward:
//   bn_act    z and act'(z) are recomputed from the saved x, mean, invstd (z is never stored).  d = (g + g_pool[b][c]) act'(z) (pool is a SUM over hw);
//             g_beta = sum d, g_gamma = sum d xhat (one pass), g_x = gamma invstd (d - g_beta / M - xhat g_gamma / M) (a second
//             pass; eval mode: gamma invstd d)
//   dwconv    the data gradient is GATHERED: the 3x3 case is the same conv over g with the taps flipped, the stride-2 modes
//             are each other's adjoints, so all three run the forward kernel; every element is written once
//   se_scale  g_x = g gate, g_gate[b][c] = sum_hw g x
//
// The lane layout, the fixed-order sums, SiLU and the host-side shape checks are in mbconv_train_impl.h, shared with
// mbconv_train_io.hip (vqae_*_io): the same arithmetic in the same element order on up-cast 16-bit tensors, one rounding on store.
#include "mbconv_train_impl.h"

namespace {

using namespace vqae;
using namespace vqae::mbt;

// ---- BatchNorm --------------------------------------------------------------------------------------------------------------
// partials[wg][0][c] = sum (x - x[0][c]), partials[wg][1][c] = sum (x - x[0][c])^2 over the workgroup's rows: the shift by the
// first row keeps a constant channel's variance at exactly 0
__global__ __launch_bounds__(MBT_THREADS)
void bn_stats_kernel(const f32x4* __restrict__ x, int64_t M, int C4, double* __restrict__ partials) {
    const Lane l = lane_of_thread(C4);
    const int64_t p0 = (int64_t)blockIdx.x * MBT_ROWS, p_end = min(p0 + MBT_ROWS, M);
    double acc[2][4] = {};
    if (l.live) {
        const f32x4 sh = x[l.cg];
        for (int64_t p = p0 + l.pl; p < p_end; p += l.PL) {
            const f32x4 v = x[p * C4 + l.cg];
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

// One wave per channel: mean, biased variance, invstd (kept in fp64: the backward at a handful of rows is a difference of
// nearly equal numbers); running statistics updated in place with the unbiased variance.
__global__ __launch_bounds__(MBT_THREADS)
void bn_finish_kernel(const double* __restrict__ partials, int n_rows, const float* __restrict__ x, int64_t M, int C,
                      double momentum, double eps, float* __restrict__ running_mean, float* __restrict__ running_var,
                      double* __restrict__ mean, double* __restrict__ invstd) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;                                          // wave-uniform
    const double s1 = column_sum(partials, n_rows, 2 * C, c, lane);
    const double s2 = column_sum(partials, n_rows, 2 * C, C + c, lane);
    if (lane != 0) return;
    const double m1 = s1 / (double)M;
    const double mu = (double)x[c] + m1;
    const double var = fmax(s2 / (double)M - m1 * m1, 0.0);
    mean[c] = mu;
    invstd[c] = 1.0 / sqrt(var + eps);
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mu);
    if (running_var)
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (var * ((double)M / (double)(M - 1))));
}

// grid (strips, B): y = act((x - mean) invstd gamma + beta); pool_partials [B][strips][C] = the strip's sums of y (or NULL)
__global__ __launch_bounds__(MBT_THREADS)
void bn_apply_kernel(const f32x4* __restrict__ x, const double* __restrict__ mean, const double* __restrict__ invstd,
                     const f32x4* __restrict__ gamma, const f32x4* __restrict__ beta, int act, int64_t HW, int C4,
                     f32x4* __restrict__ y, double* __restrict__ pool_partials) {
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
            const f32x4 v = x[(base + p) * C4 + l.cg];
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float z = (v[e] - mu[e]) * is[e] * ga[e] + be[e];
                o[e] = act ? silu1(z) : z;
                acc[0][e] += (double)o[e];
            }
            y[(base + p) * C4 + l.cg] = o;
        }
    }
    if (pool_partials) block_rows<1>(acc, l, C4, pool_partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * C4 * 4);
}

// d = (g + g_pool[b][c]) act'(z) in fp32, xhat = (x - mean) invstd in fp64
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

// grid (strips, B): partials[(b, strip)][0][c] = sum d, [1][c] = sum d xhat
__global__ __launch_bounds__(MBT_THREADS)
void bn_bwd_sums_kernel(const f32x4* __restrict__ g, const f32x4* __restrict__ x, const double* __restrict__ mean,
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
            bn_bwd_d(k, act, g[(base + p) * C4 + l.cg], x[(base + p) * C4 + l.cg], d, xh);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0][e] += (double)d[e];
                acc[1][e] += (double)d[e] * xh[e];
            }
        }
    }
    block_rows<2>(acc, l, C4, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * C4 * 4);
}

// sums64 [2][C] = g_beta, g_gamma, unrounded.  training: g_x = gamma invstd (d - g_beta / M - xhat g_gamma / M), combined in
// fp64 and rounded once; eval: gamma invstd d
__global__ __launch_bounds__(MBT_THREADS)
void bn_bwd_apply_kernel(const f32x4* __restrict__ g, const f32x4* __restrict__ x, const double* __restrict__ mean,
                         const double* __restrict__ invstd, const f32x4* __restrict__ gamma, const f32x4* __restrict__ beta,
                         const f32x4* __restrict__ g_pool, int act, const double* __restrict__ sums64, double inv_m,
                         int training, int64_t HW, int C4, f32x4* __restrict__ g_x) {
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
        bn_bwd_d(k, act, g[(base + p) * C4 + l.cg], x[(base + p) * C4 + l.cg], d, xh);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (float)(sc[e] * (((double)d[e] - mb[e]) - xh[e] * mg[e]));
        g_x[(base + p) * C4 + l.cg] = o;
    }
}

// ---- depthwise conv -------------------------------------------------------------------------------------------------------
// The taps of channel group cg from a [C][1][k][k] weight: wt[t][e] = w[(4 cg + e) TAPS + t]; flip: tap t reads TAPS - 1 - t
template <int TAPS>
__device__ __forceinline__ void load_taps(const float* __restrict__ w, int cg, bool flip, f32x4 (&wt)[TAPS]) {
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) wt[t][e] = w[(cg * 4 + e) * TAPS + (flip ? TAPS - 1 - t : t)];
}

// MODE 0: 3x3 / stride 1 / circular   y[oy][ox] = sum_{dy,dx} w[dy*3+dx] x[(oy+dy-1) mod H][(ox+dx-1) mod W]
// MODE 1: 2x2 / stride 2              y[oy][ox] = sum_{a,b}   w[a*2+b]   x[2oy+a][2ox+b]
// MODE 2: ConvTranspose2d 2x2 / s 2   y[2i+a][2j+b] = w[a*2+b] x[i][j]
// H, W: of x.  grid (strips of MBT_ROWS output pixels, B).
template <int MODE>
__global__ __launch_bounds__(MBT_THREADS)
void dwt_conv_kernel(const f32x4* __restrict__ x, const float* __restrict__ w, int flip, int H, int W, int C4, int Ho, int Wo,
                     f32x4* __restrict__ y) {
    constexpr int TAPS = MODE == 0 ? 9 : 4;
    const Lane l = lane_of_thread(C4);
    if (!l.live) return;
    const int hw_o = Ho * Wo;
    const int p_end = min((int)(blockIdx.x + 1) * MBT_ROWS, hw_o);
    const f32x4* xb = x + (int64_t)blockIdx.y * H * W * C4;
    f32x4* yb = y + (int64_t)blockIdx.y * hw_o * C4;
    f32x4 wt[TAPS];
    load_taps<TAPS>(w, l.cg, flip != 0, wt);
    for (int p = blockIdx.x * MBT_ROWS + l.pl; p < p_end; p += l.PL) {
        const int oy = p / Wo, ox = p - oy * Wo;
        f32x4 acc;
        if (MODE == 0) {
            const int ys[3] = {wrap_m(oy, H), oy, wrap_p(oy, H)}, xs[3] = {wrap_m(ox, W), ox, wrap_p(ox, W)};
            f32x4 v[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) v[t] = xb[((int64_t)ys[t / 3] * W + xs[t % 3]) * C4 + l.cg];
            acc = v[0] * wt[0];
#pragma unroll
            for (int t = 1; t < 9; ++t) acc = fma4(v[t], wt[t], acc);
        } else if (MODE == 1) {
            f32x4 v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = xb[((int64_t)(2 * oy + t / 2) * W + 2 * ox + t % 2) * C4 + l.cg];
            acc = v[0] * wt[0];
#pragma unroll
            for (int t = 1; t < 4; ++t) acc = fma4(v[t], wt[t], acc);
        } else {
            const f32x4 v = xb[((int64_t)(oy >> 1) * W + (ox >> 1)) * C4 + l.cg];
            const int t = (oy & 1) * 2 + (ox & 1);
            acc = v * (t == 0 ? wt[0] : (t == 1 ? wt[1] : (t == 2 ? wt[2] : wt[3])));
        }
        yb[(int64_t)p * C4 + l.cg] = acc;
    }
}

// partials[(b, strip)][t][c] = sum over the strip's pixels of g x at tap t.  The strip walks the pixels of the SMALLER of the two
// tensors: the outputs (g) for modes 0 and 1, the inputs (x) for mode 2.  H, W: of x; Hs, Ws: of the walked tensor.
template <int MODE>
__global__ __launch_bounds__(MBT_THREADS)
void dwt_wgrad_kernel(const f32x4* __restrict__ g, const f32x4* __restrict__ x, int H, int W, int C4, int Hs, int Ws,
                      double* __restrict__ partials) {
    constexpr int TAPS = MODE == 0 ? 9 : 4;
    const Lane l = lane_of_thread(C4);
    const int hw_s = Hs * Ws;
    const int p_end = min((int)(blockIdx.x + 1) * MBT_ROWS, hw_s);
    const int Hg = MODE == 0 ? H : (MODE == 1 ? H / 2 : 2 * H), Wg = MODE == 0 ? W : (MODE == 1 ? W / 2 : 2 * W);
    const f32x4* xb = x + (int64_t)blockIdx.y * H * W * C4;
    const f32x4* gb = g + (int64_t)blockIdx.y * Hg * Wg * C4;
    double acc[TAPS][4] = {};
    if (l.live) {
        for (int p = blockIdx.x * MBT_ROWS + l.pl; p < p_end; p += l.PL) {
            const int py = p / Ws, px = p - py * Ws;
            if (MODE == 0) {
                const f32x4 gv = gb[(int64_t)p * C4 + l.cg];
                const int ys[3] = {wrap_m(py, H), py, wrap_p(py, H)}, xs[3] = {wrap_m(px, W), px, wrap_p(px, W)};
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const f32x4 v = xb[((int64_t)ys[t / 3] * W + xs[t % 3]) * C4 + l.cg];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[t][e] += (double)gv[e] * (double)v[e];
                }
            } else if (MODE == 1) {
                const f32x4 gv = gb[(int64_t)p * C4 + l.cg];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const f32x4 v = xb[((int64_t)(2 * py + t / 2) * W + 2 * px + t % 2) * C4 + l.cg];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[t][e] += (double)gv[e] * (double)v[e];
                }
            } else {
                const f32x4 v = xb[(int64_t)p * C4 + l.cg];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const f32x4 gv = gb[((int64_t)(2 * py + t / 2) * Wg + 2 * px + t % 2) * C4 + l.cg];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[t][e] += (double)gv[e] * (double)v[e];
                }
            }
        }
    }
    block_rows<TAPS>(acc, l, C4, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * TAPS * C4 * 4);
}

// ---- squeeze-excite product -------------------------------------------------------------------------------------------------
// grid (strips, B).  forward (g == NULL): y = x gate.  backward: y = g gate, partials[(b, strip)][c] = sum g x
__global__ __launch_bounds__(MBT_THREADS)
void se_scale_kernel(const f32x4* __restrict__ g, const f32x4* __restrict__ x, const f32x4* __restrict__ gate, int64_t HW, int C4,
                     f32x4* __restrict__ y, double* __restrict__ partials) {
    const Lane l = lane_of_thread(C4);
    const int64_t base = (int64_t)blockIdx.y * HW;
    const int64_t p0 = (int64_t)blockIdx.x * MBT_ROWS, p_end = min(p0 + MBT_ROWS, HW);
    double acc[1][4] = {};
    if (l.live) {
        const f32x4 gt = gate[(int64_t)blockIdx.y * C4 + l.cg];
        for (int64_t p = p0 + l.pl; p < p_end; p += l.PL) {
            const f32x4 xv = x[(base + p) * C4 + l.cg];
            if (g) {
                const f32x4 gv = g[(base + p) * C4 + l.cg];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[0][e] += (double)gv[e] * (double)xv[e];
                y[(base + p) * C4 + l.cg] = gv * gt;
            } else {
                y[(base + p) * C4 + l.cg] = xv * gt;
            }
        }
    }
    if (partials) block_rows<1>(acc, l, C4, partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * C4 * 4);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// the forward kernel of `mode` on x [B][h][w][c] -> y
inline int dw_launch(int mode, const float* x, const float* wgt, int flip, int batch, int h, int w, int c, float* y,
                     hipStream_t stream) {
    int ho, wo;
    dw_out_dims(mode, h, w, &ho, &wo);
    const dim3 grid((unsigned)strips_of((int64_t)ho * wo), (unsigned)batch);
    const int C4 = c / 4;
    const f32x4* x4 = (const f32x4*)x;
    f32x4* y4 = (f32x4*)y;
    if (mode == VQAE_DW_SAME) dwt_conv_kernel<0><<<grid, MBT_THREADS, 0, stream>>>(x4, wgt, flip, h, w, C4, ho, wo, y4);
    else if (mode == VQAE_DW_DOWN) dwt_conv_kernel<1><<<grid, MBT_THREADS, 0, stream>>>(x4, wgt, flip, h, w, C4, ho, wo, y4);
    else dwt_conv_kernel<2><<<grid, MBT_THREADS, 0, stream>>>(x4, wgt, flip, h, w, C4, ho, wo, y4);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

}  // namespace

extern "C" int vqae_bn_act_train_supported(int c) { return channels_ok(c) ? 1 : 0; }

extern "C" size_t vqae_bn_act_train_workspace_bytes(int batch, int64_t hw, int c) {
    if (batch < 1 || hw < 1 || c < 1) return 0;
    return ((size_t)batch * (size_t)strips_of(hw) + 1) * 2 * (size_t)c * sizeof(double) + 256;      // partial rows + the sums
}

extern "C" int vqae_bn_act_train_forward_f32(const float* x, const float* gamma, const float* beta, float* running_mean,
                                             float* running_var, int training, double momentum, double eps, int act, int batch,
                                             int64_t hw, int c, float* y, double* mean, double* invstd, float* pool, void* ws,
                                             void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_rows("bn_act_train_forward", batch, hw, c)) return rc;
    VQAE_REQUIRE(x && gamma && beta && y && mean && invstd && ws, VQAE_ERR_INVALID, "bn_act_train_forward: null pointer");
    VQAE_REQUIRE(training || (running_mean && running_var), VQAE_ERR_INVALID,
                 "bn_act_train_forward: eval mode needs the running statistics");
    VQAE_REQUIRE((act == 0 || act == 1) && eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0, VQAE_ERR_INVALID,
                 "bn_act_train_forward: act %d eps %g momentum %g", act, eps, momentum);
    const int64_t M = (int64_t)batch * hw;
    VQAE_REQUIRE(!training || M > 1, VQAE_ERR_VALUE,
                 "Expected more than 1 value per channel when training, got input size [%d, %d, %lld]", batch, c, (long long)hw);
    VQAE_REQUIRE(aligned16({x, gamma, beta, y, mean, invstd}) && ((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID,
                 "bn_act_train_forward: tensors must be 16-byte, the workspace 8-byte aligned");
    const int C4 = c / 4;
    double* partials = (double*)ws;
    if (training) {
        const int64_t n_wg = strips_of(M);
        bn_stats_kernel<<<(unsigned)n_wg, MBT_THREADS, 0, stream>>>((const f32x4*)x, M, C4, partials);
        VQAE_LAUNCH_CHECK();
        bn_finish_kernel<<<(unsigned)ceil_div(c, 4), MBT_THREADS, 0, stream>>>(partials, (int)n_wg, x, M, c, momentum, eps,
                                                                             running_mean, running_var, mean, invstd);
    } else {
        bn_eval_stats_kernel<<<(unsigned)ceil_div(c, 256), 256, 0, stream>>>(running_mean, running_var, eps, c, mean, invstd);
    }
    VQAE_LAUNCH_CHECK();
    // without the pool the rows are one image: the grid does not depend on how M splits into batch and hw
    const int64_t n_img = pool ? batch : 1, img = pool ? hw : M;
    bn_apply_kernel<<<dim3((unsigned)strips_of(img), (unsigned)n_img), MBT_THREADS, 0, stream>>>(
        (const f32x4*)x, mean, invstd, (const f32x4*)gamma, (const f32x4*)beta, act, img, C4, (f32x4*)y,
        pool ? partials : nullptr);
    VQAE_LAUNCH_CHECK();
    if (pool) return finish(partials, batch, strips_of(hw), c, 0, pool, stream);
    return VQAE_OK;
}

extern "C" int vqae_bn_act_train_backward_f32(const float* g, const float* x, const double* mean, const double* invstd,
                                              const float* gamma, const float* beta, const float* g_pool, int training, int act,
                                              int batch, int64_t hw, int c, float* g_x, float* g_beta_gamma, void* ws,
                                              void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_rows("bn_act_train_backward", batch, hw, c)) return rc;
    VQAE_REQUIRE(g && x && mean && invstd && gamma && beta && g_x && g_beta_gamma && ws, VQAE_ERR_INVALID,
                 "bn_act_train_backward: null pointer");
    VQAE_REQUIRE(act == 0 || act == 1, VQAE_ERR_INVALID, "bn_act_train_backward: act %d", act);
    VQAE_REQUIRE(aligned16({g, x, mean, invstd, gamma, beta, g_pool, g_x, g_beta_gamma}) && ((uintptr_t)ws & 7) == 0,
                 VQAE_ERR_INVALID, "bn_act_train_backward: tensors must be 16-byte, the workspace 8-byte aligned");
    const int C4 = c / 4;
    const int64_t M = (int64_t)batch * hw;
    const int64_t n_img = g_pool ? batch : 1, img = g_pool ? hw : M;
    const dim3 grid((unsigned)strips_of(img), (unsigned)n_img);
    double* partials = (double*)ws;
    double* sums64 = partials + (size_t)grid.x * grid.y * 2 * c;
    const f32x4 *g4 = (const f32x4*)g, *x4 = (const f32x4*)x;
    const double *mu = mean, *is = invstd;
    const f32x4 *ga = (const f32x4*)gamma, *be = (const f32x4*)beta, *gp = (const f32x4*)g_pool;
    bn_bwd_sums_kernel<<<grid, MBT_THREADS, 0, stream>>>(g4, x4, mu, is, ga, be, gp, act, img, C4, partials);
    VQAE_LAUNCH_CHECK();
    if (int rc = finish(partials, 1, (int64_t)grid.x * grid.y, 2 * c, 0, g_beta_gamma, stream, sums64)) return rc;
    bn_bwd_apply_kernel<<<grid, MBT_THREADS, 0, stream>>>(g4, x4, mu, is, ga, be, gp, act, sums64, 1.0 / (double)M,
                                                         training != 0, img, C4, (f32x4*)g_x);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" int vqae_dwconv_train_supported(int c, int h, int w, int mode) {
    if (!channels_ok(c) || h < 1 || w < 1 || h > 16384 || w > 16384 || mode < VQAE_DW_SAME || mode > VQAE_DW_UP) return 0;
    if (mode == VQAE_DW_DOWN && (h % 2 || w % 2)) return 0;
    if (mode == VQAE_DW_UP && (h > 8192 || w > 8192)) return 0;
    return 1;
}

extern "C" size_t vqae_dwconv_train_workspace_bytes(int batch, int h, int w, int c, int mode) {
    if (batch < 1 || !vqae_dwconv_train_supported(c, h, w, mode)) return 0;
    const int64_t walked = mode == VQAE_DW_DOWN ? (int64_t)(h / 2) * (w / 2) : (int64_t)h * w;
    return (size_t)batch * (size_t)strips_of(walked) * (mode == VQAE_DW_SAME ? 9 : 4) * (size_t)c * sizeof(double) + 256;
}

extern "C" int vqae_dwconv_train_forward_f32(const float* x, const float* wgt, int mode, int batch, int h, int w, int c, float* y,
                                             void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = dw_check("dwconv_train_forward", batch, h, w, c, mode)) return rc;
    VQAE_REQUIRE(x && wgt && y, VQAE_ERR_INVALID, "dwconv_train_forward: null pointer");
    VQAE_REQUIRE(aligned16({x, y}), VQAE_ERR_INVALID, "dwconv_train_forward: tensors must be 16-byte aligned");
    return dw_launch(mode, x, wgt, 0, batch, h, w, c, y, stream);
}

extern "C" int vqae_dwconv_train_backward_f32(const float* g, const float* x, const float* wgt, int mode, int batch, int h, int w,
                                              int c, float* g_x, float* g_w, void* ws, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = dw_check("dwconv_train_backward", batch, h, w, c, mode)) return rc;
    VQAE_REQUIRE(g && (!g_x || wgt) && (!g_w || (x && ws)), VQAE_ERR_INVALID, "dwconv_train_backward: null pointer");
    VQAE_REQUIRE(aligned16({g, x, g_x}) && ((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID,
                 "dwconv_train_backward: tensors must be 16-byte, the workspace 8-byte aligned");
    int ho, wo;
    dw_out_dims(mode, h, w, &ho, &wo);
    if (g_x) {       // gathered: the 3x3 over g with flipped taps; the stride-2 modes are each other's adjoints
        const int adj = mode == VQAE_DW_SAME ? VQAE_DW_SAME : (mode == VQAE_DW_DOWN ? VQAE_DW_UP : VQAE_DW_DOWN);
        if (int rc = dw_launch(adj, g, wgt, mode == VQAE_DW_SAME, batch, ho, wo, c, g_x, stream)) return rc;
    }
    if (g_w) {
        const int hs = mode == VQAE_DW_DOWN ? ho : h, wsz = mode == VQAE_DW_DOWN ? wo : w;     // the walked (smaller) tensor
        const dim3 grid((unsigned)strips_of((int64_t)hs * wsz), (unsigned)batch);
        const int C4 = c / 4, taps = mode == VQAE_DW_SAME ? 9 : 4;
        const f32x4 *g4 = (const f32x4*)g, *x4 = (const f32x4*)x;
        double* partials = (double*)ws;
        if (mode == VQAE_DW_SAME) dwt_wgrad_kernel<0><<<grid, MBT_THREADS, 0, stream>>>(g4, x4, h, w, C4, hs, wsz, partials);
        else if (mode == VQAE_DW_DOWN) dwt_wgrad_kernel<1><<<grid, MBT_THREADS, 0, stream>>>(g4, x4, h, w, C4, hs, wsz, partials);
        else dwt_wgrad_kernel<2><<<grid, MBT_THREADS, 0, stream>>>(g4, x4, h, w, C4, hs, wsz, partials);
        VQAE_LAUNCH_CHECK();
        return finish(partials, 1, (int64_t)grid.x * grid.y, taps * c, taps, g_w, stream);
    }
    return VQAE_OK;
}

extern "C" size_t vqae_se_scale_workspace_bytes(int batch, int64_t hw, int c) {
    if (batch < 1 || hw < 1 || c < 1) return 0;
    return (size_t)batch * (size_t)strips_of(hw) * (size_t)c * sizeof(double) + 256;
}

extern "C" int vqae_se_scale_forward_f32(const float* x, const float* gate, int batch, int64_t hw, int c, float* y,
                                         void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_rows("se_scale_forward", batch, hw, c)) return rc;
    VQAE_REQUIRE(x && gate && y, VQAE_ERR_INVALID, "se_scale_forward: null pointer");
    VQAE_REQUIRE(aligned16({x, gate, y}), VQAE_ERR_INVALID, "se_scale_forward: tensors must be 16-byte aligned");
    se_scale_kernel<<<dim3((unsigned)strips_of(hw), (unsigned)batch), MBT_THREADS, 0, stream>>>(
        nullptr, (const f32x4*)x, (const f32x4*)gate, hw, c / 4, (f32x4*)y, nullptr);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" int vqae_se_scale_backward_f32(const float* g, const float* x, const float* gate, int batch, int64_t hw, int c,
                                          float* g_x, float* g_gate, void* ws, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_rows("se_scale_backward", batch, hw, c)) return rc;
    VQAE_REQUIRE(g && x && gate && g_x && g_gate && ws, VQAE_ERR_INVALID, "se_scale_backward: null pointer");
    VQAE_REQUIRE(aligned16({g, x, gate, g_x}) && ((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID,
                 "se_scale_backward: tensors must be 16-byte, the workspace 8-byte aligned");
    se_scale_kernel<<<dim3((unsigned)strips_of(hw), (unsigned)batch), MBT_THREADS, 0, stream>>>(
        (const f32x4*)g, (const f32x4*)x, (const f32x4*)gate, hw, c / 4, (f32x4*)g_x, (double*)ws);
    VQAE_LAUNCH_CHECK();
    return finish((double*)ws, batch, strips_of(hw), c, 0, g_gate, stream);
}
