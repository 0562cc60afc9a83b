// Per-image reconstruction metrics (MSE, Huber, PSNR, SSIM) of a batch of reconstructions against their targets (gfx950):
// the metrics the reference's validation logs (vq_ae/model.py:82-93; conf/model/metrics/{mse,psnr,ssim}.yaml,
// conf/model/loss_f/huber.yaml; torchmetrics 0.8.2 semantics, restated in metrics.py and DESIGN.md section 9).
//
// Four launches, no atomics; every partition depends on the image shape only, never on the batch, so an image's results are
// bit-identical run to run and whatever batch it sits in:
//   1. stats_kernel      streaming: per (image, chunk) fp64 sums of d^2 and huber(d), fp32 min / max of p and t -> workspace
//   2. stats_final       per image, chunks summed in fixed order in fp64 -> mse, huber, psnr, min / max           -> out
//   3. ssim_kernel       per (image, output tile), all channels: the 11x11 Gaussian moments over the valid window centres
//                        (separable: horizontal 11-tap pass from LDS, vertical pass as a per-thread 11-row register ring),
//                        s summed in fp64 per thread and per workgroup                                          -> workspace
//   4. ssim_final        per image, tiles summed in fixed order in fp64 / (C (H-10) (W-10))                      -> out
// The u8 target form normalises (u - mean255[c]) * inv_std255[c] on the fly (as vqae_conv3x3_direct_f32 does), so the target
// never exists in fp32.
#include "common.h"
#include "mfma.h"

#include <cmath>

namespace {

using namespace vqae;

constexpr int K = VQAE_METRICS_K;
constexpr int NSTAT = 6;            // pass-1 partial row: sum d^2, sum huber, pmin, pmax, tmin, tmax (as double)
constexpr int T1 = 256;             // pass-1 threads
constexpr int NB1_MAX = 64;         // pass-1 workgroups per image
constexpr int TW = 128;             // SSIM: output columns per workgroup (one per thread)
constexpr int WIN = 11;             // window = rows per staged chunk, so the ring slot of every unrolled phase is static
constexpr int TH = 56;              // SSIM: output rows per workgroup (TH + 10 = 66 input rows = 6 chunks)
constexpr int IW = TW + WIN - 1;    // staged input columns

// torchmetrics 0.8.2 `_gaussian(11, 1.5)`: exp(-(k / 1.5)^2 / 2), k = -5 .. 5, normalised to sum 1 -- its fp32 values
__constant__ const float kG[WIN] = {0.0010283804f, 0.007598756f, 0.036000773f, 0.10936068f, 0.21300553f, 0.26601171f,
                                    0.21300553f,   0.10936068f,  0.036000773f, 0.007598756f, 0.0010283804f};

// target kinds: fp32 in the prediction's layout | uint8 NHWC (prediction NHWC) | uint8 NHWC (prediction NCHW)
enum { TK_F32 = 0, TK_U8_SAME = 1, TK_U8_NCHW = 2 };

int stats_blocks(int64_t n, int64_t* chunk) {
    const int64_t nb = std::min<int64_t>(NB1_MAX, std::max<int64_t>(1, vqae::ceil_div(n, T1 * 16)));
    *chunk = vqae::round_up(vqae::ceil_div(n, nb), 4);
    return (int)vqae::ceil_div(n, *chunk);
}

void ssim_tiles(int h, int w, int* tx, int* ty) {
    *tx = (int)vqae::ceil_div(w - (WIN - 1), TW);
    *ty = (int)vqae::ceil_div(h - (WIN - 1), TH);
}

size_t stats_bytes(int batch, int64_t n) {
    int64_t chunk;
    return (size_t)vqae::round_up((int64_t)batch * stats_blocks(n, &chunk) * NSTAT * 8, 256);
}

// ---- pass 1 --------------------------------------------------------------------------------------------------------------
template <int VEC, int TK>
__global__ __launch_bounds__(T1) void stats_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                   const uint8_t* __restrict__ tgt_u8, Norm3 nrm, int C, int64_t hw,
                                                   int64_t n, int64_t chunk, float delta, double* __restrict__ part) {
    const int b = blockIdx.y, j = blockIdx.x, nb = gridDim.x;
    const int64_t lo = (int64_t)j * chunk, hi = std::min(lo + chunk, n);
    const float* p = pred + (int64_t)b * n;
    const float* t = tgt ? tgt + (int64_t)b * n : nullptr;
    const uint8_t* u = tgt_u8 ? tgt_u8 + (int64_t)b * n : nullptr;
    const double dd = delta;
    double s2 = 0.0, sh = 0.0;
    float pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY;
    for (int64_t i = lo + (int64_t)threadIdx.x * VEC; i < hi; i += (int64_t)T1 * VEC) {   // lo, hi, n: multiples of VEC
        float pv[VEC], tv[VEC];
        if constexpr (VEC == 4) {
            const float4 a = *reinterpret_cast<const float4*>(p + i);
            pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
        } else {
            pv[0] = p[i];
        }
        if constexpr (TK == TK_F32) {
            if constexpr (VEC == 4) {
                const float4 a = *reinterpret_cast<const float4*>(t + i);
                tv[0] = a.x; tv[1] = a.y; tv[2] = a.z; tv[3] = a.w;
            } else {
                tv[0] = t[i];
            }
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                int c;
                int64_t ti;
                if constexpr (TK == TK_U8_SAME) {
                    c = (int)((i + e) % C);
                    ti = i + e;
                } else {                                      // prediction NCHW, target NHWC
                    c = (int)((i + e) / hw);
                    ti = ((i + e) - c * hw) * C + c;
                }
                tv[e] = ((float)u[ti] - nrm.mean[c]) * nrm.inv[c];
            }
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const double d = (double)(pv[e] - tv[e]);
            const double ad = fabs(d);
            s2 = fma(d, d, s2);
            sh += ad < dd ? 0.5 * d * d : dd * (ad - 0.5 * dd);
            pmin = fminf(pmin, pv[e]); pmax = fmaxf(pmax, pv[e]);
            tmin = fminf(tmin, tv[e]); tmax = fmaxf(tmax, tv[e]);
        }
    }
    s2 = wave_sum(s2); sh = wave_sum(sh);
    pmin = wave_min(pmin); pmax = wave_max(pmax); tmin = wave_min(tmin); tmax = wave_max(tmax);
    __shared__ double red[T1 / 64][NSTAT];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wv][0] = s2; red[wv][1] = sh; red[wv][2] = pmin; red[wv][3] = pmax; red[wv][4] = tmin; red[wv][5] = tmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r[NSTAT] = {red[0][0], red[0][1], red[0][2], red[0][3], red[0][4], red[0][5]};
        for (int w = 1; w < T1 / 64; ++w) {
            r[0] += red[w][0]; r[1] += red[w][1];
            r[2] = fmin(r[2], red[w][2]); r[3] = fmax(r[3], red[w][3]);
            r[4] = fmin(r[4], red[w][4]); r[5] = fmax(r[5], red[w][5]);
        }
        double* o = part + ((int64_t)b * nb + j) * NSTAT;
        for (int k = 0; k < NSTAT; ++k) o[k] = r[k];
    }
}

__global__ void stats_final(const double* __restrict__ part, int batch, int nb, int64_t n, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const double* q = part + (int64_t)b * nb * NSTAT;
    double r[NSTAT] = {q[0], q[1], q[2], q[3], q[4], q[5]};
    for (int j = 1; j < nb; ++j) {
        const double* s = q + (int64_t)j * NSTAT;
        r[0] += s[0]; r[1] += s[1];
        r[2] = fmin(r[2], s[2]); r[3] = fmax(r[3], s[3]); r[4] = fmin(r[4], s[4]); r[5] = fmax(r[5], s[5]);
    }
    double* o = out + (int64_t)b * K;
    const double mse = r[0] / (double)n, rt = r[5] - r[4];
    o[VQAE_METRIC_MSE] = mse;
    o[VQAE_METRIC_HUBER] = r[1] / (double)n;
    o[VQAE_METRIC_PSNR] = 10.0 * log10(rt * rt / mse);      // mse = 0 -> +inf (torchmetrics 0.8.2 likewise)
    o[VQAE_METRIC_PRED_MIN] = r[2]; o[VQAE_METRIC_PRED_MAX] = r[3];
    o[VQAE_METRIC_TARGET_MIN] = r[4]; o[VQAE_METRIC_TARGET_MAX] = r[5];
}

// ---- pass 2: SSIM ---------------------------------------------------------------------------------------------------------
template <int NCHW, int TK>
__device__ __forceinline__ void load_pt(const float* __restrict__ pred, const float* __restrict__ tgt,
                                        const uint8_t* __restrict__ tgt_u8, const Norm3& nrm, int b, int c, int C, int H,
                                        int W, int y, int x, float& pv, float& tv) {
    const int64_t pi = NCHW ? (((int64_t)b * C + c) * H + y) * W + x : (((int64_t)b * H + y) * W + x) * C + c;
    pv = pred[pi];
    if constexpr (TK == TK_F32) {
        tv = tgt[pi];
    } else {
        const int64_t ti = (((int64_t)b * H + y) * W + x) * C + c;
        tv = ((float)tgt_u8[ti] - nrm.mean[c]) * nrm.inv[c];
    }
}

constexpr int PER_T = (WIN * IW + TW - 1) / TW;    // staged elements per thread and tensor

template <int NCHW, int TK>
__global__ __launch_bounds__(TW) void ssim_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                  const uint8_t* __restrict__ tgt_u8, Norm3 nrm, int C, int H, int W,
                                                  int tiles_x, const double* __restrict__ stats, double* __restrict__ part) {
    __shared__ float sp[WIN][IW], st[WIN][IW];
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int Ho = H - (WIN - 1), Wo = W - (WIN - 1);
    const int x0 = (tile % tiles_x) * TW, y0 = (tile / tiles_x) * TH;
    const int rows_in = min(TH, Ho - y0) + WIN - 1;       // input rows y0 .. y0 + rows_in - 1, all < H
    const int cols_in = min(TW, Wo - x0) + WIN - 1;       // input cols x0 .. x0 + cols_in - 1, all < W
    const bool active = tid < cols_in - (WIN - 1);         // this thread's output column x0 + tid is a valid centre
    const double* sb = stats + (int64_t)b * K;
    // torchmetrics 0.8.2: data_range = max(preds.max() - preds.min(), target.max() - target.min()), c = (k * data_range)^2, fp32
    const float r = fmaxf((float)sb[VQAE_METRIC_PRED_MAX] - (float)sb[VQAE_METRIC_PRED_MIN],
                          (float)sb[VQAE_METRIC_TARGET_MAX] - (float)sb[VQAE_METRIC_TARGET_MIN]);
    const float c1 = (0.01f * r) * (0.01f * r), c2 = (0.03f * r) * (0.03f * r);
    double acc = 0.0;

    for (int c = 0; c < C; ++c) {
        float rp[PER_T], rt[PER_T];
        auto fetch = [&](int chunk) {
#pragma unroll
            for (int i = 0; i < PER_T; ++i) {
                const int e = tid + i * TW, lr = e / IW, lc = e - lr * IW, row = chunk * WIN + lr;
                rp[i] = 0.f; rt[i] = 0.f;
                if (e < WIN * IW && row < rows_in && lc < cols_in)
                    load_pt<NCHW, TK>(pred, tgt, tgt_u8, nrm, b, c, C, H, W, y0 + row, x0 + lc, rp[i], rt[i]);
            }
        };
        float ring[WIN][5];
        fetch(0);
        for (int chunk = 0; chunk * WIN < rows_in; ++chunk) {
            vqae::lds_barrier();                           // every thread is done with the previous chunk
#pragma unroll
            for (int i = 0; i < PER_T; ++i) {
                const int e = tid + i * TW;
                if (e < WIN * IW) {
                    const int lr = e / IW, lc = e - lr * IW;
                    sp[lr][lc] = rp[i]; st[lr][lc] = rt[i];
                }
            }
            vqae::lds_barrier();
            if ((chunk + 1) * WIN < rows_in) fetch(chunk + 1);     // in flight while this chunk is filtered
#pragma unroll
            for (int ph = 0; ph < WIN; ++ph) {
                const int row = chunk * WIN + ph;                  // workgroup-uniform
                if (row < rows_in) {
                    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;   // horizontal moments of p, t, pp, tt, pt
#pragma unroll
                    for (int k = 0; k < WIN; ++k) {
                        const float a = sp[ph][tid + k], v = st[ph][tid + k], g = kG[k];
                        m0 = fmaf(g, a, m0); m1 = fmaf(g, v, m1);
                        m2 = fmaf(g, a * a, m2); m3 = fmaf(g, v * v, m3); m4 = fmaf(g, a * v, m4);
                    }
                    ring[ph][0] = m0; ring[ph][1] = m1; ring[ph][2] = m2; ring[ph][3] = m3; ring[ph][4] = m4;
                    if (row >= WIN - 1) {                              // output row y0 + row - 10: rows row-10 .. row are in the ring
                        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f;
#pragma unroll
                        for (int k = 0; k < WIN; ++k) {
                            const int s = (ph + 1 + k) % WIN;          // compile-time after unrolling
                            const float g = kG[k];
                            v0 = fmaf(g, ring[s][0], v0); v1 = fmaf(g, ring[s][1], v1); v2 = fmaf(g, ring[s][2], v2);
                            v3 = fmaf(g, ring[s][3], v3); v4 = fmaf(g, ring[s][4], v4);
                        }
                        // torchmetrics 0.8.2 `_ssim_compute`, its op order (un-centred moments)
                        const float mpp = v0 * v0, mtt = v1 * v1, mpt = v0 * v1;
                        const float spp = v2 - mpp, stt = v3 - mtt, spt = v4 - mpt;
                        const float upper = 2.f * spt + c2, lower = spp + stt + c2;
                        const float s = ((2.f * mpt + c1) * upper) / ((mpp + mtt + c1) * lower);
                        if (active) acc += (double)s;
                    }
                }
            }
        }
    }
    acc = wave_sum(acc);
    __shared__ double red[TW / 64];
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double sum = red[0];
        for (int w = 1; w < TW / 64; ++w) sum += red[w];
        part[(int64_t)b * gridDim.x + tile] = sum;
    }
}

__global__ void ssim_final(const double* __restrict__ part, int batch, int ntiles, double count, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const double* q = part + (int64_t)b * ntiles;
    double s = 0.0;
    for (int j = 0; j < ntiles; ++j) s += q[j];
    out[(int64_t)b * K + VQAE_METRIC_SSIM] = s / count;
}

template <int VEC, int TK>
void launch_stats(dim3 g, hipStream_t st, const float* p, const float* t, const uint8_t* u, const Norm3& nrm, int C,
                  int64_t hw, int64_t n, int64_t chunk, float delta, double* part) {
    stats_kernel<VEC, TK><<<g, T1, 0, st>>>(p, t, u, nrm, C, hw, n, chunk, delta, part);
}

template <int NCHW, int TK>
void launch_ssim(dim3 g, hipStream_t st, const float* p, const float* t, const uint8_t* u, const Norm3& nrm, int C, int H,
                 int W, int tiles_x, const double* stats, double* part) {
    ssim_kernel<NCHW, TK><<<g, TW, 0, st>>>(p, t, u, nrm, C, H, W, tiles_x, stats, part);
}

}  // namespace

extern "C" size_t vqae_recon_metrics_workspace_bytes(int batch, int channels, int h, int w) {
    if (batch <= 0 || channels <= 0 || h < WIN || w < WIN) return 0;
    int tx, ty;
    ssim_tiles(h, w, &tx, &ty);
    return stats_bytes(batch, (int64_t)channels * h * w) + (size_t)vqae::round_up((int64_t)batch * tx * ty * 8, 256);
}

extern "C" int vqae_recon_metrics_f32(const float* pred_dev, const float* target_dev, const uint8_t* target_u8_dev,
                                      const float* mean255, const float* inv_std255, int batch, int channels, int h, int w,
                                      int layout, float huber_delta, double* out_dev, void* workspace_dev, void* stream) {
    using vqae::fail;
    VQAE_REQUIRE(pred_dev && out_dev && workspace_dev, VQAE_ERR_INVALID, "recon_metrics: null pointer");
    VQAE_REQUIRE((target_dev != nullptr) != (target_u8_dev != nullptr), VQAE_ERR_INVALID,
                 "recon_metrics: pass exactly one of target_dev / target_u8_dev");
    VQAE_REQUIRE(batch >= 0 && channels >= 1 && h >= 1 && w >= 1, VQAE_ERR_INVALID,
                 "recon_metrics: bad shape batch=%d channels=%d h=%d w=%d", batch, channels, h, w);
    VQAE_REQUIRE(layout == VQAE_LAYOUT_NHWC || layout == VQAE_LAYOUT_NCHW, VQAE_ERR_INVALID, "recon_metrics: bad layout %d",
                 layout);
    VQAE_REQUIRE(std::isfinite(huber_delta) && huber_delta > 0.f, VQAE_ERR_INVALID, "recon_metrics: huber_delta must be > 0");
    VQAE_REQUIRE(h >= WIN && w >= WIN, VQAE_ERR_VALUE,
                 "recon_metrics: SSIM needs an image of at least 11 x 11 (the Gaussian window), got h=%d w=%d", h, w);
    VQAE_REQUIRE(!target_u8_dev || channels == 3, VQAE_ERR_UNSUPPORTED, "recon_metrics: a uint8 target needs 3 channels");
    VQAE_REQUIRE(batch <= 65535, VQAE_ERR_UNSUPPORTED, "recon_metrics: batch %d > 65535", batch);
    if (batch == 0) return VQAE_OK;

    Norm3 nrm;
    for (int i = 0; i < 4; ++i) {
        nrm.mean[i] = (mean255 && i < 3) ? mean255[i] : 0.f;
        nrm.inv[i] = (inv_std255 && i < 3) ? inv_std255[i] : 1.f;
    }
    const hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)h * w, n = hw * channels;
    int64_t chunk;
    const int nb = stats_blocks(n, &chunk);
    int tx, ty;
    ssim_tiles(h, w, &tx, &ty);
    double* part1 = (double*)workspace_dev;
    double* part2 = (double*)((char*)workspace_dev + stats_bytes(batch, n));
    const bool nchw = layout == VQAE_LAYOUT_NCHW;
    const int tk = target_dev ? TK_F32 : (nchw ? TK_U8_NCHW : TK_U8_SAME);
    // float4 loads when every image starts 16-byte aligned (and a u8 target's 4-byte groups 4-byte aligned)
    const bool vec = n % 4 == 0 && (uintptr_t)pred_dev % 16 == 0 &&
                     (target_dev ? (uintptr_t)target_dev % 16 == 0 : (uintptr_t)target_u8_dev % 4 == 0);

    const dim3 g1(nb, batch);
    if (vec) {
        if (tk == TK_F32) launch_stats<4, TK_F32>(g1, st, pred_dev, target_dev, target_u8_dev, nrm, channels, hw, n, chunk, huber_delta, part1);
        else if (tk == TK_U8_SAME) launch_stats<4, TK_U8_SAME>(g1, st, pred_dev, target_dev, target_u8_dev, nrm, channels, hw, n, chunk, huber_delta, part1);
        else launch_stats<4, TK_U8_NCHW>(g1, st, pred_dev, target_dev, target_u8_dev, nrm, channels, hw, n, chunk, huber_delta, part1);
    } else {
        if (tk == TK_F32) launch_stats<1, TK_F32>(g1, st, pred_dev, target_dev, target_u8_dev, nrm, channels, hw, n, chunk, huber_delta, part1);
        else if (tk == TK_U8_SAME) launch_stats<1, TK_U8_SAME>(g1, st, pred_dev, target_dev, target_u8_dev, nrm, channels, hw, n, chunk, huber_delta, part1);
        else launch_stats<1, TK_U8_NCHW>(g1, st, pred_dev, target_dev, target_u8_dev, nrm, channels, hw, n, chunk, huber_delta, part1);
    }
    VQAE_LAUNCH_CHECK();
    stats_final<<<(unsigned)vqae::ceil_div(batch, 64), 64, 0, st>>>(part1, batch, nb, n, out_dev);
    VQAE_LAUNCH_CHECK();

    const dim3 g2(tx * ty, batch);
    if (nchw) {
        if (tk == TK_F32) launch_ssim<1, TK_F32>(g2, st, pred_dev, target_dev, target_u8_dev, nrm, channels, h, w, tx, out_dev, part2);
        else launch_ssim<1, TK_U8_NCHW>(g2, st, pred_dev, target_dev, target_u8_dev, nrm, channels, h, w, tx, out_dev, part2);
    } else {
        if (tk == TK_F32) launch_ssim<0, TK_F32>(g2, st, pred_dev, target_dev, target_u8_dev, nrm, channels, h, w, tx, out_dev, part2);
        else launch_ssim<0, TK_U8_SAME>(g2, st, pred_dev, target_dev, target_u8_dev, nrm, channels, h, w, tx, out_dev, part2);
    }
    VQAE_LAUNCH_CHECK();
    ssim_final<<<(unsigned)vqae::ceil_div(batch, 64), 64, 0, st>>>(part2, batch, tx * ty,
                                                                   (double)channels * (h - (WIN - 1)) * (w - (WIN - 1)), out_dev);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}
