// Backward of the VQ bottleneck (vq_ae/layers/vq.py:143-146 and :190-192): the gradients autograd derives for
//   loss      = commitment_cost * mse_loss(inputs, quantized)                   (vq.py:143)
//   quantized = inputs + (quantized - inputs).detach()                          (vq.py:146, straight-through)
//   out       = proj_out(quantized of proj_in(x))                               (vq.py:190-192)
// in closed form.  Rows are the channel-last flattening [N, .]; g_out / g_loss are the incoming gradients of the first
// output and of the 0-d loss, s = g_loss * commitment_cost * 2 / (N * D) (mse_loss's mean over N * D elements):
//   plain      g_x = g_out + s (x - q)
//   projected  g_q = g_out W_out          g_W_out = g_out^T q       g_b_out = sum_n g_out
//              g_z = g_q + s (z - q)      g_W_in  = g_z^T x         g_b_in  = sum_n g_z          g_x = g_z W_in
// Nothing flows into the codebook (embed / embed_avg / cluster_size are buffers, vq.py:27-34).  g_loss is read ON THE
// DEVICE, so a backward pass never synchronises.
//
// vq_proj_bwd_kernel: ONE pass over g_out and x, lane-owns-channels.  A wave instruction covers two rows: lane L works on
// row 2 i + (L >> 5) and on the channels 128 s + 4 (L & 31) .. + 3 of every 128-channel slab s -- a 16-byte load per lane and
// slab, two whole 512-byte row pieces per instruction (the store shape of vq_proj_fused_kernel).  The lane keeps the 4 x 8
// proj_out and proj_in weights of its channels in registers for the whole launch (C <= 128) or re-reads them from LDS
// (C <= 256).  Per step:
//   g_q   each lane's 4-channel partial of the 8 sums, then a reduce-scatter over the 32 lanes of the row (xor 16, 8, 4 halve
//         the sums a lane carries to 4, 2, 1; xor 2, 1 finish it): lane L ends with g_q[j], j = (L & 31) >> 2.  9 cross-lane
//         moves instead of the 40 of a butterfly on all 8 sums; the order of the adds is fixed, so the result is too
//   g_z   on the owning lane from its own z[j], q[j] (one 4-byte load each), then 8 + 8 cross-lane reads hand every lane
//         all of g_z and q
//   g_x   the lane's 4 channels: 8-term fp32 fma chains, one 16-byte store
//   sums  over the rows: g_out[c] q[j], g_z[j] x[c], g_out[c], g_z[j] -- each product of two fp32 is exact in fp64 and is
//         accumulated there (v_fma_f64), 17 accumulators per channel and lane.  No fp32 partial sum exists anywhere.
// A workgroup (4 waves) walks a contiguous range of rows whose length depends on (N) only; at the end its 8 lane sets are
// added through LDS in a fixed order and written as one fp64 row of the workspace; vq_proj_bwd_final adds the rows in a fixed
// order and rounds to fp32 once.  No floating-point atomics: gradients are bit-identical run to run.
#include <algorithm>

#include "kernels.h"
#include "mfma.h"

namespace {

using namespace vqae;

constexpr int PD = 8;                    // projection_dim
constexpr int BW_THREADS = 256;          // 4 waves
constexpr int BW_STEP_ROWS = 8;          // rows per workgroup step: 4 waves x 2 rows
constexpr int BW_MAX_WG = 512;           // rows of fp64 partials (C = 128: 8.9 MB)
constexpr int BW_MIN_ROWS = 256;         // rows per workgroup before the grid grows
constexpr int BW_MAX_C = 256;            // two slabs: 2 x 68 fp64 accumulators per lane is what the register file holds

struct VqBwdK {
    const float* __restrict__ g_out;     // [N][C] or null
    const float* __restrict__ x;         // [N][C]
    const float* __restrict__ z;         // [N][8]
    const float* __restrict__ q;         // [N][8]
    const float* __restrict__ g_loss;    // one fp32 or null
    const float* __restrict__ wt_in;     // [C][8]
    const float* __restrict__ w_out;     // [C][8]
    float* __restrict__ g_x;             // [N][C] or null
    double* __restrict__ partials;       // [n_wg][row_len]
    int64_t N, rows_per_wg;
    int C, row_len;
    float cc;
};

// layout of a partial row (and of the final kernel's index t): g_W_out [C][8] | g_W_in [8][C] | g_b_out [C] | g_b_in [8]
__host__ __device__ inline int bw_row_len(int C) { return 17 * C + PD; }

inline void bw_grid(int64_t N, int64_t* rows_per_wg, int* n_wg) {
    const int64_t want = std::min<int64_t>(BW_MAX_WG, ceil_div(N, BW_MIN_ROWS));
    *rows_per_wg = round_up(ceil_div(N, std::max<int64_t>(want, 1)), BW_STEP_ROWS);
    *n_wg = (int)ceil_div(N, *rows_per_wg);              // no workgroup without rows
}

template <int NSLAB, int U, bool WLDS>
__global__ __launch_bounds__(BW_THREADS)
void vq_proj_bwd_kernel(const VqBwdK p) {
    extern __shared__ __attribute__((aligned(16))) double red[];                      // [row_len] fp64, then (WLDS) w_out [C][8] and wt_in [C][8]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, cq = lane & 31;
    const int jo = cq >> 2;                              // the g_q / g_z element this lane ends up owning
    const bool b4 = (cq & 16) != 0, b3 = (cq & 8) != 0, b2 = (cq & 4) != 0;
    const int C = p.C;
    const bool has_go = p.g_out != nullptr;              // uniform
    const float* __restrict__ const gsrc = has_go ? p.g_out : p.x;   // always a readable address; zeroed below

    int c0[NSLAB];
    bool cv[NSLAB];
#pragma unroll
    for (int s = 0; s < NSLAB; ++s) {
        const int c = 128 * s + 4 * cq;
        cv[s] = c < C;                                   // C % 4 == 0: the lane's 4 channels are valid together
        c0[s] = cv[s] ? c : 0;                           // lanes past C: channel 0's addresses, inputs zeroed, nothing stored
    }
    // The weights of the lane's channels: in registers for the whole launch (one slab), or re-read from LDS at every step
    // (two slabs: the fp64 accumulators take the registers).  A lane past C gets channel 0's: its g_out and x are zeroed.
    float* const s_wo = reinterpret_cast<float*>(red + p.row_len);
    float* const s_wi = s_wo + C * PD;
    float wreg[WLDS ? 1 : NSLAB][2][4][PD];
    if constexpr (WLDS) {
        for (int i = tid; i < C * PD / 4; i += BW_THREADS) {
            reinterpret_cast<f32x4*>(s_wo)[i] = reinterpret_cast<const f32x4*>(p.w_out)[i];
            reinterpret_cast<f32x4*>(s_wi)[i] = reinterpret_cast<const f32x4*>(p.wt_in)[i];
        }
        __syncthreads();
    } else {
#pragma unroll
        for (int s = 0; s < NSLAB; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(p.w_out + (c0[s] + e) * PD);
                const f32x4 a1 = *reinterpret_cast<const f32x4*>(p.w_out + (c0[s] + e) * PD + 4);
                const f32x4 i0 = *reinterpret_cast<const f32x4*>(p.wt_in + (c0[s] + e) * PD);
                const f32x4 i1 = *reinterpret_cast<const f32x4*>(p.wt_in + (c0[s] + e) * PD + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    wreg[s][0][e][j] = a0[j]; wreg[s][0][e][j + 4] = a1[j];
                    wreg[s][1][e][j] = i0[j]; wreg[s][1][e][j + 4] = i1[j];
                }
            }
    }
    auto slab_weights = [&](int s, int which, float (&w)[4][PD]) {       // which: 0 proj_out, 1 proj_in (transposed)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (WLDS) {
                int off = (c0[s] + e) * PD;
                asm volatile("" : "+v"(off));             // opaque per step: the loads stay in the loop, not in 128 registers
                const float* src = (which ? s_wi : s_wo) + off;
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(src), a1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { w[e][j] = a0[j]; w[e][j + 4] = a1[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < PD; ++j) w[e][j] = wreg[s][which][e][j];
            }
        }
    };
    const float sc = p.g_loss ? (float)((double)*p.g_loss * (double)p.cc * 2.0 / ((double)p.N * (double)PD)) : 0.f;

    double a_wo[NSLAB][4][PD], a_wi[NSLAB][4][PD], a_bo[NSLAB][4], a_bi = 0.0;
#pragma unroll
    for (int s = 0; s < NSLAB; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a_bo[s][e] = 0.0;
#pragma unroll
            for (int j = 0; j < PD; ++j) { a_wo[s][e][j] = 0.0; a_wi[s][e][j] = 0.0; }
        }

    const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_wg;
    const int64_t r1 = r0 + p.rows_per_wg < p.N ? r0 + p.rows_per_wg : p.N;      // r0 < r1: bw_grid leaves no empty workgroup

    struct Step {
        f32x4 go[NSLAB], xv[NSLAB];
        float z, q;
    };
    // rows of step t of this wave: r0 + 8 t + 2 wave + half.  Rows past the range are clamped to its last row and masked.
    auto load_step = [&](int64_t t, Step& st) {
        const int64_t row = r0 + t * BW_STEP_ROWS + 2 * wave + half;
        const int64_t rr = row < r1 ? row : r1 - 1;
#pragma unroll
        for (int s = 0; s < NSLAB; ++s) {
            st.go[s] = *reinterpret_cast<const f32x4*>(gsrc + rr * C + c0[s]);
            st.xv[s] = *reinterpret_cast<const f32x4*>(p.x + rr * C + c0[s]);
        }
        st.z = p.z[rr * PD + jo];
        st.q = p.q[rr * PD + jo];
    };
    auto compute_step = [&](int64_t t, const Step& st) {
        const int64_t row = r0 + t * BW_STEP_ROWS + 2 * wave + half;
        const bool live = row < r1;
        f32x4 go[NSLAB], xv[NSLAB];
#pragma unroll
        for (int s = 0; s < NSLAB; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                go[s][e] = (live && has_go && cv[s]) ? st.go[s][e] : 0.f;
                xv[s][e] = (live && cv[s]) ? st.xv[s][e] : 0.f;
            }
        // ---- g_q: 4-channel partials, reduce-scatter over the row's 32 lanes ----------------------------------------
        float gq[PD];
#pragma unroll
        for (int j = 0; j < PD; ++j) gq[j] = 0.f;
#pragma unroll
        for (int s = 0; s < NSLAB; ++s) {
            float wo[4][PD];
            slab_weights(s, 0, wo);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < PD; ++j) gq[j] = __builtin_fmaf(go[s][e], wo[e][j], gq[j]);
        }
        float t4[4], t2[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float keep = b4 ? gq[4 + i] : gq[i], send = b4 ? gq[i] : gq[4 + i];
            t4[i] = keep + __shfl_xor(send, 16);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float keep = b3 ? t4[2 + i] : t4[i], send = b3 ? t4[i] : t4[2 + i];
            t2[i] = keep + __shfl_xor(send, 8);
        }
        float t1;
        {
            const float keep = b2 ? t2[1] : t2[0], send = b2 ? t2[0] : t2[1];
            t1 = keep + __shfl_xor(send, 4);
        }
        t1 += __shfl_xor(t1, 2);
        t1 += __shfl_xor(t1, 1);                           // g_q[jo] of the lane's row, the same bits in its 4 holders
        // ---- g_z on the owning lane, then every lane gets all of g_z and q -------------------------------------------
        const float gz_own = live ? t1 + sc * (st.z - st.q) : 0.f;
        float gz[PD], qv[PD];
#pragma unroll
        for (int j = 0; j < PD; ++j) {
            gz[j] = __shfl(gz_own, (lane & 32) + 4 * j);
            qv[j] = __shfl(st.q, (lane & 32) + 4 * j);
        }
        // ---- g_x -----------------------------------------------------------------------------------------------------
        if (p.g_x) {
#pragma unroll
            for (int s = 0; s < NSLAB; ++s) {
                float wi[4][PD];
                slab_weights(s, 1, wi);
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float a = 0.f;
#pragma unroll
                    for (int j = 0; j < PD; ++j) a = __builtin_fmaf(gz[j], wi[e][j], a);
                    o[e] = a;
                }
                if (live && cv[s]) *reinterpret_cast<f32x4*>(p.g_x + row * C + c0[s]) = o;
            }
        }
        // ---- the sums over the rows, in fp64 -----------------------------------------------------------------------------
        double gzd[PD], qd[PD];
#pragma unroll
        for (int j = 0; j < PD; ++j) { gzd[j] = (double)gz[j]; qd[j] = (double)qv[j]; }
#pragma unroll
        for (int s = 0; s < NSLAB; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double g = (double)go[s][e], xd = (double)xv[s][e];
#pragma unroll
                for (int j = 0; j < PD; ++j) {
                    a_wo[s][e][j] = __builtin_fma(g, qd[j], a_wo[s][e][j]);
                    a_wi[s][e][j] = __builtin_fma(gzd[j], xd, a_wi[s][e][j]);
                }
                a_bo[s][e] += g;
            }
        a_bi += (double)gz_own;
    };

    // U steps per trip; the next trip's rows are requested before this trip's arithmetic (the registers are the wave's
    // only way to keep loads in flight: its accumulators leave room for one wave per SIMD)
    const int64_t n_steps = (r1 - r0 + BW_STEP_ROWS - 1) / BW_STEP_ROWS;
    Step cur[U], nxt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) load_step(u, cur[u]);
    for (int64_t t = 0; t < n_steps; t += U) {
        const bool more = t + U < n_steps;               // uniform
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) load_step(t + U + u, nxt[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) compute_step(t + u, cur[u]);
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
    }

    // ---- the workgroup's 8 lane sets (wave, half), added in that order through LDS --------------------------------------
    for (int rep = 0; rep < 8; ++rep) {
        if (2 * wave + half == rep) {
#pragma unroll
            for (int s = 0; s < NSLAB; ++s) {
                if (!cv[s]) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = c0[s] + e;
#pragma unroll
                    for (int j = 0; j < PD; ++j) {
                        const int to = c * PD + j, ti = 8 * C + j * C + c;
                        red[to] = (rep ? red[to] : 0.0) + a_wo[s][e][j];
                        red[ti] = (rep ? red[ti] : 0.0) + a_wi[s][e][j];
                    }
                    red[16 * C + c] = (rep ? red[16 * C + c] : 0.0) + a_bo[s][e];
                }
            }
            if ((cq & 3) == 0) red[17 * C + jo] = (rep ? red[17 * C + jo] : 0.0) + a_bi;
        }
        __syncthreads();
    }
    double* __restrict__ const prow = p.partials + (int64_t)blockIdx.x * p.row_len;
    for (int t = tid; t < p.row_len; t += BW_THREADS) prow[t] = red[t];
}

// The partial rows added in a fixed order and rounded to fp32 once: a workgroup takes FIN_T elements of the row; slice
// ws of its FIN_W thread slices adds the rows [ws * per, (ws + 1) * per) in index order, thread slice 0 then adds the FIN_W
// slice sums in index order.  (One thread per element walking all rows alone -- 9 workgroups, up to 512 dependent adds behind
// as many loads -- cost more than the pass over the activations.)
constexpr int FIN_T = 16, FIN_W = 16;

__global__ __launch_bounds__(FIN_T * FIN_W)
void vq_proj_bwd_final(const double* __restrict__ partials, int n_wg, int row_len, int C, float* __restrict__ g_w_in,
                       float* __restrict__ g_b_in, float* __restrict__ g_w_out, float* __restrict__ g_b_out) {
    __shared__ double part[FIN_W][FIN_T];
    const int tl = threadIdx.x % FIN_T, ws = threadIdx.x / FIN_T;
    const int t = blockIdx.x * FIN_T + tl;
    const int per = (n_wg + FIN_W - 1) / FIN_W;
    const int w0 = ws * per, w1 = (w0 + per < n_wg) ? w0 + per : n_wg;
    double a = 0.0;
    if (t < row_len) {
#pragma unroll 8
        for (int w = w0; w < w1; ++w) a += partials[(int64_t)w * row_len + t];
    }
    part[ws][tl] = a;
    __syncthreads();
    if (ws != 0 || t >= row_len) return;
    for (int i = 1; i < FIN_W; ++i) a += part[i][tl];
    const float v = (float)a;
    if (t < 8 * C) { if (g_w_out) g_w_out[t] = v; }
    else if (t < 16 * C) { if (g_w_in) g_w_in[t - 8 * C] = v; }
    else if (t < 17 * C) { if (g_b_out) g_b_out[t - 16 * C] = v; }
    else if (g_b_in) g_b_in[t - 17 * C] = v;
}

// g_z = g_q + s (z - q), s = g_loss * cc * two_over_n; g_q null: 0; g_loss null: s = 0 (z, q are not read)
__global__ __launch_bounds__(256)
void vq_bwd_elem_kernel(const float* __restrict__ g_q, const float* __restrict__ z, const float* __restrict__ q,
                        const float* __restrict__ g_loss, float cc, double two_over_n, int64_t total, int64_t n4,
                        float* __restrict__ g_z) {
    const bool has_loss = g_loss != nullptr;
    const float sc = has_loss ? (float)((double)*g_loss * (double)cc * two_over_n) : 0.f;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (g_q) g = reinterpret_cast<const f32x4*>(g_q)[i];
        if (has_loss) {
            const f32x4 zv = reinterpret_cast<const f32x4*>(z)[i], qv = reinterpret_cast<const f32x4*>(q)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = g[e] + sc * (zv[e] - qv[e]);
        }
        reinterpret_cast<f32x4*>(g_z)[i] = g;
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        float g = g_q ? g_q[i] : 0.f;
        if (has_loss) g = g + sc * (z[i] - q[i]);
        g_z[i] = g;
    }
}

template <int NSLAB, int U, bool WLDS>
int launch_vq_proj_bwd(const VqBwdK& k, int n_wg, hipStream_t stream) {
    const size_t lds_bytes = (size_t)k.row_len * sizeof(double) + (WLDS ? (size_t)2 * k.C * PD * sizeof(float) : 0);   // <= 51 KB
    vq_proj_bwd_kernel<NSLAB, U, WLDS><<<n_wg, BW_THREADS, lds_bytes, stream>>>(k);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

}  // namespace

extern "C" int vqae_vq_backward_f32(const float* g_q, const float* z, const float* q, const float* g_loss, float commitment,
                                    int64_t N, int D, float* g_z, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VQAE_REQUIRE(N >= 0 && N < (1ll << 31), VQAE_ERR_INVALID, "vq_backward: n_rows %lld out of range", (long long)N);
    VQAE_REQUIRE(D >= 1 && D <= 4096, VQAE_ERR_UNSUPPORTED, "vq_backward: dim %d", D);
    if (N == 0) return VQAE_OK;
    VQAE_REQUIRE(g_z && (!g_loss || (z && q)), VQAE_ERR_INVALID, "vq_backward: null pointer");
    const int64_t total = N * D;
    const bool aligned = (((uintptr_t)g_q | (uintptr_t)z | (uintptr_t)q | (uintptr_t)g_z) & 15) == 0;
    const int64_t n4 = aligned ? total / 4 : 0;
    const unsigned grid = (unsigned)std::min<int64_t>(vqae::ceil_div(n4 > 0 ? n4 : total, 256), 8192);
    vq_bwd_elem_kernel<<<grid, 256, 0, stream>>>(g_q, z, q, g_loss, commitment, 2.0 / ((double)N * (double)D), total, n4, g_z);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" size_t vqae_vq_projected_backward_workspace_bytes(int64_t n_rows, int channels) {
    if (n_rows <= 0 || channels <= 0) return 256;
    int64_t rows_per_wg;
    int n_wg;
    bw_grid(n_rows, &rows_per_wg, &n_wg);
    return (size_t)n_wg * (size_t)bw_row_len(channels) * sizeof(double) + 256;
}

extern "C" int vqae_vq_projected_backward_f32(const float* g_out, const float* x, const float* z, const float* q,
                                              const float* g_loss, const float* wt_in, const float* w_out, int64_t N, int C,
                                              int D, float commitment, float* g_x, float* g_w_in, float* g_b_in,
                                              float* g_w_out, float* g_b_out, void* ws, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VQAE_REQUIRE(N >= 0 && N < (1ll << 31), VQAE_ERR_INVALID, "vq_projected_backward: n_rows %lld out of range", (long long)N);
    VQAE_REQUIRE(D == PD, VQAE_ERR_UNSUPPORTED, "vq_projected_backward: projection_dim %d (only %d is fused)", D, PD);
    VQAE_REQUIRE(C >= 4 && C % 4 == 0 && C <= BW_MAX_C, VQAE_ERR_UNSUPPORTED, "vq_projected_backward: channels %d", C);
    if (N == 0) {                                        // an empty batch: zero gradients
        if (g_w_in) VQAE_HIP_CHECK(hipMemsetAsync(g_w_in, 0, (size_t)PD * C * sizeof(float), stream));
        if (g_b_in) VQAE_HIP_CHECK(hipMemsetAsync(g_b_in, 0, PD * sizeof(float), stream));
        if (g_w_out) VQAE_HIP_CHECK(hipMemsetAsync(g_w_out, 0, (size_t)PD * C * sizeof(float), stream));
        if (g_b_out) VQAE_HIP_CHECK(hipMemsetAsync(g_b_out, 0, (size_t)C * sizeof(float), stream));
        return VQAE_OK;
    }
    VQAE_REQUIRE(x && z && q && wt_in && w_out && ws, VQAE_ERR_INVALID, "vq_projected_backward: null pointer");
    VqBwdK k;
    k.g_out = g_out; k.x = x; k.z = z; k.q = q; k.g_loss = g_loss; k.wt_in = wt_in; k.w_out = w_out; k.g_x = g_x;
    k.partials = (double*)ws;
    k.N = N; k.C = C; k.row_len = bw_row_len(C); k.cc = commitment;
    int n_wg;
    bw_grid(N, &k.rows_per_wg, &n_wg);
    int rc = C <= 128 ? launch_vq_proj_bwd<1, 4, false>(k, n_wg, stream) : launch_vq_proj_bwd<2, 1, true>(k, n_wg, stream);
    if (rc) return rc;
    if (g_w_in || g_b_in || g_w_out || g_b_out) {
        vq_proj_bwd_final<<<(unsigned)vqae::ceil_div(k.row_len, FIN_T), FIN_T * FIN_W, 0, stream>>>(k.partials, n_wg, k.row_len, C, g_w_in, g_b_in,
                                                                                        g_w_out, g_b_out);
        VQAE_LAUNCH_CHECK();
    }
    return VQAE_OK;
}
