// Training the slide classifier on stored code grids (gfx950): Camelyon16BCELoss (utils/train_helpers.py:101-138) and the
// gradients of all seven parameter tensors of the validation_nn CNNClassifier (validation_nn/model.py:131-139, the `step`
// whose loss Lightning differentiates) without one activation tensor in HBM.
//
//   launch 1  the forward tile kernel of classifier.hip with stats, which also stores g = dL/dlogit (fp32, 4 B per code)
//   launch 2  classifier_backward_kernel: a workgroup walks output tiles of TH x TW codes (the forward's tile sizes) and, per
//             tile, recomputes from the codes
//               E0 on tile + 4, A = ELU(in_conv) on tile + 3, B = ELU(hidden_conv1) on tile + 2      (0 outside the grid)
//             reads g on tile + 3 (0 outside the grid), and forms in LDS, in place,
//               dB = elu'(B) * (w3 transposed * g)  on tile + 2   (over B)
//               dA = elu'(A) * (w2 transposed * dB) on tile + 1   (over A)
//             elu' = 1 where the activation is > 0, activation + 1 elsewhere; both 0 outside the grid, so no gradient
//             flows through the constant-zero border.  Every weight gradient is a correlation
//               dW[cin][tap][cout] = sum over the positions q OF THE TILE of D[cout][q] * X[cin][q + tap]
//             (D, X) = (g, B), (dB, A), (dA, E0), and the bias gradient is the sum of D: a position belongs to exactly one
//             tile, so nothing is counted twice.  The embedding gradient dE0 = w1 transposed * dA on the tile is scattered
//             by code.
//   launch 3  train_final: adds the workgroups' rows in order, in fp64, and scales by 1 / n_valid for reduction = mean.
//
// Reduction.  A thread owns one (cin, cout) pair and a fixed slice of the tile's positions for each correlation: its 9 taps
// and the bias term are summed in fp32 over runs of 32 positions and then in fp64 registers, over all the tiles of its
// workgroup (tile g, g + G, g + 2G ... of the batch, G = min(tiles, 512) workgroups: a function of the shape alone).  At
// the end the slices of a pair are added in slice order through LDS and the workgroup writes ONE fp64 row; launch 3 adds the
// rows in row order.  No floating-point atomics and no dependence on timing: bit-identical run to run.
// The table gradient is a scatter by code.  Each addend is rounded to 64-bit fixed point with 30 fraction bits
// (resolution 2^-30 = 9.3e-10, range +-8.6e9 per table entry) and added with INTEGER atomics -- in an LDS copy of the table
// gradient while K * E <= 2048, flushed once per workgroup, and straight into the [K][E] buffer in HBM for larger tables.
// Integer addition is associative, so the sum does not depend on the order the atomics land in.
#include "classifier_impl.h"

#include <cmath>

using namespace vqae_cls;

namespace {

constexpr int MAX_WG = 512;             // rows of weight-gradient partials: the fp64 workspace stays below 11 MB
constexpr int EMB_LDS_MAX = 2048;       // table entries whose fixed-point gradient is accumulated in LDS (16 KB)
constexpr double FIX_ONE = 1073741824.0;   // 2^30

// What a thread owns in one correlation: the (cin, cout) pair and the tile positions q0 .. q1-1 (row-major over TH x TW).
struct Slice { int ci, co, q0, q1; };

template <int TW>
__device__ __forceinline__ Slice make_slice(int tid, int nci, int nco) {
    const int np = nci * nco, ng = NT / np, grp = tid / np, p = tid - grp * np;
    const int npos = TH * TW, chunk = (npos + ng - 1) / ng;
    Slice s;
    s.ci = p / nco; s.co = p - s.ci * nco;
    s.q0 = grp < ng ? min(npos, grp * chunk) : 0;
    s.q1 = grp < ng ? min(npos, s.q0 + chunk) : 0;
    return s;
}

// acc[t] += sum over the slice of D[co][q] * X[ci][q + tap t] (t < 9), acc[9] += sum of D[co][q].  d0: the tile's origin
// in D's plane; x0: the tile's origin minus (1, 1) in X's plane.
template <int TW>
__device__ __forceinline__ void correlate(const Slice& s, const float* __restrict__ D, int dn, int dw, int d0,
                                          const float* __restrict__ X, int xn, int xw, int x0, double acc[10]) {
    float a[10];
#pragma unroll
    for (int t = 0; t < 10; ++t) a[t] = 0.0f;
    const float* dp = D + s.co * dn + d0;
    const float* xp = X + s.ci * xn + x0;
    int run = 0;
    for (int q = s.q0; q < s.q1; ++q) {
        const int y = q / TW, x = q - y * TW;
        const float d = dp[y * dw + x];
        const float* xq = xp + y * xw + x;
#pragma unroll
        for (int t = 0; t < 9; ++t) a[t] = fmaf(d, xq[(t / 3) * xw + (t % 3)], a[t]);
        a[9] += d;
        if (++run == 32) {
            run = 0;
#pragma unroll
            for (int t = 0; t < 10; ++t) { acc[t] += (double)a[t]; a[t] = 0.0f; }
        }
    }
#pragma unroll
    for (int t = 0; t < 10; ++t) acc[t] += (double)a[t];
}

// The slices of each pair, added in slice order: weight [cout][cin][3][3] and bias [cout] in PyTorch's layout.
__device__ __forceinline__ void reduce_slices(double* red, const double acc[10], int nci, int nco, double* __restrict__ w_out,
                                              double* __restrict__ b_out) {
    const int tid = threadIdx.x;
    __syncthreads();                                              // red is free (planes dead, or the previous reduction read)
#pragma unroll
    for (int t = 0; t < 10; ++t) red[tid * 10 + t] = acc[t];
    __syncthreads();
    const int np = nci * nco, ng = NT / np;
    for (int j = tid; j < np * 10; j += NT) {
        const int p = j / 10, t = j - p * 10;
        double r = red[p * 10 + t];
        for (int g = 1; g < ng; ++g) r += red[(g * np + p) * 10 + t];
        const int ci = p / nco, co = p - ci * nco;
        if (t < 9) w_out[(co * nci + ci) * 9 + t] = r;
        else if (ci == 0) b_out[co] = r;
    }
}

template <int C, int NO, int TW>
__global__ __launch_bounds__(NT)
void classifier_backward_kernel(const void* __restrict__ codes, int idx_dtype, int H, int W, int tiles_x, int ntiles, int64_t total,
                                const float* __restrict__ table, int K, int E,
                                const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                const float* __restrict__ b2, const float* __restrict__ w3,
                                const float* __restrict__ glogit, int emb_lds, unsigned long long* __restrict__ emb_fix,
                                double* __restrict__ rows, int row_len) {
    constexpr int EH = TH + 8, EW = TW + 8, EN = EH * EW;         // embedding: tile + 4
    constexpr int AH = TH + 6, AW = TW + 6, AN = AH * AW;         // layer 1 and g: tile + 3
    constexpr int BH = TH + 4, BW = TW + 4, BN = BH * BW;         // layer 2: tile + 2
    constexpr int DW = TW + 2, DN = (TH + 2) * DW;                // dA: tile + 1
    static_assert(NT * 10 * 8 <= C * AN * 4, "the slice reduction reuses plane A");
    extern __shared__ double lds_d[];
    unsigned long long* const pfix = (unsigned long long*)lds_d;              // [K][E] fixed-point table gradient when emb_lds
    float* const pa = (float*)(lds_d + (emb_lds ? K * E : 0));   // A [C][AH][AW], then dA on its tile + 1
    float* const pb = pa + C * AN;                                // B [C][BH][BW], then dB
    float* const pg = pb + C * BN;                                // g [NO][AH][AW]
    float* const pe = pg + NO * AN;                               // E0 [E][EH][EW]
    const int tid = threadIdx.x;
    const int64_t hw = (int64_t)H * W;

    if (emb_lds)
        for (int i = tid; i < K * E; i += NT) pfix[i] = 0ull;

    const Slice s3 = make_slice<TW>(tid, C, NO), s2 = make_slice<TW>(tid, C, C), s1 = make_slice<TW>(tid, E, C);
    double acc3[10], acc2[10], acc1[10];
#pragma unroll
    for (int t = 0; t < 10; ++t) acc3[t] = acc2[t] = acc1[t] = 0.0;

    for (int64_t gt = blockIdx.x; gt < total; gt += gridDim.x) {
        const int b = (int)(gt / ntiles), tile = (int)(gt - (int64_t)b * ntiles);
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int y0 = ty * TH, x0 = tx * TW;
        __syncthreads();                                          // the previous tile's readers are done (and pfix is zero)

        // ---- embedding on tile + 4, g on tile + 3 ------------------------------------------------------------------------
        for (int i = tid; i < EN; i += NT) {
            const int ly = i / EW, lx = i - ly * EW;
            const int gy = y0 - 4 + ly, gx = x0 - 4 + lx;
            int64_t code = -1;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) code = load_code(codes, idx_dtype, (int64_t)b * hw + (int64_t)gy * W + gx);
            const bool ok = code >= 0 && code < K;
            const int64_t row = ok ? code * E : 0;
            for (int e = 0; e < E; ++e) pe[e * EN + i] = ok ? table[row + e] : 0.0f;
        }
        for (int i = tid; i < AN; i += NT) {
            const int ly = i / AW, lx = i - ly * AW;
            const int gy = y0 - 3 + ly, gx = x0 - 3 + lx;
            if constexpr (NO == 1) {                               // (spelled as before NO existed, here and in the out-conv
                                                                  //  correlation's plane stride: the n_out = 1 kernels
                                                                  //  compile to the instruction stream they had)
                pg[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? glogit[(int64_t)b * hw + (int64_t)gy * W + gx] : 0.0f;
            } else {
                const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
                for (int o = 0; o < NO; ++o)
                    pg[o * AN + i] = inside ? glogit[((int64_t)b * NO + o) * hw + (int64_t)gy * W + gx] : 0.0f;
            }
        }
        __syncthreads();

        // ---- A = ELU(in_conv) on tile + 3: the forward's sums, in the forward's order ------------------------------------
        for (int i = tid; i < AN; i += NT) {
            const int ly = i / AW, lx = i - ly * AW;
            const int gy = y0 - 3 + ly, gx = x0 - 3 + lx;
            float acc[C];
#pragma unroll
            for (int co = 0; co < C; ++co) acc[co] = b1[co];
#pragma unroll 1
            for (int e = 0; e < E; ++e) {
                const float* ep = pe + e * EN + ly * EW + lx;
                const float* wp = w1 + e * 9 * C;
                float in[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) in[t] = ep[(t / 3) * EW + (t % 3)];
#pragma unroll
                for (int t = 0; t < 9; ++t)
#pragma unroll
                    for (int co = 0; co < C; ++co) acc[co] = fmaf(wp[t * C + co], in[t], acc[co]);
            }
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
            for (int co = 0; co < C; ++co) pa[co * AN + i] = inside ? elu1(acc[co]) : 0.0f;
        }
        __syncthreads();

        // ---- B = ELU(hidden_conv1) on tile + 2 ---------------------------------------------------------------------------
        for (int i = tid; i < BN; i += NT) {
            const int ly = i / BW, lx = i - ly * BW;
            const int gy = y0 - 2 + ly, gx = x0 - 2 + lx;
            float acc[C];
#pragma unroll
            for (int co = 0; co < C; ++co) acc[co] = b2[co];
#pragma unroll 1
            for (int ci = 0; ci < C; ++ci) {
                const float* ap = pa + ci * AN + ly * AW + lx;
                const float* wp = w2 + ci * 9 * C;
                float in[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) in[t] = ap[(t / 3) * AW + (t % 3)];
#pragma unroll
                for (int t = 0; t < 9; ++t)
#pragma unroll
                    for (int co = 0; co < C; ++co) acc[co] = fmaf(wp[t * C + co], in[t], acc[co]);
            }
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
            for (int co = 0; co < C; ++co) pb[co * BN + i] = inside ? elu1(acc[co]) : 0.0f;
        }
        __syncthreads();

        // ---- out_conv: dW3 = g (*) B, db3 = sum g ------------------------------------------------------------------------
        correlate<TW>(s3, pg, NO == 1 ? 0 : AN, AW, 3 * AW + 3, pb, BN, BW, 1 * BW + 1, acc3);
        __syncthreads();

        // ---- dB = elu'(B) * sum_{o,t} w3[c][t][o] g[o][q - t] on tile + 2, over B ----------------------------------------
        for (int i = tid; i < BN; i += NT) {
            const int ly = i / BW, lx = i - ly * BW;
            const int gy = y0 - 2 + ly, gx = x0 - 2 + lx;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
            float gv[NO][9];
#pragma unroll
            for (int o = 0; o < NO; ++o)
#pragma unroll
                for (int t = 0; t < 9; ++t) gv[o][t] = pg[o * AN + (ly + 2 - t / 3) * AW + (lx + 2 - t % 3)];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float s = 0.0f;
#pragma unroll
                for (int o = 0; o < NO; ++o)
#pragma unroll
                    for (int t = 0; t < 9; ++t) s = fmaf(w3[(c * 9 + t) * NO + o], gv[o][t], s);
                const float act = pb[c * BN + i];
                pb[c * BN + i] = inside ? (act > 0.0f ? s : s * (act + 1.0f)) : 0.0f;
            }
        }
        __syncthreads();

        // ---- hidden_conv1: dW2 = dB (*) A, db2 = sum dB -------------------------------------------------------------------
        correlate<TW>(s2, pb, BN, BW, 2 * BW + 2, pa, AN, AW, 2 * AW + 2, acc2);
        __syncthreads();

        // ---- dA = elu'(A) * sum_{co,t} w2[c][t][co] dB[co][r - t] on tile + 1, over A ------------------------------------
        for (int i = tid; i < DN; i += NT) {
            const int dy = i / DW, ly = 2 + dy, lx = 2 + (i - dy * DW);
            const int gy = y0 - 3 + ly, gx = x0 - 3 + lx;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
            float acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 0.0f;
#pragma unroll 1
            for (int co = 0; co < C; ++co) {
                const float* bp = pb + co * BN + ly * BW + lx;
                float d[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) d[t] = bp[-(t / 3) * BW - (t % 3)];
#pragma unroll
                for (int t = 0; t < 9; ++t)
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] = fmaf(w2[(c * 9 + t) * C + co], d[t], acc[c]);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float act = pa[c * AN + ly * AW + lx];
                pa[c * AN + ly * AW + lx] = inside ? (act > 0.0f ? acc[c] : acc[c] * (act + 1.0f)) : 0.0f;
            }
        }
        __syncthreads();

        // ---- in_conv: dW1 = dA (*) E0, db1 = sum dA; table: dE0 = w1 transposed * dA on the tile, scattered by code --------
        correlate<TW>(s1, pa, AN, AW, 3 * AW + 3, pe, EN, EW, 3 * EW + 3, acc1);
        for (int i = tid; i < TH * TW; i += NT) {
            const int sy = i / TW, sx = i - sy * TW;
            const int gy = y0 + sy, gx = x0 + sx;
            if (gy >= H || gx >= W) continue;
            const int64_t code = load_code(codes, idx_dtype, (int64_t)b * hw + (int64_t)gy * W + gx);
            if (code < 0 || code >= K) continue;                  // a zero vector: no gradient
            float de[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) de[e] = 0.0f;
#pragma unroll 1
            for (int co = 0; co < C; ++co) {
                const float* ap = pa + co * AN + (sy + 4) * AW + (sx + 4);
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const float d = ap[-(t / 3) * AW - (t % 3)];
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (e < E) de[e] = fmaf(w1[(e * 9 + t) * C + co], d, de[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e < E && de[e] != 0.0f) {
                    const unsigned long long q = (unsigned long long)__double2ll_rn((double)de[e] * FIX_ONE);
                    atomicAdd((emb_lds ? pfix : emb_fix) + code * E + e, q);
                }
            }
        }
    }

    // ---- one row per workgroup -----------------------------------------------------------------------------------------------
    // row: in_conv.weight [C][E][9], in_conv.bias [C], hidden_conv1.weight [C][C][9], .bias [C], out_conv.weight [NO][C][9], .bias [NO]
    double* const row = rows + (int64_t)blockIdx.x * row_len;
    double* const red = (double*)pa;
    double* r1 = row, *rb1 = r1 + C * E * 9, *r2 = rb1 + C, *rb2 = r2 + C * C * 9, *r3 = rb2 + C, *rb3 = r3 + NO * C * 9;
    reduce_slices(red, acc1, E, C, r1, rb1);
    reduce_slices(red, acc2, C, C, r2, rb2);
    reduce_slices(red, acc3, C, NO, r3, rb3);
    if (emb_lds) {                                                // (reduce_slices' barriers order the last tile's atomics)
        for (int i = tid; i < K * E; i += NT)
            if (pfix[i]) atomicAdd(emb_fix + i, pfix[i]);
    }
}

// loss and the scale of the gradients from the batch's stats rows, in row order: out[0] = loss, out[1] = scale
__global__ void train_scale(const double* __restrict__ stats, int batch, int mean, double* __restrict__ loss, double* __restrict__ scale) {
    double n = 0.0, l = 0.0;
    for (int b = 0; b < batch; ++b) { n += stats[b * SK + VQAE_CLS_N_VALID]; l += stats[b * SK + VQAE_CLS_LOSS_SUM]; }
    *loss = mean ? l / n : l;                                     // (mean over no valid code: nan, as the reference's)
    *scale = mean ? (n > 0.0 ? 1.0 / n : 0.0) : 1.0;
}

// the same for cross-entropy rows: loss = (1 - eps) * sum nll + (eps / NO) * sum smooth, 'mean' divides by sum w[y]
__global__ void train_scale_ce(const double* __restrict__ stats, int batch, int mean, double keep, double smooth,
                               double* __restrict__ loss, double* __restrict__ scale) {
    double n = 0.0, a = 0.0, s = 0.0;
    for (int b = 0; b < batch; ++b) {
        n += stats[b * CEK + VQAE_CE_WEIGHT_SUM]; a += stats[b * CEK + VQAE_CE_NLL_SUM]; s += stats[b * CEK + VQAE_CE_SMOOTH_SUM];
    }
    const double l = keep * a + smooth * s;
    *loss = mean ? l / n : l;                                     // (mean over a zero weight sum: nan, as torch's)
    *scale = mean ? (n > 0.0 ? 1.0 / n : 0.0) : 1.0;
}

__global__ __launch_bounds__(NT)
void train_final(const unsigned long long* __restrict__ emb_fix, int n_emb, const double* __restrict__ rows, int n_rows, int row_len,
                 const double* __restrict__ scale, double* __restrict__ grads) {
    const int j = blockIdx.x * NT + threadIdx.x;
    if (j >= n_emb + row_len) return;
    double r;
    if (j < n_emb) {
        r = (double)(long long)emb_fix[j] * (1.0 / FIX_ONE);
    } else {
        const double* q = rows + (j - n_emb);
        r = q[0];
        for (int i = 1; i < n_rows; ++i) r += q[(int64_t)i * row_len];
    }
    grads[j] = r * *scale;
}

struct Plan {
    int64_t total; int n_wg, row_len, n_emb;
    size_t o_glogit, o_fix, o_rows, o_scale, bytes;
};

Plan make_plan(const vqae_classifier* c, int batch, int h, int w, bool ce = false) {
    Plan p;
    p.total = (int64_t)batch * tile_count(c, h, w, nullptr);
    p.n_wg = (int)(p.total < MAX_WG ? p.total : MAX_WG);
    p.n_emb = c->K * c->E;
    p.row_len = c->C * c->E * 9 + c->C + c->C * c->C * 9 + c->C + c->NO * c->C * 9 + c->NO;
    // the forward's stats partials come first
    size_t n = ce ? vqae_classifier_ce_workspace_bytes(c, batch, h, w) : vqae_classifier_workspace_bytes(c, batch, h, w);
    auto take = [&n](int64_t bytes) { const size_t o = n; n += (size_t)vqae::round_up(bytes, 256); return o; };
    p.o_glogit = take((int64_t)batch * c->NO * h * w * 4);
    p.o_fix = take((int64_t)p.n_emb * 8);
    p.o_rows = take((int64_t)p.n_wg * p.row_len * 8);
    p.o_scale = take(8);
    p.bytes = n;
    return p;
}

// Where the fixed-point table gradient is accumulated: in LDS while the table has at most EMB_LDS_MAX entries AND the planes
// beside it stay within the 160 KiB a workgroup may request, in HBM otherwise.  The planes depend on (E, C, NO) and on the
// tile width, itself a function of (E, C): the choice, and with it the partition and the bits, is a function of
// (K, E, C, NO) alone.  (With the geometries in use -- TW = 62 only for C = 8, E <= 6 -- the largest case, E = 6, NO = 4,
// takes 140 256 B of planes + 16 384 B of table = 156 640 B: the LDS path is always taken for K * E <= 2048.)
template <int C, int NO, int TW>
int launch_backward(const vqae_classifier* c, const Plan& p, const void* codes, int idx_dtype, int h, int w, int tiles_x, int ntiles,
                    char* ws, hipStream_t st) {
    constexpr int EN = (TH + 8) * (TW + 8), AN = (TH + 6) * (TW + 6), BN = (TH + 4) * (TW + 4);
    const int planes = 4 * (C * AN + C * BN + NO * AN + c->E * EN);
    const int emb_lds = p.n_emb <= EMB_LDS_MAX && p.n_emb * 8 + planes <= 160 * 1024;
    const int lds = (emb_lds ? p.n_emb * 8 : 0) + planes;
    VQAE_REQUIRE(lds <= 160 * 1024, VQAE_ERR_UNSUPPORTED, "classifier backward: %d bytes of LDS", lds);
    auto kern = classifier_backward_kernel<C, NO, TW>;
    if (int rc = vqae::set_max_dynamic_lds((const void*)kern, 160 * 1024)) return rc;
    kern<<<p.n_wg, NT, lds, st>>>(codes, idx_dtype, h, w, tiles_x, ntiles, p.total, c->dev + c->o_table, c->K, c->E,
                                  c->dev + c->o_w1, c->dev + c->o_b1, c->dev + c->o_w2, c->dev + c->o_b2, c->dev + c->o_w3,
                                  (const float*)(ws + p.o_glogit), emb_lds, (unsigned long long*)(ws + p.o_fix),
                                  (double*)(ws + p.o_rows), p.row_len);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

}  // namespace

extern "C" size_t vqae_classifier_grad_floats(const vqae_classifier* c) {
    if (!c) return 0;
    return (size_t)c->K * c->E + (size_t)c->C * c->E * 9 + c->C + (size_t)c->C * c->C * 9 + c->C + (size_t)c->NO * c->C * 9 + c->NO;
}

extern "C" size_t vqae_classifier_train_workspace_bytes(const vqae_classifier* c, int batch, int h, int w) {
    if (!c || c->NO != 1 || batch <= 0 || h < 1 || w < 1) return 0;
    return make_plan(c, batch, h, w).bytes;
}

extern "C" int vqae_classifier_loss_grad(vqae_classifier* c, const void* codes_dev, int idx_dtype, int batch, int h, int w,
                                         const uint8_t* mask_dev, const float* target_dev, float pos_weight, int reduction,
                                         double* grads_dev, double* stats_dev, double* loss_dev, void* workspace_dev, void* stream) {
    VQAE_REQUIRE(c && codes_dev && mask_dev && grads_dev && stats_dev && loss_dev && workspace_dev, VQAE_ERR_INVALID,
                 "classifier_loss_grad: null pointer");
    VQAE_REQUIRE(idx_dtype_ok(idx_dtype), VQAE_ERR_INVALID, "classifier_loss_grad: bad index dtype %d", idx_dtype);
    VQAE_REQUIRE(batch >= 0 && h >= 1 && w >= 1, VQAE_ERR_INVALID, "classifier_loss_grad: bad shape batch=%d h=%d w=%d", batch, h, w);
    VQAE_REQUIRE(std::isfinite(pos_weight) && pos_weight >= 0.f, VQAE_ERR_INVALID,
                 "classifier_loss_grad: pos_weight must be finite and >= 0");
    VQAE_REQUIRE(reduction == 0 || reduction == 1, VQAE_ERR_INVALID, "classifier_loss_grad: reduction %d is not 0 (sum) or 1 (mean)",
                 reduction);
    VQAE_REQUIRE(c->NO == 1, VQAE_ERR_UNSUPPORTED, "classifier_loss_grad: the loss is defined for n_out == 1, this classifier has %d",
                 c->NO);
    VQAE_REQUIRE(batch <= 65535, VQAE_ERR_UNSUPPORTED, "classifier_loss_grad: batch %d > 65535", batch);
    int tiles_x = 0;
    const int64_t ntiles = tile_count(c, h, w, &tiles_x);
    VQAE_REQUIRE(ntiles < (1ll << 31), VQAE_ERR_UNSUPPORTED, "classifier_loss_grad: a grid of %d x %d codes", h, w);
    const hipStream_t st = (hipStream_t)stream;
    const size_t ng = vqae_classifier_grad_floats(c);
    if (batch == 0) {
        VQAE_HIP_CHECK(hipMemsetAsync(grads_dev, 0, ng * sizeof(double), st));
        VQAE_HIP_CHECK(hipMemsetAsync(loss_dev, 0, sizeof(double), st));
        return VQAE_OK;
    }
    const Plan p = make_plan(c, batch, h, w);
    char* ws = (char*)workspace_dev;
    if (int rc = forward_launch(c, codes_dev, idx_dtype, batch, h, w, nullptr, nullptr, mask_dev, target_dev, pos_weight,
                                (float*)(ws + p.o_glogit), stats_dev, workspace_dev, st))
        return rc;
    VQAE_HIP_CHECK(hipMemsetAsync(ws + p.o_fix, 0, (size_t)p.n_emb * 8, st));
    int rc;
    if (c->tw == 62) rc = launch_backward<8, 1, 62>(c, p, codes_dev, idx_dtype, h, w, tiles_x, (int)ntiles, ws, st);
    else if (c->C == 8) rc = launch_backward<8, 1, 30>(c, p, codes_dev, idx_dtype, h, w, tiles_x, (int)ntiles, ws, st);
    else rc = launch_backward<16, 1, 30>(c, p, codes_dev, idx_dtype, h, w, tiles_x, (int)ntiles, ws, st);
    if (rc) return rc;
    double* scale = (double*)(ws + p.o_scale);
    train_scale<<<1, 1, 0, st>>>(stats_dev, batch, reduction, loss_dev, scale);
    VQAE_LAUNCH_CHECK();
    const int n_out = p.n_emb + p.row_len;
    train_final<<<(unsigned)vqae::ceil_div(n_out, NT), NT, 0, st>>>((const unsigned long long*)(ws + p.o_fix), p.n_emb,
                                                                   (const double*)(ws + p.o_rows), p.n_wg, p.row_len, scale, grads_dev);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

// ---- Multi-class: nn.CrossEntropyLoss as loss_f of CNNClassifier.step -------------------------------------------------------
namespace {

template <int C, int TW>
int launch_backward_no(const vqae_classifier* c, const Plan& p, const void* codes, int idx_dtype, int h, int w, int tiles_x, int ntiles,
                       char* ws, hipStream_t st) {
    switch (c->NO) {
        case 2: return launch_backward<C, 2, TW>(c, p, codes, idx_dtype, h, w, tiles_x, ntiles, ws, st);
        case 3: return launch_backward<C, 3, TW>(c, p, codes, idx_dtype, h, w, tiles_x, ntiles, ws, st);
        default: return launch_backward<C, 4, TW>(c, p, codes, idx_dtype, h, w, tiles_x, ntiles, ws, st);
    }
}

}  // namespace

extern "C" size_t vqae_classifier_ce_train_workspace_bytes(const vqae_classifier* c, int batch, int h, int w) {
    if (!c || c->NO == 1 || batch <= 0 || h < 1 || w < 1) return 0;
    return make_plan(c, batch, h, w, true).bytes;
}

extern "C" int vqae_classifier_loss_grad_ce(vqae_classifier* c, const void* codes_dev, int idx_dtype, int batch, int h, int w,
                                            const uint8_t* labels_dev, const float* weight, float label_smoothing, int reduction,
                                            double* grads_dev, double* stats_dev, double* loss_dev, void* workspace_dev, void* stream) {
    VQAE_REQUIRE(c && codes_dev && labels_dev && grads_dev && stats_dev && loss_dev && workspace_dev, VQAE_ERR_INVALID,
                 "classifier_loss_grad_ce: null pointer");
    VQAE_REQUIRE(idx_dtype_ok(idx_dtype), VQAE_ERR_INVALID, "classifier_loss_grad_ce: bad index dtype %d", idx_dtype);
    VQAE_REQUIRE(batch >= 0 && h >= 1 && w >= 1, VQAE_ERR_INVALID, "classifier_loss_grad_ce: bad shape batch=%d h=%d w=%d", batch, h, w);
    CeArgs ce;
    if (int rc = ce_args("classifier_loss_grad_ce", c, weight, label_smoothing, &ce)) return rc;
    VQAE_REQUIRE(reduction == 0 || reduction == 1, VQAE_ERR_INVALID, "classifier_loss_grad_ce: reduction %d is not 0 (sum) or 1 (mean)",
                 reduction);
    VQAE_REQUIRE(c->NO > 1, VQAE_ERR_UNSUPPORTED,
                 "classifier_loss_grad_ce: cross-entropy needs n_out >= 2; vqae_classifier_loss_grad trains n_out == 1");
    VQAE_REQUIRE(batch <= 65535, VQAE_ERR_UNSUPPORTED, "classifier_loss_grad_ce: batch %d > 65535", batch);
    int tiles_x = 0;
    const int64_t ntiles = tile_count(c, h, w, &tiles_x);
    VQAE_REQUIRE(ntiles < (1ll << 31), VQAE_ERR_UNSUPPORTED, "classifier_loss_grad_ce: a grid of %d x %d codes", h, w);
    const hipStream_t st = (hipStream_t)stream;
    const size_t ng = vqae_classifier_grad_floats(c);
    if (batch == 0) {
        VQAE_HIP_CHECK(hipMemsetAsync(grads_dev, 0, ng * sizeof(double), st));
        VQAE_HIP_CHECK(hipMemsetAsync(loss_dev, 0, sizeof(double), st));
        return VQAE_OK;
    }
    const Plan p = make_plan(c, batch, h, w, true);
    char* ws = (char*)workspace_dev;
    if (int rc = forward_launch(c, codes_dev, idx_dtype, batch, h, w, nullptr, nullptr, labels_dev, nullptr, 1.0f,
                                (float*)(ws + p.o_glogit), stats_dev, workspace_dev, st, &ce))
        return rc;
    VQAE_HIP_CHECK(hipMemsetAsync(ws + p.o_fix, 0, (size_t)p.n_emb * 8, st));
    int rc;
    if (c->tw == 62) rc = launch_backward_no<8, 62>(c, p, codes_dev, idx_dtype, h, w, tiles_x, (int)ntiles, ws, st);
    else if (c->C == 8) rc = launch_backward_no<8, 30>(c, p, codes_dev, idx_dtype, h, w, tiles_x, (int)ntiles, ws, st);
    else rc = launch_backward_no<16, 30>(c, p, codes_dev, idx_dtype, h, w, tiles_x, (int)ntiles, ws, st);
    if (rc) return rc;
    double* scale = (double*)(ws + p.o_scale);
    train_scale_ce<<<1, 1, 0, st>>>(stats_dev, batch, reduction, (double)ce.keep, (double)ce.smooth, loss_dev, scale);
    VQAE_LAUNCH_CHECK();
    const int n_out = p.n_emb + p.row_len;
    train_final<<<(unsigned)vqae::ceil_div(n_out, NT), NT, 0, st>>>((const unsigned long long*)(ws + p.o_fix), p.n_emb,
                                                                   (const double*)(ws + p.o_rows), p.n_wg, p.row_len, scale, grads_dev);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}
