// Trainable 2x2, stride-2 convolution of a Fixup 'down' block (conv_block.py:196-216; down2d.yaml: kernel 2, stride 2, padding 0,
// no bias), fp32, NHWC, with the element-wise op in front of it folded in.  The four taps do not overlap, so the conv is a plain
// GEMM over gathered rows:
//     x [B][H][W][Ci], H and W even;  OH = H / 2, OW = W / 2, M = B OH OW;  y [M][Co] = u_gathered [M][4 Ci] . w^T
//     row m = (b, oh, ow), column k = (kh, kw, ci):  u_gathered[m][k] = u[b][2 oh + kh][2 ow + kw][ci]
//     pre = 0: u = x        pre = 1: u = x + *b        pre = 2: u = ELU(x + *a) + *b        (a, b read from DEVICE memory)
// u is never written to memory.  All products run on v_mfma_f32_32x32x2_f32.  The scheme is csrc/conv1x1_train.hip's, with
// its kernels duplicated here (that file is untouched): what changes is the addressing.  For a fixed kh the two kw pixels are
// neighbours in memory, so a row of the operand is two contiguous segments of 2 Ci floats:
//     address(m, k) = xbase(m) + (k / 2Ci) W Ci + k % 2Ci,     xbase(m) = ((m / OW) 4 OW + 2 (m % OW)) Ci      (H = 2 OH, W = 2 OW)
// and a weight stored [Co][kh][kw][Ci] (a channels_last [Co, Ci, 2, 2] tensor) is k-contiguous against it.
//
// Weights: w_layout 1 = [Co][2][2][Ci] is used as it lies; w_layout 0 = [Co][Ci][2][2] (contiguous) is permuted into the
// workspace by cd_permute_w first (every call: the weight changes every step).  g_w is written in the layout the weight has.
//
//   cd_gemm<NT, false>   forward: c1_gemm<NT, false> with K = 4 Ci.  A workgroup of 4 waves owns 128 rows x all Co columns, K
//                        walked in chunks of 32, the x chunk staged to LDS with the pre-op applied once per element (no expm1f
//                        in the MFMA loop), the next chunk fetched into registers, branch-free, while the current one
//                        multiplies.  The row bases of a tile are computed once per tile (one 64-bit division per thread).
//   cd_gemm<NT, true>    data gradient  g_u [M][4 Ci] = g [M][Co] . w [Co][4 Ci]  in pieces of at most 256 columns (blockIdx.y;
//                        a piece is 32 NT columns, NT from min(4 Ci, 256)); the epilogue scatters: column n = (kh, kw, ci) of
//                        row m is input element xbase(m) + (n / 2Ci) W Ci + n % 2Ci, g_x = g_u * ELU'(x + *a) with x read
//                        there.  (m, n) -> element is one to one and onto (H, W even): every element of g_x is written
//                        exactly once, by a plain store.  fp64 sums of g_x and g_u per thread in a fixed order.
//   cd_wgrad             weight gradient  g_w [co][n] = sum_m g[m][co] u_gathered[m][n]: c1_wgrad on a Co x 4 Ci output.  Grid
//                        (P, tiles of up to 64 co x 64 n); rows in blocks of 64, workgroup p takes blocks p, p + P, ...; fp32
//                        runs of CD_RUN = 512 rows go into the workgroup's OWN fp64 slot (plain store on the first run);
//                        cd_wgrad_final adds the P slots in index order in fp64, rounds once and writes the weight's layout.
//
// Determinism: every grid is a function of (B, H, W, Ci, Co) alone, there are no floating-point atomics, every sum has one
// fixed order.  Scalar sums: thread (fp64, index order) -> wave shuffle -> 4 waves in order -> one fp64 row per workgroup
// and piece -> cd_sum_final (one workgroup, fixed order, one rounding).
//
// Workspace (vqae_conv_down_train_workspace_bytes): the permuted weight (4 Ci Co floats, at most 1 MiB) + P slots of 4 Ci Co
// doubles with P <= 256 and P 4 Ci Co <= 2^21 (at most 16 MiB whatever M is) + 4096 rows of two doubles for the scalar sums
// + 256 bytes of alignment slack: below 17.2 MiB in all.
#include <algorithm>

#include "kernels.h"
#include "mfma.h"

namespace {

using namespace vqae;

constexpr int CD_THREADS = 256;
constexpr int CD_BM = 128;               // rows of a forward / data-gradient workgroup tile
constexpr int CD_KC = 32;                // k chunk staged per step
constexpr int CD_LD = CD_KC + 4;         // LDS row stride in floats: 16-byte aligned rows, 128-bit reads of 16 lanes hit all banks
constexpr int CD_MAX_WG = 1024;          // workgroups of cd_gemm per piece
constexpr int CD_MAX_PIECES = 4;         // 4 * 256 / 256
constexpr int CD_RUN = 512;              // longest fp32 accumulation run of g_w, in rows
constexpr int CD_WM = 64;                // rows of a cd_wgrad block
constexpr int CD_PG = 8;                 // row pairs a cd_wgrad wave loads ahead of its MFMAs
constexpr int CD_SLOTS = 256;            // P <= CD_SLOTS and P 4 Ci Co <= CD_SLOT_ELEMS (P >= 1): at most 16 MiB of fp64 partials
constexpr int64_t CD_SLOT_ELEMS = 1 << 21;
constexpr int CD_MAXC = 256;

__device__ __forceinline__ float elu_train(float v) { return v > 0.f ? v : expm1f(v); }
__device__ __forceinline__ float elu_grad(float v) { return v > 0.f ? 1.f : expf(v); }

__device__ __forceinline__ f32x4 pre_op(f32x4 v, int pre, float a, float b) {
    if (pre == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = elu_train(v[e] + a) + b;
    } else if (pre == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] + b;
    }
    return v;
}

// Row m = q OW + ow (q = b OH + oh: input row pair 2 q, 2 q + 1 of the [B H][W][Ci] array) -> offset of pixel (2 q, 2 ow).
struct RowPos { int64_t q; unsigned ow; };
__device__ __forceinline__ RowPos row_pos(int64_t m, int OW) {
    RowPos p;
    p.q = m / OW;
    p.ow = (unsigned)(m - p.q * OW);
    return p;
}
// offset of the row d >= 0 (small) after p
__device__ __forceinline__ int64_t row_base(RowPos p, unsigned d, int OW, int Ci) {
    const unsigned t = p.ow + d, dq = t / (unsigned)OW, ow = t - dq * (unsigned)OW;
    return ((p.q + dq) * 4 * OW + 2 * (int64_t)ow) * Ci;
}
// offset of column n = (kh, kw, ci) of [0, 4 Ci) inside a row's 2 x 2 window;  row_stride = W Ci
__device__ __forceinline__ int64_t col_off(int n, int Ci, int64_t row_stride) {
    const int kh = n >= 2 * Ci ? 1 : 0;
    return kh * row_stride + (n - kh * 2 * Ci);
}

// w [Co][Ci][2][2] -> wp [Co][2][2][Ci]
__global__ __launch_bounds__(CD_THREADS)
void cd_permute_w(const float* __restrict__ w, int Ci, int n, float* __restrict__ wp) {
    const int i = blockIdx.x * CD_THREADS + threadIdx.x;
    if (i >= n) return;
    const int co = i / (4 * Ci), r = i - co * 4 * Ci, tap = r / Ci, ci = r - tap * Ci;
    wp[i] = w[(int64_t)co * 4 * Ci + ci * 4 + tap];
}

// BWD false:  out [M][N] = pre(x gathered [M][K]) . w [N][K]^T                        (forward: K = 4 Ci, N = Co, one piece)
// BWD true:   g_x scattered = (A [M][K] . w [K][piece of NW]) * ELU'(xe + a), sums     (data gradient: K = Co, NW = 4 Ci)
// N is the number of columns in all (the row stride of w for BWD), blockIdx.y * 32 NT the first column of this piece.
template <int NT, bool BWD>
__global__ __launch_bounds__(CD_THREADS)
void cd_gemm(const float* __restrict__ A, const float* __restrict__ xe, const float* __restrict__ pa,
             const float* __restrict__ pb, int pre, const float* __restrict__ w, int64_t M, int OW, int Ci, int K, int N,
             float* __restrict__ out, double* __restrict__ partials) {
    __shared__ __attribute__((aligned(16))) float Al[CD_BM * CD_LD];
    __shared__ __attribute__((aligned(16))) float Wl[NT * 32 * CD_LD];
    __shared__ double red[2][CD_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    const float a = pre == 2 ? *pa : 0.f, b = (!BWD && pre >= 1) ? *pb : 0.f;
    const int64_t n_tiles = (M + CD_BM - 1) / CD_BM;
    const int64_t row_stride = (int64_t)2 * OW * Ci;                      // W Ci
    const int n0 = BWD ? (int)blockIdx.y * NT * 32 : 0;
    double s0 = 0.0, s1 = 0.0;
    // One chunk = 128 rows x 32 k of A (4 16-byte groups per thread, all with the same k) and NT * 32 columns x 32 k of w (NT
    // groups per thread), zero where a row, a column or k is out of range (Ci % 8 == 0, Co % 8 == 0: a group is in or out as a
    // whole, and lies inside one tap).  fetch() brings the NEXT chunk into registers while the MFMA loop runs on the current
    // one: branch-free loads, an out-of-range group reads the nearest valid address instead; commit() zeroes those groups,
    // applies the pre-op and writes the chunk to LDS.  rows() sets the offsets of this thread's four rows of a tile.
    constexpr int AG = CD_BM * (CD_KC / 4) / CD_THREADS;
    f32x4 ra[AG], rw[NT];
    int64_t rb[AG];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    auto rows = [&](int64_t m0) __attribute__((always_inline)) {
        const int64_t mf = std::min(m0 + (tid >> 3), M - 1);
        if (!BWD) {
            const RowPos p = row_pos(mf, OW);
#pragma unroll
            for (int j = 0; j < AG; ++j) {
                const int64_t m = std::min(m0 + (tid >> 3) + 32 * j, M - 1);
                rb[j] = row_base(p, (unsigned)(m - mf), OW, Ci);
            }
        } else {
#pragma unroll
            for (int j = 0; j < AG; ++j) rb[j] = std::min(m0 + (tid >> 3) + 32 * j, M - 1) * K;
        }
    };
    auto fetch = [&](int k0) __attribute__((always_inline)) {
        const int k = std::min(k0 + 4 * (tid & 7), K - 4);
        const int64_t ko = BWD ? (int64_t)k : col_off(k, Ci, row_stride);
#pragma unroll
        for (int j = 0; j < AG; ++j) ra[j] = *reinterpret_cast<const f32x4*>(A + rb[j] + ko);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int i = tid + j * CD_THREADS;
            if (!BWD) {                  // w [n][k]: k-contiguous
                const int n = i >> 3;
                rw[j] = *reinterpret_cast<const f32x4*>(w + (int64_t)std::min(n, N - 1) * K + k);
            } else {                     // w [k][n]: n-contiguous, row stride N
                const int kk = i / (NT * 8), n = n0 + 4 * (i % (NT * 8));
                rw[j] = *reinterpret_cast<const f32x4*>(w + (int64_t)std::min(k0 + kk, K - 1) * N + std::min(n, N - 4));
            }
        }
    };
    auto commit = [&](int64_t m0, int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < AG; ++j) {
            const int i = tid + j * CD_THREADS, k = k0 + 4 * (i & 7);
            const int64_t m = m0 + (i >> 3);
            f32x4 v = (m < M && k < K) ? ra[j] : zero4;
            if (!BWD && m < M && k < K) v = pre_op(v, pre, a, b);          // zero-filled elements stay zero
            *reinterpret_cast<f32x4*>(Al + (i >> 3) * CD_LD + 4 * (i & 7)) = v;
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int i = tid + j * CD_THREADS;
            if (!BWD) {
                *reinterpret_cast<f32x4*>(Wl + (i >> 3) * CD_LD + 4 * (i & 7)) = ((i >> 3) < N && k0 + 4 * (i & 7) < K) ? rw[j] : zero4;
            } else {                     // transposed into the k-contiguous LDS rows
                const int kk = i / (NT * 8), n = 4 * (i % (NT * 8));
#pragma unroll
                for (int e = 0; e < 4; ++e) Wl[(n + e) * CD_LD + kk] = (k0 + kk < K && n0 + n < N) ? rw[j][e] : 0.f;
            }
        }
    };
    int64_t co[NT];                                      // data gradient: this lane's columns inside a row's window
    if (BWD) {
#pragma unroll
        for (int t = 0; t < NT; ++t) co[t] = col_off(std::min(n0 + t * 32 + li, N - 1), Ci, row_stride);
    }
    if ((int64_t)blockIdx.x < n_tiles) {
        rows((int64_t)blockIdx.x * CD_BM);
        fetch(0);
    }
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t m0 = tile * CD_BM;
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        for (int k0 = 0; k0 < K; k0 += CD_KC) {
            commit(m0, k0);
            __syncthreads();
            if (k0 + CD_KC < K) {
                fetch(k0 + CD_KC);
            } else if (tile + gridDim.x < n_tiles) {
                rows((tile + gridDim.x) * CD_BM);
                fetch(0);
            }
            const int slices = std::min(CD_KC, K - k0) / 8;
            const float* ap = Al + (wave * 32 + li) * CD_LD + 4 * hh;
            const float* bp = Wl + li * CD_LD + 4 * hh;
            for (int u = 0; u < slices; ++u) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(ap + 8 * u);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const f32x4 bv = *reinterpret_cast<const f32x4*>(bp + t * 32 * CD_LD + 8 * u);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r], bv[r], acc[t], 0, 0, 0);
                }
            }
            __syncthreads();
        }
        // D [i = row][j = column]: lane (li, hh) holds column li of its tile, rows 8 (r / 4) + 4 hh + r % 4
        if (!BWD) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int col = t * 32 + li;
                if (col < N) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t m = m0 + wave * 32 + 8 * (r >> 2) + 4 * hh + (r & 3);
                        if (m < M) out[m * N + col] = acc[t][r];
                    }
                }
            }
        } else {
            const int64_t mf = m0 + wave * 32 + 4 * hh;                    // this lane's first row: rows mf + 8 (r / 4) + r % 4
            if (mf < M) {
                const RowPos p = row_pos(mf, OW);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned d = 8 * (r >> 2) + (r & 3);
                    if (mf + d < M) {
                        const int64_t base = row_base(p, d, OW, Ci);
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            if (n0 + t * 32 + li < N) {
                                float v = acc[t][r];
                                s1 += (double)v;
                                if (pre == 2) v = v * elu_grad(xe[base + co[t]] + a);
                                s0 += (double)v;
                                if (out) out[base + co[t]] = v;
                            }
                        }
                    }
                }
            }
        }
    }
    if (BWD) {
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        if (lane == 0) { red[0][wave] = s0; red[1][wave] = s1; }
        __syncthreads();
        if (tid == 0) {
            const int64_t row = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
            partials[row * 2 + 0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
            partials[row * 2 + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        }
    }
}

// One workgroup: thread t adds rows t, t + 256, ... in that order, then the wave / workgroup order of cd_gemm.
__global__ __launch_bounds__(CD_THREADS)
void cd_sum_final(const double* __restrict__ partials, int n_rows, float* __restrict__ o0, float* __restrict__ o1) {
    __shared__ double red[2][CD_THREADS / 64];
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < n_rows; i += CD_THREADS) {
        s0 += partials[(int64_t)i * 2 + 0];
        s1 += partials[(int64_t)i * 2 + 1];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if (lane == 0) { red[0][wave] = s0; red[1][wave] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (o0) *o0 = (float)(((red[0][0] + red[0][1]) + red[0][2]) + red[0][3]);
        if (o1) *o1 = (float)(((red[1][0] + red[1][1]) + red[1][2]) + red[1][3]);
    }
}

// c1_wgrad with a gathered activation operand: the output is Co x N (N = 4 Ci, column n = (kh, kw, ci)), a tile 32 NCO co x
// 32 NCN n.  Rows in blocks of CD_WM = 64; workgroup p takes blocks p, p + P, ...; wave w the row pairs w, w + 4, ..., w + 28 of
// a block (lane (li, hh) row 2 pair + hh), operands straight from global memory (lane = channel: 32 consecutive columns are
// one 128-byte segment, or two where they cross a tap pair), one block of loads ahead of its MFMAs; no LDS, no barrier in the
// loop.  After every CD_RUN / 64 = 8 blocks and at the end the four accumulators are added in wave order through LDS and
// wave 3 adds the run into the workgroup's fp64 slot [co][n].  PRE is a template argument so that the loop is straight-line.
template <int NCO, int NCN, int PRE>
__global__ __launch_bounds__(CD_THREADS)
void cd_wgrad(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ pa,
              const float* __restrict__ pb, int64_t M, int OW, int Ci, int Co, double* __restrict__ slots) {
    static_assert(CD_WM == 8 * CD_PG && CD_RUN % CD_WM == 0 && (CD_RUN / CD_WM) % 2 == 0, "a block is one load group per wave");
    __shared__ float red[NCO * NCN * 16 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    const int N = 4 * Ci;
    const int tiles_n = (N + 32 * NCN - 1) / (32 * NCN);
    const int co0 = (blockIdx.y / tiles_n) * 32 * NCO, n0 = (blockIdx.y % tiles_n) * 32 * NCN;
    const float a = PRE == 2 ? *pa : 0.f, b = PRE >= 1 ? *pb : 0.f;
    const int64_t n_blocks = (M + CD_WM - 1) / CD_WM;
    const int64_t row_stride = (int64_t)2 * OW * Ci;
    const int P = gridDim.x;
    int cg[NCO];                                          // this lane's channels / window offsets, clamped for the loads
    int64_t cx[NCN];
#pragma unroll
    for (int s = 0; s < NCO; ++s) cg[s] = std::min(co0 + 32 * s + li, Co - 1);
#pragma unroll
    for (int t = 0; t < NCN; ++t) cx[t] = col_off(std::min(n0 + 32 * t + li, N - 1), Ci, row_stride);
    const int nb = (int)((n_blocks - blockIdx.x + P - 1) / P);                        // this workgroup's blocks: >= 1
    double* slot = slots + (int64_t)blockIdx.x * Co * N;
    f32x16 acc[NCO][NCN];
    auto clear = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NCO; ++s)
#pragma unroll
            for (int t = 0; t < NCN; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[s][t][r] = 0.f;
    };
    float bg[2][CD_PG][NCO], bx[2][CD_PG][NCN];
    auto base_of = [&](int blk) __attribute__((always_inline)) { return ((int64_t)blockIdx.x + (int64_t)blk * P) * CD_WM; };
    auto row_in = [&](int q) __attribute__((always_inline)) { return 2 * (wave + 4 * q) + hh; };
    // branch-free: a block past the end reads the last block, a row past the end row M - 1, a missing column the last one;
    // compute() zeroes them.
    auto fetch = [&](int blk, int buf) __attribute__((always_inline)) {
        const int64_t base = std::min(base_of(blk), (n_blocks - 1) * CD_WM);
        const int last = (int)std::min<int64_t>(CD_WM - 1, M - 1 - base);
        const float* gb = g + base * Co;
        const RowPos p = row_pos(base, OW);
#pragma unroll
        for (int q = 0; q < CD_PG; ++q) {
            const unsigned r = (unsigned)std::min(row_in(q), last);
            const float* xr = x + row_base(p, r, OW, Ci);
#pragma unroll
            for (int s = 0; s < NCO; ++s) bg[buf][q][s] = gb[r * (unsigned)Co + (unsigned)cg[s]];
#pragma unroll
            for (int t = 0; t < NCN; ++t) bx[buf][q][t] = xr[cx[t]];
        }
    };
    auto compute = [&](int blk, int buf) __attribute__((always_inline)) {
        float u[CD_PG][NCN];
#pragma unroll
        for (int q = 0; q < CD_PG; ++q) {                 // all activations of the block first: independent chains
            const bool ok = blk < nb && base_of(blk) + row_in(q) < M;
#pragma unroll
            for (int t = 0; t < NCN; ++t) {
                float v = bx[buf][q][t];
                if (PRE == 2) {
                    v = v + a;
                    const float e = expm1f(v > 0.f ? 0.f : v);                        // elu_train without a branch (NaN stays NaN)
                    v = (v > 0.f ? v : e) + b;
                } else if (PRE == 1) {
                    v = v + b;
                }
                u[q][t] = (ok && n0 + 32 * t + li < N) ? v : 0.f;                     // zero-filled elements stay zero
            }
        }
#pragma unroll
        for (int q = 0; q < CD_PG; ++q) {
            const bool ok = blk < nb && base_of(blk) + row_in(q) < M;
#pragma unroll
            for (int s = 0; s < NCO; ++s) {
                const float gv = (ok && co0 + 32 * s + li < Co) ? bg[buf][q][s] : 0.f;
#pragma unroll
                for (int t = 0; t < NCN; ++t) acc[s][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv, u[q][t], acc[s][t], 0, 0, 0);
            }
        }
    };
    bool first = true;
    clear();
    fetch(0, 0);
    for (int blk = 0; blk < nb; blk += 2) {
        fetch(blk + 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        compute(blk, 0);
        fetch(blk + 2, 0);
        __builtin_amdgcn_sched_barrier(0);
        compute(blk + 1, 1);                              // adds zeros where blk + 1 == nb
        if ((blk + 2) % (CD_RUN / CD_WM) != 0 && blk + 2 < nb) continue;
        // end of an fp32 run: the four waves' sums in wave order; D [i = co][j = n]: lane holds n = li of sub-tile t, co rows
        // 8 (r / 4) + 4 hh + r % 4
        for (int wv = 0; wv < CD_THREADS / 64; ++wv) {
            if (wave == wv) {
#pragma unroll
                for (int s = 0; s < NCO; ++s)
#pragma unroll
                    for (int t = 0; t < NCN; ++t) {
                        const int n = n0 + 32 * t + li;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float* rp = red + ((s * NCN + t) * 16 + r) * 64 + lane;
                            if (wv == 0) {
                                *rp = acc[s][t][r];
                            } else if (wv < CD_THREADS / 64 - 1) {
                                *rp = *rp + acc[s][t][r];
                            } else {
                                const float v = *rp + acc[s][t][r];
                                const int co = co0 + 32 * s + 8 * (r >> 2) + 4 * hh + (r & 3);
                                if (co < Co && n < N) {
                                    double* p = slot + (int64_t)co * N + n;
                                    *p = first ? (double)v : *p + (double)v;
                                }
                            }
                        }
                    }
            }
            __syncthreads();
        }
        first = false;
        clear();
    }
}

// slots [P][Co][2][2][Ci] -> g_w in the weight's own layout (0: [Co][Ci][2][2], 1: [Co][2][2][Ci])
__global__ __launch_bounds__(CD_THREADS)
void cd_wgrad_final(const double* __restrict__ slots, int P, int n, int Ci, int w_layout, float* __restrict__ g_w) {
    const int i = blockIdx.x * CD_THREADS + threadIdx.x;
    if (i >= n) return;
    // index order, 32 loads in flight at a time (a slot past the end reads the last one and is not added)
    double s = 0.0;
    for (int p0 = 0; p0 < P; p0 += 32) {
        double v[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) v[j] = slots[(int64_t)std::min(p0 + j, P - 1) * n + i];
#pragma unroll
        for (int j = 0; j < 32; ++j) s = p0 + j < P ? s + v[j] : s;
    }
    int o = i;
    if (w_layout == 0) {
        const int co = i / (4 * Ci), r = i - co * 4 * Ci, tap = r / Ci, ci = r - tap * Ci;
        o = co * 4 * Ci + ci * 4 + tap;
    }
    g_w[o] = (float)s;
}

inline bool cd_supported(int cin, int cout) {
    return cin >= 8 && cout >= 8 && cin <= CD_MAXC && cout <= CD_MAXC && cin % 8 == 0 && cout % 8 == 0;
}

struct WgradPlan { int P; int tiles; int nco; int ncn; };
inline WgradPlan wgrad_plan(int64_t m, int cin, int cout) {
    WgradPlan p;
    p.nco = cout <= 32 ? 1 : 2;                                        // output tile: 32 nco co x 32 ncn columns of 4 cin
    p.ncn = 4 * cin <= 32 ? 1 : 2;
    p.tiles = (int)(ceil_div(cout, 32 * p.nco) * ceil_div(4 * cin, 32 * p.ncn));
    const int64_t pmax = std::min<int64_t>(CD_SLOTS, std::max<int64_t>(1, CD_SLOT_ELEMS / ((int64_t)4 * cin * cout)));
    p.P = (int)std::min<int64_t>(pmax, ceil_div(m, CD_WM));          // every workgroup has at least one 64-row block
    return p;
}

inline bool cd_aligned16(std::initializer_list<const void*> ps) {
    uintptr_t m = 0;
    for (const void* p : ps) m |= (uintptr_t)p;
    return (m & 15) == 0;
}

template <bool BWD>
inline void launch_gemm(int nt, dim3 grid, hipStream_t stream, const float* A, const float* xe, const float* pa, const float* pb,
                        int pre, const float* w, int64_t M, int OW, int Ci, int K, int N, float* out, double* partials) {
    if (nt == 1) cd_gemm<1, BWD><<<grid, CD_THREADS, 0, stream>>>(A, xe, pa, pb, pre, w, M, OW, Ci, K, N, out, partials);
    else if (nt == 2) cd_gemm<2, BWD><<<grid, CD_THREADS, 0, stream>>>(A, xe, pa, pb, pre, w, M, OW, Ci, K, N, out, partials);
    else if (nt == 4) cd_gemm<4, BWD><<<grid, CD_THREADS, 0, stream>>>(A, xe, pa, pb, pre, w, M, OW, Ci, K, N, out, partials);
    else cd_gemm<8, BWD><<<grid, CD_THREADS, 0, stream>>>(A, xe, pa, pb, pre, w, M, OW, Ci, K, N, out, partials);
}

template <int NCO, int NCN>
inline void launch_wgrad_pre(int pre, dim3 grid, hipStream_t stream, const float* g, const float* x, const float* a, const float* b,
                             int64_t m, int ow, int cin, int cout, double* slots) {
    if (pre == 0) cd_wgrad<NCO, NCN, 0><<<grid, CD_THREADS, 0, stream>>>(g, x, a, b, m, ow, cin, cout, slots);
    else if (pre == 1) cd_wgrad<NCO, NCN, 1><<<grid, CD_THREADS, 0, stream>>>(g, x, a, b, m, ow, cin, cout, slots);
    else cd_wgrad<NCO, NCN, 2><<<grid, CD_THREADS, 0, stream>>>(g, x, a, b, m, ow, cin, cout, slots);
}

inline void launch_wgrad(int nco, int ncn, int pre, dim3 grid, hipStream_t stream, const float* g, const float* x, const float* a,
                         const float* b, int64_t m, int ow, int cin, int cout, double* slots) {
    if (nco == 1 && ncn == 1) launch_wgrad_pre<1, 1>(pre, grid, stream, g, x, a, b, m, ow, cin, cout, slots);
    else if (nco == 1) launch_wgrad_pre<1, 2>(pre, grid, stream, g, x, a, b, m, ow, cin, cout, slots);
    else if (ncn == 1) launch_wgrad_pre<2, 1>(pre, grid, stream, g, x, a, b, m, ow, cin, cout, slots);
    else launch_wgrad_pre<2, 2>(pre, grid, stream, g, x, a, b, m, ow, cin, cout, slots);
}

inline int tiles_for(int n) { return n <= 32 ? 1 : n <= 64 ? 2 : n <= 128 ? 4 : 8; }
inline int gemm_grid(int64_t m) { return (int)std::min<int64_t>(CD_MAX_WG, ceil_div(m, CD_BM)); }

// rows M = b (h / 2) (w / 2) when the geometry is valid and M < 2^40, else 0
inline int64_t cd_rows(int64_t b, int h, int w) {
    if (b < 1 || h < 2 || w < 2 || (h & 1) || (w & 1)) return 0;
    const int64_t per = (int64_t)(h / 2) * (w / 2);
    if (per >= (1ll << 40) || b >= (1ll << 40) / per + 1) return 0;
    const int64_t m = b * per;
    return m < (1ll << 40) ? m : 0;
}

// the workspace: [permuted weight, 16-byte aligned][slots][partials]
struct Workspace { float* wp; double* slots; double* partials; };
inline size_t wp_bytes(int cin, int cout) { return (size_t)round_up((int64_t)4 * cin * cout * sizeof(float), 256); }
inline Workspace carve(void* ws, const WgradPlan& plan, int cin, int cout) {
    Workspace o;
    char* p = (char*)(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    o.wp = (float*)p;
    o.slots = (double*)(p + wp_bytes(cin, cout));
    o.partials = o.slots + (size_t)plan.P * 4 * cin * cout;
    return o;
}

inline void permute_w(const float* w, int cin, int cout, float* wp, hipStream_t stream) {
    const int n = 4 * cin * cout;
    cd_permute_w<<<(n + CD_THREADS - 1) / CD_THREADS, CD_THREADS, 0, stream>>>(w, cin, n, wp);
}

}  // namespace

extern "C" int vqae_conv_down_train_supported(int cin, int cout) { return cd_supported(cin, cout) ? 1 : 0; }

extern "C" int vqae_conv_down_train_wgrad_run(void) { return CD_RUN; }

extern "C" size_t vqae_conv_down_train_workspace_bytes(int64_t b, int h, int w, int cin, int cout) {
    const int64_t m = cd_rows(b, h, w);
    if (m < 1 || !cd_supported(cin, cout)) return 0;
    const WgradPlan p = wgrad_plan(m, cin, cout);
    return wp_bytes(cin, cout) + (size_t)p.P * 4 * cin * cout * sizeof(double) +
           (size_t)CD_MAX_WG * CD_MAX_PIECES * 2 * sizeof(double) + 256;
}

extern "C" int vqae_conv_down_train_forward_f32(const float* x, const float* a, const float* b, int pre, const float* w,
                                                int w_layout, int64_t batch, int h, int wd, int cin, int cout, float* y, void* ws,
                                                void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VQAE_REQUIRE(batch >= 1 && h >= 1 && wd >= 1, VQAE_ERR_INVALID, "conv_down_train_forward: batch %lld h %d w %d",
                 (long long)batch, h, wd);
    VQAE_REQUIRE(pre >= 0 && pre <= 2, VQAE_ERR_INVALID, "conv_down_train_forward: pre %d", pre);
    VQAE_REQUIRE(w_layout >= 0 && w_layout <= 1, VQAE_ERR_INVALID, "conv_down_train_forward: w_layout %d", w_layout);
    VQAE_REQUIRE(x && w && y && (ws || w_layout == 1) && (pre < 1 || b) && (pre < 2 || a), VQAE_ERR_INVALID,
                 "conv_down_train_forward: null pointer");                 // the forward uses the workspace for w_layout 0 only
    VQAE_REQUIRE(cd_supported(cin, cout), VQAE_ERR_UNSUPPORTED,
                 "conv_down_train_forward: cin %d cout %d (multiples of 8, 8 .. %d)", cin, cout, CD_MAXC);
    VQAE_REQUIRE(h % 2 == 0 && wd % 2 == 0, VQAE_ERR_UNSUPPORTED, "conv_down_train_forward: h %d w %d must be even", h, wd);
    const int64_t m = cd_rows(batch, h, wd);
    VQAE_REQUIRE(m >= 1, VQAE_ERR_INVALID, "conv_down_train_forward: batch %lld x %d x %d output rows exceed 2^40",
                 (long long)batch, h / 2, wd / 2);
    VQAE_REQUIRE(cd_aligned16({x, w, y}) && ((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID,
                 "conv_down_train_forward: x, w and y must be 16-byte aligned, the workspace 8-byte aligned");
    const Workspace wk = carve(ws, wgrad_plan(m, cin, cout), cin, cout);
    if (w_layout == 0) {
        permute_w(w, cin, cout, wk.wp, stream);
        VQAE_LAUNCH_CHECK();
    }
    launch_gemm<false>(tiles_for(cout), dim3(gemm_grid(m)), stream, x, nullptr, a, b, pre, w_layout == 0 ? wk.wp : w, m, wd / 2, cin,
                       4 * cin, cout, y, nullptr);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" int vqae_conv_down_train_backward_f32(const float* g, const float* x, const float* a, const float* b, int pre,
                                                 const float* w, int w_layout, int64_t batch, int h, int wd, int cin, int cout,
                                                 float* g_x, float* g_w, float* g_a, float* g_b, void* ws, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VQAE_REQUIRE(batch >= 1 && h >= 1 && wd >= 1, VQAE_ERR_INVALID, "conv_down_train_backward: batch %lld h %d w %d",
                 (long long)batch, h, wd);
    VQAE_REQUIRE(pre >= 0 && pre <= 2, VQAE_ERR_INVALID, "conv_down_train_backward: pre %d", pre);
    VQAE_REQUIRE(w_layout >= 0 && w_layout <= 1, VQAE_ERR_INVALID, "conv_down_train_backward: w_layout %d", w_layout);
    VQAE_REQUIRE(g && x && w && ws && (pre < 1 || b) && (pre < 2 || a), VQAE_ERR_INVALID, "conv_down_train_backward: null pointer");
    VQAE_REQUIRE(cd_supported(cin, cout), VQAE_ERR_UNSUPPORTED,
                 "conv_down_train_backward: cin %d cout %d (multiples of 8, 8 .. %d)", cin, cout, CD_MAXC);
    VQAE_REQUIRE(h % 2 == 0 && wd % 2 == 0, VQAE_ERR_UNSUPPORTED, "conv_down_train_backward: h %d w %d must be even", h, wd);
    const int64_t m = cd_rows(batch, h, wd);
    VQAE_REQUIRE(m >= 1, VQAE_ERR_INVALID, "conv_down_train_backward: batch %lld x %d x %d output rows exceed 2^40",
                 (long long)batch, h / 2, wd / 2);
    VQAE_REQUIRE(cd_aligned16({g, x, w, g_x, g_w}) && ((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID,
                 "conv_down_train_backward: tensors must be 16-byte aligned, the workspace 8-byte aligned");
    const WgradPlan plan = wgrad_plan(m, cin, cout);
    const Workspace wk = carve(ws, plan, cin, cout);
    const int ow = wd / 2, n_all = 4 * cin;
    float* o_a = pre == 2 ? g_a : nullptr;
    float* o_b = pre >= 1 ? g_b : nullptr;
    if (g_x || o_a || o_b) {
        if (w_layout == 0) {
            permute_w(w, cin, cout, wk.wp, stream);
            VQAE_LAUNCH_CHECK();
        }
        const int nt = tiles_for(std::min(n_all, 256));
        const dim3 grid(gemm_grid(m), (unsigned)ceil_div(n_all, 32 * nt));
        launch_gemm<true>(nt, grid, stream, g, x, a, b, pre, w_layout == 0 ? wk.wp : w, m, ow, cin, cout, n_all, g_x, wk.partials);
        VQAE_LAUNCH_CHECK();
        if (o_a || o_b) {
            cd_sum_final<<<1, CD_THREADS, 0, stream>>>(wk.partials, (int)(grid.x * grid.y), o_a, o_b);
            VQAE_LAUNCH_CHECK();
        }
    }
    if (g_w) {
        const dim3 grid(plan.P, plan.tiles);
        launch_wgrad(plan.nco, plan.ncn, pre, grid, stream, g, x, a, b, m, ow, cin, cout, wk.slots);
        VQAE_LAUNCH_CHECK();
        const int n = n_all * cout;
        cd_wgrad_final<<<(n + CD_THREADS - 1) / CD_THREADS, CD_THREADS, 0, stream>>>(wk.slots, plan.P, n, cin, w_layout, g_w);
        VQAE_LAUNCH_CHECK();
    }
    return VQAE_OK;
}
