// Trainable 1x1, stride-1 convolution of a Fixup block (conv_block.py:196-216; proj2d.yaml: bias-free 1x1), fp32, NHWC, with the
// element-wise op in front of it folded in:  y [M][Co] = u [M][Ci] . w^T,  M = B H W,  w [Co][Ci] as torch stores [Co, Ci, 1, 1],
//     pre = 0: u = x        pre = 1: u = x + *b        pre = 2: u = ELU(x + *a) + *b        (a, b read from DEVICE memory)
// u is never written to memory.  All products run on v_mfma_f32_32x32x2_f32.
//
// Three kernels, all shape-generic (Ci, Co multiples of 8 up to 256, any M; in the M, K and N tails the operands are zero and
// the stores range-checked; templates choose tile COUNTS, never a shape).  The backward is two launches -- data gradient, then
// weight gradient -- not one: a fused form would hold a Co x Ci accumulator next to the 128 x Ci one of the data gradient
// (at 256 x 256 that is 64 K + 32 K floats per workgroup, more than the register file of a CU), and either output may be
// NULL.  The price is that g and x are read twice.
//
//   c1_gemm<NT, false>   forward.   A workgroup of 4 waves owns 128 rows x all Co columns (wave = 32 rows x NT 32-column
//                        tiles, NT = 1 / 2 / 4 / 8 by Co), K = Ci walked in chunks of 32: the x chunk is staged to LDS with the
//                        pre-op applied ONCE per element (fp32 MFMA and VALU do not co-execute, so no expm1f in the MFMA loop),
//                        the w chunk next to it; both k-contiguous, row stride 36 floats: a lane reads 4 consecutive k of its
//                        row with one 128-bit LDS read and feeds 4 MFMAs (the same k permutation on both operands).
//   c1_gemm<NT, true>    data gradient, the same loop with A = g, K = Co, N = Ci and w staged TRANSPOSED (w [k][n] is
//                        n-contiguous);  epilogue: g_u = acc, g_x = g_u * ELU'(x + *a) (ELU'(v) = v > 0 ? 1 : exp(v), x read at
//                        the output element), fp64 sums of g_x and g_u per thread in a fixed order.
//                        Both forms load the next chunk into registers while the MFMAs of the current one run.
//   c1_wgrad             weight gradient  g_w [co][ci] = sum_m g[m][co] u[m][ci], u recomputed from x.  Grid (P, output tiles of
//                        up to 64 co x 64 ci).  Rows are cut into blocks of 64; workgroup p takes blocks p, p + P, ...; its four
//                        waves split the rows of a block and each accumulates the whole tile in fp32, operands straight from
//                        global memory (lane = channel, the MFMA's own layout), one block of loads ahead.  After a run of
//                        C1_RUN = 512 rows the waves' sums are added in wave order and the run goes into the workgroup's OWN
//                        fp64 slot of the workspace (plain store on the first run: the workspace needs no clearing, nobody
//                        else touches the slot).  c1_wgrad_final adds the P slots in index order in fp64, rounds to fp32 once.
//
// Determinism: every grid is a function of (M, Ci, Co) alone, there are no floating-point atomics, every sum has one fixed
// order: two runs give the same bits.  The scalar sums follow fixup_train.hip: thread (fp64, index order) -> wave shuffle ->
// 4 waves in order -> one fp64 row per workgroup -> c1_sum_final (one workgroup, fixed order, one rounding).
//
// Workspace: P slots of Co Ci doubles with P <= 256 and P Co Ci <= 2^20 (at most 8 MiB whatever M is) + 1024 rows of two
// doubles for the scalar sums.
#include <algorithm>

#include "kernels.h"
#include "mfma.h"

namespace {

using namespace vqae;

constexpr int C1_THREADS = 256;
constexpr int C1_BM = 128;               // rows of a forward / data-gradient workgroup tile
constexpr int C1_KC = 32;                // k chunk staged per step
constexpr int C1_LD = C1_KC + 4;         // LDS row stride in floats: 16-byte aligned rows, 128-bit reads of 16 lanes hit all banks
constexpr int C1_MAX_WG = 1024;          // workgroups of c1_gemm = rows of fp64 partials of the scalar sums
constexpr int C1_RUN = 512;              // longest fp32 accumulation run of g_w, in rows
constexpr int C1_WM = 64;                // rows of a c1_wgrad block
constexpr int C1_PG = 8;                 // row pairs a c1_wgrad wave loads ahead of its MFMAs
constexpr int C1_SLOTS = 256;            // P <= C1_SLOTS and P Co Ci <= C1_SLOT_ELEMS (P >= 1): at most 8 MiB of fp64 partials
constexpr int64_t C1_SLOT_ELEMS = 1 << 20;
constexpr int C1_MAXC = 256;

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

// BWD false:  out [M][N] = pre(A [M][K]) . w [N][K]^T                                 (forward: K = Ci, N = Co)
// BWD true:   out [M][N] = (A [M][K] . w [K][N]) * ELU'(xe [M][N] + a), sums           (data gradient: K = Co, N = Ci)
template <int NT, bool BWD>
__global__ __launch_bounds__(C1_THREADS)
void c1_gemm(const float* __restrict__ A, const float* __restrict__ xe, const float* __restrict__ pa,
             const float* __restrict__ pb, int pre, const float* __restrict__ w, int64_t M, int K, int N,
             float* __restrict__ out, double* __restrict__ partials) {
    __shared__ __attribute__((aligned(16))) float Al[C1_BM * C1_LD];
    __shared__ __attribute__((aligned(16))) float Wl[NT * 32 * C1_LD];
    __shared__ double red[2][C1_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    const float a = pre == 2 ? *pa : 0.f, b = (!BWD && pre >= 1) ? *pb : 0.f;
    const int64_t n_tiles = (M + C1_BM - 1) / C1_BM;
    double s0 = 0.0, s1 = 0.0;
    // One chunk = 128 rows x 32 k of A (4 16-byte groups per thread) and NT * 32 columns x 32 k of w (NT groups per thread),
    // zero where a row, a column or k is out of range (K % 8 == 0, N % 8 == 0: a group is in or out as a whole).  fetch()
    // brings the NEXT chunk into registers while the MFMA loop runs on the current one: branch-free loads, an out-of-range
    // group reads the nearest valid address instead (no control flow between the loads and the MFMA loop, so nothing waits
    // for them there); commit() zeroes those groups, applies the pre-op and writes the chunk to LDS.
    f32x4 ra[C1_BM * (C1_KC / 4) / C1_THREADS], rw[NT];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    auto fetch = [&](int64_t m0, int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < C1_BM * (C1_KC / 4) / C1_THREADS; ++j) {
            const int i = tid + j * C1_THREADS, k = k0 + 4 * (i & 7);
            const int64_t m = m0 + (i >> 3);
            ra[j] = *reinterpret_cast<const f32x4*>(A + std::min(m, M - 1) * K + std::min(k, K - 4));
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int i = tid + j * C1_THREADS;
            if (!BWD) {                  // w [n][k]: k-contiguous as stored
                const int n = i >> 3, k = k0 + 4 * (i & 7);
                rw[j] = *reinterpret_cast<const f32x4*>(w + (int64_t)std::min(n, N - 1) * K + std::min(k, K - 4));
            } else {                     // w [k][n]: n-contiguous
                const int kk = i / (NT * 8), n = 4 * (i % (NT * 8));
                rw[j] = *reinterpret_cast<const f32x4*>(w + (int64_t)std::min(k0 + kk, K - 1) * N + std::min(n, N - 4));
            }
        }
    };
    auto commit = [&](int64_t m0, int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < C1_BM * (C1_KC / 4) / C1_THREADS; ++j) {
            const int i = tid + j * C1_THREADS, k = k0 + 4 * (i & 7);
            const int64_t m = m0 + (i >> 3);
            f32x4 v = (m < M && k < K) ? ra[j] : zero4;
            if (!BWD && m < M && k < K) v = pre_op(v, pre, a, b);          // zero-filled elements stay zero
            *reinterpret_cast<f32x4*>(Al + (i >> 3) * C1_LD + 4 * (i & 7)) = v;
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int i = tid + j * C1_THREADS;
            if (!BWD) {
                *reinterpret_cast<f32x4*>(Wl + (i >> 3) * C1_LD + 4 * (i & 7)) = ((i >> 3) < N && k0 + 4 * (i & 7) < K) ? rw[j] : zero4;
            } else {                     // transposed into the k-contiguous LDS rows
                const int kk = i / (NT * 8), n = 4 * (i % (NT * 8));
#pragma unroll
                for (int e = 0; e < 4; ++e) Wl[(n + e) * C1_LD + kk] = (k0 + kk < K && n < N) ? rw[j][e] : 0.f;
            }
        }
    };
    if ((int64_t)blockIdx.x < n_tiles) fetch((int64_t)blockIdx.x * C1_BM, 0);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t m0 = tile * C1_BM;
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        for (int k0 = 0; k0 < K; k0 += C1_KC) {
            commit(m0, k0);
            __syncthreads();
            if (k0 + C1_KC < K) fetch(m0, k0 + C1_KC);
            else if (tile + gridDim.x < n_tiles) fetch((tile + gridDim.x) * C1_BM, 0);
            const int slices = std::min(C1_KC, K - k0) / 8;
            const float* ap = Al + (wave * 32 + li) * C1_LD + 4 * hh;
            const float* bp = Wl + li * C1_LD + 4 * hh;
            for (int u = 0; u < slices; ++u) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(ap + 8 * u);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const f32x4 bv = *reinterpret_cast<const f32x4*>(bp + t * 32 * C1_LD + 8 * u);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r], bv[r], acc[t], 0, 0, 0);
                }
            }
            __syncthreads();
        }
        // D [i = row][j = column]: lane (li, hh) holds column li of its tile, rows 8 (r / 4) + 4 hh + r % 4
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = t * 32 + li;
            if (col < N) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t m = m0 + wave * 32 + 8 * (r >> 2) + 4 * hh + (r & 3);
                    if (m < M) {
                        float v = acc[t][r];
                        if (BWD) {
                            s1 += (double)v;
                            if (pre == 2) v = v * elu_grad(xe[m * N + col] + a);
                            s0 += (double)v;
                        }
                        if (out) out[m * N + col] = v;
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
            partials[(int64_t)blockIdx.x * 2 + 0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
            partials[(int64_t)blockIdx.x * 2 + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        }
    }
}

// One workgroup: thread t adds rows t, t + 256, ... in that order, then the wave / workgroup order of c1_gemm.
__global__ __launch_bounds__(C1_THREADS)
void c1_sum_final(const double* __restrict__ partials, int n_wg, float* __restrict__ o0, float* __restrict__ o1) {
    __shared__ double red[2][C1_THREADS / 64];
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < n_wg; i += C1_THREADS) {
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

// Rows are cut into blocks of C1_WM = 64; workgroup p of the P of an output tile (blockIdx.y: 32 NCO co x 32 NCI ci) takes
// the blocks p, p + P, p + 2 P, ... in that order -- interleaved, so that at any moment the workgroups read neighbouring
// memory and not addresses a power of two apart.  The four waves split the ROWS of a block: wave w takes its row pairs
// w, w + 4, ..., w + 28 (lane (li, hh) row 2 pair + hh), reads its operands straight from global memory (32 consecutive
// channels of a row per half-wave: one 128-byte segment) and accumulates the whole tile; no LDS, no barrier in the loop.
// The loads of a block are issued one block ahead of its MFMAs.  After every C1_RUN / 64 = 8 blocks (one fp32 run) and at the
// end, the four accumulators are added in wave order through LDS, ((w0 + w1) + w2) + w3, and wave 3 adds the run into the
// workgroup's fp64 slot.
// PRE is a template argument so that the loop body is straight-line code: with a run-time branch per element the compiler
// sinks the early loads down to their uses and the latency is paid in full.
template <int NCO, int NCI, int PRE>
__global__ __launch_bounds__(C1_THREADS)
void c1_wgrad(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ pa,
              const float* __restrict__ pb, int64_t M, int Ci, int Co, double* __restrict__ slots) {
    static_assert(C1_WM == 8 * C1_PG && C1_RUN % C1_WM == 0 && (C1_RUN / C1_WM) % 2 == 0, "a block is one load group per wave");
    __shared__ float red[NCO * NCI * 16 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    const int tiles_ci = (Ci + 32 * NCI - 1) / (32 * NCI);
    const int co0 = (blockIdx.y / tiles_ci) * 32 * NCO, ci0 = (blockIdx.y % tiles_ci) * 32 * NCI;
    const float a = PRE == 2 ? *pa : 0.f, b = PRE >= 1 ? *pb : 0.f;
    const int64_t n_blocks = (M + C1_WM - 1) / C1_WM;
    const int P = gridDim.x;
    int cg[NCO], cx[NCI];                                 // this lane's channels, clamped for the loads
#pragma unroll
    for (int s = 0; s < NCO; ++s) cg[s] = std::min(co0 + 32 * s + li, Co - 1);
#pragma unroll
    for (int t = 0; t < NCI; ++t) cx[t] = std::min(ci0 + 32 * t + li, Ci - 1);
    const int nb = (int)((n_blocks - blockIdx.x + P - 1) / P);                        // this workgroup's blocks: >= 1
    double* slot = slots + (int64_t)blockIdx.x * Co * Ci;
    f32x16 acc[NCO][NCI];
    auto clear = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NCO; ++s)
#pragma unroll
            for (int t = 0; t < NCI; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[s][t][r] = 0.f;
    };
    float bg[2][C1_PG][NCO], bx[2][C1_PG][NCI];
    // first row of the workgroup's block number blk (uniform), and this lane's row inside a block for pair q of its wave
    auto base_of = [&](int blk) __attribute__((always_inline)) { return ((int64_t)blockIdx.x + (int64_t)blk * P) * C1_WM; };
    auto row_in = [&](int q) __attribute__((always_inline)) { return 2 * (wave + 4 * q) + hh; };
    // branch-free: a block past the end reads the last block, a row past the end row M - 1, a missing channel the last one;
    // compute() zeroes them.  One 64-bit base per block, 32-bit offsets per load.
    auto fetch = [&](int blk, int buf) __attribute__((always_inline)) {
        const int64_t base = std::min(base_of(blk), (n_blocks - 1) * C1_WM);
        const int last = (int)std::min<int64_t>(C1_WM - 1, M - 1 - base);
        const float* gb = g + base * Co;
        const float* xb = x + base * Ci;
#pragma unroll
        for (int q = 0; q < C1_PG; ++q) {
            const unsigned r = (unsigned)std::min(row_in(q), last);
#pragma unroll
            for (int s = 0; s < NCO; ++s) bg[buf][q][s] = gb[r * (unsigned)Co + (unsigned)cg[s]];
#pragma unroll
            for (int t = 0; t < NCI; ++t) bx[buf][q][t] = xb[r * (unsigned)Ci + (unsigned)cx[t]];
        }
    };
    auto compute = [&](int blk, int buf) __attribute__((always_inline)) {
        float u[C1_PG][NCI];
#pragma unroll
        for (int q = 0; q < C1_PG; ++q) {                 // all activations of the block first: independent chains
            const bool ok = blk < nb && base_of(blk) + row_in(q) < M;
#pragma unroll
            for (int t = 0; t < NCI; ++t) {
                float v = bx[buf][q][t];
                if (PRE == 2) {
                    v = v + a;
                    const float e = expm1f(v > 0.f ? 0.f : v);                        // elu_train without a branch (NaN stays NaN)
                    v = (v > 0.f ? v : e) + b;
                } else if (PRE == 1) {
                    v = v + b;
                }
                u[q][t] = (ok && ci0 + 32 * t + li < Ci) ? v : 0.f;                   // zero-filled elements stay zero
            }
        }
#pragma unroll
        for (int q = 0; q < C1_PG; ++q) {
            const bool ok = blk < nb && base_of(blk) + row_in(q) < M;
#pragma unroll
            for (int s = 0; s < NCO; ++s) {
                const float gv = (ok && co0 + 32 * s + li < Co) ? bg[buf][q][s] : 0.f;
#pragma unroll
                for (int t = 0; t < NCI; ++t) acc[s][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv, u[q][t], acc[s][t], 0, 0, 0);
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
        if ((blk + 2) % (C1_RUN / C1_WM) != 0 && blk + 2 < nb) continue;
        // end of an fp32 run: the four waves' sums in wave order; D [i = co][j = ci]: lane holds ci = li of sub-tile t, co rows
        // 8 (r / 4) + 4 hh + r % 4
        for (int wv = 0; wv < C1_THREADS / 64; ++wv) {
            if (wave == wv) {
#pragma unroll
                for (int s = 0; s < NCO; ++s)
#pragma unroll
                    for (int t = 0; t < NCI; ++t) {
                        const int ci = ci0 + 32 * t + li;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float* rp = red + ((s * NCI + t) * 16 + r) * 64 + lane;
                            if (wv == 0) {
                                *rp = acc[s][t][r];
                            } else if (wv < C1_THREADS / 64 - 1) {
                                *rp = *rp + acc[s][t][r];
                            } else {
                                const float v = *rp + acc[s][t][r];
                                const int co = co0 + 32 * s + 8 * (r >> 2) + 4 * hh + (r & 3);
                                if (co < Co && ci < Ci) {
                                    double* p = slot + (int64_t)co * Ci + ci;
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

__global__ __launch_bounds__(C1_THREADS)
void c1_wgrad_final(const double* __restrict__ slots, int P, int n, float* __restrict__ g_w) {
    const int i = blockIdx.x * C1_THREADS + threadIdx.x;
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
    g_w[i] = (float)s;
}

inline bool c1_supported(int cin, int cout) {
    return cin >= 8 && cout >= 8 && cin <= C1_MAXC && cout <= C1_MAXC && cin % 8 == 0 && cout % 8 == 0;
}

struct WgradPlan { int P; int tiles; int nco; int nci; };
inline WgradPlan wgrad_plan(int64_t m, int cin, int cout) {
    WgradPlan p;
    p.nco = cout <= 32 ? 1 : 2;                                        // output tile: 32 nco co x 32 nci ci
    p.nci = cin <= 32 ? 1 : 2;
    p.tiles = (int)(ceil_div(cout, 32 * p.nco) * ceil_div(cin, 32 * p.nci));
    const int64_t pmax = std::min<int64_t>(C1_SLOTS, std::max<int64_t>(1, C1_SLOT_ELEMS / ((int64_t)cin * cout)));
    p.P = (int)std::min<int64_t>(pmax, ceil_div(m, C1_WM));          // every workgroup has at least one 64-row block
    return p;
}

inline bool c1_aligned16(std::initializer_list<const void*> ps) {
    uintptr_t m = 0;
    for (const void* p : ps) m |= (uintptr_t)p;
    return (m & 15) == 0;
}

template <bool BWD>
inline void launch_gemm(int nt, int grid, hipStream_t stream, const float* A, const float* xe, const float* pa, const float* pb,
                        int pre, const float* w, int64_t M, int K, int N, float* out, double* partials) {
    if (nt == 1) c1_gemm<1, BWD><<<grid, C1_THREADS, 0, stream>>>(A, xe, pa, pb, pre, w, M, K, N, out, partials);
    else if (nt == 2) c1_gemm<2, BWD><<<grid, C1_THREADS, 0, stream>>>(A, xe, pa, pb, pre, w, M, K, N, out, partials);
    else if (nt == 4) c1_gemm<4, BWD><<<grid, C1_THREADS, 0, stream>>>(A, xe, pa, pb, pre, w, M, K, N, out, partials);
    else c1_gemm<8, BWD><<<grid, C1_THREADS, 0, stream>>>(A, xe, pa, pb, pre, w, M, K, N, out, partials);
}

template <int NCO, int NCI>
inline void launch_wgrad_pre(int pre, dim3 grid, hipStream_t stream, const float* g, const float* x, const float* a, const float* b,
                             int64_t m, int cin, int cout, double* slots) {
    if (pre == 0) c1_wgrad<NCO, NCI, 0><<<grid, C1_THREADS, 0, stream>>>(g, x, a, b, m, cin, cout, slots);
    else if (pre == 1) c1_wgrad<NCO, NCI, 1><<<grid, C1_THREADS, 0, stream>>>(g, x, a, b, m, cin, cout, slots);
    else c1_wgrad<NCO, NCI, 2><<<grid, C1_THREADS, 0, stream>>>(g, x, a, b, m, cin, cout, slots);
}

inline void launch_wgrad(int nco, int nci, int pre, dim3 grid, hipStream_t stream, const float* g, const float* x, const float* a,
                         const float* b, int64_t m, int cin, int cout, double* slots) {
    if (nco == 1 && nci == 1) launch_wgrad_pre<1, 1>(pre, grid, stream, g, x, a, b, m, cin, cout, slots);
    else if (nco == 1) launch_wgrad_pre<1, 2>(pre, grid, stream, g, x, a, b, m, cin, cout, slots);
    else if (nci == 1) launch_wgrad_pre<2, 1>(pre, grid, stream, g, x, a, b, m, cin, cout, slots);
    else launch_wgrad_pre<2, 2>(pre, grid, stream, g, x, a, b, m, cin, cout, slots);
}

inline int tiles_for(int n) { return n <= 32 ? 1 : n <= 64 ? 2 : n <= 128 ? 4 : 8; }
inline int gemm_grid(int64_t m) { return (int)std::min<int64_t>(C1_MAX_WG, ceil_div(m, C1_BM)); }

}  // namespace

extern "C" int vqae_conv1x1_train_supported(int cin, int cout) { return c1_supported(cin, cout) ? 1 : 0; }

extern "C" int vqae_conv1x1_train_wgrad_run(void) { return C1_RUN; }

extern "C" size_t vqae_conv1x1_train_workspace_bytes(int64_t m, int cin, int cout) {
    if (m < 1 || !c1_supported(cin, cout)) return 0;
    const WgradPlan p = wgrad_plan(m, cin, cout);
    return (size_t)p.P * cin * cout * sizeof(double) + (size_t)C1_MAX_WG * 2 * sizeof(double) + 256;
}

extern "C" int vqae_conv1x1_train_forward_f32(const float* x, const float* a, const float* b, int pre, const float* w, int64_t m,
                                              int cin, int cout, float* y, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VQAE_REQUIRE(m >= 1 && m < (1ll << 40), VQAE_ERR_INVALID, "conv1x1_train_forward: %lld rows", (long long)m);
    VQAE_REQUIRE(pre >= 0 && pre <= 2, VQAE_ERR_INVALID, "conv1x1_train_forward: pre %d", pre);
    VQAE_REQUIRE(x && w && y && (pre < 1 || b) && (pre < 2 || a), VQAE_ERR_INVALID, "conv1x1_train_forward: null pointer");
    VQAE_REQUIRE(c1_supported(cin, cout), VQAE_ERR_UNSUPPORTED,
                 "conv1x1_train_forward: cin %d cout %d (multiples of 8, 8 .. %d)", cin, cout, C1_MAXC);
    VQAE_REQUIRE(c1_aligned16({x, w, y}), VQAE_ERR_INVALID, "conv1x1_train_forward: x, w and y must be 16-byte aligned");
    launch_gemm<false>(tiles_for(cout), gemm_grid(m), stream, x, nullptr, a, b, pre, w, m, cin, cout, y, nullptr);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" int vqae_conv1x1_train_backward_f32(const float* g, const float* x, const float* a, const float* b, int pre,
                                               const float* w, int64_t m, int cin, int cout, float* g_x, float* g_w, float* g_a,
                                               float* g_b, void* ws, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VQAE_REQUIRE(m >= 1 && m < (1ll << 40), VQAE_ERR_INVALID, "conv1x1_train_backward: %lld rows", (long long)m);
    VQAE_REQUIRE(pre >= 0 && pre <= 2, VQAE_ERR_INVALID, "conv1x1_train_backward: pre %d", pre);
    VQAE_REQUIRE(g && x && w && ws && (pre < 1 || b) && (pre < 2 || a), VQAE_ERR_INVALID, "conv1x1_train_backward: null pointer");
    VQAE_REQUIRE(c1_supported(cin, cout), VQAE_ERR_UNSUPPORTED,
                 "conv1x1_train_backward: cin %d cout %d (multiples of 8, 8 .. %d)", cin, cout, C1_MAXC);
    VQAE_REQUIRE(c1_aligned16({g, x, w, g_x, g_w}) && ((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID,
                 "conv1x1_train_backward: tensors must be 16-byte aligned, the workspace 8-byte aligned");
    const WgradPlan plan = wgrad_plan(m, cin, cout);
    double* slots = (double*)ws;
    double* partials = slots + (size_t)plan.P * cin * cout;
    float* o_a = pre == 2 ? g_a : nullptr;
    float* o_b = pre >= 1 ? g_b : nullptr;
    if (g_x || o_a || o_b) {
        const int grid = gemm_grid(m);
        launch_gemm<true>(tiles_for(cin), grid, stream, g, x, a, b, pre, w, m, cout, cin, g_x, partials);
        VQAE_LAUNCH_CHECK();
        if (o_a || o_b) {
            c1_sum_final<<<1, C1_THREADS, 0, stream>>>(partials, grid, o_a, o_b);
            VQAE_LAUNCH_CHECK();
        }
    }
    if (g_w) {
        const dim3 grid(plan.P, plan.tiles);
        launch_wgrad(plan.nco, plan.nci, pre, grid, stream, g, x, a, b, m, cin, cout, slots);
        VQAE_LAUNCH_CHECK();
        const int n = cin * cout;
        c1_wgrad_final<<<(n + C1_THREADS - 1) / C1_THREADS, C1_THREADS, 0, stream>>>(slots, plan.P, n, g_w);
        VQAE_LAUNCH_CHECK();
    }
    return VQAE_OK;
}
