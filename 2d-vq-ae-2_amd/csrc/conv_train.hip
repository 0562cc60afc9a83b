// Trainable convolutions of a Fixup block as GEMMs over (gathered) rows (conv_block.py:196-216), fp32, NHWC, no bias, with the
// element-wise op in front of the conv folded in:
//     y [M][Co] = u [M][N] . w^T,    N = TAPS Ci columns, w [Co][N] k-contiguous against a row of u
//     pre = 0: u = x        pre = 1: u = x + *b        pre = 2: u = ELU(x + *a) + *b        (a, b read from DEVICE memory)
// u is never written to memory.  All products run on v_mfma_f32_32x32x2_f32.  ONE scheme serves three nodes, which differ in how
// a row of the activation operand is addressed (the policies Dense, Down2x2 and Circ3x3 below) and in nothing the kernels branch
// on at run time:
//
//   Dense    the 1x1, stride-1 conv (proj2d.yaml), vqae_conv1x1_train_*: M = B H W, TAPS = 1, row m starts at m Ci and column
//            k is at + k;  w [Co][Ci] as torch stores [Co, Ci, 1, 1].
//   Down2x2  the 2x2, stride-2 conv of a 'down' block (down2d.yaml: padding 0), vqae_conv_down_train_*: x [B][H][W][Ci], H and
//            W even, OH = H / 2, OW = W / 2, M = B OH OW, TAPS = 4.  The four taps do not overlap, so the conv is a GEMM over
//            gathered rows: row m = (b, oh, ow), column k = (kh, kw, ci) is u[b][2 oh + kh][2 ow + kw][ci].  For a fixed kh
//            the two kw pixels are neighbours in memory, so a row is two contiguous segments of 2 Ci floats, one image row apart:
//                address(m, k) = xbase(m) + (k / 2Ci) W Ci + k % 2Ci,     xbase(m) = ((m / OW) 4 OW + 2 (m % OW)) Ci
//            and a weight stored [Co][kh][kw][Ci] (a channels_last [Co, Ci, 2, 2] tensor) is k-contiguous against it.
//            w_layout 1 = [Co][2][2][Ci] is used as it lies; w_layout 0 = [Co][Ci][2][2] (contiguous) is permuted into the
//            workspace by ct_permute_w first (every call: the weight changes every step).  g_w is written in the layout the
//            weight has.
//   Circ3x3  the 3x3, stride-1 conv with circular padding 1 of a 'same' / 'out' block (same2d.yaml, out2d.yaml: branch_conv2),
//            vqae_conv3x3_train_*: x [B][H][W][Ci], any H, W >= 1, M = B H W, TAPS = 9: row m = (b, h, w), column
//            k = (kh, kw, ci) is u[b][(h + kh - 1) mod H][(w + kw - 1) mod W][ci].  Neither u nor a halo is written: the centre tap
//            of row m is at m Ci, a neighbour is (dh W + dw) Ci away with dh, dw in -1 .. 1 corrected by +-H, +-W at an image
//            edge -- two compare-and-selects per axis on the (h, w) a row keeps, no division per load.  w_layout 1 =
//            [Co][3][3][Ci] as it lies, w_layout 0 = [Co][Ci][3][3] through ct_permute_w.  The taps OVERLAP, so the data
//            gradient cannot scatter without atomics: it is the same gather applied to g,
//                g_u[b][h][w][ci] = sum_{kh,kw,co} g[b][(h + kh - 1) mod H][(w + kw - 1) mod W][co] wt[ci][kh][kw][co],
//                wt[ci][kh][kw][co] = w[co][ci][2 - kh][2 - kw]   (ct_flip_w, from either layout, every call),
//            i.e. the forward's loop with K = 9 Co, N = Ci, followed by Dense's epilogue (g_u [M][Ci] lies densely).
//
// Three kernels, all shape-generic (Ci, Co multiples of 8 up to 256, any M; in the M, K and N tails the operands are zero and
// the stores range-checked; templates choose tile COUNTS, never a shape).  The backward is two launches -- data gradient, then
// weight gradient -- not one: a fused form would hold a Co x N accumulator next to the 128 x N one of the data gradient
// (at 256 x 256 that is 64 K + 32 K floats per workgroup, more than the register file of a CU), and either output may be
// NULL.  The price is that g and x are read twice.
//
//   ct_gemm<.., BWD = false>   forward.   A workgroup of 4 waves owns 128 rows x all Co columns (wave = 32 rows x NT 32-column
//                        tiles, NT = 1 / 2 / 4 / 8 by Co), K = N walked in chunks of 32: the x chunk is staged to LDS with the
//                        pre-op applied ONCE per element (fp32 MFMA and VALU do not co-execute, so no expm1f in the MFMA loop),
//                        the w chunk next to it; both k-contiguous, row stride 36 floats: a lane reads 4 consecutive k of its
//                        row with one 128-bit LDS read and feeds 4 MFMAs (the same k permutation on both operands).  The row
//                        bases of a tile are computed once per tile (Down2x2: one 64-bit division per thread; Circ3x3: two,
//                        and two 32-bit ones per further row).
//   ct_gemm<.., BWD = true>    data gradient  g_u [M][N] = g [M][Co] . w [Co][N], the same loop with A = g, K = Co and w staged
//                        TRANSPOSED (w [k][n] is n-contiguous), in pieces of at most 256 columns (blockIdx.y; a piece is 32 NT
//                        columns, NT from min(N, 256); Dense has one piece).  The epilogue writes column n of row m to the
//                        input element it came from: g_x = g_u * ELU'(x + *a) (ELU'(v) = v > 0 ? 1 : exp(v)) with x read
//                        there.  (m, n) -> element is one to one and onto (Down2x2: H, W even): every element of g_x is
//                        written exactly once, by a plain store.  fp64 sums of g_x and g_u per thread in a fixed order.
//                        (Circ3x3: the gather form above, w = wt staged as in the forward, the same epilogue at dense
//                        addresses.)  Both forms load the next chunk into registers while the MFMAs of the current one run.
//   ct_wgrad<Addr, ..>   weight gradient  g_w [co][n] = sum_m g[m][co] u[m][n], u recomputed from x.  Grid (P, output tiles of
//                        up to 64 co x 64 n).  Rows are cut into blocks of 64; workgroup p takes blocks p, p + P, ...; its four
//                        waves split the rows of a block and each accumulates the whole tile in fp32, operands straight from
//                        global memory (lane = channel, the MFMA's own layout), one block of loads ahead.  After a run of
//                        CT_RUN = 512 rows the waves' sums are added in wave order and the run goes into the workgroup's OWN
//                        fp64 slot of the workspace (plain store on the first run: the workspace needs no clearing, nobody
//                        else touches the slot).  ct_wgrad_final adds the P slots in index order in fp64, rounds to fp32 once
//                        and writes the weight's layout.
//
// Determinism: every grid is a function of the shape (M or B, H, W; Ci, Co) alone, there are no floating-point atomics, every
// sum has one fixed order: two runs give the same bits.  The scalar sums follow fixup_train.hip: thread (fp64, index order) ->
// wave shuffle -> 4 waves in order -> one fp64 row per workgroup and piece -> ct_sum_final (one workgroup, fixed order, one
// rounding).
//
// Workspace: P slots of N Co doubles with P <= 256 and P N Co <= Addr::SLOT_ELEMS + 1024 Addr::MAX_PIECES rows of two doubles
// for the scalar sums + 256 bytes of slack.  Dense: [slots][partials], 2^20 slot elements: at most 8 MiB of slots whatever M
// is.  Down2x2: [permuted weight, 16-byte aligned][slots][partials]: the weight (4 Ci Co floats, at most 1 MiB) + 2^21 slot
// elements (at most 16 MiB) + 4096 rows: below 17.2 MiB in all.  Circ3x3: [permuted weight][flipped weight][slots][partials]:
// two weights of 9 Ci Co floats (at most 2.25 MiB each) + 2^22 slot elements (at most 32 MiB; one slot of 9 Ci Co doubles is at
// most 4.5 MiB, so P >= 7) + 1024 rows: below 36.6 MiB in all.
#include <algorithm>

#include "kernels.h"
#include "mfma.h"

namespace {

using namespace vqae;

constexpr int CT_THREADS = 256;
constexpr int CT_BM = 128;               // rows of a forward / data-gradient workgroup tile
constexpr int CT_KC = 32;                // k chunk staged per step
constexpr int CT_LD = CT_KC + 4;         // LDS row stride in floats: 16-byte aligned rows, 128-bit reads of 16 lanes hit all banks
constexpr int CT_MAX_WG = 1024;          // workgroups of ct_gemm per piece = rows of fp64 partials of the scalar sums per piece
constexpr int CT_RUN = 512;              // longest fp32 accumulation run of g_w, in rows
constexpr int CT_WM = 64;                // rows of a ct_wgrad block
constexpr int CT_PG = 8;                 // row pairs a ct_wgrad wave loads ahead of its MFMAs
constexpr int CT_SLOTS = 256;            // P <= CT_SLOTS and P N Co <= Addr::SLOT_ELEMS (P >= 1)
constexpr int CT_MAXC = 256;

// ---- the three addressings of the activation operand -------------------------------------------------------------------------
// Geo: what a policy needs of the image: W is the length of a line of rows (Down2x2: OW; Circ3x3: W), H the lines per image
// (Circ3x3 alone).  Row: the position of a row m;  row_ref(p, d): what ct_gemm keeps of the row d >= 0 (small) after p;
// col_off(n): column n inside a row;  at(r, c): the offset of column c of row r -- r + c, except at an image edge of Circ3x3;
// x_ptr(x, p, d, c): the element at column c of row d after p, for ct_wgrad's per-lane loads.  row_base(p, d), SUMS_ROW_OUTER
// and MAX_PIECES serve the data gradient's epilogue, which writes one element per (row, column): Dense and Down2x2.
struct Geo { int H, W; };

struct Dense {
    static constexpr int TAPS = 1;                        // columns of the operand per input channel
    static constexpr int MAX_PIECES = 1;                  // data gradient: N = Ci <= 256 is one piece
    static constexpr bool SUMS_ROW_OUTER = false;         // data gradient's per-thread sums walk tile t outer, row r inner
    static constexpr int64_t SLOT_ELEMS = 1 << 20;        // at most 8 MiB of fp64 partials
    static constexpr bool KEEPS_ROW_BASES = false;        // ct_gemm: a row base is one multiply, recomputed per chunk
    static constexpr bool GATHERS_GRAD = false;           // data gradient: column n of row m IS one element of g_x
    using Col = int;
    using RowRef = int64_t;
    struct Row { int64_t m; };
    static __device__ __forceinline__ int64_t row_stride(Geo, int) { return 0; }
    static __device__ __forceinline__ Row row_pos(int64_t m, Geo) { return Row{m}; }
    static __device__ __forceinline__ int64_t row_base(Row p, int64_t d, Geo, int Ci) { return (p.m + d) * Ci; }
    static __device__ __forceinline__ RowRef row_ref(Row p, int64_t d, Geo g, int Ci) { return row_base(p, d, g, Ci); }
    static __device__ __forceinline__ Col col_off(int n, int, int64_t) { return n; }
    static __device__ __forceinline__ int64_t at(RowRef r, Col c, Geo, int) { return r + c; }
    // one 64-bit base per block (uniform), 32-bit offsets per load
    static __device__ __forceinline__ const float* x_ptr(const float* x, Row p, unsigned d, Col c, Geo, int Ci) {
        return x + p.m * Ci + (d * (unsigned)Ci + (unsigned)c);
    }
};

struct Down2x2 {
    static constexpr int TAPS = 4;
    static constexpr int MAX_PIECES = 4;                  // data gradient: N = 4 Ci <= 4 * 256 in pieces of 256 columns
    static constexpr bool SUMS_ROW_OUTER = true;          // row r outer, tile t inner
    static constexpr int64_t SLOT_ELEMS = 1 << 21;        // at most 16 MiB of fp64 partials
    static constexpr bool KEEPS_ROW_BASES = true;         // ct_gemm: a row base costs a division, kept in registers per tile
    static constexpr bool GATHERS_GRAD = false;
    using Col = int64_t;
    using RowRef = int64_t;
    static __device__ __forceinline__ int64_t row_stride(Geo g, int Ci) { return (int64_t)2 * g.W * Ci; }      // W Ci
    // Row m = q OW + ow (q = b OH + oh: input row pair 2 q, 2 q + 1 of the [B H][W][Ci] array) -> offset of pixel (2 q, 2 ow).
    struct Row { int64_t q; unsigned ow; };
    static __device__ __forceinline__ Row row_pos(int64_t m, Geo g) {
        Row p;
        p.q = m / g.W;
        p.ow = (unsigned)(m - p.q * g.W);
        return p;
    }
    static __device__ __forceinline__ int64_t row_base(Row p, unsigned d, Geo g, int Ci) {
        const unsigned t = p.ow + d, dq = t / (unsigned)g.W, ow = t - dq * (unsigned)g.W;
        return ((p.q + dq) * 4 * g.W + 2 * (int64_t)ow) * Ci;
    }
    static __device__ __forceinline__ RowRef row_ref(Row p, unsigned d, Geo g, int Ci) { return row_base(p, d, g, Ci); }
    // column n = (kh, kw, ci) of [0, 4 Ci) inside a row's 2 x 2 window;  row_stride = W Ci
    static __device__ __forceinline__ Col col_off(int n, int Ci, int64_t row_stride) {
        const int kh = n >= 2 * Ci ? 1 : 0;
        return kh * row_stride + (n - kh * 2 * Ci);
    }
    static __device__ __forceinline__ int64_t at(RowRef r, Col c, Geo, int) { return r + c; }
    static __device__ __forceinline__ const float* x_ptr(const float* x, Row p, unsigned d, Col c, Geo g, int Ci) {
        return x + row_base(p, d, g, Ci) + c;
    }
};

// The 3x3, stride-1 conv with circular padding 1: row m = (b, h, w) of [B][H][W][C], column (kh, kw, c) is the pixel
// ((h + kh - 1) mod H, (w + kw - 1) mod W) of the same image.  The centre tap of row m is at m C; a neighbour is a whole number of
// pixels away, and WHICH number depends on the row at an image edge, so a row keeps (h, w) next to its base and the wrap is two
// compare-and-selects per axis in at().  For H = 1 (W = 1) all three kh (kw) land on the row itself, as F.pad(circular) has it.
struct Circ3x3 {
    static constexpr int TAPS = 9;
    static constexpr int MAX_PIECES = 1;                  // its data gradient is a gather that ends in Dense's epilogue
    static constexpr int64_t SLOT_ELEMS = 1 << 22;        // at most 32 MiB of fp64 partials
    static constexpr bool KEEPS_ROW_BASES = true;         // ct_gemm: (h, w) of a row cost divisions, kept in registers per tile
    static constexpr bool GATHERS_GRAD = true;            // nine columns of nine rows meet in one element: gather, never scatter
    struct Col { int dh, dw, c; };                        // tap (dh, dw) in -1 .. 1, channel c
    struct Row { int64_t m; unsigned h, w; };
    struct RowRef { int64_t base; int h, w; };
    static __device__ __forceinline__ int64_t row_stride(Geo, int) { return 0; }
    static __device__ __forceinline__ Row row_pos(int64_t m, Geo g) {
        const int64_t q = m / g.W;                        // b H + h
        Row p;
        p.m = m;
        p.w = (unsigned)(m - q * g.W);
        p.h = (unsigned)(q % g.H);
        return p;
    }
    // d rows on: 32-bit divisions (a tile may cross many image lines when W is small, and images when H W is)
    static __device__ __forceinline__ RowRef row_ref(Row p, unsigned d, Geo g, int C) {
        const unsigned t = p.w + d, dq = t / (unsigned)g.W, hq = p.h + dq;
        RowRef r;
        r.base = (p.m + d) * C;
        r.w = (int)(t - dq * (unsigned)g.W);
        r.h = (int)(hq % (unsigned)g.H);
        return r;
    }
    static __device__ __forceinline__ Col col_off(int n, int C, int64_t) {
        const int tap = n / C, kh = tap / 3;
        return Col{kh - 1, tap - 3 * kh - 1, n - tap * C};
    }
    static __device__ __forceinline__ int64_t at(RowRef r, Col c, Geo g, int C) {
        int h = r.h + c.dh, w = r.w + c.dw;
        h = h < 0 ? h + g.H : h;
        h = h >= g.H ? h - g.H : h;
        w = w < 0 ? w + g.W : w;
        w = w >= g.W ? w - g.W : w;
        return r.base + ((int64_t)(h - r.h) * g.W + (w - r.w)) * C + c.c;
    }
    static __device__ __forceinline__ const float* x_ptr(const float* x, Row p, unsigned d, Col c, Geo g, int C) {
        return x + at(row_ref(p, d, g, C), c, g, C);
    }
};

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

// w [Co][Ci][taps] -> wp [Co][taps][Ci]
__global__ __launch_bounds__(CT_THREADS)
void ct_permute_w(const float* __restrict__ w, int Ci, int taps, int n, float* __restrict__ wp) {
    const int i = blockIdx.x * CT_THREADS + threadIdx.x;
    if (i >= n) return;
    const int co = i / (taps * Ci), r = i - co * taps * Ci, tap = r / Ci, ci = r - tap * Ci;
    wp[i] = w[(int64_t)co * taps * Ci + ci * taps + tap];
}

// Circ3x3's data gradient is the same gather applied to g with the flipped, transposed weight:
// wt [Ci][3][3][Co],  wt[ci][kh][kw][co] = w[co][ci][2 - kh][2 - kw];  tap 3 kh + kw <- tap 8 - (3 kh + kw).  Either layout of w.
__global__ __launch_bounds__(CT_THREADS)
void ct_flip_w(const float* __restrict__ w, int Ci, int Co, int w_layout, int n, float* __restrict__ wt) {
    const int i = blockIdx.x * CT_THREADS + threadIdx.x;
    if (i >= n) return;
    const int ci = i / (9 * Co), r = i - ci * 9 * Co, tap = r / Co, co = r - tap * Co, src = 8 - tap;
    wt[i] = w[w_layout == 0 ? ((int64_t)co * Ci + ci) * 9 + src : ((int64_t)co * 9 + src) * Ci + ci];
}

// Three things vary, each a template argument: AA, how the rows of the A operand [M][K = AA::TAPS Ca] are addressed (Ca its
// channels per tap);  BWD, which epilogue runs;  WT, how w lies.
// BWD false:  out [M][N] = pre(A rows) . w^T, stored densely                                        (a forward: N = Co)
// BWD true:   g_x = (A rows . w) * ELU'(xe + a) at the addresses of EA (channels Ci), with the sums; no pre-op on A = g
// WT false:   w [N][K], k-contiguous against a row of A (one piece)
// WT true:    w [K][N], n-contiguous: staged transposed, in pieces of 32 NT columns, blockIdx.y * 32 NT the first of this piece
//   forward        <Addr, Dense, ., false, false>  K = TAPS Ci (EA is not used)
//   data gradient  <Dense, Addr, ., true, true>    Dense, Down2x2: A = g [M][Co] in dense rows, N = TAPS Ci columns scattered
//                                                  one to one onto x's elements
//                  <Circ3x3, Dense, ., true, false>  Circ3x3: the taps overlap, so g_u is GATHERED: the forward's loop over
//                                                  A = g with Ca = Co, K = 9 Co, w = ct_flip_w's wt [Ci][K], N = Ci dense columns
template <class AA, class EA, int NT, bool BWD, bool WT>
__global__ __launch_bounds__(CT_THREADS)
void ct_gemm(const float* __restrict__ A, const float* __restrict__ xe, const float* __restrict__ pa,
             const float* __restrict__ pb, int pre, const float* __restrict__ w, int64_t M, Geo geo, int Ca, int Ci, int K, int N,
             float* __restrict__ out, double* __restrict__ partials) {
    __shared__ __attribute__((aligned(16))) float Al[CT_BM * CT_LD];
    __shared__ __attribute__((aligned(16))) float Wl[NT * 32 * CT_LD];
    __shared__ double red[2][CT_THREADS / 64];
    constexpr bool KEEP = AA::KEEPS_ROW_BASES || (BWD && EA::KEEPS_ROW_BASES);    // a tile that pays a division anyway
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    const float a = pre == 2 ? *pa : 0.f, b = (!BWD && pre >= 1) ? *pb : 0.f;
    const int64_t n_tiles = (M + CT_BM - 1) / CT_BM;
    const int n0 = (WT && EA::MAX_PIECES > 1) ? (int)blockIdx.y * NT * 32 : 0;
    double s0 = 0.0, s1 = 0.0;
    // One chunk = 128 rows x 32 k of A (4 16-byte groups per thread, all with the same k) and NT * 32 columns x 32 k of w (NT
    // groups per thread), zero where a row, a column or k is out of range (Ci % 8 == 0, Co % 8 == 0: a group is in or out as a
    // whole, and lies inside one tap).  fetch() brings the NEXT chunk into registers while the MFMA loop runs on the current
    // one: branch-free loads, an out-of-range group reads the nearest valid address instead (no control flow between the loads
    // and the MFMA loop, so nothing waits for them there); commit() zeroes those groups, applies the pre-op and writes the
    // chunk to LDS.  rows() sets the offsets of this thread's four rows of a tile.
    constexpr int AG = CT_BM * (CT_KC / 4) / CT_THREADS;
    f32x4 ra[AG], rw[NT];
    typename AA::RowRef rb[AG];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    auto rows = [&](int64_t m0) __attribute__((always_inline)) {
        const int64_t mf = std::min(m0 + (tid >> 3), M - 1);
        const typename AA::Row p = AA::row_pos(mf, geo);
#pragma unroll
        for (int j = 0; j < AG; ++j) {
            const int64_t m = std::min(m0 + (tid >> 3) + 32 * j, M - 1);
            rb[j] = AA::row_ref(p, m - mf, geo, Ca);                       // 0 <= m - mf <= 96
        }
    };
    auto fetch = [&](int64_t m0, int k0, bool new_tile) __attribute__((always_inline)) {
        if (new_tile || !KEEP) rows(m0);
        const int k = std::min(k0 + 4 * (tid & 7), K - 4);
        const typename AA::Col ko = AA::col_off(k, Ca, AA::row_stride(geo, Ca));
#pragma unroll
        for (int j = 0; j < AG; ++j) ra[j] = *reinterpret_cast<const f32x4*>(A + AA::at(rb[j], ko, geo, Ca));
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int i = tid + j * CT_THREADS;
            if (!WT) {                   // w [n][k]: k-contiguous
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
            const int i = tid + j * CT_THREADS, k = k0 + 4 * (i & 7);
            const int64_t m = m0 + (i >> 3);
            f32x4 v = (m < M && k < K) ? ra[j] : zero4;
            if (!BWD && m < M && k < K) v = pre_op(v, pre, a, b);          // zero-filled elements stay zero
            *reinterpret_cast<f32x4*>(Al + (i >> 3) * CT_LD + 4 * (i & 7)) = v;
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int i = tid + j * CT_THREADS;
            if (!WT) {
                *reinterpret_cast<f32x4*>(Wl + (i >> 3) * CT_LD + 4 * (i & 7)) = ((i >> 3) < N && k0 + 4 * (i & 7) < K) ? rw[j] : zero4;
            } else {                     // transposed into the k-contiguous LDS rows
                const int kk = i / (NT * 8), n = 4 * (i % (NT * 8));
#pragma unroll
                for (int e = 0; e < 4; ++e) Wl[(n + e) * CT_LD + kk] = (k0 + kk < K && n0 + n < N) ? rw[j][e] : 0.f;
            }
        }
    };
    typename EA::Col co[NT];                             // data gradient: this lane's columns inside a row
    if (BWD) {
#pragma unroll
        for (int t = 0; t < NT; ++t) co[t] = EA::col_off(std::min(n0 + t * 32 + li, N - 1), Ci, EA::row_stride(geo, Ci));
    }
    if ((int64_t)blockIdx.x < n_tiles) fetch((int64_t)blockIdx.x * CT_BM, 0, true);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t m0 = tile * CT_BM;
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        for (int k0 = 0; k0 < K; k0 += CT_KC) {
            commit(m0, k0);
            __syncthreads();
            if (k0 + CT_KC < K) fetch(m0, k0 + CT_KC, false);
            else if (tile + gridDim.x < n_tiles) fetch((tile + gridDim.x) * CT_BM, 0, true);
            const int slices = std::min(CT_KC, K - k0) / 8;
            const float* ap = Al + (wave * 32 + li) * CT_LD + 4 * hh;
            const float* bp = Wl + li * CT_LD + 4 * hh;
            for (int u = 0; u < slices; ++u) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(ap + 8 * u);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const f32x4 bv = *reinterpret_cast<const f32x4*>(bp + t * 32 * CT_LD + 8 * u);
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
                const typename EA::Row p = EA::row_pos(mf, geo);
                // one element of the row at `base`; the order of the calls is the order of the fp64 sums, which defines the
                // bits of g_a and g_b
                auto element = [&](int t, int r, int64_t base) __attribute__((always_inline)) {
                    const int64_t e = base + co[t];
                    float v = acc[t][r];
                    s1 += (double)v;
                    if (pre == 2) v = v * elu_grad(xe[e] + a);
                    s0 += (double)v;
                    if (out) out[e] = v;
                };
                auto row_d = [](int r) __attribute__((always_inline)) { return (unsigned)(8 * (r >> 2) + (r & 3)); };
                if constexpr (EA::SUMS_ROW_OUTER) {    // the row's base (Down2x2: a division) once per row
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        if (mf + row_d(r) < M) {
                            const int64_t base = EA::row_base(p, row_d(r), geo, Ci);
#pragma unroll
                            for (int t = 0; t < NT; ++t)
                                if (n0 + t * 32 + li < N) element(t, r, base);
                        }
                    }
                } else {                                 // both guards at the element: with the column guard around the r
                                                         // loop the compiler holds all 16 row bases (scratch at NT = 8)
#pragma unroll
                    for (int t = 0; t < NT; ++t)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (n0 + t * 32 + li < N && mf + row_d(r) < M) element(t, r, EA::row_base(p, row_d(r), geo, Ci));
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
            const int64_t row = (WT && EA::MAX_PIECES > 1) ? (int64_t)blockIdx.y * gridDim.x + blockIdx.x : (int64_t)blockIdx.x;
            partials[row * 2 + 0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
            partials[row * 2 + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        }
    }
}

// One workgroup: thread t adds rows t, t + 256, ... in that order, then the wave / workgroup order of ct_gemm.
__global__ __launch_bounds__(CT_THREADS)
void ct_sum_final(const double* __restrict__ partials, int n_rows, float* __restrict__ o0, float* __restrict__ o1) {
    __shared__ double red[2][CT_THREADS / 64];
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < n_rows; i += CT_THREADS) {
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

// The output is Co x N (N = TAPS Ci), a tile (blockIdx.y) 32 NCO co x 32 NCN n.  Rows are cut into blocks of CT_WM = 64;
// workgroup p of the P of an output tile takes the blocks p, p + P, p + 2 P, ... in that order -- interleaved, so that at any
// moment the workgroups read neighbouring memory and not addresses a power of two apart.  The four waves split the ROWS of a
// block: wave w takes its row pairs w, w + 4, ..., w + 28 (lane (li, hh) row 2 pair + hh), reads its operands straight from
// global memory (lane = channel: 32 consecutive columns of a row per half-wave are one 128-byte segment, or two where they cross
// a tap pair of Down2x2) and accumulates the whole tile; no LDS, no barrier in the loop.  The loads of a block are issued one
// block ahead of its MFMAs.  After every CT_RUN / 64 = 8 blocks (one fp32 run) and at the end, the four accumulators are added
// in wave order through LDS, ((w0 + w1) + w2) + w3, and wave 3 adds the run into the workgroup's fp64 slot [co][n].
// PRE is a template argument so that the loop body is straight-line code: with a run-time branch per element the compiler
// sinks the early loads down to their uses and the latency is paid in full.
template <class Addr, int NCO, int NCN, int PRE>
__global__ __launch_bounds__(CT_THREADS)
void ct_wgrad(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ pa,
              const float* __restrict__ pb, int64_t M, Geo geo, int Ci, int Co, double* __restrict__ slots) {
    static_assert(CT_WM == 8 * CT_PG && CT_RUN % CT_WM == 0 && (CT_RUN / CT_WM) % 2 == 0, "a block is one load group per wave");
    __shared__ float red[NCO * NCN * 16 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
    const int N = Addr::TAPS * Ci;
    const int tiles_n = (N + 32 * NCN - 1) / (32 * NCN);
    const int co0 = (blockIdx.y / tiles_n) * 32 * NCO, n0 = (blockIdx.y % tiles_n) * 32 * NCN;
    const float a = PRE == 2 ? *pa : 0.f, b = PRE >= 1 ? *pb : 0.f;
    const int64_t n_blocks = (M + CT_WM - 1) / CT_WM;
    const int64_t row_stride = Addr::row_stride(geo, Ci);
    const int P = gridDim.x;
    int cg[NCO];                                          // this lane's channels / column offsets, clamped for the loads
    typename Addr::Col cx[NCN];
#pragma unroll
    for (int s = 0; s < NCO; ++s) cg[s] = std::min(co0 + 32 * s + li, Co - 1);
#pragma unroll
    for (int t = 0; t < NCN; ++t) cx[t] = Addr::col_off(std::min(n0 + 32 * t + li, N - 1), Ci, row_stride);
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
    float bg[2][CT_PG][NCO], bx[2][CT_PG][NCN];
    // first row of the workgroup's block number blk (uniform), and this lane's row inside a block for pair q of its wave
    auto base_of = [&](int blk) __attribute__((always_inline)) { return ((int64_t)blockIdx.x + (int64_t)blk * P) * CT_WM; };
    auto row_in = [&](int q) __attribute__((always_inline)) { return 2 * (wave + 4 * q) + hh; };
    // branch-free: a block past the end reads the last block, a row past the end row M - 1, a missing column the last one;
    // compute() zeroes them.
    auto fetch = [&](int blk, int buf) __attribute__((always_inline)) {
        const int64_t base = std::min(base_of(blk), (n_blocks - 1) * CT_WM);
        const int last = (int)std::min<int64_t>(CT_WM - 1, M - 1 - base);
        const float* gb = g + base * Co;
        const typename Addr::Row p = Addr::row_pos(base, geo);
#pragma unroll
        for (int q = 0; q < CT_PG; ++q) {
            const unsigned r = (unsigned)std::min(row_in(q), last);
#pragma unroll
            for (int s = 0; s < NCO; ++s) bg[buf][q][s] = gb[r * (unsigned)Co + (unsigned)cg[s]];
#pragma unroll
            for (int t = 0; t < NCN; ++t) bx[buf][q][t] = *Addr::x_ptr(x, p, r, cx[t], geo, Ci);
        }
    };
    auto compute = [&](int blk, int buf) __attribute__((always_inline)) {
        float u[CT_PG][NCN];
#pragma unroll
        for (int q = 0; q < CT_PG; ++q) {                 // all activations of the block first: independent chains
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
        for (int q = 0; q < CT_PG; ++q) {
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
        if ((blk + 2) % (CT_RUN / CT_WM) != 0 && blk + 2 < nb) continue;
        // end of an fp32 run: the four waves' sums in wave order; D [i = co][j = n]: lane holds n = li of sub-tile t, co rows
        // 8 (r / 4) + 4 hh + r % 4
        for (int wv = 0; wv < CT_THREADS / 64; ++wv) {
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
                            } else if (wv < CT_THREADS / 64 - 1) {
                                *rp = *rp + acc[s][t][r];
                            } else {
                                const float v = *rp + acc[s][t][r];
                                const int co = co0 + 32 * s + 8 * (r >> 2) + 4 * hh + (r & 3);
                                if (co < Co && n < N) {
                                    double* sp = slot + (int64_t)co * N + n;
                                    *sp = first ? (double)v : *sp + (double)v;
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

// slots [P][n], n = Co N elements in the kernels' order [Co][taps][Ci] -> g_w in the weight's own layout: w_layout 1 is that
// order (Dense always; [Co][2][2][Ci], [Co][3][3][Ci]), w_layout 0 is [Co][Ci][taps] (Down2x2: taps = 4, Circ3x3: 9).
__global__ __launch_bounds__(CT_THREADS)
void ct_wgrad_final(const double* __restrict__ slots, int P, int n, int Ci, int taps, int w_layout, float* __restrict__ g_w) {
    const int i = blockIdx.x * CT_THREADS + threadIdx.x;
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
        const int co = i / (taps * Ci), r = i - co * taps * Ci, tap = r / Ci, ci = r - tap * Ci;
        o = co * taps * Ci + ci * taps + tap;
    }
    g_w[o] = (float)s;
}

// ---- host: plans, the launch ladders, the backward all nodes share ----------------------------------------------------------
inline bool supported(int cin, int cout) {
    return cin >= 8 && cout >= 8 && cin <= CT_MAXC && cout <= CT_MAXC && cin % 8 == 0 && cout % 8 == 0;
}

struct WgradPlan { int P; int tiles; int nco; int ncn; };
template <class Addr>
inline WgradPlan wgrad_plan(int64_t m, int cin, int cout) {
    const int n = Addr::TAPS * cin;
    WgradPlan p;
    p.nco = cout <= 32 ? 1 : 2;                                        // output tile: 32 nco co x 32 ncn columns of n
    p.ncn = n <= 32 ? 1 : 2;
    p.tiles = (int)(ceil_div(cout, 32 * p.nco) * ceil_div(n, 32 * p.ncn));
    const int64_t pmax = std::min<int64_t>(CT_SLOTS, std::max<int64_t>(1, Addr::SLOT_ELEMS / ((int64_t)n * cout)));
    p.P = (int)std::min<int64_t>(pmax, ceil_div(m, CT_WM));          // every workgroup has at least one 64-row block
    return p;
}
template <class Addr>
inline size_t slots_and_partials_bytes(const WgradPlan& p, int cin, int cout) {
    return (size_t)p.P * Addr::TAPS * cin * cout * sizeof(double) + (size_t)CT_MAX_WG * Addr::MAX_PIECES * 2 * sizeof(double) + 256;
}

template <class AA, class EA, bool BWD, bool WT>
inline void launch_gemm(int nt, dim3 grid, hipStream_t stream, const float* A, const float* xe, const float* pa, const float* pb,
                        int pre, const float* w, int64_t M, Geo geo, int Ca, int Ci, int K, int N, float* out, double* partials) {
    if (nt == 1) ct_gemm<AA, EA, 1, BWD, WT><<<grid, CT_THREADS, 0, stream>>>(A, xe, pa, pb, pre, w, M, geo, Ca, Ci, K, N, out, partials);
    else if (nt == 2) ct_gemm<AA, EA, 2, BWD, WT><<<grid, CT_THREADS, 0, stream>>>(A, xe, pa, pb, pre, w, M, geo, Ca, Ci, K, N, out, partials);
    else if (nt == 4) ct_gemm<AA, EA, 4, BWD, WT><<<grid, CT_THREADS, 0, stream>>>(A, xe, pa, pb, pre, w, M, geo, Ca, Ci, K, N, out, partials);
    else ct_gemm<AA, EA, 8, BWD, WT><<<grid, CT_THREADS, 0, stream>>>(A, xe, pa, pb, pre, w, M, geo, Ca, Ci, K, N, out, partials);
}

template <class Addr, int NCO, int NCN>
inline void launch_wgrad_pre(int pre, dim3 grid, hipStream_t stream, const float* g, const float* x, const float* a, const float* b,
                             int64_t m, Geo geo, int cin, int cout, double* slots) {
    if (pre == 0) ct_wgrad<Addr, NCO, NCN, 0><<<grid, CT_THREADS, 0, stream>>>(g, x, a, b, m, geo, cin, cout, slots);
    else if (pre == 1) ct_wgrad<Addr, NCO, NCN, 1><<<grid, CT_THREADS, 0, stream>>>(g, x, a, b, m, geo, cin, cout, slots);
    else ct_wgrad<Addr, NCO, NCN, 2><<<grid, CT_THREADS, 0, stream>>>(g, x, a, b, m, geo, cin, cout, slots);
}

template <class Addr>
inline void launch_wgrad(int nco, int ncn, int pre, dim3 grid, hipStream_t stream, const float* g, const float* x, const float* a,
                         const float* b, int64_t m, Geo geo, int cin, int cout, double* slots) {
    if (nco == 1 && ncn == 1) launch_wgrad_pre<Addr, 1, 1>(pre, grid, stream, g, x, a, b, m, geo, cin, cout, slots);
    else if (nco == 1) launch_wgrad_pre<Addr, 1, 2>(pre, grid, stream, g, x, a, b, m, geo, cin, cout, slots);
    else if (ncn == 1) launch_wgrad_pre<Addr, 2, 1>(pre, grid, stream, g, x, a, b, m, geo, cin, cout, slots);
    else launch_wgrad_pre<Addr, 2, 2>(pre, grid, stream, g, x, a, b, m, geo, cin, cout, slots);
}

inline int tiles_for(int n) { return n <= 32 ? 1 : n <= 64 ? 2 : n <= 128 ? 4 : 8; }
inline int gemm_grid(int64_t m) { return (int)std::min<int64_t>(CT_MAX_WG, ceil_div(m, CT_BM)); }
inline int blocks_for(int n) { return (n + CT_THREADS - 1) / CT_THREADS; }

// w [Co][TAPS Ci]: k-contiguous against the operand's rows
template <class Addr>
inline int forward(const float* x, const float* a, const float* b, int pre, const float* w, int64_t m, Geo geo, int cin, int cout,
                   float* y, hipStream_t stream) {
    launch_gemm<Addr, Dense, false, false>(tiles_for(cout), dim3(gemm_grid(m)), stream, x, nullptr, a, b, pre, w, m, geo, cin, cin,
                                          Addr::TAPS * cin, cout, y, nullptr);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

// What a launch uses of the workspace (carve below).  wp: the weight of w_layout 0 in the k-contiguous order (ct_permute_w);
// wt: Circ3x3's flipped, transposed weight (ct_flip_w).
struct Workspace { float* wp; float* wt; double* slots; double* partials; };

// w is k-contiguous against the operand's rows unless w_layout == 0.  The scattering data gradient (Dense, Down2x2) then reads
// ct_permute_w's copy in wk.wp; the gathering one (Circ3x3) reads ct_flip_w's wk.wt, made from either layout.
template <class Addr>
inline int backward(const float* g, const float* x, const float* a, const float* b, int pre, const float* w, int w_layout,
                    const Workspace& wk, const WgradPlan& plan, int64_t m, Geo geo, int cin, int cout, float* g_x, float* g_w,
                    float* g_a, float* g_b, hipStream_t stream) {
    const int n_all = Addr::TAPS * cin;
    float* o_a = pre == 2 ? g_a : nullptr;
    float* o_b = pre >= 1 ? g_b : nullptr;
    if (g_x || o_a || o_b) {
        dim3 grid(gemm_grid(m));
        if constexpr (Addr::GATHERS_GRAD) {
            ct_flip_w<<<blocks_for(n_all * cout), CT_THREADS, 0, stream>>>(w, cin, cout, w_layout, n_all * cout, wk.wt);
            VQAE_LAUNCH_CHECK();
            launch_gemm<Addr, Dense, true, false>(tiles_for(cin), grid, stream, g, x, a, b, pre, wk.wt, m, geo, cout, cin,
                                                  Addr::TAPS * cout, cin, g_x, wk.partials);
        } else {
            if (w_layout == 0) {
                ct_permute_w<<<blocks_for(n_all * cout), CT_THREADS, 0, stream>>>(w, cin, Addr::TAPS, n_all * cout, wk.wp);
                VQAE_LAUNCH_CHECK();
            }
            const int nt = tiles_for(std::min(n_all, 256));
            grid.y = (unsigned)ceil_div(n_all, 32 * nt);
            launch_gemm<Dense, Addr, true, true>(nt, grid, stream, g, x, a, b, pre, w_layout == 0 ? wk.wp : w, m, geo, cout, cin,
                                                 cout, n_all, g_x, wk.partials);
        }
        VQAE_LAUNCH_CHECK();
        if (o_a || o_b) {
            ct_sum_final<<<1, CT_THREADS, 0, stream>>>(wk.partials, (int)(grid.x * grid.y), o_a, o_b);
            VQAE_LAUNCH_CHECK();
        }
    }
    if (g_w) {
        const dim3 grid(plan.P, plan.tiles);
        launch_wgrad<Addr>(plan.nco, plan.ncn, pre, grid, stream, g, x, a, b, m, geo, cin, cout, wk.slots);
        VQAE_LAUNCH_CHECK();
        const int n = n_all * cout;
        ct_wgrad_final<<<blocks_for(n), CT_THREADS, 0, stream>>>(wk.slots, plan.P, n, cin, Addr::TAPS, w_layout, g_w);
        VQAE_LAUNCH_CHECK();
    }
    return VQAE_OK;
}

// ---- host: the nodes ---------------------------------------------------------------------------------------------------------
// What the C ABI states of a node, once: its policy, its name in messages, its stride (rows M = batch (h / STRIDE) (w / STRIDE);
// h and w must be multiples of it), the Geo its kernels take, and whether it is called with an image (batch, h, w), a weight
// layout and a forward workspace -- or, Dense, with M rows as given, its weight always k-contiguous.  WEIGHT_COPIES: the weights
// (of round_up(TAPS Ci Co floats, 256) bytes each) in front of [slots][partials] in the workspace, wp then wt; with any, the
// workspace starts at the next 16-byte boundary, with none at the pointer as given.
struct Conv1x1 {
    using Addr = Dense;
    static constexpr const char* NAME = "conv1x1_train";
    static constexpr int STRIDE = 1, WEIGHT_COPIES = 0;
    static constexpr bool IMAGE = false;
    static Geo geo(int, int) { return Geo{0, 0}; }
};
struct ConvDown {
    using Addr = Down2x2;
    static constexpr const char* NAME = "conv_down_train";
    static constexpr int STRIDE = 2, WEIGHT_COPIES = 1;
    static constexpr bool IMAGE = true;
    static Geo geo(int, int w) { return Geo{0, w / 2}; }
};
struct Conv3x3 {
    using Addr = Circ3x3;
    static constexpr const char* NAME = "conv3x3_train";
    static constexpr int STRIDE = 1, WEIGHT_COPIES = 2;
    static constexpr bool IMAGE = true;
    static Geo geo(int h, int w) { return Geo{h, w}; }
};

// rows M when the geometry is valid and M < 2^40, else 0
template <class Node>
inline int64_t rows(int64_t b, int h, int w) {
    if (b < 1 || h < 1 || w < 1 || h % Node::STRIDE || w % Node::STRIDE) return 0;
    const int64_t per = (int64_t)(h / Node::STRIDE) * (w / Node::STRIDE);              // >= 1, < 2^62
    return per < (1ll << 40) && b <= (1ll << 40) / per && b * per < (1ll << 40) ? b * per : 0;
}

template <class Node>
inline size_t weight_bytes(int cin, int cout) {
    return (size_t)round_up((int64_t)Node::Addr::TAPS * cin * cout * sizeof(float), 256);
}
template <class Node>
inline Workspace carve(void* ws, const WgradPlan& plan, int cin, int cout) {
    char* p = (char*)ws;
    if (Node::WEIGHT_COPIES) p = (char*)(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    Workspace o;
    o.wp = (float*)p;
    o.wt = Node::WEIGHT_COPIES > 1 ? (float*)(p + weight_bytes<Node>(cin, cout)) : nullptr;
    o.slots = (double*)(p + Node::WEIGHT_COPIES * weight_bytes<Node>(cin, cout));
    o.partials = o.slots + (size_t)plan.P * Node::Addr::TAPS * cin * cout;
    return o;
}

template <class Node>
inline size_t entry_workspace_bytes(int64_t b, int h, int w, int cin, int cout) {
    const int64_t m = Node::IMAGE ? rows<Node>(b, h, w) : b;                          // rows as given have a size past 2^40 too
    if (m < 1 || !supported(cin, cout)) return 0;
    return Node::WEIGHT_COPIES * weight_bytes<Node>(cin, cout)
           + slots_and_partials_bytes<typename Node::Addr>(wgrad_plan<typename Node::Addr>(m, cin, cout), cin, cout);
}

// The checks both entries share, in the order that decides which code a call with two faults returns; *m: the rows.  A node
// without an image passes its rows as batch, h = w = 1 and w_layout = 1.
template <class Node>
inline int entry_checks(const char* op, bool pointers, int pre, int w_layout, const float* a, const float* b, int64_t batch, int h,
                        int wd, int cin, int cout, int64_t* m) {
    *m = rows<Node>(batch, h, wd);
    if (Node::IMAGE)
        VQAE_REQUIRE(batch >= 1 && h >= 1 && wd >= 1, VQAE_ERR_INVALID, "%s_%s: batch %lld h %d w %d", Node::NAME, op,
                     (long long)batch, h, wd);
    else
        VQAE_REQUIRE(*m >= 1, VQAE_ERR_INVALID, "%s_%s: %lld rows", Node::NAME, op, (long long)batch);
    VQAE_REQUIRE(pre >= 0 && pre <= 2, VQAE_ERR_INVALID, "%s_%s: pre %d", Node::NAME, op, pre);
    VQAE_REQUIRE(w_layout >= 0 && w_layout <= 1, VQAE_ERR_INVALID, "%s_%s: w_layout %d", Node::NAME, op, w_layout);
    VQAE_REQUIRE(pointers && (pre < 1 || b) && (pre < 2 || a), VQAE_ERR_INVALID, "%s_%s: null pointer", Node::NAME, op);
    VQAE_REQUIRE(supported(cin, cout), VQAE_ERR_UNSUPPORTED, "%s_%s: cin %d cout %d (multiples of 8, 8 .. %d)", Node::NAME, op, cin,
                 cout, CT_MAXC);
    VQAE_REQUIRE(h % Node::STRIDE == 0 && wd % Node::STRIDE == 0, VQAE_ERR_UNSUPPORTED, "%s_%s: h %d w %d must be even",
                 Node::NAME, op, h, wd);
    VQAE_REQUIRE(*m >= 1, VQAE_ERR_INVALID, "%s_%s: batch %lld x %d x %d %srows exceed 2^40", Node::NAME, op, (long long)batch,
                 h / Node::STRIDE, wd / Node::STRIDE, Node::STRIDE > 1 ? "output " : "");
    return VQAE_OK;
}

// the forward uses the workspace for w_layout 0 only
template <class Node>
inline int entry_forward(const float* x, const float* a, const float* b, int pre, const float* w, int w_layout, int64_t batch,
                         int h, int wd, int cin, int cout, float* y, void* ws, void* stream_) {
    using Addr = typename Node::Addr;
    hipStream_t stream = (hipStream_t)stream_;
    int64_t m;
    if (const int e = entry_checks<Node>("forward", x && w && y && (ws || w_layout == 1), pre, w_layout, a, b, batch, h, wd, cin,
                                         cout, &m))
        return e;
    VQAE_REQUIRE(aligned16({x, w, y}) && ((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID,
                 Node::IMAGE ? "%s_forward: x, w and y must be 16-byte aligned, the workspace 8-byte aligned"
                             : "%s_forward: x, w and y must be 16-byte aligned", Node::NAME);
    if (w_layout == 0) {
        const Workspace wk = carve<Node>(ws, wgrad_plan<Addr>(m, cin, cout), cin, cout);
        const int n = Addr::TAPS * cin * cout;
        ct_permute_w<<<blocks_for(n), CT_THREADS, 0, stream>>>(w, cin, Addr::TAPS, n, wk.wp);
        VQAE_LAUNCH_CHECK();
        w = wk.wp;
    }
    return forward<Addr>(x, a, b, pre, w, m, Node::geo(h, wd), cin, cout, y, stream);
}

template <class Node>
inline int entry_backward(const float* g, const float* x, const float* a, const float* b, int pre, const float* w, int w_layout,
                          int64_t batch, int h, int wd, int cin, int cout, float* g_x, float* g_w, float* g_a, float* g_b,
                          void* ws, void* stream_) {
    using Addr = typename Node::Addr;
    int64_t m;
    if (const int e = entry_checks<Node>("backward", g && x && w && ws, pre, w_layout, a, b, batch, h, wd, cin, cout, &m)) return e;
    VQAE_REQUIRE(aligned16({g, x, w, g_x, g_w}) && ((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID,
                 "%s_backward: tensors must be 16-byte aligned, the workspace 8-byte aligned", Node::NAME);
    const WgradPlan plan = wgrad_plan<Addr>(m, cin, cout);
    return backward<Addr>(g, x, a, b, pre, w, w_layout, carve<Node>(ws, plan, cin, cout), plan, m, Node::geo(h, wd), cin, cout, g_x,
                          g_w, g_a, g_b, (hipStream_t)stream_);
}

}  // namespace

// ---- kernels.h: the two final-sum launches, for conv_train_thin.hip ---------------------------------------------------------
int vqae::conv_train_sum_final(const double* partials, int n_rows, float* o0, float* o1, hipStream_t stream) {
    ct_sum_final<<<1, CT_THREADS, 0, stream>>>(partials, n_rows, o0, o1);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}
int vqae::conv_train_wgrad_final(const double* slots, int P, int n, int cin, int taps, int w_layout, float* g_w,
                                 hipStream_t stream) {
    ct_wgrad_final<<<blocks_for(n), CT_THREADS, 0, stream>>>(slots, P, n, cin, taps, w_layout, g_w);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

// ---- the C ABI ---------------------------------------------------------------------------------------------------------------
// the 1x1, stride-1 node
extern "C" int vqae_conv1x1_train_supported(int cin, int cout) { return supported(cin, cout) ? 1 : 0; }
extern "C" int vqae_conv1x1_train_wgrad_run(void) { return CT_RUN; }
extern "C" size_t vqae_conv1x1_train_workspace_bytes(int64_t m, int cin, int cout) {
    return entry_workspace_bytes<Conv1x1>(m, 1, 1, cin, cout);
}
extern "C" int vqae_conv1x1_train_forward_f32(const float* x, const float* a, const float* b, int pre, const float* w, int64_t m,
                                              int cin, int cout, float* y, void* stream) {
    return entry_forward<Conv1x1>(x, a, b, pre, w, 1, m, 1, 1, cin, cout, y, nullptr, stream);
}
extern "C" int vqae_conv1x1_train_backward_f32(const float* g, const float* x, const float* a, const float* b, int pre,
                                               const float* w, int64_t m, int cin, int cout, float* g_x, float* g_w, float* g_a,
                                               float* g_b, void* ws, void* stream) {
    return entry_backward<Conv1x1>(g, x, a, b, pre, w, 1, m, 1, 1, cin, cout, g_x, g_w, g_a, g_b, ws, stream);
}

// the 2x2, stride-2 node
extern "C" int vqae_conv_down_train_supported(int cin, int cout) { return supported(cin, cout) ? 1 : 0; }
extern "C" int vqae_conv_down_train_wgrad_run(void) { return CT_RUN; }
extern "C" size_t vqae_conv_down_train_workspace_bytes(int64_t b, int h, int w, int cin, int cout) {
    return entry_workspace_bytes<ConvDown>(b, h, w, cin, cout);
}
extern "C" int vqae_conv_down_train_forward_f32(const float* x, const float* a, const float* b, int pre, const float* w,
                                                int w_layout, int64_t batch, int h, int wd, int cin, int cout, float* y, void* ws,
                                                void* stream) {
    return entry_forward<ConvDown>(x, a, b, pre, w, w_layout, batch, h, wd, cin, cout, y, ws, stream);
}
extern "C" int vqae_conv_down_train_backward_f32(const float* g, const float* x, const float* a, const float* b, int pre,
                                                 const float* w, int w_layout, int64_t batch, int h, int wd, int cin, int cout,
                                                 float* g_x, float* g_w, float* g_a, float* g_b, void* ws, void* stream) {
    return entry_backward<ConvDown>(g, x, a, b, pre, w, w_layout, batch, h, wd, cin, cout, g_x, g_w, g_a, g_b, ws, stream);
}

// the circular 3x3, stride-1 node
extern "C" int vqae_conv3x3_train_supported(int cin, int cout) { return supported(cin, cout) ? 1 : 0; }
extern "C" int vqae_conv3x3_train_wgrad_run(void) { return CT_RUN; }
extern "C" size_t vqae_conv3x3_train_workspace_bytes(int64_t b, int h, int w, int cin, int cout) {
    return entry_workspace_bytes<Conv3x3>(b, h, w, cin, cout);
}
extern "C" int vqae_conv3x3_train_forward_f32(const float* x, const float* a, const float* b, int pre, const float* w, int w_layout,
                                              int64_t batch, int h, int wd, int cin, int cout, float* y, void* ws, void* stream) {
    return entry_forward<Conv3x3>(x, a, b, pre, w, w_layout, batch, h, wd, cin, cout, y, ws, stream);
}
extern "C" int vqae_conv3x3_train_backward_f32(const float* g, const float* x, const float* a, const float* b, int pre,
                                               const float* w, int w_layout, int64_t batch, int h, int wd, int cin, int cout,
                                               float* g_x, float* g_w, float* g_a, float* g_b, void* ws, void* stream) {
    return entry_backward<Conv3x3>(g, x, a, b, pre, w, w_layout, batch, h, wd, cin, cout, g_x, g_w, g_a, g_b, ws, stream);
}
