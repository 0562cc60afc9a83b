// Winograd F(4x4, 3x3) form of the C = 128 trunk Fixup block on the 32-wide code grid, fp32 (round 3):
//   conv2 (3x3 circular, conv_block.py:208)  as  Y = A^T [ sum_c (G g G^T) .* (B^T d B) ] A   on 6 x 6 input / 4 x 4 output tiles,
// followed in the same workgroup by conv3 (+ scale / bias4 / residual) and the NEXT block's conv1 -- the contract of
// wino_trunk_kernel (conv_wino.hip), whose 1x1 tails this kernel repeats on two 128-pixel halves.
//
// Why: on gfx950 the fp32 matrix instruction runs at the vector rate and does not co-execute with vector work, so the trunk
// kernel is bound by MFMA + VALU issue cycles.  F(4x4, 3x3) needs 36 multiplies per 16 outputs and channel pair
// (2.25 per output) where F(2x2, 3x3) needs 4: conv2's matrix work drops 1.78x, the block's (conv2 + two 1x1) 1.41x, for ~1.3x the
// transform / fold vector work.  The price is numerical: B^T / A^T carry entries up to 8, and the fp32 result is ~4x further
// from the exact value than the direct form (5e-7 instead of 1.4e-7 of the feature range through the 68-block encoder;
// tools/dbg/wino43_numerics.py) -- indices stay bit-exact on every fixture.  VQAE_WINO43=0 keeps F(2x2, 3x3).
//
// Work split.  A 256-thread workgroup owns 8 image rows x 32 columns = 256 output pixels = 16 tiles (2 tile rows x 8 tile
// columns).  A wave owns 32 output channels (two 16-channel MFMA row blocks) x all 16 tiles, on v_mfma_f32_16x16x4_f32 with the
// weights as the ROW operand: lane (li, q) receives tile li, channels 4 q .. 4 q + 3 of each block -- four consecutive channels,
// so every LDS / global access of the epilogue is 128 bits wide.  The 6 x 6 transformed domain is walked one row xi at a time:
//   transform  V_xi[nu][tile][c] = (B^T d B)[xi][nu], nu = 0..5, all 128 channels -> LDS (6 x 16 x 132 floats); thread = (tile column,
//              channel quad), two tile rows; input rows straight from global / L2 in batches of 2 columns, two batches in flight
//   GEMM       acc (2 blocks x 4 registers) = U[xi, nu] (32 ch x 128) x V_xi[nu] (128 x 16 tiles): one ds_read_b128 + two 1 KiB
//              weight-fragment loads feed 8 MFMAs
//   fold       Z[b] += A^T[b][nu] acc  (pairs nu = 1, 2 and 3, 4 share their sum / difference);  after nu = 5:  Y[a][b] += A^T[a][xi] Z[b]
// Live: Y 128 + Z 32 + 2 x 8 accumulator registers.  The passes xi = 1..4 share one loop body (their row combinations
// d4 + c1 d1 + c2 d2 + c3 d3 and folds Y_a += a_a Z differ in coefficients only); xi = 0 and 5 are specialised (three rows, one Y row).
// Tails: output rows {0, 1} of every tile (image rows {0, 1, 4, 5} of the 8) form the first 128-pixel half, rows {2, 3} the second;
// each half is t2 -> LDS [128 px][132], conv3, epilogue, next conv1 exactly as in wino_trunk_kernel.
// Split form (SPLIT, the default at C = 128; VQAE_W43_SPLIT=0 keeps the above): the same walk with every GEMM on the bf16 MFMA, each fp32
// operand as three bf16 pieces and six of their nine products.
// The same kernel serves the level above the trunk (C = 64 on the 64-wide grid: 2 slices x 2 tile groups) and C = 256 on the code
// grid (8 slices, 512 threads, one workgroup per CU).
// Wide form (WIDE: the split form at C = 128 when H % 16 == 0): one 512-thread workgroup per CU owns 16 image rows = two 8-row bands =
// 32 tiles.  Wave cb = 0..7 owns ONE 16-channel block and both bands: the block index of Y / Z / acc becomes the band index, and every
// weight fragment a wave loads (one per plane and chunk: 16 registers double-buffered, where the 8-row form has 32 single-buffered for
// two blocks) feeds both bands' V fragments, so the weight stream per CU and position is 96 KiB instead of 2 x 96 KiB.  Every
// accumulator sees the MFMAs of the 8-row form in their order: the results are that form's bit for bit (tests/test_wino43_wide_gpu.py).
// V is [nu][32 tiles][3 C + 8] bf16 = 150 528 B, T [256 px][132] fp32 overlays it; both exceed the 64 KiB a DS offset field
// reaches, hence the second, opaque bases.  H % 8 == 0 only, VQAE_W43_SPLIT=0, C = 64 and C = 256 keep the 8-row kernels.
// Wide transform: every input column once per pass.  Neighbouring tile columns share two of their six input columns, and the 8-row
// transform (thread = tile column x channel quad, six columns each) fetches both copies from L2.  In the wide form a wave holds all
// eight tile columns of a band for 32 channels (lane = 8 tile column + quad), a thread loads columns 4 t - 1 .. 4 t + 2 only (four
// batches of 2 columns per pass instead of six, two in flight) and, after the row combination, takes columns 4 t + 3, 4 t + 4 from the
// lane 8 further on (ds_bpermute_b32, 8 dwords per tile row; the rotation over the wave is the wrap in x): the neighbour formed them
// from the same raw values through the same fma chain, so V is bit for bit what it was.  V slots are permuted within a band
// (4 (t & 3) + 2 (t >> 2) + tile row) to keep the transform's ds_write_b64 free of bank conflicts under the new lane order; the GEMM
// reads slot li, the tails map li back to (tile row, tile column).  tests/test_wino43_columns_gpu.py; DESIGN.md section 8.
#include "kernels.h"
#include "mfma.h"

namespace {

using namespace vqae;

struct W43K {
    const float* __restrict__ t1;        // [M][C] conv2 input
    const float* __restrict__ U;         // G g G^T, [36 pos][C / 32 slices][C / 16 k-groups][2 blocks][64 lanes][4]
    const float* __restrict__ w3;        // [C][C], fragment order (frag_offset, k-slice 8)
    const float* __restrict__ w1n;       // same, the next block's conv1 (TAIL == 2)
    float* xio;                          // [M][C] residual stream, updated in place
    float* y2;                           // [M][C] next block's t1 (TAIL == 2)
    // split form (SPLIT): the same weights as three bf16 planes, hi + mid + lo (wino43_split_weight_kernel / split_1x1_kernel)
    const float* __restrict__ Us;        // [36 pos][C / 32 slices][C / 32 chunks][2 blocks][3 planes][64 lanes][8 bf16]
    const float* __restrict__ w3s;       // [C / 32 blocks][C / 16 k-slices][3 planes][64 lanes][8 bf16]
    const float* __restrict__ w1ns;      // same, the next block's conv1 (TAIL == 2)
    int H, M;
    float act_a, act_b, t_scale, t_b4, n_b1a, n_b1b, n_b2a, n_b2b;
};

// (C, grid width): (256, 32) [512 threads, one workgroup per CU], (128, 32), (64, 64): 8 image rows x the whole grid width
// WIDE (C = 128, split form, H % 16 == 0): 512 threads own two 8-row bands, 16 image rows x 32 columns, one workgroup per CU
template <int C_, bool WIDE_ = false> struct W43Cfg {
    static constexpr int C = C_;
    static constexpr bool WIDE = WIDE_;
    static constexpr int BANDS = WIDE ? 2 : 1;          // 8-row bands of a workgroup
    static constexpr int ROWS = 8 * BANDS;
    static constexpr int W = C >= 128 ? 32 : 64;
    static constexpr int NT = (C == 256 || WIDE) ? 512 : 256;
    static constexpr int NWV = NT / 64;
    static constexpr int NS = C / 32;                  // 32-channel slices
    static constexpr int TG = NWV / NS;                // 16-tile groups (a wave = one slice x one group; WIDE: the two bands)
    static constexpr int TILES = 16 * TG;              // = 2 tile rows x W / 4 tile columns per band
    static constexpr int TC = W / 4;
    static constexpr int PXH = 4 * W * BANDS;          // pixels of one half (4 of the 8 rows of every band)
    static constexpr int C4 = C / 4;
    static constexpr int RP = NT / C4;                 // pixels one sweep of the workgroup's threads covers (= TC)
    static constexpr int LDT = C + 4;
    static constexpr int KG = C / 16;                  // k-groups (16 channels = 4 MFMAs per block) per position
    static constexpr int KS = C / 8;                   // tails: k-slices
    static constexpr int NI = 2;                       // tails: 32-channel tiles per wave
    static constexpr int WN = C / (32 * NI);           //        waves along the channels
    static constexpr int MI = PXH / ((NWV / WN) * 32); //        32-pixel tiles per wave (MI * NI = 4 accumulators)
    static constexpr int V_BYTES = 6 * TILES * LDT * 4, T_BYTES = PXH * LDT * 4;
    static constexpr int LDS_BYTES = V_BYTES > T_BYTES ? V_BYTES : T_BYTES;
    // split form: V_xi as three bf16 planes per tile row (plane p at p * C), 16 bytes of padding; the tails keep T in fp32
    static constexpr int LDVB = 3 * C + 8, KC = C / 32, KS2 = C / 16;
    static constexpr int VS_BYTES = 6 * TILES * LDVB * 2;
    static constexpr int LDS_SPLIT = VS_BYTES > T_BYTES ? VS_BYTES : T_BYTES;
    static_assert(TILES == 2 * TC * BANDS && RP == TC * BANDS && PXH / RP == 16 && MI * NI == 4, "geometry");
    static_assert(!WIDE || C == 128, "the wide form serves C = 128");
};
constexpr int EARLY = 1;                             // input batches of the next pass requested before the fold over xi (0, 1, 2)
constexpr int RD = 4;                                // weight-fragment ring depth (k-groups of 8 MFMAs = 256 MFMA cycles each)
constexpr int NRES0 = 4;                             // tails: residual rows requested ahead of the first half's conv3
constexpr int RT = 3;                                // tails: ring depth in k-slices (16 MFMAs = 1024 cycles each)

// v = h0 + h1 + h2 + O(2^-24 |v|): each piece rounded to bf16 (RNE, v_cvt_pk_bf16_f32), the residuals exact in fp32.
// bf16 x bf16 products are exact in fp32, so of the nine piece products the six of order >= 2^-18 carry the fp32 product
// (Henry, Tang & Heinecke, ARITH 2019: "bf16x6").
__device__ __forceinline__ void split3(const f32x4& v, bf16x4 (&h)[3]) {
    h[0] = __builtin_convertvector(v, bf16x4);
    const f32x4 r1 = v - __builtin_convertvector(h[0], f32x4);
    h[1] = __builtin_convertvector(r1, bf16x4);
    const f32x4 r2 = r1 - __builtin_convertvector(h[1], f32x4);
    h[2] = __builtin_convertvector(r2, bf16x4);
}
__device__ __forceinline__ bf16x8 as_bf8(const f32x4& v) { return __builtin_bit_cast(bf16x8, v); }

__device__ __forceinline__ f32x4 fma4(const f32x4& a, float s, const f32x4& c) {
    return __builtin_elementwise_fma(a, f32x4{s, s, s, s}, c);
}

// uniform base (SGPR pair) + 32-bit per-lane byte offset: the `global_load ... v_off, s[base]` form.  (A per-lane 64-bit pointer plus
// a large constant offset per load makes hipcc materialise -- and, hoisted out of the xi loop, spill -- one address pair per load.)
__device__ __forceinline__ f32x4 ldg(const float* sbase, unsigned voff_bytes) {
    return *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(sbase) + voff_bytes);
}

template <int N> struct IC { static constexpr int value = N; };

// image row (relative to the workgroup's first row of the half) of row r of T: band r / 4, rows {0, 1, 4, 5} of its 8.  Used by the wide
// form only: the 8-row forms spell 4 (r >> 1) + (r & 1) out in place, because routing that one expression through a function, even an
// inlined one with the same text, changes hipcc's address arithmetic around it (a few dozen instructions per kernel), and those kernels
// are to stay what they were, instruction for instruction.
constexpr int tail_row(int r) { return 8 * (r >> 2) + 4 * ((r >> 1) & 1) + (r & 1); }

template <int C, int TAIL, bool SPLIT, bool WIDE = false>
__global__ __launch_bounds__((W43Cfg<C, WIDE>::NT), (W43Cfg<C, WIDE>::NT == 512 ? 1 : 2))
void wino43_trunk_kernel(const W43K p) {
    using K = W43Cfg<C, WIDE>;
    static_assert(!WIDE || SPLIT, "the wide form is a split form");
    constexpr int W = K::W, LDT = K::LDT, KG = K::KG, KS = K::KS, TILES = K::TILES, TC = K::TC, NS = K::NS, C4 = K::C4, RP = K::RP;
    constexpr int MI = K::MI, NI = K::NI, WN = K::WN;
    constexpr int LDVB = K::LDVB, KC = K::KC, KS2 = K::KS2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, q = lane >> 4;                         // main phase: tile of the group, channel quad of the 16-channel block
    // main phase: 32-channel slice, 16-tile group.  WIDE: wave = 16-channel block cb of slice cb >> 1, both bands (16 tiles each)
    const int ns = WIDE ? wave >> 1 : wave % NS, tg = WIDE ? 0 : wave / NS;

    int tile_m;                                                      // XCD-contiguous order (conv_wino.hip)
    {
        const int nwg = gridDim.x, bid = blockIdx.x;
        const int qq = nwg >> 3, r = nwg & 7, xcd = bid & 7;
        tile_m = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + (bid >> 3);
    }
    const int tpi = p.H / K::ROWS;
    const int img = tile_m / tpi;
    const int row0 = K::ROWS * (tile_m - img * tpi);
    const float* const xim = p.t1 + (int64_t)img * p.H * W * C;

    // ---- transform geometry: thread -> channel quad cg, tile column tj, both tile rows ------------------------------------
    // (WIDE: the band is uniform per wave, and its halo rows may lie in the other band or workgroup.  A wave covers all eight tile
    // columns of its band for 32 channels -- lane = 8 tile column + channel quad of the 32, wave = 4 band + channel quarter -- and a
    // thread loads only the first four of its six columns: the other two are the first two of the next tile column, which the lane 8
    // further on holds row-combined after combine(); the rotation over the whole wave is the circular wrap in x (W = 32).)
    const int cg = tid % C4, tj = tid / C4;                          // (the tails' row-coalesced view in every form)
    const int xcg = WIDE ? 8 * (wave & 3) + (lane & 7) : cg, tjc = WIDE ? lane >> 3 : tj, band = WIDE ? wave >> 2 : 0;
    constexpr int NCOL = WIDE ? 4 : 6, NB = NCOL / 2;                // columns a thread loads; batches (of 2 columns) per tile row
    unsigned coff[NCOL];                                             // per-lane byte offsets of the unit's columns
    int roff[2][6];                                                  // uniform float offsets of its 6 rows
#pragma unroll
    for (int j = 0; j < NCOL; ++j) coff[j] = (unsigned)((((4 * tjc - 1 + j) & (W - 1)) * C + 4 * xcg) * 4);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            int r = row0 + 8 * band + 4 * s - 1 + i;
            r = r < 0 ? r + p.H : (r >= p.H ? r - p.H : r);
            roff[s][i] = r * W * C;
        }

    // One pass's input: per tile row s, column pair cp: rows (0, 2, 4) [KIND 0], (1, 3, 5) [KIND 5] or (1, 2, 3, 4) [KIND 1].
    f32x4 d[2][4][2];                                                // two batches in flight
    f32x4 w[6];                                                      // row-combined columns of the unit in work
    auto issue = [&](auto kind_c, int k) __attribute__((always_inline)) {                           // batch k = NB s + cp (compile-time after unrolling)
        constexpr int KIND = decltype(kind_c)::value;
        const int s = k / NB, cp = k % NB, bf = k & 1;
#pragma unroll
        for (int i = 0; i < (KIND == 1 ? 4 : 3); ++i) {
            const int row = KIND == 0 ? 2 * i : (KIND == 5 ? 2 * i + 1 : i + 1);
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) d[bf][i][jj] = ldg(xim + roff[s][row], coff[2 * cp + jj]);
        }
    };
    auto combine = [&](auto kind_c, int k, float c1, float c2, float c3) __attribute__((always_inline)) {
        constexpr int KIND = decltype(kind_c)::value;
        const int cp = k % NB, bf = k & 1;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            if (KIND == 1) w[2 * cp + jj] = fma4(d[bf][0][jj], c1, fma4(d[bf][1][jj], c2, fma4(d[bf][2][jj], c3, d[bf][3][jj])));
            else w[2 * cp + jj] = fma4(d[bf][0][jj], 4.f, fma4(d[bf][1][jj], -5.f, d[bf][2][jj]));     // B^T rows 0 / 5: [4 0 -5 0 1 0]
        }
    };
    // WIDE: columns 4, 5 of the unit = columns 0, 1 of the next tile column (the same raw values through the same fma chain, so the
    // same bits), from the lane 8 further on: 8 ds_bpermute_b32 per tile row, no LDS memory, no barrier
    auto exchange = [&]() __attribute__((always_inline)) {
        const int nb = 4 * ((lane + 8) & 63);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float mine = w[jj][e];                         // (a scalar copy: __builtin_bit_cast of a vector element reads element 0)
                w[4 + jj][e] = __int_as_float(__builtin_amdgcn_ds_bpermute(nb, __float_as_int(mine)));
            }
    };
    // V slot of tile (s, tile column) within its band.  WIDE: 4 (tjc & 3) + 2 (tjc >> 2) + s, so that neighbouring tile columns lie
    // 4 slots = 16 banks (LDVB / 2 = 196 dwords = 4 mod 32) apart, next to the 16 banks of a lane group's eight channel quads: the
    // 16 lanes of a ds_write_b64 group (two tile columns x eight quads) cover all 32 banks once.  The GEMM reads slot li, whatever tile
    // that is; the tails invert the permutation (ty, tx).
    auto columns = [&](int s) __attribute__((always_inline)) {                                      // (w B)[nu] -> V[nu][tile][c]
        const int slot = WIDE ? 4 * (tjc & 3) + 2 * (tjc >> 2) + s : s * TC + tjc;
        float* const dst = lds + (16 * band + slot) * LDT + 4 * xcg;
        __bf16* const dsb = reinterpret_cast<__bf16*>(lds) + (16 * band + slot) * LDVB + 4 * xcg;
        // WIDE: V spans 147 KiB and a DS instruction's offset field 64 KiB, so nu = 3..5 go through a second base, opaque so that
        // hipcc forms it once per use instead of keeping (and spilling) one address per access
        int vhi = 3 * TILES * LDVB;
        if constexpr (WIDE) asm volatile("" : "+v"(vhi));
        auto put = [&](int nu, const f32x4& v) __attribute__((always_inline)) {
            if constexpr (SPLIT) {                                    // split once here, not after every wave's ds_read
                bf16x4 h[3];
                split3(v, h);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    if (WIDE && nu >= 3) *reinterpret_cast<bf16x4*>(dsb + vhi + (nu - 3) * TILES * LDVB + pl * C) = h[pl];
                    else *reinterpret_cast<bf16x4*>(dsb + nu * TILES * LDVB + pl * C) = h[pl];
                }
            } else {
                *reinterpret_cast<f32x4*>(dst + nu * TILES * LDT) = v;
            }
        };
        const f32x4 t1 = fma4(w[2], -4.f, w[4]), t2 = fma4(w[1], -4.f, w[3]);
        const f32x4 t3 = w[4] - w[2], t4 = w[3] - w[1];
        put(0, fma4(w[0], 4.f, fma4(w[2], -5.f, w[4])));
        put(1, t1 + t2);
        put(2, t1 - t2);
        put(3, fma4(t4, 2.f, t3));
        put(4, fma4(t4, -2.f, t3));
        put(5, fma4(w[1], 4.f, fma4(w[3], -5.f, w[5])));
    };

    // weights: this wave's 16 KiB of a position are contiguous ([k-group][block][lane][4]); positions C * C floats apart
    const float* const ub = p.U + ns * (KG * 512);                   // uniform; + 16 lane bytes per lane
    // split form: this wave's 24 KiB of a position (WIDE: the 12 KiB of its 16-channel block, 768 floats into every chunk)
    const float* const ubs = p.Us + ns * (KC * 1536) + (WIDE ? 768 * (wave & 1) : 0);
    const __bf16* const vbs = reinterpret_cast<const __bf16*>(lds) + (16 * tg + li) * LDVB + 8 * q;   // split V fragment base
    const unsigned wl = 16u * lane;
    const float* const bfrag = lds + (16 * tg + li) * LDT + 4 * q;  // V fragment base, + nu * TILES * LDT + 16 kg

    f32x4 Y[4][4][2];                                                // [a][b][block]: conv2 output (4 a' + a, 4 b' + b) of tile li, 4 channels
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) { Y[a][b][0] = f32x4{0.f, 0.f, 0.f, 0.f}; Y[a][b][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    // ---- one pass: V_xi -> LDS, 6 GEMMs, fold.  The first two input batches of the pass are already in flight. -----------------
    auto pass = [&](auto kind_c, auto next_c, int xi, float c1, float c2, float c3, float a1, float a2, float a3) __attribute__((always_inline)) {
        constexpr int KIND = decltype(kind_c)::value;
        constexpr int NEXT = decltype(next_c)::value;                // kind of the following pass (-1: none)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < NCOL; ++j) asm volatile("" : "+v"(coff[j]));  // opaque per pass (as uoff below): no hoisted 64-bit address per (row, column)
        if (EARLY < 1) issue(kind_c, 0);                             // (EARLY batches of this pass went out before the previous pass's fold)
        if (EARLY < 2) issue(kind_c, 1);
#pragma unroll
        for (int k = 0; k < 2 * NB; ++k) {
            combine(kind_c, k, c1, c2, c3);
            if (k % NB == NB - 1) {
                if constexpr (WIDE) exchange();
                columns(k / NB);                                     // before the next request: w, the column temporaries and TWO batches in flight do not fit
            }
            if (k + 2 < 2 * NB) issue(kind_c, k + 2);
        }
        __builtin_amdgcn_sched_barrier(0);                            // (the weight loads below must not rise into the transform: registers)
        f32x4 Z[4][2];
        f32x4 acc[2][2];
        // fold over nu: Z[b] += A^T[b][nu] acc,  A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
        auto fold_nu = [&](int nu) __attribute__((always_inline)) {
#pragma unroll
            for (int bl = 0; bl < 2; ++bl) {
                if (nu == 0) Z[0][bl] = Z[0][bl] + acc[0][bl];
                if (nu == 2) {                                        // nu = 1 (set 1) and nu = 2 (set 0)
                    const f32x4 sm = acc[1][bl] + acc[0][bl], df = acc[1][bl] - acc[0][bl];
                    Z[0][bl] = Z[0][bl] + sm; Z[2][bl] = Z[2][bl] + sm;
                    Z[1][bl] = Z[1][bl] + df; Z[3][bl] = Z[3][bl] + df;
                }
                if (nu == 4) {                                        // nu = 3 (set 1) and nu = 4 (set 0)
                    const f32x4 sm = acc[1][bl] + acc[0][bl], df = acc[1][bl] - acc[0][bl];
                    Z[0][bl] = Z[0][bl] + sm; Z[2][bl] = fma4(sm, 4.f, Z[2][bl]);
                    Z[1][bl] = fma4(df, 2.f, Z[1][bl]); Z[3][bl] = fma4(df, 8.f, Z[3][bl]);
                }
                if (nu == 5) Z[3][bl] = Z[3][bl] + acc[1][bl];
            }
            if (nu == 0 || nu == 2 || nu == 4)
                asm volatile("" : "+v"(Z[0][0]), "+v"(Z[0][1]), "+v"(Z[1][0]), "+v"(Z[1][1]), "+v"(Z[2][0]), "+v"(Z[2][1]), "+v"(Z[3][0]), "+v"(Z[3][1]));
        };
        if constexpr (WIDE) {
            // Wide form: the split walk below with the band in place of the 16-channel block -- per 32-channel chunk one fragment
            // per plane (16 registers) feeds both bands' V fragments (24 registers); every accumulator sees the MFMAs of the
            // 8-row form in their order.
            int64_t uoff = (int64_t)xi * 6 * (3 * C * C / 2);
            asm volatile("" : "+s"(uoff));
            const float* const ux = ubs + uoff;
#define WS(s, pl) (((s) / KC) * (3 * C * C / 2) + 1536 * ((s) % KC) + 256 * (pl))
            // (nu = 3..5 through a second, opaque base: see columns())
            int vhi = 3 * TILES * LDVB;
            asm volatile("" : "+v"(vhi));
            const __bf16* const vbh = vbs + vhi;
#define VB(s, g, pl) (*reinterpret_cast<const bf16x8*>(((s) / KC >= 3 ? vbh - 3 * TILES * LDVB : vbs) + ((s) / KC) * TILES * LDVB + (g) * 16 * LDVB + (pl) * C + 32 * ((s) % KC)))
            f32x4 w0[2], w1[2], w2[2];                                   // [slot]: every plane two chunks ahead
            w1[0] = ldg(ux + WS(0, 1), wl);
            w2[0] = ldg(ux + WS(0, 2), wl);
            w0[0] = ldg(ux + WS(0, 0), wl);
            w1[1] = ldg(ux + WS(1, 1), wl);
            w2[1] = ldg(ux + WS(1, 2), wl);
            w0[1] = ldg(ux + WS(1, 0), wl);
            lds_barrier();                                               // V complete
#pragma unroll
            for (int b = 0; b < 4; ++b) { Z[b][0] = f32x4{0.f, 0.f, 0.f, 0.f}; Z[b][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            bf16x8 vb0[2], vb1[2], vb2[2];                               // [band]
#pragma unroll
            for (int g = 0; g < 2; ++g) { vb0[g] = VB(0, g, 0); vb1[g] = VB(0, g, 1); vb2[g] = VB(0, g, 2); }
#pragma unroll
            for (int nu = 0; nu < 6; ++nu) {
                const int st = nu & 1;
                acc[st][0] = f32x4{0.f, 0.f, 0.f, 0.f};
                acc[st][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kc = 0; kc < KC; ++kc) {
                    const int s = KC * nu + kc, sl = s & 1;
                    const bool nxt = s + 1 < 6 * KC;
#define MM(wa, vb) for (int g = 0; g < 2; ++g) acc[st][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf8(wa), vb[g], acc[st][g], 0, 0, 0)
                    MM(w1[sl], vb1);                                     // a1 b1
                    MM(w1[sl], vb0);                                     // a1 b0
                    if (s + 2 < 6 * KC) w1[sl] = ldg(ux + WS(s + 2, 1), wl);
                    MM(w2[sl], vb0);                                     // a2 b0
                    if (s + 2 < 6 * KC) w2[sl] = ldg(ux + WS(s + 2, 2), wl);
                    MM(w0[sl], vb2);                                     // a0 b2
                    if (nxt) for (int g = 0; g < 2; ++g) vb2[g] = VB(s + 1, g, 2);
                    MM(w0[sl], vb1);                                     // a0 b1
                    if (nxt) for (int g = 0; g < 2; ++g) vb1[g] = VB(s + 1, g, 1);
                    MM(w0[sl], vb0);                                     // a0 b0
                    if (s + 2 < 6 * KC) w0[sl] = ldg(ux + WS(s + 2, 0), wl);
                    if (nxt) for (int g = 0; g < 2; ++g) vb0[g] = VB(s + 1, g, 0);
#undef MM
                    __builtin_amdgcn_sched_barrier(0);
                }
                fold_nu(nu);
            }
#undef WS
#undef VB
        } else if constexpr (SPLIT) {
            // Split form: per 32-channel chunk, six v_mfma_f32_16x16x32_bf16 per block (96 cycles) replace 16 v_mfma_f32_16x16x4_f32
            // (256 cycles).  Registers allow 32 for weights (Y, Z and the accumulators hold 176): the hi plane is double-buffered, mid and
            // lo are used first in each chunk and re-requested for the next one right after their last use; the V planes likewise.
            int64_t uoff = (int64_t)xi * 6 * (3 * C * C / 2);
            asm volatile("" : "+s"(uoff));
            const float* const ux = ubs + uoff;
#define WS(s, bl, pl) (((s) / KC) * (3 * C * C / 2) + 1536 * ((s) % KC) + 256 * (3 * (bl) + (pl)))
#define VB(s, pl) (*reinterpret_cast<const bf16x8*>(vbs + ((s) / KC) * TILES * LDVB + (pl) * C + 32 * ((s) % KC)))
            f32x4 w0[2][2], w1[2], w2[2];                                // [slot][block] hi plane, [block] mid / lo planes
#pragma unroll
            for (int bl = 0; bl < 2; ++bl) {
                w0[0][bl] = ldg(ux + WS(0, bl, 0), wl);
                w1[bl] = ldg(ux + WS(0, bl, 1), wl);
                w2[bl] = ldg(ux + WS(0, bl, 2), wl);
                w0[1][bl] = ldg(ux + WS(1, bl, 0), wl);
            }
            lds_barrier();                                               // V complete
#pragma unroll
            for (int b = 0; b < 4; ++b) { Z[b][0] = f32x4{0.f, 0.f, 0.f, 0.f}; Z[b][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            bf16x8 vb0 = VB(0, 0), vb1 = VB(0, 1), vb2 = VB(0, 2);
#pragma unroll
            for (int nu = 0; nu < 6; ++nu) {
                const int st = nu & 1;
                acc[st][0] = f32x4{0.f, 0.f, 0.f, 0.f};
                acc[st][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kc = 0; kc < KC; ++kc) {
                    const int s = KC * nu + kc, sl = s & 1;
                    const bool nxt = s + 1 < 6 * KC;
#define MM(wa, vb) for (int bl = 0; bl < 2; ++bl) acc[st][bl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf8(wa[bl]), vb, acc[st][bl], 0, 0, 0)
                    MM(w1, vb1);                                         // a1 b1
                    MM(w1, vb0);                                         // a1 b0
                    if (nxt) for (int bl = 0; bl < 2; ++bl) w1[bl] = ldg(ux + WS(s + 1, bl, 1), wl);
                    MM(w2, vb0);                                         // a2 b0
                    if (nxt) for (int bl = 0; bl < 2; ++bl) w2[bl] = ldg(ux + WS(s + 1, bl, 2), wl);
                    MM(w0[sl], vb2);                                     // a0 b2
                    if (nxt) vb2 = VB(s + 1, 2);
                    MM(w0[sl], vb1);                                     // a0 b1
                    if (nxt) vb1 = VB(s + 1, 1);
                    MM(w0[sl], vb0);                                     // a0 b0
                    if (s + 2 < 6 * KC) for (int bl = 0; bl < 2; ++bl) w0[sl][bl] = ldg(ux + WS(s + 2, bl, 0), wl);
                    if (nxt) vb0 = VB(s + 1, 0);
#undef MM
                    __builtin_amdgcn_sched_barrier(0);
                }
                fold_nu(nu);
            }
#undef WS
#undef VB
        } else {
            int64_t uoff = (int64_t)xi * 6 * (C * C);
            asm volatile("" : "+s"(uoff));                                // opaque per pass: keeps hipcc from hoisting one address pair per load out of the xi loop
            const float* const ux = ub + uoff;
#define WB(s) (((s) / KG) * (C * C) + 512 * ((s) % KG))
            f32x4 wq[RD][2];
#pragma unroll
            for (int s = 0; s < RD; ++s) {                               // first weight fragments: in flight across the barrier
                wq[s][0] = ldg(ux + WB(s), wl);
                wq[s][1] = ldg(ux + WB(s) + 256, wl);
            }
            lds_barrier();                                               // V complete
#pragma unroll
            for (int b = 0; b < 4; ++b) { Z[b][0] = f32x4{0.f, 0.f, 0.f, 0.f}; Z[b][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            f32x4 bq[2];
            bq[0] = *reinterpret_cast<const f32x4*>(bfrag);
#pragma unroll
            for (int nu = 0; nu < 6; ++nu) {
                const int st = nu & 1;
                acc[st][0] = f32x4{0.f, 0.f, 0.f, 0.f};
                acc[st][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kg = 0; kg < KG; ++kg) {
                    const int s = KG * nu + kg;
                    if (s + 1 < 6 * KG)
                        bq[(s + 1) & 1] = *reinterpret_cast<const f32x4*>(bfrag + ((s + 1) / KG) * TILES * LDT + 16 * ((s + 1) % KG));
                    const f32x4 wa = wq[s % RD][0], wb = wq[s % RD][1];
                    if (s + RD < 6 * KG) {
                        wq[s % RD][0] = ldg(ux + WB(s + RD), wl);
                        wq[s % RD][1] = ldg(ux + WB(s + RD) + 256, wl);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[st][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[j], bq[s & 1][j], acc[st][0], 0, 0, 0);   // D[channel][tile]
                        acc[st][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[j], bq[s & 1][j], acc[st][1], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);                    // keep the prefetch distances as written
                }
                fold_nu(nu);
            }
#undef WB
        }
        // the next pass's first input batches go out before the fold over xi and the barrier
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (NEXT == 9) {                                   // inside the xi = 1..4 loop: rows (1, 2, 3, 4) of pass xi + 1 <= 4, rows (1, 3, 5, -) of pass 5
#pragma unroll
            for (int k = 0; k < EARLY; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ro = xi < 4 ? roff[0][i + 1] : roff[0][i < 3 ? 2 * i + 1 : 5];
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) d[k & 1][i][jj] = ldg(xim + ro, coff[2 * k + jj]);
                }
        } else {
            if constexpr (NEXT >= 0 && EARLY >= 1) issue(next_c, 0);
            if constexpr (NEXT >= 0 && EARLY >= 2) issue(next_c, 1);
        }
        // fold over xi: Y[a][b] += A^T[a][xi] Z[b]
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int bl = 0; bl < 2; ++bl) {
                if (KIND == 0) Y[0][b][bl] = Y[0][b][bl] + Z[b][bl];
                else if (KIND == 5) Y[3][b][bl] = Y[3][b][bl] + Z[b][bl];
                else {
                    Y[0][b][bl] = Y[0][b][bl] + Z[b][bl];
                    Y[1][b][bl] = fma4(Z[b][bl], a1, Y[1][b][bl]);
                    Y[2][b][bl] = fma4(Z[b][bl], a2, Y[2][b][bl]);
                    Y[3][b][bl] = fma4(Z[b][bl], a3, Y[3][b][bl]);
                }
            }
        lds_barrier();                                               // every wave is done reading V of this pass
    };

    if (EARLY >= 1) issue(IC<0>{}, 0);
    if (EARLY >= 2) issue(IC<0>{}, 1);
    pass(IC<0>{}, IC<1>{}, 0, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int xi = 1; xi <= 4; ++xi) {
        // B^T rows 1..4: [0 -4 -4 1 1 0], [0 4 -4 -1 1 0], [0 -2 -1 2 1 0], [0 2 -1 -2 1 0];  A^T columns 1..4: (1,1,1,1), (1,-1,1,-1), (1,2,4,8), (1,-2,4,-8)
        const float sg = (xi & 1) ? 1.f : -1.f;                      // xi = 1, 3: +; 2, 4: -
        const bool lo = xi <= 2;
        const float c1 = lo ? -4.f * sg : -2.f * sg, c2 = lo ? -4.f : -1.f, c3 = lo ? sg : 2.f * sg;
        const float a1 = lo ? sg : 2.f * sg, a2 = lo ? 1.f : 4.f, a3 = lo ? sg : 8.f * sg;
        pass(IC<1>{}, IC<9>{}, xi, c1, c2, c3, a1, a2, a3);
    }
    pass(IC<5>{}, IC<-1>{}, 5, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);

    // ---- tails on two 128-pixel halves: half hf = output rows 2 hf, 2 hf + 1 of every tile = image rows row0 + {0, 1, 4, 5} + 2 hf ----
    // (WIDE: 256-pixel halves, band 0's 128 pixels then band 1's; the wave tiling is the same with four waves along the pixels)
    float* const T = lds;
    const int li32 = lane & 31, hh = lane >> 5;                      // 32x32x2 layout of the tails
    const int wm = wave / WN, wn = wave % WN;                        // MI * 32 pixels x NI * 32 channels per wave
    const int tj0 = tj;                                              // row-coalesced view: thread (cg, tj0) owns pixels tj0 + RP i of the half
    [[maybe_unused]] float* const trow = WIDE ? nullptr : T + tj0 * LDT + 4 * cg;   // 8-row forms; WIDE: tr() below
    // tile row / column of the lane's Y (WIDE: li is the permuted V slot of columns())
    const int ty = WIDE ? li & 1 : (16 * tg + li) / TC, tx = WIDE ? 4 * ((li >> 1) & 1) + (li >> 2) : (16 * tg + li) % TC;
    f32x4 bt[RT][NI];
    f32x4 bs0[2][NI], bs1[NI], bs2[NI];                              // split form: the hi plane of two k-slices, mid / lo of one
    auto tail_prefetch = [&](const float* __restrict__ wsrc) __attribute__((always_inline)) {
        if constexpr (SPLIT) {
            const float* b0 = wsrc + (wn * NI) * (KS2 * 768);
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                bs0[0][ni] = ldg(b0 + ni * (KS2 * 768), wl);
                bs1[ni] = ldg(b0 + ni * (KS2 * 768) + 256, wl);
                bs2[ni] = ldg(b0 + ni * (KS2 * 768) + 512, wl);
                bs0[1][ni] = ldg(b0 + ni * (KS2 * 768) + 768, wl);
            }
            return;
        }
        const float* b0 = wsrc + (wn * NI) * (KS * 256);
#pragma unroll
        for (int u = 0; u < RT; ++u)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) bt[u][ni] = ldg(b0 + ni * (KS * 256) + 256 * u, wl);
    };
    f32x16 acc[MI][NI];
    // Split form of gemm_tail: per 16-channel k-slice, each lane reads its 8 fp32 values of T per 32-pixel tile and splits them
    // (the WN waves along the channels repeat this); six v_mfma_f32_32x32x16_bf16 per tile pair (192 cycles) replace
    // 8 v_mfma_f32_32x32x2_f32 (512 cycles), in the order and weight ring of the main phase.  The output layout is that of the fp32 form.
    auto gemm_tail_split = [&](const float* __restrict__ wsrc) __attribute__((always_inline)) {
        const float* a0 = T + (wm * MI * 32 + li32) * LDT + 8 * hh;
        const float* b0 = wsrc + (wn * NI) * (KS2 * 768);
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) {
            const int sl = ks & 1;
            bf16x8 x[MI][3];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                bf16x4 lo[3], hi[3];
                split3(*reinterpret_cast<const f32x4*>(a0 + mi * 32 * LDT + 16 * ks), lo);
                split3(*reinterpret_cast<const f32x4*>(a0 + mi * 32 * LDT + 16 * ks + 4), hi);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) x[mi][pl] = __builtin_shufflevector(lo[pl], hi[pl], 0, 1, 2, 3, 4, 5, 6, 7);
            }
#define MM(wa, pb) for (int mi = 0; mi < MI; ++mi) for (int ni = 0; ni < NI; ++ni) \
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf8(wa[ni]), x[mi][pb], acc[mi][ni], 0, 0, 0)
#define RELOAD(dst, k, pl) for (int ni = 0; ni < NI; ++ni) dst[ni] = ldg(b0 + ni * (KS2 * 768) + 768 * (k) + 256 * (pl), wl)
            MM(bs1, 1);
            MM(bs1, 0);
            if (ks + 1 < KS2) RELOAD(bs1, ks + 1, 1);
            MM(bs2, 0);
            if (ks + 1 < KS2) RELOAD(bs2, ks + 1, 2);
            MM(bs0[sl], 2);
            MM(bs0[sl], 1);
            MM(bs0[sl], 0);
            if (ks + 2 < KS2) RELOAD(bs0[sl], ks + 2, 0);
#undef MM
#undef RELOAD
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto gemm_tail = [&](const float* __restrict__ wsrc) __attribute__((always_inline)) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
        if constexpr (SPLIT) {
            gemm_tail_split(wsrc);
            return;
        }
        const float* a0 = T + (wm * MI * 32 + li32) * LDT + 4 * hh;
        const float* b0 = wsrc + (wn * NI) * (KS * 256);
        f32x4 a[2][MI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) a[0][mi] = *reinterpret_cast<const f32x4*>(a0 + mi * 32 * LDT);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks + 1 < KS) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) a[(ks + 1) & 1][mi] = *reinterpret_cast<const f32x4*>(a0 + mi * 32 * LDT + 8 * (ks + 1));
            }
            f32x4 bc[NI];
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) bc[ni] = bt[ks % RT][ni];
            if (ks + RT < KS) {
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) bt[ks % RT][ni] = ldg(b0 + ni * (KS * 256) + 256 * (ks + RT), wl);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(bc[ni][r], a[ks & 1][mi][r], acc[mi][ni], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto acc_to_lds = [&]() __attribute__((always_inline)) {                                         // D[channel][pixel] -> T[pixel][channel], 128-bit writes
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = acc[mi][ni][4 * g + e];
                    *reinterpret_cast<f32x4*>(T + (wm * MI * 32 + mi * 32 + li32) * LDT + (wn * NI + ni) * 32 + 8 * g + 4 * hh) = o;
                }
    };

#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        // WIDE: T spans 132 KiB (a DS offset field: 64 KiB), so band 1 / the sweeps i >= 8 go through second bases, opaque per half so
        // that hipcc neither forms one address per access nor keeps them from one half to the next
        int tbo = (2 * ty * W + 4 * tx) * LDT + 16 * wave + 4 * q, tro = tj0 * LDT + 4 * cg;
        if constexpr (WIDE) asm volatile("" : "+v"(tbo), "+v"(tro));
        int tbo1 = tbo + 4 * W * LDT, tro1 = tro + 8 * RP * LDT;
        if constexpr (WIDE) asm volatile("" : "+v"(tbo1), "+v"(tro1));
        auto tr = [&](int i) __attribute__((always_inline)) {
            if constexpr (WIDE) return reinterpret_cast<f32x4*>(T + (i < 8 ? tro + RP * i * LDT : tro1 + RP * (i - 8) * LDT));
            else return reinterpret_cast<f32x4*>(trow + RP * i * LDT);
        };
        // t2 = ELU(conv2 + b3a) + b3b -> T[pixel][channel]; T row r' <-> image row row0 + 4 (r' >> 1) + 2 hf + (r' & 1)
#pragma unroll
        for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int bl = 0; bl < 2; ++bl) {
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = elu_act(Y[2 * hf + a2][b][bl][e] + p.act_a) + p.act_b;
                    if constexpr (WIDE) *reinterpret_cast<f32x4*>(T + (bl ? tbo1 : tbo) + (a2 * W + b) * LDT) = o;
                    else *reinterpret_cast<f32x4*>(T + ((2 * ty + a2) * W + 4 * tx + b) * LDT + 32 * ns + 16 * bl + 4 * q) = o;
                }
        tail_prefetch(SPLIT ? p.w3s : p.w3);
        // pixel (i) of the thread in the residual stream / the next t1.  8-row forms: one pointer per row of the half.  WIDE: eight row
        // pointers per half do not fit the registers; a uniform row base + one per-lane offset (as ldg) instead
        [[maybe_unused]] float* xr[WIDE ? 1 : K::PXH / W];
        [[maybe_unused]] int64_t xu = 0;
        [[maybe_unused]] unsigned xvo = 0;
        if constexpr (WIDE) {
            xu = (((int64_t)img * p.H + row0 + 2 * hf) * W) * C;
            xvo = (unsigned)((tj0 * C + 4 * cg) * 4);
            asm volatile("" : "+v"(xvo));
        } else {
            const int64_t pixb = ((int64_t)img * p.H + row0 + 2 * hf) * W + tj0;
#pragma unroll
            for (int r = 0; r < K::PXH / W; ++r) xr[r] = p.xio + (pixb + (int64_t)(4 * (r >> 1) + (r & 1)) * W) * C + 4 * cg;
        }
        auto xp = [&](float* base, int i) __attribute__((always_inline)) {
            const int r = (RP * i) / W;
            if constexpr (WIDE) {
                int64_t ro = xu + (tail_row(r) * W + (RP * i) % W) * C;
                asm volatile("" : "+s"(ro));                          // stays a scalar base: no 64-bit per-lane address per row
                return reinterpret_cast<f32x4*>(reinterpret_cast<char*>(base + ro) + xvo);
            } else {
                return reinterpret_cast<f32x4*>(xr[r] + ((RP * i) % W) * C);
            }
        };
        // residual rows: requested ahead of conv3 -- in the first half only half of them (the second half's Y is still live: registers)
        f32x4 res[16];
#pragma unroll
        for (int i = 0; i < (hf == 0 ? NRES0 : 16); ++i) res[i] = __builtin_nontemporal_load(xp(p.xio, i));
        lds_barrier();                                               // t2 complete
        gemm_tail(SPLIT ? p.w3s : p.w3);                             // conv3
        if (hf == 0) {
#pragma unroll
            for (int i = NRES0; i < 16; ++i) res[i] = __builtin_nontemporal_load(xp(p.xio, i));
        }
        if (TAIL == 2) tail_prefetch(SPLIT ? p.w1ns : p.w1n);
        lds_barrier();                                               // every wave is done reading t2
        acc_to_lds();
        lds_barrier();
        // out = conv3 * scale + bias4 + x, in place over the residual stream, whole pixel rows per 8th of a workgroup
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            f32x4 t = *tr(i);
            t = t * p.t_scale;
            t = t + p.t_b4;
            t = t + res[i];
            __builtin_nontemporal_store(t, xp(p.xio, i));
            if (TAIL == 2) {                                          // next block's conv1 pre-op, back into T in place
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = elu_act(t[e] + p.n_b1a) + p.n_b1b;
                *tr(i) = t;
            }
        }
        if constexpr (TAIL == 2) {
            lds_barrier();
            gemm_tail(SPLIT ? p.w1ns : p.w1n);                       // next block's conv1
            lds_barrier();                                           // every wave is done reading T
            acc_to_lds();
            lds_barrier();
            [[maybe_unused]] float* y0 = nullptr;
            if constexpr (!WIDE) y0 = p.y2 + (xr[0] - p.xio);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                f32x4 t = *tr(i);
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = elu_act(t[e] + p.n_b2a) + p.n_b2b;
                const int r = (RP * i) / W;
                if constexpr (WIDE) __builtin_nontemporal_store(t, xp(p.y2, i));
                else __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(y0 + ((4 * (r >> 1) + (r & 1)) * W + (RP * i) % W) * C));
            }
        }
        if (hf == 0) lds_barrier();                                  // T is rewritten by the second half's t2
    }
}

// U[pos = 6 xi + nu] = (G g G^T)[xi][nu] for g = w[n][k][3][3], evaluated in fp64;
// G = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
__device__ void wino43_u(const float* __restrict__ w, int64_t i, double (&u)[36]) {
    const double G[6][3] = {{0.25, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                            {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    double g[3][3], t[6][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) g[a][b] = (double)w[i * 9 + a * 3 + b];
    for (int x = 0; x < 6; ++x)
        for (int b = 0; b < 3; ++b) t[x][b] = G[x][0] * g[0][b] + G[x][1] * g[1][b] + G[x][2] * g[2][b];
    for (int x = 0; x < 6; ++x)
        for (int y = 0; y < 6; ++y) u[x * 6 + y] = t[x][0] * G[y][0] + t[x][1] * G[y][1] + t[x][2] * G[y][2];
}

// rounded once -> [pos][n >> 5][k >> 4][(n >> 4) & 1][lane = ((k >> 2) & 3) * 16 + (n & 15)][k & 3]: what lane (li, q) feeds to MFMA k & 3
// of the k-group.
__global__ void wino43_weight_kernel(const float* __restrict__ w, int c, float* __restrict__ U) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;              // over n * c + k
    if (i >= c * c) return;
    double u[36];
    wino43_u(w, i, u);
    const int n = i / c, k = i % c;
    const int64_t fo = ((((int64_t)(n >> 5) * (c / 16) + (k >> 4)) * 2 + ((n >> 4) & 1)) * 64 + ((k >> 2) & 3) * 16 + (n & 15)) * 4 + (k & 3);
    const int64_t cc = (int64_t)c * c;
    for (int x = 0; x < 36; ++x) U[x * cc + fo] = (float)u[x];
}

// v = h0 + h1 + h2 + O(2^-25 |v|), each piece bf16 (RNE), the residuals taken in fp64
__device__ void split3_f64(double v, __bf16 (&h)[3]) {
    for (int pl = 0; pl < 3; ++pl) {
        h[pl] = (__bf16)(float)v;
        v -= (double)(float)h[pl];
    }
}

// split form: U split from the fp64 value -> [pos][n >> 5][k >> 5][(n >> 4) & 1][plane][lane = ((k >> 3) & 3) * 16 + (n & 15)][k & 7],
// the A fragment of v_mfma_f32_16x16x32_bf16 (lane (li, q) holds row li, k = 8 q .. 8 q + 7 of the 32-channel chunk)
__global__ void wino43_split_weight_kernel(const float* __restrict__ w, int c, __bf16* __restrict__ U) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c * c) return;
    double u[36];
    wino43_u(w, i, u);
    const int n = i / c, k = i % c;
    const int64_t fo = (((int64_t)(n >> 5) * (c / 32) + (k >> 5)) * 2 + ((n >> 4) & 1)) * 3 * 512 + (((k >> 3) & 3) * 16 + (n & 15)) * 8 + (k & 7);
    const int64_t cc = (int64_t)c * c;
    for (int x = 0; x < 36; ++x) {
        __bf16 h[3];
        split3_f64(u[x], h);
        for (int pl = 0; pl < 3; ++pl) U[x * 3 * cc + fo + pl * 512] = h[pl];
    }
}

// split form of a 1x1 tail weight, packed [n][k] -> [n >> 5][k >> 4][plane][lane = ((k >> 3) & 1) * 32 + (n & 31)][k & 7]:
// the A fragment of v_mfma_f32_32x32x16_bf16
__global__ void split_1x1_kernel(const float* __restrict__ w, int c, __bf16* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c * c) return;
    const int n = i / c, k = i % c;
    __bf16 h[3];
    split3_f64((double)w[i], h);
    const int64_t fo = ((int64_t)(n >> 5) * (c / 16) + (k >> 4)) * 3 * 512 + (((k >> 3) & 1) * 32 + (n & 31)) * 8 + (k & 7);
    for (int pl = 0; pl < 3; ++pl) out[fo + pl * 512] = h[pl];
}

}  // namespace

namespace vqae {

// C = 32 on the 128-wide grid keeps F(2x2, 3x3) and its smaller rounding error: that level is bound by HBM and vector issue,
// and the 30 % fewer MFMAs of F(4x4, 3x3) bought nothing there (675 us either way)
bool wino43_channels(int c) { return c == 256 || c == 128 || c == 64; }

// geometry only; whether a handle uses this form at all is decided when it is created (VQAE_WINO43=0: F(2x2, 3x3) everywhere)
bool wino43_supported(int c, int h, int w, int dtype) {
    return dtype == VQAE_DT_F32 && wino43_channels(c) && w == (c == 64 ? 64 : 32) && h >= 8 && h % 8 == 0;
}
bool wino43_enabled() { return env_int("VQAE_WINO43", 1) != 0; }

size_t wino43_weight_floats(int c) { return (size_t)36 * c * c; }

// The split (bf16x6) form serves C = 128 only: C = 64 and 256 keep the fp32 matrix instruction.
// VQAE_W43_SPLIT=0 (read once per handle) keeps it at C = 128 too.
bool wino43_split_supported(int c) { return c == 128; }
size_t wino43_split_weight_bytes(int c) { return (size_t)36 * c * c * 3 * 2; }
size_t split_1x1_bytes(int c) { return (size_t)c * c * 3 * 2; }

int wino43_split_weight(const float* w_oihw_dev, int c, void* U_dev, hipStream_t stream) {
    VQAE_REQUIRE(wino43_split_supported(c), VQAE_ERR_UNSUPPORTED, "wino43_split_weight: C = %d", c);
    wino43_split_weight_kernel<<<(unsigned)ceil_div(c * c, 256), 256, 0, stream>>>(w_oihw_dev, c, (__bf16*)U_dev);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

int split_1x1_weight(const float* w_packed_dev, int c, void* out_dev, hipStream_t stream) {
    VQAE_REQUIRE(wino43_split_supported(c), VQAE_ERR_UNSUPPORTED, "split_1x1_weight: C = %d", c);
    split_1x1_kernel<<<(unsigned)ceil_div(c * c, 256), 256, 0, stream>>>(w_packed_dev, c, (__bf16*)out_dev);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

int wino43_transform_weight(const float* w_oihw_dev, int c, float* U_dev, hipStream_t stream) {
    VQAE_REQUIRE(wino43_channels(c), VQAE_ERR_UNSUPPORTED, "wino43_transform_weight: C = %d", c);
    wino43_weight_kernel<<<(unsigned)ceil_div(c * c, 256), 256, 0, stream>>>(w_oihw_dev, c, U_dev);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

template <int C, bool SPLIT, bool WIDE = false>
static int launch_w43(W43K& k, int64_t M, bool chain, hipStream_t stream) {
    using K = W43Cfg<C, WIDE>;
    constexpr int lds = SPLIT ? K::LDS_SPLIT : K::LDS_BYTES;
    if (int rc = set_max_dynamic_lds((const void*)wino43_trunk_kernel<C, 1, SPLIT, WIDE>, lds)) return rc;
    if (int rc = set_max_dynamic_lds((const void*)wino43_trunk_kernel<C, 2, SPLIT, WIDE>, lds)) return rc;
    const unsigned grid = (unsigned)(M / (K::ROWS * K::W));
    // executed matrix work: 36 GEMMs of K = C per 16 output pixels (K_eff = 2.25 C per pixel) + the 1x1 tails, priced as fp32 work
    // in both forms (the split form executes 3x these products on the bf16 pipe)
    const double flops = 2.0 * (double)M * C * (2.25 * C + C + (chain ? C : 0));
    ProfScope prof(C >= 128 ? PROF_CONV3X3_TRUNK : PROF_NONE, stream, flops);
    if (chain) wino43_trunk_kernel<C, 2, SPLIT, WIDE><<<grid, K::NT, lds, stream>>>(k);
    else wino43_trunk_kernel<C, 1, SPLIT, WIDE><<<grid, K::NT, lds, stream>>>(k);
    prof.done();
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

int wino43_trunk_tail(const float* t1, const float* U, const float* w3, float act_a, float act_b, float t_scale, float t_b4,
                      float* xio, const NextConv1& next, int batch, int h, int w, int c, hipStream_t stream,
                      const void* Us, const void* w3s) {
    if (batch == 0) return VQAE_OK;
    const float* w1n = (const float*)next.w1;
    float* t1_next = (float*)next.t1_next;
    VQAE_REQUIRE(t1 && U && w3 && xio && (!w1n || t1_next), VQAE_ERR_INVALID, "wino43_trunk_tail: null pointer");
    VQAE_REQUIRE(wino43_supported(c, h, w, VQAE_DT_F32), VQAE_ERR_UNSUPPORTED, "wino43_trunk_tail: C = %d, H = %d, W = %d", c, h, w);
    const int64_t M = (int64_t)batch * h * w;
    VQAE_REQUIRE(M < (1ll << 31) - 1024, VQAE_ERR_UNSUPPORTED, "wino43_trunk_tail: too many pixels");
    W43K k;
    memset(&k, 0, sizeof(k));
    k.t1 = t1; k.U = U; k.w3 = w3; k.w1n = w1n; k.xio = xio; k.y2 = t1_next;
    k.H = h; k.M = (int)M;
    k.act_a = act_a; k.act_b = act_b; k.t_scale = t_scale; k.t_b4 = t_b4;
    k.n_b1a = next.b1a; k.n_b1b = next.b1b; k.n_b2a = next.b2a; k.n_b2b = next.b2b;
    if (Us) {
        VQAE_REQUIRE(wino43_split_supported(c) && w3s && (!w1n || next.w1s), VQAE_ERR_INVALID, "wino43_trunk_tail: split form needs C = 128 and its three weights");
        k.Us = (const float*)Us; k.w3s = (const float*)w3s; k.w1ns = (const float*)next.w1s;
        if (h % 16 == 0) return launch_w43<128, true, true>(k, M, w1n != nullptr, stream);   // 16-row workgroups: every weight fragment once per CU
        return launch_w43<128, true>(k, M, w1n != nullptr, stream);
    }
    switch (c) {
        case 256: return launch_w43<256, false>(k, M, w1n != nullptr, stream);
        case 128: return launch_w43<128, false>(k, M, w1n != nullptr, stream);
        default: return launch_w43<64, false>(k, M, w1n != nullptr, stream);
    }
}

}  // namespace vqae
