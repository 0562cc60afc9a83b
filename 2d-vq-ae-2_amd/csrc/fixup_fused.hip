// Fused Fixup "same" block for the high-resolution, small-channel levels (C = 8 / 16 / 32):
//   y = conv3(ELU(conv2(ELU(conv1(ELU(x+b1a)+b1b)+b2a)+b2b)+b3a)+b3b)*scale + b4 + x
// (reference vq_ae/layers/conv_block.py:196-216, mode 'same': 1x1 -> 3x3 circular -> 1x1) in ONE kernel.
//
// Unfused, these levels are HBM-bound: the activation tensors are 8x larger than at the 32x32 trunk
// (C*H*W = 1 M floats per patch) and a block makes 7 passes over them.  Here a workgroup owns a
// TH x 32 pixel tile of one image: it computes conv1 on the (TH+2) x 34 halo straight from global
// memory (operand fragments loaded in MFMA layout, Fixup pre-op applied in registers), keeps t1 in LDS,
// runs the 9 taps of the 3x3 from that LDS tile (no re-staging), writes t2 over t1, runs conv3 and adds
// the residual: algorithmic HBM traffic = one read + one write of the activation (+ halo rows).
// All three weight matrices stay resident in LDS ([n][k] rows, +4 float pad: conflict-free
// ds_read_b128 fragments); workgroups are persistent and walk tiles in an XCD-contiguous order.
#include "common.h"
#include "mfma.h"

namespace {

using namespace vqae;

// autocast rounding point: compiled in only for the 16-bit instantiations (p.dt picks bf16 / f16)
#define RND(v) (R16 ? vqae::round_dt((v), p.dt) : (v))


struct FusedP {
    const float* __restrict__ x;
    float* __restrict__ y;
    const float* __restrict__ w1;   // packed [>=32][C]
    const float* __restrict__ w2;   // packed [>=32][9C]
    const float* __restrict__ w3;   // packed [>=32][C]
    int B, H, W;
    int tiles_x, tiles_y, n_tiles;
    float b1a, b1b, b2a, b2b, b3a, b3b, b4, scale;
    int dt;                              // VQAE_DT_*: autocast rounding points
};


template <int C, int TH>
struct FusedCfg {
    static constexpr int LDT = C + 4;                  // t1 / t2 row stride (floats)
    static constexpr int LDW2 = 9 * C + 4;             // W2 row stride
    static constexpr int HP = (TH + 2) * 34;           // halo pixels
    static constexpr int HPP = (HP + 31) / 32 * 32;
    static constexpr int G1 = HPP / 32;                // 32-pixel groups of the halo (conv1 M tiles)
    static constexpr int GPW = (G1 + 3) / 4;           // per wave
    static constexpr int MPW = TH / 4;                 // output image rows (M tiles) per wave
    static constexpr int LDS_FLOATS = 2 * 32 * LDT + 32 * LDW2 + HPP * LDT;
    // 16x16x4 kernel: 16 weight rows per matrix and exactly HP halo rows: 39.2 KB at C = 16 -> four workgroups per CU
    static constexpr int LDS_FLOATS_TINY = 2 * 16 * LDT + 16 * LDW2 + HP * LDT;
};

template <int C, int TH, bool R16>
__global__ __launch_bounds__(256, (C <= 16 ? 3 : 2))
void fixup_same_small_kernel(const FusedP p) {
    using K = FusedCfg<C, TH>;
    constexpr int LDT = K::LDT, LDW2 = K::LDW2, HP = K::HP, G1 = K::G1, GPW = K::GPW, MPW = K::MPW;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const W1s = lds;
    float* const W3s = W1s + 32 * LDT;
    float* const W2s = W3s + 32 * LDT;
    float* const T1 = W2s + 32 * LDW2;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, h = lane >> 5;

    // weights -> LDS, once per (persistent) workgroup
    for (int i = tid; i < 32 * (C / 4); i += 256) {
        const int n = i / (C / 4), c4 = i % (C / 4);
        *reinterpret_cast<f32x4*>(W1s + n * LDT + 4 * c4) = *reinterpret_cast<const f32x4*>(p.w1 + n * C + 4 * c4);
        *reinterpret_cast<f32x4*>(W3s + n * LDT + 4 * c4) = *reinterpret_cast<const f32x4*>(p.w3 + n * C + 4 * c4);
    }
    for (int i = tid; i < 32 * (9 * C / 4); i += 256) {
        const int n = i / (9 * C / 4), c4 = i % (9 * C / 4);
        *reinterpret_cast<f32x4*>(W2s + n * LDW2 + 4 * c4) = *reinterpret_cast<const f32x4*>(p.w2 + n * 9 * C + 4 * c4);
    }
    __syncthreads();

    // XCD-contiguous tile ranges: blocks b, b+8, ... share an XCD (L2); give each XCD a contiguous run of
    // tiles so the halo rows of neighbouring tiles hit in one L2 (speed only).
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3, per_xcd_wg = (nwg + 7 - xcd) >> 3;
    const int q = p.n_tiles >> 3, rr = p.n_tiles & 7;
    const int xcd_lo = xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q;
    const int xcd_n = q + (xcd < rr ? 1 : 0);

    const float* const w1f = W1s + li * LDT + 4 * h;
    const float* const w3f = W3s + li * LDT + 4 * h;
    const float* const w2f = W2s + li * LDW2 + 4 * h;

    for (int t = slot; t < xcd_n; t += per_xcd_wg) {
        const int tile = xcd_lo + t;
        const int txi = tile % p.tiles_x;
        const int tyi = (tile / p.tiles_x) % p.tiles_y;
        const int b = tile / (p.tiles_x * p.tiles_y);
        const int ty0 = tyi * TH, tx0 = txi * 32;
        const float* const xim = p.x + (int64_t)b * p.H * p.W * C;

        // ---- P1: t1 = ELU(conv1(ELU(x+b1a)+b1b) + b2a) + b2b on the halo ---------------------------
#pragma unroll
        for (int gi = 0; gi < GPW; ++gi) {
            const int g = wave + 4 * gi;
            if (g < G1) {
                int hp = 32 * g + li;
                hp = hp < HP ? hp : HP - 1;
                const int hy = hp / 34, hx = hp - 34 * hy;
                int iy = ty0 + hy - 1, ix = tx0 + hx - 1;
                iy = iy < 0 ? iy + p.H : (iy >= p.H ? iy - p.H : iy);
                ix = ix < 0 ? ix + p.W : (ix >= p.W ? ix - p.W : ix);
                const float* src = xim + ((int64_t)iy * p.W + ix) * C + 4 * h;
                f32x4 a[C / 8];
#pragma unroll
                for (int u = 0; u < C / 8; ++u) a[u] = *reinterpret_cast<const f32x4*>(src + 8 * u);
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
                for (int u = 0; u < C / 8; ++u) {
                    f32x4 v = a[u] + p.b1a;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = RND(elu_act(v[e]) + p.b1b);
                    const f32x4 bw = *reinterpret_cast<const f32x4*>(w1f + 8 * u);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[r], bw[r], acc, 0, 0, 0);
                }
                if (li < C) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                        T1[(32 * g + row) * LDT + li] = RND(elu_act(RND(acc[r]) + p.b2a) + p.b2b);
                    }
                }
            }
        }
        __syncthreads();

        // ---- P2: 3x3 circular conv straight from the LDS halo tile --------------------------------
        f32x16 acc2[MPW];
#pragma unroll
        for (int mt = 0; mt < MPW; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[mt][r] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap % 3;
#pragma unroll
            for (int u = 0; u < C / 8; ++u) {
                const f32x4 bw = *reinterpret_cast<const f32x4*>(w2f + tap * C + 8 * u);
#pragma unroll
                for (int mt = 0; mt < MPW; ++mt) {
                    const int ry = wave + 4 * mt;
                    const f32x4 av = *reinterpret_cast<const f32x4*>(T1 + ((ry + dy) * 34 + li + dx) * LDT + 8 * u + 4 * h);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        acc2[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r], bw[r], acc2[mt], 0, 0, 0);
                }
            }
        }
        __syncthreads();                               // every wave is done reading t1
        if (li < C) {
#pragma unroll
            for (int mt = 0; mt < MPW; ++mt) {
                const int ry = wave + 4 * mt;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                    T1[(ry * 32 + row) * LDT + li] = RND(elu_act(RND(acc2[mt][r]) + p.b3a) + p.b3b);   // t2 over t1
                }
            }
        }
        __syncthreads();

        // ---- P3: conv3 (1x1) + scale/bias4 + residual ----------------------------------------------
#pragma unroll
        for (int mt = 0; mt < MPW; ++mt) {
            const int ry = wave + 4 * mt;
            f32x16 acc3;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc3[r] = 0.f;
#pragma unroll
            for (int u = 0; u < C / 8; ++u) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(T1 + (ry * 32 + li) * LDT + 8 * u + 4 * h);
                const f32x4 bw = *reinterpret_cast<const f32x4*>(w3f + 8 * u);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r], bw[r], acc3, 0, 0, 0);
            }
            if (li < C) {
                const int64_t rowbase = (((int64_t)b * p.H + ty0 + ry) * p.W + tx0) * C + li;
                float res[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) res[r] = p.x[rowbase + ((r & 3) + 8 * (r >> 2) + 4 * h) * C];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float tv = RND(acc3[r]) * p.scale;
                    tv = tv + p.b4;
                    tv = tv + res[r];
                    p.y[rowbase + ((r & 3) + 8 * (r >> 2) + 4 * h) * C] = tv;
                }
            }
        }
        __syncthreads();                               // t2 is dead: the next tile may overwrite the LDS tile
    }
}

template <int C, int TH, bool R16>
int launch_fused_r(FusedP& p, hipStream_t stream) {
    using K = FusedCfg<C, TH>;
    constexpr int lds_bytes = K::LDS_FLOATS * (int)sizeof(float);
    if (int rc = vqae::set_max_dynamic_lds((const void*)fixup_same_small_kernel<C, TH, R16>, lds_bytes)) return rc;
    p.tiles_x = p.W / 32;
    p.tiles_y = p.H / TH;
    p.n_tiles = p.B * p.tiles_x * p.tiles_y;
    const int per_cu = (C <= 16 ? 3 : 2);
    int grid = 256 * per_cu;
    if (grid > p.n_tiles) grid = p.n_tiles;
    fixup_same_small_kernel<C, TH, R16><<<grid, 256, lds_bytes, stream>>>(p);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

// ------------------------------------------------------------------------------------------------
// C = 8 / 16: same structure on v_mfma_f32_16x16x4_f32 (A[i = l&15][k = l>>4], B[k = l>>4][j = l&15],
// D: col = l&15, row = 4*(l>>4) + reg).  A 16-wide N tile wastes nothing at C = 16 (the 32x32x2 form
// pads N to 32: half the matrix work and half of every epilogue lane were idle) and half at C = 8.
// Lane (i, q) reads KQ = C/4 consecutive channels at KQ*q and feeds them to KQ MFMAs; the k-th
// MFMA sums channels {KQ*q' + k : q' = 0..3}, identically permuted for A and B.  Launched at C = 16 (the 16-bit modes
// and VQAE_NO_WINO16); C = 8 runs on the VALU kernel below, which measured faster.
// ------------------------------------------------------------------------------------------------

template <int C> struct KVec;
template <> struct KVec<16> { typedef f32x4 type; };
template <> struct KVec<8> { typedef f32x2 type; };

template <int C, int TH, bool R16>
__global__ __launch_bounds__(256, 4)
void fixup_same_tiny_kernel(const FusedP p) {
    using K = FusedCfg<C, TH>;
    using kvec = typename KVec<C>::type;
    constexpr int KQ = C / 4;                           // channels per lane per fragment (4 or 2)
    constexpr int LDT = K::LDT, LDW2 = K::LDW2, HP = K::HP;
    constexpr int G1 = K::HPP / 16;                     // 16-pixel groups of the halo
    constexpr int GPW = (G1 + 3) / 4;
    constexpr int MPW = TH / 4;                         // image rows per wave; 2 M tiles (16 px) each
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const W1s = lds;                             // [16][LDT]
    float* const W3s = W1s + 16 * LDT;
    float* const W2s = W3s + 16 * LDT;                  // [16][LDW2]
    float* const T1 = W2s + 16 * LDW2;                  // [HP][LDT]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, q = lane >> 4;

    for (int i = tid; i < 16 * (C / 4); i += 256) {
        const int n = i / (C / 4), c4 = i % (C / 4);
        *reinterpret_cast<f32x4*>(W1s + n * LDT + 4 * c4) = *reinterpret_cast<const f32x4*>(p.w1 + n * C + 4 * c4);
        *reinterpret_cast<f32x4*>(W3s + n * LDT + 4 * c4) = *reinterpret_cast<const f32x4*>(p.w3 + n * C + 4 * c4);
    }
    for (int i = tid; i < 16 * (9 * C / 4); i += 256) {
        const int n = i / (9 * C / 4), c4 = i % (9 * C / 4);
        *reinterpret_cast<f32x4*>(W2s + n * LDW2 + 4 * c4) = *reinterpret_cast<const f32x4*>(p.w2 + n * 9 * C + 4 * c4);
    }
    __syncthreads();

    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3, per_xcd_wg = (nwg + 7 - xcd) >> 3;
    const int qq = p.n_tiles >> 3, rr = p.n_tiles & 7;
    const int xcd_lo = xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq;
    const int xcd_n = qq + (xcd < rr ? 1 : 0);

    const float* const w1f = W1s + li * LDT + KQ * q;
    const float* const w3f = W3s + li * LDT + KQ * q;
    const float* const w2f = W2s + li * LDW2 + KQ * q;
    // The weights are the MFMA's row operand, so the accumulator is D[channel 4q + r][pixel li]: a lane owns four
    // consecutive channels of one pixel and every LDS / global access of the epilogues is 128 bits wide.
    const bool c_ok = 4 * q < C;                          // C = 8: channel rows 8..15 are padding

    for (int t = slot; t < xcd_n; t += per_xcd_wg) {
        const int tile = xcd_lo + t;
        const int txi = tile % p.tiles_x;
        const int tyi = (tile / p.tiles_x) % p.tiles_y;
        const int b = tile / (p.tiles_x * p.tiles_y);
        const int ty0 = tyi * TH, tx0 = txi * 32;
        const float* const xim = p.x + (int64_t)b * p.H * p.W * C;

        // ---- P1 ------------------------------------------------------------------------------------
        const kvec w1v = *reinterpret_cast<const kvec*>(w1f);
#pragma unroll
        for (int gi = 0; gi < GPW; ++gi) {
            const int g = wave + 4 * gi;
            if (g < G1) {
                int hp = 16 * g + li;
                hp = hp < HP ? hp : HP - 1;
                const int hy = hp / 34, hx = hp - 34 * hy;
                int iy = ty0 + hy - 1, ix = tx0 + hx - 1;
                iy = iy < 0 ? iy + p.H : (iy >= p.H ? iy - p.H : iy);
                ix = ix < 0 ? ix + p.W : (ix >= p.W ? ix - p.W : ix);
                kvec v = *reinterpret_cast<const kvec*>(xim + ((int64_t)iy * p.W + ix) * C + KQ * q);
                v = v + p.b1a;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < KQ; ++k) {
                    const float av = RND(elu_act(v[k]) + p.b1b);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1v[k], av, acc, 0, 0, 0);   // D[channel 4q + r][pixel li]
                }
                if (c_ok && 16 * g + li < HP) {        // rows past the halo are padding of the last 16-pixel group
                    f32x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = RND(elu_act(RND(acc[r]) + p.b2a) + p.b2b);
                    *reinterpret_cast<f32x4*>(T1 + (16 * g + li) * LDT + 4 * q) = o;
                }
            }
        }
        __syncthreads();

        // ---- P2 ------------------------------------------------------------------------------------
        f32x4 acc2[MPW][2];
#pragma unroll
        for (int mt = 0; mt < MPW; ++mt)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) acc2[mt][hf] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap % 3;
            const kvec bw = *reinterpret_cast<const kvec*>(w2f + tap * C);
#pragma unroll
            for (int mt = 0; mt < MPW; ++mt) {
                const int ry = wave + 4 * mt;
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    const kvec av = *reinterpret_cast<const kvec*>(T1 + ((ry + dy) * 34 + 16 * hf + li + dx) * LDT + KQ * q);
#pragma unroll
                    for (int k = 0; k < KQ; ++k)
                        acc2[mt][hf] = __builtin_amdgcn_mfma_f32_16x16x4f32(bw[k], av[k], acc2[mt][hf], 0, 0, 0);
                }
            }
        }
        __syncthreads();
        if (c_ok) {
#pragma unroll
            for (int mt = 0; mt < MPW; ++mt)
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    f32x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = RND(elu_act(RND(acc2[mt][hf][r]) + p.b3a) + p.b3b);
                    *reinterpret_cast<f32x4*>(T1 + ((wave + 4 * mt) * 32 + 16 * hf + li) * LDT + 4 * q) = o;   // t2 over t1
                }
        }
        __syncthreads();

        // ---- P3 ------------------------------------------------------------------------------------
        const kvec w3v = *reinterpret_cast<const kvec*>(w3f);
#pragma unroll
        for (int mt = 0; mt < MPW; ++mt) {
            const int ry = wave + 4 * mt;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const kvec av = *reinterpret_cast<const kvec*>(T1 + (ry * 32 + 16 * hf + li) * LDT + KQ * q);
                f32x4 acc3 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < KQ; ++k) acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(w3v[k], av[k], acc3, 0, 0, 0);
                if (c_ok) {                             // lane: pixel li, channels 4q .. 4q+3 -> one 128-bit load / store
                    const int64_t base = (((int64_t)b * p.H + ty0 + ry) * p.W + tx0 + 16 * hf + li) * C + 4 * q;
                    const f32x4 res = *reinterpret_cast<const f32x4*>(p.x + base);
                    f32x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float tv = RND(acc3[r]) * p.scale;
                        tv = tv + p.b4;
                        o[r] = tv + res[r];
                    }
                    *reinterpret_cast<f32x4*>(p.y + base) = o;
                }
            }
        }
        __syncthreads();
    }
}

template <int C, int TH, bool R16>
int launch_tiny_r(FusedP& p, hipStream_t stream) {
    using K = FusedCfg<C, TH>;
    constexpr int lds_bytes = K::LDS_FLOATS_TINY * (int)sizeof(float);
    if (int rc = vqae::set_max_dynamic_lds((const void*)fixup_same_tiny_kernel<C, TH, R16>, lds_bytes)) return rc;
    p.tiles_x = p.W / 32;
    p.tiles_y = p.H / TH;
    p.n_tiles = p.B * p.tiles_x * p.tiles_y;
    int grid = 256 * 4;
    if (grid > p.n_tiles) grid = p.n_tiles;
    fixup_same_tiny_kernel<C, TH, R16><<<grid, 256, lds_bytes, stream>>>(p);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

// ------------------------------------------------------------------------------------------------
// C = 16, fp32 (round 3): the same block with conv2 as Winograd F(2x2, 3x3), everything after conv1 in REGISTERS.
// The kernel above runs 728 v_mfma_f32_16x16x4_f32 per 8 x 32 tile (88 conv1 on the halo + 576 conv2 + 64 conv3) -- at the
// 256 x 256 level of cfg B (2.1 GB moved per block: 0.3 ms of HBM) the fp32 matrix pipe is the bound (0.6 ms at 100 %; measured
// 1.12 ms).  F(2x2, 3x3) needs 16 multiplies per 2 x 2 outputs instead of 36: conv2 becomes 256 MFMAs, 408 in all.
// What makes it cheap here is the operand layout of the 16x16x4 MFMA with the weights as the ROW operand: lane (li, q) feeds
// B[k = q][column li] = 4 channels (4 q ..) of "column" li and receives D[4 q + r][li] = 4 output channels of the same column.
// With column = one 2 x 2 Winograd tile (a wave owns one tile row: 16 tiles) a lane
//   * reads the 4 x 4 input patch of ITS tile and ITS 4 channels from the t1 halo in LDS (16 x ds_read_b128),
//   * forms B^T d B in registers (adds only): the 16 transformed values ARE the B operands of the 16 position GEMMs,
//   * folds the 16 products through A^T . A into the 2 x 2 outputs (adds only), applies ELU: 4 pixels x 4 channels in the
//     layout conv3's B operand wants, runs conv3 per sub-pixel, adds the residual and stores 16 bytes per pixel.
// No LDS traffic and no barrier between conv1 and the store; U = G g G^T (16 x [16 x 16], 16 KiB) is built once per
// (persistent) workgroup and read as linear 1 KiB fragments.  Results differ from the direct form by fp32 rounding only.
template <int TH, bool PF>
__global__ __launch_bounds__(256, 3)
void fixup_same_wino16_kernel(const FusedP p) {
    constexpr int C = 16;
    using K = FusedCfg<C, TH>;
    constexpr int LDT = K::LDT, HP = K::HP;
    constexpr int G1 = K::HPP / 16;                     // 16-pixel groups of the halo
    constexpr int GPW = (G1 + 3) / 4;
    static_assert(TH == 8, "a wave owns one Winograd tile row: 4 waves x 2 image rows");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const W1s = lds;                             // [16][LDT]
    float* const W3s = W1s + 16 * LDT;
    float* const Us = W3s + 16 * LDT;                   // [16 pos][16 n][16 k]
    float* const T1 = Us + 16 * 256;                    // [HP][LDT]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, q = lane >> 4;

    for (int i = tid; i < 16 * (C / 4); i += 256) {
        const int n = i / (C / 4), c4 = i % (C / 4);
        *reinterpret_cast<f32x4*>(W1s + n * LDT + 4 * c4) = *reinterpret_cast<const f32x4*>(p.w1 + n * C + 4 * c4);
        *reinterpret_cast<f32x4*>(W3s + n * LDT + 4 * c4) = *reinterpret_cast<const f32x4*>(p.w3 + n * C + 4 * c4);
    }
    {   // U[xi * 4 + nu][n][k] = (G g G^T)[xi][nu],  g = w2[n][tap][k],  G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]
        const int n = tid >> 4, k = tid & 15;
        float g[3][3], t[4][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) g[a][b] = p.w2[n * 9 * C + (3 * a + b) * C + k];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            t[0][b] = g[0][b];
            t[1][b] = 0.5f * (g[0][b] + g[1][b] + g[2][b]);
            t[2][b] = 0.5f * (g[0][b] - g[1][b] + g[2][b]);
            t[3][b] = g[2][b];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            Us[(a * 4 + 0) * 256 + tid] = t[a][0];
            Us[(a * 4 + 1) * 256 + tid] = 0.5f * (t[a][0] + t[a][1] + t[a][2]);
            Us[(a * 4 + 2) * 256 + tid] = 0.5f * (t[a][0] - t[a][1] + t[a][2]);
            Us[(a * 4 + 3) * 256 + tid] = t[a][2];
        }
    }
    __syncthreads();

    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3, per_xcd_wg = (nwg + 7 - xcd) >> 3;
    const int qq = p.n_tiles >> 3, rr = p.n_tiles & 7;
    const int xcd_lo = xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq;
    const int xcd_n = qq + (xcd < rr ? 1 : 0);

    const f32x4 w1v = *reinterpret_cast<const f32x4*>(W1s + li * LDT + 4 * q);
    const f32x4 w3v = *reinterpret_cast<const f32x4*>(W3s + li * LDT + 4 * q);
    const float* const uf = Us + li * 16 + 4 * q;       // + pos * 256: one linear KiB per wave-wide read
    const float* const dp = T1 + ((2 * wave) * 34 + 2 * li) * LDT + 4 * q;   // this lane's 4 x 4 patch: + (i * 34 + j) * LDT

    f32x4 xin[GPW];
    auto p1_load = [&](int tile_, f32x4 (&dst)[GPW]) {
        const int txi_ = tile_ % p.tiles_x;
        const int tyi_ = (tile_ / p.tiles_x) % p.tiles_y;
        const int b_ = tile_ / (p.tiles_x * p.tiles_y);
        const float* const xim_ = p.x + (int64_t)b_ * p.H * p.W * C;
#pragma unroll
        for (int gi = 0; gi < GPW; ++gi) {
            int g = wave + 4 * gi;
            g = g < G1 ? g : G1 - 1;
            int hp = 16 * g + li;
            hp = hp < HP ? hp : HP - 1;
            const int hy = hp / 34, hx = hp - 34 * hy;
            int iy = tyi_ * TH + hy - 1, ix = txi_ * 32 + hx - 1;
            iy = iy < 0 ? iy + p.H : (iy >= p.H ? iy - p.H : iy);
            ix = ix < 0 ? ix + p.W : (ix >= p.W ? ix - p.W : ix);
            dst[gi] = *reinterpret_cast<const f32x4*>(xim_ + ((int64_t)iy * p.W + ix) * C + 4 * q);
        }
    };
    for (int t = slot; t < xcd_n; t += per_xcd_wg) {
        const int tile = xcd_lo + t;
        const int txi = tile % p.tiles_x;
        const int tyi = (tile / p.tiles_x) % p.tiles_y;
        const int b = tile / (p.tiles_x * p.tiles_y);
        const int ty0 = tyi * TH, tx0 = txi * 32;

        // ---- P1: t1 = ELU(conv1(ELU(x + b1a) + b1b) + b2a) + b2b on the (TH + 2) x 34 halo -> LDS --------------------------------
        // PF: the halo rows were requested during the previous tile's conv2 / conv3 (xin); else they are requested here
        if (!PF || t == slot) p1_load(tile, xin);
#pragma unroll
        for (int gi = 0; gi < GPW; ++gi) {
            const int g = wave + 4 * gi;
            if (g < G1) {
                f32x4 v = xin[gi] + p.b1a;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float av = elu_act(v[k]) + p.b1b;
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1v[k], av, acc, 0, 0, 0);   // D[channel 4q + r][pixel li]
                }
                if (16 * g + li < HP) {                 // rows past the halo are padding of the last 16-pixel group
                    f32x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = elu_act(acc[r] + p.b2a) + p.b2b;
                    *reinterpret_cast<f32x4*>(T1 + (16 * g + li) * LDT + 4 * q) = o;
                }
            }
        }
        // residual pixels of this lane's 2 x 2 tile: requested now, used after conv3
        const int64_t pix = (((int64_t)b * p.H + ty0 + 2 * wave) * p.W + tx0 + 2 * li) * C + 4 * q;
        f32x4 res[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) res[a][bb] = *reinterpret_cast<const f32x4*>(p.x + pix + ((int64_t)a * p.W + bb) * C);
        __syncthreads();                                // t1 complete

        // ---- P2: conv2 = A^T [ sum_c U .* (B^T d B) ] A, from registers --------------------------------------------------------------
        f32x4 d[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) d[i][j] = *reinterpret_cast<const f32x4*>(dp + (i * 34 + j) * LDT);
        __syncthreads();                                // every wave holds its patches: the next tile's conv1 may overwrite t1
        if (PF && t + per_xcd_wg < xcd_n) p1_load(xcd_lo + t + per_xcd_wg, xin);   // in flight under conv2 / conv3 of this tile
        f32x4 y00 = {0.f, 0.f, 0.f, 0.f}, y01 = y00, y10 = y00, y11 = y00;
#pragma unroll
        for (int xi = 0; xi < 4; ++xi) {
            // row xi of B^T d:  B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
            f32x4 c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                c[j] = xi == 0 ? d[0][j] - d[2][j] : (xi == 1 ? d[1][j] + d[2][j] : (xi == 2 ? d[2][j] - d[1][j] : d[1][j] - d[3][j]));
            f32x4 v[4];
            v[0] = c[0] - c[2];
            v[1] = c[1] + c[2];
            v[2] = c[2] - c[1];
            v[3] = c[1] - c[3];
#pragma unroll
            for (int nu = 0; nu < 4; ++nu) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(uf + (4 * xi + nu) * 256);
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 4; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(u[k], v[nu][k], acc, 0, 0, 0);
                // fold: Y[a][b] += A^T[a][xi] * A^T[b][nu] * acc,  A^T = [1 1 1 0; 0 1 -1 -1]
                const int ca0 = xi <= 2 ? 1 : 0, ca1 = xi == 0 ? 0 : (xi == 1 ? 1 : -1);
                const int cb0 = nu <= 2 ? 1 : 0, cb1 = nu == 0 ? 0 : (nu == 1 ? 1 : -1);
                if (ca0 * cb0 != 0) y00 = y00 + acc;
                if (ca0 * cb1 == 1) y01 = y01 + acc; else if (ca0 * cb1 == -1) y01 = y01 - acc;
                if (ca1 * cb0 == 1) y10 = y10 + acc; else if (ca1 * cb0 == -1) y10 = y10 - acc;
                if (ca1 * cb1 == 1) y11 = y11 + acc; else if (ca1 * cb1 == -1) y11 = y11 - acc;
            }
        }
        // ---- P3: t2 = ELU(conv2 + b3a) + b3b (already conv3's B operand), conv3, * scale + bias4 + x -> global ----------------------
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const f32x4 yv = a == 0 ? (bb == 0 ? y00 : y01) : (bb == 0 ? y10 : y11);
                f32x4 acc3 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float tv = elu_act(yv[k] + p.b3a) + p.b3b;
                    acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(w3v[k], tv, acc3, 0, 0, 0);
                }
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float tv = acc3[r] * p.scale;
                    tv = tv + p.b4;
                    o[r] = tv + res[a][bb][r];
                }
                *reinterpret_cast<f32x4*>(p.y + pix + ((int64_t)a * p.W + bb) * C) = o;
            }
    }
}

template <int TH>
int launch_wino16(FusedP& p, hipStream_t stream) {
    using K = FusedCfg<16, TH>;
    constexpr int lds_bytes = (2 * 16 * K::LDT + 16 * 256 + K::HP * K::LDT) * (int)sizeof(float);
    if (int rc = vqae::set_max_dynamic_lds((const void*)fixup_same_wino16_kernel<TH, true>, lds_bytes)) return rc;
    p.tiles_x = p.W / 32;
    p.tiles_y = p.H / TH;
    p.n_tiles = p.B * p.tiles_x * p.tiles_y;
    int grid = 256 * 3;
    if (grid > p.n_tiles) grid = p.n_tiles;
    // PF: the next tile's halo rows are requested under this tile's conv2 / conv3 (24 registers): 0.88 -> 0.82 ms
    fixup_same_wino16_kernel<TH, true><<<grid, 256, lds_bytes, stream>>>(p);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

// ------------------------------------------------------------------------------------------------
// C = 8 (stem-width level of the reference default model, 512x512 resolution): a VALU kernel.  With 8 channels an
// MFMA tile is mostly padding (16x16x4: half of N, two k-steps per tap) and the block's 704 MACs per pixel fit the
// vector ALUs: one thread per output pixel, t1 of the (TH+2) x 34 halo in LDS, the 704 weights in LDS too (read as
// wave-uniform 128-bit broadcasts), t2 and conv3 stay in registers.  Same rounding points as the MFMA form.
// ------------------------------------------------------------------------------------------------
template <int DT>                                                        // autocast rounding points compiled in
__global__ __launch_bounds__(256)
void fixup_same_c8_kernel(const FusedP p) {
    auto RC = [](float v) -> float {
        if (DT == VQAE_DT_BF16) return (float)(__bf16)v;
        if (DT == VQAE_DT_F16) return (float)(_Float16)v;
        return v;
    };
    constexpr int TH = 8, HP = (TH + 2) * 34, LDP = 12;              // LDS pixel stride (floats): 48 B, fewer bank conflicts
    __shared__ __attribute__((aligned(16))) float T1[HP * LDP];
    __shared__ __attribute__((aligned(16))) float Wl[8 * 8 + 8 * 72 + 8 * 8];
    const int tid = threadIdx.x;
    // packed weights: rows = output channels; w1 [8][8], w2 [8][72] (k = tap * 8 + ci), w3 [8][8]
    for (int i = tid; i < 704; i += 256) Wl[i] = i < 64 ? p.w1[i] : (i < 640 ? p.w2[i - 64] : p.w3[i - 640]);
    const float* const w1 = Wl;
    const float* const w2 = Wl + 64;
    const float* const w3 = Wl + 640;
    __syncthreads();
    for (int tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        const int txi = tile % p.tiles_x;
        const int tyi = (tile / p.tiles_x) % p.tiles_y;
        const int b = tile / (p.tiles_x * p.tiles_y);
        const int ty0 = tyi * TH, tx0 = txi * 32;
        const float* const xim = p.x + (int64_t)b * p.H * p.W * 8;
        // ---- P1: t1 = ELU(conv1(ELU(x + b1a) + b1b) + b2a) + b2b on the halo --------------------------------------
        for (int hp = tid; hp < HP; hp += 256) {
            const int hy = hp / 34, hx = hp - 34 * hy;
            int iy = ty0 + hy - 1, ix = tx0 + hx - 1;
            iy = iy < 0 ? iy + p.H : (iy >= p.H ? iy - p.H : iy);
            ix = ix < 0 ? ix + p.W : (ix >= p.W ? ix - p.W : ix);
            const f32x4* src = reinterpret_cast<const f32x4*>(xim + ((int64_t)iy * p.W + ix) * 8);
            const f32x4 a0 = src[0], a1 = src[1];
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = a0[e]; v[4 + e] = a1[e]; }
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = RC(elu_act(v[k] + p.b1a) + p.b1b);
            f32x4 o0, o1;
#pragma unroll
            for (int co = 0; co < 8; ++co) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc = __builtin_fmaf(v[k], w1[co * 8 + k], acc);
                const float t = RC(elu_act(RC(acc) + p.b2a) + p.b2b);
                if (co < 4) o0[co] = t; else o1[co - 4] = t;
            }
            *reinterpret_cast<f32x4*>(T1 + hp * LDP) = o0;
            *reinterpret_cast<f32x4*>(T1 + hp * LDP + 4) = o1;
        }
        __syncthreads();
        // ---- P2 + P3: one output pixel per thread ------------------------------------------------------------------
        {
            const int py = tid >> 5, px = tid & 31;
            float acc[8];
#pragma unroll
            for (int co = 0; co < 8; ++co) acc[co] = 0.f;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float* tp = T1 + ((py + tap / 3) * 34 + px + tap % 3) * LDP;
                const f32x4 t0 = *reinterpret_cast<const f32x4*>(tp), t1v = *reinterpret_cast<const f32x4*>(tp + 4);
                float tv[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) { tv[e] = t0[e]; tv[4 + e] = t1v[e]; }
#pragma unroll
                for (int co = 0; co < 8; ++co)
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[co] = __builtin_fmaf(tv[k], w2[co * 72 + tap * 8 + k], acc[co]);
            }
            float t2[8];
#pragma unroll
            for (int co = 0; co < 8; ++co) t2[co] = RC(elu_act(RC(acc[co]) + p.b3a) + p.b3b);
            const int64_t o = (((int64_t)b * p.H + ty0 + py) * p.W + tx0 + px) * 8;
            const f32x4 r0 = *reinterpret_cast<const f32x4*>(p.x + o), r1 = *reinterpret_cast<const f32x4*>(p.x + o + 4);
            f32x4 y0, y1;
#pragma unroll
            for (int co = 0; co < 8; ++co) {
                float a3 = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) a3 = __builtin_fmaf(t2[k], w3[co * 8 + k], a3);
                float tv = RC(a3) * p.scale;
                tv = tv + p.b4;
                tv = tv + (co < 4 ? r0[co] : r1[co - 4]);
                if (co < 4) y0[co] = tv; else y1[co - 4] = tv;
            }
            *reinterpret_cast<f32x4*>(p.y + o) = y0;
            *reinterpret_cast<f32x4*>(p.y + o + 4) = y1;
        }
        __syncthreads();                               // t1 is dead: the next tile may overwrite it
    }
}

int launch_c8(FusedP& p, hipStream_t stream) {
    p.tiles_x = p.W / 32;
    p.tiles_y = p.H / 8;
    p.n_tiles = p.B * p.tiles_x * p.tiles_y;
    int grid = 256 * 8;
    if (grid > p.n_tiles) grid = p.n_tiles;
    if (p.dt == VQAE_DT_BF16) fixup_same_c8_kernel<VQAE_DT_BF16><<<grid, 256, 0, stream>>>(p);
    else if (p.dt == VQAE_DT_F16) fixup_same_c8_kernel<VQAE_DT_F16><<<grid, 256, 0, stream>>>(p);
    else fixup_same_c8_kernel<VQAE_DT_F32><<<grid, 256, 0, stream>>>(p);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

template <int C, int TH>
int launch_fused(FusedP& p, hipStream_t stream) {
    return p.dt ? launch_fused_r<C, TH, true>(p, stream) : launch_fused_r<C, TH, false>(p, stream);
}
template <int C, int TH>
int launch_tiny(FusedP& p, hipStream_t stream) {
    return p.dt ? launch_tiny_r<C, TH, true>(p, stream) : launch_tiny_r<C, TH, false>(p, stream);
}
#undef RND

}  // namespace

extern "C" int vqae_fixup_same_supported(int c, int h, int w) {
    if (w % 32 != 0) return 0;
    if (c == 8 || c == 16) return h % 8 == 0;
    if (c == 32) return h % 4 == 0;
    return 0;
}

extern "C" int vqae_fixup_same_block_f32(const float* x, float* y, const float* w1_packed, const float* w2_packed,
                                         const float* w3_packed, int batch, int h, int w, int c,
                                         const float* scalars8, int dtype, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VQAE_REQUIRE(scalars8, VQAE_ERR_INVALID, "fixup_same_block: null scalars");
    if (batch == 0) return VQAE_OK;
    VQAE_REQUIRE(x && y && w1_packed && w2_packed && w3_packed, VQAE_ERR_INVALID, "fixup_same_block: null pointer");
    VQAE_REQUIRE(x != y, VQAE_ERR_INVALID, "fixup_same_block: in-place is not supported (halo reads)");
    VQAE_REQUIRE(vqae_fixup_same_supported(c, h, w), VQAE_ERR_UNSUPPORTED,
                 "fixup_same_block: unsupported shape C=%d H=%d W=%d", c, h, w);
    FusedP p;
    p.x = x; p.y = y; p.w1 = w1_packed; p.w2 = w2_packed; p.w3 = w3_packed;
    p.B = batch; p.H = h; p.W = w;
    p.b1a = scalars8[0]; p.b1b = scalars8[1]; p.b2a = scalars8[2]; p.b2b = scalars8[3];
    p.b3a = scalars8[4]; p.b3b = scalars8[5]; p.b4 = scalars8[6]; p.scale = scalars8[7];
    VQAE_REQUIRE(dtype >= VQAE_DT_F32 && dtype <= VQAE_DT_F16, VQAE_ERR_INVALID, "fixup_same_block: dtype %d", dtype);
    p.dt = dtype;
    if (c == 8) return launch_c8(p, stream);
    // fp32, C = 16: conv2 as Winograd F(2x2, 3x3) from registers (fixup_same_wino16_kernel); read per call so that tests can compare
    // the forms inside one process
    if (c == 16 && dtype == VQAE_DT_F32 && vqae::env_int("VQAE_NO_WINO16", 0) == 0) return launch_wino16<8>(p, stream);
    if (c == 16) return launch_tiny<16, 8>(p, stream);
    return launch_fused<32, 4>(p, stream);
}
