// Trainable zero-padded 3x3 convolutions with one THIN side of 3 channels (vqae_conv3x3z_train_*): the stems (model.py:198,
// :291: 3 -> C0 and C0 -> 3, zero padding 1, bias) and the skip_conv of an 'out' block (conv_block.py:211 with out2d.yaml:
// C -> 3, zero padding 1, no bias), fp32, NHWC, with the op in front of the conv folded in:
//     y[b][h][w][co] = bias[co] + sum_{kh,kw,ci} uz[b][h + kh - 1][w + kw - 1][ci] w[co][ci][kh][kw]
//     pre = 0: u = x      pre = 1: u = x + *b (b read from DEVICE memory);      uz = u inside the image, 0 OUTSIDE
// The padding comes after the pre-op (F.conv2d(x + c, w, padding=1) pads zeros, not c): an out-of-image tap is a select on the
// staged value, never a branch.  A GEMM with N = 3 or K = 27 would waste nine tenths of a 32-wide MFMA tile, and the fp32 MFMA runs
// at the vector rate on gfx950 anyway: these are direct convs on the vector ALU, bound by the bytes of the wide side.
//
// Channel rule: exactly one side is 3.  Ci = 3 with Co a multiple of 8 in 8 .. 64; Co = 3 with Ci a multiple of 8 in 8 .. 256.
// C names the wide side, t < 3 a thin channel, tap = 3 kh + kw.  w is read as it lies, by strides (w_layout 0 [Co][Ci][3][3],
// 1 [Co][3][3][Ci]); the data gradient reads tap 8 - tap (the flipped kernel): no permuted or flipped copy is written.
//
// Three kernels.  A workgroup of 256 threads owns tiles of 8 x 32 pixels of one image (grid-stride over the tiles, at most 1024
// workgroups); the input pixels of a tile with their one-pixel rim, 10 x 34, go through LDS once, pre-op and zero select applied
// there; rim positions are clamped for the load, so every address read lies inside the tensor.
//
//   zt_wide_to_thin   out[p][t] = bias[t] + sum_{tap,c} inz[p + tap][c] wk[tap][c][t]: the forward of Co = 3 (in = x) and the data
//                     gradient of Ci = 3 (in = g, flipped taps).  The wide input is staged in chunks of 32 channels by 16-byte
//                     loads, each element read once per tile; the chunk's weights lie next to it; thread = pixel, 3 accumulators.
//   zt_thin_to_wide   out[p][c] = bias[c] + sum_{tap,t} inz[p + tap][t] wk[tap][t][c]: the forward of Ci = 3 (in = x) and the data
//                     gradient of Co = 3 (in = g, flipped taps).  The thin tile (10 x 34 x 3 floats) and the whole weight (27 C
//                     floats) stay in LDS; thread = (pixel, group of 4 channels), consecutive lanes write consecutive 16 bytes:
//                     the wide output is written once, by 16-byte stores.
//   zt_wgrad          g_w = sum_q wide[q][c] thinz[q +- tap][t] (the wide side is g for Ci = 3, u for Co = 3) and
//                     g_bias = sum_q g[q][co].  A run is two tiles, at most ZT_RUN = 512 rows; workgroup p of P takes runs
//                     p, p + P, ...  The thin side of a tile goes through LDS with its rim; thread (s, c) of the 256 / C
//                     sub-lanes takes the tile's pixels s, s + 256 / C, ..., reads its wide element once and keeps
//                     27 + 1 fp32 sums; the sub-lanes are added in index order through LDS and the run goes into the workgroup's
//                     OWN fp64 slot (plain store on the first run: no clearing).  The final launch (ct_wgrad_final of
//                     conv_train.hip, through kernels.h) adds the P slots in index order in fp64, rounds once and writes the
//                     weight's layout; the same for the bias slots.
//
// Determinism: every grid is a function of (B, H, W, Ci, Co) alone, there are no floating-point atomics, every sum has one fixed
// order.  g_c = sum g_x (pre = 1): thread (fp64, index order) -> wave shuffle -> 4 waves in order -> one fp64 row per workgroup
// -> ct_sum_final (one workgroup, one rounding), as in fixup_train.hip.  An output passed as NULL launches nothing of its own.
//
// Workspace (backward only): [slots P 27 C doubles][bias slots P Co doubles][1024 rows of two doubles] + 256 bytes, with
// P <= 1024 and P 27 C <= 2^21: at most 16 MiB + 0.5 MiB + 16 KiB + 256 bytes, below 16.6 MiB whatever B, H, W are.
#include <algorithm>

#include "kernels.h"
#include "mfma.h"

namespace {

using namespace vqae;

constexpr int ZT_THREADS = 256;
constexpr int ZT_TH = 8, ZT_TW = 32;                 // pixels of a tile: one per thread
constexpr int ZT_PH = ZT_TH + 2, ZT_PW = ZT_TW + 2;  // with the rim
constexpr int ZT_KC = 32;                            // wide channels staged per chunk
constexpr int ZT_LD = ZT_KC + 4;                     // floats per staged pixel: 16-byte aligned, neighbours on other banks
constexpr int ZT_MAX_WG = 1024;                      // workgroups of a tile kernel = fp64 rows of the scalar sum
constexpr int ZT_RUN_TILES = 2;                      // tiles of a run of the weight gradient
constexpr int ZT_RUN = ZT_RUN_TILES * ZT_TH * ZT_TW; // = 512: longest fp32 accumulation run of g_w / g_bias, in rows
constexpr int ZT_SLOTS = 1024;                       // P <= ZT_SLOTS and P 27 C <= ZT_SLOT_ELEMS
constexpr int64_t ZT_SLOT_ELEMS = 1 << 21;
constexpr int ZT_ACC = 28;                           // 27 weight sums + the bias sum
constexpr int ZT_MAXC = 256;

// w[c * sC + t * sT + tap' * sTap], tap' = 8 - tap for the data gradient
struct WAddr {
    int sC, sT, sTap, flip;
    __host__ __device__ __forceinline__ int at(int tap, int c, int t) const { return c * sC + t * sT + (flip ? 8 - tap : tap) * sTap; }
};

struct TileGeo { int H, W, tiles_w; int64_t per_image, n_tiles; };

// tile -> its image and first pixel
__device__ __forceinline__ void tile_pos(int64_t tile, const TileGeo& g, int64_t* img, int* h0, int* w0) {
    const int64_t b = tile / g.per_image, r = tile - b * g.per_image, th = r / g.tiles_w;
    *img = b;
    *h0 = (int)th * ZT_TH;
    *w0 = (int)(r - th * g.tiles_w) * ZT_TW;
}

// the workgroup's fp64 sum -> its row of the partials (second column 0: ct_sum_final adds pairs)
__device__ __forceinline__ void block_partial(double s, double* __restrict__ partials) {
    __shared__ double red[ZT_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[(int64_t)blockIdx.x * 2 + 0] = ((red[0] + red[1]) + red[2]) + red[3];
        partials[(int64_t)blockIdx.x * 2 + 1] = 0.0;
    }
}

template <bool SUM>
__global__ __launch_bounds__(ZT_THREADS)
void zt_wide_to_thin(const float* __restrict__ in, const float* __restrict__ pb, int pre, const float* __restrict__ w, WAddr wa,
                     const float* __restrict__ bias, TileGeo geo, int C, float* __restrict__ out, double* __restrict__ partials) {
    __shared__ __attribute__((aligned(16))) float tile[ZT_PH * ZT_PW * ZT_LD];
    __shared__ __attribute__((aligned(16))) float wl[9 * ZT_KC * 3];           // the chunk's weights [tap][c][t]
    const int tid = threadIdx.x, ty = tid >> 5, tx = tid & 31;
    const int H = geo.H, W = geo.W;
    const float b = pre == 1 ? *pb : 0.f;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    double s = 0.0;
    for (int64_t t_i = blockIdx.x; t_i < geo.n_tiles; t_i += gridDim.x) {
        int64_t img;
        int h0, w0;
        tile_pos(t_i, geo, &img, &h0, &w0);
        float acc[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[t] = bias ? bias[t] : 0.f;
        for (int c0 = 0; c0 < C; c0 += ZT_KC) {
            const int kc = std::min(ZT_KC, C - c0), g4 = kc >> 2;
            __syncthreads();                                                      // the previous chunk has been read
            for (int i = tid; i < ZT_PH * ZT_PW * g4; i += ZT_THREADS) {
                const int pix = i / g4, q = i - pix * g4, py = pix / ZT_PW, px = pix - py * ZT_PW;
                const int h = h0 + py - 1, x = w0 + px - 1;
                const bool ok = h >= 0 && h < H && x >= 0 && x < W;
                const int hc = std::min(std::max(h, 0), H - 1), xc = std::min(std::max(x, 0), W - 1);
                f32x4 v = *reinterpret_cast<const f32x4*>(in + ((img * H + hc) * W + xc) * C + c0 + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] + b;
                *reinterpret_cast<f32x4*>(tile + pix * ZT_LD + 4 * q) = ok ? v : zero4;   // zero AFTER the pre-op
            }
            for (int i = tid; i < 9 * kc * 3; i += ZT_THREADS) {
                const int tap = i / (kc * 3), r = i - tap * kc * 3, cc = r / 3;
                wl[i] = w[wa.at(tap, c0 + cc, r - cc * 3)];
            }
            __syncthreads();
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float* ap = tile + ((ty + tap / 3) * ZT_PW + tx + tap % 3) * ZT_LD;
                const float* wp = wl + tap * kc * 3;
                for (int q = 0; q < g4; ++q) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(ap + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int t = 0; t < 3; ++t) acc[t] = __builtin_fmaf(a[e], wp[(4 * q + e) * 3 + t], acc[t]);
                }
            }
        }
        const int h = h0 + ty, x = w0 + tx;
        if (h < H && x < W) {
            if (out) {
                float* o = out + ((img * H + h) * W + x) * 3;
#pragma unroll
                for (int t = 0; t < 3; ++t) o[t] = acc[t];
            }
            if (SUM) s += ((double)acc[0] + (double)acc[1]) + (double)acc[2];
        }
    }
    if (SUM) block_partial(s, partials);
}

template <bool SUM>
__global__ __launch_bounds__(ZT_THREADS)
void zt_thin_to_wide(const float* __restrict__ in, const float* __restrict__ pb, int pre, const float* __restrict__ w, WAddr wa,
                     const float* __restrict__ bias, TileGeo geo, int C, float* __restrict__ out, double* __restrict__ partials) {
    __shared__ __attribute__((aligned(16))) float wl[27 * ZT_MAXC];           // [tap][t][c]
    __shared__ float tile[ZT_PH * ZT_PW * 3];
    const int tid = threadIdx.x;
    const int H = geo.H, W = geo.W, G = C >> 2;
    const float b = pre == 1 ? *pb : 0.f;
    for (int i = tid; i < 27 * C; i += ZT_THREADS) {
        const int k = i / C, tap = k / 3;
        wl[i] = w[wa.at(tap, i - k * C, k - tap * 3)];
    }
    double s = 0.0;
    for (int64_t t_i = blockIdx.x; t_i < geo.n_tiles; t_i += gridDim.x) {
        int64_t img;
        int h0, w0;
        tile_pos(t_i, geo, &img, &h0, &w0);
        __syncthreads();                                                          // the previous tile has been read (and wl written)
        for (int i = tid; i < ZT_PH * ZT_PW * 3; i += ZT_THREADS) {
            const int pix = i / 3, py = pix / ZT_PW, px = pix - py * ZT_PW;
            const int h = h0 + py - 1, x = w0 + px - 1;
            const bool ok = h >= 0 && h < H && x >= 0 && x < W;
            const int hc = std::min(std::max(h, 0), H - 1), xc = std::min(std::max(x, 0), W - 1);
            const float v = in[((img * H + hc) * W + xc) * 3 + (i - pix * 3)] + b;
            tile[i] = ok ? v : 0.f;                                               // zero AFTER the pre-op
        }
        __syncthreads();
        for (int i = tid; i < ZT_THREADS * G; i += ZT_THREADS) {
            const int pix = i / G, cg = i - pix * G, ty = pix >> 5, tx = pix & 31;
            f32x4 acc = bias ? *reinterpret_cast<const f32x4*>(bias + 4 * cg) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float* ap = tile + ((ty + tap / 3) * ZT_PW + tx + tap % 3) * 3;
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const float a = ap[t];
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + (tap * 3 + t) * C + 4 * cg);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(a, wv[e], acc[e]);
                }
            }
            const int h = h0 + ty, x = w0 + tx;
            if (h < H && x < W) {
                if (out) *reinterpret_cast<f32x4*>(out + ((img * H + h) * W + x) * C + 4 * cg) = acc;
                if (SUM) s += (((double)acc[0] + (double)acc[1]) + (double)acc[2]) + (double)acc[3];
            }
        }
    }
    if (SUM) block_partial(s, partials);
}

// WIDE_G true (Ci = 3):  wide = g [M][C = Co], thin = x: slot[(c 9 + tap) 3 + t] += g[q][c] uz[q + tap][t]; bias slot[c] += g[q][c]
// WIDE_G false (Co = 3): wide = x [M][C = Ci], thin = g: slot[(t 9 + tap) C + c] += u[q][c] gz[q - tap][t]; bias slot[t] += g[q][t]
// (the second form is the first with the sum re-indexed by the input pixel: g outside the image counts as zero)
// A run is ZT_RUN_TILES = 2 tiles, at most ZT_RUN = 512 rows.  The thin side of a tile, with its rim, is staged in LDS as in
// zt_thin_to_wide; the wide side is read once from global memory, lane = channel.
template <bool WIDE_G>
__global__ __launch_bounds__(ZT_THREADS)
void zt_wgrad(const float* __restrict__ wide, const float* __restrict__ thin, const float* __restrict__ pb, int pre, TileGeo geo,
              int C, int n_bias, double* __restrict__ slots, double* __restrict__ bslots) {
    __shared__ float red[ZT_THREADS * ZT_ACC];                                    // [sub][k][c]
    __shared__ float tile[ZT_PH * ZT_PW * 3];
    const int tid = threadIdx.x, nsub = ZT_THREADS / C, sub = tid / C, c = tid - sub * C;
    const int H = geo.H, W = geo.W;
    const bool active = sub < nsub;
    const float b = pre == 1 ? *pb : 0.f, bw = WIDE_G ? 0.f : b, bt = WIDE_G ? b : 0.f;
    const int64_t n_runs = (geo.n_tiles + ZT_RUN_TILES - 1) / ZT_RUN_TILES;
    double* slot = slots + (int64_t)blockIdx.x * 27 * C;
    double* bslot = bslots + (int64_t)blockIdx.x * n_bias;
    bool first = true;
    for (int64_t run = blockIdx.x; run < n_runs; run += gridDim.x) {
        float acc[ZT_ACC];
#pragma unroll
        for (int k = 0; k < ZT_ACC; ++k) acc[k] = 0.f;
        for (int64_t t_i = run * ZT_RUN_TILES; t_i < std::min(geo.n_tiles, (run + 1) * ZT_RUN_TILES); ++t_i) {
            int64_t img;
            int h0, w0;
            tile_pos(t_i, geo, &img, &h0, &w0);
            __syncthreads();                                                      // the previous tile has been read
            for (int i = tid; i < ZT_PH * ZT_PW * 3; i += ZT_THREADS) {
                const int pix = i / 3, py = pix / ZT_PW, px = pix - py * ZT_PW;
                const int h = h0 + py - 1, x = w0 + px - 1;
                const bool ok = h >= 0 && h < H && x >= 0 && x < W;
                const int hc = std::min(std::max(h, 0), H - 1), xc = std::min(std::max(x, 0), W - 1);
                const float v = thin[((img * H + hc) * W + xc) * 3 + (i - pix * 3)] + bt;
                tile[i] = ok ? v : 0.f;                                           // zero AFTER the pre-op
            }
            __syncthreads();
            if (active) {
                for (int d = sub; d < ZT_TH * ZT_TW; d += nsub) {
                    const int ty = d >> 5, tx = d & 31, h = h0 + ty, x = w0 + tx;
                    if (h >= H || x >= W) continue;
                    const float wv = wide[((img * H + h) * W + x) * C + c] + bw;
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) {
                        const int kh = WIDE_G ? tap / 3 : 2 - tap / 3, kw = WIDE_G ? tap % 3 : 2 - tap % 3;
                        const float* tp = tile + ((ty + kh) * ZT_PW + tx + kw) * 3;
#pragma unroll
                        for (int t = 0; t < 3; ++t) acc[tap * 3 + t] = __builtin_fmaf(wv, tp[t], acc[tap * 3 + t]);
                    }
                    const float* ctr = tile + ((ty + 1) * ZT_PW + tx + 1) * 3;
                    acc[27] += WIDE_G ? wv : ctr[c < 3 ? c : 0];
                }
            }
        }
        if (active) {
#pragma unroll
            for (int k = 0; k < ZT_ACC; ++k) red[(sub * ZT_ACC + k) * C + c] = acc[k];
        }
        __syncthreads();
        for (int i = tid; i < ZT_ACC * C; i += ZT_THREADS) {
            const int k = i / C, cc = i - k * C;
            float v = red[k * C + cc];
            for (int sb = 1; sb < nsub; ++sb) v += red[(sb * ZT_ACC + k) * C + cc];
            double* sp = nullptr;
            if (k < 27) {
                const int tap = k / 3, t = k - tap * 3;
                sp = slot + (WIDE_G ? (cc * 9 + tap) * 3 + t : (t * 9 + tap) * C + cc);
            } else if (cc < n_bias) {
                sp = bslot + cc;
            }
            if (sp) *sp = first ? (double)v : *sp + (double)v;
        }
        __syncthreads();
        first = false;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
inline bool supported(int cin, int cout) {
    if (cin == 3) return cout >= 8 && cout <= 64 && cout % 8 == 0;
    if (cout == 3) return cin >= 8 && cin <= ZT_MAXC && cin % 8 == 0;
    return false;
}

// rows M = batch h w when the geometry is valid and M < 2^40, else 0
inline int64_t rows(int64_t b, int h, int w) {
    if (b < 1 || h < 1 || w < 1) return 0;
    const int64_t per = (int64_t)h * w;
    return per < (1ll << 40) && b <= (1ll << 40) / per && b * per < (1ll << 40) ? b * per : 0;
}

inline TileGeo tile_geo(int64_t b, int h, int w) {
    TileGeo g;
    g.H = h;
    g.W = w;
    g.tiles_w = (int)ceil_div(w, ZT_TW);
    g.per_image = ceil_div(h, ZT_TH) * g.tiles_w;
    g.n_tiles = b * g.per_image;                          // <= b h w < 2^40
    return g;
}
inline int tile_grid(const TileGeo& g) { return (int)std::min<int64_t>(ZT_MAX_WG, g.n_tiles); }

inline int wgrad_slots(const TileGeo& g, int wide) {
    const int64_t pmax = std::min<int64_t>(ZT_SLOTS, ZT_SLOT_ELEMS / (27 * (int64_t)wide));
    return (int)std::min<int64_t>(pmax, ceil_div(g.n_tiles, ZT_RUN_TILES));
}

inline WAddr waddr(int cin, int w_layout, bool flip) {
    WAddr a;
    if (cin == 3) {                                       // c = co, t = ci
        a.sC = 27;
        a.sT = w_layout ? 1 : 9;
        a.sTap = w_layout ? 3 : 1;
    } else {                                              // c = ci, t = co
        a.sC = w_layout ? 1 : 9;
        a.sT = 9 * cin;
        a.sTap = w_layout ? cin : 1;
    }
    a.flip = flip ? 1 : 0;
    return a;
}

struct Workspace { double* slots; double* bslots; double* partials; };
inline Workspace carve(void* ws, int P, int wide, int cout) {
    Workspace o;
    o.slots = (double*)ws;
    o.bslots = o.slots + (size_t)P * 27 * wide;
    o.partials = o.bslots + (size_t)P * cout;
    return o;
}

// The checks both entries share, in the order of conv_train.hip's entry_checks: geometry, pre, w_layout, null pointers, the
// channel rule (pre = 2 has no caller at this seat: unsupported), 2^40 rows; the caller checks the alignment last.
inline int entry_checks(const char* op, bool pointers, int pre, int w_layout, const float* b, int64_t batch, int h, int wd, int cin,
                        int cout, int64_t* m) {
    *m = rows(batch, h, wd);
    VQAE_REQUIRE(batch >= 1 && h >= 1 && wd >= 1, VQAE_ERR_INVALID, "conv3x3z_train_%s: batch %lld h %d w %d", op, (long long)batch,
                 h, wd);
    VQAE_REQUIRE(pre >= 0 && pre <= 2, VQAE_ERR_INVALID, "conv3x3z_train_%s: pre %d", op, pre);
    VQAE_REQUIRE(w_layout >= 0 && w_layout <= 1, VQAE_ERR_INVALID, "conv3x3z_train_%s: w_layout %d", op, w_layout);
    VQAE_REQUIRE(pointers && (pre < 1 || b), VQAE_ERR_INVALID, "conv3x3z_train_%s: null pointer", op);
    VQAE_REQUIRE(supported(cin, cout), VQAE_ERR_UNSUPPORTED,
                 "conv3x3z_train_%s: cin %d cout %d (one side 3; the other a multiple of 8: cout 8 .. 64, cin 8 .. %d)", op, cin, cout,
                 ZT_MAXC);
    VQAE_REQUIRE(pre != 2, VQAE_ERR_UNSUPPORTED, "conv3x3z_train_%s: pre 2 (ELU) is not built for the zero-padded conv", op);
    VQAE_REQUIRE(*m >= 1, VQAE_ERR_INVALID, "conv3x3z_train_%s: batch %lld x %d x %d rows exceed 2^40", op, (long long)batch, h, wd);
    return VQAE_OK;
}

}  // namespace

// ---- the C ABI ---------------------------------------------------------------------------------------------------------------
extern "C" int vqae_conv3x3z_train_supported(int cin, int cout) { return supported(cin, cout) ? 1 : 0; }
extern "C" int vqae_conv3x3z_train_wgrad_run(void) { return ZT_RUN; }
extern "C" size_t vqae_conv3x3z_train_workspace_bytes(int64_t batch, int h, int w, int cin, int cout) {
    const int64_t m = rows(batch, h, w);
    if (m < 1 || !supported(cin, cout)) return 0;
    const int wide = cin == 3 ? cout : cin;
    return ((size_t)wgrad_slots(tile_geo(batch, h, w), wide) * (27 * wide + cout) + (size_t)ZT_MAX_WG * 2) * sizeof(double) + 256;
}

extern "C" int vqae_conv3x3z_train_forward_f32(const float* x, const float* a, const float* b, int pre, const float* w,
                                               const float* bias, int w_layout, int64_t batch, int h, int wd, int cin, int cout,
                                               float* y, void* ws, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int64_t m;
    (void)a;
    (void)ws;
    if (const int e = entry_checks("forward", x && w && y, pre, w_layout, b, batch, h, wd, cin, cout, &m)) return e;
    VQAE_REQUIRE(aligned16({x, w, bias, y}), VQAE_ERR_INVALID, "conv3x3z_train_forward: x, w, bias and y must be 16-byte aligned");
    const TileGeo geo = tile_geo(batch, h, wd);
    const WAddr wa = waddr(cin, w_layout, false);
    if (cin == 3)
        zt_thin_to_wide<false><<<tile_grid(geo), ZT_THREADS, 0, stream>>>(x, b, pre, w, wa, bias, geo, cout, y, nullptr);
    else
        zt_wide_to_thin<false><<<tile_grid(geo), ZT_THREADS, 0, stream>>>(x, b, pre, w, wa, bias, geo, cin, y, nullptr);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

extern "C" int vqae_conv3x3z_train_backward_f32(const float* g, const float* x, const float* a, const float* b, int pre,
                                                const float* w, int w_layout, int64_t batch, int h, int wd, int cin, int cout,
                                                float* g_x, float* g_w, float* g_a, float* g_b, float* g_bias, void* ws,
                                                void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int64_t m;
    (void)a;
    (void)g_a;                                            // pre = 2 alone has a g_a
    if (const int e = entry_checks("backward", g && x && w && ws, pre, w_layout, b, batch, h, wd, cin, cout, &m)) return e;
    VQAE_REQUIRE(aligned16({g, x, w, g_x, g_w, g_bias}) && ((uintptr_t)ws & 7) == 0, VQAE_ERR_INVALID,
                 "conv3x3z_train_backward: tensors must be 16-byte aligned, the workspace 8-byte aligned");
    const TileGeo geo = tile_geo(batch, h, wd);
    const int wide = cin == 3 ? cout : cin, P = wgrad_slots(geo, wide);
    const Workspace wk = carve(ws, P, wide, cout);
    float* o_c = pre == 1 ? g_b : nullptr;
    if (g_x || o_c) {
        const WAddr wa = waddr(cin, w_layout, true);
        const int grid = tile_grid(geo);
        if (cin == 3) {
            if (o_c) zt_wide_to_thin<true><<<grid, ZT_THREADS, 0, stream>>>(g, nullptr, 0, w, wa, nullptr, geo, cout, g_x, wk.partials);
            else zt_wide_to_thin<false><<<grid, ZT_THREADS, 0, stream>>>(g, nullptr, 0, w, wa, nullptr, geo, cout, g_x, nullptr);
        } else {
            if (o_c) zt_thin_to_wide<true><<<grid, ZT_THREADS, 0, stream>>>(g, nullptr, 0, w, wa, nullptr, geo, cin, g_x, wk.partials);
            else zt_thin_to_wide<false><<<grid, ZT_THREADS, 0, stream>>>(g, nullptr, 0, w, wa, nullptr, geo, cin, g_x, nullptr);
        }
        VQAE_LAUNCH_CHECK();
        if (o_c)
            if (const int e = conv_train_sum_final(wk.partials, grid, o_c, nullptr, stream)) return e;
    }
    if (g_w || g_bias) {
        if (cin == 3) zt_wgrad<true><<<P, ZT_THREADS, 0, stream>>>(g, x, b, pre, geo, wide, cout, wk.slots, wk.bslots);
        else zt_wgrad<false><<<P, ZT_THREADS, 0, stream>>>(x, g, b, pre, geo, wide, cout, wk.slots, wk.bslots);
        VQAE_LAUNCH_CHECK();
        if (g_w)
            if (const int e = conv_train_wgrad_final(wk.slots, P, 27 * wide, cin, 9, w_layout, g_w, stream)) return e;
        if (g_bias)
            if (const int e = conv_train_wgrad_final(wk.bslots, P, cout, 1, 1, 1, g_bias, stream)) return e;
    }
    return VQAE_OK;
}
