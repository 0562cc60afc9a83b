// fp32 'up' Fixup block in the conv-before-resize order of handle.hip (R_UP_CONV_FIRST{,_TAIL}) as two launches: the head
// (up_head_kernel, below: the three 1x1 convs at the low resolution) and, at the stem-side levels, the tail (up_tail_kernel):
//   out = conv3(ELU(bicubic_x2(q) + b3a) + b3b) * scale + b4 + bicubic_x2(s)
// q [B][H][W][CB] = branch_conv2 output at the low resolution, s [B][H][W][CO] = skip_conv output, out [B][2H][2W][CO].
// Unfused this is two resize launches that write 4x-larger tensors and a 1x1 conv that reads them back (8 GB per call
// at 256x256x32 for a batch of 256).
//
// Bicubic x2 (A = -0.75, align_corners = False, clamped indices) is separable: output o takes the four inputs i-2..i+1
// (o even, weights w75) or i-1..i+2 (o odd, w25) with i = o >> 1, and out = sum_i wy_i * (sum_j wx_j * v_ij), both sums
// left to right (first product, then three fmas).  A 256-thread workgroup owns 8 x 16 output pixels:
//   stage    the 8 x 12 low-resolution window (clamped indices) of q and of s -> LDS, every load requested before the
//            first store
//   rows     thread = (output column, channel quad): the 8 window rows interpolated horizontally ONCE each, kept in registers
//   columns  the same thread combines them for the tile's 8 output rows; branch values get the ELU -> Tb, skip values -> Ts
//   conv3    thread = (pixel, 4 output channels): CB x CO on v_mfma_f32_16x16x4_f32 from Tb (weights resident in registers for
//            the whole persistent launch), + scale / bias4 / resized skip from Ts, 128-bit stores.
// Per resized value that is 4 + 4 fmas (a window row per output row) and three quarters of a 128-bit load; the earlier form -- a
// thread per 2 x 2 output block that fetched and interpolated its own 4 x 4 window -- spent 4 + 8 and 4 loads, and was
// bound by vector issue.  Every value runs the chain it ran there on the same inputs: same bits.
// The window lies over Tb / Ts (it is dead once the row results are in registers), so LDS is what Tb and Ts take:
// 29 KB at (32, 16), 52 KB at (64, 32).
#include <type_traits>

#include "kernels.h"
#include "mfma.h"

namespace {

using namespace vqae;

// the (window pixel, channel quad) items of one tensor's window that this thread stages: global -> registers
template <int C, int WRN, int WCN, int NIT>
__device__ __forceinline__ void window_load(const float* __restrict__ img, int iy0, int jx0, int H, int W, int tid, f32x4 (&v)[NIT]) {
    constexpr int G = C / 4, NITEM = WRN * WCN * G;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        int idx = tid + 256 * i;
        idx = idx < NITEM ? idx : NITEM - 1;
        const int wp = idx / G, g = idx % G;
        int iy = iy0 - 2 + wp / WCN, ix = jx0 - 2 + wp % WCN;
        iy = iy < 0 ? 0 : (iy > H - 1 ? H - 1 : iy);
        ix = ix < 0 ? 0 : (ix > W - 1 ? W - 1 : ix);
        v[i] = *reinterpret_cast<const f32x4*>(img + ((int64_t)iy * W + ix) * C + 4 * g);
    }
}

// ... registers -> LDS [window pixel][L]
template <int C, int WRN, int WCN, int L, int NIT>
__device__ __forceinline__ void window_store(float* win, int tid, const f32x4 (&v)[NIT]) {
    constexpr int G = C / 4, NITEM = WRN * WCN * G;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int idx = tid + 256 * i;
        if (NITEM % 256 == 0 || idx < NITEM) *reinterpret_cast<f32x4*>(win + (idx / G) * L + 4 * (idx % G)) = v[i];
    }
}

template <int CB, int CO>
__global__ __launch_bounds__(256, CB == 64 ? 2 : 4)
void up_tail_kernel(const float* __restrict__ q, const float* __restrict__ sk, const float* __restrict__ w3, int B, int H,
                    int W, int tiles_x, int tiles_y, float b3a, float b3b, float scale, float b4, float* __restrict__ y) {
    constexpr int TR = 8, TC = 16;                                                  // output tile: rows x columns
    constexpr int WRN = TR / 2 + 4, WCN = TC / 2 + 4;                               // its low-resolution window
    constexpr int LB = CB + 4, LS = CO + 4, GB = CB / 4, GS = CO / 4;
    constexpr int NITEM = TC * (GB + GS), NI = (NITEM + 255) / 256;                 // (output column, channel quad) items, per thread
    constexpr int NLB = (WRN * WCN * GB + 255) / 256, NLS = (WRN * WCN * GS + 255) / 256;
    constexpr int NTL = (CO + 15) / 16;                                             // 16-channel output tiles (CO = 8: half a tile)
    static_assert(CB % 16 == 0 && CO % 4 == 0, "conv3 runs on 16x16x4 MFMA tiles");
    static_assert(TR * TC == 128 && WRN * WCN <= 128 && (TC * GB) % 64 == 0, "window under Tb / Ts; branch and skip items in separate waves");
    const float w75[4] = {-0.03515625f, 0.26171875f, 0.87890625f, -0.10546875f};   // even outputs (offset .75)
    const float w25[4] = {-0.10546875f, 0.87890625f, 0.26171875f, -0.03515625f};   // odd outputs  (offset .25)
    __shared__ __attribute__((aligned(16))) float Tb[128 * LB];                     // window of q [wp][LB], then ELU'd resized branch [pixel][ci]
    __shared__ __attribute__((aligned(16))) float Ts[128 * LS];                     // window of s [wp][LS], then resized skip [pixel][co]
    const int tid = threadIdx.x;
    // conv3 weights as the MFMA row operand, kept in registers for the whole (persistent) launch: lane (li, q) of n-tile nt, k-slice s
    // holds w3[co = 16 nt + li][ci = 16 s + 4 q .. + 3] (packed rows are [co][ci])
    float4 w3r[NTL][CB / 16];
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
        for (int s_ = 0; s_ < CB / 16; ++s_) {
            const int co = 16 * nt + (tid & 15);
            w3r[nt][s_] = co < CO ? *reinterpret_cast<const float4*>(w3 + co * CB + 16 * s_ + 4 * ((tid & 63) >> 4)) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    const int OW = 2 * W, OH = 2 * H;
    const int n_tiles = B * tiles_x * tiles_y;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int txi = tile % tiles_x;
        const int tyi = (tile / tiles_x) % tiles_y;
        const int64_t b = tile / (tiles_x * tiles_y);
        const int oy0 = TR * tyi, ox0 = TC * txi;                                   // first output pixel of the tile
        // ---- stage: the window's loads go out before the barrier, so they fly while the other waves finish the previous tile ---------
        f32x4 vb[NLB], vs[NLS];
        window_load<CB, WRN, WCN, NLB>(q + b * H * W * CB, oy0 >> 1, ox0 >> 1, H, W, tid, vb);
        window_load<CO, WRN, WCN, NLS>(sk + b * H * W * CO, oy0 >> 1, ox0 >> 1, H, W, tid, vs);
        lds_barrier();                                                             // previous tile's conv3 is done with Tb / Ts
        window_store<CB, WRN, WCN, LB, NLB>(Tb, tid, vb);
        window_store<CO, WRN, WCN, LS, NLS>(Ts, tid, vs);
        lds_barrier();
        // ---- rows: item = (output column c, channel quad); the first TC * GB items are the branch's (whole waves) ----------------------
        // lanes 0..15 of a quad read 9 window pixels whose 16-byte slots (9 p + g) mod 16 are distinct (L = C + 4): no bank conflict
        f32x4 h[NI][WRN];
#pragma unroll
        for (int ii = 0; ii < NI; ++ii) {
            const int it = tid + 256 * ii;
            if (NITEM % 256 != 0 && it >= NITEM) continue;
            const bool branch = it < TC * GB;
            const int c = it & (TC - 1), g = branch ? it / TC : it / TC - GB;
            const int L = branch ? LB : LS;
            const float* src = (branch ? Tb : Ts) + ((c >> 1) + (c & 1)) * L + 4 * g;
            const float* wx = (c & 1) ? w25 : w75;
            const float wx0 = wx[0], wx1 = wx[1], wx2 = wx[2], wx3 = wx[3];
#pragma unroll
            for (int wr = 0; wr < WRN; ++wr) {
                const float* p = src + wr * WCN * L;
                f32x4 a = *reinterpret_cast<const f32x4*>(p) * wx0;
                a = __builtin_elementwise_fma(*reinterpret_cast<const f32x4*>(p + L), (f32x4){wx1, wx1, wx1, wx1}, a);
                a = __builtin_elementwise_fma(*reinterpret_cast<const f32x4*>(p + 2 * L), (f32x4){wx2, wx2, wx2, wx2}, a);
                a = __builtin_elementwise_fma(*reinterpret_cast<const f32x4*>(p + 3 * L), (f32x4){wx3, wx3, wx3, wx3}, a);
                h[ii][wr] = a;
            }
        }
        lds_barrier();                                                             // every thread is done with the window
        // ---- columns: output row r takes row results (r >> 1) + (r & 1) .. + 3 ---------------------------------------------------------
#pragma unroll
        for (int ii = 0; ii < NI; ++ii) {
            const int it = tid + 256 * ii;
            if (NITEM % 256 != 0 && it >= NITEM) continue;
            const bool branch = it < TC * GB;
            const int c = it & (TC - 1), g = branch ? it / TC : it / TC - GB;
            float* dst = branch ? Tb + c * LB + 4 * g : Ts + c * LS + 4 * g;
            const int L = branch ? LB : LS;
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const int wrb = (r >> 1) + (r & 1);
                const float* wy = (r & 1) ? w25 : w75;
                f32x4 o = h[ii][wrb] * wy[0];
#pragma unroll
                for (int k = 1; k < 4; ++k) o = __builtin_elementwise_fma(h[ii][wrb + k], (f32x4){wy[k], wy[k], wy[k], wy[k]}, o);
                if (branch) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = elu_act(o[e] + b3a) + b3b;
                }
                *reinterpret_cast<f32x4*>(dst + r * TC * L) = o;
            }
        }
        lds_barrier();
        // ---- conv3 on the fp32 MFMA ----------------------------------------------------------------------------------------------------
        // v_mfma_f32_16x16x4_f32 with the weights as the row operand: lane (li, q) feeds Tb[pixel li][16 s + 4 q ..] and receives
        // D[4 q + r][li] = 4 consecutive output channels of its pixel -> 16-byte skip read and store.  A wave owns 2 groups of 16
        // pixels: two output rows of the tile.
        {
            const int lane = tid & 63, wv = tid >> 6;
            const int li = lane & 15, qd = lane >> 4;
#pragma unroll
            for (int gg = 0; gg < 2; ++gg) {
                const int px = 32 * wv + 16 * gg + li;
                const int oy = oy0 + (px >> 4), ox = ox0 + (px & 15);
                float4 tb[CB / 16];
#pragma unroll
                for (int s_ = 0; s_ < CB / 16; ++s_) tb[s_] = *reinterpret_cast<const float4*>(Tb + px * LB + 16 * s_ + 4 * qd);
#pragma unroll
                for (int nt = 0; nt < NTL; ++nt) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s_ = 0; s_ < CB / 16; ++s_) {
                        const float4 wv4 = w3r[nt][s_];
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.x, tb[s_].x, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.y, tb[s_].y, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.z, tb[s_].z, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.w, tb[s_].w, acc, 0, 0, 0);
                    }
                    if (oy < OH && ox < OW && 16 * nt + 4 * qd < CO) {
                        const float4 sp = *reinterpret_cast<const float4*>(Ts + px * LS + 16 * nt + 4 * qd);
                        float o[4];
                        const float sv[4] = {sp.x, sp.y, sp.z, sp.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float tv = acc[e] * scale;
                            tv = tv + b4;
                            o[e] = tv + sv[e];
                        }
                        *reinterpret_cast<float4*>(y + ((b * OH + oy) * OW + ox) * CO + 16 * nt + 4 * qd) = make_float4(o[0], o[1], o[2], o[3]);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The head: the block's three 1x1 convs at the low resolution in one launch.
//   Q  = skip_conv(x + b1c) + b1d                             C -> C / 2
//   t1 = ELU(conv1(ELU(x + b1a) + b1b) + b2a) + b2b           C -> C, LDS only
//   R  = conv2(t1)                                            C -> C
// As three generic launches x is read twice and t1 written only to be read back (2.95 GB at the stem-side level where the
// block needs 1.34 GB: read x, write R and Q).  A 256-thread workgroup owns 128 consecutive pixels, a wave 32 of them for
// all three GEMMs: its x rows are requested before any arithmetic (down_fused.hip phase 1 says why) and feed both pre-ops
// from the same registers; t1 goes accumulator -> LDS T1[px][C + 4] -> operand within the wave, so the launch has no
// workgroup barrier.  The GEMMs run on v_mfma_f32_32x32x2_f32 with the WEIGHTS as the row operand (fragment order, from L2,
// a ring of 4 fragments in flight), so a lane holds four consecutive channels of one pixel and every store is 128 bits.
// Every output element sees conv_mfma's sequence (MP<DT, false>::mma): 8-deep k-slices ascending, inside a slice MFMA r
// = 0..3 on the pair k = 8 u + r, 8 u + 4 + r, and the same pre-op / bias / activation expressions: same bits.
// ------------------------------------------------------------------------------------------------
struct UpHeadK {
    const float* __restrict__ x;         // [M][C]
    const float* __restrict__ w1;        // fragment order (frag_weight, k-slice 8): [C][C]
    const float* __restrict__ w2;        //   [C][C]
    const float* __restrict__ wsk;       //   [max(C / 2, 32)][C], rows past C / 2 zero
    float* __restrict__ q;               // [M][C / 2]
    float* __restrict__ r;               // [M][C]
    int64_t M;
    FixupScalars s;
};

template <int C>
__global__ __launch_bounds__(256, 2)
void up_head_kernel(const UpHeadK p) {
    constexpr int CO = C / 2;
    constexpr int KU = C / 8;                         // k-slices of every GEMM (K = C)
    constexpr int NT = C / 32, NTS = (CO + 31) / 32;  // 32-channel output tiles: conv1 / conv2, skip_conv
    constexpr int LD = C + 4;                         // T1 row stride (floats): lane li reads 16-byte slot li (C / 4 + 1) + .., odd stride
    constexpr int WR = 4;                             // weight fragments in flight
    extern __shared__ __attribute__((aligned(16))) float lds[];      // T1[128][LD]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, hh = lane >> 5;
    const int64_t m = (int64_t)blockIdx.x * 128 + 32 * wave + li;    // this lane's pixel
    const bool m_ok = m < p.M;                                       // the M tail re-reads the last pixel; its stores are dropped

    f32x4 xin[KU];
    {
        const float* src = p.x + (m_ok ? m : p.M - 1) * C + 4 * hh;
#pragma unroll
        for (int u = 0; u < KU; ++u) xin[u] = *reinterpret_cast<const f32x4*>(src + 8 * u);
    }
    // one GEMM of `ntiles` 32-channel tiles: fragments stream from w in the order they are used ([tile][k-slice][lane][4])
    auto gemm = [&](const float* __restrict__ w, auto ntiles, auto&& operand, auto&& epilogue) {
        constexpr int N = decltype(ntiles)::value * KU;
        static_assert(N >= WR, "the ring's first loads stay inside the matrix");
        const float* wl = w + 4 * lane;
        f32x4 wq[WR];
#pragma unroll
        for (int j = 0; j < WR; ++j) wq[j] = *reinterpret_cast<const f32x4*>(wl + 256 * j);
        f32x16 acc;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int ct = j / KU, u = j % KU;
            if (u == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            }
            const f32x4 wv = wq[j % WR];
            if (j + WR < N) wq[j % WR] = *reinterpret_cast<const f32x4*>(wl + 256 * (j + WR));
            const f32x4 v = operand(u);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[r], v[r], acc, 0, 0, 0);   // D[channel][pixel]
            if (u == KU - 1) epilogue(ct, acc);
        }
    };
    // ---- skip_conv ------------------------------------------------------------------------------------------------------
    gemm(p.wsk, std::integral_constant<int, NTS>(), [&](int u) { return xin[u] + p.s.b1c; }, [&](int ct, const f32x16& acc) {
        float* dst = p.q + m * CO + 32 * ct + 4 * hh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (32 * ct + 8 * g >= CO) continue;                    // CO = 16: half a tile
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = acc[4 * g + e] + p.s.b1d;
            if (m_ok) *reinterpret_cast<f32x4*>(dst + 8 * g) = o;
        }
    });
    // ---- conv1 -> T1 (rows of this wave's pixels) -----------------------------------------------------------------------
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) xin[u][e] = elu_act(xin[u][e] + p.s.b1a) + p.s.b1b;
    float* const trow = lds + (32 * wave + li) * LD + 4 * hh;
    gemm(p.w1, std::integral_constant<int, NT>(), [&](int u) { return xin[u]; }, [&](int ct, const f32x16& acc) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = elu_act(acc[4 * g + e] + p.s.b2a) + p.s.b2b;
            *reinterpret_cast<f32x4*>(trow + 32 * ct + 8 * g) = o;
        }
    });
    // ---- conv2 from T1 --------------------------------------------------------------------------------------------------
    gemm(p.w2, std::integral_constant<int, NT>(), [&](int u) { return *reinterpret_cast<const f32x4*>(trow + 8 * u); },
         [&](int ct, const f32x16& acc) {
        float* dst = p.r + m * C + 32 * ct + 4 * hh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 o = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
            if (m_ok) *reinterpret_cast<f32x4*>(dst + 8 * g) = o;
        }
    });
}

template <int C>
int launch_up_head(const UpHeadK& k, hipStream_t stream) {
    constexpr int lds_bytes = 128 * (C + 4) * 4;
    if (int rc = vqae::set_max_dynamic_lds((const void*)up_head_kernel<C>, lds_bytes)) return rc;
    up_head_kernel<C><<<(unsigned)ceil_div(k.M, 128), 256, lds_bytes, stream>>>(k);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

}  // namespace

namespace vqae {

bool up_head_channels(int c) { return c == 32 || c == 64 || c == 128; }

int up_head(const float* x, const float* w1f, const float* w2f, const float* wskf, int64_t M, int c, const FixupScalars& s,
            float* q, float* r, hipStream_t stream) {
    if (M == 0) return VQAE_OK;
    VQAE_REQUIRE(x && w1f && w2f && wskf && q && r, VQAE_ERR_INVALID, "up_head: null pointer");
    VQAE_REQUIRE(up_head_channels(c), VQAE_ERR_UNSUPPORTED, "up_head: C = %d", c);
    VQAE_REQUIRE(M > 0 && M < (1ll << 31) * 128, VQAE_ERR_UNSUPPORTED, "up_head: too many pixels");
    UpHeadK k;
    k.x = x; k.w1 = w1f; k.w2 = w2f; k.wsk = wskf; k.q = q; k.r = r; k.M = M; k.s = s;
    if (c == 32) return launch_up_head<32>(k, stream);
    if (c == 64) return launch_up_head<64>(k, stream);
    return launch_up_head<128>(k, stream);
}

bool up_tail_supported(int cb, int co) { return (cb == 64 && co == 32) || (cb == 32 && co == 16) || (cb == 16 && co == 8); }

int up_tail(const float* q, const float* s, const float* w3_packed, int B, int H, int W, int cb, int co, float b3a, float b3b,
            float scale, float b4, float* y, hipStream_t stream) {
    VQAE_REQUIRE(q && s && w3_packed && y, VQAE_ERR_INVALID, "up_tail: null pointer");
    VQAE_REQUIRE(up_tail_supported(cb, co), VQAE_ERR_UNSUPPORTED, "up_tail: channels %d -> %d", cb, co);
    if ((int64_t)B * H * W == 0) return VQAE_OK;
    const int tiles_x = (int)ceil_div(2 * W, 16), tiles_y = (int)ceil_div(2 * H, 8);      // 8 x 16 output pixels per tile
    const int64_t n_tiles = (int64_t)B * tiles_x * tiles_y;
    VQAE_REQUIRE(n_tiles < (1ll << 31), VQAE_ERR_UNSUPPORTED, "up_tail: too many tiles");
    const unsigned grid = (unsigned)std::min<int64_t>(n_tiles, 256 * 40);
    if (cb == 64) up_tail_kernel<64, 32><<<grid, 256, 0, stream>>>(q, s, w3_packed, B, H, W, tiles_x, tiles_y, b3a, b3b, scale, b4, y);
    else if (cb == 32) up_tail_kernel<32, 16><<<grid, 256, 0, stream>>>(q, s, w3_packed, B, H, W, tiles_x, tiles_y, b3a, b3b, scale, b4, y);
    else up_tail_kernel<16, 8><<<grid, 256, 0, stream>>>(q, s, w3_packed, B, H, W, tiles_x, tiles_y, b3a, b3b, scale, b4, y);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

}  // namespace vqae
