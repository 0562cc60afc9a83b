// The way in from slide pixels to code grids (gfx950): cutting encoder tiles out of a resident uint8 pixel canvas (the
// device form of CAMELYON16SlicePatchDataSet.__getitem__, datamodules/camelyon16.py:149-211) and pooling a mask canvas
// straight into the label grid (the adaptive_max_pool2d of run_eval, extract_embeddings.py:127-130, for every tile of a
// region at once).  Both are streaming kernels over bytes: no LDS, no atomics, no barrier; every source byte is read once.
#include <algorithm>

#include "kernels.h"

namespace {

// A tile's source origin in the canvas, or false when the tile does not lie wholly inside it (negative position included).
__device__ __forceinline__ bool tile_origin(const int32_t* __restrict__ rc, int t, int src_h, int src_w, int y0, int x0,
                                            int canvas_h, int canvas_w, int64_t& sy, int64_t& sx) {
    const int r = rc[2 * t], c = rc[2 * t + 1];
    sy = (int64_t)y0 + (int64_t)r * src_h;
    sx = (int64_t)x0 + (int64_t)c * src_w;
    return r >= 0 && c >= 0 && sy + src_h <= canvas_h && sx + src_w <= canvas_w;
}

// ------------------------------------------------------------------------------------------------
// Level 0: a copy of h rows of row_bytes = w * ch bytes per tile.  A lane owns one 16-byte chunk of one row.  Whether that
// chunk moves as one 16-byte load and store or as bytes is decided from the two addresses themselves, so rows that happen
// to be aligned take the wide path whatever the canvas pitch is (a pitch of 300 bytes aligns every fourth row) and a tail
// chunk shorter than 16 bytes is always bytes.  blockIdx.y walks the tiles, blockIdx.x the chunks of a tile.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void cut_copy_kernel(const uint8_t* __restrict__ canvas, int canvas_h, int canvas_w, int ch, const int32_t* __restrict__ rc,
                     int n_tiles, int h, int w, int y0, int x0, uint8_t* __restrict__ tiles) {
    const int row_bytes = w * ch;
    const int chunks = (row_bytes + 15) >> 4;
    const int items = h * chunks;                                    // per tile: <= 2^30 (checked on the host)
    const int64_t pitch = (int64_t)canvas_w * ch;
    for (int t = blockIdx.y; t < n_tiles; t += gridDim.y) {
        int64_t sy, sx;
        if (!tile_origin(rc, t, h, w, y0, x0, canvas_h, canvas_w, sy, sx)) continue;
        const uint8_t* src0 = canvas + sy * pitch + sx * ch;
        uint8_t* dst0 = tiles + (int64_t)t * h * row_bytes;
        for (int j = blockIdx.x * 256 + threadIdx.x; j < items; j += gridDim.x * 256) {
            const int y = j / chunks, k = j - y * chunks;
            const uint8_t* s = src0 + (int64_t)y * pitch + 16 * k;
            uint8_t* d = dst0 + (int64_t)y * row_bytes + 16 * k;
            const int n = min(16, row_bytes - 16 * k);
            if (n == 16 && (((uintptr_t)s | (uintptr_t)d) & 15) == 0) {
                *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
            } else {
                for (int b = 0; b < n; ++b) d[b] = s[b];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Level L >= 1: out[Y][X][c] = (sum of the f x f block + f*f/2) >> 2L, f = 2^L: exact integer sums (255 * 4^6 + 2^11 fits 32
// bits), rounding half up, independent of the summation order -- the rule of vqae_pixels_u8_level.
//   VEC  a lane owns a run of 16 source pixels (CH 16-byte loads per row) and walks the f rows of its output block, UNROLL rows of
//        loads in flight, adding every byte into the sum of its output pixel.  f <= 16: 16 / f output pixels per lane, stored as
//        dwords where the destination is dword aligned; f = 32, 64: the f / 16 neighbouring lanes of a block, which lie in one
//        wave because a row holds w * f / 16 runs, add up with __shfl_xor and the first of them stores the pixel.
//   else a thread owns one output pixel and loops over its f x f inputs: any width, any alignment.
// ------------------------------------------------------------------------------------------------
template <int CH, int L, bool VEC>
__global__ __launch_bounds__(256)
void cut_level_kernel(const uint8_t* __restrict__ canvas, int canvas_h, int canvas_w, const int32_t* __restrict__ rc, int n_tiles,
                      int h, int w, int y0, int x0, uint8_t* __restrict__ tiles) {
    constexpr int F = 1 << L;
    constexpr uint32_t HALF = (uint32_t)(F * F) / 2;
    constexpr int NOUT = F <= 16 ? 16 / F : 1;                       // output pixels per lane (VEC)
    constexpr int G = F <= 16 ? 1 : F / 16;                          // lanes per output pixel (VEC)
    constexpr int UNROLL = F < 4 ? F : 4;                            // rows whose loads are issued together
    const int per_row = VEC ? (int)(((int64_t)w * F) >> 4) : w;
    const int items = h * per_row;                                   // per tile: <= 2^30 (checked on the host)
    const int64_t pitch = (int64_t)canvas_w * CH;
    for (int t = blockIdx.y; t < n_tiles; t += gridDim.y) {
        int64_t sy, sx;
        if (!tile_origin(rc, t, h * F, w * F, y0, x0, canvas_h, canvas_w, sy, sx)) continue;
        const uint8_t* src0 = canvas + sy * pitch + sx * CH;
        uint8_t* dst0 = tiles + (int64_t)t * h * w * CH;
        // (the bound is uniform per workgroup, so that the lanes of a block reach the shuffles together)
        for (int base = blockIdx.x * 256; base < items; base += gridDim.x * 256) {
            const int j = base + threadIdx.x;
            const bool live = j < items;
            const int Y = live ? j / per_row : 0, u = live ? j - Y * per_row : 0;
            if constexpr (VEC) {
                uint32_t a[NOUT * CH];
#pragma unroll
                for (int i = 0; i < NOUT * CH; ++i) a[i] = 0;
                if (live) {
                    const uint8_t* s = src0 + (int64_t)Y * F * pitch + (int64_t)u * 16 * CH;
                    for (int dy = 0; dy < F; dy += UNROLL) {
                        uint4 v[UNROLL][CH];
#pragma unroll
                        for (int q = 0; q < UNROLL; ++q)
#pragma unroll
                            for (int k = 0; k < CH; ++k)
                                v[q][k] = reinterpret_cast<const uint4*>(s + (int64_t)(dy + q) * pitch)[k];
#pragma unroll
                        for (int q = 0; q < UNROLL; ++q)
#pragma unroll
                            for (int k = 0; k < CH; ++k) {
                                const uint32_t wd[4] = {v[q][k].x, v[q][k].y, v[q][k].z, v[q][k].w};
#pragma unroll
                                for (int b = 0; b < 16; ++b) {
                                    const int byte = 16 * k + b;     // of the run: pixel byte / CH, channel byte % CH
                                    a[((byte / CH) / F) % NOUT * CH + byte % CH] += (wd[b >> 2] >> (8 * (b & 3))) & 0xffu;
                                }
                            }
                    }
                }
                if constexpr (G > 1) {
#pragma unroll
                    for (int c = 0; c < CH; ++c)
#pragma unroll
                        for (int m = 1; m < G; m <<= 1) a[c] += (uint32_t)__shfl_xor((int)a[c], m);
                }
                if (live && (u & (G - 1)) == 0) {
                    uint8_t* d = dst0 + ((int64_t)Y * w + (int64_t)(u / G) * NOUT) * CH;
                    constexpr int NB = NOUT * CH;
                    if constexpr (NB % 4 == 0) {
                        uint32_t pk[NB / 4];
#pragma unroll
                        for (int i = 0; i < NB / 4; ++i) {
                            pk[i] = 0;
#pragma unroll
                            for (int b = 0; b < 4; ++b) pk[i] |= ((a[4 * i + b] + HALF) >> (2 * L)) << (8 * b);
                        }
                        if (((uintptr_t)d & 3) == 0) {
#pragma unroll
                            for (int i = 0; i < NB / 4; ++i) reinterpret_cast<uint32_t*>(d)[i] = pk[i];
                        } else {
#pragma unroll
                            for (int i = 0; i < NB; ++i) d[i] = (uint8_t)(pk[i >> 2] >> (8 * (i & 3)));
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < NB; ++i) d[i] = (uint8_t)((a[i] + HALF) >> (2 * L));
                    }
                }
            } else {
                if (live) {
                    uint32_t a[CH];
#pragma unroll
                    for (int c = 0; c < CH; ++c) a[c] = 0;
                    const uint8_t* s = src0 + (int64_t)Y * F * pitch + (int64_t)u * F * CH;
                    for (int dy = 0; dy < F; ++dy)
                        for (int dx = 0; dx < F * CH; dx += CH)
#pragma unroll
                            for (int c = 0; c < CH; ++c) a[c] += s[(int64_t)dy * pitch + dx + c];
                    uint8_t* d = dst0 + ((int64_t)Y * w + u) * CH;
#pragma unroll
                    for (int c = 0; c < CH; ++c) d[c] = (uint8_t)((a[c] + HALF) >> (2 * L));
                }
            }
        }
    }
}

template <int CH, int L>
void launch_cut_level(bool vec, dim3 grid, hipStream_t stream, const uint8_t* canvas, int canvas_h, int canvas_w, const int32_t* rc,
                      int n_tiles, int h, int w, int y0, int x0, uint8_t* tiles) {
    if (vec) cut_level_kernel<CH, L, true><<<grid, 256, 0, stream>>>(canvas, canvas_h, canvas_w, rc, n_tiles, h, w, y0, x0, tiles);
    else cut_level_kernel<CH, L, false><<<grid, 256, 0, stream>>>(canvas, canvas_h, canvas_w, rc, n_tiles, h, w, y0, x0, tiles);
}

template <int CH>
void launch_cut_ch(int level, bool vec, dim3 grid, hipStream_t stream, const uint8_t* canvas, int canvas_h, int canvas_w,
                   const int32_t* rc, int n_tiles, int h, int w, int y0, int x0, uint8_t* tiles) {
    switch (level) {
        case 1: launch_cut_level<CH, 1>(vec, grid, stream, canvas, canvas_h, canvas_w, rc, n_tiles, h, w, y0, x0, tiles); break;
        case 2: launch_cut_level<CH, 2>(vec, grid, stream, canvas, canvas_h, canvas_w, rc, n_tiles, h, w, y0, x0, tiles); break;
        case 3: launch_cut_level<CH, 3>(vec, grid, stream, canvas, canvas_h, canvas_w, rc, n_tiles, h, w, y0, x0, tiles); break;
        case 4: launch_cut_level<CH, 4>(vec, grid, stream, canvas, canvas_h, canvas_w, rc, n_tiles, h, w, y0, x0, tiles); break;
        case 5: launch_cut_level<CH, 5>(vec, grid, stream, canvas, canvas_h, canvas_w, rc, n_tiles, h, w, y0, x0, tiles); break;
        default: launch_cut_level<CH, 6>(vec, grid, stream, canvas, canvas_h, canvas_w, rc, n_tiles, h, w, y0, x0, tiles); break;
    }
}

// ------------------------------------------------------------------------------------------------
// Label pooling: out[Y][X] = max of the win_h x win_w window of the mask at (y0 + Y * win_h, x0 + X * win_w).
//   VEC  (LW = log2 win_w; mask base, pitch and x0 multiples of 16) a lane owns a 16-byte column of one output row and walks its
//        win_h mask rows with 16-byte loads, UNROLL of them in flight.  The running maximum is kept on packed bytes: the even
//        and the odd bytes of every dword as two 16-bit lanes each, one v_pk_max_u16 per pair and row.  win_w <= 16: the lane
//        then folds its 16 column maxima into 16 / win_w outputs; win_w = 32 .. 1024: the win_w / 16 neighbouring lanes of a
//        window, which lie in one wave because a row holds out_w * win_w / 16 columns, combine with __shfl_xor.
//   else a thread owns one output and loops over its window: any window, any alignment.
// Each workgroup strides over the output rows, so a thread produces several outputs either way.
// ------------------------------------------------------------------------------------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
    const u16x2 m = __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b));
    return __builtin_bit_cast(uint32_t, m);
}

template <int LW>
__global__ __launch_bounds__(256)
void pool_labels_vec_kernel(const uint8_t* __restrict__ mask, int mask_w, int y0, int x0, int win_h, uint8_t* __restrict__ out,
                            int out_h, int out_w) {
    constexpr int WW = 1 << LW;
    constexpr int NOUT = WW <= 16 ? 16 / WW : 1;                     // outputs per lane
    constexpr int G = WW <= 16 ? 1 : WW / 16;                        // lanes per output
    constexpr int UNROLL = 4;
    const int per_row = (int)(((int64_t)out_w * WW + 15) >> 4);      // 16-byte columns of an output row
    const int64_t items = (int64_t)out_h * per_row;
    // (the bound is uniform per workgroup, so that the lanes of a window reach the shuffles together)
    for (int64_t base = (int64_t)blockIdx.x * 256; base < items; base += (int64_t)gridDim.x * 256) {
        const int64_t j = base + threadIdx.x;
        const bool live = j < items;
        const int64_t Y = live ? j / per_row : 0;
        const int u = live ? (int)(j - Y * per_row) : 0;
        uint32_t ev[4] = {0, 0, 0, 0}, od[4] = {0, 0, 0, 0};        // maxima of the even / odd bytes of the 4 dwords
        if (live) {
            const uint8_t* s = mask + ((int64_t)y0 + Y * win_h) * mask_w + x0 + 16 * (int64_t)u;
            int dy = 0;
            for (; dy + UNROLL <= win_h; dy += UNROLL) {
                uint4 v[UNROLL];
#pragma unroll
                for (int q = 0; q < UNROLL; ++q) v[q] = *reinterpret_cast<const uint4*>(s + (int64_t)(dy + q) * mask_w);
#pragma unroll
                for (int q = 0; q < UNROLL; ++q) {
                    const uint32_t wd[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        ev[i] = pk_max_u16(ev[i], wd[i] & 0x00ff00ffu);
                        od[i] = pk_max_u16(od[i], (wd[i] >> 8) & 0x00ff00ffu);
                    }
                }
            }
            for (; dy < win_h; ++dy) {
                const uint4 v = *reinterpret_cast<const uint4*>(s + (int64_t)dy * mask_w);
                const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ev[i] = pk_max_u16(ev[i], wd[i] & 0x00ff00ffu);
                    od[i] = pk_max_u16(od[i], (wd[i] >> 8) & 0x00ff00ffu);
                }
            }
        }
        uint32_t b[16];                                              // the 16 column maxima
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            b[4 * i] = ev[i] & 0xffu; b[4 * i + 1] = od[i] & 0xffu; b[4 * i + 2] = ev[i] >> 16; b[4 * i + 3] = od[i] >> 16;
        }
        constexpr int SPAN = 16 / NOUT;                              // columns per output inside the lane
        uint32_t o[NOUT];
#pragma unroll
        for (int i = 0; i < NOUT; ++i) {
            o[i] = b[i * SPAN];
#pragma unroll
            for (int k = 1; k < SPAN; ++k) o[i] = max(o[i], b[i * SPAN + k]);
        }
        if constexpr (G > 1) {
#pragma unroll
            for (int m = 1; m < G; m <<= 1) o[0] = max(o[0], (uint32_t)__shfl_xor((int)o[0], m));
        }
        if (live && (u & (G - 1)) == 0) {
            const int X0 = (u / G) * NOUT;                           // first output of the lane; the last lane of a row may own fewer
            uint8_t* d = out + Y * out_w + X0;
            const int n = min(NOUT, out_w - X0);
            if constexpr (NOUT == 16) {
                if (n == 16 && ((uintptr_t)d & 15) == 0) {
                    uint4 pk;
                    pk.x = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
                    pk.y = o[4] | o[5] << 8 | o[6] << 16 | o[7] << 24;
                    pk.z = o[8] | o[9] << 8 | o[10] << 16 | o[11] << 24;
                    pk.w = o[12] | o[13] << 8 | o[14] << 16 | o[15] << 24;
                    *reinterpret_cast<uint4*>(d) = pk;
                    continue;
                }
            }
#pragma unroll
            for (int i = 0; i < NOUT; ++i)
                if (i < n) d[i] = (uint8_t)o[i];
        }
    }
}

__global__ __launch_bounds__(256)
void pool_labels_any_kernel(const uint8_t* __restrict__ mask, int mask_w, int y0, int x0, int win_h, int win_w,
                            uint8_t* __restrict__ out, int out_h, int out_w) {
    const int64_t total = (int64_t)out_h * out_w;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t Y = i / out_w;
        const int X = (int)(i - Y * out_w);
        const uint8_t* s = mask + ((int64_t)y0 + Y * win_h) * mask_w + x0 + (int64_t)X * win_w;
        uint32_t m = 0;
        for (int dy = 0; dy < win_h; ++dy)
            for (int dx = 0; dx < win_w; ++dx) m = max(m, (uint32_t)s[(int64_t)dy * mask_w + dx]);
        out[i] = (uint8_t)m;
    }
}

template <int LW>
void launch_pool_vec(unsigned grid, hipStream_t stream, const uint8_t* mask, int mask_w, int y0, int x0, int win_h, uint8_t* out,
                     int out_h, int out_w) {
    pool_labels_vec_kernel<LW><<<grid, 256, 0, stream>>>(mask, mask_w, y0, x0, win_h, out, out_h, out_w);
}

}  // namespace

namespace vqae {

int cut_pixels_u8(const uint8_t* canvas, int canvas_h, int canvas_w, int ch, const int32_t* rc, int n_tiles, int h, int w, int y0,
                  int x0, int level, uint8_t* tiles, hipStream_t stream) {
    VQAE_REQUIRE(ch == 1 || ch == 3, VQAE_ERR_INVALID, "cut_pixels_u8: %d channels (1 or 3)", ch);
    VQAE_REQUIRE(n_tiles >= 0 && h >= 1 && w >= 1 && canvas_h >= 1 && canvas_w >= 1, VQAE_ERR_INVALID, "cut_pixels_u8: bad shape");
    VQAE_REQUIRE(y0 >= 0 && x0 >= 0, VQAE_ERR_INVALID, "cut_pixels_u8: origin (%d, %d)", y0, x0);
    VQAE_REQUIRE(level >= 0, VQAE_ERR_INVALID, "cut_pixels_u8: level %d", level);
    VQAE_REQUIRE(level <= VQAE_MAX_PIXEL_LEVEL, VQAE_ERR_UNSUPPORTED, "cut_pixels_u8: level %d is above %d", level,
                 VQAE_MAX_PIXEL_LEVEL);
    const int f = 1 << level;
    // (the kernels walk a tile with an int that steps by up to 2048 * 256 past the last item; tile_origin multiplies in 64 bits)
    VQAE_REQUIRE((int64_t)h * w * ch <= (1ll << 30) && (int64_t)h * f < (1ll << 31) && (int64_t)w * f < (1ll << 31),
                 VQAE_ERR_UNSUPPORTED, "cut_pixels_u8: tile of %d x %d pixels at level %d", h, w, level);
    VQAE_REQUIRE((int64_t)y0 + (int64_t)h * f <= canvas_h && (int64_t)x0 + (int64_t)w * f <= canvas_w, VQAE_ERR_INVALID,
                 "cut_pixels_u8: canvas %d x %d holds no %d x %d tile at origin (%d, %d)", canvas_h, canvas_w, h * f, w * f, y0, x0);
    if (n_tiles == 0) return VQAE_OK;
    VQAE_REQUIRE(canvas && rc && tiles, VQAE_ERR_INVALID, "cut_pixels_u8: null pointer");
    if (level == 0) {
        const int items = h * (int)ceil_div((int64_t)w * ch, 16);
        // memory-bound: about 8 workgroups per CU in all, grid-stride over the rest
        const unsigned gx = (unsigned)std::min<int64_t>(ceil_div(items, 256), 2048);
        const unsigned gy = (unsigned)std::min<int64_t>(n_tiles, std::max<int64_t>(1, 2048 / gx));
        cut_copy_kernel<<<dim3(gx, gy), 256, 0, stream>>>(canvas, canvas_h, canvas_w, ch, rc, n_tiles, h, w, y0, x0, tiles);
        VQAE_LAUNCH_CHECK();
        return VQAE_OK;
    }
    // the 16-pixel path: every source run 16-byte aligned (base, pitch and origin; runs of 16 pixels tile a row of w * f)
    const bool vec = (uintptr_t)canvas % 16 == 0 && ((int64_t)canvas_w * ch) % 16 == 0 && ((int64_t)x0 * ch) % 16 == 0 &&
                     ((int64_t)w * f) % 16 == 0;
    const int64_t items = (int64_t)h * (vec ? ((int64_t)w * f) / 16 : w);
    VQAE_REQUIRE(items <= (1ll << 30), VQAE_ERR_UNSUPPORTED, "cut_pixels_u8: tile of %d x %d pixels at level %d", h, w, level);
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div(items, 256), 2048);
    const unsigned gy = (unsigned)std::min<int64_t>(n_tiles, std::max<int64_t>(1, 2048 / gx));
    const dim3 grid(gx, gy);
    if (ch == 3) launch_cut_ch<3>(level, vec, grid, stream, canvas, canvas_h, canvas_w, rc, n_tiles, h, w, y0, x0, tiles);
    else launch_cut_ch<1>(level, vec, grid, stream, canvas, canvas_h, canvas_w, rc, n_tiles, h, w, y0, x0, tiles);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

int pool_labels_u8(const uint8_t* mask, int mask_h, int mask_w, int y0, int x0, int win_h, int win_w, uint8_t* out, int out_h,
                   int out_w, hipStream_t stream) {
    VQAE_REQUIRE(mask_h >= 1 && mask_w >= 1 && win_h >= 1 && win_w >= 1 && out_h >= 0 && out_w >= 0, VQAE_ERR_INVALID,
                 "pool_labels_u8: bad shape");
    VQAE_REQUIRE(y0 >= 0 && x0 >= 0, VQAE_ERR_INVALID, "pool_labels_u8: origin (%d, %d)", y0, x0);
    VQAE_REQUIRE((int64_t)y0 + (int64_t)out_h * win_h <= mask_h && (int64_t)x0 + (int64_t)out_w * win_w <= mask_w, VQAE_ERR_INVALID,
                 "pool_labels_u8: %d x %d windows of %d x %d at (%d, %d) reach outside the %d x %d mask", out_h, out_w, win_h, win_w,
                 y0, x0, mask_h, mask_w);
    if (out_h == 0 || out_w == 0) return VQAE_OK;
    VQAE_REQUIRE(mask && out, VQAE_ERR_INVALID, "pool_labels_u8: null pointer");
    int lw = -1;
    for (int k = 0; k <= 10; ++k)
        if (win_w == 1 << k) lw = k;
    // the 16-byte path: a power-of-two window width up to 1024 and 16-byte aligned columns (x0 and the pitch being multiples of
    // 16, the last column of a row, which may reach past the windows, still ends inside its mask row)
    const bool vec = lw >= 0 && (uintptr_t)mask % 16 == 0 && mask_w % 16 == 0 && x0 % 16 == 0;
    const int64_t items = vec ? (int64_t)out_h * ceil_div((int64_t)out_w * win_w, 16) : (int64_t)out_h * out_w;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(items, 256), 4096);
    if (!vec) {
        pool_labels_any_kernel<<<grid, 256, 0, stream>>>(mask, mask_w, y0, x0, win_h, win_w, out, out_h, out_w);
    } else {
        switch (lw) {
            case 0: launch_pool_vec<0>(grid, stream, mask, mask_w, y0, x0, win_h, out, out_h, out_w); break;
            case 1: launch_pool_vec<1>(grid, stream, mask, mask_w, y0, x0, win_h, out, out_h, out_w); break;
            case 2: launch_pool_vec<2>(grid, stream, mask, mask_w, y0, x0, win_h, out, out_h, out_w); break;
            case 3: launch_pool_vec<3>(grid, stream, mask, mask_w, y0, x0, win_h, out, out_h, out_w); break;
            case 4: launch_pool_vec<4>(grid, stream, mask, mask_w, y0, x0, win_h, out, out_h, out_w); break;
            case 5: launch_pool_vec<5>(grid, stream, mask, mask_w, y0, x0, win_h, out, out_h, out_w); break;
            case 6: launch_pool_vec<6>(grid, stream, mask, mask_w, y0, x0, win_h, out, out_h, out_w); break;
            case 7: launch_pool_vec<7>(grid, stream, mask, mask_w, y0, x0, win_h, out, out_h, out_w); break;
            case 8: launch_pool_vec<8>(grid, stream, mask, mask_w, y0, x0, win_h, out, out_h, out_w); break;
            case 9: launch_pool_vec<9>(grid, stream, mask, mask_w, y0, x0, win_h, out, out_h, out_w); break;
            default: launch_pool_vec<10>(grid, stream, mask, mask_w, y0, x0, win_h, out, out_h, out_w); break;
        }
    }
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

}  // namespace vqae

extern "C" int vqae_cut_pixels_u8(const uint8_t* canvas, int canvas_h, int canvas_w, int ch, const int32_t* rc, int n_tiles, int h,
                                  int w, int y0, int x0, int level, uint8_t* tiles, void* stream) {
    return vqae::cut_pixels_u8(canvas, canvas_h, canvas_w, ch, rc, n_tiles, h, w, y0, x0, level, tiles, (hipStream_t)stream);
}

extern "C" int vqae_pool_labels_u8(const uint8_t* mask, int mask_h, int mask_w, int y0, int x0, int win_h, int win_w, uint8_t* out,
                                   int out_h, int out_w, void* stream) {
    return vqae::pool_labels_u8(mask, mask_h, mask_w, y0, x0, win_h, win_w, out, out_h, out_w, (hipStream_t)stream);
}
