// The way back from code grids to pictures (gfx950): cutting a stored slide grid into code tiles (the inverse of the
// stitch of misc_kernels.hip) and turning the decoder's fp32 reconstruction into uint8 pixels, pasted into a canvas.
#include <algorithm>

#include "kernels.h"

namespace {

// tiles[t][y][x] = grid[(r*th + y) * gw + c*tw + x] for (r, c) = rc[t]; elements whose grid position is outside the
// grid are neither read nor written.
template <typename TI, typename TO>
__global__ __launch_bounds__(256)
void unstitch_kernel(const TI* __restrict__ grid, const int32_t* __restrict__ rc, int64_t total, int th, int tw,
                     TO* __restrict__ tiles, int gh, int gw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % tw), yy = (int)((i / tw) % th);
    const int64_t t = i / ((int64_t)tw * th);
    const int r = rc[2 * t], c = rc[2 * t + 1];
    const int64_t gy = (int64_t)r * th + yy, gx = (int64_t)c * tw + x;
    if (r >= 0 && c >= 0 && gy < gh && gx < gw) tiles[i] = (TO)grid[gy * gw + gx];
}

template <typename TI>
int unstitch_out(const TI* grid, const int32_t* rc, int64_t total, int th, int tw, void* tiles, int tdt, int gh, int gw,
                 hipStream_t stream) {
    const unsigned g = (unsigned)vqae::ceil_div(total, 256);
    switch (tdt) {
        case VQAE_IDX_I64: unstitch_kernel<TI, int64_t><<<g, 256, 0, stream>>>(grid, rc, total, th, tw, (int64_t*)tiles, gh, gw); break;
        case VQAE_IDX_U8: unstitch_kernel<TI, uint8_t><<<g, 256, 0, stream>>>(grid, rc, total, th, tw, (uint8_t*)tiles, gh, gw); break;
        case VQAE_IDX_U16: unstitch_kernel<TI, uint16_t><<<g, 256, 0, stream>>>(grid, rc, total, th, tw, (uint16_t*)tiles, gh, gw); break;
        case VQAE_IDX_I32: unstitch_kernel<TI, int32_t><<<g, 256, 0, stream>>>(grid, rc, total, th, tw, (int32_t*)tiles, gh, gw); break;
        default: return vqae::fail(VQAE_ERR_INVALID, "unstitch: bad tile dtype %d", tdt);
    }
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

// ------------------------------------------------------------------------------------------------
// fp32 reconstruction -> uint8 NHWC pixels: the inverse of the Normalize transform the ingest kernels apply
// (camelyon16_transforms.yaml:15-23), u = clamp(rint(x * std255[c] + mean255[c]), 0, 255) with one fused multiply-add,
// round-to-nearest-even, NaN -> 0.  12 B in and 3 B out per pixel, nothing else: HBM-bound.
//   VEC  a thread owns 4 pixels of one row: NHWC three 16-byte loads (12 consecutive floats), NCHW one 16-byte load per
//        plane; 12 contiguous output bytes as three dwords (the host checks W % 4 == 0 and the alignment of both sides).
//   else a thread owns one pixel, 3 loads and 3 byte stores: any width, any alignment.
// blockIdx.y walks the tiles (rc and the paste origin are uniform per workgroup), blockIdx.x the pixels of a tile.  A tile
// that does not lie wholly inside the canvas is skipped.
// ------------------------------------------------------------------------------------------------
struct Denorm3 { float mean[3]; float scale[3]; };

__device__ __forceinline__ uint32_t quant_u8(float x, float s, float m) {
    const float r = rintf(__builtin_fmaf(x, s, m));
    return !(r > 0.f) ? 0u : (r > 255.f ? 255u : (uint32_t)r);       // NaN, -inf, -0: 0
}

template <bool NCHW, bool VEC>
__global__ __launch_bounds__(256)
void pixels_u8_kernel(const float* __restrict__ x, int B, int H, int W, const int32_t* __restrict__ rc, Denorm3 dn,
                      uint8_t* __restrict__ out, int out_h, int out_w) {
    const int per_row = VEC ? W >> 2 : W;
    const int items = H * per_row;                                   // per tile: <= 2^30 (checked on the host)
    const int64_t hw = (int64_t)H * W;
    for (int t = blockIdx.y; t < B; t += gridDim.y) {
        int64_t oy0, ox0;
        if (rc) {
            const int r = rc[2 * t], c = rc[2 * t + 1];
            oy0 = (int64_t)r * H; ox0 = (int64_t)c * W;
            if (r < 0 || c < 0 || oy0 + H > out_h || ox0 + W > out_w) continue;
        } else {
            oy0 = (int64_t)t * H; ox0 = 0;                           // dense [B][H][W][3] = a canvas of B*H rows
        }
        const float* xt = x + (int64_t)t * hw * 3;
        for (int j = blockIdx.x * 256 + threadIdx.x; j < items; j += gridDim.x * 256) {
            const int y = j / per_row, xq = j - y * per_row;
            uint8_t* dst = out + ((oy0 + y) * out_w + ox0) * 3;
            if constexpr (VEC) {
                float e[12];                                         // e[3 p + c]: pixel p of the run, channel c
                if constexpr (NCHW) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float4 v = *reinterpret_cast<const float4*>(xt + c * hw + (int64_t)y * W + 4 * xq);
                        e[c] = v.x; e[3 + c] = v.y; e[6 + c] = v.z; e[9 + c] = v.w;
                    }
                } else {
                    const float4* src = reinterpret_cast<const float4*>(xt + ((int64_t)y * W + 4 * xq) * 3);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const float4 v = src[k];
                        e[4 * k] = v.x; e[4 * k + 1] = v.y; e[4 * k + 2] = v.z; e[4 * k + 3] = v.w;
                    }
                }
                uint32_t wd[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    wd[k] = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int i = 4 * k + b;
                        wd[k] |= quant_u8(e[i], dn.scale[i % 3], dn.mean[i % 3]) << (8 * b);
                    }
                }
                uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + 12 * xq);
                d32[0] = wd[0]; d32[1] = wd[1]; d32[2] = wd[2];
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v = NCHW ? xt[c * hw + (int64_t)y * W + xq] : xt[((int64_t)y * W + xq) * 3 + c];
                    dst[3 * xq + c] = (uint8_t)quant_u8(v, dn.scale[c], dn.mean[c]);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Overview levels: out[Y][X][c] = (sum of the f x f block of level-0 pixels u + f*f/2) >> 2L, f = 2^L, with u the bits
// quant_u8 gives at level 0 -- an integer mean that rounds half up, independent of the summation order.
//   VEC  a lane owns the same run of 4 pixels as at level 0 and walks the f rows of its output block (adjacent lanes read
//        adjacent 48 bytes of every row; UNROLL rows of loads are in flight at once), keeping 12 uint32 column sums.  f = 2:
//        two output pixels per lane (three 16-bit stores); f = 4: one; f >= 8: the f/4 neighbouring lanes of a block, which
//        lie in one wave because W/4 is a multiple of f/4 <= 16, add up with __shfl_xor and the first of them stores the
//        3 bytes.  No LDS, no atomics, no barrier.
//   else a thread owns one output pixel and loops over its f x f inputs: any width, any alignment.
// blockIdx.y walks the tiles as in pixels_u8_kernel; the canvas and the paste origin are in level-L pixels.
// ------------------------------------------------------------------------------------------------
template <bool NCHW, bool VEC, int L>
__global__ __launch_bounds__(256)
void pixels_u8_level_kernel(const float* __restrict__ x, int B, int H, int W, const int32_t* __restrict__ rc, Denorm3 dn,
                            uint8_t* __restrict__ out, int out_h, int out_w) {
    constexpr int F = 1 << L;
    constexpr int UNROLL = F < 8 ? F : 8;                            // rows whose loads are issued together
    constexpr uint32_t HALF = (uint32_t)(F * F) / 2;
    const int oh = H >> L, ow = W >> L;                              // the reduced tile
    const int per_row = VEC ? W >> 2 : ow;
    const int items = oh * per_row;                                  // per tile: <= 2^30 (checked on the host)
    const int64_t hw = (int64_t)H * W;
    for (int t = blockIdx.y; t < B; t += gridDim.y) {
        int64_t oy0, ox0;
        if (rc) {
            const int r = rc[2 * t], c = rc[2 * t + 1];
            oy0 = (int64_t)r * oh; ox0 = (int64_t)c * ow;
            if (r < 0 || c < 0 || oy0 + oh > out_h || ox0 + ow > out_w) continue;
        } else {
            oy0 = (int64_t)t * oh; ox0 = 0;                          // dense [B][H/f][W/f][3] = a canvas of B*H/f rows
        }
        const float* xt = x + (int64_t)t * hw * 3;
        // (the bound is uniform per workgroup, so that the lanes of a block reach the shuffles together)
        for (int base = blockIdx.x * 256; base < items; base += gridDim.x * 256) {
            const int j = base + threadIdx.x;
            const bool live = j < items;
            const int Y = live ? j / per_row : 0, xq = live ? j - Y * per_row : 0;
            uint8_t* dst = out + ((oy0 + Y) * out_w + ox0) * 3;
            if constexpr (VEC) {
                uint32_t s[12];                                      // s[3 p + c]: column sums of pixel p of the run, channel c
#pragma unroll
                for (int i = 0; i < 12; ++i) s[i] = 0;
                if (live) {
                    for (int dy = 0; dy < F; dy += UNROLL) {
                        float4 v[UNROLL][3];
#pragma unroll
                        for (int u = 0; u < UNROLL; ++u) {
                            const int64_t y = (int64_t)Y * F + dy + u;
#pragma unroll
                            for (int k = 0; k < 3; ++k)
                                v[u][k] = NCHW ? *reinterpret_cast<const float4*>(xt + k * hw + y * W + 4 * xq)
                                               : reinterpret_cast<const float4*>(xt + (y * W + 4 * xq) * 3)[k];
                        }
#pragma unroll
                        for (int u = 0; u < UNROLL; ++u) {
                            float e[12];                             // e[3 p + c], as in pixels_u8_kernel
#pragma unroll
                            for (int k = 0; k < 3; ++k) {
                                if constexpr (NCHW) { e[k] = v[u][k].x; e[3 + k] = v[u][k].y; e[6 + k] = v[u][k].z; e[9 + k] = v[u][k].w; }
                                else { e[4 * k] = v[u][k].x; e[4 * k + 1] = v[u][k].y; e[4 * k + 2] = v[u][k].z; e[4 * k + 3] = v[u][k].w; }
                            }
#pragma unroll
                            for (int i = 0; i < 12; ++i) s[i] += quant_u8(e[i], dn.scale[i % 3], dn.mean[i % 3]);
                        }
                    }
                }
                if constexpr (L == 1) {
                    if (live) {
                        uint32_t b[6];                               // two output pixels
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            b[c] = (s[c] + s[3 + c] + HALF) >> 2;
                            b[3 + c] = (s[6 + c] + s[9 + c] + HALF) >> 2;
                        }
                        uint16_t* d16 = reinterpret_cast<uint16_t*>(dst + 6 * xq);
                        d16[0] = (uint16_t)(b[0] | b[1] << 8); d16[1] = (uint16_t)(b[2] | b[3] << 8); d16[2] = (uint16_t)(b[4] | b[5] << 8);
                    }
                } else {
                    constexpr int G = F / 4;                         // lanes per output block
                    uint32_t a[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        a[c] = s[c] + s[3 + c] + s[6 + c] + s[9 + c];
#pragma unroll
                        for (int m = 1; m < G; m <<= 1) a[c] += (uint32_t)__shfl_xor((int)a[c], m);
                    }
                    if (live && (xq & (G - 1)) == 0) {
                        uint8_t* d = dst + 3 * (xq / G);
#pragma unroll
                        for (int c = 0; c < 3; ++c) d[c] = (uint8_t)((a[c] + HALF) >> (2 * L));
                    }
                }
            } else {
                if (live) {
                    uint32_t a[3] = {0, 0, 0};
                    for (int dy = 0; dy < F; ++dy) {
                        const int64_t y = (int64_t)Y * F + dy;
                        for (int dx = 0; dx < F; ++dx) {
                            const int64_t xx = (int64_t)xq * F + dx;
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                const float v = NCHW ? xt[c * hw + y * W + xx] : xt[(y * W + xx) * 3 + c];
                                a[c] += quant_u8(v, dn.scale[c], dn.mean[c]);
                            }
                        }
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) dst[3 * xq + c] = (uint8_t)((a[c] + HALF) >> (2 * L));
                }
            }
        }
    }
}

template <int L>
void launch_level(bool nchw, bool vec, dim3 grid, hipStream_t stream, const float* x, int B, int H, int W, const int32_t* rc,
                  const Denorm3& dn, uint8_t* out, int out_h, int out_w) {
    if (vec && nchw) pixels_u8_level_kernel<true, true, L><<<grid, 256, 0, stream>>>(x, B, H, W, rc, dn, out, out_h, out_w);
    else if (vec) pixels_u8_level_kernel<false, true, L><<<grid, 256, 0, stream>>>(x, B, H, W, rc, dn, out, out_h, out_w);
    else if (nchw) pixels_u8_level_kernel<true, false, L><<<grid, 256, 0, stream>>>(x, B, H, W, rc, dn, out, out_h, out_w);
    else pixels_u8_level_kernel<false, false, L><<<grid, 256, 0, stream>>>(x, B, H, W, rc, dn, out, out_h, out_w);
}

}  // namespace

namespace vqae {

int unstitch_tiles(const void* grid, int grid_dtype, const int32_t* rc, int n_tiles, int th, int tw, void* tiles,
                   int idx_dtype, int gh, int gw, hipStream_t stream) {
    VQAE_REQUIRE(grid && rc && tiles, VQAE_ERR_INVALID, "unstitch: null pointer");
    VQAE_REQUIRE(n_tiles >= 0 && th >= 1 && tw >= 1 && gh >= 0 && gw >= 0, VQAE_ERR_INVALID, "unstitch: bad shape");
    const int64_t total = (int64_t)n_tiles * th * tw;
    if (total == 0) return VQAE_OK;
    VQAE_REQUIRE(ceil_div(total, 256) < (1ll << 31), VQAE_ERR_UNSUPPORTED, "unstitch: too many elements");
    switch (grid_dtype) {
        case VQAE_IDX_I64: return unstitch_out((const int64_t*)grid, rc, total, th, tw, tiles, idx_dtype, gh, gw, stream);
        case VQAE_IDX_U8: return unstitch_out((const uint8_t*)grid, rc, total, th, tw, tiles, idx_dtype, gh, gw, stream);
        case VQAE_IDX_U16: return unstitch_out((const uint16_t*)grid, rc, total, th, tw, tiles, idx_dtype, gh, gw, stream);
        case VQAE_IDX_I32: return unstitch_out((const int32_t*)grid, rc, total, th, tw, tiles, idx_dtype, gh, gw, stream);
        default: return fail(VQAE_ERR_INVALID, "unstitch: bad grid dtype %d", grid_dtype);
    }
}

int pixels_u8(const float* x, int layout, int B, int H, int W, const int32_t* rc, const float* mean255, const float* std255,
              uint8_t* out, int canvas_h, int canvas_w, hipStream_t stream) {
    VQAE_REQUIRE(x && out, VQAE_ERR_INVALID, "pixels_u8: null pointer");
    VQAE_REQUIRE(layout == VQAE_LAYOUT_NHWC || layout == VQAE_LAYOUT_NCHW, VQAE_ERR_INVALID, "pixels_u8: bad layout %d", layout);
    VQAE_REQUIRE(B >= 0 && H >= 1 && W >= 1, VQAE_ERR_INVALID, "pixels_u8: bad shape");
    // (the kernel walks a tile with an int that steps by up to 2048 * 256 past the last pixel)
    VQAE_REQUIRE((int64_t)H * W <= (1ll << 30), VQAE_ERR_UNSUPPORTED, "pixels_u8: tile of %d x %d pixels", H, W);
    if (rc) {
        VQAE_REQUIRE(canvas_h >= H && canvas_w >= W, VQAE_ERR_INVALID, "pixels_u8: canvas %d x %d is smaller than one %d x %d tile",
                     canvas_h, canvas_w, H, W);
    } else {
        VQAE_REQUIRE(canvas_h == 0 && canvas_w == 0, VQAE_ERR_INVALID, "pixels_u8: canvas sizes given for a dense destination");
        VQAE_REQUIRE((int64_t)B * H < (1ll << 31), VQAE_ERR_UNSUPPORTED, "pixels_u8: %d x %d rows", B, H);
    }
    if (B == 0) return VQAE_OK;
    Denorm3 dn;
    for (int c = 0; c < 3; ++c) {
        dn.mean[c] = mean255 ? mean255[c] : 0.f;
        dn.scale[c] = std255 ? std255[c] : 1.f;
    }
    const int out_h = rc ? canvas_h : B * H, out_w = rc ? canvas_w : W;
    // the 4-pixel path: 16-byte aligned loads (W % 4 == 0 keeps every row and plane aligned) and dword-aligned 12-byte stores
    const bool vec = W % 4 == 0 && out_w % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)out % 4 == 0;
    const int items = H * (vec ? W / 4 : W);
    // memory-bound: about 8 workgroups per CU in all, grid-stride over the rest
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div(items, 256), 2048);
    const unsigned gy = (unsigned)std::min<int64_t>(B, std::max<int64_t>(1, 2048 / gx));
    const dim3 grid(gx, gy);
    const bool nchw = layout == VQAE_LAYOUT_NCHW;
    if (vec && nchw) pixels_u8_kernel<true, true><<<grid, 256, 0, stream>>>(x, B, H, W, rc, dn, out, out_h, out_w);
    else if (vec) pixels_u8_kernel<false, true><<<grid, 256, 0, stream>>>(x, B, H, W, rc, dn, out, out_h, out_w);
    else if (nchw) pixels_u8_kernel<true, false><<<grid, 256, 0, stream>>>(x, B, H, W, rc, dn, out, out_h, out_w);
    else pixels_u8_kernel<false, false><<<grid, 256, 0, stream>>>(x, B, H, W, rc, dn, out, out_h, out_w);
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

int pixels_u8_level_check(const char* who, int H, int W, int level, bool canvas, int canvas_h, int canvas_w) {
    VQAE_REQUIRE(level >= 0, VQAE_ERR_INVALID, "%s: level %d", who, level);
    VQAE_REQUIRE(level <= VQAE_MAX_PIXEL_LEVEL, VQAE_ERR_UNSUPPORTED, "%s: level %d is above %d", who, level, VQAE_MAX_PIXEL_LEVEL);
    const int f = 1 << level;
    VQAE_REQUIRE(H % f == 0 && W % f == 0, VQAE_ERR_INVALID, "%s: %d does not divide the %d x %d tile", who, f, H, W);
    if (canvas)
        VQAE_REQUIRE(canvas_h >= H / f && canvas_w >= W / f, VQAE_ERR_INVALID, "%s: canvas %d x %d is smaller than one %d x %d tile",
                     who, canvas_h, canvas_w, H / f, W / f);
    else
        VQAE_REQUIRE(canvas_h == 0 && canvas_w == 0, VQAE_ERR_INVALID, "%s: canvas sizes given for a dense destination", who);
    return VQAE_OK;
}

int pixels_u8_level(const float* x, int layout, int B, int H, int W, int level, const int32_t* rc, const float* mean255,
                    const float* std255, uint8_t* out, int canvas_h, int canvas_w, hipStream_t stream) {
    VQAE_REQUIRE(layout == VQAE_LAYOUT_NHWC || layout == VQAE_LAYOUT_NCHW, VQAE_ERR_INVALID, "pixels_u8_level: bad layout %d", layout);
    VQAE_REQUIRE(B >= 0 && H >= 1 && W >= 1, VQAE_ERR_INVALID, "pixels_u8_level: bad shape");
    // (the level before the pointers: a level that leaves no pixel leaves the caller no destination to point at)
    if (int e = pixels_u8_level_check("pixels_u8_level", H, W, level, rc != nullptr, canvas_h, canvas_w)) return e;
    VQAE_REQUIRE(x && out, VQAE_ERR_INVALID, "pixels_u8_level: null pointer");
    if (level == 0) return pixels_u8(x, layout, B, H, W, rc, mean255, std255, out, canvas_h, canvas_w, stream);
    VQAE_REQUIRE((int64_t)H * W <= (1ll << 30), VQAE_ERR_UNSUPPORTED, "pixels_u8_level: tile of %d x %d pixels", H, W);
    const int oh = H >> level, ow = W >> level;
    if (!rc) VQAE_REQUIRE((int64_t)B * oh < (1ll << 31), VQAE_ERR_UNSUPPORTED, "pixels_u8_level: %d x %d rows", B, oh);
    if (B == 0) return VQAE_OK;
    Denorm3 dn;
    for (int c = 0; c < 3; ++c) {
        dn.mean[c] = mean255 ? mean255[c] : 0.f;
        dn.scale[c] = std255 ? std255[c] : 1.f;
    }
    const int out_h = rc ? canvas_h : B * oh, out_w = rc ? canvas_w : ow;
    // the 4-pixel path: 16-byte aligned loads as at level 0; its only stores wider than a byte are the 16-bit ones of
    // level 1 (W % 4 == 0 makes W / 2 even, so an even row pitch and an even base keep every one of them aligned)
    const bool vec = W % 4 == 0 && (uintptr_t)x % 16 == 0 && (level > 1 || (out_w % 2 == 0 && (uintptr_t)out % 2 == 0));
    const int items = oh * (vec ? W / 4 : ow);
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div(items, 256), 2048);
    const unsigned gy = (unsigned)std::min<int64_t>(B, std::max<int64_t>(1, 2048 / gx));
    const dim3 grid(gx, gy);
    const bool nchw = layout == VQAE_LAYOUT_NCHW;
    switch (level) {
        case 1: launch_level<1>(nchw, vec, grid, stream, x, B, H, W, rc, dn, out, out_h, out_w); break;
        case 2: launch_level<2>(nchw, vec, grid, stream, x, B, H, W, rc, dn, out, out_h, out_w); break;
        case 3: launch_level<3>(nchw, vec, grid, stream, x, B, H, W, rc, dn, out, out_h, out_w); break;
        case 4: launch_level<4>(nchw, vec, grid, stream, x, B, H, W, rc, dn, out, out_h, out_w); break;
        case 5: launch_level<5>(nchw, vec, grid, stream, x, B, H, W, rc, dn, out, out_h, out_w); break;
        default: launch_level<6>(nchw, vec, grid, stream, x, B, H, W, rc, dn, out, out_h, out_w); break;
    }
    VQAE_LAUNCH_CHECK();
    return VQAE_OK;
}

}  // namespace vqae

extern "C" int vqae_unstitch_tiles(const void* grid, int grid_dtype, const int32_t* rc, int n_tiles, int th, int tw,
                                   void* tiles, int idx_dtype, int gh, int gw, void* stream) {
    return vqae::unstitch_tiles(grid, grid_dtype, rc, n_tiles, th, tw, tiles, idx_dtype, gh, gw, (hipStream_t)stream);
}

extern "C" int vqae_pixels_u8(const float* x, int layout, int B, int H, int W, const int32_t* rc, const float* mean255,
                              const float* std255, uint8_t* out, int canvas_h, int canvas_w, void* stream) {
    return vqae::pixels_u8(x, layout, B, H, W, rc, mean255, std255, out, canvas_h, canvas_w, (hipStream_t)stream);
}

extern "C" int vqae_pixels_u8_level(const float* x, int layout, int B, int H, int W, int level, const int32_t* rc,
                                    const float* mean255, const float* std255, uint8_t* out, int canvas_h, int canvas_w,
                                    void* stream) {
    return vqae::pixels_u8_level(x, layout, B, H, W, level, rc, mean255, std255, out, canvas_h, canvas_w, (hipStream_t)stream);
}
