// Internal interface of libvqae_hip.so: every vqae:: function that one .hip file defines and another calls, declared once
// and grouped by defining file.  Each file that defines or calls one of them includes this header, so a changed parameter
// list fails to compile instead of failing to link.  The C ABI is include/vqae_hip.h; shared inline helpers are in common.h (host and device)
// and mfma.h (vector types, MFMA operands, the fragment order).
#pragma once
#include "common.h"

namespace vqae {

// ---- parameter bundles (plain data) ------------------------------------------------------------
// The Fixup scalars of one block (conv_block.py:196-216) in the order the fused kernels take them: the first eight are the
// `scalars8` of vqae_fixup_same_block_f32, all ten the scalars of a 'down' / 'up' block (b1c / b1d: the skip path, 0 for 'same').
struct FixupScalars {
    float b1a, b1b, b2a, b2b, b3a, b3b, b4, scale, b1c, b1d;
};
static_assert(sizeof(FixupScalars) == 10 * sizeof(float), "FixupScalars is read as float[8] / float[10]");

// What a trunk-tail launch needs to run the FOLLOWING block's conv1 as well ("chain"): that block's conv1 weights in the
// launching kernel's fragment order, its pre-activation scalars and where its t1 goes.  w1 == nullptr: no chain.
struct NextConv1 {
    const void* w1 = nullptr;     // float (fp32 tails) or 16-bit (trunk16) fragments
    const void* w1s = nullptr;    // split (3 x bf16) form of w1, read by the split F(4x4, 3x3) kernel only
    float b1a = 0.f, b1b = 0.f, b2a = 0.f, b2b = 0.f;
    void* t1_next = nullptr;      // float, or 16-bit for trunk16
};

// ---- conv_mfma.hip -----------------------------------------------------------------------------
// Channel counts conv_trunk_tail serves.
bool conv_trunk_tail_channels(int c);
// k-slice width of the engine conv_trunk_tail will use for this dtype / channel count (8: fp32 MFMA, 16: 16-bit MFMA);
// w3 / next.w1 must be in fragment order (frag_weight) for that width
int conv_tail_kslice(int dtype, int cin);
// Trunk tail, direct form: conv2 (3x3 circular; `a` carries its geometry and its ELU epilogue) + conv3 (+ next conv1).
// t1 [M][C] -> xio [M][C] updated in place (the block's output) and, when chained, next.t1_next [M][C].
int conv_trunk_tail(const vqae_conv_args* a, const float* t1, const float* w2, const float* w3, float t_scale, float t_b4,
                    float* xio, const NextConv1& next, hipStream_t stream);

// ---- conv_wino.hip -----------------------------------------------------------------------------
// Channel counts with a Winograd F(2x2, 3x3) trunk kernel: fp32 C in {256, 128, 64, 32}; 16-bit modes C = 32 only.
bool wino_trunk_channels(int c, int dtype);
// ... on a grid whose width is a multiple of the workgroup's column span (32, 32, 64, 128) and whose height is one of 4
bool wino_trunk_supported(int c, int h, int w, int dtype);
size_t wino_weight_floats(int c);
// w_oihw_dev [c][c][3][3] (PyTorch layout, device) -> U_dev [16][c][c] (fragment order)
int wino_transform_weight(const float* w_oihw_dev, int c, int dtype, float* U_dev, hipStream_t stream);
// The fp32 fragment packer (frag_offset, mfma.h): packed [n_rows][K] weights (device; vqae_conv_pack_weight_f32) -> fragment
// order (device); sk = 8 (fp32 MFMA k-slice) or 16 (16-bit MFMA); n_rows % 32 == 0, K % sk == 0
int frag_weight(const float* w_packed_dev, int n_rows, int K, int sk, float* out_dev, hipStream_t stream);
// Same contract as conv_trunk_tail: t1 -> xio in place (+ next.t1_next); U, w3, next.w1 in fragment order (k-slice 8).
int wino_trunk_tail(const float* t1, const float* U, const float* w3, float act_a, float act_b, float t_scale, float t_b4,
                    float* xio, const NextConv1& next, int batch, int h, int w, int c, int dtype, hipStream_t stream);
// chain-head conv1 (w1f in fragment order): fp32, C in {256, 128, 64, 32}, M a multiple of the kernel's pixel tile
bool fixup_conv1_supported(int c, int64_t m);
int fixup_conv1(const float* x, const float* w1f, float pa, float pb, float aa, float ab, float* y, int64_t m, int c,
                hipStream_t stream);

// ---- conv_wino43.hip ---------------------------------------------------------------------------
// Channel counts with an F(4x4, 3x3) trunk kernel (fp32): 256, 128, 64.  C = 32 keeps F(2x2, 3x3).
bool wino43_channels(int c);
// geometry only: 256 / 128 on the 32-wide grid, 64 on the 64-wide one, height a multiple of 8
bool wino43_supported(int c, int h, int w, int dtype);
bool wino43_enabled();          // VQAE_WINO43, read at every call
size_t wino43_weight_floats(int c);
// w_oihw_dev [c][c][3][3] (PyTorch layout, device) -> U_dev [36][c][c] (fragment order)
int wino43_transform_weight(const float* w_oihw_dev, int c, float* U_dev, hipStream_t stream);
// split form (GEMM operands as three bf16 planes): C = 128 only
bool wino43_split_supported(int c);
size_t wino43_split_weight_bytes(int c);
size_t split_1x1_bytes(int c);
int wino43_split_weight(const float* w_oihw_dev, int c, void* U_dev, hipStream_t stream);
// packed [c][c] 1x1 weights (device) -> the split tail fragments
int split_1x1_weight(const float* w_packed_dev, int c, void* out_dev, hipStream_t stream);
// Same contract as wino_trunk_tail.  Us non-null: the split form, which reads Us / w3s / next.w1s instead of U / w3 / next.w1
// (all of them must be given; next.w1s only when chained).
int wino43_trunk_tail(const float* t1, const float* U, const float* w3, float act_a, float act_b, float t_scale, float t_b4,
                      float* xio, const NextConv1& next, int batch, int h, int w, int c, hipStream_t stream,
                      const void* Us, const void* w3s);

// ---- trunk16.hip (16-bit modes) ----------------------------------------------------------------
// Channel counts whose 'same' blocks take 16-bit fragments [c][taps * c] (trunk16_block, or same16_16_block at C = 16 / 32).
bool trunk16_channels(int c);
// (C, grid width) pairs with a kernel; off under VQAE_NO_TRUNK16 (the weights are packed regardless)
bool trunk16_supported(int c, int h, int w, int dtype);
// bytes of a buffer for pack16_weight(c, taps * c) that trunk16_kernel may read: the fragments + its ring's look-ahead
size_t trunk16_weight_bytes(int c, int taps);
// fp32 [n] (n % 4 == 0) -> 16-bit, RNE: t1 of a chain head produced by the generic conv1 launch
int trunk16_round_pack(const float* src, void* dst, int64_t n, int dtype, hipStream_t stream);
// chain-head conv1: x fp32 [M][c] -> t1 16-bit [M][c] (out32: fp32, not rounded after the activation);
// w1f from pack16_weight([c][c]); C in {16, 32, 64, 128}, M % 32 == 0
bool trunk16_head_supported(int c, int64_t m, int dtype);
int trunk16_head(const float* x, const void* w1f, float b1a, float b1b, float b2a, float b2b, void* t1, int64_t m, int c,
                 int dtype, bool out32, hipStream_t stream);
// One trunk Fixup block: t1 (16-bit) -> xio updated in place (+ next.t1_next, 16-bit, when chained).
int trunk16_block(const void* t1, const void* w2f, const void* w3f, float act_a, float act_b, float t_scale, float t_b4,
                  float* xio, const NextConv1& next, int batch, int h, int w, int c, int dtype, hipStream_t stream);

// ---- same8_16.hip (16-bit modes, whole 'same' block per launch) --------------------------------
bool same8_16_channels(int c);          // 8
bool same8_16_supported(int c, int h, int w, int dtype);
// x -> y (x != y), [B][H][W][8] fp32; w1: packed fp32 (rounded) [>= 8][8]; w2h / w3h: pack16_weight(w2 [8][72]) / (w3 [8][8])
int same8_16_block(const float* x, float* y, const float* w1_packed, const void* w2h, const void* w3h, int B, int H, int W,
                   const FixupScalars& s, int dtype, hipStream_t stream);
// C = 16 / 32: x -> y (x != y), [B][H][W][C] fp32; w1h / w2h / w3h: pack16_weight([C][C]) / ([C][9 C]) / ([C][C])
bool same16_16_supported(int c, int h, int w, int dtype);
int same16_16_block(const float* x, float* y, const void* w1h, const void* w2h, const void* w3h, int B, int H, int W, int c,
                    const FixupScalars& s, int dtype, hipStream_t stream);

// ---- down_fused.hip / down16.hip ('down' block per launch: fp32 engine / 16-bit MFMA) ----------
bool down_block_channels(int cin);      // 16, 32, 64
// ... output width a multiple of 32, output height a multiple of the tile's rows (4, 2, 1)
bool down_block_supported(int cin, int h, int w);
// x [B][H][W][cin] -> y [B][H/2][W/2][2 cin]; weights in fragment order (frag_weight, k-slice 8)
int down_block(const float* x, const float* w1f, const float* w2f, const float* w3f, const float* wskf, int B, int H, int W,
               int cin, const FixupScalars& s, int dtype, float* y, hipStream_t stream);
bool down16_channels(int cin);          // 8, 16, 32, 64
// ... output width a multiple of 32, output height a multiple of the tile's rows (4, 4, 2, 1)
bool down16_supported(int cin, int h, int w);
size_t down16_weight_bytes(int n_rows, int K);
// The 16-bit fragment packer, for every kernel of the 16-bit modes but the stems: packed [>= max(n_rows, 32)][K] fp32 (device;
// vqae_conv_pack_weight_f32 pads the rows to 128 with zeros; K = taps * cin, tap-major) -> 16-bit fragment order (device);
// n_rows % 32 == 0 or n_rows in {8, 16}; K % 8 == 0 (padded to 16 with zeros); dtype bf16 / f16
int pack16_weight(const float* w_packed_dev, int n_rows, int K, int dtype, void* out_dev, hipStream_t stream);
// as down_block, weights from pack16_weight; dtype bf16 / f16
int down16_block(const float* x, const void* w1h, const void* w2h, const void* w3h, const void* wskh, int B, int H, int W,
                 int cin, const FixupScalars& s, int dtype, float* y, hipStream_t stream);

// ---- up16.hip (16-bit modes) -------------------------------------------------------------------
bool up16_channels(int c);              // the block's input channels: 16, 32, 64, 128
// ... low-resolution width a multiple of 16, output height a multiple of the tile's rows (4; 2 at c = 128): exactly what up16_block runs
bool up16_supported(int c, int h, int w, int dtype);
// x, t1 (trunk16_head, out32): [B][H][W][c] fp32 -> y [B][2H][2W][c / 2] fp32; weights: pack16_weight([c][c]), ([c / 2][c]), ([c / 2][c])
int up16_block(const float* x, const float* t1, const void* w2h, const void* w3h, const void* wskh, int B, int H, int W, int c,
               const FixupScalars& s, int dtype, float* y, hipStream_t stream);

// ---- stem16.hip (16-bit modes) -----------------------------------------------------------------
bool stem16_channels(int c0);           // stem widths: 8, 16, 32
bool stem16_supported(int c0, int h, int w, int dtype);
size_t stem16_weight_bytes(int cin);
// w: PyTorch [n_out][cin][3][3] fp32 (device) -> 16-bit fragments (device)
int stem16_pack_weight(const float* w_dev, int n_out, int cin, int dtype, void* out_dev, hipStream_t stream);
// in-stem: x (x_kind 0 NHWC f32 / 1 NCHW f32 / 2 uint8 NHWC + normalisation) -> y [B][H][W][c0] fp32
int istem16(const void* x, int x_kind, const float* mean255, const float* inv_std255, const void* wf, const float* bias, int B,
            int H, int W, int c0, float* y, int dtype, hipStream_t stream);
// out-stem: x [B][H][W][c] fp32 -> y (NCHW [B][3][H][W] if y_nchw else NHWC) fp32
int ostem16(const float* x, const void* wf, const float* bias, int B, int H, int W, int c, float* y, int y_nchw, int dtype,
            hipStream_t stream);

// ---- up_fused.hip (fp32 'up' blocks, convs before the resize) -----------------------------------
// Head: Q = skip_conv(x + b1c) + b1d and R = conv2(ELU(conv1(ELU(x + b1a) + b1b) + b2a) + b2b) in one launch, bit-identical to the
// three generic launches; x [M][c] -> q [M][c / 2], r [M][c]; c in {32, 64, 128}, any M; weights in fragment order (frag_weight,
// k-slice 8): w1f, w2f [c][c], wskf [max(c / 2, 32)][c] with zero rows past c / 2
bool up_head_channels(int c);
int up_head(const float* x, const float* w1f, const float* w2f, const float* wskf, int64_t M, int c, const FixupScalars& s,
            float* q, float* r, hipStream_t stream);
// Fused tail: both resizes, the ELU and conv3; (branch channels, out channels) in {(64, 32), (32, 16), (16, 8)}, any H, W >= 1
// q [B][H][W][cb], s [B][H][W][co] -> y [B][2H][2W][co]
bool up_tail_supported(int cb, int co);
int up_tail(const float* q, const float* s, const float* w3_packed, int B, int H, int W, int cb, int co, float b3a, float b3b,
            float scale, float b4, float* y, hipStream_t stream);

// ---- misc_kernels.hip --------------------------------------------------------------------------
// 1x1 / stride 1 or 2x2 / stride 2, no padding, cin == 8, cout % 4 == 0 (VALU kernel at the HBM rate)
bool conv_small_k_supported(const vqae_conv_args* a);
int conv_small_k(const vqae_conv_args* a, const float* x, const float* w, const float* bias_vec, const float* residual,
                 float* y, hipStream_t stream);
// the stems: x_kind 0 NHWC f32 / 1 NCHW f32 / 2 u8 NHWC; y_nchw 0/1
int conv3x3_direct(const void* x, int x_kind, const float* mean255, const float* inv_std255, const float* w,
                   const float* bias, int B, int H, int W, int cin, int cout, float* y, int y_nchw, int dt,
                   hipStream_t stream);

// ---- pixels.hip --------------------------------------------------------------------------------
// vqae_unstitch_tiles / vqae_pixels_u8 (include/vqae_hip.h) on a hipStream_t
int unstitch_tiles(const void* grid, int grid_dtype, const int32_t* rc, int n_tiles, int th, int tw, void* tiles,
                   int idx_dtype, int gh, int gw, hipStream_t stream);
int pixels_u8(const float* x, int layout, int B, int H, int W, const int32_t* rc, const float* mean255, const float* std255,
              uint8_t* out, int canvas_h, int canvas_w, hipStream_t stream);
// vqae_pixels_u8_level; its argument checks on their own (who: the caller's name for the message), so that a caller with
// several levels can refuse all of them before it launches anything
int pixels_u8_level_check(const char* who, int H, int W, int level, bool canvas, int canvas_h, int canvas_w);
int pixels_u8_level(const float* x, int layout, int B, int H, int W, int level, const int32_t* rc, const float* mean255,
                    const float* std255, uint8_t* out, int canvas_h, int canvas_w, hipStream_t stream);

// ---- ingest.hip --------------------------------------------------------------------------------
// vqae_cut_pixels_u8 / vqae_pool_labels_u8 (include/vqae_hip.h) on a hipStream_t
int cut_pixels_u8(const uint8_t* canvas, int canvas_h, int canvas_w, int ch, const int32_t* rc, int n_tiles, int h, int w, int y0,
                  int x0, int level, uint8_t* tiles, hipStream_t stream);
int pool_labels_u8(const uint8_t* mask, int mask_h, int mask_w, int y0, int x0, int win_h, int win_w, uint8_t* out, int out_h,
                   int out_w, hipStream_t stream);

// ---- vq_filter.hip / vq_kernels.hip ------------------------------------------------------------
bool vq_filter_supported(int K, int D);
size_t vq_filter_table_bytes(int K, int D);
// flags: 4 zeroed ints ([0] = flagged-row counter shared with tier 1 / tier 2).  After this call either idx32 / flag_list are
// filled (flags[1] == 0) or nothing was done and flags[1] != 0 tells vq_tier1_kernel to run.
int vq_filter_run(const float* z, const float* embed, int64_t N, int K, int D, float thr, int* idx32, int* flags, int* flag_list,
                  void* table, hipStream_t stream);
// shared with the fused projected quantiser (vq_proj.hip)
int vq_tier2_run(const float* z, const float* embed, int K, int D, int* idx32, const int* flag_count, const int* flag_list,
                 hipStream_t stream);
// *loss = commitment * mean((z - embed[idx])^2) (vq.py:143); partials: >= 1024 doubles of scratch
int vq_loss_from_idx(const float* z, const float* embed, const int* idx32, int64_t N, int D, float commitment, double* partials,
                     float* loss, hipStream_t stream);
int vq_write_idx(const int* idx32, int64_t N, void* out, int idx_dtype, hipStream_t stream);

// ---- vq_backward.hip ---------------------------------------------------------------------------
// The backward of both quantisers (vqae_vq_backward_f32, vqae_vq_projected_backward_f32 and its workspace size): C ABI
// only, include/vqae_hip.h.  Rows per workgroup and the number of fp64 partial rows are functions of n_rows alone
// (bw_grid there), which is what makes the gradients bit-identical run to run.

// ---- fixup_train.hip ---------------------------------------------------------------------------
// The training forms of a Fixup block's non-conv ops (vqae_fixup_act_f32 / _backward, vqae_fixup_out_f32 / _backward,
// vqae_bicubic_up2_bias_f32, vqae_bicubic_up2_backward_f32 and their workspace size): C ABI only, include/vqae_hip.h.  The
// grid and the number of fp64 partial rows are functions of the shape alone (ft_grid there).

// ---- mbconv_train.hip --------------------------------------------------------------------------
// The training forms of an MBConv block's non-dense ops (vqae_bn_act_train_*, vqae_dwconv_train_*, vqae_se_scale_*): C ABI
// only, include/vqae_hip.h.  One workgroup reduces VQAE_MBT_ROWS rows; the grid and the number of fp64 partial rows are
// functions of the shape alone.

// ---- conv_train.hip ----------------------------------------------------------------------------
// The trainable 1x1, 2x2 stride-2 and circular 3x3 convs: C ABI only, include/vqae_hip.h.  Its two final-sum launches serve
// conv_train_thin.hip (the zero-padded 3x3 convs with a 3-channel side) as well:
// partials [n_rows][2] doubles -> *o0, *o1 (each may be NULL): one workgroup, fixed order, one rounding
int conv_train_sum_final(const double* partials, int n_rows, float* o0, float* o1, hipStream_t stream);
// slots [P][n] doubles, an element order [cout][taps][cin] -> g_w [n] floats in the weight's layout (w_layout 1: that order,
// 0: [cout][cin][taps]): the P slots added in index order in fp64, rounded once
int conv_train_wgrad_final(const double* slots, int P, int n, int cin, int taps, int w_layout, float* g_w, hipStream_t stream);

}  // namespace vqae
