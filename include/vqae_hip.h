/* vqae_hip.h -- C ABI of libvqae_hip.so: the MI355X (gfx950) native VQ-AE inference hot path.
 *
 * Drop-in boundary for sara-nl/2D-VQ-AE-2's conv-encoder -> vector-quantise -> conv-decoder
 * forward pass.  The reference has no native interface: its plugin mechanism is
 * Hydra `_target_` class-path substitution (conf/model/layers/vq/ema_vq.yaml:1,
 * conf/model/layers/conv_block/pre_activation_fixup.yaml:24, conf/model/{encoder,decoder}/default.yaml) over
 * nn.Module.forward contracts.  Each entry point below cites the reference interface it replaces;
 * INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain C types only; every `*_dev` pointer is a device (HBM) pointer owned by the caller;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all calls are
 *     asynchronous on it and allocate nothing (handle workspaces grow only inside
 *     vqae_reserve / on the first call with a larger batch, never during steady state);
 *   - activations are fp32, NHWC ("channels-last": [B][H][W][C], C contiguous).  NCHW tensors
 *     (the reference's layout, model.py:189) cross the boundary through vqae_nchw_to_nhwc /
 *     vqae_nhwc_to_nchw or the `layout` argument of the handle-level calls;
 *   - return value: 0 on success, negative vqae_status otherwise; vqae_last_error() returns a
 *     thread-local message.  The Python binding maps them back to the reference's exception
 *     types (AssertionError / NotImplementedError / ValueError), see vqae_status.
 */
#ifndef VQAE_HIP_H
#define VQAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vqae_status {
    VQAE_OK = 0,
    VQAE_ERR_INVALID = -1,        /* bad argument / failed assert  (reference: AssertionError, vq.py:98, conv_block.py:148) */
    VQAE_ERR_UNSUPPORTED = -2,    /* reference: NotImplementedError (vq.py:100-104) */
    VQAE_ERR_HIP = -3,            /* HIP runtime failure */
    VQAE_ERR_NOMEM = -4,
    VQAE_ERR_NOT_FOUND = -5,      /* missing tensor name in a weight set (reference: KeyError in load_state_dict) */
    VQAE_ERR_VALUE = -6           /* reference: ValueError (torchmetrics SSIM on an image smaller than its window) */
} vqae_status;

enum { VQAE_LAYOUT_NHWC = 0, VQAE_LAYOUT_NCHW = 1 };
/* Compute precision of the convolutions, with torch.autocast semantics (the reference's extraction runs
 * `with torch.autocast('cuda')`, scripts/extract_embeddings/extract_embeddings.py:124-125): conv inputs,
 * weights and conv biases are rounded (RNE) to the 16-bit type, products are accumulated in fp32, the conv
 * output is rounded to the 16-bit type; everything else (Fixup scalar biases/scale, ELU, residual adds,
 * bicubic, the p=4 distance, losses) stays fp32, exactly as type promotion leaves it in the reference. */
enum { VQAE_DT_F32 = 0, VQAE_DT_BF16 = 1, VQAE_DT_F16 = 2 };
enum { VQAE_IDX_I64 = 0, VQAE_IDX_U8 = 1, VQAE_IDX_U16 = 2, VQAE_IDX_I32 = 3 };

const char* vqae_last_error(void);
/* "gfx950;<git describe or build date>" */
const char* vqae_build_info(void);

/* ---------------------------------------------------------------------------------------------
 * 1. Vector quantiser  -- replaces EMAVectorQuantizer.forward, vq_ae/layers/vq.py:96-154
 *    (eval mode) and embed_code, vq.py:44-45.
 * ------------------------------------------------------------------------------------------- */

/* Bytes of scratch vqae_vq_forward_f32 needs for N rows (tie re-check list, loss partials). */
size_t vqae_vq_workspace_bytes(int64_t n_rows, int n_codes, int dim);

/* idx[n] = argmin_k ( sum_c |z[n][c] - embed[k][c]|^4 )^(1/4), lowest k on ties
 *          (vq.py:121-129: torch.cdist(flat, embed, p = inputs.dim() = 4) + argmin(dim=1));
 * q[n]   = z[n] + (embed[idx[n]] - z[n])        (vq.py:130,146: lookup + straight-through value);
 * *loss  = commitment_cost * mean((z - embed[idx])^2)   (vq.py:143).
 *   z_dev     [n_rows][dim] fp32 (the NHWC activation, i.e. the reference's `flat_input`, vq.py:116)
 *   embed_dev [n_codes][dim] fp32 (buffer `embed`, vq.py:27)
 *   idx_dev   [n_rows] of idx_dtype (VQAE_IDX_*); required
 *   q_dev     [n_rows][dim] fp32 or NULL;  loss_dev  one fp32 or NULL
 *   margin_dev [n_rows] fp32 or NULL: relative gap between best and second-best 4th-power sums
 *   workspace_dev: vqae_vq_workspace_bytes(...) bytes.
 *   dim: any 1 .. 4096 like the reference; a dim that is not a multiple of 4 runs on zero-padded copies of z and of the
 *   codebook (stream-ordered scratch): the same sums, indices and q bit for bit.
 * Errors: dim < 1 or > 4096, n_codes < 1 or > 65536 -> VQAE_ERR_UNSUPPORTED. */
int vqae_vq_forward_f32(const float* z_dev, const float* embed_dev, int64_t n_rows, int n_codes, int dim,
                        float commitment_cost, void* idx_dev, int idx_dtype, float* q_dev, float* loss_dev,
                        float* margin_dev, void* workspace_dev, void* stream);

/* The same with the Minkowski exponent spelled out: the reference passes `p = inputs.dim()` to torch.cdist (vq.py:97,121-129), i.e.
 * p = 3 for [B, D, L] inputs, 4 for [B, D, h, w] (vqae_vq_forward_f32), 5 for [B, D, d, h, w]:
 *   idx[n] = argmin_k ( sum_c |z[n][c] - embed[k][c]|^p )^(1/p), lowest k on ties.
 * z_dev is the channel-last flattening of the input (vq.py:107-116) whatever its rank.
 * Errors: p outside 3 .. 5 -> VQAE_ERR_UNSUPPORTED; otherwise as vqae_vq_forward_f32. */
int vqae_vq_forward_p_f32(const float* z_dev, const float* embed_dev, int64_t n_rows, int n_codes, int dim, int p,
                          float commitment_cost, void* idx_dev, int idx_dtype, float* q_dev, float* loss_dev,
                          float* margin_dev, void* workspace_dev, void* stream);

/* ProjectedEMAVectorQuantizer2d.forward (vq.py:190-192), projection_dim = 8 (the reference default,
 * conf/model/layers/vq/projected_ema_vq_2d.yaml): proj_out(VQ(proj_in(x))) in one pass over the activation.
 *   x_dev      [n_rows][channels] fp32 (NHWC activation)
 *   wt_in_dev  [channels][8]   proj_in.weight  ([8][channels][1][1], vq.py:178-182) TRANSPOSED
 *   b_in_dev   [8]             proj_in.bias
 *   embed_dev  [n_codes][8]    buffer `embed` (vq.py:27)
 *   w_out_dev  [channels][8]   proj_out.weight ([channels][8][1][1], vq.py:183-187) as stored
 *   b_out_dev  [channels]      proj_out.bias
 *   dtype      VQAE_DT_*: autocast rounding of the two convolutions (weights / biases pre-rounded by the caller)
 *   idx_dev    [n_rows] idx_dtype; out_dev [n_rows][channels] = proj_out(z + (embed[idx] - z)); z_dev [n_rows][8] or NULL
 *   loss_dev   commitment_cost * mean((z - embed[idx])^2) in the 8-D space, or NULL; margin_dev as vqae_vq_forward_f32
 *   workspace_dev: vqae_vq_projected_workspace_bytes(n_rows) bytes.
 * Errors: projection_dim != 8, channels % 4 != 0 -> VQAE_ERR_UNSUPPORTED. */
size_t vqae_vq_projected_workspace_bytes(int64_t n_rows);
int vqae_vq_projected_f32(const float* x_dev, const float* wt_in_dev, const float* b_in_dev, const float* embed_dev,
                          const float* w_out_dev, const float* b_out_dev, int64_t n_rows, int channels, int projection_dim,
                          int n_codes, float commitment_cost, int dtype, void* idx_dev, int idx_dtype, float* out_dev,
                          float* z_dev, float* loss_dev, float* margin_dev, void* workspace_dev, void* stream);

/* Backward of EMAVectorQuantizer.forward (vq.py:143-146): the gradient autograd gives `inputs` through
 *   loss = commitment_cost * mse_loss(inputs, quantized) (vq.py:143) and quantized = inputs + (quantized - inputs).detach()
 *   (vq.py:146), on the channel-last rows of vq.py:107-116:
 *   g_z[n][c] = g_q[n][c] + g_loss * commitment_cost * 2 / (n_rows * dim) * (z[n][c] - q[n][c]).
 *   g_q_dev    [n_rows][dim] incoming gradient of the first output, or NULL (zero)
 *   z_dev, q_dev [n_rows][dim] the forward's rows and its lookup (the q of the PRE-update codebook in training mode)
 *   g_loss_dev one fp32 ON THE DEVICE, the incoming gradient of the loss, or NULL (zero; z / q are then not read):
 *              the kernel forms the scale itself, so no value is read back and nothing synchronises
 *   g_z_dev    [n_rows][dim]; may alias g_q_dev.   dim: any 1 .. 4096.  n_rows == 0 -> VQAE_OK. */
int vqae_vq_backward_f32(const float* g_q_dev, const float* z_dev, const float* q_dev, const float* g_loss_dev,
                         float commitment_cost, int64_t n_rows, int dim, float* g_z_dev, void* stream);

/* Backward of ProjectedEMAVectorQuantizer2d.forward (vq.py:190-192 around vq.py:143-146), projection_dim = 8, in one pass
 * over g_out and x (each read once, g_x written once):
 *   g_q = g_out W_out                      g_W_out = g_out^T q    [channels][8]     g_b_out = sum_n g_out  [channels]
 *   g_z = g_q + g_loss cc 2 / (8 n_rows) (z - q)    g_W_in = g_z^T x  [8][channels]     g_b_in  = sum_n g_z    [8]
 *   g_x = g_z W_in
 *   g_out_dev  [n_rows][channels] incoming gradient of the output (NHWC rows), or NULL (zero)
 *   x_dev [n_rows][channels], z_dev [n_rows][8] = proj_in(x), q_dev [n_rows][8]: saved by the forward
 *   g_loss_dev one fp32 on the device or NULL, as vqae_vq_backward_f32
 *   wt_in_dev [channels][8] proj_in.weight TRANSPOSED, w_out_dev [channels][8] proj_out.weight as stored
 *     (the layouts of vqae_vq_projected_f32)
 *   g_x_dev [n_rows][channels], g_w_in_dev [8][channels], g_b_in_dev [8], g_w_out_dev [channels][8], g_b_out_dev [channels]:
 *     each may be NULL (not written)
 *   workspace_dev: vqae_vq_projected_backward_workspace_bytes(n_rows, channels) bytes.
 * The three sums over n_rows are accumulated in fp64 per workgroup, written to the workspace and added in index order by a
 * second launch; the grid is a function of the shapes alone and there are no floating-point atomics: bit-identical run to
 * run.  n_rows == 0 writes zeros.
 * Errors: projection_dim != 8, channels % 4 != 0, channels > 256 -> VQAE_ERR_UNSUPPORTED. */
size_t vqae_vq_projected_backward_workspace_bytes(int64_t n_rows, int channels);
int vqae_vq_projected_backward_f32(const float* g_out_dev, const float* x_dev, const float* z_dev, const float* q_dev,
                                   const float* g_loss_dev, const float* wt_in_dev, const float* w_out_dev, int64_t n_rows,
                                   int channels, int projection_dim, float commitment_cost, float* g_x_dev,
                                   float* g_w_in_dev, float* g_b_in_dev, float* g_w_out_dev, float* g_b_out_dev,
                                   void* workspace_dev, void* stream);

/* out[n][:] = embed[idx[n]][:]   (embed_code, vq.py:44-45 = F.embedding) */
int vqae_embed_code_f32(const void* idx_dev, int idx_dtype, const float* embed_dev, int64_t n_rows, int n_codes,
                        int dim, float* out_dev, void* stream);

/* Training-mode bookkeeping (vq.py:47-74 `_update_ema`): counts n_k and sums dw_k of the rows
 * assigned to each code.  counts_dev [n_codes] fp32, dw_dev [n_codes][dim] fp32 (both overwritten).
 * n_rows == 0 (a rank's empty shard; z_dev / idx_dev may be NULL) zero-fills both.  dim <= 512. */
int vqae_vq_code_stats_f32(const float* z_dev, const void* idx_dev, int idx_dtype, int64_t n_rows, int n_codes,
                           int dim, float* counts_dev, float* dw_dev, void* stream);
/* EMA + Laplace smoothing step of `_update_ema` (vq.py:60-74), after the caller all-reduced
 * counts/dw over ranks (vq.py:57-58): updates cluster_size, embed_avg, embed in place.
 * decay and laplace_alpha are the module's Python doubles: decay, 1 - decay, laplace_alpha and
 * n_codes * laplace_alpha are formed in double and rounded to fp32 once, as torch does. */
int vqae_vq_ema_update_f32(float* embed_dev, float* embed_avg_dev, float* cluster_size_dev, const float* counts_dev,
                           const float* dw_dev, int n_codes, int dim, double decay, double laplace_alpha,
                           void* workspace_dev /* >= 16 bytes */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 2. Conv stack primitives -- replace the torch.nn.Conv2d / ELU / Upsample call sites of
 *    PreActFixupResBlock.forward (vq_ae/layers/conv_block.py:196-216) and ResizeConv2D.forward
 *    (vq_ae/layers/conv.py:10-11).
 * ------------------------------------------------------------------------------------------- */

enum { VQAE_PAD_NONE = 0, VQAE_PAD_CIRCULAR = 1, VQAE_PAD_ZEROS = 2 };
enum { VQAE_PRE_NONE = 0, VQAE_PRE_BIAS = 1, VQAE_PRE_BIAS_ELU_BIAS = 2, VQAE_PRE_CHANNEL_GATE = 3 };
enum { VQAE_ACT_NONE = 0, VQAE_ACT_ELU = 1, VQAE_ACT_SILU = 2 };      /* vqae_conv_args.has_act */

/* Floats needed for the packed form of a [cout][cin][k][k] weight (rows padded to 32 couts). */
size_t vqae_conv_packed_floats(int cout, int cin, int ksize);
/* Repack a PyTorch-layout conv weight [cout][cin][k][k] (device) into the kernel's
 * [cout_pad][k*k*cin] layout (tap-major K, zero rows for the pad). */
int vqae_conv_pack_weight_f32(const float* w_oihw_dev, int cout, int cin, int ksize, float* packed_dev,
                              void* stream);

typedef struct vqae_conv_args {
    /* geometry: y[b][oy][ox][:] = sum_{dy,dx,ci} W[:, ci, dy, dx] * pre(x[b][oy*stride+dy-pad][ox*stride+dx-pad][ci]) */
    int batch, in_h, in_w, cin, cout;
    int ksize;            /* 1, 2 or 3 */
    int stride;           /* 1 or 2 */
    int pad;              /* 0 or 1 */
    int pad_mode;         /* VQAE_PAD_* (circular: padding_mode='circular', pre_activation_fixup.yaml:56-58) */
    /* pre-op on the input (Fixup scalar biases, conv_block.py:199-206,211):
     *   VQAE_PRE_BIAS:           x + pre_a
     *   VQAE_PRE_BIAS_ELU_BIAS:  ELU(x + pre_a) + pre_b        (ELU alpha = 1, activation/elu.yaml)
     *   VQAE_PRE_CHANNEL_GATE:   x * gate[b][ci]               (SELayer's `x * y`, layers/misc.py:30; only through
     *                                                           vqae_conv2d_gated_f32: fp32, 1x1, cin % 32 == 0) */
    int pre_mode;
    float pre_a, pre_b;
    /* epilogue, in the reference's rounding order (conv_block.py:208-214):
     *   t = acc; if (bias_vec) t = t + bias_vec[c];  (the conv's own bias)   t = round_dtype(t);
     *   if (has_scale) t = t * scale + bias_s;  else if (has_bias_s) t = t + bias_s;
     *   if (residual) t = t + residual[m][c];
     *   has_act == VQAE_ACT_ELU:  t = ELU(t + act_a) + act_b;   (the NEXT conv's pre-op, fused here)
     *   has_act == VQAE_ACT_SILU: t = t * sigmoid(t)            (MBConv: activation/silu.yaml after the folded BN) */
    int has_scale, has_bias_s, has_act;
    float scale, bias_s, act_a, act_b;
    int dtype;            /* VQAE_DT_*: autocast rounding of operands (after the pre-op) and of acc (+ bias_vec) */
} vqae_conv_args;

/* x_dev [B][H][W][cin], w_packed_dev from vqae_conv_pack_weight_f32, bias_vec_dev [cout] or NULL,
 * residual_dev [B][Ho][Wo][cout] or NULL, y_dev [B][Ho][Wo][cout].  fp32 MFMA implicit GEMM.
 * Requires cin % 8 == 0 (use vqae_conv_small_cin_f32 for the 3-channel stem). */
int vqae_conv2d_f32(const vqae_conv_args* a, const float* x_dev, const float* w_packed_dev,
                    const float* bias_vec_dev, const float* residual_dev, float* y_dev, void* stream);

/* Same conv with the input multiplied by a per-(image, input channel) gate [B][cin] while it is loaded
 * (a->pre_mode == VQAE_PRE_CHANNEL_GATE): conv3 of an MBConv consuming SELayer's output without materialising it
 * (conv_block.py:290-297, layers/misc.py:30). */
int vqae_conv2d_gated_f32(const vqae_conv_args* a, const float* x_dev, const float* gate_dev, const float* w_packed_dev,
                          const float* bias_vec_dev, const float* residual_dev, float* y_dev, void* stream);

/* ---- MBConv pieces (vq_ae/layers/conv_block.py:240-321; BatchNorms folded into weights/bias by the caller) ----
 * Depthwise conv over NHWC x [B][H][W][C] (branch_conv2 with groups = C, conv_block.py:276-281):
 *   VQAE_DW_SAME  3x3 / stride 1 / circular pad     (same2d.yaml + padding_mode circular, mbconv.yaml:60-63)
 *   VQAE_DW_DOWN  2x2 / stride 2                     (down2d.yaml)
 *   VQAE_DW_UP    ConvTranspose2d 2x2 / stride 2     (up2d.yaml)
 * w_taps_dev [k*k][C] (tap-major), bias_dev [C] or NULL, optional SiLU; y_dev [B][Ho][Wo][C].
 * If partial_dev != NULL (vqae_dw_partial_floats() floats) it receives per-(image, 256-pixel strip, channel) sums of
 * y for SELayer's spatial mean, reduced in a fixed order (bit-reproducible run to run). */
enum { VQAE_DW_SAME = 0, VQAE_DW_DOWN = 1, VQAE_DW_UP = 2 };
size_t vqae_dw_partial_floats(int batch, int out_h, int out_w, int channels);
int vqae_dwconv_f32(const float* x_dev, const float* w_taps_dev, const float* bias_dev, int batch, int h, int w,
                    int channels, int mode, int silu, float* y_dev, float* partial_dev, void* stream);
/* SELayer.forward up to the gate (layers/misc.py:23-29): mean over (out_h, out_w) from the partial sums ->
 * Linear(channels, hidden) -> SiLU -> Linear(hidden, channels) -> sigmoid; gate_dev [B][channels].
 * fc*_w are nn.Linear weights [out][in] on the device. */
int vqae_se_gate_f32(const float* partial_dev, int batch, int out_h, int out_w, int channels, const float* fc0_w_dev,
                     const float* fc0_b_dev, int hidden, const float* fc2_w_dev, const float* fc2_b_dev, float* gate_dev,
                     void* stream);
/* x [B][H][W][4*c] with channel order (a, b, c) -> y [B][2H][2W][c], y[2i+a][2j+b] = x[i][j][(a, b, :)]: the pixel
 * placement of ConvTranspose2d(k = 2, s = 2) (skip_conv of an 'up' MBConv) after its channel mixing ran as a 1x1 conv. */
int vqae_pixel_shuffle2_f32(const float* x_dev, int batch, int h, int w, int c, float* y_dev, void* stream);

/* One whole PreActFixupResBlock.forward, mode 'same' (conv_block.py:196-216: 1x1 -> 3x3 circular -> 1x1,
 * in_channels == out_channels == c) in a single launch, for the HBM-bound high-resolution levels.
 * x_dev, y_dev [B][H][W][c] (y != x: neighbouring tiles read halo rows of x); w*_packed_dev from
 * vqae_conv_pack_weight_f32; scalars8 (host) = {bias1a, bias1b, bias2a, bias2b, bias3a, bias3b, bias4, scale}.
 * vqae_fixup_same_supported() tells whether a (c, h, w) has a fused kernel (c in {8, 16, 32}, w % 32 == 0). */
int vqae_fixup_same_supported(int c, int h, int w);
int vqae_fixup_same_block_f32(const float* x_dev, float* y_dev, const float* w1_packed_dev, const float* w2_packed_dev,
                              const float* w3_packed_dev, int batch, int h, int w, int c, const float* scalars8,
                              int dtype /* VQAE_DT_* */, void* stream);
/* Round a device fp32 array in place to bf16/f16-representable values (autocast weight cast). */
int vqae_round_inplace_f32(float* x_dev, int64_t n, int dtype, void* stream);

/* Direct (VALU) 3x3 / stride 1 / zero-pad conv with per-channel bias for tiny channel counts:
 * the stems `in_stem` (3 -> C0, model.py:198) and `out_stem` (C0 -> 3, model.py:291).
 * w_oihw_dev is the PyTorch-layout weight [cout][cin][3][3]; cin, cout <= 64.
 * If x_u8_dev != NULL the input is uint8 NHWC and is normalised on the fly
 * ((u - mean255[c]) * inv_std255[c], albumentations Normalize, camelyon16_transforms.yaml:15-23). */
int vqae_conv3x3_direct_f32(const float* x_dev, const uint8_t* x_u8_dev, const float* mean255, const float* inv_std255,
                            const float* w_oihw_dev, const float* bias_dev, int batch, int h, int w, int cin,
                            int cout, float* y_dev, int dtype /* VQAE_DT_* */, void* stream);

/* y = bicubic_x2(x + pre_bias), A = -0.75, align_corners = False, index-clamped borders
 * (nn.Upsample(mode='bicubic', scale_factor=2), layers/conv.py:8).  x [B][H][W][C] -> y [B][2H][2W][C]. */
int vqae_bicubic_up2_f32(const float* x_dev, int batch, int h, int w, int c, float pre_bias, float* y_dev,
                         void* stream);

/* Layout shuffles at the boundary (reference tensors are NCHW, model.py:189). */
int vqae_nchw_to_nhwc_f32(const float* x_dev, int batch, int c, int h, int w, float* y_dev, void* stream);
int vqae_nhwc_to_nchw_f32(const float* x_dev, int batch, int c, int h, int w, float* y_dev, void* stream);

/* labels [B][H][W] (u8) -> [B][out][out] max over (H/out x W/out) windows
 * (F.adaptive_max_pool2d in run_eval, scripts/extract_embeddings/extract_embeddings.py:127-130). */
int vqae_label_maxpool_u8(const uint8_t* labels_dev, int batch, int h, int w, int out, uint8_t* y_dev, void* stream);

/* Stitch code tiles into a slide grid (get_encodings, extract_embeddings.py:77-84):
 * grid[(r*th + y) * grid_w + c*tw + x] = tiles[t][y][x] for tile t at patch position (r, c) = rc[t].
 * tiles idx_dtype in, grid_dtype out (VQAE_IDX_*; narrowing is the caller's cast_to_lowest_dtype choice). */
int vqae_stitch_tiles(const void* tiles_dev, int idx_dtype, const int32_t* rc_dev, int n_tiles, int th, int tw,
                      void* grid_dev, int grid_dtype, int grid_h, int grid_w, void* stream);

/* Cut a stored slide grid back into code tiles: the exact inverse of vqae_stitch_tiles, i.e. of the grid layout of
 * get_encodings (scripts/extract_embeddings/extract_embeddings.py:77-84):
 * tiles[t][y][x] = grid[(r*th + y) * grid_w + c*tw + x] for (r, c) = rc[t].
 * grid grid_dtype in (as stored: uint8 / uint16 / wider), tiles idx_dtype out (VQAE_IDX_*, every pairing vqae_stitch_tiles
 * takes; widening is exact).  An element whose grid position lies outside the grid is neither read nor written (the tile
 * keeps what it held): the caller validates positions on the host. */
int vqae_unstitch_tiles(const void* grid_dev, int grid_dtype, const int32_t* rc_dev, int n_tiles, int th, int tw,
                        void* tiles_dev, int idx_dtype, int grid_h, int grid_w, void* stream);

/* fp32 reconstruction -> uint8 NHWC pixels: the inverse of the Normalize transform vqae_conv3x3_direct_f32 applies on ingest
 * (albumentations Normalize, camelyon16_transforms.yaml:15-23), per channel c
 *   u = clamp(rintf(fmaf(x, std255[c], mean255[c])), 0, 255)     one fused multiply-add, round-to-nearest-even, NaN -> 0.
 *   x_dev      [B][H][W][3] (VQAE_LAYOUT_NHWC) or [B][3][H][W] (VQAE_LAYOUT_NCHW) fp32
 *   mean255, std255  host arrays of 3 (NULL -> 0 / 1)
 *   rc_dev == NULL: out_dev is a dense [B][H][W][3] batch and canvas_h = canvas_w = 0;
 *   otherwise tile t is pasted into the canvas out_dev [canvas_h][canvas_w][3] at pixel (rc[t].r * H, rc[t].c * W); a tile
 *   that does not lie wholly inside the canvas is skipped (no access outside it), the rest of the canvas is not written.
 * Errors: null pointers / bad layout / canvas sizes with a dense destination / a canvas smaller than one tile ->
 * VQAE_ERR_INVALID. */
int vqae_pixels_u8(const float* x_dev, int layout, int batch, int h, int w, const int32_t* rc_dev, const float* mean255,
                   const float* std255, uint8_t* out_dev, int canvas_h, int canvas_w, void* stream);

/* The same pixels, box-reduced to overview level L (f = 2^level) on the device: with u[y][x][c] the level-0 pixel exactly as
 * vqae_pixels_u8 defines it,
 *   out[Y][X][c] = ( sum over dy < f, dx < f of u[f*Y + dy][f*X + dx][c]  +  f*f/2 ) >> (2*level)
 * an integer mean of the rounded uint8 pixels that rounds half up -- what box-filtering the level-0 image gives.  The sums are
 * integers (255 * 4^level + f*f/2 fits 32 bits), so the result does not depend on the summation order; every level is
 * defined from level 0, not from the level below.  level == 0 is vqae_pixels_u8.
 *   rc_dev == NULL: out_dev is a dense [B][H/f][W/f][3] batch and canvas_h = canvas_w = 0;
 *   otherwise tile t is pasted as an (H/f) x (W/f) block into the canvas out_dev [canvas_h][canvas_w][3], given in level-L
 *   pixels, at pixel (rc[t].r * H/f, rc[t].c * W/f); a tile at a negative position or one that does not lie wholly inside the
 *   canvas is skipped (no access outside it), the rest of the canvas is not written.
 * Errors: as vqae_pixels_u8 (a canvas smaller than one reduced tile); level < 0, or f not dividing both h and w ->
 * VQAE_ERR_INVALID; level > VQAE_MAX_PIXEL_LEVEL -> VQAE_ERR_UNSUPPORTED. */
enum { VQAE_MAX_PIXEL_LEVEL = 6 };
int vqae_pixels_u8_level(const float* x_dev, int layout, int batch, int h, int w, int level, const int32_t* rc_dev,
                         const float* mean255, const float* std255, uint8_t* out_dev, int canvas_h, int canvas_w,
                         void* stream);

/* Cut encoder tiles out of a resident uint8 pixel canvas, box-reduced to level L (f = 2^level): the device form of
 * CAMELYON16SlicePatchDataSet.__getitem__ (datamodules/camelyon16.py:149-211: the patch at patch position (r, c) is the
 * patch_size block at pixel (r, c) * patch_size of the slide's level) for a slide that is already an array:
 *   tiles[t][y][x][c] = ( sum over dy < f, dx < f of canvas[y0 + (rc[t].r*h + y)*f + dy][x0 + (rc[t].c*w + x)*f + dx][c]
 *                         +  f*f/2 ) >> (2*level)
 *   canvas_dev [canvas_h][canvas_w][ch] uint8, ch 1 or 3; tiles_dev dense [n_tiles][h][w][ch] uint8, what vqae_encode_u8 takes;
 *   rc_dev [n_tiles][2] int32 patch positions as get_encodings uses them (extract_embeddings.py:77-84); (y0, x0) a pixel
 *   origin in the canvas.  level 0 is a plain copy; level L > 0 is the integer rule of vqae_pixels_u8_level: exact sums,
 *   rounding half up, independent of the summation order.  Row offsets are 64-bit (a 100 000 x 200 000-pixel canvas indexes
 *   correctly); every canvas byte of a tile is read once, in 16-byte loads where the rows are 16-byte aligned.
 * A tile at a negative position or one that does not lie wholly inside the canvas is skipped (no access outside it) and its
 * destination left untouched, the convention of vqae_unstitch_tiles.
 * Errors: ch outside {1, 3}, a bad shape, a negative origin or level, a canvas that holds no tile at the origin, null pointers
 * -> VQAE_ERR_INVALID; level > VQAE_MAX_PIXEL_LEVEL -> VQAE_ERR_UNSUPPORTED. */
int vqae_cut_pixels_u8(const uint8_t* canvas_dev, int canvas_h, int canvas_w, int ch, const int32_t* rc_dev, int n_tiles, int h,
                       int w, int y0, int x0, int level, uint8_t* tiles_dev, void* stream);

/* Pool a mask canvas straight into a label grid:
 *   out[Y][X] = max over dy < win_h, dx < win_w of mask[y0 + Y*win_h + dy][x0 + X*win_w + dx]
 * mask_dev [mask_h][mask_w] uint8, out_dev dense [out_h][out_w] uint8.  Tiles are aligned and do not overlap and a code tile
 * is patch / 2^n_down, so the per-tile F.adaptive_max_pool2d of run_eval (scripts/extract_embeddings/extract_embeddings.py:
 * 127-130) over a region is ONE window maximum with win = 2^n_down * 2^level over the region's mask: a streaming pass that
 * reads every mask byte once (vqae_label_maxpool_u8 remains the per-batch form).
 * Errors: a bad shape, a negative origin, a window reaching outside the mask, null pointers -> VQAE_ERR_INVALID. */
int vqae_pool_labels_u8(const uint8_t* mask_dev, int mask_h, int mask_w, int y0, int x0, int win_h, int win_w, uint8_t* out_dev,
                        int out_h, int out_w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 3. Whole-model handle-- replaces Encoder.forward (vq_ae/model.py:189-217), Decoder.forward
 *    (:274-291) and VQAE.forward (:41-48) for the single-VQ-level Fixup model that every shipped
 *    config composes.
 * ------------------------------------------------------------------------------------------- */
typedef struct vqae_config {
    int in_channels;      /* 3                 conf/model/vq_ae.yaml:23 */
    int stem;             /* stem out_channels vq_ae.yaml:24 */
    int n_down;           /* vq_ae.yaml:26 */
    int n_pre, n_post;    /* vq_ae.yaml:27-28 */
    int n_enc;            /* n_pre_enc_layers = n_post_enc_layers, vq_ae.yaml:29,39 */
    int num_embeddings;   /* layers/vq/ema_vq.yaml:2 */
    int projection_dim;   /* 0: EMAVectorQuantizer; >0: ProjectedEMAVectorQuantizer2d (vq.py:157-192) */
    float commitment_cost;
    int compute_dtype;    /* VQAE_DT_F32 (default) or autocast bf16 / f16 */
    int block_kind;       /* VQAE_BLOCK_FIXUP (default) | VQAE_BLOCK_MBCONV (conf/model/{encoder,decoder}/efficientnetv2.yaml) */
    int expand_ratio;     /* MBConv: mbconv.yaml:32 (4) */
    int se_divisor;       /* MBConv: layers/misc/se.yaml:5 (4) */
    float bn_eps;         /* MBConv: layers/misc/batchnorm2d.yaml:4 (1e-5) */
} vqae_config;
enum { VQAE_BLOCK_FIXUP = 0, VQAE_BLOCK_MBCONV = 1 };

/* One named fp32 host tensor, named as in the reference's state_dict, e.g.
 * "encoder.pre_enc_layers.0.7.branch_conv2.weight" with PyTorch shapes ([cout][cin][k][k], (1,) ...). */
typedef struct vqae_tensor {
    const char* name;
    const float* data;    /* host pointer */
    int64_t numel;
} vqae_tensor;

typedef struct vqae_handle vqae_handle;

int vqae_create(const vqae_config* cfg, const vqae_tensor* tensors, int n_tensors, vqae_handle** out);
void vqae_destroy(vqae_handle* h);
/* Pre-size the internal workspace for `max_batch` patches of in_h x in_w (optional). */
int vqae_reserve(vqae_handle* h, int max_batch, int in_h, int in_w);
/* Replace the codebook (e.g. after calibration / EMA updates): embed_host [K][D] fp32. */
int vqae_set_codebook(vqae_handle* h, const float* embed_host);

/* Encoder.forward: x [B,3,H,W] (layout per `layout`) -> idx [B][h][w] (idx_dtype), optional
 * q_dev [B][C][h][w] (fp32, `layout`), optional loss_dev (one fp32).  h = H / 2^n_down. */
int vqae_encode(vqae_handle* h, const float* x_dev, int batch, int in_h, int in_w, int layout, void* idx_dev,
                int idx_dtype, float* q_dev, float* loss_dev, void* stream);
/* Same, from raw uint8 NHWC patches normalised on device. */
int vqae_encode_u8(vqae_handle* h, const uint8_t* x_u8_dev, int batch, int in_h, int in_w, void* idx_dev,
                   int idx_dtype, float* q_dev, int q_layout, float* loss_dev, void* stream);
/* Pre-VQ activations z [B][h][w][C] NHWC (for codebook calibration, vq.py:76-94 `_init_ema`);
 * with projection, the projected [B][h][w][D] tensor. */
int vqae_encode_features(vqae_handle* h, const float* x_dev, int batch, int in_h, int in_w, int layout,
                         float* z_dev, void* stream);
/* Decoder.forward: q [B][C][h][w] -> out [B,3,H,W]  (q_h, q_w = latent grid size). */
int vqae_decode(vqae_handle* h, const float* q_dev, int batch, int q_h, int q_w, int layout, float* out_dev,
                void* stream);
/* Decode from code indices: embed_code (+ proj_out) then Decoder.forward. */
int vqae_decode_indices(vqae_handle* h, const void* idx_dev, int idx_dtype, int batch, int q_h, int q_w, int layout,
                        float* out_dev, void* stream);
/* The same, down to displayable pixels: embed_code (vq.py:44-45; + proj_out when the model projects) -> Decoder.forward
 * (vq_ae/model.py:274-291) with the out-stem writing into the handle's own NHWC fp32 workspace -> vqae_pixels_u8 with the
 * constants of the handle's ingest normalisation (mean255 = MEAN * 255, std255 = STD * 255, formed in fp32): no fp32 tensor
 * of the caller's and no layout transpose.  idx [B][q_h][q_w] of idx_dtype; tile size H x W = q_h, q_w * 2^n_down.
 *   rc_dev == NULL: canvas_dev is a dense uint8 [B][H][W][3] batch and canvas_h = canvas_w = 0;
 *   otherwise tile t lands in canvas_dev [canvas_h][canvas_w][3] at pixel (rc[t].r * H, rc[t].c * W), i.e. rc are the patch
 *   positions of get_encodings (scripts/extract_embeddings/extract_embeddings.py:77-84) relative to the canvas.
 * Preconditions and errors as vqae_decode_indices; canvas sizes with a dense destination, or a canvas smaller than one
 * tile -> VQAE_ERR_INVALID.  batch == 0 -> VQAE_OK. */
int vqae_decode_indices_u8(vqae_handle* h, const void* idx_dev, int idx_dtype, int batch, int q_h, int q_w,
                           const int32_t* rc_dev, uint8_t* canvas_dev, int canvas_h, int canvas_w, void* stream);
/* Overview levels of the same reconstruction: ONE decoder pass into the handle's NHWC fp32 workspace, then one
 * vqae_pixels_u8_level launch per requested level on that tensor (the decoder is tens of milliseconds, a pixel pass tens of
 * microseconds).  levels, canvases, canvas_h, canvas_w: host arrays of n_levels entries, 1 <= n_levels <= 7, the levels
 * distinct and each 0 .. VQAE_MAX_PIXEL_LEVEL with 2^level dividing the tile size H x W = q_h, q_w * 2^n_down; canvases[i] is the
 * device destination of levels[i]:
 *   rc_dev == NULL: a dense uint8 [B][H/f][W/f][3] batch, canvas_h[i] = canvas_w[i] = 0;
 *   otherwise a canvas [canvas_h[i]][canvas_w[i]][3] in level pixels, tile t at pixel (rc[t].r * H/f, rc[t].c * W/f).
 * Every level is validated before anything is launched: on an error no destination is written.
 * Preconditions and errors as vqae_decode_indices_u8 and vqae_pixels_u8_level; n_levels outside 1 .. 7, a repeated level or a
 * null array / canvas -> VQAE_ERR_INVALID.  batch == 0 -> VQAE_OK. */
int vqae_decode_indices_u8_levels(vqae_handle* h, const void* idx_dev, int idx_dtype, int batch, int q_h, int q_w,
                                  const int32_t* rc_dev, int n_levels, const int* levels, uint8_t* const* canvases,
                                  const int* canvas_h, const int* canvas_w, void* stream);
/* VQAE.forward: out [B,3,H,W], idx (optional), loss (optional). */
int vqae_forward(vqae_handle* h, const float* x_dev, int batch, int in_h, int in_w, int layout, float* out_dev,
                 void* idx_dev, int idx_dtype, float* loss_dev, void* stream);

/* Sub-module calls.  The reference lets a caller run any part of the block stacks on its own
 * (`model.encoder.down_layers[0].layers[l].layers[b](x)`, `model.encoder.pre_enc_layers[0][i:j](x)` --
 * nn.ModuleList / nn.Sequential of PreActFixupResBlock, vq_ae/model.py:160-176,249-264, conv_block.py:196-216).
 * vqae_run_blocks runs residual blocks [first, first + count) of the encoder block list (side 0: the DownBlock
 * levels in order, then pre_enc; model.py:199-208) or of the decoder list (side 1: post_enc, then the UpBlock
 * levels; model.py:278-289) on x_dev [B][in_h][in_w][cin of block `first`] (NHWC fp32) through exactly the kernels
 * the handle-level calls dispatch (including the cross-block fusions when count > 1), and writes
 * y_dev [B][*out_h][*out_w][cout of the last block].  The per-block parity tests are built on it. */
int vqae_block_count(const vqae_handle* h, int side);
int vqae_run_blocks(vqae_handle* h, int side, int first, int count, const float* x_dev, int batch, int in_h, int in_w,
                    float* y_dev, int* out_h, int* out_w, void* stream);
/* Which kernel family vqae_run_blocks (and every handle-level call) runs block `index` of that list on, for a
 * [batch][in_h][in_w] input of the block: the name of the dispatch's route -- "same16_16", "trunk16", "wino43_split",
 * "wino43", "wino", "tail", "same8_16", "fixup_fused", "same", "down16", "down_fused", "down", "up_conv_first_tail",
 * "up_conv_first", "up16", "up" ("mbconv" for an MBConv handle) -- as a static string.  chained != 0: the next block of
 * the list runs in the same call (only then can a route depend on it).  Read-only: launches and allocates nothing.
 * NULL handle, side not 0 / 1, index outside the list, batch / in_h / in_w < 1 -> NULL, vqae_last_error() says which. */
const char* vqae_block_route(const vqae_handle* h, int side, int index, int chained, int batch, int in_h, int in_w);

/* Introspection for benchmarks: algorithmic FLOPs (2*MACs) of the conv stacks per patch. */
double vqae_flops_per_patch(const vqae_handle* h, int in_h, int in_w, int encoder, int decoder);

/* ---------------------------------------------------------------------------------------------
 * 4. Reconstruction metrics -- replaces the validation scoring of the reference: VQAE.shared_step
 *    (vq_ae/model.py:82-93: `val_recon_loss` = loss_f(out, x) with loss_f/huber.yaml, and the torchmetrics
 *    collection of conf/model/metrics/{mse,psnr,ssim}.yaml, torchmetrics 0.8.2), which
 *    scripts/extract_validation_metrics/eval.py:13-45 runs over a checkpoint with batch size 1.
 *    Per image i (p, t = prediction, target [C][H][W], N = C*H*W, d = p - t):
 *      mse   = sum d^2 / N;   huber = sum h(d) / N,  h(d) = 0.5 d^2 if |d| < delta else delta (|d| - 0.5 delta);
 *      psnr  = 10 log10((max t - min t)^2 / mse)       (PeakSignalNoiseRatio, data_range=None; mse = 0 -> +inf);
 *      ssim  = mean over C x (H-10) x (W-10) valid window centres of the Gaussian(11, 1.5) SSIM map with
 *              r = max(max p - min p, max t - min t), c1 = (0.01 r)^2, c2 = (0.03 r)^2, un-centred moments
 *              (StructuralSimilarityIndexMeasure: reflect pad + conv + crop keeps only the valid centres);
 *      and the min / max of p and of t.
 *    Evaluated in fp32 with fp64 sums; per-workgroup partials are reduced in a fixed order (no atomics), and the
 *    partition depends on (channels, h, w) only: an image's results are bit-identical run to run and in any batch.
 * ------------------------------------------------------------------------------------------- */
enum { VQAE_METRIC_MSE = 0, VQAE_METRIC_HUBER = 1, VQAE_METRIC_PSNR = 2, VQAE_METRIC_SSIM = 3, VQAE_METRIC_PRED_MIN = 4,
       VQAE_METRIC_PRED_MAX = 5, VQAE_METRIC_TARGET_MIN = 6, VQAE_METRIC_TARGET_MAX = 7, VQAE_METRICS_K = 8 };
/* Bytes of scratch vqae_recon_metrics_f32 needs (0 for an empty batch or an image under 11 x 11). */
size_t vqae_recon_metrics_workspace_bytes(int batch, int channels, int h, int w);
/*   pred_dev      [B][C][H][W] (layout VQAE_LAYOUT_NCHW) or [B][H][W][C] (VQAE_LAYOUT_NHWC), fp32
 *   target_dev    fp32 in the same layout, or NULL;
 *   target_u8_dev uint8 NHWC [B][H][W][3] normalised on the fly, (u - mean255[c]) * inv_std255[c] as
 *                 vqae_conv3x3_direct_f32 does (host arrays of 3; NULL -> 0 / 1), or NULL -- exactly one of the two;
 *   huber_delta   HuberLoss delta (loss_f/huber.yaml: 1.0);
 *   out_dev       double [B][VQAE_METRICS_K], indexed by VQAE_METRIC_*;
 *   workspace_dev vqae_recon_metrics_workspace_bytes(B, C, H, W) bytes.
 * Errors: null pointers / both or neither target / bad layout / delta <= 0 -> VQAE_ERR_INVALID; H < 11 or W < 11 ->
 * VQAE_ERR_VALUE; a uint8 target with C != 3, B > 65535 -> VQAE_ERR_UNSUPPORTED.  Both targets constant (r = 0):
 * c1 = c2 = 0 and SSIM is 0/0, as in torchmetrics. */
int vqae_recon_metrics_f32(const float* pred_dev, const float* target_dev, const uint8_t* target_u8_dev,
                           const float* mean255, const float* inv_std255, int batch, int channels, int h, int w,
                           int layout, float huber_delta, double* out_dev, void* workspace_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 5. Measurement hook (bench.py `roofline`): time every launch of one kernel class with HIP events
 *    recorded on the launch stream.  kernel_class: 1 = trunk 3x3 circular conv (MFMA, cin >= 128; incl. its fused conv3/conv1 tail),
 *    2 = trunk 1x1 conv, 3 = VQ tier-1 argmin.  Not thread-safe; off by default.
 * ------------------------------------------------------------------------------------------- */
int vqae_prof_begin(int kernel_class, int max_launches);
/* total_work: algorithmic flops of the timed launches (class 1: 2*M*N*K of the 3x3 conv plus, when the
 * launch also ran the fused conv3 / next-conv1 tail, their 2*M*128*128 each; class 3: 3*N*K*D VALU ops). */
int vqae_prof_end(double* total_ms, int* n_launches, double* total_work);

/* ---------------------------------------------------------------------------------------------
 * 6. Slide classifier on stored code grids -- replaces CNNClassifier.forward (validation_nn/model.py:141-142,
 *    `self.layers(data)`) for the layer stack conf/model/cnn_classifier.yaml composes:
 *      nn.Embedding(K, E) -> FlattenAfterEmbedding (validation_nn/layers/misc.py:9-22: [B,1,H,W,E] -> [B,E,H,W])
 *      -> Conv2d(E, C, 3, padding 1, zeros, bias) -> ELU(1) -> Conv2d(C, C, 3) -> ELU(1) -> Conv2d(C, n_out, 3)
 *    and, for n_out == 1, the scoring Camelyon16BCELoss (utils/train_helpers.py:101-138) and the precision / recall
 *    collection of cnn_classifier.yaml apply to its output.  One fused launch per call: HBM sees the codes once (plus
 *    halo re-reads) and each requested output once; the 8- or 16-channel activations never leave the CU.
 *    Every conv pads ITS OWN input with zeros at the grid border (activations outside the grid are 0, not
 *    ELU(bias + ...)); a code outside 0 .. K-1 contributes a zero embedding vector and reads nothing outside the table
 *    (the Python layer raises IndexError for it, as nn.Embedding does).  fp32 fmaf sums; ELU's negative side to <= 3 ulp
 *    of expm1.
 * ------------------------------------------------------------------------------------------- */
/* Columns of a stats row.  Over the codes of one slide with mask != 0 (labels 0 background, 1 tissue, 2 cancer: the contract
 * Camelyon16BCELoss checks, train_helpers.py:115-119), target t = mask - 1 (train_helpers.py:121-127), prediction = logit > 0:
 * the four confusion counts and their total (exact integers held in doubles), and
 *   loss_sum = sum of pos_weight * t * softplus(-x) + (1 - t) * softplus(x)
 * = Camelyon16BCELoss(reduction='sum', pos_weight, label_smoothing=0) (train_helpers.py:129-138), softplus in fp32, the
 * sum in fp64. */
enum { VQAE_CLS_TP = 0, VQAE_CLS_FP = 1, VQAE_CLS_FN = 2, VQAE_CLS_TN = 3, VQAE_CLS_N_VALID = 4, VQAE_CLS_LOSS_SUM = 5,
       VQAE_CLS_STATS_K = 6 };

typedef struct vqae_classifier vqae_classifier;

/* Builds the classifier from named fp32 host tensors in the reference's state-dict naming and PyTorch shapes
 * (cnn_classifier.yaml's layer names under `layers.`): layers.embedding.weight [K][E], layers.in_conv.weight [C][E][3][3],
 * layers.in_conv.bias [C], layers.hidden_conv1.weight [C][C][3][3], layers.hidden_conv1.bias [C],
 * layers.out_conv.weight [n_out][C][3][3], layers.out_conv.bias [n_out]; other tensors are ignored.  The weights are
 * copied; nothing touches the device before the first vqae_classifier_forward.
 * Errors: embedding_dim outside 1 .. 8, hidden not 8 or 16, n_out outside 1 .. 4, num_embeddings outside 1 .. 65536 ->
 * VQAE_ERR_UNSUPPORTED; a missing tensor -> VQAE_ERR_NOT_FOUND; a tensor of another size, null pointers -> VQAE_ERR_INVALID. */
int vqae_classifier_create(int num_embeddings, int embedding_dim, int hidden, int n_out, const vqae_tensor* tensors,
                           int n_tensors, vqae_classifier** out);
void vqae_classifier_destroy(vqae_classifier* c);
/* Bytes of scratch a call with stats needs for `batch` grids of h x w codes (0 for an empty batch or a bad shape). */
size_t vqae_classifier_workspace_bytes(const vqae_classifier* c, int batch, int h, int w);
/* CNNClassifier.forward (validation_nn/model.py:141-142) on codes_dev [B][h][w] of idx_dtype (VQAE_IDX_*, as stored), any
 * h, w >= 1.  Each output is optional, at least one is required:
 *   logits_dev   fp32 [B][n_out][h][w], the reference's NCHW output;
 *   heat_u8_dev  uint8 [B][h][w] = rintf(255 * sigmoid(logit)), n_out == 1 only;
 *   stats_dev    double [B][VQAE_CLS_STATS_K] (VQAE_CLS_*) over mask_dev uint8 [B][h][w] with `pos_weight`, n_out == 1
 *                only; needs workspace_dev of vqae_classifier_workspace_bytes(c, B, h, w) bytes.  Per-workgroup partials
 *                are reduced in a fixed order (no atomics) and the partition depends on (h, w) only: a slide's row is
 *                bit-identical run to run and at any batch position.
 * Errors, all before any HIP call: null c / codes, no output at all, stats without a mask or without the workspace, heat or
 * stats with n_out != 1, a bad idx_dtype, h < 1 or w < 1, batch < 0, a negative or non-finite pos_weight with stats ->
 * VQAE_ERR_INVALID; batch > 65535 -> VQAE_ERR_UNSUPPORTED; batch == 0 -> VQAE_OK. */
int vqae_classifier_forward(vqae_classifier* c, const void* codes_dev, int idx_dtype, int batch, int h, int w,
                            float* logits_dev, uint8_t* heat_u8_dev, const uint8_t* mask_dev, float pos_weight,
                            double* stats_dev, void* workspace_dev, void* stream);

/* ---- Training: replaces CNNClassifier.step (validation_nn/model.py:131-139: forward, then the loss Lightning
 * differentiates) with Camelyon16BCELoss (utils/train_helpers.py:101-138) as loss_f, and the backward() autograd runs over
 * both, for n_out == 1.  No activation tensor is stored: the backward recomputes the tiles from the codes. ---- */
/* Replaces the weights of an existing classifier: the same names, shapes and checks as vqae_classifier_create (dimensions are
 * those the handle was created with).  The host copy changes at once; the device copy is refreshed by the next call that
 * uses the handle, on that call's stream.  No HIP call is made here, so an optimiser step does not rebuild the handle.
 * The handle keeps the weights twice, a host image and a device image, and either can be the newer one: after this call (and
 * after create) it is the host image, which the next forward / loss_grad / optimiser step uploads first; after a
 * vqae_classifier_optim step it is the device image, which no later call overwrites with the older host copy.  An update
 * after such a step wins: the stepped weights are dropped, the optimiser's moments and step count stay.
 * Errors: null pointers, a tensor of another size -> VQAE_ERR_INVALID; a missing tensor -> VQAE_ERR_NOT_FOUND. */
int vqae_classifier_update(vqae_classifier* c, const vqae_tensor* tensors, int n_tensors);
/* Length of the packed gradient vector of vqae_classifier_loss_grad (0 for a null handle): the seven tensors, dense, in
 * PyTorch's shapes and parameter order --
 *   embedding.weight [K][E], in_conv.weight [C][E][3][3], in_conv.bias [C], hidden_conv1.weight [C][C][3][3],
 *   hidden_conv1.bias [C], out_conv.weight [n_out][C][3][3], out_conv.bias [n_out]. */
size_t vqae_classifier_grad_floats(const vqae_classifier* c);
/* Bytes of scratch vqae_classifier_loss_grad needs for `batch` grids of h x w codes: the forward's stats partials, dL/dlogit
 * (4 B per code), the fixed-point table gradient (8 B per table entry) and at most 512 fp64 rows of weight-gradient
 * partials.  0 for an empty batch, a bad shape or n_out != 1. */
size_t vqae_classifier_train_workspace_bytes(const vqae_classifier* c, int batch, int h, int w);
/* Loss and gradients for codes_dev [B][h][w] (idx_dtype as stored) and mask_dev uint8 [B][h][w] (0 background, 1 tissue,
 * 2 cancer), over the codes with mask != 0:
 *   loss_sum = sum of pos_weight * t * softplus(-x) + (1 - t) * softplus(x),   t = mask - 1 (train_helpers.py:121-127), or,
 *   with target_dev (optional fp32 [B][h][w], read only where mask != 0), the soft target in [0, 1] stored there: the
 *   caller's label smoothing (train_helpers.py:133-135; the noise is the caller's);
 *   dL/dlogit = sigmoid(x) * (1 - t + pos_weight * t) - pos_weight * t on those codes, 0 elsewhere.
 * reduction 0 = 'sum', 1 = 'mean' (loss and gradients times 1 / n_valid of the WHOLE batch, applied once, in fp64; with no
 * valid code the loss is nan and the gradients are 0).  Outputs:
 *   grads_dev  double [vqae_classifier_grad_floats(c)], the gradients of the loss summed over the batch;
 *   stats_dev  double [B][VQAE_CLS_STATS_K], exactly vqae_classifier_forward's rows (counts against the hard labels);
 *   loss_dev   double [1].
 * Border rule: activations and embeddings outside the grid are the constant 0 and pass no gradient; a code outside 0 .. K-1
 * is a zero vector and its (non-existent) table row receives nothing.  Sums are fixed-order fp64 over fp32 products; the
 * table gradient is accumulated in 64-bit fixed point (2^-30 resolution, |entry| < 8.6e9) with integer atomics.  All outputs
 * are bit-identical between two calls on the same inputs.
 * Errors, all before any HIP call: null c / codes / mask / grads / stats / loss / workspace, a bad idx_dtype, h < 1 or
 * w < 1, batch < 0, a negative or non-finite pos_weight, a reduction other than 0 or 1 -> VQAE_ERR_INVALID; n_out != 1,
 * batch > 65535 -> VQAE_ERR_UNSUPPORTED.  batch == 0 -> VQAE_OK with zero gradients and a zero loss. */
int vqae_classifier_loss_grad(vqae_classifier* c, const void* codes_dev, int idx_dtype, int batch, int h, int w,
                              const uint8_t* mask_dev, const float* target_dev, float pos_weight, int reduction,
                              double* grads_dev, double* stats_dev, double* loss_dev, void* workspace_dev, void* stream);

/* ---- Optimiser: replaces the optimizer.step() Lightning runs after CNNClassifier.step's backward with the three optimisers
 * of conf/model/optim/ -- torch.optim.Adam / AdamW (adam.yaml, adamw.yaml), vq_ae/optim/lamb.py (lamb.yaml) and, around
 * either, vq_ae/optim/sam.py (sam.yaml; CNNClassifier.sam_step_and_update, validation_nn/model.py:115-129) -- on the handle's
 * own device weights.  The step reads the packed gradient vqae_classifier_loss_grad left in HBM and rewrites the packed
 * weight image the forward and backward kernels read: no tensor crosses PCIe and nothing blocks between two steps. ---- */
enum { VQAE_OPTIM_ADAM = 0, VQAE_OPTIM_ADAMW = 1, VQAE_OPTIM_LAMB = 2 };
typedef struct vqae_classifier_optim_config {
    int kind;                 /* VQAE_OPTIM_*; amsgrad / maximize are not provided */
    double lr, beta1, beta2, eps, weight_decay;
    double sam_rho;           /* < 0: no SAM; otherwise sam.py's rho */
    int sam_adaptive;         /* sam.py's adaptive */
} vqae_classifier_optim_config;
typedef struct vqae_classifier_optim vqae_classifier_optim;

/* An optimiser over the seven tensors of `c` (which must outlive it), with exp_avg = exp_avg_sq = 0 and step = 0
 * (lamb.py:69-76; torch.optim.Adam's lazy state).  Uploads c's weights to the current device, where the state is allocated;
 * every later call must run on that device.
 * Errors, before any HIP call: null pointers, an unknown kind, lr < 0, eps < 0, a beta outside [0, 1), weight_decay < 0 (the
 * ValueErrors of lamb.py:34-41 and torch.optim.Adam), a nan sam_rho -> VQAE_ERR_INVALID; n_out != 1 -> VQAE_ERR_UNSUPPORTED. */
int vqae_classifier_optim_create(vqae_classifier* c, const vqae_classifier_optim_config* cfg, vqae_classifier_optim** out);
void vqae_classifier_optim_destroy(vqae_classifier_optim* opt);
/* New hyper-parameters from the next step on (param_groups[0]['lr'] = ... of an lr schedule).  The same checks as create; the
 * kind, and whether SAM is on, cannot change -> VQAE_ERR_INVALID.  No HIP call. */
int vqae_classifier_optim_set(vqae_classifier_optim* opt, const vqae_classifier_optim_config* cfg);
/* One optimizer.step() with grads_dev = double [vqae_classifier_grad_floats(c)], exactly vqae_classifier_loss_grad's output,
 * stream-ordered behind it.  Each gradient is rounded to fp32 once (as `.grad` of an fp32 parameter holds it); moments and
 * weights are fp32; bias corrections and scalar factors are formed in double on the host; step counts from 1.
 *   AdamW (torch.optim.adam._single_tensor_adam): p *= 1 - lr * wd (wd != 0);  m += (g - m) * (1 - b1);
 *          v = b2 * v + (1 - b2) * g * g;  p += (-lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
 *   Adam:  the same with g += wd * p in place of the decay
 *   LAMB (lamb.py:78-114): m = b1 * m + (1 - b1) * g;  v likewise;  u = (m / bc1) / (sqrt(v / bc2) + eps) + wd * p;
 *          per tensor r = ||p|| / ||u|| where both are > 0, else 1;  p -= lr * r * u.  The embedding table is one tensor.
 * After vqae_classifier_optim_sam_first this is SAM.second_step (sam.py:49-60): the weights saved there come back first.
 * Norms are fixed-order fp64 sums of fp32 squares (no atomics): weights and moments are bit-identical between two runs on the
 * same inputs.  Up to 4096 parameters the step is one launch of one workgroup, beyond that two launches (one for Adam /
 * AdamW at any size).  No host synchronisation, no copy and no allocation; a pending vqae_classifier_update is uploaded
 * first (that one upload synchronises).  A non-finite gradient is not an error: it propagates as in torch.
 * Errors: null pointers -> VQAE_ERR_INVALID, before any HIP call; another device than create's -> VQAE_ERR_INVALID. */
int vqae_classifier_optim_step(vqae_classifier_optim* opt, const double* grads_dev, void* stream);
/* SAM.first_step (sam.py:31-46) with _grad_norm (sam.py:96-111): n = sqrt(sum over all seven tensors of (a * g)^2), a = |p|
 * if sam_adaptive else 1; the weights are saved and p += (p * p if sam_adaptive else 1) * g * rho / (n + 1e-12).  The caller
 * then evaluates vqae_classifier_loss_grad at the climbed weights and hands those gradients to vqae_classifier_optim_step.
 * Errors, before any HIP call: null pointers, an optimiser created with sam_rho < 0, a second first step without a step in
 * between -> VQAE_ERR_INVALID. */
int vqae_classifier_optim_sam_first(vqae_classifier_optim* opt, const double* grads_dev, void* stream);
/* The current weights as the seven PyTorch-shaped fp32 host tensors, in parameter order (the order and shapes of
 * vqae_classifier_grad_floats): the inverse of create's repacking.  Where an optimiser stepped the device image it is
 * fetched on `stream` (one synchronising copy) and becomes the host image too; otherwise no HIP call is made.
 * Errors: null pointers -> VQAE_ERR_INVALID. */
int vqae_classifier_download(vqae_classifier* c, float* const tensors[7], void* stream);
/* The packed weight image as the kernels read it, for checks of the layout: vqae_classifier_image_floats(c) floats (0 for a
 * null handle) -- table [K][E], in_conv [E][9][C], its bias, hidden_conv1 [C][9][C], its bias, out_conv [C][9][n_out], its
 * bias, each block padded with zeros to a multiple of 16 floats.  The device copy where one exists (one synchronising copy on
 * `stream`), the host copy otherwise; nothing else changes.  Errors: null pointers -> VQAE_ERR_INVALID. */
size_t vqae_classifier_image_floats(const vqae_classifier* c);
int vqae_classifier_image(vqae_classifier* c, float* image_host, void* stream);
/* state[p]['exp_avg'], ['exp_avg_sq'] and ['step'] of torch.optim's state_dict: two host arrays of
 * vqae_classifier_grad_floats(c) floats, the seven tensors dense in parameter order, and the one step count.  Both
 * synchronise `stream`.  Import with a SAM first step pending, step < 0, null pointers -> VQAE_ERR_INVALID. */
int vqae_classifier_optim_export(vqae_classifier_optim* opt, float* exp_avg, float* exp_avg_sq, int64_t* step, void* stream);
int vqae_classifier_optim_import(vqae_classifier_optim* opt, const float* exp_avg, const float* exp_avg_sq, int64_t step,
                                 void* stream);

/* ---- Multi-class (n_out = 2 .. 4): replaces torch.nn.CrossEntropyLoss(weight, label_smoothing, reduction) as loss_f of
 * CNNClassifier.step (validation_nn/model.py:131-139; conf/model/loss_f/cross_entropy.yaml, with the weights and smoothing of
 * conf/model/optional_overrides/loss_f/cross_entropy_camelyon16_embeddings.yaml), over logits [B][n_out][h][w] and the stored
 * mask bytes as class indices [B][h][w] (datamodules/camelyon16.py:259 casts them for the loss; out_conv's channels are
 * [background, tissue, cancer], cnn_classifier.yaml).  There is no ignore_index.  Per position with label y, p = softmax(x):
 *   nll = w[y] * -log p_y,   smooth = sum_c w[c] * -log p_c,
 *   loss_sum = (1 - eps) * sum nll + (eps / n_out) * sum smooth;   'mean' divides by sum w[y] over the whole batch;
 *   dL/dx_k = (1 - eps) * w[y] * (p_k - [k == y]) + (eps / n_out) * (W * p_k - w_k),   W = sum_c w_c.
 * The log-softmax is taken in fp32 on the max-subtracted logits, the sums in fp64.  A position whose label is >= n_out is
 * counted aside and contributes to nothing else (zero gradient).  The n_out == 1 entry points above are unchanged and keep
 * refusing n_out != 1; these refuse n_out == 1. ---- */
/* Columns of a cross-entropy stats row: 0 .. 15 the confusion counts at [label * 4 + prediction] over the positions with
 * label < n_out (exact integers held in doubles, unused cells 0; prediction = argmax, lowest index on ties), then
 * sum w[y], sum nll, sum smooth, and the number of positions with label >= n_out. */
enum { VQAE_CE_CONFUSION = 0, VQAE_CE_WEIGHT_SUM = 16, VQAE_CE_NLL_SUM = 17, VQAE_CE_SMOOTH_SUM = 18, VQAE_CE_N_BAD = 19,
       VQAE_CE_STATS_K = 20 };
/* Bytes of scratch vqae_classifier_forward_ce needs with stats (0 for an empty batch, a bad shape or n_out == 1). */
size_t vqae_classifier_ce_workspace_bytes(const vqae_classifier* c, int batch, int h, int w);
/* CNNClassifier.forward (validation_nn/model.py:141-142) and the scores of CNNClassifier.step with the cross-entropy loss on
 * codes_dev [B][h][w], one launch.  Each output is optional, at least one is required:
 *   logits_dev    fp32 [B][n_out][h][w];
 *   prob_u8_dev   uint8 [B][n_out][h][w] = rintf(255 * softmax(logits));
 *   class_u8_dev  uint8 [B][h][w] = argmax over the classes, the lowest index on ties (torch.argmax);
 *   stats_dev     double [B][VQAE_CE_STATS_K] over labels_dev uint8 [B][h][w] with `weight` (HOST float [n_out], null = ones)
 *                 and label_smoothing; needs workspace_dev of vqae_classifier_ce_workspace_bytes bytes.  Reduced as
 *                 vqae_classifier_forward's rows are: bit-identical run to run and at any batch position.
 * The raw counts are the loss's; the `out[:, 0][labels == 0] = inf` of validation_nn/model.py:103 (row 0 of the confusion
 * matrix collapses into column 0) is the caller's, from these counts.
 * Errors, all before any HIP call: null c / codes, no output at all, stats without labels or without the workspace, a bad
 * idx_dtype, h < 1 or w < 1, batch < 0, a negative or non-finite weight, label_smoothing outside [0, 1] ->
 * VQAE_ERR_INVALID; n_out == 1, batch > 65535 -> VQAE_ERR_UNSUPPORTED; batch == 0 -> VQAE_OK. */
int vqae_classifier_forward_ce(vqae_classifier* c, const void* codes_dev, int idx_dtype, int batch, int h, int w,
                               float* logits_dev, uint8_t* prob_u8_dev, uint8_t* class_u8_dev, const uint8_t* labels_dev,
                               const float* weight, float label_smoothing, double* stats_dev, void* workspace_dev, void* stream);
/* Bytes of scratch vqae_classifier_loss_grad_ce needs: as vqae_classifier_train_workspace_bytes, with dL/dlogit at
 * 4 * n_out bytes per code.  0 for an empty batch, a bad shape or n_out == 1. */
size_t vqae_classifier_ce_train_workspace_bytes(const vqae_classifier* c, int batch, int h, int w);
/* Loss and gradients of the cross-entropy step (validation_nn/model.py:131-139 with loss_f = nn.CrossEntropyLoss and the
 * backward() autograd runs over both): the forward launch above storing dL/dlogit, then vqae_classifier_loss_grad's backward
 * with n_out planes of it.  reduction 0 = 'sum', 1 = 'mean' (loss and gradients times 1 / sum w[y] of the whole batch, applied
 * once, in fp64; a zero weight sum gives a nan loss and zero gradients).  Outputs as vqae_classifier_loss_grad's: grads_dev
 * double [vqae_classifier_grad_floats(c)] packed as described there, stats_dev double [B][VQAE_CE_STATS_K] exactly
 * vqae_classifier_forward_ce's rows, loss_dev double [1].  Border rule, sums and determinism as there.
 * Errors, all before any HIP call: null c / codes / labels / grads / stats / loss / workspace, a bad idx_dtype, h < 1 or
 * w < 1, batch < 0, a negative or non-finite weight, label_smoothing outside [0, 1], a reduction other than 0 or 1 ->
 * VQAE_ERR_INVALID; n_out == 1, batch > 65535 -> VQAE_ERR_UNSUPPORTED.  batch == 0 -> VQAE_OK with zero gradients and loss. */
int vqae_classifier_loss_grad_ce(vqae_classifier* c, const void* codes_dev, int idx_dtype, int batch, int h, int w,
                                 const uint8_t* labels_dev, const float* weight, float label_smoothing, int reduction,
                                 double* grads_dev, double* stats_dev, double* loss_dev, void* workspace_dev, void* stream);
/* vqae_classifier_optim_create for a classifier with n_out = 2 .. 4 (the optimizer.step() after the cross-entropy step): the
 * same optimiser, state and checks; every other vqae_classifier_optim_* call takes its handle.  out_conv's weight and bias
 * are tensors of their own for LAMB's norms at any n_out.  n_out == 1 -> VQAE_ERR_UNSUPPORTED. */
int vqae_classifier_optim_create_ce(vqae_classifier* c, const vqae_classifier_optim_config* cfg, vqae_classifier_optim** out);

/* ---- Optimiser over any list of tensors: replaces the optimizer.step() of the auto-encoder's own training
 * (conf/model/optim/: torch.optim.Adam / AdamW, vq_ae/optim/lamb.py, and vq_ae/optim/sam.py around either) for n fp32 tensors
 * given as device pointers -- the ~1 600 parameters of an Encoder / Decoder, most of them Fixup scalars.  The arithmetic per
 * element is the classifier optimiser's above (the same code); norms are formed on the device, nothing is read back and
 * nothing in a step synchronises the host.  vqae_classifier_optim_config holds the hyper-parameters of one param group. ---- */
/* VQAE_OPTIM_CHUNK: a tensor of more than VQAE_OPTIM_SMALL elements is stepped in pieces of this many, one workgroup and one
 * row of fp64 partial sums each; a tensor of at most VQAE_OPTIM_SMALL elements is taken whole by one wave, four per workgroup. */
enum { VQAE_OPTIM_CHUNK = 4096, VQAE_OPTIM_SMALL = 64 };
typedef struct vqae_optim vqae_optim;
/* An optimiser over n_tensors tensors of numel[i] elements, tensor i in param group group_of[i] of n_groups, with exp_avg =
 * exp_avg_sq = 0 and step = 0 for every tensor (lamb.py:69-76; torch.optim.Adam's lazy state).  The state (exp_avg,
 * exp_avg_sq, SAM's old_p: 12 bytes per element, every tensor on a 16-byte boundary), the sums and a ring of table slots are
 * allocated here, on the current device, where every later call must run; a step allocates nothing.
 * Errors, all before any HIP call: null pointers, n_tensors < 1, n_groups < 1, a numel < 1, a group index outside
 * 0 .. n_groups - 1, per group the checks of vqae_classifier_optim_create (the ValueErrors of lamb.py:34-41 and
 * torch.optim.Adam, a nan sam_rho), groups that differ in kind or in whether SAM is on (sam_rho >= 0) -> VQAE_ERR_INVALID;
 * more than 2^31 - 1 elements in all -> VQAE_ERR_UNSUPPORTED. */
int vqae_optim_create(int n_tensors, const int64_t* numel, const int* group_of, int n_groups,
                      const vqae_classifier_optim_config* groups, vqae_optim** out);
void vqae_optim_destroy(vqae_optim* opt);
/* New hyper-parameters of all n_groups groups from the next call on (an lr schedule's writes to param_groups).  The checks of
 * create; the kind, and whether SAM is on, cannot change -> VQAE_ERR_INVALID.  No HIP call. */
int vqae_optim_set(vqae_optim* opt, const vqae_classifier_optim_config* groups);
/* One optimizer.step().  params_dev / grads_dev are HOST arrays of n_tensors device pointers, each to numel[i] fp32 values
 * that are 4-byte aligned (16-byte accesses are used where both pointers of a tensor allow); they may differ from call to
 * call.  A tensor whose gradient pointer is null is skipped as lamb.py:81-82 skips `p.grad is None`: it does not move and
 * its step count, which is therefore per tensor, does not advance.  Formulas, rounding and bias corrections are those of
 * vqae_classifier_optim_step, with each tensor's own step count and its group's hyper-parameters.  After
 * vqae_optim_sam_first this is SAM.second_step (sam.py:49-60): the tensors climbed there are read from their saved values.
 *   Adam / AdamW  one launch.
 *   LAMB          three: moments and partial norms (tensors of <= VQAE_OPTIM_SMALL elements are finished there), each
 *                 larger tensor's rows added in index order, the update with u recomputed from the stored moments.
 * The pointers and scalars travel in a table written to page-locked memory and copied on `stream` into one of 8 device slots;
 * an event behind the step's last kernel guards the slot, and the host waits for it only once it is 8 tables ahead.  Sums
 * are fp64 of fp32 squares in an order fixed by the element counts: results are bit-identical run to run.  A non-finite
 * gradient is not an error: it propagates as in torch.
 * Errors, before any HIP call: a null handle or array, a null parameter pointer -> VQAE_ERR_INVALID; then another current
 * device than create's -> VQAE_ERR_INVALID. */
int vqae_optim_step(vqae_optim* opt, float* const* params_dev, const float* const* grads_dev, void* stream);
/* SAM.first_step (sam.py:31-46) with _grad_norm (sam.py:96-111) over the tensors that have a gradient: n = sqrt(sum of
 * (a * g)^2), a = |p| if sam_adaptive else 1; each is saved and p += (p * p if sam_adaptive else 1) * g * rho / (n + 1e-12),
 * rho and sam_adaptive being the tensor's group's.  Three launches: partial sums, their total in one workgroup, the climb.
 * Errors, before any HIP call: as vqae_optim_step, an optimiser created without SAM, a second first step without a step in
 * between -> VQAE_ERR_INVALID. */
int vqae_optim_sam_first(vqae_optim* opt, float* const* params_dev, const float* const* grads_dev, void* stream);
/* state[p]['exp_avg'], ['exp_avg_sq'] and ['step'] of torch.optim's state_dict: two HOST arrays of sum(numel) floats, the
 * tensors dense in list order (each in the order its elements lie in memory), and n_tensors step counts.  Both synchronise
 * `stream`.  Import with a SAM first step pending, a step < 0, null pointers -> VQAE_ERR_INVALID, before any HIP call. */
int vqae_optim_export(vqae_optim* opt, float* exp_avg, float* exp_avg_sq, int64_t* steps, void* stream);
int vqae_optim_import(vqae_optim* opt, const float* exp_avg, const float* exp_avg_sq, const int64_t* steps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 6b. Training forms of the non-conv ops of a Fixup block (conv_block.py:196-216), fp32, NHWC: forward and backward of
 *     everything between the block's convolutions, which stay with the caller.  Every one-element parameter (bias1a ..
 *     bias4, scale, bias1c / bias1d) is a pointer to ONE fp32 ON THE DEVICE and every scalar gradient is written to one fp32
 *     on the device: no call synchronises.  Sums are per-workgroup fp64 partials over a grid that depends on the shape
 *     only, added in a fixed order by a second launch and rounded to fp32 once; no floating-point atomics: bit-identical
 *     run to run.  workspace_dev: vqae_fixup_train_workspace_bytes(n) bytes, 8-byte aligned, n = the element count of the
 *     largest tensor of the call.  Errors, before any HIP call: null pointers, a dimension < 1, a bad act / halo ->
 *     VQAE_ERR_INVALID; more than 2^40 elements, the plain mode with a halo -> VQAE_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
size_t vqae_fixup_train_workspace_bytes(int64_t n_elems);
/* act != 0: y = ELU(x + *a) + *b (alpha 1, expm1-accurate); act == 0 ("plain"): y = x + *b, a unused.
 * x [B][H][W][C].  halo == 0: y [B][H][W][C].  halo == 1 (act only): y [B][H+2][W+2][C] with the circular wrap written,
 * y[b][py][px] = value at ((py-1) mod H, (px-1) mod W): bit for bit F.pad(y, (1, 1, 1, 1), mode='circular'). */
int vqae_fixup_act_f32(const float* x_dev, const float* a_dev, const float* b_dev, int act, int halo, int batch, int h, int w,
                       int c, float* y_dev, void* stream);
/* g: the shape of the forward's y; x [B][H][W][C] and *a: the forward's (NULL for the plain mode).  act: with a halo the
 * padded gradient is first folded onto the interior (each interior pixel adds its images, gather form), then
 *   g_x [B][H][W][C] = fold * ELU'(x + *a), ELU'(v) = v > 0 ? 1 : exp(v);   *g_a = sum g_x;   *g_b = sum fold.
 * plain: *g_b = sum g; g_x is the incoming tensor itself and is not written (pass NULL).  g_a / g_b may be NULL. */
int vqae_fixup_act_backward_f32(const float* g_dev, const float* x_dev, const float* a_dev, int act, int halo, int batch, int h,
                                int w, int c, float* g_x_dev, float* g_a_dev, float* g_b_dev, void* workspace_dev,
                                void* stream);
/* y = (t * *scale + *bias4) + (skip + *bias1d), or + skip where bias1d_dev is NULL (conv_block.py:208-214), n elements. */
int vqae_fixup_out_f32(const float* t_dev, const float* skip_dev, const float* scale_dev, const float* bias4_dev,
                       const float* bias1d_dev, int64_t n, float* y_dev, void* stream);
/* g_t = g * *scale (one rounding);  *g_scale = sum g * t;  *g_bias4 = *g_bias1d = sum g (each may be NULL).  The skip
 * gradient is g itself. */
int vqae_fixup_out_backward_f32(const float* g_dev, const float* t_dev, const float* scale_dev, int64_t n, float* g_t_dev,
                                float* g_scale_dev, float* g_bias4_dev, float* g_bias1d_dev, void* workspace_dev,
                                void* stream);
/* Mixed-precision forms of the four entries above, for training under 16-bit autocast (csrc/fixup_train_io.hip): each
 * tensor is fp32 or a 16-bit type, stated by a VQAE_DT_* code; the one-element parameters, the scalar gradients and the
 * workspace (vqae_fixup_train_workspace_bytes) stay as above.  The arithmetic is the fp32 entry's on the up-cast values,
 * and a 16-bit result is rounded once (RNE, torch's cast): every output tensor is bit for bit the _f32 entry on the
 * up-cast inputs followed by the cast.  The scalar gradients are fp64 sums of the UNROUNDED fp32 terms, in the fp32
 * entries' element order: bit for bit theirs where every tensor is aligned to its 4-element access (16 bytes fp32, 8 bytes
 * 16-bit); any other alignment is taken, on the scalar path.  inf / NaN pass through.  All tensors fp32: the _f32 entry.
 * Errors as above, and: a dtype code outside VQAE_DT_* -> VQAE_ERR_INVALID; two different 16-bit types in one call, a y
 * of vqae_fixup_out_io other than fp32 -> VQAE_ERR_UNSUPPORTED.
 *
 * vqae_fixup_act_io: x (x_dtype) -> y (y_dtype), shapes as vqae_fixup_act_f32. */
int vqae_fixup_act_io(const void* x_dev, int x_dtype, const float* a_dev, const float* b_dev, int act, int halo, int batch,
                      int h, int w, int c, void* y_dev, int y_dtype, void* stream);
/* g has the forward's y dtype (g_dtype), x its own (x_dtype); g_x is written in x_dtype.  Plain mode: x_dev is unused
 * (NULL); where g_dtype == x_dtype g_x is the incoming tensor itself and is not written (pass NULL), otherwise g_x = g
 * cast to x_dtype is written in the pass that sums it. */
int vqae_fixup_act_backward_io(const void* g_dev, int g_dtype, const void* x_dev, int x_dtype, const float* a_dev, int act,
                               int halo, int batch, int h, int w, int c, void* g_x_dev, float* g_a_dev, float* g_b_dev,
                               void* workspace_dev, void* stream);
/* t (t_dtype), skip (skip_dtype) -> y, which is the residual stream: y_dtype must be VQAE_DT_F32. */
int vqae_fixup_out_io(const void* t_dev, int t_dtype, const void* skip_dev, int skip_dtype, const float* scale_dev,
                      const float* bias4_dev, const float* bias1d_dev, int64_t n, void* y_dev, int y_dtype, void* stream);
/* g fp32; g_t = g * *scale is written in t_dtype.  A 16-bit skip_dtype: g_skip_dev gets g cast to it in the same pass;
 * fp32: the skip gradient is g itself and g_skip_dev is not written (pass NULL). */
int vqae_fixup_out_backward_io(const float* g_dev, const void* t_dev, int t_dtype, const float* scale_dev, int64_t n,
                               void* g_t_dev, void* g_skip_dev, int skip_dtype, float* g_scale_dev, float* g_bias4_dev,
                               float* g_bias1d_dev, void* workspace_dev, void* stream);
/* vqae_bicubic_up2_f32 with pre_bias read from the device (NULL: none) and any channel count; per output the same sums
 * in the same order. */
int vqae_bicubic_up2_bias_f32(const float* x_dev, int batch, int h, int w, int c, const float* pre_bias_dev, float* y_dev,
                              void* stream);
/* The exact adjoint: g [B][2H][2W][C] -> g_x [B][H][W][C], gather form (input pixel i adds, over the outputs 2i-3 .. 2i+4 of
 * each axis, the sum of that output's taps whose clamped index is i);  *g_pre_bias = sum g_x (may be NULL). */
int vqae_bicubic_up2_backward_f32(const float* g_dev, int batch, int h, int w, int c, float* g_x_dev, float* g_pre_bias_dev,
                                  void* workspace_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 6b'. The two full-resolution ops of an 'up' block whose 1x1 convs run BEFORE the bicubic x2 (conv_block.py:196-216,
 *     conv.py:4-11: a 1x1 conv and the resize commute, the clamped taps summing to 1), fp32, NHWC, any c >= 1 and h, w >= 1.
 *     up2 is the bicubic of vqae_bicubic_up2_bias_f32 and up2^T the gather of vqae_bicubic_up2_backward_f32: the same sums in
 *     the same order, so each entry is bit for bit the composition of the 6b entries it fuses; what it removes is memory.
 *     One-element parameters, sums, determinism and errors as in 6b.  workspace_dev: vqae_up_train_workspace_bytes(batch, h,
 *     w, c) bytes, 8-byte aligned; h, w are the LOW-resolution extents everywhere.
 * ------------------------------------------------------------------------------------------- */
size_t vqae_up_train_workspace_bytes(int batch, int h, int w, int c);
/* conv_block.py:196-216, conv.py:4-11.  y [B][2H][2W][C] = ELU(v + *a) + *b, v = up2(t_low), t_low [B][H][W][C]; v is not
 * written. */
int vqae_up2_act_f32(const float* t_low_dev, const float* a_dev, const float* b_dev, int batch, int h, int w, int c,
                     float* y_dev, void* stream);
/* conv_block.py:196-216, conv.py:4-11.  g [B][2H][2W][C]; g_v = g * ELU'(v + *a) with v recomputed from t_low (never
 * written);  g_t_low [B][H][W][C] = up2^T g_v;  *g_a = sum g_v;  *g_b = sum g (each may be NULL). */
int vqae_up2_act_backward_f32(const float* g_dev, const float* t_low_dev, const float* a_dev, int batch, int h, int w, int c,
                              float* g_t_low_dev, float* g_a_dev, float* g_b_dev, void* workspace_dev, void* stream);
/* conv_block.py:196-216, conv.py:4-11.  y = (t * *scale + *bias4) + (up2(s_low) + *bias1d); t, y [B][2H][2W][C], s_low
 * [B][H][W][C]; the upsampled skip is not written. */
int vqae_fixup_out_up_f32(const float* t_dev, const float* s_low_dev, const float* scale_dev, const float* bias4_dev,
                          const float* bias1d_dev, int batch, int h, int w, int c, float* y_dev, void* stream);
/* conv_block.py:196-216, conv.py:4-11.  One pass over g [B][2H][2W][C]: g_t = g * *scale;  g_s_low [B][H][W][C] = up2^T g;
 * *g_scale = sum g * t;  *g_bias4 = *g_bias1d = sum g (each may be NULL). */
int vqae_fixup_out_up_backward_f32(const float* g_dev, const float* t_dev, const float* scale_dev, int batch, int h, int w,
                                   int c, float* g_t_dev, float* g_s_low_dev, float* g_scale_dev, float* g_bias4_dev,
                                   float* g_bias1d_dev, void* workspace_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 6c. Trainable 1x1, stride-1 convolutions of a Fixup block (conv_block.py:196-216: branch_conv1, branch_conv3, the 1x1 after
 *     the bicubic of 'up' blocks, skip_conv of 'same' blocks; conf/model/layers/conv_layer/proj2d.yaml: kernel 1, no bias), fp32,
 *     NHWC, with the element-wise op in front of the conv folded into the operand load:
 *         m = B H W rows;  x [m][cin];  w [cout][cin] exactly as torch stores a [cout, cin, 1, 1] weight (no packing);  y [m][cout]
 *         pre = 0: u = x      pre = 1: u = x + *b      pre = 2: u = ELU(x + *a) + *b (alpha 1, expm1-accurate)
 *         y = u . w^T       (u is never written to memory)
 *     a, b: pointers to ONE fp32 ON THE DEVICE (a unused for pre < 2, b for pre < 1); no call synchronises.  All products
 *     run on the fp32-input MFMA.  Grids depend on (m, cin, cout) only, no floating-point atomics: bit-identical run to run.
 *     Supported: cin, cout multiples of 8 in 8 .. 256, any m >= 1; x, w, y and the gradients 16-byte aligned.
 *     Errors, before any HIP call: null pointers, m < 1, pre outside 0 .. 2, misaligned pointers -> VQAE_ERR_INVALID; any other
 *     cin / cout -> VQAE_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
int vqae_conv1x1_train_supported(int cin, int cout);
/* Bytes of workspace of the backward (0 for an unsupported shape or m < 1): P fp64 partials of g_w with P <= 256 and
 * P cin cout <= 2^20 (at most 8 MiB whatever m is), plus 1024 rows of the scalar sums.  8-byte aligned. */
size_t vqae_conv1x1_train_workspace_bytes(int64_t m, int cin, int cout);
/* R: the longest fp32 accumulation run of g_w, in rows.  Longer row ranges are added run by run in fp64. */
int vqae_conv1x1_train_wgrad_run(void);
int vqae_conv1x1_train_forward_f32(const float* x_dev, const float* a_dev, const float* b_dev, int pre, const float* w_dev,
                                   int64_t m, int cin, int cout, float* y_dev, void* stream);
/* From g [m][cout] and the forward's x, a, b, w:
 *   g_u = g . w;   g_x [m][cin] = g_u * ELU'(x + *a) for pre = 2 (ELU'(v) = v > 0 ? 1 : exp(v)), g_u otherwise;
 *   *g_a = sum g_x (pre = 2);   *g_b = sum g_u (pre >= 1);   g_w [cout][cin] = sum_m g[m][co] u[m][ci], u recomputed from x.
 * g_x, g_w, g_a, g_b may each be NULL: what is not asked for is not computed (g_a / g_b are not written for a pre without
 * them).  g_w: fp32 accumulation over runs of at most R rows, the runs added in fp64 in index order, rounded to fp32 once;
 * the scalar sums in fp64 in a fixed order, rounded once. */
int vqae_conv1x1_train_backward_f32(const float* g_dev, const float* x_dev, const float* a_dev, const float* b_dev, int pre,
                                    const float* w_dev, int64_t m, int cin, int cout, float* g_x_dev, float* g_w_dev,
                                    float* g_a_dev, float* g_b_dev, void* workspace_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 6d. Trainable 2x2, stride-2 convolutions of a Fixup 'down' block (conv_block.py:196-216: branch_conv2 and skip_conv;
 *     conf/model/layers/conv_layer/down2d.yaml: kernel 2, stride 2, padding 0, no bias), fp32, NHWC, with the element-wise op in
 *     front of the conv folded into the operand load as in 6c:
 *         x [batch][h][w][cin], h and w even;  y [batch][h/2][w/2][cout];  m = batch (h/2) (w/2) rows
 *         y[b][oh][ow][co] = sum_{kh,kw,ci} u[b][2 oh + kh][2 ow + kw][ci] w[co][ci][kh][kw],   u from x by `pre` as in 6c
 *         w_layout 0: w [cout][cin][2][2] (a contiguous torch weight)    1: w [cout][2][2][cin] (a channels_last one)
 *     Neither layout is copied on the torch side; gradients of w come back in the layout given.  The four taps do not overlap:
 *     the conv is a GEMM with K = 4 cin over gathered rows, on the fp32-input MFMA.  Grids depend on (batch, h, w, cin, cout)
 *     only, no floating-point atomics: bit-identical run to run.
 *     Supported: cin, cout multiples of 8 in 8 .. 256, h and w even, m < 2^40; tensors 16-byte, the workspace 8-byte aligned.
 *     Errors, before any HIP call: null pointers, batch / h / w < 1, m >= 2^40, pre outside 0 .. 2, w_layout outside 0 .. 1,
 *     misaligned pointers -> VQAE_ERR_INVALID; any other cin / cout, odd h or w -> VQAE_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
int vqae_conv_down_train_supported(int cin, int cout);
/* R: the longest fp32 accumulation run of g_w, in rows.  Longer row ranges are added run by run in fp64. */
int vqae_conv_down_train_wgrad_run(void);
/* Bytes of workspace (0 for an unsupported shape): the permuted weight of w_layout 0 (4 cin cout floats), P fp64 partials of
 * g_w with P <= 256 and P 4 cin cout <= 2^21 (at most 16 MiB whatever m is), 4096 rows of the scalar sums: below 17.2 MiB. */
size_t vqae_conv_down_train_workspace_bytes(int64_t batch, int h, int w, int cin, int cout);
/* workspace_dev may be NULL for w_layout 1 (the forward uses it for the permuted weight only). */
int vqae_conv_down_train_forward_f32(const float* x_dev, const float* a_dev, const float* b_dev, int pre, const float* w_dev,
                                     int w_layout, int64_t batch, int h, int w, int cin, int cout, float* y_dev,
                                     void* workspace_dev, void* stream);
/* From g [batch][h/2][w/2][cout] and the forward's x, a, b, w:
 *   g_u = the conv's data gradient (every input element gets exactly one term per co);   g_x [batch][h][w][cin] =
 *   g_u * ELU'(x + *a) for pre = 2, g_u otherwise, every element written once by a plain store;   *g_a = sum g_x (pre = 2);
 *   *g_b = sum g_u (pre >= 1);   g_w (w's layout) = sum_m g[m][co] u[b][2 oh + kh][2 ow + kw][ci], u recomputed from x.
 * g_x, g_w, g_a, g_b may each be NULL.  g_w: fp32 accumulation over runs of at most R rows, the runs added in fp64 in index
 * order, rounded to fp32 once; the scalar sums in fp64 in a fixed order, rounded once. */
int vqae_conv_down_train_backward_f32(const float* g_dev, const float* x_dev, const float* a_dev, const float* b_dev, int pre,
                                      const float* w_dev, int w_layout, int64_t batch, int h, int w, int cin, int cout,
                                      float* g_x_dev, float* g_w_dev, float* g_a_dev, float* g_b_dev, void* workspace_dev,
                                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * 6e. Trainable circular 3x3 convolution of a Fixup 'same' / 'out' block (conv_block.py:196-216: branch_conv2;
 *     conf/model/layers/conv_layer/same2d.yaml: kernel 3, stride 1, padding 1, padding_mode circular, no bias), fp32, NHWC, with
 *     the element-wise op in front of the conv folded into the operand load as in 6c:
 *         x [batch][h][w][cin];  y [batch][h][w][cout];  m = batch h w rows
 *         y[b][i][j][co] = sum_{kh,kw,ci} u[b][(i + kh - 1) mod h][(j + kw - 1) mod w][ci] w[co][ci][kh][kw],   u from x by `pre`
 *         w_layout 0: w [cout][cin][3][3] (a contiguous torch weight)    1: w [cout][3][3][cin] (a channels_last one)
 *     Neither u nor its circular halo is written to memory: the wrap is done in the operand addressing.  For h = 1 (w = 1) all
 *     three kh (kw) read the row (column) itself, as F.pad(mode="circular") does.  Neither layout is copied on the torch
 *     side; gradients of w come back in the layout given.  A GEMM with K = 9 cin over gathered rows on the fp32-input MFMA.
 *     Grids depend on (batch, h, w, cin, cout) only, no floating-point atomics: bit-identical run to run.
 *     Supported: cin, cout multiples of 8 in 8 .. 256, any batch, h, w >= 1 with m < 2^40; tensors 16-byte, the workspace 8-byte
 *     aligned.
 *     Errors, before any HIP call: null pointers, batch / h / w < 1, m >= 2^40, pre outside 0 .. 2, w_layout outside 0 .. 1,
 *     misaligned pointers -> VQAE_ERR_INVALID; any other cin / cout -> VQAE_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
int vqae_conv3x3_train_supported(int cin, int cout);
/* R: the longest fp32 accumulation run of g_w, in rows.  Longer row ranges are added run by run in fp64. */
int vqae_conv3x3_train_wgrad_run(void);
/* Bytes of workspace (0 for an unsupported shape): the permuted weight of w_layout 0 and the flipped, transposed weight of the
 * data gradient (9 cin cout floats each, together at most 4.5 MiB), P fp64 partials of g_w with P <= 256 and
 * P 9 cin cout <= 2^22 (P = 1 above that: at most 32 MiB whatever m is), 1024 rows of the scalar sums: below 36.6 MiB. */
size_t vqae_conv3x3_train_workspace_bytes(int64_t batch, int h, int w, int cin, int cout);
/* workspace_dev may be NULL for w_layout 1 (the forward uses it for the permuted weight only). */
int vqae_conv3x3_train_forward_f32(const float* x_dev, const float* a_dev, const float* b_dev, int pre, const float* w_dev,
                                   int w_layout, int64_t batch, int h, int w, int cin, int cout, float* y_dev,
                                   void* workspace_dev, void* stream);
/* From g [batch][h][w][cout] and the forward's x, a, b, w:
 *   g_u[b][i][j][ci] = sum_{kh,kw,co} g[b][(i - kh + 1) mod h][(j - kw + 1) mod w][co] w[co][ci][kh][kw], GATHERED (the same
 *   circular 3x3 over g with the flipped, transposed weight, written to the workspace on every call), never scattered;
 *   g_x [batch][h][w][cin] = g_u * ELU'(x + *a) for pre = 2, g_u otherwise, every element written once by a plain store;
 *   *g_a = sum g_x (pre = 2);   *g_b = sum g_u (pre >= 1);
 *   g_w (w's layout) = sum_m g[m][co] u[b][(i + kh - 1) mod h][(j + kw - 1) mod w][ci], u recomputed from x.
 * g_x, g_w, g_a, g_b may each be NULL.  g_w: fp32 accumulation over runs of at most R rows, the runs added in fp64 in index
 * order, rounded to fp32 once; the scalar sums in fp64 in a fixed order, rounded once. */
int vqae_conv3x3_train_backward_f32(const float* g_dev, const float* x_dev, const float* a_dev, const float* b_dev, int pre,
                                    const float* w_dev, int w_layout, int64_t batch, int h, int w, int cin, int cout,
                                    float* g_x_dev, float* g_w_dev, float* g_a_dev, float* g_b_dev, void* workspace_dev,
                                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * 6f. Trainable zero-padded 3x3 convolutions with a 3-channel side: encoder.in_stem (model.py:198: 3 -> C0, bias),
 *     decoder.out_stem (model.py:291: C0 -> 3, bias) and the skip_conv of a Fixup 'out' block (conv_block.py:211 with
 *     conf/model/layers/conv_layer/out2d.yaml: kernel 3, stride 1, padding 1, padding_mode zeros, no bias), fp32, NHWC:
 *         x [batch][h][w][cin];  y [batch][h][w][cout];  m = batch h w rows
 *         y[b][i][j][co] = bias[co] + sum_{kh,kw,ci} uz[b][i + kh - 1][j + kw - 1][ci] w[co][ci][kh][kw]
 *         pre = 0: u = x      pre = 1: u = x + *b;      uz = u inside the image and 0 OUTSIDE (the padding follows the pre-op,
 *         as in F.conv2d(x + c, w, padding=1));  pre = 2 has no caller at this seat: VQAE_ERR_UNSUPPORTED
 *         w_layout 0: w [cout][cin][3][3] (a contiguous torch weight)    1: w [cout][3][3][cin] (a channels_last one)
 *     Both layouts are read as they lie (no copy on either side); gradients of w come back in the layout given.  Direct convs on
 *     the vector ALU.  Grids depend on (batch, h, w, cin, cout) only, no floating-point atomics: bit-identical run to run.
 *     Supported: exactly one side of 3 channels -- cin = 3 with cout a multiple of 8 in 8 .. 64, or cout = 3 with cin a
 *     multiple of 8 in 8 .. 256 -- any batch, h, w >= 1 with m < 2^40; tensors 16-byte, the workspace 8-byte aligned.
 *     Errors, before any HIP call, in this order: batch / h / w < 1, pre outside 0 .. 2, w_layout outside 0 .. 1, null pointers
 *     -> VQAE_ERR_INVALID; any other cin / cout, pre = 2 -> VQAE_ERR_UNSUPPORTED; m >= 2^40, misaligned pointers ->
 *     VQAE_ERR_INVALID.
 * ------------------------------------------------------------------------------------------- */
int vqae_conv3x3z_train_supported(int cin, int cout);
/* R: the longest fp32 accumulation run of g_w and g_bias, in rows.  Longer row ranges are added run by run in fp64. */
int vqae_conv3x3z_train_wgrad_run(void);
/* Bytes of workspace of the backward (0 for an unsupported shape): P fp64 partials of g_w (27 C doubles each, C the wide side)
 * and of g_bias (cout each) with P <= 1024 and P 27 C <= 2^21, 1024 rows of the scalar sum: below 16.6 MiB whatever m is. */
size_t vqae_conv3x3z_train_workspace_bytes(int64_t batch, int h, int w, int cin, int cout);
/* bias_dev [cout] or NULL.  a_dev is not read (pre < 2); workspace_dev is not used and may be NULL. */
int vqae_conv3x3z_train_forward_f32(const float* x_dev, const float* a_dev, const float* b_dev, int pre, const float* w_dev,
                                    const float* bias_dev, int w_layout, int64_t batch, int h, int w, int cin, int cout,
                                    float* y_dev, void* workspace_dev, void* stream);
/* From g [batch][h][w][cout] and the forward's x, b, w:
 *   g_x[b][i][j][ci] = sum_{kh,kw,co} g[b][i - kh + 1][j - kw + 1][co] w[co][ci][kh][kw] over the positions inside the image,
 *   GATHERED, every element written once by a plain store;   *g_b = sum g_x (pre = 1);   g_a is not written;
 *   g_w (w's layout) = sum_m g[m][co] uz[b][i + kh - 1][j + kw - 1][ci], u recomputed from x;   g_bias[co] = sum_m g[m][co].
 * g_x, g_w, g_b, g_bias may each be NULL: what is not asked for is not computed.  g_w, g_bias: fp32 accumulation over runs of at
 * most R rows, the runs added in fp64 in index order, rounded to fp32 once; g_b in fp64 in a fixed order, rounded once. */
int vqae_conv3x3z_train_backward_f32(const float* g_dev, const float* x_dev, const float* a_dev, const float* b_dev, int pre,
                                     const float* w_dev, int w_layout, int64_t batch, int h, int w, int cin, int cout,
                                     float* g_x_dev, float* g_w_dev, float* g_a_dev, float* g_b_dev, float* g_bias_dev,
                                     void* workspace_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 6g. Training forms of the non-dense ops of an MBConv block (conv_block.py:240-321, misc.py:7-30; mbconv.yaml): the three
 *     BatchNorms with batch statistics (+ SiLU), the depthwise conv of branch[3] and the SE product, forward and backward,
 *     fp32, NHWC.  The dense 1x1 and skip convs stay with the caller.  One float4 of channels per lane: c a multiple of 4 in
 *     4 .. 1024 (other c: VQAE_ERR_UNSUPPORTED), batch <= 65535, tensors 16-byte and workspaces 8-byte aligned.
 *     Sums: every workgroup reduces VQAE_MBT_ROWS rows in fp64 in a fixed order and writes one fp64 partial row to the
 *     workspace; a second launch adds the rows of one column with VQAE_MBT_FIN_LANES lanes (lane l: rows l, l + 64, ... in
 *     order, then the lanes by shuffle) and rounds to fp32 once.  Grids depend on the shape only, no floating-point atomics:
 *     bit-identical run to run.  No call synchronises.
 *     Errors, before any HIP call: a dimension < 1, null pointers, a bad act / mode, misaligned pointers -> VQAE_ERR_INVALID;
 *     c outside the rule, batch > 65535, batch hw c >= 2^40 -> VQAE_ERR_UNSUPPORTED; one row in training mode ->
 *     VQAE_ERR_VALUE (torch's ValueError).
 * ------------------------------------------------------------------------------------------- */
#define VQAE_MBT_ROWS 256
#define VQAE_MBT_FIN_LANES 64
int vqae_bn_act_train_supported(int c);
/* Bytes of workspace of the forward and of the backward (0 for a bad shape). */
size_t vqae_bn_act_train_workspace_bytes(int batch, int64_t hw, int c);
/* x, y [batch][hw][c]; gamma, beta, running_mean, running_var [c] floats; mean, invstd [c] DOUBLES (at a handful of rows the
 * backward is a difference of nearly equal numbers, and a statistic rounded to fp32 would dominate it); M = batch hw rows.
 * training != 0: mean and the BIASED variance of the M rows (fp64 sums of x - x[0] and its square, so that a constant channel
 *   has variance exactly 0), invstd = 1 / sqrt(var + eps); in the launch that finishes the sums
 *   running_mean = (1 - momentum) running_mean + momentum mean and running_var likewise with the UNBIASED variance
 *   var M / (M - 1) (either may be NULL: not tracked).  M == 1 -> VQAE_ERR_VALUE.
 * training == 0: mean = running_mean, invstd = 1 / sqrt(running_var + eps); no buffer is written.
 * y = act((x - mean) invstd gamma + beta), act 0: identity, 1: SiLU.  mean and invstd are outputs: the backward's inputs.
 * pool [batch][c] or NULL: pool[b][c] = sum over the image's hw rows of y (the squeeze of the SE layer before its division). */
int vqae_bn_act_train_forward_f32(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* running_mean_dev,
                                  float* running_var_dev, int training, double momentum, double eps, int act, int batch,
                                  int64_t hw, int c, float* y_dev, double* mean_dev, double* invstd_dev, float* pool_dev,
                                  void* workspace_dev, void* stream);
/* From g (the gradient of y), the forward's x, mean, invstd, gamma, beta and g_pool [batch][c] (the gradient of pool, or NULL):
 *   xhat = (x - mean) invstd,  z = xhat gamma + beta (recomputed, never stored),  d = (g + g_pool[b]) act'(z) (pool is a sum);
 *   g_beta_gamma [2][c]: row 0 = g_beta = sum d, row 1 = g_gamma = sum d xhat;
 *   g_x = gamma invstd (d - g_beta / M - xhat g_gamma / M) for training != 0, gamma invstd d otherwise: xhat, the unrounded
 *   sums and this combination in fp64, rounded to fp32 once. */
int vqae_bn_act_train_backward_f32(const float* g_dev, const float* x_dev, const double* mean_dev, const double* invstd_dev,
                                   const float* gamma_dev, const float* beta_dev, const float* g_pool_dev, int training, int act,
                                   int batch, int64_t hw, int c, float* g_x_dev, float* g_beta_gamma_dev, void* workspace_dev,
                                   void* stream);
/* Depthwise conv of x [batch][h][w][c] with the module's own weight [c][1][k][k], read in place; no bias, no activation.
 * mode: VQAE_DW_SAME (3x3, circular, any h, w >= 1: the wrap is in the addressing), VQAE_DW_DOWN (2x2 stride 2, h and w even),
 * VQAE_DW_UP (ConvTranspose2d 2x2 stride 2, weight [c][1][2][2]).  Supported: c as above, h, w and the output's at most 16384. */
int vqae_dwconv_train_supported(int c, int h, int w, int mode);
size_t vqae_dwconv_train_workspace_bytes(int batch, int h, int w, int c, int mode);
int vqae_dwconv_train_forward_f32(const float* x_dev, const float* w_dev, int mode, int batch, int h, int w, int c, float* y_dev,
                                  void* stream);
/* h, w: of the forward's x.  g_x (x's shape) is GATHERED, every element written once by a plain store: the same 3x3 over g
 * with flipped taps, the stride-2 modes by each other's kernel.  g_w (w's shape) = sum over batch and pixels of g x at each
 * tap, in fp64 as above.  g_x or g_w may be NULL (x and the workspace are read for g_w only, w for g_x only). */
int vqae_dwconv_train_backward_f32(const float* g_dev, const float* x_dev, const float* w_dev, int mode, int batch, int h, int w,
                                   int c, float* g_x_dev, float* g_w_dev, void* workspace_dev, void* stream);
/* The SE product (misc.py:30): y[b][p][c] = x[b][p][c] gate[b][c];  g_x = g gate,  g_gate[b][c] = sum_p g x. */
size_t vqae_se_scale_workspace_bytes(int batch, int64_t hw, int c);
int vqae_se_scale_forward_f32(const float* x_dev, const float* gate_dev, int batch, int64_t hw, int c, float* y_dev, void* stream);
int vqae_se_scale_backward_f32(const float* g_dev, const float* x_dev, const float* gate_dev, int batch, int64_t hw, int c,
                               float* g_x_dev, float* g_gate_dev, void* workspace_dev, void* stream);
/* Mixed-precision forms of the six entries above, for training under 16-bit autocast (csrc/mbconv_train_io.hip): the _f32
 * signatures with void* tensors plus dtype codes.  The [batch][h][w][c] tensors of a call (x, y, g, g_x) share ONE type,
 * io_dtype (VQAE_DT_*); gamma, beta, the running statistics, pool, g_pool, g_beta_gamma and g_w stay fp32, mean and invstd
 * fp64, the weight of the depthwise conv the module's own fp32 one.  gate and g_gate share a code of their own, gate_dtype:
 * VQAE_DT_F32 or io_dtype.  The vqae_*_supported and vqae_*_workspace_bytes functions above hold unchanged (the partial rows
 * are fp64 either way).
 * The values are up-cast on load (exact), the arithmetic and the element-to-thread order are the fp32 entries', and a 16-bit
 * result is rounded once on store (RNE, torch's cast): every tensor output is bit for bit the _f32 entry on the up-cast
 * inputs followed by the cast, and every sum (mean, invstd, the running statistics, pool, g_beta_gamma, g_w, an fp32 g_gate)
 * is the _f32 entry's bit for bit, taken from the UNROUNDED fp32 terms.  A BatchNorm + SiLU node therefore rounds ONCE (y), where
 * stock torch under autocast rounds z and SiLU(z); its backward recomputes z from the saved 16-bit x in fp32.  The depthwise taps
 * are rounded to io_dtype in registers (autocast casts the conv weight), in the forward and in the data gradient.  A 16-bit
 * g_gate is the fp32 sum rounded once more.  inf / NaN pass through.  io_dtype VQAE_DT_F32: the _f32 entry.
 * Errors as above, and: a dtype code outside VQAE_DT_* -> VQAE_ERR_INVALID; a 16-bit tensor (or gate) not on 8 bytes, an fp32
 * one not on 16 -> VQAE_ERR_INVALID; two different 16-bit types in one call, a 16-bit gate beside fp32 tensors ->
 * VQAE_ERR_UNSUPPORTED. */
int vqae_bn_act_train_forward_io(const void* x_dev, const float* gamma_dev, const float* beta_dev, float* running_mean_dev,
                                 float* running_var_dev, int training, double momentum, double eps, int act, int batch,
                                 int64_t hw, int c, void* y_dev, double* mean_dev, double* invstd_dev, float* pool_dev,
                                 void* workspace_dev, int io_dtype, void* stream);
int vqae_bn_act_train_backward_io(const void* g_dev, const void* x_dev, const double* mean_dev, const double* invstd_dev,
                                  const float* gamma_dev, const float* beta_dev, const float* g_pool_dev, int training, int act,
                                  int batch, int64_t hw, int c, void* g_x_dev, float* g_beta_gamma_dev, void* workspace_dev,
                                  int io_dtype, void* stream);
int vqae_dwconv_train_forward_io(const void* x_dev, const float* w_dev, int mode, int batch, int h, int w, int c, void* y_dev,
                                 int io_dtype, void* stream);
int vqae_dwconv_train_backward_io(const void* g_dev, const void* x_dev, const float* w_dev, int mode, int batch, int h, int w,
                                  int c, void* g_x_dev, float* g_w_dev, void* workspace_dev, int io_dtype, void* stream);
int vqae_se_scale_forward_io(const void* x_dev, const void* gate_dev, int batch, int64_t hw, int c, void* y_dev, int io_dtype,
                             int gate_dtype, void* stream);
int vqae_se_scale_backward_io(const void* g_dev, const void* x_dev, const void* gate_dev, int batch, int64_t hw, int c,
                              void* g_x_dev, void* g_gate_dev, void* workspace_dev, int io_dtype, int gate_dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 7. Counts of stored code grids -- produces what the reference commits as data under scripts/create_wsi_histograms/
 *    (embedding_idx_histogram_{K}_{split}.npy, histogram_{split}.npy; it ships no program for them) and reads its loss
 *    weights from (conf/model/optional_overrides/loss_f/bce_with_logits_loss_camelyon16_embeddings.yaml: "values taken
 *    from validation marginal"): the joint (label x code) histogram of a batch of equally sized grids, in exact integers.
 *      hist[b][l][k] = number of positions of grid b with mask == l and code == k.
 *    No float appears anywhere: the result does not depend on summation order, partition or batch position, and a bin may
 *    exceed 2^24 (vqae_vq_code_stats_f32, the training bookkeeping of section 1, counts in fp32).
 * ------------------------------------------------------------------------------------------- */
enum { VQAE_HIST_MAX_LABELS = 8 };
/* Bytes of scratch vqae_code_histogram needs (0 for an empty batch or a bad shape; grows with batch). */
size_t vqae_code_histogram_workspace_bytes(int batch, int64_t n_per_grid, int n_codes, int n_labels);
/*   codes_dev  [B][n_per_grid] of idx_dtype (VQAE_IDX_*, as stored), any alignment the element type allows (a contiguous
 *              view into a larger tensor; a uint8 grid may start at an odd address);
 *   mask_dev   uint8 [B][n_per_grid] (any address), or NULL: every position then has label 0 and n_labels must be 1;
 *   hist_dev   int64 [B][n_labels][n_codes], or [1][n_labels][n_codes] with pooled != 0 (the sum over the batch);
 *   bad_dev    int64 [B or 1][2] or NULL: bad[0] = positions whose code lies outside 0 .. n_codes-1 (negative codes of the
 *              signed widths included, whatever their label), bad[1] = positions with a code in range and a label >=
 *              n_labels.  Neither kind is counted in hist or used as an index: hist.sum() + bad[0] + bad[1] == n_per_grid
 *              per grid;
 *   accumulate != 0: the counts are ADDED to what hist_dev and bad_dev hold (pool a whole split on the device, download
 *              once); otherwise both are overwritten, every zero bin included;
 *   workspace_dev  vqae_code_histogram_workspace_bytes(...) bytes, 8-byte aligned.
 * Tables of n_labels * n_codes + 2 <= 32768 bins are counted in LDS (every shipped K = 128 .. 1024 with 3 labels, and
 * K = 8192 with 3); larger ones, up to K = 65536 with 8 labels, with 64-bit integer atomics straight into hist_dev.
 * Errors, all before any HIP call: null codes / hist / workspace, n_labels > 1 without a mask, a bad idx_dtype,
 * n_per_grid < 1, batch < 0 -> VQAE_ERR_INVALID; n_codes outside 1 .. 65536, n_labels outside 1 .. VQAE_HIST_MAX_LABELS,
 * batch > 65535 -> VQAE_ERR_UNSUPPORTED.  batch == 0 -> VQAE_OK (without accumulate a pooled table is zeroed). */
int vqae_code_histogram(const void* codes_dev, int idx_dtype, const uint8_t* mask_dev, int batch, int64_t n_per_grid,
                        int n_codes, int n_labels, int pooled, int accumulate, int64_t* hist_dev, int64_t* bad_dev,
                        void* workspace_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQAE_HIP_H */
