"""Training through the Fixup mirrors: every op of a PreActFixupResBlock that is not a convolution (conv_block.py:196-216)
is a fused HIP forward / backward (csrc/fixup_train.hip) behind a torch.autograd.Function; the convolutions themselves are
`torch.nn.functional.conv2d` on the block's own `weight` Parameters, whose gradients torch has on ROCm.  Of the four seams
per block (conv1, conv2, conv3, skip_conv) the 1x1, stride-1 ones have a kernel of ours behind the keyword `conv1x1`:

    conv1x1="torch"  (default)   every conv is F.conv2d: the graph this module has always built, op for op
    conv1x1="hip"                every 1x1, stride-1 conv whose channel counts csrc/conv_train.hip takes (multiples of 8 up
                                 to 256) is ONE node together with the op in front of it: fixup_act + conv1 / conv3,
                                 fixup_add + the skip conv of a 'same' block, the 1x1 after the bicubic of an 'up' block.
                                 Other shapes (Co = 3 of an 'out' block) take the torch route, counted in
                                 stats["conv1x1_fallbacks"]; stats["conv1x1_hip"] counts the fused nodes.
The 2x2, stride-2 convs of a 'down' block (branch_conv2, skip_conv) have one behind the independent keyword `conv_down`:

    conv_down="torch" (default)  F.conv2d(..., stride=2) behind fixup_act / fixup_add, as always
    conv_down="hip"              each is ONE node of csrc/conv_train.hip with the op in front of it folded in (fixup_act +
                                 branch_conv2, fixup_add + skip_conv): the activation in front of branch_conv2, the largest tensor
                                 of a step, is never written.  Odd H or W and channel counts outside the kernels' rule take the
                                 torch route, counted in stats["conv_down_fallbacks"]; stats["conv_down_hip"] counts the nodes.
The circular 3x3 conv of a 'same' or 'out' block (branch_conv2, 9/11 of a trunk block's FLOPs) has one behind the independent
keyword `conv3x3`:

    conv3x3="torch" (default)    fixup_act(..., halo=1) writes ELU(t + bias2a) + bias2b with its circular halo,
                                 [B, H + 2, W + 2, C], and F.conv2d runs on that, as always
    conv3x3="hip"                ONE node of csrc/conv_train.hip: the activation is folded into the operand staging and the wrap
                                 into the operand addressing, so neither the activation nor its halo is written or kept.  Channel
                                 counts outside the kernels' rule take the torch route, counted in stats["conv3x3_fallbacks"];
                                 stats["conv3x3_hip"] counts the nodes.
The zero-padded 3x3 convs with a 3-channel side -- encoder.in_stem (3 -> C0, bias), decoder.out_stem (C0 -> 3, bias) and the
skip_conv of an 'out' block (C -> 3) -- have one behind the independent keyword `conv3x3z`:

    conv3x3z="torch" (default)   F.conv2d(..., padding=1), behind fixup_add(x, bias1c) for the skip_conv, as always
    conv3x3z="hip"               ONE node of csrc/conv_train_thin.hip, a direct conv on the vector ALU: the conv's bias and, for
                                 the skip_conv, x + bias1c are folded in, and the zeros are padded behind the pre-op by select, so
                                 no padded or re-laid-out copy of a full-resolution tensor exists.  Channel counts outside the
                                 kernels' rule (one side 3, the other a multiple of 8) take the torch route, counted in
                                 stats["conv3x3z_fallbacks"]; stats["conv3x3z_hip"] counts the nodes.
The 'up' blocks have a fifth, independent keyword, `conv_up`, which selects the ORDER of the block and two fused nodes, not a
conv kernel (the 1x1 convs stay routed by `conv1x1`):

    conv_up="torch" (default)    conv2 and the skip_conv run at FULL resolution, behind bicubic_up2, as always
    conv_up="hip"                a 1x1 conv and the bicubic x2 commute (the conv mixes channels per pixel, the resize pixels per
                                 channel, and its clamped taps sum to 1, so the pre-bias commutes too): conv2 and the skip_conv run
                                 at LOW resolution, a quarter of the FLOPs and of the weight gradients' rows, and the resize moves
                                 into the two element-wise ops behind them, each ONE node of csrc/up_train.hip:
                                 up2_act = ELU(up2(t_low) + bias3a) + bias3b in front of conv3, and fixup_out_up = (t * scale +
                                 bias4) + (up2(s_low) + bias1d).  No upsampled tensor is written in either direction.  Any shape;
                                 stats["conv_up_hip"] counts the nodes (two per block); stats["conv_up_fallbacks"] counts the
                                 'up' blocks without a skip_conv, which no constructor builds and which raise as the torch route.
With all five keywords at their defaults the graph is op for op the one described above.
No conv then stays with torch except branch_conv3 8 -> 3 of an 'out' block, a counted conv1x1 fall-back (no shipped config
instantiates an 'out' block), and the quantiser's 1x1 projections, which have their own fused backward (layers/vq.py).

    block_forward(block, x)      one block, NCHW in and out, any of the four modes, with or without a skip_conv
    forward_train(model, x)      VQAE.forward (vq_ae/model.py:41-48) over a vqae_amd.model.VQAE mirror -> (out, (vq_loss,))
    step(model, batch, loss_f)   VQAE.step (vq_ae/model.py:114-122) -> (out, recon_loss, (vq_loss,))
    conv1x1(x, w, a, b)          the fused node on [B, H, W, Ci]
    conv_down(x, w, a, b)        the fused 2x2, stride-2 node: [B, H, W, Ci] -> [B, H/2, W/2, Co]
    conv3x3(x, w, a, b)          the fused circular 3x3 node: [B, H, W, Ci] -> [B, H, W, Co]
    conv3x3z(x, w, bias, c)      the fused zero-padded 3x3 node with a 3-channel side: [B, H, W, Ci] -> [B, H, W, Co]
    up2_act(t_low, a, b)         ELU(bicubic_up2(t_low) + a) + b as one node: [B, H, W, C] -> [B, 2H, 2W, C]
    fixup_out_up(t, s_low, scale, bias4, bias1d)   (t * scale + bias4) + (bicubic_up2(s_low) + bias1d) as one node

The functional ops (fixup_act, fixup_add, fixup_out, bicubic_up2) take channel-last tensors [B, H, W, C], like every other
op of the package.  The graph stays channel-last throughout (the reference trains in channels_last: model.py:124-126): a conv
sees the NCHW-shaped view of an NHWC tensor, and a conv result that comes back in another layout is copied once
(`stats["layout_copies"]` counts those copies, `stats["layout_checks"]` the places where one could happen).

The one-element parameters (bias1a .. bias4, scale, bias1c / bias1d) are read by the kernels from device memory and their
gradients are written to device tensors by fixed-order fp64 sums: a step never synchronises the host for them, and two runs
of any op here give the same bits -- under conv1x1="hip" the 1x1 convs and their weight gradients included, under
conv_down="hip" the 2x2, stride-2 ones, under conv3x3="hip" the circular 3x3 ones: under conv1x1="hip", conv3x3="hip" no conv
of a 'same' block is MIOpen's, and every gradient of the block repeats bit for bit; under conv3x3z="hip" the stems and the
'out' block's skip_conv too, so that with all four keywords "hip" no conv of a step on a shipped-style spec is MIOpen's and two
runs of the step give the same gradients bit for bit.

Each Function has a restatement in plain torch ops, taken when its tensors are on the CPU: the same forward, and the SAME
hand-derived backward (the gather-fold of the halo, the bicubic adjoint, the fixed-order sums), which is what
torch.autograd.gradcheck checks in tests/test_fixup_train_cpu.py.  The Functions are once-differentiable.

16-bit autocast (`torch.autocast("cuda", dtype=torch.bfloat16 | torch.float16)` around the step; no keyword -- autocast is the
switch; f16 with torch.amp.GradScaler, inf / NaN pass through the nodes as through torch's ops).  The reference's rounding
points under autocast: a conv output is 16-bit; `conv_out + bias` promotes to fp32 (the biases are fp32 [1] Parameters), so
ELU and the second bias are fp32; the next conv rounds its input to 16 bits; `out * scale + bias4 + x` is fp32, so the
residual stream stays fp32; the gradient of a 16-bit tensor is 16-bit, of an fp32 tensor fp32.  The three element-wise nodes
fixup_act, fixup_add and fixup_out follow them with 16-bit I/O (csrc/fixup_train_io.hip, ops.*_io):

    reads     a 16-bit tensor (a conv output) as it is -- no `.float()` copy -- and saves it as it is: half the activation
              memory of these nodes
    writes    the autocast dtype where the consumer is an F.conv2d on the torch route with nothing in between (feeds_conv:
              the bits the conv's own cast of the fp32 result would read, the cast kernel gone), fp32 anywhere else: an act in
              front of bicubic_up2 stays fp32, and fixup_out always writes fp32
    backward  g in the output's dtype, g_x in the input's; the scalar gradients are fp32, fp64 sums of the unrounded terms

The arithmetic is the fp32 kernels' on the up-cast values with one rounding on store, so a node is bit for bit its fp32 form
between the casts torch would have made.  With every tensor fp32 the Functions call what they always called.
stats["io16_hip"] counts the nodes that ran a 16-bit form; stats["io16_fallbacks"] counts, under autocast, the nodes that have
none and run their fp32 kernels on explicitly cast operands, correct but not 16-bit-native: the resize nodes (bicubic_up2,
up2_act, fixup_out_up) and the fused conv nodes of the "hip" routes, which get fp32 operands.  The quantiser runs fp32, as in
the reference (cdist is an fp32 op under autocast); MBConv training under autocast is train_mbconv.py's.
"""
import functools

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import ops
from .layers.conv_block import PreActFixupResBlock
from .layers.vq import ProjectedEMAVectorQuantizer2d

stats = {"layout_checks": 0, "layout_copies": 0, "conv1x1_hip": 0, "conv1x1_fallbacks": 0, "conv_down_hip": 0,
         "conv_down_fallbacks": 0, "conv3x3_hip": 0, "conv3x3_fallbacks": 0, "conv3x3z_hip": 0, "conv3x3z_fallbacks": 0,
         "conv_up_hip": 0, "conv_up_fallbacks": 0, "io16_hip": 0, "io16_fallbacks": 0}
ROUTES = ("torch", "hip")                           # of each of the keywords conv1x1, conv_down, conv3x3, conv3x3z, conv_up
CONV1X1_ROUTES = CONV_DOWN_ROUTES = CONV3X3_ROUTES = CONV3X3Z_ROUTES = CONV_UP_ROUTES = ROUTES

_W75 = (-0.03515625, 0.26171875, 0.87890625, -0.10546875)     # even outputs: inputs m-2 .. m+1, m = o >> 1
_W25 = (-0.10546875, 0.87890625, 0.26171875, -0.03515625)     # odd outputs:  inputs m-1 .. m+2


def _dense(t):
    stats["layout_checks"] += 1
    if not t.is_contiguous():
        stats["layout_copies"] += 1
        t = t.contiguous()
    return t


def to_nhwc(x):
    """NCHW-shaped tensor -> its [B, H, W, C] form, a view when x is channels_last already."""
    return _dense(x.permute(0, 2, 3, 1))


def to_nchw(x):
    """[B, H, W, C] -> the NCHW-shaped (channels_last) view."""
    return x.permute(0, 3, 1, 2)


# ---- plain-torch restatements (CPU) ------------------------------------------------------------------------------------
def _wrap_index(n, device):
    return torch.arange(-1, n + 1, device=device) % n


def pad_circular_nhwc(y):
    """F.pad(y, (1, 1, 1, 1), mode='circular') of the NCHW view, on [B, H, W, C]."""
    return y[:, _wrap_index(y.shape[1], y.device)][:, :, _wrap_index(y.shape[2], y.device)]


def fold_circular_nhwc(g):
    """The adjoint of pad_circular_nhwc: [B, H + 2, W + 2, C] -> [B, H, W, C], every interior pixel the sum of its images."""
    B, PH, PW, C = g.shape
    rows = g.new_zeros((B, PH - 2, PW, C)).index_add_(1, _wrap_index(PH - 2, g.device), g)
    return g.new_zeros((B, PH - 2, PW - 2, C)).index_add_(2, _wrap_index(PW - 2, g.device), rows)


def elu_grad(v):
    """ELU'(v), alpha = 1: 1 where v > 0, exp(v) elsewhere."""
    return torch.where(v > 0, torch.ones_like(v), torch.exp(v))


@functools.lru_cache(maxsize=64)
def _up2_matrix_cached(n):
    a = torch.zeros(2 * n, n, dtype=torch.float64)
    for o in range(2 * n):
        odd = o & 1
        base = (o >> 1) - (1 if odd else 2)
        for k in range(4):
            a[o, min(max(base + k, 0), n - 1)] += (_W25 if odd else _W75)[k]
    return a


def up2_matrix(n, dtype=torch.float64, device="cpu"):
    """[2n, n]: the bicubic x2 operator (A = -0.75, align_corners False, clamped indices) along one axis.  Row o holds the sums
    of o's taps by clamped index; its non-zeros lie in the columns i with 2i - 3 <= o <= 2i + 4, the window the kernel walks."""
    return _up2_matrix_cached(int(n)).to(device=device, dtype=dtype)


def _bicubic_up2_torch(x, pre_bias):
    ah, aw = up2_matrix(x.shape[1], x.dtype, x.device), up2_matrix(x.shape[2], x.dtype, x.device)
    v = x if pre_bias is None else x + pre_bias
    return torch.einsum("oh,bhwc->bowc", ah, torch.einsum("pw,bhwc->bhpc", aw, v))


def _bicubic_up2_adjoint_torch(g):
    ah, aw = up2_matrix(g.shape[1] // 2, g.dtype, g.device), up2_matrix(g.shape[2] // 2, g.dtype, g.device)
    return torch.einsum("pw,bhpc->bhwc", aw, torch.einsum("oh,bowc->bhwc", ah, g))


def _like(g, p):
    """A [1] sum as the gradient of parameter p."""
    return g.reshape(p.shape).to(p.dtype)


# ---- dtypes under autocast -----------------------------------------------------------------------------------------------------
_IO16 = (torch.bfloat16, torch.float16)


def autocast16(t):
    """The 16-bit dtype an F.conv2d rounds its input to under the autocast that is on for t's device; None without one."""
    kind = t.device.type
    if not torch.is_autocast_enabled(kind):
        return None
    dtype = torch.get_autocast_dtype(kind)
    return dtype if dtype in _IO16 else None


def _one16(*dtypes):
    """Whether the dtypes hold one 16-bit type at most (the kernels' rule)."""
    return len({d for d in dtypes if d in _IO16}) <= 1


def _up(t):
    """A 16-bit tensor up-cast (exact); any other as it is."""
    return t.float() if t.dtype in _IO16 else t


# ---- autograd Functions --------------------------------------------------------------------------------------------------
class _ActFn(torch.autograd.Function):
    """y = ELU(x + a) + b (+ circular halo).  Saves x: ELU' from the output, (y - b) + 1, has no correct bits where the ELU
    saturates, and Adam steps dead channels by the sign of that noise (DESIGN section 16 has both measured distances).
    out_dtype: None (fp32 on the device, the promoted dtype on the CPU) or the 16-bit dtype of the conv that reads y.  A 16-bit
    x (a conv output under autocast) is read and saved as it is; g_x has x's dtype."""

    @staticmethod
    def forward(ctx, x, a, b, halo, out_dtype):
        if x.is_cuda and (x.dtype in _IO16 or out_dtype in _IO16):
            if not _one16(x.dtype, out_dtype):
                x = x.float()
            stats["io16_hip"] += 1
            y = ops.fixup_act_io(x, a, b, halo, out_dtype or torch.float32)
        elif x.is_cuda:
            y = ops.fixup_act(x.float(), a, b, halo)
        else:
            y = F.elu(x + a) + b                        # a, b are [1] fp32 tensors: a 16-bit x promotes to fp32
            if out_dtype is not None:
                y = y.to(out_dtype)
            if halo:
                y = pad_circular_nhwc(y)
        ctx.save_for_backward(x, a)
        ctx.halo, ctx.b = halo, b
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, a = ctx.saved_tensors
        if g.is_cuda and (g.dtype in _IO16 or x.dtype in _IO16):
            g_x, g_a, g_b = ops.fixup_act_backward_io(_dense(g), x, a, ctx.halo)
        elif g.is_cuda:
            g_x, g_a, g_b = ops.fixup_act_backward(_dense(g.float()), x.float(), a, ctx.halo)
        else:
            g = _up(g)
            if ctx.halo:
                g = fold_circular_nhwc(g)
            g_x = g * elu_grad(x + a)
            g_a, g_b = g_x.sum(), g.sum()               # of the unrounded terms
            g_x = g_x.to(x.dtype)
        return g_x, _like(g_a, a), _like(g_b, ctx.b), None, None


class _AddFn(torch.autograd.Function):
    """y = x + c, c a one-element parameter.  g_c = sum g; g_x is the incoming gradient itself, or, where y and x differ in
    dtype (a 16-bit y of an fp32 x, an fp32 y of a 16-bit x), its cast, written by the launch that sums it."""

    @staticmethod
    def forward(ctx, x, c, out_dtype):
        ctx.c, ctx.x_dtype = c, x.dtype
        if x.is_cuda and (x.dtype in _IO16 or out_dtype in _IO16):
            if not _one16(x.dtype, out_dtype):
                x = x.float()
            stats["io16_hip"] += 1
            return ops.fixup_act_io(x, None, c, 0, out_dtype or torch.float32)
        if x.is_cuda:
            return ops.fixup_act(x.float(), None, c)
        y = x + c
        return y if out_dtype is None else y.to(out_dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g.is_cuda and (g.dtype in _IO16 or ctx.x_dtype in _IO16) and _one16(g.dtype, ctx.x_dtype):
            g, _, g_c = ops.fixup_act_backward_io(_dense(g), None, None, act=False, x_dtype=ctx.x_dtype)
        elif g.is_cuda:
            g, _, g_c = ops.fixup_act_backward(_dense(g.float()), None, None, act=False)
        else:
            g_c = _up(g).sum()
            g = g.to(ctx.x_dtype)
        return g, _like(g_c, ctx.c), None


class _OutFn(torch.autograd.Function):
    """y = (t * scale + bias4) + (skip [+ bias1d]), the fp32 residual stream.  t and skip may each be 16-bit (conv outputs under
    autocast): they are read, and t is saved, as they are; g_t has t's dtype and a 16-bit skip gets its own copy of g."""

    @staticmethod
    def forward(ctx, t, skip, scale, bias4, bias1d):
        ctx.skip_dtype = skip.dtype
        if t.is_cuda and (t.dtype in _IO16 or skip.dtype in _IO16):
            stats["io16_hip"] += 1
            y = ops.fixup_out_io(t, _dense(skip), scale, bias4, bias1d)
        elif t.is_cuda:
            y = ops.fixup_out(t.float(), _dense(skip.float()), scale, bias4, bias1d)
        else:
            y = (t * scale + bias4) + (skip if bias1d is None else skip + bias1d)
        ctx.save_for_backward(t, scale)
        ctx.b4, ctx.b1d = bias4, bias1d
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        t, scale = ctx.saved_tensors
        if g.is_cuda and (t.dtype in _IO16 or ctx.skip_dtype in _IO16):
            g_t, g_skip, g_scale, g_bias = ops.fixup_out_backward_io(_dense(g.float()), t, scale, ctx.skip_dtype)
        elif g.is_cuda:
            g_skip = _dense(g.float())
            g_t, g_scale, g_bias = ops.fixup_out_backward(g_skip, t.float(), scale)
        else:
            g = _up(g)
            g_t, g_skip, g_scale, g_bias = (g * scale).to(t.dtype), g.to(ctx.skip_dtype), (g * t).sum(), g.sum()
        return (g_t, g_skip, _like(g_scale, scale), _like(g_bias, ctx.b4),
                _like(g_bias, ctx.b1d) if ctx.b1d is not None else None)


class _BicubicFn(torch.autograd.Function):
    """y = bicubic_x2(x + pre_bias) (nn.Upsample of ResizeConv2D, layers/conv.py:8) and its exact adjoint."""

    @staticmethod
    def forward(ctx, x, pre_bias):
        ctx.pb = pre_bias
        if not x.is_cuda:
            with torch.autocast("cpu", enabled=False):
                return _bicubic_up2_torch(_up(x), pre_bias)
        if pre_bias is None and x.shape[3] % 4 == 0:
            return ops.bicubic_up2(x.float())                  # the inference kernel: the same sums in the same order
        return ops.bicubic_up2_bias(x.float(), pre_bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g.is_cuda:
            g_x, g_pb = ops.bicubic_up2_backward(_dense(g.float()), want_bias=ctx.pb is not None)
        else:
            g_x = _bicubic_up2_adjoint_torch(_up(g))
            g_pb = g_x.sum()
        return g_x, _like(g_pb, ctx.pb) if ctx.pb is not None else None


class _Up2ActFn(torch.autograd.Function):
    """y = ELU(up2(t_low) + a) + b, up2 the bicubic x2 of _BicubicFn.  Saves t_low only: the backward recomputes up2(t_low) for
    ELU' (csrc/up_train.hip: in LDS), so no full-resolution tensor is kept or written."""

    @staticmethod
    def forward(ctx, t_low, a, b):
        if t_low.is_cuda:
            y = ops.up2_act(t_low.float(), a, b)
        else:
            with torch.autocast("cpu", enabled=False):
                y = F.elu(_bicubic_up2_torch(_up(t_low), None) + a) + b
        ctx.save_for_backward(t_low, a)
        ctx.b = b
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        t_low, a = ctx.saved_tensors
        if g.is_cuda:
            g_t_low, g_a, g_b = ops.up2_act_backward(_dense(g.float()), t_low.float(), a)
        else:
            g_v = _up(g) * elu_grad(_bicubic_up2_torch(_up(t_low), None) + a)
            g_t_low, g_a, g_b = _bicubic_up2_adjoint_torch(g_v), g_v.sum(), g.sum()
        return g_t_low, _like(g_a, a), _like(g_b, ctx.b)


class _OutUpFn(torch.autograd.Function):
    """y = (t * scale + bias4) + (up2(s_low) + bias1d): the output op of an 'up' block whose skip_conv ran at low resolution."""

    @staticmethod
    def forward(ctx, t, s_low, scale, bias4, bias1d):
        if t.is_cuda:
            y = ops.fixup_out_up(t.float(), _dense(s_low.float()), scale, bias4, bias1d)
        else:
            with torch.autocast("cpu", enabled=False):
                y = (t * scale + bias4) + (_bicubic_up2_torch(_up(s_low), None) + bias1d)
        ctx.save_for_backward(t, scale)
        ctx.b4, ctx.b1d = bias4, bias1d
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        t, scale = ctx.saved_tensors
        if g.is_cuda:
            g_t, g_s_low, g_scale, g_bias = ops.fixup_out_up_backward(_dense(g.float()), t.float(), scale)
        else:
            g = _up(g)
            g_t, g_s_low, g_scale, g_bias = g * scale, _bicubic_up2_adjoint_torch(g), (g * t).sum(), g.sum()
        return g_t, g_s_low, _like(g_scale, scale), _like(g_bias, ctx.b4), _like(g_bias, ctx.b1d)


def _pre_op_torch(x, a, b):
    if b is None:
        return x
    return x + b if a is None else F.elu(x + a) + b


class _PreConvFn(torch.autograd.Function):
    """The ctx plumbing of a conv node with the op in front of it folded in: u = x (a, b None), x + b (a None) or
    ELU(x + a) + b.  Saves x, w and whichever of a, b exist -- not u: the backward recomputes it for g_w and takes ELU' from
    x + a.  On the device it is ops.<NODE>_train_forward / _backward; a node names itself and states its restatement for CPU
    tensors, _forward(x, w, a, b) -> y and _backward(g, x, w, a, b, need_x, need_w) -> (g_x, g_w, g_a, g_b)."""

    @classmethod
    def forward(cls, ctx, x, w, a, b):
        ctx.save_for_backward(x, w, *(t for t in (a, b) if t is not None))
        ctx.has = (a is not None, b is not None)
        if x.is_cuda:
            return getattr(ops, cls.NODE + "_train_forward")(x.float(), w, a, b)
        with torch.autocast("cpu", enabled=False):
            return cls._forward(_up(x), w, a, b)

    @classmethod
    @once_differentiable
    def backward(cls, ctx, g):
        x, w, *ab = ctx.saved_tensors
        a = ab[0] if ctx.has[0] else None
        b = ab[-1] if ctx.has[1] else None
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g.is_cuda:
            g, x, backward = _dense(g.float()), x.float(), getattr(ops, cls.NODE + "_train_backward")
        else:
            g, x, backward = _up(g), _up(x), cls._backward
        g_x, g_w, g_a, g_b = backward(g, x, w, a, b, need_x, need_w)
        return (g_x if need_x else None, g_w.to(w.dtype) if need_w else None, _like(g_a, a) if a is not None else None,
                _like(g_b, b) if b is not None else None)


class _Conv1x1Fn(_PreConvFn):
    """y = u . w^T on [B, H, W, Ci], w [Co, Ci, 1, 1]."""
    NODE = "conv1x1"

    @staticmethod
    def _forward(x, w, a, b):
        return to_nhwc(F.conv2d(to_nchw(_pre_op_torch(x, a, b)), w))

    @staticmethod
    def _backward(g, x, w, a, b, need_x, need_w):
        w2 = w.reshape(w.shape[0], w.shape[1])
        g_u = g @ w2
        g_x = g_u * elu_grad(x + a) if a is not None else g_u
        g_w = None
        if need_w:
            u = _pre_op_torch(x, a, b)
            g_w = (g.reshape(-1, g.shape[-1]).t() @ u.reshape(-1, u.shape[-1])).reshape(w.shape)
        return g_x, g_w, g_x.sum(), g_u.sum()


def conv1x1(x, w, a=None, b=None):
    """A 1x1, stride-1 conv on [B, H, W, Ci] -> [B, H, W, Co], w [Co, Ci, 1, 1], of ELU(x + a) + b (a None: of x + b; both
    None: of x) as ONE node: csrc/conv_train.hip on the device, a plain-torch restatement on CPU tensors."""
    assert a is None or b is not None
    return _Conv1x1Fn.apply(x, w, a, b)


def _space_to_depth(t):
    """[B, H, W, C] (H, W even) -> [B H/2 W/2, 4 C], column (kh, kw, c): the rows of the 2x2, stride-2 conv's GEMM."""
    B, H, W, C = t.shape
    return t.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4 * C)


def _depth_to_space(m, B, OH, OW):
    """The inverse (and, the map being a permutation, the adjoint) of _space_to_depth."""
    C = m.shape[-1] // 4
    return m.reshape(B, OH, OW, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * OH, 2 * OW, C)


class _ConvDownFn(_PreConvFn):
    """y [B, H/2, W/2, Co] = the 2x2, stride-2 conv (no padding, no bias) of u [B, H, W, Ci] with w [Co, Ci, 2, 2].  The four
    taps do not overlap, so the backward is two matmuls on the space-to-depth form: g_u = depth_to_space(g . w2),
    g_w = g^T . space_to_depth(u), w2 [Co, (kh, kw, ci)]."""
    NODE = "conv_down"

    @staticmethod
    def _forward(x, w, a, b):
        return to_nhwc(F.conv2d(to_nchw(_pre_op_torch(x, a, b)), w, stride=2))

    @staticmethod
    def _backward(g, x, w, a, b, need_x, need_w):
        B, OH, OW, Co = g.shape
        g2 = g.reshape(-1, Co)
        g_u = _depth_to_space(g2 @ w.permute(0, 2, 3, 1).reshape(Co, -1), B, OH, OW)
        g_x = g_u * elu_grad(x + a) if a is not None else g_u
        g_w = None
        if need_w:
            g_w = (g2.t() @ _space_to_depth(_pre_op_torch(x, a, b))).reshape(Co, 2, 2, -1).permute(0, 3, 1, 2)
            if w.is_contiguous():
                g_w = g_w.contiguous()
        return g_x, g_w, g_x.sum(), g_u.sum()


def conv_down(x, w, a=None, b=None):
    """The 2x2, stride-2 conv on [B, H, W, Ci] (H, W even) -> [B, H/2, W/2, Co], w [Co, Ci, 2, 2], of ELU(x + a) + b (a None:
    of x + b; both None: of x) as ONE node: csrc/conv_train.hip on the device, a plain-torch restatement on CPU tensors."""
    assert a is None or b is not None
    assert x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0, x.shape
    return _ConvDownFn.apply(x, w, a, b)


class _Conv3x3Fn(_PreConvFn):
    """y [B, H, W, Co] = the 3x3, stride-1 conv with circular padding 1 (no bias) of u [B, H, W, Ci] with w [Co, Ci, 3, 3].  The
    taps overlap: the data gradient is the fold of the padded one (the adjoint of the wrap), g_w a matmul on the unfolded
    patches of the padded u."""
    NODE = "conv3x3"

    @staticmethod
    def _forward(x, w, a, b):
        return to_nhwc(F.conv2d(to_nchw(pad_circular_nhwc(_pre_op_torch(x, a, b))), w))

    @staticmethod
    def _backward(g, x, w, a, b, need_x, need_w):
        Co = g.shape[-1]
        # the padded data gradient [B, H + 2, W + 2, Ci]: pixel (p, q) collects g[p - kh][q - kw] . w[:, :, kh, kw]
        g_u = fold_circular_nhwc(F.conv_transpose2d(to_nchw(g), w).permute(0, 2, 3, 1))
        g_x = g_u * elu_grad(x + a) if a is not None else g_u
        g_w = None
        if need_w:
            patches = pad_circular_nhwc(_pre_op_torch(x, a, b)).unfold(1, 3, 1).unfold(2, 3, 1)      # [B, H, W, Ci, kh, kw]
            g_w = (g.reshape(-1, Co).t() @ patches.reshape(-1, 9 * x.shape[-1])).reshape(w.shape)
            if not w.is_contiguous() and w.is_contiguous(memory_format=torch.channels_last):
                g_w = g_w.contiguous(memory_format=torch.channels_last)
        return g_x, g_w, g_x.sum(), g_u.sum()


def conv3x3(x, w, a=None, b=None):
    """The 3x3, stride-1, circular-padding-1 conv on [B, H, W, Ci] -> [B, H, W, Co], w [Co, Ci, 3, 3], of ELU(x + a) + b (a
    None: of x + b; both None: of x) as ONE node: csrc/conv_train.hip on the device, a plain-torch restatement on CPU tensors."""
    assert a is None or b is not None
    return _Conv3x3Fn.apply(x, w, a, b)


def _conv3x3z_backward_torch(g, x, w, c, need_x, need_w, need_bias):
    """The hand-derived backward of F.conv2d(x + c, w, bias, padding=1) on [B, H, W, C] tensors -> (g_x, g_w, g_bias, g_c)."""
    Co = g.shape[-1]
    # the data gradient of the padded input [B, H + 2, W + 2, Ci], cropped: the rim's gradient belongs to the zeros
    g_x = F.conv_transpose2d(to_nchw(g), w)[:, :, 1:-1, 1:-1].permute(0, 2, 3, 1)
    g_w = None
    if need_w:
        u = x if c is None else x + c
        patches = F.pad(u, (0, 0, 1, 1, 1, 1)).unfold(1, 3, 1).unfold(2, 3, 1)                    # [B, H, W, Ci, kh, kw]
        g_w = (g.reshape(-1, Co).t() @ patches.reshape(-1, 9 * x.shape[-1])).reshape(w.shape)
        if not w.is_contiguous() and w.is_contiguous(memory_format=torch.channels_last):
            g_w = g_w.contiguous(memory_format=torch.channels_last)
    return g_x, g_w, g.sum((0, 1, 2)) if need_bias else None, g_x.sum()


class _Conv3x3zFn(torch.autograd.Function):
    """y [B, H, W, Co] = bias + the 3x3, stride-1 conv with ZERO padding 1 of u = x + c (c None: x) with w [Co, Ci, 3, 3]: the
    stems and the skip_conv of an 'out' block.  The zeros are padded after the pre-op.  Saves x, w and c, not u.  On the device
    ops.conv3x3z_train_forward / _backward (csrc/conv_train_thin.hip); on CPU tensors the restatement above."""

    @staticmethod
    def forward(ctx, x, w, bias, c):
        ctx.save_for_backward(x, w, *(() if c is None else (c,)))
        ctx.bias = bias
        if x.is_cuda:
            return ops.conv3x3z_train_forward(x.float(), w, bias, c)
        with torch.autocast("cpu", enabled=False):
            x = _up(x)
            return to_nhwc(F.conv2d(to_nchw(x if c is None else x + c), w, bias, padding=1))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w, *rest = ctx.saved_tensors
        c = rest[0] if rest else None
        need_x, need_w, need_bias = ctx.needs_input_grad[:3]
        need_bias = need_bias and ctx.bias is not None
        if g.is_cuda:
            g_x, g_w, g_bias, g_c = ops.conv3x3z_train_backward(_dense(g.float()), x.float(), w, c, need_x, need_w, need_bias)
        else:
            g_x, g_w, g_bias, g_c = _conv3x3z_backward_torch(_up(g), _up(x), w, c, need_x, need_w, need_bias)
        return (g_x if need_x else None, g_w.to(w.dtype) if need_w else None,
                g_bias.to(ctx.bias.dtype) if need_bias else None, _like(g_c, c) if c is not None else None)


def conv3x3z(x, w, bias=None, c=None):
    """The 3x3, stride-1, zero-padding-1 conv on [B, H, W, Ci] -> [B, H, W, Co], w [Co, Ci, 3, 3], bias [Co] or None, of x + c
    (c None: of x) as ONE node -- F.conv2d(x + c, w, bias, padding=1): csrc/conv_train_thin.hip on the device (one side of 3
    channels: ops.conv3x3z_train_supported), a plain-torch restatement on CPU tensors."""
    return _Conv3x3zFn.apply(x, w, bias, c)


def fixup_act(x, a, b, halo=0, feeds_conv=False):
    """ELU(x + a) + b on [B, H, W, C]; halo = 1: [B, H + 2, W + 2, C] with the circular wrap written.  feeds_conv: an F.conv2d
    reads the result directly, so under 16-bit autocast the result is written in the autocast dtype -- the bits the conv's own
    cast of the fp32 result would read; anywhere else, and without autocast, the result is fp32."""
    return _ActFn.apply(x, a, b, int(halo), autocast16(x) if feeds_conv else None)


def fixup_add(x, c, feeds_conv=False):
    """x + c; feeds_conv as in fixup_act."""
    return _AddFn.apply(x, c, autocast16(x) if feeds_conv else None)


def fixup_out(t, skip, scale, bias4, bias1d=None):
    return _OutFn.apply(t, skip, scale, bias4, bias1d)


def _fp32_node(x):
    """A node without a 16-bit form (the resize nodes, the fused conv nodes): under 16-bit autocast it runs its fp32 kernels
    on explicitly cast operands, correct but not 16-bit-native, and is counted."""
    if autocast16(x) is not None:
        stats["io16_fallbacks"] += 1


def bicubic_up2(x, pre_bias=None):
    _fp32_node(x)
    return _BicubicFn.apply(x, pre_bias)


def up2_act(t_low, a, b):
    """ELU(bicubic_up2(t_low) + a) + b on [B, H, W, C] -> [B, 2H, 2W, C] as ONE node: csrc/up_train.hip on the device, a
    plain-torch restatement on CPU tensors."""
    _fp32_node(t_low)
    return _Up2ActFn.apply(t_low, a, b)


def fixup_out_up(t, s_low, scale, bias4, bias1d):
    """(t * scale + bias4) + (bicubic_up2(s_low) + bias1d), t [B, 2H, 2W, C], s_low [B, H, W, C], as ONE node: csrc/up_train.hip
    on the device, a plain-torch restatement on CPU tensors."""
    assert tuple(t.shape) == (s_low.shape[0], 2 * s_low.shape[1], 2 * s_low.shape[2], s_low.shape[3]), (t.shape, s_low.shape)
    _fp32_node(t)
    return _OutUpFn.apply(t, s_low, scale, bias4, bias1d)


# ---- blocks and the model ------------------------------------------------------------------------------------------------
def _conv(t, w, bias=None, stride=1, padding=0):
    """F.conv2d on a channel-last tensor, channel-last result."""
    return to_nhwc(F.conv2d(to_nchw(t), w, bias, stride=stride, padding=padding))


def conv_routes(conv1x1="torch", conv_down="torch", conv3x3="torch", conv3x3z="torch", conv_up="torch"):
    """The five route keywords, checked -> {node: whether its convs are the fused nodes of csrc/conv_train.hip and
    csrc/conv_train_thin.hip; "conv_up": whether an 'up' block runs its convs at low resolution around csrc/up_train.hip}."""
    routes = dict(conv1x1=conv1x1, conv_down=conv_down, conv3x3=conv3x3, conv3x3z=conv3x3z, conv_up=conv_up)
    for keyword, value in routes.items():
        if value not in ROUTES:
            raise ValueError(f"{keyword} must be one of {ROUTES}, not {value!r}")
    return {node: value == "hip" for node, value in routes.items()}


def _pre_torch(x, a, b):
    """The op in front of an F.conv2d on the torch route: nothing sits between them, so under autocast it writes 16 bits."""
    if b is None:
        return x
    return fixup_add(x, b, feeds_conv=True) if a is None else fixup_act(x, a, b, feeds_conv=True)


# node -> (the fused node, the torch route).  conv3x3's: the activation writes the wrap, the conv pads nothing.  conv3x3z's: the
# conv pads zeros behind x + b, and takes the conv's bias (its pre-op is never an activation: a is None).
_NODES = {"conv1x1": (conv1x1, lambda x, a, b, w: _conv(_pre_torch(x, a, b), w)),
          "conv_down": (conv_down, lambda x, a, b, w: _conv(_pre_torch(x, a, b), w, stride=2)),
          "conv3x3": (conv3x3, lambda x, a, b, w: _conv(fixup_act(x, a, b, halo=1, feeds_conv=True), w)),
          "conv3x3z": (lambda x, w, a, b, bias=None: conv3x3z(x, w, bias, b),
                       lambda x, a, b, w, bias=None: _conv(_pre_torch(x, a, b), w, bias, padding=1))}


def _pre_conv(node, hip, x, a, b, w, bias=None):
    """The conv of a node of ops.L.CONV_TRAIN on ELU(x + a) + b (a None: x + b; both None: x).  hip[node]: one fused node where
    the kernels take the shape (the node's kernel size, H and W multiples of its stride, their channel rule); any other
    shape takes the torch route and is counted.  bias: the conv's own, for a node with a bias seat."""
    fused, torch_route = _NODES[node]
    extra = () if bias is None else (bias,)
    if hip[node]:
        _, k, stride, _, _ = ops.L.CONV_TRAIN[node]
        if (tuple(w.shape[2:]) == (k, k) and x.shape[1] % stride == 0 and x.shape[2] % stride == 0
                and getattr(ops, node + "_train_supported")(w.shape[1], w.shape[0])):
            stats[node + "_hip"] += 1
            _fp32_node(x)
            return fused(x, w, a, b, *extra)
        stats[node + "_fallbacks"] += 1
    return torch_route(x, a, b, w, *extra)


def _up_block_low(block, x, hip):
    """An 'up' block in the commuted order (conv_up = "hip"): conv2 and the skip_conv at LOW resolution, the bicubic x2 inside
    the two ops behind them.  up2(conv(u)) = conv(up2(u)) for a 1x1 conv, and up2(s) + c = up2(s + c), so this is the block's
    function; the sums are the same products in another order."""
    t = _pre_conv("conv1x1", hip, x, block.bias1a, block.bias1b, block.branch_conv1.weight)
    t_low = _pre_conv("conv1x1", hip, t, block.bias2a, block.bias2b, block.branch_conv2.weight)
    stats["conv_up_hip"] += 1
    u = up2_act(t_low, block.bias3a, block.bias3b)
    t = _pre_conv("conv1x1", hip, u, None, None, block.branch_conv3.weight)
    s_low = _pre_conv("conv1x1", hip, x, None, block.bias1c, block.skip_conv.weight)
    stats["conv_up_hip"] += 1
    return fixup_out_up(t, s_low, block.scale, block.bias4, block.bias1d)


def block_forward_nhwc(block, x, **routes):
    """conv_block.py:196-216 on [B, H, W, C] with a graph: the fused ops around F.conv2d.  routes: the keywords of conv_routes,
    each "torch" by default.  conv1x1 = "hip": every 1x1, stride-1 conv the kernels support is one node with the op in front
    of it (csrc/conv_train.hip); conv_down = "hip": so is each 2x2, stride-2 conv of a 'down' block; conv3x3 = "hip": so is
    the circular 3x3 of a 'same' or 'out' block; conv3x3z = "hip": so is the zero-padded 3x3 skip_conv of an 'out' block
    (csrc/conv_train_thin.hip); "torch": F.conv2d.  conv_up = "hip": an 'up' block runs conv2 and its skip_conv at low
    resolution, with the bicubic x2 inside up2_act and fixup_out_up (csrc/up_train.hip); "torch": behind bicubic_up2."""
    if not isinstance(block, PreActFixupResBlock):
        raise NotImplementedError(f"training is implemented for Fixup blocks only (no MBConv / BatchNorm training), not "
                                  f"{type(block).__name__}")
    hip = conv_routes(**routes)
    mode = block.mode
    if mode == "up" and hip["conv_up"]:
        if block.skip_conv is not None:
            return _up_block_low(block, x, hip)
        # No constructor builds an 'up' block without a skip_conv, and fixup_out_up has no such form (t and x differ in shape):
        # counted, and the order below raises on those shapes as it always has.
        stats["conv_up_fallbacks"] += 1
    t = _pre_conv("conv1x1", hip, x, block.bias1a, block.bias1b, block.branch_conv1.weight)
    if mode in ("same", "out"):                         # 3x3 circular
        t = _pre_conv("conv3x3", hip, t, block.bias2a, block.bias2b, block.branch_conv2.weight)
    elif mode == "down":
        t = _pre_conv("conv_down", hip, t, block.bias2a, block.bias2b, block.branch_conv2.weight)
    else:                                               # ResizeConv2D: bicubic x2, then 1x1
        t = _pre_conv("conv1x1", hip, bicubic_up2(fixup_act(t, block.bias2a, block.bias2b)), None, None, block.branch_conv2.weight)
    t = _pre_conv("conv1x1", hip, t, block.bias3a, block.bias3b, block.branch_conv3.weight)
    if block.skip_conv is None:
        return fixup_out(t, x, block.scale, block.bias4)
    w = block.skip_conv.weight
    if mode == "up":
        skip = _pre_conv("conv1x1", hip, bicubic_up2(x, block.bias1c), None, None, w)
    elif mode == "down":
        skip = _pre_conv("conv_down", hip, x, None, block.bias1c, w)
    elif mode == "same":
        skip = _pre_conv("conv1x1", hip, x, None, block.bias1c, w)
    else:                                               # out2d: 3x3, zero padding
        skip = _pre_conv("conv3x3z", hip, x, None, block.bias1c, w)
    return fixup_out(t, skip, block.scale, block.bias4, block.bias1d)


def _compute_dtype(x):
    """fp32 on the device; fp64 CPU tensors stay fp64 (gradcheck, the fp64 restatement)."""
    return x if x.dtype == torch.float64 and not x.is_cuda else x.float()


def block_forward(block, x, **routes):
    """One PreActFixupResBlock mirror on an NCHW-shaped tensor (channels_last preferred: no copy) -> NCHW-shaped, with a graph.
    routes: conv1x1 / conv_down / conv3x3 / conv3x3z / conv_up, as in block_forward_nhwc."""
    return to_nchw(block_forward_nhwc(block, to_nhwc(_compute_dtype(x)), **routes))


def block_forward_torch(block, x):
    """The same block written with stock torch ops only (F.elu, F.pad, F.interpolate, the same F.conv2d), NCHW-shaped in and
    out, autograd's own backward: the yardstick of the tests and of tools/bench_fixup_train.py.  No training path calls it."""
    mode, conv = block.mode, F.conv2d
    up = lambda t: F.interpolate(t, scale_factor=2, mode="bicubic", align_corners=False)
    t = conv(F.elu(x + block.bias1a) + block.bias1b, block.branch_conv1.weight)
    t = F.elu(t + block.bias2a) + block.bias2b
    if mode in ("same", "out"):
        t = conv(F.pad(t, (1, 1, 1, 1), mode="circular"), block.branch_conv2.weight)
    elif mode == "down":
        t = conv(t, block.branch_conv2.weight, stride=2)
    else:
        t = conv(up(t), block.branch_conv2.weight)
    t = conv(F.elu(t + block.bias3a) + block.bias3b, block.branch_conv3.weight)
    t = t * block.scale + block.bias4
    if block.skip_conv is None:
        return t + x
    s, w = x + block.bias1c, block.skip_conv.weight
    if mode == "up":
        s = conv(up(s), w)
    elif mode == "down":
        s = conv(s, w, stride=2)
    else:
        s = conv(s, w, padding=1 if mode == "out" else 0)
    return t + (s + block.bias1d)


def _quantize_torch(vq, inputs):
    """EMAVectorQuantizer.forward (vq.py:96-154; :190-192 for the projected form) in torch ops, for tensors on the CPU: the
    restatement of the device quantiser, its training-mode bookkeeping (vq.py:47-94) included."""
    projected = isinstance(vq, ProjectedEMAVectorQuantizer2d)
    z = F.conv2d(inputs, vq.proj_in.weight, vq.proj_in.bias) if projected else inputs
    with torch.no_grad():
        cl = z.permute(0, 2, 3, 1)
        flat = cl.reshape(-1, vq.embedding_dim)
        if vq.first_pass and vq.training:
            vq._init_ema(flat)
        idx = torch.argmin(torch.cdist(flat, vq.embed, 4, compute_mode="donot_use_mm_for_euclid_dist"), dim=1)
        q = vq.embed[idx].reshape(cl.shape).permute(0, 3, 1, 2)
        if vq.training:
            onehot = F.one_hot(idx, num_classes=vq.num_embeddings).type_as(flat)
            vq.cluster_size.mul_(vq.decay).add_(onehot.sum(dim=0), alpha=1 - vq.decay)
            vq.embed_avg.mul_(vq.decay).add_(onehot.T @ flat, alpha=1 - vq.decay)
            n = vq.cluster_size.sum()
            size = n * ((vq.cluster_size + vq.laplace_alpha) / (n + vq.num_embeddings * vq.laplace_alpha))
            vq.embed.copy_(vq.embed_avg / size.unsqueeze(-1))
    loss = F.mse_loss(z, q) * vq.commitment_cost
    q = z + (q - z).detach()
    if projected:
        q = F.conv2d(q, vq.proj_out.weight, vq.proj_out.bias)
    return q, idx.reshape(cl.shape[:-1]), loss


def forward_train(model, x, return_indices=False, **routes):
    """VQAE.forward (vq_ae/model.py:41-48) over a vqae_amd.model.VQAE mirror, with a graph: -> (out, (vq_loss,)), out NCHW-shaped
    (channels_last).  The stems are F.conv2d (conv3x3z = "hip": the fused zero-padded node, where the kernels take the stem's
    width), the blocks block_forward, the quantiser its own trainable mirror (its EMA buffers are updated in training mode, as in
    the reference).  routes: conv1x1 / conv_down / conv3x3 / conv3x3z / conv_up = "torch" (default) | "hip", the routes of the
    blocks' 1x1, 2x2 stride-2, circular 3x3 and zero-padded 3x3 convs and the order of the 'up' blocks (block_forward_nhwc)."""
    hip = conv_routes(**routes)
    enc, dec = model.encoder, model.decoder
    h = to_nhwc(_compute_dtype(x))
    h = _pre_conv("conv3x3z", hip, h, None, None, enc.in_stem.weight, enc.in_stem.bias)
    for level in enc.down_layers[0].layers:
        for blk in level.layers:
            h = block_forward_nhwc(blk, h, **routes)
    for blk in enc.pre_enc_layers[0]:
        h = block_forward_nhwc(blk, h, **routes)
    vq = enc.vq_layers[0]
    q, idx, vq_loss = vq(to_nchw(h)) if h.is_cuda else _quantize_torch(vq, to_nchw(h))
    h = to_nhwc(q)
    for blk in dec.post_enc_layers[0]:
        h = block_forward_nhwc(blk, h, **routes)
    for level in dec.up_layers[0].layers:
        for blk in level.layers:
            h = block_forward_nhwc(blk, h, **routes)
    out = to_nchw(_pre_conv("conv3x3z", hip, h, None, None, dec.out_stem.weight, dec.out_stem.bias))
    if return_indices:
        return out, (vq_loss,), (idx,)
    return out, (vq_loss,)


def step(model, batch, loss_f=F.huber_loss, **routes):
    """VQAE.step (vq_ae/model.py:114-122): -> (out, recon_loss, (vq_loss,)); the caller backpropagates recon_loss + sum(vq_loss).
    routes: conv1x1 / conv_down / conv3x3 / conv3x3z / conv_up, as in forward_train."""
    out, encoding_loss = forward_train(model, batch, **routes)
    return out, loss_f(input=out, target=batch), encoding_loss
