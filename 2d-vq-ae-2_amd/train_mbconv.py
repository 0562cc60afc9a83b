"""Training through the MBConv mirrors (reference vq_ae/layers/conv_block.py:240-321, vq_ae/layers/misc.py:7-30): every op of
an MBConv block that is not a dense conv is a fused HIP forward / backward (csrc/mbconv_train.hip) behind a
torch.autograd.Function; the dense 1x1 convs and the skip convs are `F.conv2d` / `F.conv_transpose2d` on the block's own
`weight` Parameters, the SE gate's two Linear layers torch ops on [B, e].  The graph of one block:

    x -- conv2d 1x1 -- bn_act(SiLU) -- dwconv -- bn_act(SiLU, pool) -- se_scale -- conv2d 1x1 -- bn_act -- + -- y
     \\                                               \\ pool / HW -- fc -- gate /                          /
      \\------------------------------------------ skip (x or its conv) --------------------------------/

    bn_act(x, bn, silu, want_pool)   BatchNorm2d of an nn.BatchNorm2d's parameters and buffers (+ SiLU) on [B, H, W, C]: batch
                                     statistics and the in-place running-statistics update where bn.training, the running
                                     statistics otherwise; want_pool: -> (y, pool [B, C] = sum_hw y), the squeeze of the SE layer
    dwconv(x, w, mode)               the depthwise conv of branch[3], w [e, 1, k, k] read in place; mode "same" | "out" (3x3
                                     circular), "down" (2x2 stride 2), "up" (ConvTranspose 2x2 stride 2)
    se_scale(x, gate)                x * gate[b, c]
    block_forward(block, x)          one block, NCHW in and out (block_forward_nhwc: [B, H, W, C])
    forward_train(model, x)          VQAE.forward over a vqae_amd.model.VQAE mirror of an MBConv spec -> (out, (vq_loss,))
    step(model, batch, loss_f)       VQAE.step -> (out, recon_loss, (vq_loss,))

Saved for backward: bn_act keeps x, mean and invstd, never z -- the backward recomputes z and SiLU'(z); dwconv keeps x and w;
se_scale keeps x and gate.  Route rules: the kernels take channel counts that are multiples of 4 (up to 1024) and, for the
stride-2 depthwise conv, even H and W.  A BatchNorm of another width (the 3 channels of an 'out' block's last one) runs the
plain-torch restatement on the device, counted in stats["bn_fallbacks"] beside stats["bn_hip"]; a depthwise conv outside the
rule runs F.conv2d(groups=e) / F.conv_transpose2d, counted in stats["dwconv_fallbacks"] beside stats["dwconv_hip"].

Every sum of the three nodes (the batch statistics, g_gamma / g_beta, pool, the depthwise weight gradient, g_gate) is a
fixed-order fp64 sum without atomics: two runs give the same bits.  The dense convs' gradients are torch's.

Each Function has a restatement in plain torch ops, taken when its tensors are on the CPU: the same forward and the SAME
hand-derived backward, which is what torch.autograd.gradcheck checks in tests/test_mbconv_train_cpu.py.  The Functions are
once-differentiable.  train.py and the inference mirrors are untouched: `train.forward_train` still refuses an MBConv model
and `layers.conv_block.MBConv` still refuses `.train()`; the trainable module is layers.mbconv_train.MBConv.

16-bit autocast (`torch.autocast("cuda", dtype=torch.bfloat16 | torch.float16)` around the step; no keyword -- autocast is the
switch, because the convs produce the 16-bit tensors; f16 with torch.amp.GradScaler, inf / NaN pass through the nodes as
through torch's ops).  The reference's rounding points: under autocast EVERY activation tensor of an MBConv block is 16-bit --
the conv outputs, the BatchNorm output, SiLU, the depthwise conv, the SE mean, the gate, the SE product, the last BatchNorm and
the residual sum -- while the running statistics and every parameter gradient stay fp32.  So, unlike the Fixup stacks, the
residual stream is 16-bit, and each of the three nodes reads and writes 16 bits (csrc/mbconv_train_io.hip, ops.*_io):

    reads     a 16-bit x as it is -- no `.float()` copy -- and saves it as it is: half the saved activation memory of the node
    writes    y, and in the backward g_x, in x's dtype, rounded ONCE on store from the fp32 arithmetic of the fp32 kernels
    small     mean, invstd fp64; pool, g_gamma, g_beta, g_w, the running statistics fp32, all sums of the UNROUNDED fp32 terms;
              the gate (and g_gate) in fp32 or x's dtype, as the gate MLP hands it over; the depthwise taps are the module's
              fp32 weight rounded to x's dtype in registers (autocast casts a conv weight)

One rounding per node, on purpose: stock torch rounds z to 16 bits between BatchNorm and SiLU and again behind SiLU; the fused
node rounds y only, and its backward recomputes z from the saved 16-bit x in fp32.  A node is therefore bit for bit its fp32 form
between the casts torch would have made, not bit for bit the reference's 16-bit run; the tests hold it to the distance to fp64.
With every tensor fp32 the Functions call what they always called.  The fall-backs (a BatchNorm or depthwise conv outside the
route rule) and the CPU restatements follow the same rule in plain torch ops: a 16-bit input is up-cast, the arithmetic is fp32
with autocast off, the result is rounded once to the input's dtype.  io16_stats["io16_hip"] counts the nodes that ran a 16-bit
kernel, io16_stats["io16_fallbacks"] the 16-bit tensors that took a torch restatement on the device (a dict beside `stats`,
whose four route counters keep counting every node).  forward_train up-casts the pre-VQ
features to fp32 in front of the quantiser (cdist is an fp32 op under autocast); `t + skip`, the SE gate MLP and
num_batches_tracked stay torch ops.
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib as L
from . import ops, train
from .layers.conv_block import MBConv as _MBConvMirror
from .train import _IO16, _compute_dtype, _dense, autocast16, pad_circular_nhwc, to_nchw, to_nhwc

stats = {"bn_hip": 0, "bn_fallbacks": 0, "dwconv_hip": 0, "dwconv_fallbacks": 0}
# beside `stats` and not in it: tests/test_mbconv_train_gpu.py pins the key set of `stats` to the four route counters
io16_stats = {"io16_hip": 0, "io16_fallbacks": 0}
DW_MODES = {"same": L.DW_SAME, "out": L.DW_SAME, "down": L.DW_DOWN, "up": L.DW_UP}


def silu_grad(z):
    """SiLU'(z) = s (1 + z (1 - s)), s = sigmoid(z)."""
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _bump(t):
    """A kernel wrote t in place: tell torch (the inference mirrors key their folded weights on the version counters)."""
    if hasattr(torch.autograd.graph, "increment_version"):
        torch.autograd.graph.increment_version(t)
    else:
        t.add_(0)


def _fp32_math(t):
    """The context of a torch restatement on a 16-bit tensor: autocast off for t's device, so that the up-cast operands stay
    fp32 through F.conv2d and the einsums."""
    return torch.autocast(t.device.type, enabled=False)


def _count16(x, fused):
    """A node on a 16-bit device tensor: a 16-bit kernel (fused) or a torch restatement."""
    if x.is_cuda and x.dtype in _IO16:
        io16_stats["io16_hip" if fused else "io16_fallbacks"] += 1


# ---- autograd Functions --------------------------------------------------------------------------------------------------
def _bn_forward_torch(x, gamma, beta, running_mean, running_var, training, momentum, eps, silu, want_pool):
    """The restatement of bn_act's forward on an up-cast x (the 16-bit rule) -> (y, mean, invstd, pool | None), all fp32."""
    B, H, W, C = x.shape
    M = B * H * W
    if training:
        mean = x.mean((0, 1, 2))
        var = ((x - mean) ** 2).mean((0, 1, 2))
        if running_mean is not None:
            running_mean.mul_(1 - momentum).add_(mean.to(running_mean.dtype), alpha=momentum)
        if running_var is not None:
            running_var.mul_(1 - momentum).add_((var * (M / (M - 1))).to(running_var.dtype), alpha=momentum)
    else:
        mean, var = running_mean.to(x.dtype), running_var.to(x.dtype)
    invstd = torch.rsqrt(var + eps)
    z = (x - mean) * invstd * gamma + beta
    y = F.silu(z) if silu else z
    return y, mean, invstd, (y.sum((1, 2)) if want_pool else None)


def _bn_backward_torch(g, g_pool, x, mean, invstd, gamma, beta, training, silu):
    """The hand-derived backward of bn_act on up-cast g and x -> (g_x, g_gamma, g_beta), all fp32."""
    B, H, W, C = x.shape
    if g_pool is not None:
        g = g + g_pool.reshape(B, 1, 1, C)
    xhat = (x - mean) * invstd
    d = g * silu_grad(xhat * gamma + beta) if silu else g
    g_beta, g_gamma = d.sum((0, 1, 2)), (d * xhat).sum((0, 1, 2))
    M = B * H * W
    g_x = gamma * invstd * (d - g_beta / M - xhat * (g_gamma / M) if training else d)
    return g_x, g_gamma, g_beta


class _BnActFn(torch.autograd.Function):
    """(y, pool) = BatchNorm2d (+ SiLU) of x [B, H, W, C]; pool [B, C] = sum_hw y where want_pool, else an empty tensor.  Saves x,
    mean, invstd -- not z.  A 16-bit x is read and saved as it is; y and g_x have its dtype, pool and the statistics do not."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, silu, want_pool):
        B, H, W, C = x.shape
        M = B * H * W
        if training and M <= 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {[B, C, H, W]}")
        hip = x.is_cuda and ops.bn_act_train_supported(C)
        if hip:
            fwd = ops.bn_act_train_forward_io if x.dtype in _IO16 else ops.bn_act_train_forward
            y, mean, invstd, pool = fwd(x if x.dtype in _IO16 else x.float(), gamma, beta, running_mean, running_var, training,
                                        momentum, eps, silu, want_pool)
            if training:
                for t in (running_mean, running_var):
                    if t is not None:
                        _bump(t)
        elif x.dtype in _IO16:
            with _fp32_math(x):
                y, mean, invstd, pool = _bn_forward_torch(x.float(), gamma.float(), beta.float(), running_mean, running_var,
                                                          training, momentum, eps, silu, want_pool)
            y = y.to(x.dtype)
        else:
            if training:
                mean = x.mean((0, 1, 2))
                var = ((x - mean) ** 2).mean((0, 1, 2))
                if running_mean is not None:
                    running_mean.mul_(1 - momentum).add_(mean.to(running_mean.dtype), alpha=momentum)
                if running_var is not None:
                    running_var.mul_(1 - momentum).add_((var * (M / (M - 1))).to(running_var.dtype), alpha=momentum)
            else:
                mean, var = running_mean.to(x.dtype), running_var.to(x.dtype)
            invstd = torch.rsqrt(var + eps)
            z = (x - mean) * invstd * gamma + beta
            y = F.silu(z) if silu else z
            pool = y.sum((1, 2)) if want_pool else None
        ctx.save_for_backward(x, mean, invstd, gamma, beta)
        ctx.conf = (hip, bool(training), bool(silu), bool(want_pool))
        ctx.set_materialize_grads(False)
        if pool is None:
            pool = x.new_empty(0)
            ctx.mark_non_differentiable(pool)
        return y, pool

    @staticmethod
    @once_differentiable
    def backward(ctx, g, g_pool):
        x, mean, invstd, gamma, beta = ctx.saved_tensors
        hip, training, silu, want_pool = ctx.conf
        if not want_pool:
            g_pool = None
        if g is None:
            g = torch.zeros_like(x)
        B, H, W, C = x.shape
        if hip and x.dtype in _IO16:
            g_x, g_gamma, g_beta = ops.bn_act_train_backward_io(_dense(g.to(x.dtype)), x, mean, invstd, gamma, beta, training,
                                                                silu, g_pool)
        elif hip:
            g_x, g_gamma, g_beta = ops.bn_act_train_backward(_dense(g.float()), x.float(), mean, invstd, gamma, beta, training,
                                                             silu, g_pool)
        elif x.dtype in _IO16:
            with _fp32_math(x):
                g_x, g_gamma, g_beta = _bn_backward_torch(g.float(), None if g_pool is None else g_pool.float(), x.float(), mean,
                                                          invstd, gamma.float(), beta.float(), training, silu)
            g_x = g_x.to(x.dtype)
        else:
            if g_pool is not None:
                g = g + g_pool.reshape(B, 1, 1, C)
            xhat = (x - mean) * invstd
            d = g * silu_grad(xhat * gamma + beta) if silu else g
            g_beta, g_gamma = d.sum((0, 1, 2)), (d * xhat).sum((0, 1, 2))
            M = B * H * W
            g_x = gamma * invstd * (d - g_beta / M - xhat * (g_gamma / M) if training else d)
        return (g_x, g_gamma.to(gamma.dtype).reshape(gamma.shape), g_beta.to(beta.dtype).reshape(beta.shape)) + (None,) * 7


def _dw_forward_torch(x, w, mode):
    xc = to_nchw(x)
    if mode == L.DW_SAME:
        y = F.conv2d(to_nchw(pad_circular_nhwc(x)), w, groups=x.shape[-1])
    elif mode == L.DW_DOWN:
        y = F.conv2d(xc, w, stride=2, groups=x.shape[-1])
    else:
        y = F.conv_transpose2d(xc, w, stride=2, groups=x.shape[-1])
    return y.permute(0, 2, 3, 1).contiguous()


def _dw_backward_torch(g, x, w, mode, need_x, need_w):
    """The hand-derived backward of the three modes on [B, H, W, C] tensors -> (g_x, g_w): the data gradient gathered (the 3x3
    over g with flipped taps; the stride-2 modes each other's adjoints), the weight gradient a sum over batch and pixels."""
    B, H, W, C = x.shape
    g_x = g_w = None
    if mode == L.DW_SAME:
        if need_x:
            g_x = F.conv2d(to_nchw(pad_circular_nhwc(g)), w.flip(2, 3), groups=C).permute(0, 2, 3, 1)
        if need_w:
            patches = pad_circular_nhwc(x).unfold(1, 3, 1).unfold(2, 3, 1)                   # [B, H, W, C, kh, kw]
            g_w = torch.einsum("bhwc,bhwckl->ckl", g, patches).reshape(w.shape)
        return g_x, g_w
    k = w.reshape(C, 2, 2)
    if mode == L.DW_DOWN:                                                                     # x6 [b, i, a, j, k, c]
        if need_x:
            g_x = torch.einsum("bijc,cak->biajkc", g, k).reshape(B, H, W, C)
        if need_w:
            g_w = torch.einsum("bijc,biajkc->cak", g, x.reshape(B, H // 2, 2, W // 2, 2, C)).reshape(w.shape)
        return g_x, g_w
    g6 = g.reshape(B, H, 2, W, 2, C)
    if need_x:
        g_x = torch.einsum("biajkc,cak->bijc", g6, k)
    if need_w:
        g_w = torch.einsum("biajkc,bijc->cak", g6, x).reshape(w.shape)
    return g_x, g_w


class _DwConvFn(torch.autograd.Function):
    """y = the depthwise conv of x [B, H, W, C] with w [C, 1, k, k]; no bias, no activation (a BatchNorm follows)."""

    @staticmethod
    def forward(ctx, x, w, mode):
        ctx.save_for_backward(x, w)
        ctx.mode = mode
        if x.dtype in _IO16:
            if x.is_cuda:
                return ops.dwconv_train_forward_io(x, w, mode)
            with _fp32_math(x):                                # the taps rounded to x's dtype: autocast casts a conv weight
                return _dw_forward_torch(x.float(), w.to(x.dtype).float(), mode).to(x.dtype)
        if x.is_cuda:
            return ops.dwconv_train_forward(x.float(), w, mode)
        return _dw_forward_torch(x, w, mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[:2]
        if x.dtype in _IO16:
            if g.is_cuda:
                g_x, g_w = ops.dwconv_train_backward_io(_dense(g.to(x.dtype)), x, w, ctx.mode, need_x, need_w)
            else:
                with _fp32_math(x):
                    g_x, g_w = _dw_backward_torch(g.float(), x.float(), w.to(x.dtype).float(), ctx.mode, need_x, need_w)
                g_x = g_x.to(x.dtype) if need_x else None
        elif g.is_cuda:
            g_x, g_w = ops.dwconv_train_backward(_dense(g.float()), x.float(), w, ctx.mode, need_x, need_w)
        else:
            g_x, g_w = _dw_backward_torch(g, x, w, ctx.mode, need_x, need_w)
        return g_x, g_w.to(w.dtype) if need_w else None, None


class _SeScaleFn(torch.autograd.Function):
    """y = x * gate[b, c] (misc.py:30);  g_x = g * gate,  g_gate[b, c] = sum_hw g * x."""

    @staticmethod
    def forward(ctx, x, gate):
        ctx.save_for_backward(x, gate)
        ctx.hip = x.is_cuda and ops.bn_act_train_supported(x.shape[-1])
        if x.dtype in _IO16:
            if ctx.hip:
                return ops.se_scale_forward_io(x, gate)
            with _fp32_math(x):
                return (x.float() * gate.float().reshape(gate.shape[0], 1, 1, -1)).to(x.dtype)
        if ctx.hip:
            return ops.se_scale_forward(x.float(), gate)
        return x * gate.reshape(gate.shape[0], 1, 1, -1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, gate = ctx.saved_tensors
        if x.dtype in _IO16:
            if ctx.hip:
                g_x, g_gate = ops.se_scale_backward_io(_dense(g.to(x.dtype)), x, gate)
            else:
                with _fp32_math(x):
                    gf = g.float()
                    g_x = (gf * gate.float().reshape(gate.shape[0], 1, 1, -1)).to(x.dtype)
                    g_gate = (gf * x.float()).sum((1, 2))
        elif ctx.hip:
            g_x, g_gate = ops.se_scale_backward(_dense(g.float()), x.float(), gate)
        else:
            g_x, g_gate = g * gate.reshape(gate.shape[0], 1, 1, -1), (g * x).sum((1, 2))
        return g_x, g_gate.to(gate.dtype)


# ---- functional ops ------------------------------------------------------------------------------------------------------
def bn_act(x, bn, silu=False, want_pool=False):
    """nn.BatchNorm2d `bn` (+ SiLU) on x [B, H, W, C] as ONE node -> y, or (y, pool [B, C] = sum_hw y) with want_pool.  In
    bn.training the batch statistics normalise and bn.running_mean / running_var / num_batches_tracked are updated in place, as
    torch does; otherwise the running statistics normalise and no buffer is touched."""
    if bn.momentum is None:
        raise NotImplementedError("BatchNorm2d(momentum=None), the cumulative average, is not implemented (batchnorm2d.yaml: 0.1)")
    if not (bn.affine and bn.track_running_stats):
        raise NotImplementedError("BatchNorm2d must be affine with running statistics (batchnorm2d.yaml)")
    y, pool = _BnActFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training, float(bn.momentum),
                             float(bn.eps), bool(silu), bool(want_pool))
    if x.is_cuda:
        fused = ops.bn_act_train_supported(x.shape[-1])
        stats["bn_hip" if fused else "bn_fallbacks"] += 1
        _count16(x, fused)
    if bn.training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return (y, pool) if want_pool else y


def dwconv(x, w, mode):
    """The depthwise conv of branch[3] on x [B, H, W, C]: mode "same" / "out" 3x3 circular, "down" 2x2 stride 2, "up"
    ConvTranspose 2x2 stride 2; w the module's own [C, 1, k, k].  ONE node where the kernels take the shape
    (ops.dwconv_train_supported) and on CPU tensors of such a shape; F.conv2d(groups=C) / F.conv_transpose2d otherwise."""
    m = DW_MODES[mode] if isinstance(mode, str) else int(mode)
    B, H, W, C = x.shape
    if x.is_cuda:
        fused = ops.dwconv_train_supported(C, H, W, m)
        stats["dwconv_hip" if fused else "dwconv_fallbacks"] += 1
        _count16(x, fused)
    else:
        fused = m != L.DW_DOWN or (H % 2 == 0 and W % 2 == 0)
    if fused:
        return _DwConvFn.apply(x, w, m)
    if x.dtype in _IO16:
        with _fp32_math(x):
            return _dw_forward_torch(x.float(), w.to(x.dtype).float(), m).to(x.dtype)
    return _dw_forward_torch(x, w, m)


def se_scale(x, gate):
    """x [B, H, W, C] * gate [B, C] as ONE node; a 16-bit x takes the gate in fp32 or in its own dtype."""
    _count16(x, ops.bn_act_train_supported(x.shape[-1]) if x.is_cuda else False)
    return _SeScaleFn.apply(x, gate)


# ---- blocks and the model ------------------------------------------------------------------------------------------------
def _conv(t, w, stride=1):
    return to_nhwc(F.conv2d(to_nchw(t), w, stride=stride))


def _skip(block, x):
    w, mode = block.skip_conv.weight, block.mode
    if mode == "same":
        return _conv(x, w)
    if mode == "out":
        return _conv(pad_circular_nhwc(x), w)
    if mode == "down":
        return _conv(x, w, stride=2)
    return to_nhwc(F.conv_transpose2d(to_nchw(x), w, stride=2))


def block_forward_nhwc(block, x):
    """conv_block.py:316-321 on [B, H, W, C] with a graph: the three fused nodes around F.conv2d.  Each BatchNorm follows its
    own module's `.training`."""
    if not isinstance(block, _MBConvMirror):
        raise NotImplementedError(f"train_mbconv trains MBConv blocks only (vqae_amd.train has the Fixup ones), not "
                                  f"{type(block).__name__}")
    b = block.branch
    t = bn_act(_conv(x, b[0].weight), b[1], silu=True)
    t = dwconv(t, b[3].weight, block.mode)
    t, pool = bn_act(t, b[4], silu=True, want_pool=True)
    gate = b[6].fc(pool / (t.shape[1] * t.shape[2]))                    # misc.py:27-28: two Linear on [B, e], SiLU, sigmoid
    t = se_scale(t, gate)
    t = bn_act(_conv(t, b[7].weight), b[8])
    return t + (x if block.skip_conv is None else _skip(block, x))


def block_forward(block, x):
    """One MBConv mirror on an NCHW-shaped tensor (channels_last preferred: no copy) -> NCHW-shaped, with a graph.  Under 16-bit
    autocast an x of the autocast dtype (the residual stream of the stack) is taken as it is."""
    if x.dtype not in _IO16 or autocast16(x) != x.dtype:
        x = _compute_dtype(x)
    return to_nchw(block_forward_nhwc(block, to_nhwc(x)))


def block_forward_torch(block, x):
    """The same block written with stock torch ops only (F.batch_norm, F.silu, F.conv2d(groups=), the SE multiply), NCHW-shaped
    in and out, autograd's own backward: the yardstick of the tests and of tools/bench_mbconv_train.py.  No training path calls
    it.  Like nn.BatchNorm2d it updates the running statistics of a block in train mode."""
    b, e = block.branch, block.expanded

    def bn(t, m):
        if m.training:
            m.num_batches_tracked.add_(1)
        return F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, m.training, m.momentum, m.eps)

    t = F.silu(bn(F.conv2d(x, b[0].weight), b[1]))
    if block.mode in ("same", "out"):
        t = F.conv2d(F.pad(t, (1, 1, 1, 1), mode="circular"), b[3].weight, groups=e)
    elif block.mode == "down":
        t = F.conv2d(t, b[3].weight, stride=2, groups=e)
    else:
        t = F.conv_transpose2d(t, b[3].weight, stride=2, groups=e)
    t = F.silu(bn(t, b[4]))
    t = t * b[6].fc(t.mean((2, 3))).reshape(t.shape[0], e, 1, 1)
    t = bn(F.conv2d(t, b[7].weight), b[8])
    if block.skip_conv is None:
        return t + x
    w = block.skip_conv.weight
    if block.mode == "up":
        return t + F.conv_transpose2d(x, w, stride=2)
    if block.mode == "out":
        return t + F.conv2d(F.pad(x, (1, 1, 1, 1), mode="circular"), w)
    return t + F.conv2d(x, w, stride=2 if block.mode == "down" else 1)


def _blocks(model):
    enc, dec = model.encoder, model.decoder
    pre = [blk for level in enc.down_layers[0].layers for blk in level.layers] + list(enc.pre_enc_layers[0])
    post = list(dec.post_enc_layers[0]) + [blk for level in dec.up_layers[0].layers for blk in level.layers]
    return pre, post


def forward_train(model, x, return_indices=False, conv3x3z="torch"):
    """VQAE.forward (vq_ae/model.py:41-48) over a vqae_amd.model.VQAE mirror of an MBConv spec, with a graph: -> (out,
    (vq_loss,)), out NCHW-shaped (channels_last).  The stems are F.conv2d (conv3x3z = "hip": train.py's fused zero-padded
    node), the blocks block_forward_nhwc, the quantiser its own trainable mirror."""
    hip = train.conv_routes(conv3x3z=conv3x3z)
    enc, dec = model.encoder, model.decoder
    pre, post = _blocks(model)
    for blk in pre + post:
        if not isinstance(blk, _MBConvMirror):
            raise NotImplementedError(f"train_mbconv.forward_train trains MBConv models only (vqae_amd.train has the Fixup "
                                      f"ones), not {type(blk).__name__}")
    h = to_nhwc(_compute_dtype(x))
    h = train._pre_conv("conv3x3z", hip, h, None, None, enc.in_stem.weight, enc.in_stem.bias)
    for blk in pre:
        h = block_forward_nhwc(blk, h)
    vq = enc.vq_layers[0]
    h = h.float()                           # the quantiser is fp32 under autocast too (cdist); a no-op on an fp32 tensor
    q, idx, vq_loss = vq(to_nchw(h)) if h.is_cuda else train._quantize_torch(vq, to_nchw(h))
    h = to_nhwc(q)
    for blk in post:
        h = block_forward_nhwc(blk, h)
    out = to_nchw(train._pre_conv("conv3x3z", hip, h, None, None, dec.out_stem.weight, dec.out_stem.bias))
    if return_indices:
        return out, (vq_loss,), (idx,)
    return out, (vq_loss,)


def step(model, batch, loss_f=F.huber_loss, conv3x3z="torch"):
    """VQAE.step (vq_ae/model.py:114-122): -> (out, recon_loss, (vq_loss,)); the caller backpropagates recon_loss +
    sum(vq_loss)."""
    out, encoding_loss = forward_train(model, batch, conv3x3z=conv3x3z)
    return out, loss_f(input=out, target=batch), encoding_loss
