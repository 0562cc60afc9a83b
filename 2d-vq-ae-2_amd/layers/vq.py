"""Drop-in mirrors of vq_ae.layers.vq.{EMAVectorQuantizer, ProjectedEMAVectorQuantizer2d}
(reference vq_ae/layers/vq.py:6-154, 157-192) backed by libvqae_hip.so.

Same constructor kwargs, buffer names (embed / embed_avg / cluster_size / first_pass, vq.py:27-34),
forward contract `(quantized, encoding_indices, loss)` ("don't change this order", vq.py:148-154) and
exception types.  Select through Hydra with
    _target_: vqae_amd.layers.vq.EMAVectorQuantizer

Gradients.  When grad mode is on and the input (or, for the projected form, a projection parameter) requires grad, the
forward runs inside a torch.autograd.Function: the same launches in the same order (values, indices, loss and the EMA
buffers are bit-equal to the no-grad call), plus the rows the backward needs -- x, z = proj_in(x) and q, the lookup in the
codebook as it was BEFORE the training-mode EMA update rewrote `embed` in place.  The backward is the closed form of what
autograd derives from vq.py:143-146 (and :190-192), in HIP (csrc/vq_backward.hip):
    plain       g_x = g_out + s (x - q),                      s = g_loss * commitment_cost * 2 / (N * D)
    projected   g_q = g_out W_out,  g_z = g_q + s (z - q),    g_x = g_z W_in,
                g_W_out = g_out^T q,  g_b_out = sum_n g_out,  g_W_in = g_z^T x,  g_b_in = sum_n g_z
Nothing flows into the codebook (a buffer, updated by EMA).  The Functions are once-differentiable.  Autocast: the mirrors
compute in fp32 whatever the input dtype, so the gradient is the fp32 one, cast back to the dtype of each input.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops


def fused_all_reduce_stats(counts, dw):
    """`all_reduce(new_cluster_size)` + `all_reduce(dw)` of _update_ema (vq.py:57-58) as ONE all-reduce of the flat
    [K] + [K * D] buffer (latency-bound messages: 1 KB + 8..128 KB).  Element-wise SUM: fusing changes no element's
    reduction, only the number of collectives (tests/test_driver_cpu.py checks equality under 2 ranks)."""
    flat = torch.cat([counts.reshape(-1), dw.reshape(-1)])
    torch.distributed.all_reduce(flat)
    return flat[: counts.numel()].reshape_as(counts), flat[counts.numel():].reshape_as(dw)


def backward_reference(g_out, x, q, g_loss, commitment_cost):
    """The plain quantiser's input gradient on channel-last rows, in torch ops of the arguments' device and dtype:
    g_out [N, D] | None, x, q [N, D], g_loss 0-d | None -> g_x [N, D]."""
    g_x = torch.zeros_like(x) if g_out is None else g_out.clone()
    if g_loss is not None:
        g_x = g_x + (g_loss * (commitment_cost * 2.0 / max(x.numel(), 1))) * (x - q)
    return g_x


def projected_backward_reference(g_out, x, z, q, g_loss, commitment_cost, w_in, w_out):
    """The projected quantiser's five gradients composed from torch matmuls (any device, any dtype): the yardstick of the
    fused kernel and the backward of the shapes it does not take (projection_dim != 8, channels % 4 != 0 or > 256).
    g_out [N, C] | None, x [N, C], z = x w_in^T + b_in and q = embed[idx] [N, P], g_loss 0-d | None, w_in [P, C],
    w_out [C, P]  ->  (g_x [N, C], g_w_in [P, C], g_b_in [P], g_w_out [C, P], g_b_out [C])."""
    if g_out is None:
        g_out = torch.zeros_like(x)
    g_z = g_out @ w_out
    g_w_out = g_out.t() @ q
    g_b_out = g_out.sum(0)
    if g_loss is not None:
        g_z = g_z + (g_loss * (commitment_cost * 2.0 / max(z.numel(), 1))) * (z - q)
    return g_z @ w_in, g_z.t() @ x, g_z.sum(0), g_w_out, g_b_out


def _channel_last(t, ndim):
    """[B, D, ...] fp32 -> contiguous [B, ..., D] (vq.py:107-113)."""
    return ops.nchw_to_nhwc(t) if ndim == 4 else t.permute(0, *range(2, ndim), 1).contiguous()


def _channel_first(t, ndim):
    return ops.nhwc_to_nchw(t) if ndim == 4 else t.permute(0, -1, *range(1, ndim - 1)).contiguous()


class _QuantizeFn(torch.autograd.Function):
    """EMAVectorQuantizer.forward with the straight-through / commitment gradient of vq.py:143-146."""

    @staticmethod
    def forward(ctx, inputs, module):
        quantized, idx, loss, flat_input, q_flat = module._forward_values(inputs)
        ctx.save_for_backward(flat_input, q_flat)
        ctx.commitment_cost = module.commitment_cost
        ctx.in_dtype, ctx.in_shape = inputs.dtype, tuple(inputs.shape)
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        return quantized, idx, loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_idx, g_loss):
        if g_out is None and g_loss is None:
            return None, None
        flat_input, q_flat = ctx.saved_tensors
        shape, ndim = ctx.in_shape, len(ctx.in_shape)
        g_flat = _channel_last(g_out.float(), ndim).reshape(flat_input.shape) if g_out is not None else None
        g_x = ops.vq_backward(g_flat, flat_input, q_flat, g_loss, ctx.commitment_cost)
        g_x = _channel_first(g_x.reshape(shape[0], *shape[2:], shape[1]), ndim)
        return g_x.to(ctx.in_dtype), None


class _ProjectedQuantizeFn(torch.autograd.Function):
    """ProjectedEMAVectorQuantizer2d.forward with the gradients of vq.py:190-192 around vq.py:143-146."""

    @staticmethod
    def forward(ctx, inputs, w_in, b_in, w_out, b_out, module):
        out, idx, loss, (x_flat, z, q) = module._forward_values(inputs, save=True)
        ctx.save_for_backward(x_flat, z, q, w_in, w_out)
        ctx.commitment_cost = module.commitment_cost
        ctx.dtypes = (inputs.dtype, w_in.dtype, b_in.dtype, w_out.dtype, b_out.dtype)
        ctx.in_shape = tuple(inputs.shape)
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        return out, idx, loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_idx, g_loss):
        if g_out is None and g_loss is None:
            return (None,) * 6
        x_flat, z, q, w_in, w_out = ctx.saved_tensors
        (N, C), P = x_flat.shape, z.shape[1]
        B, _, H, W = ctx.in_shape
        g_flat = ops.nchw_to_nhwc(g_out.float()).reshape(N, C) if g_out is not None else None
        want = tuple(ctx.needs_input_grad[:5])
        if P == 8 and C % 4 == 0 and C <= 256:
            grads = ops.vq_projected_backward(g_flat, x_flat, z, q, g_loss, w_in, w_out, ctx.commitment_cost, want)
        else:                                                       # the shapes the fused kernel does not take
            grads = projected_backward_reference(g_flat, x_flat, z, q, g_loss, ctx.commitment_cost,
                                                 w_in.detach().reshape(P, C).float(), w_out.detach().reshape(C, P).float())
        g_x, g_w_in, g_b_in, g_w_out, g_b_out = (g if on else None for g, on in zip(grads, want))
        if g_x is not None:
            g_x = ops.nhwc_to_nchw(g_x.reshape(B, H, W, C))
        if g_w_in is not None:
            g_w_in = g_w_in.reshape(w_in.shape)
        if g_w_out is not None:
            g_w_out = g_w_out.reshape(w_out.shape)
        grads = (g_x, g_w_in, g_b_in, g_w_out, g_b_out)
        return tuple(g.to(dt) if g is not None else None for g, dt in zip(grads, ctx.dtypes)) + (None,)


class EMAVectorQuantizer(nn.Module):
    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float, decay: float,
                 laplace_alpha: float):
        super().__init__()
        embed = torch.randn(num_embeddings, embedding_dim)
        self.register_buffer("embed", embed)                       # e_i   (vq.py:27)
        self.register_buffer("embed_avg", embed.clone())           # m_i   (vq.py:28)
        self.register_buffer("cluster_size", torch.zeros(num_embeddings))  # N_i (vq.py:29)
        self.register_buffer("first_pass", torch.as_tensor(1))     # vq.py:33
        self.commitment_cost = commitment_cost
        self.decay = decay
        self.laplace_alpha = laplace_alpha
        self.embedding_dim = embedding_dim
        self.num_embeddings = num_embeddings

    def embed_code(self, embed_idx):                               # vq.py:44-45
        return ops.embed_code(embed_idx, self.embed)

    # ---- training-mode bookkeeping (vq.py:47-94) ------------------------------------------------
    @torch.no_grad()
    def _update_ema(self, flat_input, encoding_indices):
        counts, dw = ops.vq_code_stats(flat_input, encoding_indices, self.num_embeddings)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            counts, dw = fused_all_reduce_stats(counts, dw)
        ops.vq_ema_update(self.embed, self.embed_avg, self.cluster_size, counts.contiguous(), dw.contiguous(),
                          self.decay, self.laplace_alpha)

    @torch.no_grad()
    def _init_ema(self, flat_input):
        mean = flat_input.mean(dim=0)
        std = flat_input.std(dim=0)
        cluster_size = flat_input.size(dim=0)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            ws = torch.distributed.get_world_size()
            both = torch.stack([mean, std])
            torch.distributed.all_reduce(both)                     # vq.py:82-87 (mean of per-rank stds, sic)
            mean, std = both[0] / ws, both[1] / ws
            cluster_size *= ws
        self.embed.mul_(std)
        self.embed.add_(mean)
        self.embed_avg.copy_(self.embed)
        self.cluster_size.data.add_(cluster_size / self.num_embeddings)
        self.first_pass.mul_(0)

    def forward(self, inputs):
        ndim = inputs.dim()
        assert ndim >= 3                                           # vq.py:98
        if inputs.shape[1] != self.embedding_dim:                  # vq.py:100-104
            raise NotImplementedError(
                'VQ dim != channel dim not supported;'
                f' found channel dim of {inputs.shape[1]}, expected {self.embedding_dim}')
        if ndim > 5:
            # the reference's distance exponent is p = inputs.dim() (vq.py:121-129); the kernels implement p = 3, 4, 5
            raise NotImplementedError(f'inputs of rank 3 .. 5 (p = 3, 4, 5) are implemented; got a {ndim}-D input')
        if torch.is_grad_enabled() and inputs.requires_grad:
            return _QuantizeFn.apply(inputs, self)
        return self._forward_values(inputs)[:3]

    def _forward_values(self, inputs):
        """-> (quantized, encoding_indices, loss, flat_input, q_flat); the last two are the rows the backward keeps."""
        ndim = inputs.dim()
        with torch.no_grad():
            x = inputs.detach().float()
            if ndim == 4:
                cl = ops.nchw_to_nhwc(x)
            else:                                                      # channel last (vq.py:107-113): [B, L, D] / [B, d, h, w, D]
                cl = x.permute(0, *range(2, ndim), 1).contiguous()
            D = cl.shape[-1]
            flat_input = cl.reshape(-1, D)
            if self.first_pass and self.training:
                self._init_ema(flat_input)
            q_flat, idx, loss, _ = ops.vq_forward(flat_input, self.embed, self.commitment_cost, p=ndim)
            if self.training:
                self._update_ema(flat_input, idx)
            q_cl = q_flat.reshape(cl.shape)                             # = inputs + (q - inputs), vq.py:146
            quantized = ops.nhwc_to_nchw(q_cl) if ndim == 4 else q_cl.permute(0, -1, *range(1, ndim - 1)).contiguous()
            encoding_indices = idx.reshape(cl.shape[:-1])
        return quantized, encoding_indices, loss, flat_input, q_flat


class ProjectedEMAVectorQuantizer2d(EMAVectorQuantizer):
    """proj_out(VQ(proj_in(x))) with 1x1 convs (vq.py:157-192)."""

    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float, decay: float,
                 laplace_alpha: float, projection_dim: int):
        super().__init__(num_embeddings, projection_dim, commitment_cost, decay, laplace_alpha)
        self.proj_in = nn.Conv2d(embedding_dim, projection_dim, kernel_size=1)     # parameter holders
        self.proj_out = nn.Conv2d(projection_dim, embedding_dim, kernel_size=1)
        self._packed = None

    def _weights(self):
        key = (self.proj_in.weight._version, self.proj_out.weight._version, self.proj_in.weight.device)
        if self._packed is None or self._packed[0] != key:
            self._packed = (key, ops.pack_conv_weight(self.proj_in.weight.detach()),
                            ops.pack_conv_weight(self.proj_out.weight.detach()))
        return self._packed[1], self._packed[2]

    def forward(self, inputs):
        assert inputs.dim() == 4
        params = (self.proj_in.weight, self.proj_in.bias, self.proj_out.weight, self.proj_out.bias)
        if torch.is_grad_enabled() and (inputs.requires_grad or any(p.requires_grad for p in params)):
            return _ProjectedQuantizeFn.apply(inputs, *params, self)
        return self._forward_values(inputs)[:3]

    def _forward_values(self, inputs, save=False):
        """-> (out, encoding_indices, loss, saved); saved = (x [N, C], z [N, P], q [N, P]) for the backward when `save`,
        q being the lookup in `embed` as it is before _update_ema rewrites it."""
        if self.embedding_dim == 8 and not self.training:
            # eval mode, the reference default projection_dim: one fused launch (csrc/vq_proj.hip)
            with torch.no_grad():
                x = ops.nchw_to_nhwc(inputs.detach().float())
                B, H, W, C = x.shape
                out, idx, loss, z, _ = ops.vq_projected(x.reshape(-1, C), self.proj_in.weight.detach(), self.proj_in.bias.detach(),
                                                        self.embed, self.proj_out.weight.detach(), self.proj_out.bias.detach(),
                                                        self.commitment_cost, want_z=save)
                saved = (x.reshape(-1, C), z, ops.embed_code(idx, self.embed)) if save else None
                return ops.nhwc_to_nchw(out.reshape(B, H, W, C)), idx.reshape(B, H, W), loss, saved
        w_in, w_out = self._weights()
        with torch.no_grad():
            x = ops.nchw_to_nhwc(inputs.detach().float())
            z = ops.conv2d(x, w_in, self.embedding_dim, 1, bias_vec=self.proj_in.bias.detach())
            B, H, W, D = z.shape
            flat = z.reshape(-1, D)
            if self.first_pass and self.training:
                self._init_ema(flat)
            q_flat, idx, loss, _ = ops.vq_forward(flat, self.embed, self.commitment_cost)
            if self.training:
                self._update_ema(flat, idx)
            out = ops.conv2d(q_flat.reshape(B, H, W, D), w_out, self.proj_out.out_channels, 1,
                             bias_vec=self.proj_out.bias.detach())
            saved = (x.reshape(-1, x.shape[-1]), flat, q_flat) if save else None
            return ops.nhwc_to_nchw(out), idx.reshape(B, H, W), loss, saved
