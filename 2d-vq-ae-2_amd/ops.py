"""Functional wrappers over the C ABI for torch tensors living in HBM (plumbing only: pointers,
shapes, the current HIP stream).  Activations are NHWC fp32 unless a name says otherwise."""
import ctypes
import functools
import types

import torch

from . import _lib as L

_IDX_DTYPES = {torch.int64: L.IDX_I64, torch.uint8: L.IDX_U8, torch.int32: L.IDX_I32}
if hasattr(torch, "uint16"):
    _IDX_DTYPES[torch.uint16] = L.IDX_U16


MEAN = (0.7279, 0.5955, 0.7762)      # conf/transforms/camelyon16_transforms.yaml:15-23
STD = (0.2419, 0.3083, 0.1741)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.VqaeHipError("libvqae_hip ops need tensors in HBM (device='cuda'); there is no CPU fallback")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def idx_code(dtype):
    try:
        return _IDX_DTYPES[dtype]
    except KeyError:
        raise AssertionError(f"unsupported index dtype {dtype}")


def nchw_to_nhwc(x):
    _need_gpu(x)
    x = x.contiguous()
    B, C, H, W = x.shape
    y = torch.empty((B, H, W, C), dtype=torch.float32, device=x.device)
    L.check(L.lib().vqae_nchw_to_nhwc_f32(_p(x), B, C, H, W, _p(y), _stream()))
    return y


def nhwc_to_nchw(x):
    _need_gpu(x)
    x = x.contiguous()
    B, H, W, C = x.shape
    y = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    L.check(L.lib().vqae_nhwc_to_nchw_f32(_p(x), B, C, H, W, _p(y), _stream()))
    return y


def pack_conv_weight(w, dtype=None):
    """[cout][cin][k][k] (PyTorch) -> the MFMA kernel's packed layout; `dtype` ('bf16'/'f16') rounds the
    weights to that type (autocast casts conv weights)."""
    _need_gpu(w)
    w = w.contiguous().float()
    cout, cin, k, _ = w.shape
    n = L.lib().vqae_conv_packed_floats(cout, cin, k)
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    L.check(L.lib().vqae_conv_pack_weight_f32(_p(w), cout, cin, k, _p(out), _stream()))
    L.check(L.lib().vqae_round_inplace_f32(_p(out), n, L.dtype_code(dtype), _stream()))
    return out


def conv2d(x, w_packed, cout, ksize, stride=1, pad=0, pad_mode=L.PAD_NONE, pre=None, act=None, scale_bias=None,
           bias_s=None, bias_vec=None, residual=None, out=None, dtype=None, gate=None):
    """NHWC fp32 conv through vqae_conv2d_f32.  pre = (a,) or (a, b); act = (a, b) [ELU form] or 'silu';
    scale_bias = (s, b); gate [B, cin]: per-image channel gate applied while x is loaded (vqae_conv2d_gated_f32)."""
    _need_gpu(x, w_packed)
    x = x.contiguous()
    B, H, W, cin = x.shape
    a = L.ConvArgs()
    a.batch, a.in_h, a.in_w, a.cin, a.cout = B, H, W, cin, cout
    a.ksize, a.stride, a.pad, a.pad_mode = ksize, stride, pad, pad_mode
    a.dtype = L.dtype_code(dtype)
    if pre is not None:
        if len(pre) == 1:
            a.pre_mode, a.pre_a = L.PRE_BIAS, float(pre[0])
        else:
            a.pre_mode, a.pre_a, a.pre_b = L.PRE_BIAS_ELU_BIAS, float(pre[0]), float(pre[1])
    if isinstance(act, str):
        assert act == "silu", act
        a.has_act = L.ACT_SILU
    elif act is not None:
        a.has_act, a.act_a, a.act_b = L.ACT_ELU, float(act[0]), float(act[1])
    if scale_bias is not None:
        a.has_scale, a.scale, a.bias_s = 1, float(scale_bias[0]), float(scale_bias[1])
    elif bias_s is not None:
        a.has_bias_s, a.bias_s = 1, float(bias_s)
    Ho = (H + 2 * pad - ksize) // stride + 1
    Wo = (W + 2 * pad - ksize) // stride + 1
    if out is None:
        out = torch.empty((B, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    if gate is not None:
        assert pre is None and tuple(gate.shape) == (B, cin), (pre, gate.shape)
        _need_gpu(gate)
        a.pre_mode = L.PRE_CHANNEL_GATE
        L.check(L.lib().vqae_conv2d_gated_f32(ctypes.byref(a), _p(x), _p(gate.contiguous()), _p(w_packed), _p(bias_vec),
                                              _p(residual), _p(out), _stream()))
        return out
    L.check(L.lib().vqae_conv2d_f32(ctypes.byref(a), _p(x), _p(w_packed), _p(bias_vec), _p(residual), _p(out),
                                    _stream()))
    return out


def dwconv(x, w_taps, bias=None, mode=L.DW_SAME, silu=False, want_partial=False):
    """Depthwise conv on NHWC x [B,H,W,C]; w_taps [k*k, C].  mode: DW_SAME (3x3 circular), DW_DOWN (2x2 s2),
    DW_UP (ConvTranspose2d 2x2 s2).  -> y, or (y, strip partial sums) for se_gate."""
    _need_gpu(x, w_taps)
    x = x.contiguous()
    B, H, W, C = x.shape
    Ho, Wo = {L.DW_SAME: (H, W), L.DW_DOWN: (H // 2, W // 2), L.DW_UP: (2 * H, 2 * W)}[mode]
    y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    part = None
    if want_partial:
        part = torch.empty(int(L.lib().vqae_dw_partial_floats(B, Ho, Wo, C)), dtype=torch.float32, device=x.device)
    L.check(L.lib().vqae_dwconv_f32(_p(x), _p(w_taps.contiguous()), _p(bias), B, H, W, C, mode, int(silu), _p(y), _p(part),
                                    _stream()))
    return (y, part) if want_partial else y


def se_gate(partial, batch, out_h, out_w, fc0_w, fc0_b, fc2_w, fc2_b):
    """SELayer gate [B, C] from dwconv's strip sums (layers/misc.py:23-29)."""
    _need_gpu(partial, fc0_w, fc0_b, fc2_w, fc2_b)
    hidden, C = fc0_w.shape
    gate = torch.empty((batch, C), dtype=torch.float32, device=partial.device)
    L.check(L.lib().vqae_se_gate_f32(_p(partial), batch, out_h, out_w, C, _p(fc0_w.contiguous()), _p(fc0_b.contiguous()),
                                     hidden, _p(fc2_w.contiguous()), _p(fc2_b.contiguous()), _p(gate), _stream()))
    return gate


def pixel_shuffle2(x, c):
    """[B,H,W,4c] (a, b, c) -> [B,2H,2W,c]."""
    _need_gpu(x)
    x = x.contiguous()
    B, H, W, c4 = x.shape
    assert c4 == 4 * c
    y = torch.empty((B, 2 * H, 2 * W, c), dtype=torch.float32, device=x.device)
    L.check(L.lib().vqae_pixel_shuffle2_f32(_p(x), B, H, W, c, _p(y), _stream()))
    return y


def fixup_same_supported(c, h, w):
    return bool(L.lib().vqae_fixup_same_supported(c, h, w))


def fixup_same_block(x, w1p, w2p, w3p, scalars8, dtype=None):
    """Whole 'same' Fixup block in one launch (x NHWC [B,H,W,C]); scalars8 = (b1a,b1b,b2a,b2b,b3a,b3b,b4,scale)."""
    _need_gpu(x, w1p, w2p, w3p)
    x = x.contiguous()
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    sc = (ctypes.c_float * 8)(*[float(v) for v in scalars8])
    L.check(L.lib().vqae_fixup_same_block_f32(_p(x), _p(y), _p(w1p), _p(w2p), _p(w3p), B, H, W, C, sc,
                                              L.dtype_code(dtype), _stream()))
    return y


def conv3x3_direct(x, w, bias, x_u8=None, mean255=None, inv_std255=None, dtype=None):
    """Stem conv (3x3, zero pad, bias); x NHWC fp32 or x_u8 NHWC uint8 (normalised on device)."""
    src = x if x_u8 is None else x_u8
    _need_gpu(src, w, bias)
    src = src.contiguous()
    B, H, W, cin = src.shape
    cout = w.shape[0]
    y = torch.empty((B, H, W, cout), dtype=torch.float32, device=src.device)
    m = (ctypes.c_float * 3)(*mean255) if mean255 is not None else None
    s = (ctypes.c_float * 3)(*inv_std255) if inv_std255 is not None else None
    L.check(L.lib().vqae_conv3x3_direct_f32(_p(x) if x_u8 is None else None, _p(x_u8) if x_u8 is not None else None,
                                            m, s, _p(w.contiguous()), _p(bias.contiguous()), B, H, W, cin, cout,
                                            _p(y), L.dtype_code(dtype), _stream()))
    return y


def bicubic_up2(x, pre_bias=0.0):
    _need_gpu(x)
    x = x.contiguous()
    B, H, W, C = x.shape
    y = torch.empty((B, 2 * H, 2 * W, C), dtype=torch.float32, device=x.device)
    L.check(L.lib().vqae_bicubic_up2_f32(_p(x), B, H, W, C, float(pre_bias), _p(y), _stream()))
    return y


def _scalar(p):
    """A one-element parameter as the kernels read it: one fp32 in HBM (no copy for an fp32 Parameter); never read back."""
    if p is None:
        return None
    _need_gpu(p)
    return p.detach().reshape(-1)[:1].float().contiguous()


def _train_ws(n, dev):
    return torch.empty(L.lib().vqae_fixup_train_workspace_bytes(int(n)), dtype=torch.uint8, device=dev)


_IO_DTYPES = {torch.float32: L.DT_F32, torch.bfloat16: L.DT_BF16, torch.float16: L.DT_F16}


def _need_f32(who, **tensors):
    """The fp32 entry points read 4 bytes per element: a tensor of another dtype never reaches them (before any device call)."""
    for name, t in tensors.items():
        assert t is None or t.dtype == torch.float32, f"{who}: {name} is {t.dtype}; the fp32 op takes fp32 tensors (see {who}_io)"


def _io_code(who, name, dtype):
    try:
        return _IO_DTYPES[dtype]
    except KeyError:
        raise AssertionError(f"{who}: {name} is {dtype}; fp32, bf16 and f16 are taken")


def fixup_act(x, a, b, halo=0):
    """y = ELU(x + a) + b on x [B, H, W, C]; a, b one-element device tensors; a None: the plain mode y = x + b.
    halo = 1: y [B, H + 2, W + 2, C] with the circular wrap written (= F.pad(y, (1, 1, 1, 1), 'circular') in NCHW terms)."""
    _need_gpu(x)
    x = x.contiguous()
    B, H, W, C = x.shape
    y = torch.empty((B, H + 2 * halo, W + 2 * halo, C), dtype=torch.float32, device=x.device)
    L.check(L.lib().vqae_fixup_act_f32(_p(x), _p(_scalar(a)), _p(_scalar(b)), int(a is not None), int(halo), B, H, W, C, _p(y),
                                       _stream()))
    return y


def fixup_act_backward(g, x, a, halo=0, act=True):
    """-> (g_x [B, H, W, C], g_a [1], g_b [1]) from g (with the halo when halo = 1) and the forward's x and a.  Plain mode
    (act False; x, a unused): (g, None, g_b) -- the input gradient is the incoming tensor itself."""
    _need_f32("fixup_act_backward", g=g, x=x if act else None)
    _need_gpu(g)
    g = g.contiguous()
    B, H, W, C = g.shape[0], g.shape[1] - 2 * halo, g.shape[2] - 2 * halo, g.shape[3]
    dev = g.device
    g_b = torch.empty(1, dtype=torch.float32, device=dev)
    ws = _train_ws(g.numel(), dev)
    if not act:
        L.check(L.lib().vqae_fixup_act_backward_f32(_p(g), None, None, 0, 0, B, H, W, C, None, None, _p(g_b), _p(ws), _stream()))
        return g, None, g_b
    x = x.contiguous()
    assert tuple(x.shape) == (B, H, W, C), (x.shape, g.shape)
    g_x = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)
    g_a = torch.empty(1, dtype=torch.float32, device=dev)
    L.check(L.lib().vqae_fixup_act_backward_f32(_p(g), _p(x), _p(_scalar(a)), 1, int(halo), B, H, W, C, _p(g_x), _p(g_a), _p(g_b),
                                                _p(ws), _stream()))
    return g_x, g_a, g_b


def fixup_out(t, skip, scale, bias4, bias1d=None):
    """y = (t * scale + bias4) + (skip [+ bias1d]) on equally shaped dense tensors; the scalars are one-element device tensors."""
    _need_gpu(t, skip)
    t, skip = t.contiguous(), skip.contiguous()
    assert t.shape == skip.shape, (t.shape, skip.shape)
    y = torch.empty_like(t)
    L.check(L.lib().vqae_fixup_out_f32(_p(t), _p(skip), _p(_scalar(scale)), _p(_scalar(bias4)), _p(_scalar(bias1d)), t.numel(),
                                       _p(y), _stream()))
    return y


def fixup_out_backward(g, t, scale):
    """-> (g_t = g * scale, g_scale [1] = sum g t, g_bias [1] = sum g); the skip gradient is g itself."""
    _need_f32("fixup_out_backward", g=g, t=t)
    _need_gpu(g, t)
    g, t = g.contiguous(), t.contiguous()
    assert t.shape == g.shape, (t.shape, g.shape)
    dev = g.device
    g_t = torch.empty_like(g)
    g_scale, g_bias = (torch.empty(1, dtype=torch.float32, device=dev) for _ in range(2))
    ws = _train_ws(g.numel(), dev)
    L.check(L.lib().vqae_fixup_out_backward_f32(_p(g), _p(t), _p(_scalar(scale)), g.numel(), _p(g_t), _p(g_scale), _p(g_bias),
                                                None, _p(ws), _stream()))
    return g_t, g_scale, g_bias


def fixup_act_io(x, a, b, halo=0, out_dtype=torch.float32):
    """fixup_act with 16-bit I/O (csrc/fixup_train_io.hip): x fp32, bf16 or f16 -> y of `out_dtype` (fp32 or the same 16-bit
    type), bit for bit fixup_act(x.float(), a, b, halo).to(out_dtype) without the two casts."""
    dx, dy = _io_code("fixup_act_io", "x", x.dtype), _io_code("fixup_act_io", "out_dtype", out_dtype)
    _need_gpu(x)
    x = x.contiguous()
    B, H, W, C = x.shape
    y = torch.empty((B, H + 2 * halo, W + 2 * halo, C), dtype=out_dtype, device=x.device)
    L.check(L.lib().vqae_fixup_act_io(_p(x), dx, _p(_scalar(a)), _p(_scalar(b)), int(a is not None), int(halo), B, H, W, C,
                                      _p(y), dy, _stream()))
    return y


def fixup_act_backward_io(g, x, a, halo=0, act=True, x_dtype=None):
    """fixup_act_backward with 16-bit I/O: g in the forward's output dtype (with the halo when halo = 1), x as the forward
    read it -> (g_x in x's dtype, g_a [1], g_b [1]), g_a / g_b fp32 sums of the unrounded terms.  Plain mode (act False; x, a
    unused, x_dtype = the forward's input dtype): g_x is g itself where the dtypes agree, else g cast to x_dtype, written by
    the launch that sums it."""
    x_dtype = x.dtype if act else (g.dtype if x_dtype is None else x_dtype)
    dg, dx = _io_code("fixup_act_backward_io", "g", g.dtype), _io_code("fixup_act_backward_io", "x", x_dtype)
    _need_gpu(g, x if act else None)
    g = g.contiguous()
    B, H, W, C = g.shape[0], g.shape[1] - 2 * halo, g.shape[2] - 2 * halo, g.shape[3]
    dev = g.device
    g_b = torch.empty(1, dtype=torch.float32, device=dev)
    ws = _train_ws(g.numel(), dev)
    if not act:
        g_x = g if x_dtype == g.dtype else torch.empty(g.shape, dtype=x_dtype, device=dev)
        L.check(L.lib().vqae_fixup_act_backward_io(_p(g), dg, None, dx, None, 0, 0, B, H, W, C, None if g_x is g else _p(g_x),
                                                   None, _p(g_b), _p(ws), _stream()))
        return g_x, None, g_b
    x = x.contiguous()
    assert tuple(x.shape) == (B, H, W, C), (x.shape, g.shape)
    g_x = torch.empty((B, H, W, C), dtype=x_dtype, device=dev)
    g_a = torch.empty(1, dtype=torch.float32, device=dev)
    L.check(L.lib().vqae_fixup_act_backward_io(_p(g), dg, _p(x), dx, _p(_scalar(a)), 1, int(halo), B, H, W, C, _p(g_x), _p(g_a),
                                               _p(g_b), _p(ws), _stream()))
    return g_x, g_a, g_b


def fixup_out_io(t, skip, scale, bias4, bias1d=None, out_dtype=torch.float32):
    """fixup_out with 16-bit inputs: t and skip each fp32 or 16-bit -> y, the fp32 residual stream (any other out_dtype is
    refused by the library): bit for bit fixup_out(t.float(), skip.float(), ...)."""
    dt, ds = _io_code("fixup_out_io", "t", t.dtype), _io_code("fixup_out_io", "skip", skip.dtype)
    dy = _io_code("fixup_out_io", "out_dtype", out_dtype)
    _need_gpu(t, skip)
    t, skip = t.contiguous(), skip.contiguous()
    assert t.shape == skip.shape, (t.shape, skip.shape)
    y = torch.empty(t.shape, dtype=out_dtype, device=t.device)
    L.check(L.lib().vqae_fixup_out_io(_p(t), dt, _p(skip), ds, _p(_scalar(scale)), _p(_scalar(bias4)), _p(_scalar(bias1d)),
                                      t.numel(), _p(y), dy, _stream()))
    return y


def fixup_out_backward_io(g, t, scale, skip_dtype=torch.float32):
    """fixup_out_backward with 16-bit I/O: g fp32, t as the forward read it -> (g_t in t's dtype, g_skip, g_scale [1],
    g_bias [1]).  g_skip is g itself for an fp32 skip and g cast to a 16-bit skip_dtype, written in the same pass."""
    _need_f32("fixup_out_backward_io", g=g)
    dt, ds = _io_code("fixup_out_backward_io", "t", t.dtype), _io_code("fixup_out_backward_io", "skip_dtype", skip_dtype)
    _need_gpu(g, t)
    g, t = g.contiguous(), t.contiguous()
    assert t.shape == g.shape, (t.shape, g.shape)
    dev = g.device
    g_t = torch.empty_like(t)
    g_skip = g if skip_dtype == torch.float32 else torch.empty(g.shape, dtype=skip_dtype, device=dev)
    g_scale, g_bias = (torch.empty(1, dtype=torch.float32, device=dev) for _ in range(2))
    ws = _train_ws(g.numel(), dev)
    L.check(L.lib().vqae_fixup_out_backward_io(_p(g), _p(t), dt, _p(_scalar(scale)), g.numel(), _p(g_t),
                                               None if g_skip is g else _p(g_skip), ds, _p(g_scale), _p(g_bias), None, _p(ws),
                                               _stream()))
    return g_t, g_skip, g_scale, g_bias


def bicubic_up2_bias(x, pre_bias=None):
    """bicubic_up2 with pre_bias a one-element device tensor (or None) and any channel count."""
    _need_gpu(x)
    x = x.contiguous()
    B, H, W, C = x.shape
    y = torch.empty((B, 2 * H, 2 * W, C), dtype=torch.float32, device=x.device)
    L.check(L.lib().vqae_bicubic_up2_bias_f32(_p(x), B, H, W, C, _p(_scalar(pre_bias)), _p(y), _stream()))
    return y


def bicubic_up2_backward(g, want_bias=True):
    """The adjoint of bicubic_up2: g [B, 2H, 2W, C] -> (g_x [B, H, W, C], g_pre_bias [1] = sum g_x | None)."""
    _need_gpu(g)
    g = g.contiguous()
    B, OH, OW, C = g.shape
    assert OH % 2 == 0 and OW % 2 == 0, g.shape
    dev = g.device
    g_x = torch.empty((B, OH // 2, OW // 2, C), dtype=torch.float32, device=dev)
    g_pb = torch.empty(1, dtype=torch.float32, device=dev) if want_bias else None
    ws = _train_ws(g.numel(), dev)
    L.check(L.lib().vqae_bicubic_up2_backward_f32(_p(g), B, OH // 2, OW // 2, C, _p(g_x), _p(g_pb), _p(ws), _stream()))
    return g_x, g_pb


def _up_train_ws(B, H, W, C, dev):
    return torch.empty(L.lib().vqae_up_train_workspace_bytes(B, H, W, C), dtype=torch.uint8, device=dev)


def up2_act(t_low, a, b):
    """y [B, 2H, 2W, C] = ELU(bicubic_up2(t_low) + a) + b on t_low [B, H, W, C], one launch: bit for bit
    fixup_act(bicubic_up2_bias(t_low), a, b), without the upsampled tensor in between (csrc/up_train.hip)."""
    _need_gpu(t_low)
    t_low = t_low.contiguous()
    B, H, W, C = t_low.shape
    y = torch.empty((B, 2 * H, 2 * W, C), dtype=torch.float32, device=t_low.device)
    L.check(L.lib().vqae_up2_act_f32(_p(t_low), _p(_scalar(a)), _p(_scalar(b)), B, H, W, C, _p(y), _stream()))
    return y


def up2_act_backward(g, t_low, a):
    """-> (g_t_low [B, H, W, C], g_a [1], g_b [1]) from g [B, 2H, 2W, C] and the forward's t_low and a: the bits of
    bicubic_up2_backward(fixup_act_backward(g, bicubic_up2_bias(t_low), a)[0]) with up2(t_low) recomputed in LDS."""
    _need_gpu(g, t_low)
    g, t_low = g.contiguous(), t_low.contiguous()
    B, H, W, C = t_low.shape
    assert tuple(g.shape) == (B, 2 * H, 2 * W, C), (g.shape, t_low.shape)
    dev = g.device
    g_t_low = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)
    g_a, g_b = (torch.empty(1, dtype=torch.float32, device=dev) for _ in range(2))
    ws = _up_train_ws(B, H, W, C, dev)
    L.check(L.lib().vqae_up2_act_backward_f32(_p(g), _p(t_low), _p(_scalar(a)), B, H, W, C, _p(g_t_low), _p(g_a), _p(g_b),
                                              _p(ws), _stream()))
    return g_t_low, g_a, g_b


def fixup_out_up(t, s_low, scale, bias4, bias1d):
    """y = (t * scale + bias4) + (bicubic_up2(s_low) + bias1d), t [B, 2H, 2W, C], s_low [B, H, W, C], one launch: bit for bit
    fixup_out(t, bicubic_up2_bias(s_low), scale, bias4, bias1d), without the upsampled skip (csrc/up_train.hip)."""
    _need_gpu(t, s_low)
    t, s_low = t.contiguous(), s_low.contiguous()
    B, H, W, C = s_low.shape
    assert tuple(t.shape) == (B, 2 * H, 2 * W, C), (t.shape, s_low.shape)
    y = torch.empty_like(t)
    L.check(L.lib().vqae_fixup_out_up_f32(_p(t), _p(s_low), _p(_scalar(scale)), _p(_scalar(bias4)), _p(_scalar(bias1d)), B, H, W,
                                          C, _p(y), _stream()))
    return y


def fixup_out_up_backward(g, t, scale):
    """-> (g_t = g * scale, g_s_low [B, H, W, C] = the bicubic adjoint of g, g_scale [1] = sum g t, g_bias [1] = sum g), one
    pass over g [B, 2H, 2W, C]."""
    _need_gpu(g, t)
    g, t = g.contiguous(), t.contiguous()
    assert t.shape == g.shape and g.shape[1] % 2 == 0 and g.shape[2] % 2 == 0, (t.shape, g.shape)
    B, H, W, C = g.shape[0], g.shape[1] // 2, g.shape[2] // 2, g.shape[3]
    dev = g.device
    g_t = torch.empty_like(g)
    g_s_low = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)
    g_scale, g_bias = (torch.empty(1, dtype=torch.float32, device=dev) for _ in range(2))
    ws = _up_train_ws(B, H, W, C, dev)
    L.check(L.lib().vqae_fixup_out_up_backward_f32(_p(g), _p(t), _p(_scalar(scale)), B, H, W, C, _p(g_t), _p(g_s_low),
                                                   _p(g_scale), _p(g_bias), None, _p(ws), _stream()))
    return g_t, g_s_low, g_scale, g_bias


def _ws(n_bytes, dev):
    return torch.empty(max(int(n_bytes), 8), dtype=torch.uint8, device=dev)


def _vec(p):
    """A [C] parameter or buffer as the kernels read it: dense fp32 in HBM (no copy for an fp32 Parameter)."""
    _need_gpu(p)
    return p.detach().float().contiguous()


def bn_act_train_supported(c):
    """Whether csrc/mbconv_train.hip takes c channels (a multiple of 4 up to 1024): one rule for its three nodes."""
    return bool(L.lib().vqae_bn_act_train_supported(int(c)))


def bn_act_train_forward(x, gamma, beta, running_mean, running_var, training, momentum, eps, silu=False, want_pool=False):
    """BatchNorm2d (+ SiLU) on x [B, H, W, C] -> (y, mean [C], invstd [C] (fp64), pool [B, C] | None).  training: batch statistics, and
    running_mean / running_var (fp32 device tensors, or None) are updated IN PLACE by the launch that finishes the sums; else
    the running statistics normalise and nothing is written.  pool[b, c] = sum_hw y.  One row in training mode: ValueError."""
    _need_f32("bn_act_train_forward", x=x)
    _need_gpu(x, gamma, beta)
    x = x.contiguous()
    B, H, W, C = x.shape
    dev = x.device
    for t in (running_mean, running_var):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()), "running statistics: dense fp32 in HBM"
    y = torch.empty_like(x)
    stat = torch.empty((2, C), dtype=torch.float64, device=dev)        # mean, invstd: kept in fp64 for the backward
    pool = torch.empty((B, C), dtype=torch.float32, device=dev) if want_pool else None
    ws = _ws(L.lib().vqae_bn_act_train_workspace_bytes(B, H * W, C), dev)
    L.check(L.lib().vqae_bn_act_train_forward_f32(_p(x), _p(_vec(gamma)), _p(_vec(beta)), _p(running_mean), _p(running_var),
                                                  int(training), float(momentum), float(eps), int(silu), B, H * W, C, _p(y),
                                                  _p(stat[0]), _p(stat[1]), _p(pool), _p(ws), _stream()))
    return y, stat[0], stat[1], pool


def bn_act_train_backward(g, x, mean, invstd, gamma, beta, training, silu=False, g_pool=None):
    """-> (g_x, g_gamma [C], g_beta [C]) from the gradient of y, the forward's x, mean, invstd and (when the pooled output was
    used) the gradient of pool [B, C]."""
    _need_f32("bn_act_train_backward", g=g, x=x)
    _need_gpu(g, x, mean, invstd, gamma, beta, g_pool)
    g, x = g.contiguous(), x.contiguous()
    B, H, W, C = x.shape
    assert g.shape == x.shape, (g.shape, x.shape)
    dev = x.device
    g_x = torch.empty_like(x)
    sums = torch.empty((2, C), dtype=torch.float32, device=dev)
    ws = _ws(L.lib().vqae_bn_act_train_workspace_bytes(B, H * W, C), dev)
    gp = None if g_pool is None else g_pool.float().contiguous()
    L.check(L.lib().vqae_bn_act_train_backward_f32(_p(g), _p(x), _p(mean.contiguous()), _p(invstd.contiguous()), _p(_vec(gamma)),
                                                   _p(_vec(beta)), _p(gp), int(training), int(silu), B, H * W, C, _p(g_x),
                                                   _p(sums), _p(ws), _stream()))
    return g_x, sums[1], sums[0]


def dwconv_train_supported(c, h, w, mode):
    return bool(L.lib().vqae_dwconv_train_supported(int(c), int(h), int(w), int(mode)))


def _dw_out_shape(mode, H, W):
    return {L.DW_SAME: (H, W), L.DW_DOWN: (H // 2, W // 2), L.DW_UP: (2 * H, 2 * W)}[mode]


def dwconv_train_forward(x, w, mode):
    """The depthwise conv of branch[3] on x [B, H, W, C] with the module's own weight [C, 1, k, k], read in place."""
    _need_f32("dwconv_train_forward", x=x)
    _need_gpu(x, w)
    x = x.contiguous()
    B, H, W, C = x.shape
    k = 3 if mode == L.DW_SAME else 2
    assert tuple(w.shape) == (C, 1, k, k), (w.shape, C, mode)
    Ho, Wo = _dw_out_shape(mode, H, W)
    y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    L.check(L.lib().vqae_dwconv_train_forward_f32(_p(x), _p(_vec(w)), mode, B, H, W, C, _p(y), _stream()))
    return y


def dwconv_train_backward(g, x, w, mode, need_x=True, need_w=True):
    """-> (g_x | None, g_w in w's shape | None); g_x gathered, g_w a fixed-order fp64 sum."""
    _need_f32("dwconv_train_backward", g=g, x=x)
    _need_gpu(g, x, w)
    g, x = g.contiguous(), x.contiguous()
    B, H, W, C = x.shape
    assert tuple(g.shape) == (B, *_dw_out_shape(mode, H, W), C), (g.shape, x.shape, mode)
    dev = x.device
    g_x = torch.empty_like(x) if need_x else None
    g_w = torch.empty(tuple(w.shape), dtype=torch.float32, device=dev) if need_w else None
    ws = _ws(L.lib().vqae_dwconv_train_workspace_bytes(B, H, W, C, mode), dev) if need_w else None
    L.check(L.lib().vqae_dwconv_train_backward_f32(_p(g), _p(x), _p(_vec(w)), mode, B, H, W, C, _p(g_x), _p(g_w), _p(ws),
                                                   _stream()))
    return g_x, g_w


def se_scale_forward(x, gate):
    """x [B, H, W, C] * gate [B, C]."""
    _need_f32("se_scale_forward", x=x)
    _need_gpu(x, gate)
    x, gate = x.contiguous(), gate.float().contiguous()
    B, H, W, C = x.shape
    assert tuple(gate.shape) == (B, C), (gate.shape, x.shape)
    y = torch.empty_like(x)
    L.check(L.lib().vqae_se_scale_forward_f32(_p(x), _p(gate), B, H * W, C, _p(y), _stream()))
    return y


def se_scale_backward(g, x, gate):
    """-> (g_x = g * gate, g_gate [B, C] = sum_hw g * x)."""
    _need_f32("se_scale_backward", g=g, x=x)
    _need_gpu(g, x, gate)
    g, x, gate = g.contiguous(), x.contiguous(), gate.float().contiguous()
    B, H, W, C = x.shape
    assert g.shape == x.shape, (g.shape, x.shape)
    g_x = torch.empty_like(x)
    g_gate = torch.empty((B, C), dtype=torch.float32, device=x.device)
    ws = _ws(L.lib().vqae_se_scale_workspace_bytes(B, H * W, C), x.device)
    L.check(L.lib().vqae_se_scale_backward_f32(_p(g), _p(x), _p(gate), B, H * W, C, _p(g_x), _p(g_gate), _p(ws), _stream()))
    return g_x, g_gate


# ---- the same six ops with 16-bit I/O (csrc/mbconv_train_io.hip): the [B, H, W, C] tensors of a call share one dtype (fp32,
# bf16 or f16), the small tensors stay fp32 / fp64, the gate fp32 or the tensors' dtype.  Each is bit for bit the fp32 op on the
# up-cast inputs followed by torch's cast, without the casts.
def _same_io(who, **tensors):
    """The one dtype of the [B, H, W, C] tensors of a call -> (torch dtype, VQAE_DT_* code)."""
    dts = {t.dtype for t in tensors.values() if t is not None}
    assert len(dts) == 1, f"{who}: {', '.join(f'{k} {t.dtype}' for k, t in tensors.items() if t is not None)}: one dtype per call"
    dt = dts.pop()
    return dt, _io_code(who, "/".join(tensors), dt)


def bn_act_train_forward_io(x, gamma, beta, running_mean, running_var, training, momentum, eps, silu=False, want_pool=False):
    """bn_act_train_forward on x fp32, bf16 or f16 -> (y in x's dtype, mean, invstd (fp64), pool (fp32) | None): y rounded once,
    every statistic and pool from the unrounded fp32 values."""
    _, dt = _same_io("bn_act_train_forward_io", x=x)
    _need_gpu(x, gamma, beta)
    x = x.contiguous()
    B, H, W, C = x.shape
    dev = x.device
    for t in (running_mean, running_var):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()), "running statistics: dense fp32 in HBM"
    y = torch.empty_like(x)
    stat = torch.empty((2, C), dtype=torch.float64, device=dev)
    pool = torch.empty((B, C), dtype=torch.float32, device=dev) if want_pool else None
    ws = _ws(L.lib().vqae_bn_act_train_workspace_bytes(B, H * W, C), dev)
    L.check(L.lib().vqae_bn_act_train_forward_io(_p(x), _p(_vec(gamma)), _p(_vec(beta)), _p(running_mean), _p(running_var),
                                                 int(training), float(momentum), float(eps), int(silu), B, H * W, C, _p(y),
                                                 _p(stat[0]), _p(stat[1]), _p(pool), _p(ws), dt, _stream()))
    return y, stat[0], stat[1], pool


def bn_act_train_backward_io(g, x, mean, invstd, gamma, beta, training, silu=False, g_pool=None):
    """bn_act_train_backward on g and x of one dtype -> (g_x in that dtype, g_gamma [C], g_beta [C] fp32)."""
    _, dt = _same_io("bn_act_train_backward_io", g=g, x=x)
    _need_gpu(g, x, mean, invstd, gamma, beta, g_pool)
    g, x = g.contiguous(), x.contiguous()
    B, H, W, C = x.shape
    assert g.shape == x.shape, (g.shape, x.shape)
    dev = x.device
    g_x = torch.empty_like(x)
    sums = torch.empty((2, C), dtype=torch.float32, device=dev)
    ws = _ws(L.lib().vqae_bn_act_train_workspace_bytes(B, H * W, C), dev)
    gp = None if g_pool is None else g_pool.float().contiguous()
    L.check(L.lib().vqae_bn_act_train_backward_io(_p(g), _p(x), _p(mean.contiguous()), _p(invstd.contiguous()), _p(_vec(gamma)),
                                                  _p(_vec(beta)), _p(gp), int(training), int(silu), B, H * W, C, _p(g_x),
                                                  _p(sums), _p(ws), dt, _stream()))
    return g_x, sums[1], sums[0]


def dwconv_train_forward_io(x, w, mode):
    """dwconv_train_forward on x fp32, bf16 or f16 -> y in x's dtype; w the module's fp32 weight, each tap rounded to x's dtype
    in registers."""
    _, dt = _same_io("dwconv_train_forward_io", x=x)
    _need_gpu(x, w)
    x = x.contiguous()
    B, H, W, C = x.shape
    k = 3 if mode == L.DW_SAME else 2
    assert tuple(w.shape) == (C, 1, k, k), (w.shape, C, mode)
    Ho, Wo = _dw_out_shape(mode, H, W)
    y = torch.empty((B, Ho, Wo, C), dtype=x.dtype, device=x.device)
    L.check(L.lib().vqae_dwconv_train_forward_io(_p(x), _p(_vec(w)), mode, B, H, W, C, _p(y), dt, _stream()))
    return y


def dwconv_train_backward_io(g, x, w, mode, need_x=True, need_w=True):
    """dwconv_train_backward on g and x of one dtype -> (g_x in that dtype | None, g_w fp32 in w's shape | None)."""
    _, dt = _same_io("dwconv_train_backward_io", g=g, x=x)
    _need_gpu(g, x, w)
    g, x = g.contiguous(), x.contiguous()
    B, H, W, C = x.shape
    assert tuple(g.shape) == (B, *_dw_out_shape(mode, H, W), C), (g.shape, x.shape, mode)
    dev = x.device
    g_x = torch.empty_like(x) if need_x else None
    g_w = torch.empty(tuple(w.shape), dtype=torch.float32, device=dev) if need_w else None
    ws = _ws(L.lib().vqae_dwconv_train_workspace_bytes(B, H, W, C, mode), dev) if need_w else None
    L.check(L.lib().vqae_dwconv_train_backward_io(_p(g), _p(x), _p(_vec(w)), mode, B, H, W, C, _p(g_x), _p(g_w), _p(ws), dt,
                                                  _stream()))
    return g_x, g_w


def _gate_io(who, gate, x_dtype):
    """The gate as the kernels read it: in x's dtype or in fp32 (any other dtype is up-cast) -> (gate, its code)."""
    if gate.dtype != x_dtype and gate.dtype != torch.float32:
        gate = gate.float()
    return gate.contiguous(), _io_code(who, "gate", gate.dtype)


def se_scale_forward_io(x, gate):
    """se_scale_forward on x fp32, bf16 or f16 and gate [B, C] in fp32 or x's dtype -> y in x's dtype."""
    xd, dt = _same_io("se_scale_forward_io", x=x)
    _need_gpu(x, gate)
    x = x.contiguous()
    gate, dg = _gate_io("se_scale_forward_io", gate, xd)
    B, H, W, C = x.shape
    assert tuple(gate.shape) == (B, C), (gate.shape, x.shape)
    y = torch.empty_like(x)
    L.check(L.lib().vqae_se_scale_forward_io(_p(x), _p(gate), B, H * W, C, _p(y), dt, dg, _stream()))
    return y


def se_scale_backward_io(g, x, gate):
    """se_scale_backward on g and x of one dtype -> (g_x in that dtype, g_gate [B, C] in the gate's dtype: the fp32 sum, rounded
    once more for a 16-bit gate)."""
    xd, dt = _same_io("se_scale_backward_io", g=g, x=x)
    _need_gpu(g, x, gate)
    g, x = g.contiguous(), x.contiguous()
    gate, dg = _gate_io("se_scale_backward_io", gate, xd)
    B, H, W, C = x.shape
    assert g.shape == x.shape, (g.shape, x.shape)
    g_x = torch.empty_like(x)
    g_gate = torch.empty((B, C), dtype=gate.dtype, device=x.device)
    ws = _ws(L.lib().vqae_se_scale_workspace_bytes(B, H * W, C), x.device)
    L.check(L.lib().vqae_se_scale_backward_io(_p(g), _p(x), _p(gate), B, H * W, C, _p(g_x), _p(g_gate), _p(ws), dt, dg,
                                              _stream()))
    return g_x, g_gate


@functools.lru_cache(maxsize=None)
def _conv_train_node(node):
    """L.CONV_TRAIN[node] with its entries resolved, once."""
    stem, k, stride, image, bias = L.CONV_TRAIN[node]
    fns = {fn: getattr(L.lib(), f"{stem}_{fn}") for fn in ("workspace_bytes", "forward_f32", "backward_f32")}
    return types.SimpleNamespace(kernel=(k, k), stride=stride, image=image, bias=bias, **fns)


def _conv_train_args(nd, x, w, a, b):
    """-> (w as the library reads it, the arguments between w and cin, cin, cout, y's shape, pre) for a node nd.
    With an image: a channels_last [Co, Ci, kh, kw] weight is [Co][kh][kw][Ci] in memory and is passed as it lies (w_layout 1);
    anything else is made contiguous (w_layout 0).  No copy for either of the two ways torch stores a dense fp32 weight.
    Without: x [..., Ci], the weight always contiguous, no w_layout."""
    w = w.detach().float()
    cout, cin = w.shape[0], w.shape[1]
    if nd.image:
        assert x.dim() == 4 and tuple(w.shape[2:]) == nd.kernel and x.shape[-1] == cin, (x.shape, w.shape)
        B, H, W, _ = x.shape
        layout = int(w.is_contiguous(memory_format=torch.channels_last) and not w.is_contiguous())
        geo, y_shape = (layout, B, H, W), (B, H // nd.stride, W // nd.stride, cout)
    else:
        assert w.numel() == cout * cin and x.shape[-1] == cin, (x.shape, w.shape)
        layout, geo, y_shape = 0, (x.numel() // cin,), x.shape[:-1] + (cout,)
    assert a is None or b is not None, "pre-op: none (a, b None), x + b (a None), ELU(x + a) + b"
    return (w if layout else w.contiguous()), geo, cin, cout, y_shape, (0 if b is None else 1 if a is None else 2)


def _conv_train_ws(nd, geo, cin, cout, dev):
    return torch.empty(nd.workspace_bytes(*geo[-3:], cin, cout), dtype=torch.uint8, device=dev)         # geo without the layout


def _conv_train_forward(node, x, w, a, b, bias=None):
    """bias [Co] or None: for a node with a bias seat (L.CONV_TRAIN) only."""
    _need_gpu(x, w)
    x = x.contiguous()
    nd = _conv_train_node(node)
    assert bias is None or nd.bias, node
    wc, geo, cin, cout, y_shape, pre = _conv_train_args(nd, x, w, a, b)
    y = torch.empty(y_shape, dtype=torch.float32, device=x.device)
    # layout 0 alone needs one, and only where the node permutes the weight
    ws = _conv_train_ws(nd, geo, cin, cout, x.device) if nd.image and not nd.bias and geo[0] == 0 else None
    if bias is not None:
        _need_gpu(bias)
        bias = bias.detach().float().contiguous()
        assert tuple(bias.shape) == (cout,), (bias.shape, w.shape)
        if bias.data_ptr() % 16:                                   # a view into a flat buffer: the kernels read 16-byte groups
            bias = bias.clone()
    L.check(nd.forward_f32(_p(x), _p(_scalar(a)), _p(_scalar(b)), pre, _p(wc), *([_p(bias)] if nd.bias else []), *geo, cin, cout,
                           _p(y), *([_p(ws)] if nd.image else []), _stream()))
    return y


def _conv_train_backward(node, g, x, w, a, b, need_x, need_w, need_bias=False):
    """-> (g_x, g_w, g_a, g_b), and g_bias [Co] | None behind them for a node with a bias seat."""
    _need_gpu(g, x, w)
    g, x = g.contiguous(), x.contiguous()
    nd = _conv_train_node(node)
    wc, geo, cin, cout, y_shape, pre = _conv_train_args(nd, x, w, a, b)
    if nd.image:
        assert tuple(g.shape) == y_shape, (g.shape, x.shape, w.shape)
    else:
        assert g.shape[-1] == cout and g.numel() == geo[0] * cout, (g.shape, x.shape, w.shape)
    dev = g.device
    g_x = torch.empty_like(x) if need_x else None
    # dense: the same strides, i.e. the same layout;  without an image: contiguous in w's shape
    g_w = (torch.empty_like(wc) if nd.image else torch.empty(w.shape, dtype=torch.float32, device=dev)) if need_w else None
    g_a = torch.empty(1, dtype=torch.float32, device=dev) if pre == 2 else None
    g_b = torch.empty(1, dtype=torch.float32, device=dev) if pre >= 1 else None
    assert nd.bias or not need_bias, node
    g_bias = torch.empty(cout, dtype=torch.float32, device=dev) if need_bias else None
    ws = _conv_train_ws(nd, geo, cin, cout, dev)
    L.check(nd.backward_f32(_p(g), _p(x), _p(_scalar(a)), _p(_scalar(b)), pre, _p(wc), *geo, cin, cout, _p(g_x), _p(g_w), _p(g_a),
                            _p(g_b), *([_p(g_bias)] if nd.bias else []), _p(ws), _stream()))
    return (g_x, g_w, g_a, g_b, g_bias) if nd.bias else (g_x, g_w, g_a, g_b)


def conv1x1_train_supported(cin, cout):
    """Whether the trainable 1x1 conv kernels take (cin, cout).  A host-side question: needs no GPU."""
    return bool(L.lib().vqae_conv1x1_train_supported(int(cin), int(cout)))


def conv1x1_train_wgrad_run():
    """R: the longest fp32 accumulation run of the weight gradient, in rows."""
    return int(L.lib().vqae_conv1x1_train_wgrad_run())


def conv1x1_train_forward(x, w, a=None, b=None):
    """y [..., Co] = u [..., Ci] . w^T, w [Co, Ci(, 1, 1)] as torch stores it; u = x (a, b None), x + b (a None) or
    ELU(x + a) + b, with a, b one-element device tensors.  u is not materialised."""
    return _conv_train_forward("conv1x1", x, w, a, b)


def conv1x1_train_backward(g, x, w, a=None, b=None, need_x=True, need_w=True):
    """-> (g_x [..., Ci] | None, g_w (w's shape) | None, g_a [1] | None, g_b [1] | None) from g [..., Co] and the forward's
    x, w, a, b: g_u = g . w, g_x = g_u * ELU'(x + a) (g_u without an activation), g_a = sum g_x, g_b = sum g_u,
    g_w = g^T . u with u recomputed from x."""
    return _conv_train_backward("conv1x1", g, x, w, a, b, need_x, need_w)


def conv_down_train_supported(cin, cout):
    """Whether the trainable 2x2, stride-2 conv kernels take (cin, cout); H and W must be even besides.  Needs no GPU."""
    return bool(L.lib().vqae_conv_down_train_supported(int(cin), int(cout)))


def conv_down_train_wgrad_run():
    """R: the longest fp32 accumulation run of the weight gradient, in rows."""
    return int(L.lib().vqae_conv_down_train_wgrad_run())


def conv_down_train_forward(x, w, a=None, b=None):
    """y [B, H/2, W/2, Co] = the 2x2, stride-2 conv of u [B, H, W, Ci] with w [Co, Ci, 2, 2] (contiguous or channels_last, read
    in place); u = x (a, b None), x + b (a None) or ELU(x + a) + b, with a, b one-element device tensors.  u is not
    materialised."""
    return _conv_train_forward("conv_down", x, w, a, b)


def conv_down_train_backward(g, x, w, a=None, b=None, need_x=True, need_w=True):
    """-> (g_x [B, H, W, Ci] | None, g_w (w's shape and memory format) | None, g_a [1] | None, g_b [1] | None) from
    g [B, H/2, W/2, Co] and the forward's x, w, a, b: g_u = the data gradient, g_x = g_u * ELU'(x + a) (g_u without an
    activation), g_a = sum g_x, g_b = sum g_u, g_w = the weight gradient with u recomputed from x."""
    return _conv_train_backward("conv_down", g, x, w, a, b, need_x, need_w)


def conv3x3_train_supported(cin, cout):
    """Whether the trainable circular 3x3 conv kernels take (cin, cout); any H, W >= 1.  Needs no GPU."""
    return bool(L.lib().vqae_conv3x3_train_supported(int(cin), int(cout)))


def conv3x3_train_wgrad_run():
    """R: the longest fp32 accumulation run of the weight gradient, in rows."""
    return int(L.lib().vqae_conv3x3_train_wgrad_run())


def conv3x3_train_forward(x, w, a=None, b=None):
    """y [B, H, W, Co] = the 3x3, stride-1 conv with circular padding 1 of u [B, H, W, Ci] with w [Co, Ci, 3, 3] (contiguous or
    channels_last, read in place); u = x (a, b None), x + b (a None) or ELU(x + a) + b, with a, b one-element device tensors.
    Neither u nor its halo is materialised."""
    return _conv_train_forward("conv3x3", x, w, a, b)


def conv3x3_train_backward(g, x, w, a=None, b=None, need_x=True, need_w=True):
    """-> (g_x [B, H, W, Ci] | None, g_w (w's shape and memory format) | None, g_a [1] | None, g_b [1] | None) from
    g [B, H, W, Co] and the forward's x, w, a, b: g_u = the data gradient (gathered: the circular 3x3 of g with the flipped,
    transposed weight), g_x = g_u * ELU'(x + a) (g_u without an activation), g_a = sum g_x, g_b = sum g_u, g_w = the weight
    gradient with u recomputed from x."""
    return _conv_train_backward("conv3x3", g, x, w, a, b, need_x, need_w)


def conv3x3z_train_supported(cin, cout):
    """Whether the trainable zero-padded 3x3 conv kernels take (cin, cout): exactly one side of 3 channels (cin = 3 with cout a
    multiple of 8 up to 64, or cout = 3 with cin a multiple of 8 up to 256); any H, W >= 1.  Needs no GPU."""
    return bool(L.lib().vqae_conv3x3z_train_supported(int(cin), int(cout)))


def conv3x3z_train_wgrad_run():
    """R: the longest fp32 accumulation run of the weight and bias gradients, in rows."""
    return int(L.lib().vqae_conv3x3z_train_wgrad_run())


def conv3x3z_train_forward(x, w, bias=None, c=None):
    """y [B, H, W, Co] = bias + the 3x3, stride-1 conv with ZERO padding 1 of u [B, H, W, Ci] with w [Co, Ci, 3, 3] (contiguous
    or channels_last, read in place); u = x (c None) or x + c, c a one-element device tensor.  The padding follows the pre-op:
    F.conv2d(x + c, w, bias, padding=1).  u is not materialised."""
    return _conv_train_forward("conv3x3z", x, w, None, c, bias)


def conv3x3z_train_backward(g, x, w, c=None, need_x=True, need_w=True, need_bias=False):
    """-> (g_x [B, H, W, Ci] | None, g_w (w's shape and memory format) | None, g_bias [Co] | None, g_c [1] | None) from
    g [B, H, W, Co] and the forward's x, w, c: g_x the data gradient (gathered: the zero-padded 3x3 of g with the flipped,
    transposed weight), g_c = sum g_x, g_w the weight gradient with u recomputed from x, g_bias = sum of g over the pixels."""
    g_x, g_w, _, g_c, g_bias = _conv_train_backward("conv3x3z", g, x, w, None, c, need_x, need_w, need_bias)
    return g_x, g_w, g_bias, g_c


def vq_forward(z_flat, embed, commitment_cost=1.0, idx_dtype=torch.int64, want_q=True, want_margin=False, p=4):
    """z_flat [N, D], embed [K, D] -> (q [N, D] | None, idx [N], loss 0-d, margin [N] | None).  p: the Minkowski exponent of the
    reference's cdist = the rank of the quantiser's input (vq.py:97,121-129): 4 for NCHW, 3 / 5 for [B, D, L] / [B, D, d, h, w]."""
    _need_gpu(z_flat, embed)
    z_flat = z_flat.contiguous()
    embed = embed.contiguous()
    N, D = z_flat.shape
    K = embed.shape[0]
    dev = z_flat.device
    idx = torch.empty(N, dtype=idx_dtype, device=dev)
    q = torch.empty_like(z_flat) if want_q else None
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    margin = torch.empty(N, dtype=torch.float32, device=dev) if want_margin else None
    ws = torch.empty(L.lib().vqae_vq_workspace_bytes(N, K, D), dtype=torch.uint8, device=dev)
    L.check(L.lib().vqae_vq_forward_p_f32(_p(z_flat), _p(embed), N, K, D, int(p), float(commitment_cost), _p(idx),
                                          idx_code(idx_dtype), _p(q), _p(loss), _p(margin), _p(ws), _stream()))
    return q, idx, loss, margin


def vq_projected(x_flat, proj_in_w, proj_in_b, embed, proj_out_w, proj_out_b, commitment_cost=1.0, idx_dtype=torch.int64,
                 dtype=None, want_z=False, want_margin=False):
    """ProjectedEMAVectorQuantizer2d.forward on x_flat [N, C] (NHWC rows) in one launch (projection_dim 8):
    proj_in_w [8, C(,1,1)], proj_out_w [C, 8(,1,1)] as PyTorch stores them -> (out [N, C], idx [N], loss 0-d, z | None,
    margin | None).  With `dtype` ('bf16' / 'f16') the two convolutions round like torch.autocast."""
    _need_gpu(x_flat, proj_in_w, proj_in_b, embed, proj_out_w, proj_out_b)
    x_flat = x_flat.contiguous().float()
    N, C = x_flat.shape
    K, D = embed.shape
    dev = x_flat.device
    code = L.dtype_code(dtype)
    tdt = {L.DT_F32: None, L.DT_BF16: torch.bfloat16, L.DT_F16: torch.float16}[code]
    r = (lambda t: t.to(tdt).float()) if tdt is not None else (lambda t: t)
    wt_in = r(proj_in_w.reshape(D, C).float()).t().contiguous()
    w_out = r(proj_out_w.reshape(C, D).float()).contiguous()
    b_in, b_out = r(proj_in_b.float()).contiguous(), r(proj_out_b.float()).contiguous()
    idx = torch.empty(N, dtype=idx_dtype, device=dev)
    out = torch.empty_like(x_flat)
    z = torch.empty((N, D), dtype=torch.float32, device=dev) if want_z else None
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    margin = torch.empty(N, dtype=torch.float32, device=dev) if want_margin else None
    ws = torch.empty(L.lib().vqae_vq_projected_workspace_bytes(N), dtype=torch.uint8, device=dev)
    L.check(L.lib().vqae_vq_projected_f32(_p(x_flat), _p(wt_in), _p(b_in), _p(embed.contiguous().float()), _p(w_out), _p(b_out),
                                          N, C, D, K, float(commitment_cost), code, _p(idx), idx_code(idx_dtype), _p(out),
                                          _p(z), _p(loss), _p(margin), _p(ws), _stream()))
    return out, idx, loss, z, margin


def vq_backward(g_q, z_flat, q_flat, g_loss, commitment_cost):
    """g_z = g_q + g_loss * commitment_cost * 2 / (N * D) * (z - q) on [N, D] rows (the backward of vq.py:143-146).  g_q [N, D] or
    None, g_loss a 0-d fp32 device tensor or None (either None: a zero upstream gradient); g_loss is never read back."""
    _need_gpu(g_q, z_flat, q_flat, g_loss)
    z_flat, q_flat = z_flat.contiguous(), q_flat.contiguous()
    N, D = z_flat.shape
    g_q = g_q.contiguous().float() if g_q is not None else None
    g_loss = g_loss.reshape(()).float().contiguous() if g_loss is not None else None
    g_z = torch.empty_like(z_flat)
    L.check(L.lib().vqae_vq_backward_f32(_p(g_q), _p(z_flat), _p(q_flat), _p(g_loss), float(commitment_cost), N, D, _p(g_z),
                                         _stream()))
    return g_z


def vq_projected_backward(g_out, x_flat, z, q, g_loss, proj_in_w, proj_out_w, commitment_cost=1.0,
                          want=(True, True, True, True, True)):
    """All five gradients of ProjectedEMAVectorQuantizer2d.forward (projection_dim 8) in one pass over g_out [N, C] and
    x_flat [N, C]: -> (g_x [N, C], g_w_in [8, C], g_b_in [8], g_w_out [C, 8], g_b_out [C]), None where `want` is False.
    z, q [N, 8] as the forward saved them; g_out / g_loss may be None (zero); proj_in_w [8, C(,1,1)], proj_out_w
    [C, 8(,1,1)] as PyTorch stores them.  Bit-identical run to run."""
    _need_gpu(g_out, x_flat, z, q, g_loss, proj_in_w, proj_out_w)
    x_flat, z, q = x_flat.contiguous(), z.contiguous(), q.contiguous()
    N, C = x_flat.shape
    D = z.shape[1]
    dev = x_flat.device
    g_out = g_out.contiguous().float() if g_out is not None else None
    g_loss = g_loss.reshape(()).float().contiguous() if g_loss is not None else None
    wt_in = proj_in_w.reshape(D, C).float().t().contiguous()
    w_out = proj_out_w.reshape(C, D).float().contiguous()
    new = lambda on, *shape: torch.empty(shape, dtype=torch.float32, device=dev) if on else None
    g_x, g_w_in, g_b_in, g_w_out, g_b_out = (new(want[0], N, C), new(want[1], D, C), new(want[2], D), new(want[3], C, D),
                                             new(want[4], C))
    ws = torch.empty(L.lib().vqae_vq_projected_backward_workspace_bytes(N, C), dtype=torch.uint8, device=dev)
    L.check(L.lib().vqae_vq_projected_backward_f32(_p(g_out), _p(x_flat), _p(z), _p(q), _p(g_loss), _p(wt_in), _p(w_out), N, C, D,
                                                   float(commitment_cost), _p(g_x), _p(g_w_in), _p(g_b_in), _p(g_w_out),
                                                   _p(g_b_out), _p(ws), _stream()))
    return g_x, g_w_in, g_b_in, g_w_out, g_b_out


def embed_code(idx, embed):
    _need_gpu(idx, embed)
    idx = idx.contiguous()
    embed = embed.contiguous()
    K, D = embed.shape
    out = torch.empty(tuple(idx.shape) + (D,), dtype=torch.float32, device=idx.device)
    L.check(L.lib().vqae_embed_code_f32(_p(idx), idx_code(idx.dtype), _p(embed), idx.numel(), K, D, _p(out),
                                        _stream()))
    return out


def vq_code_stats(z_flat, idx, n_codes):
    """z_flat [N, D], idx [N] -> (counts [K], dw [K, D]) of _update_ema (vq.py:49-54); N = 0 gives zeros."""
    _need_gpu(z_flat, idx)
    z_flat = z_flat.contiguous()
    idx = idx.contiguous()
    N, D = z_flat.shape
    counts = torch.empty(n_codes, dtype=torch.float32, device=z_flat.device)
    dw = torch.empty((n_codes, D), dtype=torch.float32, device=z_flat.device)
    L.check(L.lib().vqae_vq_code_stats_f32(_p(z_flat), _p(idx), idx_code(idx.dtype), N, n_codes, D, _p(counts),
                                           _p(dw), _stream()))
    return counts, dw


def vq_ema_update(embed, embed_avg, cluster_size, counts, dw, decay, laplace_alpha):
    """The EMA + Laplace step of _update_ema, in place.  decay / laplace_alpha go down as doubles: 1 - decay and K * laplace_alpha
    are formed from them and rounded to fp32 once, the scalars torch's fp32 tensors see (vq.py:60-71)."""
    _need_gpu(embed, embed_avg, cluster_size, counts, dw)
    K, D = embed.shape
    ws = torch.empty(16, dtype=torch.uint8, device=embed.device)
    L.check(L.lib().vqae_vq_ema_update_f32(_p(embed), _p(embed_avg), _p(cluster_size), _p(counts), _p(dw), K, D,
                                           float(decay), float(laplace_alpha), _p(ws), _stream()))


def label_maxpool(labels_u8, out=32):
    _need_gpu(labels_u8)
    labels_u8 = labels_u8.contiguous()
    B, H, W = labels_u8.shape
    y = torch.empty((B, out, out), dtype=torch.uint8, device=labels_u8.device)
    L.check(L.lib().vqae_label_maxpool_u8(_p(labels_u8), B, H, W, out, _p(y), _stream()))
    return y


def stitch_tiles(tiles, rc, grid):
    """tiles [n, th, tw] scattered into grid [gh, gw] at patch positions rc [n, 2] (int32), in place."""
    _need_gpu(tiles, rc, grid)
    tiles = tiles.contiguous()
    rc = rc.to(torch.int32).contiguous()
    n, th, tw = tiles.shape
    L.check(L.lib().vqae_stitch_tiles(_p(tiles), idx_code(tiles.dtype), _p(rc), n, th, tw, _p(grid),
                                      idx_code(grid.dtype), grid.shape[0], grid.shape[1], _stream()))
    return grid


def unstitch_tiles(grid, rc, th, tw, dtype=torch.int64, out=None):
    """The inverse of stitch_tiles: grid [gh, gw] (any index dtype) cut into tiles [n, th, tw] of `dtype` at the patch positions
    rc [n, 2] (int32).  Positions are the caller's to validate: elements outside the grid are not written (they keep what
    `out`, a contiguous [n, th, tw] tensor to fill, held; without `out` they are whatever the allocation held)."""
    _need_gpu(grid, rc, out)
    grid = grid.contiguous()
    rc = rc.to(torch.int32).contiguous()
    n = rc.shape[0]
    if out is not None:
        assert tuple(out.shape) == (n, th, tw) and out.is_contiguous(), out.shape
        tiles, dtype = out, out.dtype
    else:
        tiles = torch.empty((n, th, tw), dtype=dtype, device=grid.device)
    L.check(L.lib().vqae_unstitch_tiles(_p(grid), idx_code(grid.dtype), _p(rc), n, th, tw, _p(tiles), idx_code(dtype),
                                        grid.shape[0], grid.shape[1], _stream()))
    return tiles


def _f32x3(values, scale):
    """host float[3] of fp32(v) * fp32(scale), the product formed in fp32 as the kernels' own constants are"""
    import numpy as np
    return (ctypes.c_float * 3)(*[float(np.float32(v) * np.float32(scale)) for v in values])


def pixels_u8(x, layout="NCHW", rc=None, canvas=None, mean=MEAN, std=STD, level=0):
    """fp32 reconstruction x ([B,3,H,W], or [B,H,W,3] with layout="NHWC") -> uint8 NHWC pixels
    clamp(rint(x * std * 255 + mean * 255), 0, 255) (one fma, round-to-nearest-even, NaN -> 0): the inverse of the ingest
    Normalize.  rc=None -> a dense [B,H,W,3] tensor; rc [B, 2] (int32) + canvas [ch, cw, 3] uint8 -> tile t pasted in place at
    pixel (rc[t, 0] * H, rc[t, 1] * W), the canvas returned.  mean / std: 3 floats, or None for 0 / 1.
    level L > 0 (at most 6, f = 2**L dividing H and W): the integer mean, rounding half up, of every f x f block of those
    pixels, (sum + f*f/2) >> 2L -- a dense [B,H/f,W/f,3], or tile t at pixel (rc[t, 0] * H/f, rc[t, 1] * W/f) of a canvas given
    in level-L pixels."""
    _need_gpu(x, rc, canvas)
    assert layout in ("NCHW", "NHWC"), layout
    x = x.contiguous()
    assert x.dtype == torch.float32 and x.dim() == 4, (x.dtype, x.shape)
    if layout == "NCHW":
        B, C, H, W = x.shape
    else:
        B, H, W, C = x.shape
    assert C == 3, x.shape
    level = int(level)
    m = _f32x3(mean, 255.0) if mean is not None else None
    s = _f32x3(std, 255.0) if std is not None else None
    lay = L.LAYOUT_NCHW if layout == "NCHW" else L.LAYOUT_NHWC

    def run(rc_p, out, ch, cw):
        if level == 0:
            L.check(L.lib().vqae_pixels_u8(_p(x), lay, B, H, W, rc_p, m, s, _p(out), ch, cw, _stream()))
        else:
            L.check(L.lib().vqae_pixels_u8_level(_p(x), lay, B, H, W, level, rc_p, m, s, _p(out), ch, cw, _stream()))
        return out

    if rc is None:
        assert canvas is None, "pixels_u8: a canvas needs rc"
        lv = min(max(level, 0), 31)                                    # (a shape for any level; the library judges the level)
        out = torch.empty((B, H >> lv, W >> lv, 3), dtype=torch.uint8, device=x.device)
        return run(None, out, 0, 0)
    assert canvas is not None and canvas.dtype == torch.uint8 and canvas.dim() == 3 and canvas.shape[2] == 3 and \
        canvas.is_contiguous(), "pixels_u8: canvas must be a contiguous uint8 [h, w, 3] tensor"
    rc = rc.to(torch.int32).contiguous()
    assert tuple(rc.shape) == (B, 2), rc.shape
    return run(_p(rc), canvas, canvas.shape[0], canvas.shape[1])


def cut_pixels_u8(canvas, rc, h, w, *, y0=0, x0=0, level=0, out=None):
    """Tiles [n, h, w, ch] (uint8) cut out of the pixel canvas [H, W, ch] (uint8, ch 1 or 3, in HBM) at the patch positions rc
    [n, 2] (int32), box-reduced to `level` (f = 2**level): tile t covers the (h * f) x (w * f) canvas pixels at
    (y0 + rc[t, 0] * h * f, x0 + rc[t, 1] * w * f), every output pixel the integer mean, rounding half up, of its f x f block
    (level 0: a copy).  A tile that does not lie wholly inside the canvas is skipped: it keeps what `out`, a contiguous
    [n, h, w, ch] tensor to fill, held (without `out`: whatever the allocation held)."""
    _need_gpu(canvas, rc, out)
    assert canvas.dtype == torch.uint8 and canvas.dim() == 3 and canvas.is_contiguous(), \
        "cut_pixels_u8: canvas must be a contiguous uint8 [H, W, ch] tensor"
    H, W, ch = canvas.shape
    rc = rc.to(torch.int32).contiguous()
    assert rc.dim() == 2 and rc.shape[1] == 2, rc.shape
    n = rc.shape[0]
    if out is not None:
        assert out.dtype == torch.uint8 and tuple(out.shape) == (n, h, w, ch) and out.is_contiguous(), out.shape
    else:
        out = torch.empty((n, h, w, ch), dtype=torch.uint8, device=canvas.device)
    L.check(L.lib().vqae_cut_pixels_u8(_p(canvas), H, W, ch, _p(rc) if n else None, n, int(h), int(w), int(y0), int(x0), int(level),
                                       _p(out) if n else None, _stream()))
    return out


def pool_labels_u8(mask, win, *, y0=0, x0=0, out_hw=None):
    """Label grid [out_h, out_w] (uint8) of the mask canvas [H, W] (uint8, in HBM): out[Y, X] = the maximum of the win x win (or
    (win_h, win_w)) window at (y0 + Y * win_h, x0 + X * win_w).  out_hw defaults to every whole window from the origin on; a
    window reaching outside the mask raises."""
    _need_gpu(mask)
    assert mask.dtype == torch.uint8 and mask.dim() == 2 and mask.is_contiguous(), "pool_labels_u8: mask must be a contiguous uint8 [H, W] tensor"
    wh, ww = (win, win) if isinstance(win, int) else (int(win[0]), int(win[1]))
    H, W = mask.shape
    if out_hw is None:
        assert wh >= 1 and ww >= 1, win
        out_hw = (max(H - y0, 0) // wh, max(W - x0, 0) // ww)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((max(oh, 0), max(ow, 0)), dtype=torch.uint8, device=mask.device)
    L.check(L.lib().vqae_pool_labels_u8(_p(mask), H, W, int(y0), int(x0), wh, ww, _p(out) if out.numel() else None, oh, ow,
                                        _stream()))
    return out


def cut_pixels_reference(canvas, rc, h, w, *, y0=0, x0=0, level=0, out=None):
    """numpy restatement of cut_pixels_u8 for host arrays (the yardstick of the tests, and the cut of the injected-encode
    path): the same tiles, the same skipped tiles."""
    import numpy as np
    canvas, rc = np.asarray(canvas), np.asarray(rc).reshape(-1, 2)
    assert canvas.dtype == np.uint8 and canvas.ndim == 3, (canvas.dtype, canvas.shape)
    H, W, ch = canvas.shape
    f = 1 << level
    tiles = out if out is not None else np.zeros((len(rc), h, w, ch), np.uint8)
    for t, (r, c) in enumerate(rc.tolist()):
        sy, sx = y0 + r * h * f, x0 + c * w * f
        if r < 0 or c < 0 or sy + h * f > H or sx + w * f > W:
            continue
        block = canvas[sy:sy + h * f, sx:sx + w * f].astype(np.uint32).reshape(h, f, w, f, ch)
        tiles[t] = ((block.sum(axis=(1, 3), dtype=np.uint32) + (f * f) // 2) >> (2 * level)).astype(np.uint8)
    return tiles


def pool_labels_reference(mask, win, *, y0=0, x0=0, out_hw=None):
    """numpy restatement of pool_labels_u8 for host arrays; AssertionError, like the library's, for a window reaching outside
    the mask"""
    import numpy as np
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim == 2, (mask.dtype, mask.shape)
    wh, ww = (win, win) if isinstance(win, int) else (int(win[0]), int(win[1]))
    H, W = mask.shape
    oh, ow = out_hw if out_hw is not None else ((H - y0) // wh, (W - x0) // ww)
    assert y0 >= 0 and x0 >= 0 and oh >= 0 and ow >= 0 and y0 + oh * wh <= H and x0 + ow * ww <= W, \
        f"pool_labels: {oh} x {ow} windows of {wh} x {ww} at ({y0}, {x0}) reach outside the {H} x {W} mask"
    return np.ascontiguousarray(mask[y0:y0 + oh * wh, x0:x0 + ow * ww].reshape(oh, wh, ow, ww).max(axis=(1, 3), initial=0))


def classifier_forward(handle, codes, n_out=1, logits=True, heat=False, mask=None, pos_weight=1.0):
    """vqae_classifier_forward on codes [B,H,W] (uint8 / uint16 / int32 / int64, in HBM) with the vqae_classifier `handle`
    (a ctypes pointer; classifier.NativeClassifier owns one) of `n_out` outputs -> (logits fp32 [B,n_out,H,W] | None,
    heat uint8 [B,H,W] | None, stats float64 [B, 6] in _lib.CLS_STATS_NAMES order | None).  stats are computed when `mask`
    (uint8 [B,H,W]: 0 background, 1 tissue, 2 cancer) is given; heat and stats need n_out == 1 (the library refuses)."""
    _need_gpu(codes, mask)
    assert codes.dim() == 3, codes.shape
    codes = codes.contiguous()
    B, H, W = codes.shape
    dev = codes.device
    lg = torch.empty((B, n_out, H, W), dtype=torch.float32, device=dev) if logits else None
    ht = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if heat else None
    stats = ws = None
    if mask is not None:
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == (B, H, W), (mask.dtype, mask.shape)
        mask = mask.contiguous()
        stats = torch.empty((B, len(L.CLS_STATS_NAMES)), dtype=torch.float64, device=dev)
        ws = torch.empty(max(1, L.lib().vqae_classifier_workspace_bytes(handle, B, H, W)), dtype=torch.uint8, device=dev)
    L.check(L.lib().vqae_classifier_forward(handle, _p(codes), idx_code(codes.dtype), B, H, W, _p(lg), _p(ht), _p(mask),
                                            float(pos_weight), _p(stats), _p(ws), _stream()))
    return lg, ht, stats


def classifier_loss_grad(handle, codes, mask, target=None, pos_weight=1.0, reduction="sum"):
    """vqae_classifier_loss_grad on codes [B,H,W] (as stored, in HBM) and mask uint8 [B,H,W] (0 background, 1 tissue,
    2 cancer) with the vqae_classifier `handle` (n_out == 1) -> (loss float64 [1], grads float64
    [vqae_classifier_grad_floats]: the seven tensors packed in PyTorch's shapes and parameter order, stats float64 [B, 6] in
    _lib.CLS_STATS_NAMES order).  target: optional fp32 [B,H,W] soft targets in [0, 1], read where mask != 0.  Codes are not
    checked against the table: one outside it is a zero vector without a gradient."""
    _need_gpu(codes, mask, target)
    assert codes.dim() == 3, codes.shape
    assert reduction in ("sum", "mean"), reduction
    codes = codes.contiguous()
    B, H, W = codes.shape
    dev = codes.device
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (B, H, W), (mask.dtype, mask.shape)
    mask = mask.contiguous()
    if target is not None:
        assert target.dtype == torch.float32 and tuple(target.shape) == (B, H, W), (target.dtype, target.shape)
        target = target.contiguous()
    lib = L.lib()
    grads = torch.empty(lib.vqae_classifier_grad_floats(handle), dtype=torch.float64, device=dev)
    stats = torch.empty((B, len(L.CLS_STATS_NAMES)), dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float64, device=dev)
    ws = torch.empty(max(1, lib.vqae_classifier_train_workspace_bytes(handle, B, H, W)), dtype=torch.uint8, device=dev)
    L.check(lib.vqae_classifier_loss_grad(handle, _p(codes), idx_code(codes.dtype), B, H, W, _p(mask), _p(target),
                                          float(pos_weight), 1 if reduction == "mean" else 0, _p(grads), _p(stats), _p(loss),
                                          _p(ws), _stream()))
    return loss, grads, stats


def _ce_weight(weight, n_out):
    """class weights -> a ctypes float [n_out] for the library (None = ones: a null pointer)"""
    if weight is None:
        return None
    w = [float(v) for v in (weight.tolist() if hasattr(weight, "tolist") else weight)]
    assert len(w) == n_out, f"class_weight has {len(w)} entries, the classifier {n_out} outputs"
    return (ctypes.c_float * n_out)(*w)


def classifier_forward_ce(handle, codes, n_out, logits=False, prob=False, cls=True, labels=None, weight=None, label_smoothing=0.0):
    """vqae_classifier_forward_ce on codes [B,H,W] (as stored, in HBM) with the vqae_classifier `handle` of n_out = 2 .. 4
    outputs -> (logits fp32 [B,n_out,H,W] | None, prob uint8 [B,n_out,H,W] | None, class uint8 [B,H,W] | None,
    stats float64 [B, 20] | None: the VQAE_CE_* rows, computed when `labels` (uint8 [B,H,W], class indices) is given, with
    `weight` (n_out floats or None = ones) and label_smoothing)."""
    _need_gpu(codes, labels)
    assert codes.dim() == 3, codes.shape
    codes = codes.contiguous()
    B, H, W = codes.shape
    dev = codes.device
    lg = torch.empty((B, n_out, H, W), dtype=torch.float32, device=dev) if logits else None
    pr = torch.empty((B, n_out, H, W), dtype=torch.uint8, device=dev) if prob else None
    cl = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if cls else None
    stats = ws = None
    if labels is not None:
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (B, H, W), (labels.dtype, labels.shape)
        labels = labels.contiguous()
        stats = torch.empty((B, L.CE_STATS_K), dtype=torch.float64, device=dev)
        ws = torch.empty(max(1, L.lib().vqae_classifier_ce_workspace_bytes(handle, B, H, W)), dtype=torch.uint8, device=dev)
    L.check(L.lib().vqae_classifier_forward_ce(handle, _p(codes), idx_code(codes.dtype), B, H, W, _p(lg), _p(pr), _p(cl), _p(labels),
                                               _ce_weight(weight, n_out), float(label_smoothing), _p(stats), _p(ws), _stream()))
    return lg, pr, cl, stats


def classifier_loss_grad_ce(handle, codes, labels, n_out, weight=None, label_smoothing=0.0, reduction="mean"):
    """vqae_classifier_loss_grad_ce on codes [B,H,W] (as stored, in HBM) and labels uint8 [B,H,W] (class indices) ->
    (loss float64 [1], grads float64 [vqae_classifier_grad_floats] packed as classifier_loss_grad's, stats float64 [B, 20]:
    the VQAE_CE_* rows).  Neither codes nor labels are checked: a code outside the table is a zero vector, a label >= n_out
    is counted in column 19 and passes no gradient."""
    _need_gpu(codes, labels)
    assert codes.dim() == 3, codes.shape
    assert reduction in ("sum", "mean"), reduction
    codes = codes.contiguous()
    B, H, W = codes.shape
    dev = codes.device
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (B, H, W), (labels.dtype, labels.shape)
    labels = labels.contiguous()
    lib = L.lib()
    grads = torch.empty(lib.vqae_classifier_grad_floats(handle), dtype=torch.float64, device=dev)
    stats = torch.empty((B, L.CE_STATS_K), dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float64, device=dev)
    ws = torch.empty(max(1, lib.vqae_classifier_ce_train_workspace_bytes(handle, B, H, W)), dtype=torch.uint8, device=dev)
    L.check(lib.vqae_classifier_loss_grad_ce(handle, _p(codes), idx_code(codes.dtype), B, H, W, _p(labels), _ce_weight(weight, n_out),
                                             float(label_smoothing), 1 if reduction == "mean" else 0, _p(grads), _p(stats),
                                             _p(loss), _p(ws), _stream()))
    return loss, grads, stats


def code_histogram(codes, mask=None, *, num_embeddings, n_labels=None, pooled=False, out=None, bad=None):
    """vqae_code_histogram on codes [B, ...] (uint8 / uint16 / int32 / int64 as stored, in HBM; B equally sized grids, any
    contiguous view) and mask uint8 of the same shape or None -> (hist int64 [B or 1, n_labels, num_embeddings],
    bad int64 [B or 1, 2]): hist[b, l, k] = positions of grid b with mask == l and code == k, exact; bad[:, 0] = codes outside
    the table, bad[:, 1] = labels >= n_labels (neither is counted in hist).  pooled=True sums the batch into one table.
    out= / bad= given: the counts are ADDED to them (a driver pools a split on the device and downloads once); a call that
    passes only one of the two starts the other at zero.  n_labels defaults to 3 with a mask and 1 without."""
    _need_gpu(codes, mask, out, bad)
    assert codes.dim() >= 2, f"codes [B, ...] expected, got {tuple(codes.shape)}"
    codes = codes.contiguous()
    B = codes.shape[0]
    n = codes.numel() // B if B else int(torch.Size(codes.shape[1:]).numel())
    dev = codes.device
    if n_labels is None:
        n_labels = 3 if mask is not None else 1
    if mask is not None:
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == tuple(codes.shape), (mask.dtype, mask.shape)
        mask = mask.contiguous()
    rows = 1 if pooled else B
    K = int(num_embeddings)
    for t, shape, what in ((out, (rows, int(n_labels), K), "out"), (bad, (rows, 2), "bad")):
        assert t is None or (t.dtype == torch.int64 and tuple(t.shape) == shape and t.is_contiguous()), \
            f"code_histogram: {what} must be a contiguous int64 tensor of shape {shape}"
    accumulate = out is not None or bad is not None
    if out is None:
        out = (torch.zeros if accumulate else torch.empty)((rows, max(int(n_labels), 0), max(K, 0)), dtype=torch.int64, device=dev)
    if bad is None:
        bad = (torch.zeros if accumulate else torch.empty)((rows, 2), dtype=torch.int64, device=dev)
    lib = L.lib()
    if B == 0:                                                     # nothing to count (and no pointer to pass): zeros, or out as it is
        return (out.zero_(), bad.zero_()) if not accumulate else (out, bad)
    ws = torch.empty(max(8, lib.vqae_code_histogram_workspace_bytes(B, n, K, int(n_labels))), dtype=torch.uint8, device=dev)
    L.check(lib.vqae_code_histogram(_p(codes), idx_code(codes.dtype), _p(mask), B, n, K, int(n_labels), int(bool(pooled)),
                                    int(accumulate), _p(out), _p(bad), _p(ws), _stream()))
    return out, bad
