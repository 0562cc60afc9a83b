"""CPU: the MBConv training path under 16-bit autocast (vqae_amd.train_mbconv with the 16-bit-I/O nodes of
csrc/mbconv_train_io.hip), through its plain-torch restatements, which follow the same dtype rule: a 16-bit input is up-cast,
the arithmetic is fp32, the result is rounded once to the input's dtype (tests/test_mbconv_train16_gpu.py runs the kernels).

  * the six _io entry points are declared, exported and bound, and validate their dtype codes and alignment before any HIP
    call; the fp32 wrappers of ops.py refuse a 16-bit tensor before any device call;
  * the reference's rounding points, which the design rests on: under torch.autocast("cpu") every intermediate of the stock
    block is 16-bit, the running statistics and the depthwise weight gradient are fp32, and a 16-bit F.batch_norm is bit for
    bit round(batch_norm_fp32(up(x)));
  * dtype flow: under CPU autocast train_mbconv.block_forward returns the autocast dtype from every node, saves 16-bit
    activations, leaves fp32 parameter gradients and runs no kernel;
  * distance to the fixture's fp64 values <= 4 x that of block_forward_torch under the same CPU autocast, per tensor group
    (mbconv_train_cases.result_groups).  Measured ratios e_dev / e_ref over the 150 groups of the seven cases: bf16
    0.45 .. 2.24, f16 0.52 .. 1.67 (both sides are a handful of 16-bit roundings away from fp64, at other points);
  * the fp32 / fp64 restatements are untouched: they give the bits of the formulas restated here.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import mbconv_train_cases as C

BAR = 4.0
BF16, F16 = torch.bfloat16, torch.float16
IO_SYMBOLS = ("vqae_bn_act_train_forward_io", "vqae_bn_act_train_backward_io", "vqae_dwconv_train_forward_io",
              "vqae_dwconv_train_backward_io", "vqae_se_scale_forward_io", "vqae_se_scale_backward_io")


def _cpu_autocast_works(dtype):
    """Whether this torch build has the CPU ops of a stock MBConv block in `dtype` (f16 arrived later than bf16)."""
    try:
        with torch.autocast("cpu", dtype=dtype):
            t = F.conv2d(torch.ones(1, 4, 2, 2), torch.ones(4, 4, 1, 1))
            t = F.silu(F.batch_norm(t, torch.zeros(4), torch.ones(4), torch.ones(4), torch.zeros(4), True, 0.1, 1e-5))
            t = F.conv_transpose2d(F.conv2d(t, torch.ones(4, 1, 2, 2), stride=2, groups=4), torch.ones(4, 1, 2, 2), stride=2,
                                   groups=4)
            t = t * torch.nn.Linear(4, 4)(t.mean((2, 3))).reshape(1, 4, 1, 1)
        return t.dtype == dtype
    except RuntimeError:
        return False


DTYPES = [BF16] + ([F16] if _cpu_autocast_works(F16) else [])


def under(forward, dtype):
    def run(blk, t):
        with torch.autocast("cpu", dtype=dtype):
            return forward(blk, t)
    return run


def results(block, x, g, forward):
    """mbconv_train_cases.block_results with the upstream gradient cast to the output's dtype (16-bit under autocast)."""
    x = x.detach().clone().requires_grad_()
    params = dict(block.named_parameters())
    y = forward(block, x)
    grads = torch.autograd.grad(y, [x] + list(params.values()), g.to(y.dtype))
    res = {"out": y.detach(), "input": grads[0]}
    res.update(dict(zip(params, grads[1:])))
    bnames = [k for k in block.state_dict() if k.endswith(("running_mean", "running_var"))]
    res.update({k: block.state_dict()[k].detach().clone() for k in bnames})
    return res, list(params), bnames


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_io_symbols_declared_exported_bound(amd):
    import test_abi
    declared, lib = test_abi.declared_symbols(), amd._lib.lib()
    for name in IO_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/vqae_hip.h"
        assert name in amd._lib.SYMBOLS, f"{name} is not bound in _lib.py"
        assert getattr(lib, name).argtypes == amd._lib.SYMBOLS[name][1]
    for name in ("bn_act_train_forward_io", "bn_act_train_backward_io", "dwconv_train_forward_io", "dwconv_train_backward_io",
                 "se_scale_forward_io", "se_scale_backward_io"):
        assert callable(getattr(amd.ops, name))


def test_io_entry_points_validate_before_any_launch(amd):
    """Dtype codes, the one-16-bit-type rule and the alignment (8 bytes for a 16-bit tensor, 16 for an fp32 one) are checked
    before any HIP call: the pointers below are never dereferenced."""
    L = amd._lib
    lib = L.lib()
    p16, p8, p2 = ctypes.c_void_p(64), ctypes.c_void_p(64 + 8), ctypes.c_void_p(64 + 2)
    bn_f = lambda x, y, dt: lib.vqae_bn_act_train_forward_io(x, p16, p16, p16, p16, 1, 0.1, 1e-5, 1, 2, 4, 8, y, p16, p16, None,
                                                             p16, dt, None)
    bn_b = lambda g, x, gx, dt: lib.vqae_bn_act_train_backward_io(g, x, p16, p16, p16, p16, None, 1, 1, 2, 4, 8, gx, p16, p16, dt,
                                                                  None)
    dw_f = lambda x, y, dt: lib.vqae_dwconv_train_forward_io(x, p16, L.DW_SAME, 1, 2, 2, 8, y, dt, None)
    dw_b = lambda g, x, gx, dt: lib.vqae_dwconv_train_backward_io(g, x, p16, L.DW_SAME, 1, 2, 2, 8, gx, p16, p16, dt, None)
    se_f = lambda x, gate, y, dt, dg: lib.vqae_se_scale_forward_io(x, gate, 1, 4, 8, y, dt, dg, None)
    se_b = lambda g, x, gate, gx, dt, dg: lib.vqae_se_scale_backward_io(g, x, gate, 1, 4, 8, gx, p16, p16, dt, dg, None)
    for dt in (L.DT_BF16, L.DT_F16):
        for rc in (bn_f(p2, p16, dt), bn_f(p16, p2, dt), bn_b(p2, p16, p16, dt), bn_b(p16, p2, p16, dt), bn_b(p16, p16, p2, dt),
                   dw_f(p2, p16, dt), dw_f(p16, p2, dt), dw_b(p2, p16, p16, dt), dw_b(p16, p16, p2, dt),
                   se_f(p2, p16, p16, dt, L.DT_F32), se_f(p16, p2, p16, dt, dt), se_f(p16, p8, p16, dt, L.DT_F32),
                   se_b(p16, p16, p16, p2, dt, dt)):
            with pytest.raises(AssertionError):                    # VQAE_ERR_INVALID: 1 element (2 bytes) off, fp32 gate 8 off
                L.check(rc)
            assert b"aligned" in lib.vqae_last_error()
        other = L.DT_F16 if dt == L.DT_BF16 else L.DT_BF16
        for rc in (se_f(p16, p16, p16, dt, other), se_b(p16, p16, p16, p16, dt, other), se_f(p16, p16, p16, L.DT_F32, dt)):
            with pytest.raises(NotImplementedError):               # VQAE_ERR_UNSUPPORTED
                L.check(rc)
            assert b"16-bit" in lib.vqae_last_error()
    for rc in (bn_f(p16, p16, 7), bn_b(p16, p16, p16, -1), dw_f(p16, p16, 3), dw_b(p16, p16, p16, 9),
               se_f(p16, p16, p16, 5, L.DT_F32), se_b(p16, p16, p16, p16, L.DT_BF16, 4)):
        with pytest.raises(AssertionError):
            L.check(rc)
        assert b"dtype code" in lib.vqae_last_error()
    with pytest.raises(NotImplementedError):                       # the shape rules of the fp32 entries hold
        L.check(lib.vqae_bn_act_train_forward_io(p16, p16, p16, p16, p16, 1, 0.1, 1e-5, 1, 2, 4, 6, p16, p16, p16, None, p16,
                                                 L.DT_BF16, None))
    with pytest.raises(ValueError):
        L.check(lib.vqae_bn_act_train_forward_io(p16, p16, p16, p16, p16, 1, 0.1, 1e-5, 1, 1, 1, 8, p16, p16, p16, None, p16,
                                                 L.DT_F16, None))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_fp32_wrappers_refuse_16bit_tensors(amd, dtype):
    """CPU tensors: the dtype assertion comes before the check for device memory, so before any device call."""
    ops, L = amd.ops, amd._lib
    x32, v = torch.zeros(1, 2, 2, 4), torch.ones(4)
    x16 = x32.to(dtype)
    st = torch.zeros(4, dtype=torch.float64)
    w = torch.zeros(4, 1, 3, 3)
    gate = torch.zeros(1, 4)
    with pytest.raises(AssertionError, match="bn_act_train_forward"):
        ops.bn_act_train_forward(x16, v, v, None, None, True, 0.1, 1e-5)
    with pytest.raises(AssertionError, match="dwconv_train_forward"):
        ops.dwconv_train_forward(x16, w, L.DW_SAME)
    with pytest.raises(AssertionError, match="se_scale_forward"):
        ops.se_scale_forward(x16, gate)
    for g, x in ((x32, x16), (x16, x32), (x16, x16)):
        with pytest.raises(AssertionError, match="bn_act_train_backward"):
            ops.bn_act_train_backward(g, x, st, st, v, v, True)
        with pytest.raises(AssertionError, match="dwconv_train_backward"):
            ops.dwconv_train_backward(g, x, w, L.DW_SAME)
        with pytest.raises(AssertionError, match="se_scale_backward"):
            ops.se_scale_backward(g, x, gate)
    with pytest.raises(AssertionError, match="one dtype per call"):      # the _io wrappers: one dtype for g and x
        ops.bn_act_train_backward_io(x32, x16, st, st, v, v, True)
    with pytest.raises(L.VqaeHipError):                  # fp32 CPU tensors pass the assertion and stop at the device check
        ops.se_scale_backward(x32, x32, gate)
    with pytest.raises(L.VqaeHipError):
        ops.se_scale_forward_io(x16, gate)


# ---- the reference's rounding points -------------------------------------------------------------------------------------------
class _Dtypes(torch.overrides.TorchFunctionMode):
    """Records (function name, dtype) of every floating tensor a torch function returns."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if isinstance(out, torch.Tensor) and out.is_floating_point():
            self.seen.append((getattr(func, "__name__", str(func)), out.dtype, out.dim()))
        return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", C.block_cases())
def test_stock_block_rounding_points(amd, case, dtype):
    """What the 16-bit nodes rest on: under CPU autocast EVERY activation of the stock block is 16-bit (conv outputs, BatchNorm,
    SiLU, the depthwise conv, the SE mean, the gate, the SE product, the residual sum of two 16-bit tensors); the running
    statistics and the parameter gradients, the depthwise weight's among them, stay fp32."""
    from vqae_amd.layers.mbconv_train import MBConv
    T = amd.train_mbconv
    block, x, g, _ = C.block_case(case, MBConv)
    x16 = x.to(dtype).requires_grad_()
    with _Dtypes() as rec, torch.autocast("cpu", dtype=dtype):
        y = T.block_forward_torch(block, x16)
    acts = [(name, dt) for name, dt, dim in rec.seen if dim in (2, 4) and name not in ("reshape", "__get__")]
    names = {name for name, _ in acts}
    assert {"conv2d", "batch_norm", "silu", "mean", "linear", "sigmoid", "mul", "add"} <= names, names
    assert all(dt == dtype for _, dt in acts), [a for a in acts if a[1] != dtype]
    assert y.dtype == dtype
    grads = torch.autograd.grad(y, [x16] + list(block.parameters()), g.to(dtype))
    assert grads[0].dtype == dtype and all(gp.dtype == torch.float32 for gp in grads[1:])
    assert block.branch[3].weight.dtype == torch.float32
    assert all(b.dtype == torch.float32 for n, b in block.named_buffers() if n.endswith(("running_mean", "running_var")))


@pytest.mark.parametrize("dtype", DTYPES)
def test_stock_batch_norm_rounds_once(dtype):
    """A 16-bit F.batch_norm on the CPU is bit for bit round(batch_norm_fp32(up(x))), running statistics included."""
    gen = torch.Generator().manual_seed(5)
    x = (torch.randn(3, 8, 5, 4, generator=gen) * 2 + 0.5).to(dtype)
    w, b = torch.randn(8, generator=gen), torch.randn(8, generator=gen)
    rm16, rv16, rm32, rv32 = torch.zeros(8), torch.ones(8), torch.zeros(8), torch.ones(8)
    y16 = F.batch_norm(x, rm16, rv16, w, b, True, 0.1, 1e-5)
    y32 = F.batch_norm(x.float(), rm32, rv32, w, b, True, 0.1, 1e-5)
    assert y16.dtype == dtype and torch.equal(y16, y32.to(dtype))
    # the statistics are fp32 sums either way, taken in another order by the 16-bit kernel: a few ulp of 2^-24 apart, and
    # 2^-9 (bf16) or 2^-12 (f16) away from what a statistic rounded to the 16-bit type would be
    assert rm16.dtype == rv16.dtype == torch.float32
    assert torch.allclose(rm16, rm32, rtol=1e-6, atol=1e-7) and torch.allclose(rv16, rv32, rtol=1e-6, atol=0)


# ---- dtype flow of the fused graph ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", C.block_cases())
def test_block_dtype_flow(amd, case, dtype, monkeypatch):
    from vqae_amd.layers.mbconv_train import MBConv
    T = amd.train_mbconv
    block, x, g, _ = C.block_case(case, MBConv)
    x = x.contiguous(memory_format=torch.channels_last)
    node_out = []
    for name in ("bn_act", "dwconv", "se_scale"):
        def wrap(*a, _f=getattr(T, name), _n=name, **k):
            out = _f(*a, **k)
            node_out.append((_n, a[0].dtype, (out[0] if isinstance(out, tuple) else out).dtype,
                             out[1].dtype if isinstance(out, tuple) else None))
            return out
        monkeypatch.setattr(T, name, wrap)
    saved = []
    before = dict(T.stats, **T.io16_stats)
    xr = x.detach().clone().requires_grad_()
    leaf = lambda t: t.is_leaf and t.requires_grad                         # the parameters and the input: fp32 by design
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append((t.dim(), t.dtype, leaf(t))), t)[1], lambda t: t):
        with torch.autocast("cpu", dtype=dtype):
            y = T.block_forward(block, xr)
            y_mod = block(xr.detach())                                     # the trainable _target_: the same graph
    assert dict(T.stats, **T.io16_stats) == before                         # CPU tensors: no kernel, nothing counted
    assert [n for n, *_ in node_out[:5]] == ["bn_act", "dwconv", "bn_act", "se_scale", "bn_act"]
    for name, din, dout, dpool in node_out:
        assert din == dtype and dout == dtype, (name, din, dout)           # 16 bits in, 16 bits out
        assert dpool in (None, torch.float32), (name, dpool)               # the pool is an fp32 sum of the unrounded values
    assert torch.equal(y, y_mod)
    # the identity skip adds the fp32 x of this test to a 16-bit branch (torch's promotion, as in the stock block)
    assert y.dtype == (torch.float32 if block.skip_conv is None else dtype)
    acts4 = [dt for dim, dt, is_leaf in saved if dim == 4 and not is_leaf]
    assert len(acts4) >= 8 and all(dt == dtype for dt in acts4), saved      # every saved activation is 16-bit
    grads = torch.autograd.grad(y, [xr] + list(block.parameters()), g.to(y.dtype))
    assert grads[0].dtype == torch.float32                                 # of the fp32 input
    assert all(gp.dtype == torch.float32 for gp in grads[1:])
    assert all(bool(torch.isfinite(gp).all()) for gp in grads)
    with torch.autocast("cpu", dtype=dtype):                               # a 16-bit x, the stack's residual stream, stays
        assert T.block_forward(block, x.to(dtype)).dtype == dtype
    assert T.block_forward(block, x).dtype == torch.float32                # no autocast: nothing changes


@pytest.mark.parametrize("dtype", DTYPES)
def test_node_restatements_round_once(amd, dtype):
    """Each CPU restatement on a 16-bit input is the fp32 restatement on the up-cast input, rounded once; sums stay fp32."""
    T, L = amd.train_mbconv, amd._lib
    gen = torch.Generator().manual_seed(11)
    x = (torch.randn(2, 4, 6, 8, generator=gen) * 1.5).to(dtype)
    g = torch.randn(2, 4, 6, 8, generator=gen).to(dtype)
    bn = torch.nn.BatchNorm2d(8).train()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(8, generator=gen)), bn.bias.copy_(torch.randn(8, generator=gen))
    bn32 = torch.nn.BatchNorm2d(8).train()
    bn32.load_state_dict(bn.state_dict())
    x16, x32 = x.clone().requires_grad_(), x.float().requires_grad_()
    with torch.autocast("cpu", dtype=dtype):
        y, pool = T.bn_act(x16, bn, silu=True, want_pool=True)
    y32, pool32 = T.bn_act(x32, bn32, silu=True, want_pool=True)
    assert y.dtype == dtype and pool.dtype == torch.float32
    assert torch.equal(y, y32.to(dtype)) and torch.equal(pool, pool32)
    assert torch.equal(bn.running_mean, bn32.running_mean) and torch.equal(bn.running_var, bn32.running_var)
    gp = torch.randn(2, 8, generator=gen)
    got = torch.autograd.grad([y, pool], [x16, bn.weight, bn.bias], [g, gp])
    want = torch.autograd.grad([y32, pool32], [x32, bn32.weight, bn32.bias], [g.float(), gp])
    assert got[0].dtype == dtype and torch.equal(got[0], want[0].to(dtype))
    assert got[1].dtype == torch.float32 and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    for mode, k, gs in (("same", 3, (2, 4, 6, 8)), ("down", 2, (2, 2, 3, 8)), ("up", 2, (2, 8, 12, 8))):
        w = torch.randn(8, 1, k, k, generator=gen).requires_grad_()
        wr = w.detach().to(dtype).float().requires_grad_()                 # the taps as autocast casts them
        gd = torch.randn(gs, generator=gen).to(dtype)
        with torch.autocast("cpu", dtype=dtype):
            yd = T.dwconv(x16, w, mode)
        yd32 = T.dwconv(x32, wr, mode)
        assert yd.dtype == dtype and torch.equal(yd, yd32.to(dtype)), mode
        got, want = torch.autograd.grad(yd, [x16, w], gd), torch.autograd.grad(yd32, [x32, wr], gd.float())
        assert got[0].dtype == dtype and torch.equal(got[0], want[0].to(dtype)), mode
        assert got[1].dtype == torch.float32 and torch.equal(got[1], want[1]), mode
    for gate in (torch.rand(2, 8, generator=gen), torch.rand(2, 8, generator=gen).to(dtype)):
        gate16, gate32 = gate.clone().requires_grad_(), gate.float().requires_grad_()
        ys, ys32 = T.se_scale(x16, gate16), T.se_scale(x32, gate32)
        assert ys.dtype == dtype and torch.equal(ys, ys32.to(dtype))
        got, want = torch.autograd.grad(ys, [x16, gate16], g), torch.autograd.grad(ys32, [x32, gate32], g.float())
        assert got[0].dtype == dtype and torch.equal(got[0], want[0].to(dtype))
        assert got[1].dtype == gate.dtype and torch.equal(got[1], want[1].to(gate.dtype))


# ---- distance to fp64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", C.block_cases())
def test_block_distance_to_fp64(amd, case, dtype):
    from conftest import record_parity
    from vqae_amd.layers.mbconv_train import MBConv
    T = amd.train_mbconv
    tag = "bf16" if dtype == BF16 else "f16"
    groups = {}
    for name, forward in (("dev", T.block_forward), ("stock", T.block_forward_torch)):
        block, x, g, ref = C.block_case(case, MBConv)
        res, pnames, bnames = results(block, x.contiguous(memory_format=torch.channels_last), g, under(forward, dtype))
        groups[name] = C.result_groups({k: v.float() for k, v in res.items()}, pnames, bnames)
    fails = []
    for k, (v64, _) in ref.items():
        got, stock = groups["dev"][k], groups["stock"][k]
        e_dev, e_ref = C.dist(got, v64.reshape(got.shape)), C.dist(stock, v64.reshape(stock.shape))
        print(f"mbconv_train16_cpu {tag} {case} {k}: e_dev {e_dev:.3e} e_ref {e_ref:.3e} ratio {e_dev / e_ref:.3f}")
        record_parity("mbconv_train16_cpu_block", dtype=tag, case=case, tensor=k, e_dev=e_dev, e_ref_stock_autocast=e_ref,
                      ratio=e_dev / e_ref)
        assert bool(torch.isfinite(got).all())
        if not e_dev <= BAR * e_ref:
            fails.append((k, e_dev, e_ref))
    assert not fails, fails


# ---- the fp32 / fp64 restatements are the parent's -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fp32_fp64_restatements_unchanged(amd, dtype):
    """On fp32 and fp64 inputs the CPU restatements give the bits of their formulas, restated here as they stood before the
    16-bit forms arrived -- with and without an autocast around them that their dtypes do not meet."""
    T, L = amd.train_mbconv, amd._lib
    gen = torch.Generator().manual_seed(17)
    B, H, W, Cc = 2, 4, 6, 8
    M = B * H * W
    x = torch.randn(B, H, W, Cc, generator=gen, dtype=dtype).requires_grad_()
    g = torch.randn(B, H, W, Cc, generator=gen, dtype=dtype)
    gp = torch.randn(B, Cc, generator=gen, dtype=dtype)
    bn = torch.nn.BatchNorm2d(Cc).to(dtype).train()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(Cc, generator=gen)), bn.bias.copy_(torch.randn(Cc, generator=gen))
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    y, pool = T.bn_act(x, bn, silu=True, want_pool=True)
    xd = x.detach()
    mean = xd.mean((0, 1, 2))
    var = ((xd - mean) ** 2).mean((0, 1, 2))
    invstd = torch.rsqrt(var + bn.eps)
    z = (xd - mean) * invstd * gamma + beta
    want = F.silu(z)
    assert y.dtype == dtype and torch.equal(y, want) and torch.equal(pool, want.sum((1, 2)))
    assert torch.equal(bn.running_mean, torch.zeros(Cc, dtype=dtype).mul_(0.9).add_(mean, alpha=0.1))
    assert torch.equal(bn.running_var, torch.ones(Cc, dtype=dtype).mul_(0.9).add_(var * (M / (M - 1)), alpha=0.1))
    gx, gg, gb = torch.autograd.grad([y, pool], [x, bn.weight, bn.bias], [g, gp])
    gf = g + gp.reshape(B, 1, 1, Cc)
    xhat = (xd - mean) * invstd
    d = gf * T.silu_grad(xhat * gamma + beta)
    w_gb, w_gg = d.sum((0, 1, 2)), (d * xhat).sum((0, 1, 2))
    assert torch.equal(gb, w_gb) and torch.equal(gg, w_gg)
    assert torch.equal(gx, gamma * invstd * (d - w_gb / M - xhat * (w_gg / M)))
    for mode, k, gs in (("same", 3, (B, H, W, Cc)), ("down", 2, (B, H // 2, W // 2, Cc)), ("up", 2, (B, 2 * H, 2 * W, Cc))):
        w = torch.randn(Cc, 1, k, k, generator=gen, dtype=dtype).requires_grad_()
        gd = torch.randn(gs, generator=gen, dtype=dtype)
        yd = T.dwconv(x, w, mode)
        m = T.DW_MODES[mode]
        xc, wd = xd.permute(0, 3, 1, 2), w.detach()
        if mode == "same":
            want = F.conv2d(T.pad_circular_nhwc(xd).permute(0, 3, 1, 2), wd, groups=Cc)
        elif mode == "down":
            want = F.conv2d(xc, wd, stride=2, groups=Cc)
        else:
            want = F.conv_transpose2d(xc, wd, stride=2, groups=Cc)
        assert yd.dtype == dtype and torch.equal(yd, want.permute(0, 2, 3, 1).contiguous()), mode
        got = torch.autograd.grad(yd, [x, w], gd)
        want = T._dw_backward_torch(gd, xd, w.detach(), m, True, True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), mode
    gate = torch.rand(B, Cc, generator=gen, dtype=dtype).requires_grad_()
    ys = T.se_scale(x, gate)
    assert torch.equal(ys, xd * gate.detach().reshape(B, 1, 1, Cc))
    got = torch.autograd.grad(ys, [x, gate], g)
    assert torch.equal(got[0], g * gate.detach().reshape(B, 1, 1, Cc)) and torch.equal(got[1], (g * xd).sum((1, 2)))
