"""CPU: the trainable 2x2, stride-2 conv node of vqae_amd.train (conv_down / _ConvDownFn) through its plain-torch restatement
-- the same forward and the same hand-derived backward csrc/conv_train.hip implements (tests/test_conv_down_train_gpu.py
runs the kernels).

  * torch.autograd.gradcheck of the restatement in fp64 for pre = 0 (u = x), 1 (u = x + b) and 2 (u = ELU(x + a) + b), for a
    contiguous and a channels_last weight, and with a frozen input or weight;
  * fixture case down_8_16_4x6 under conv_down="hip" on CPU tensors: the forward is the "torch" route's bit for bit (the
    restatement calls the same F.conv2d on the same u); the gradients differ by fp32 re-association only -- the fused node
    forms g_u and g_w as space-to-depth matmuls where the torch route has the convolution's own backward, the same products in
    another order -- so ||hip - torch|| / ||g64|| <= 4 e_ref and dist(hip, g64) <= 4 e_ref per tensor group, e_ref the
    fixture's own fp32-to-fp64 distance (the bound and its reasoning are tests/test_conv1x1_train_cpu.py's);
  * odd H takes the fall-back and is counted; the default keyword is the parent's graph bit for bit on every fixture case;
  * the C ABI's errors that are returned before any HIP call.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import fixup_train_cases as C

BAR = 4.0
CASE = "down_8_16_4x6"


def _p(v):
    return torch.tensor([v], dtype=torch.float64, requires_grad=True)


def _weight(co, ci, gen, channels_last):
    w = torch.randn(co, ci, 2, 2, dtype=torch.float64, generator=gen) / (4 * ci) ** 0.5
    if channels_last:
        w = w.contiguous(memory_format=torch.channels_last)
        assert not w.is_contiguous()
    return w.requires_grad_()


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("pre", [0, 1, 2])
def test_gradcheck_restatement(amd, pre, channels_last):
    T = amd.train
    gen = torch.Generator().manual_seed(pre)
    B, H, W, Ci, Co = 2, 4, 6, 8, 16
    x = torch.randn(B, H, W, Ci, dtype=torch.float64, generator=gen, requires_grad=True)
    w = _weight(Co, Ci, gen, channels_last)
    if pre == 0:
        assert torch.autograd.gradcheck(lambda x, w: T.conv_down(x, w), (x, w))
        args = ()
    elif pre == 1:
        assert torch.autograd.gradcheck(lambda x, w, b: T.conv_down(x, w, None, b), (x, w, _p(-0.2)))
        args = (None, _p(-0.2))
    else:
        assert torch.autograd.gradcheck(lambda x, w, a, b: T.conv_down(x, w, a, b), (x, w, _p(0.3), _p(-0.2)))
        args = (_p(0.3), _p(-0.2))
    y = T.conv_down(x, w, *args)
    assert y.shape == (B, H // 2, W // 2, Co)
    u = x if pre == 0 else x + args[1] if pre == 1 else F.elu(x + args[0]) + args[1]
    want = F.conv2d(u.permute(0, 3, 1, 2), w, stride=2).permute(0, 2, 3, 1)
    assert torch.equal(y, want)
    (g_w,) = torch.autograd.grad(y.sum(), [w])
    assert g_w.shape == w.shape and g_w.stride() == w.stride()           # the weight's own memory format


def test_restatement_frozen_inputs(amd):
    """needs_input_grad is honoured: a frozen weight or input gets no gradient and the other one is unchanged."""
    T = amd.train
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(1, 2, 4, 8, dtype=torch.float64, generator=gen)
    w = torch.randn(8, 8, 2, 2, dtype=torch.float64, generator=gen)
    a, b = _p(0.1), _p(0.2)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    gx, gw = torch.autograd.grad(T.conv_down(xr, wr, a, b).sum(), [xr, wr])
    (gx1,) = torch.autograd.grad(T.conv_down(xr, w, a, b).sum(), [xr])
    (gw1,) = torch.autograd.grad(T.conv_down(x, wr, a, b).sum(), [wr])
    assert torch.equal(gx, gx1) and torch.equal(gw, gw1)
    assert torch.autograd.gradcheck(lambda x: T.conv_down(x, w, a, b), (xr,))
    assert torch.autograd.gradcheck(lambda w: T.conv_down(x, w, a, b), (wr,))


def test_down_block_hip_route_on_cpu(amd):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    block, x, g, ref = C.block_case(CASE, PreActFixupResBlock)
    assert block.mode == "down" and block.skip_conv is not None
    x = x.contiguous(memory_format=torch.channels_last)
    T.stats.update(conv_down_hip=0, conv_down_fallbacks=0, conv1x1_hip=0, conv1x1_fallbacks=0)
    hip = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv_down="hip"))
    assert (T.stats["conv_down_hip"], T.stats["conv_down_fallbacks"]) == (2, 0)
    assert (T.stats["conv1x1_hip"], T.stats["conv1x1_fallbacks"]) == (0, 0)              # the keywords are independent
    tor = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv_down="torch"))
    assert (T.stats["conv_down_hip"], T.stats["conv_down_fallbacks"]) == (2, 0)          # the torch route counts nothing
    assert torch.equal(hip["out"], tor["out"])
    for k, (v64, e_ref) in ref.items():
        d = float((hip[k].double() - tor[k].double()).norm() / v64.double().norm())
        print(f"{CASE} {k}: |hip - torch| / |g64| {d:.2e}  e_ref {e_ref:.2e}")
        assert d <= BAR * e_ref, (k, d, e_ref)
        assert C.dist(hip[k], v64.reshape(hip[k].shape)) <= BAR * e_ref, k
    both = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv1x1="hip", conv_down="hip"))
    assert torch.equal(both["out"], tor["out"])
    assert (T.stats["conv_down_hip"], T.stats["conv1x1_hip"]) == (4, 2)
    # a channels_last weight (what the reference trains with): the same node, the gradient in the weight's format
    blk2 = PreActFixupResBlock(8, 16, "down", conv_down="hip")
    blk2.load_state_dict(block.state_dict())
    for conv in (blk2.branch_conv2, blk2.skip_conv):
        conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
    cl = C.block_results(blk2, x, g, lambda b, t: b(t))
    assert cl["branch_conv2.weight"].numel() == block.branch_conv2.weight.numel()
    for k, (v64, e_ref) in ref.items():
        assert C.dist(cl[k], v64.reshape(cl[k].shape)) <= BAR * e_ref, k


def test_odd_height_takes_the_fallback(amd):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    torch.manual_seed(1)
    block = PreActFixupResBlock(8, 16, "down", n_layers=4)
    gen = torch.Generator().manual_seed(2)
    for shape, want in (((1, 8, 5, 6), (0, 2)), ((1, 8, 4, 7), (0, 2)), ((1, 8, 4, 6), (2, 0))):
        x = torch.randn(shape, generator=gen)
        T.stats.update(conv_down_hip=0, conv_down_fallbacks=0)
        y = T.block_forward(block, x, conv_down="hip")
        assert (T.stats["conv_down_hip"], T.stats["conv_down_fallbacks"]) == want, shape
        assert torch.equal(y, T.block_forward(block, x)) and y.shape == (1, 16, shape[2] // 2, shape[3] // 2)
    # channel counts outside the kernels' rule
    small = PreActFixupResBlock(4, 8, "down", n_layers=4)
    T.stats.update(conv_down_hip=0, conv_down_fallbacks=0)
    T.block_forward(small, torch.randn(1, 4, 4, 4, generator=gen), conv_down="hip")
    assert (T.stats["conv_down_hip"], T.stats["conv_down_fallbacks"]) == (1, 1)          # branch_conv2 8 -> 8 fused, skip 4 -> 8 not


def test_default_route_is_torch(amd):
    """With the keyword at its default, or "torch", every fixture case gives the bits of the graph written out with the ops
    the module has always used for a 'down' block (fixup_act / fixup_add, then F.conv2d stride 2)."""
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train

    def parent_graph(block, xn):
        x = T.to_nhwc(xn)
        conv = lambda t, w, **kw: T.to_nhwc(F.conv2d(T.to_nchw(t), w, **kw))
        t = conv(T.fixup_act(x, block.bias1a, block.bias1b), block.branch_conv1.weight)
        t = conv(T.fixup_act(t, block.bias2a, block.bias2b), block.branch_conv2.weight, stride=2)
        t = conv(T.fixup_act(t, block.bias3a, block.bias3b), block.branch_conv3.weight)
        skip = conv(T.fixup_add(x, block.bias1c), block.skip_conv.weight, stride=2)
        return T.to_nchw(T.fixup_out(t, skip, block.scale, block.bias4, block.bias1d))

    T.stats.update(conv_down_hip=0, conv_down_fallbacks=0)
    for case in C.block_cases():
        block, x, g, _ = C.block_case(case, PreActFixupResBlock)
        assert block.conv_down == "torch" and block.conv1x1 == "torch"
        d = C.block_results(block, x, g, T.block_forward)
        t = C.block_results(block, x, g, lambda b, v: T.block_forward(b, v, conv_down="torch"))
        m = C.block_results(block, x, g, lambda b, v: b(v))
        for k in d:
            assert torch.equal(d[k], t[k]) and torch.equal(d[k], m[k]), (case, k)
        if block.mode == "down":
            p = C.block_results(block, x, g, parent_graph)
            for k in d:
                assert torch.equal(d[k], p[k]), (case, k)
    assert (T.stats["conv_down_hip"], T.stats["conv_down_fallbacks"]) == (0, 0)
    with pytest.raises(ValueError):
        T.block_forward(block, x, conv_down="triton")
    with pytest.raises(ValueError):
        T.forward_train(None, x, conv_down="miopen")
    with pytest.raises(ValueError):
        PreActFixupResBlock(8, 16, "down", conv_down="miopen")
    blk = PreActFixupResBlock(8, 16, "down", conv_down="hip")
    assert blk.conv_down == "hip" and blk.conv1x1 == "torch"
    assert functools.partial(PreActFixupResBlock, conv1x1="hip", conv_down="hip")(8, 16, "down").conv1x1 == "hip"


def test_forward_train_keyword_on_cpu(amd):
    """forward_train / step pass the keyword down: under "hip" the first step's output is the torch route's, and the two
    'down' blocks of spec tiny (8 -> 16, 16 -> 32) give four fused nodes."""
    T = amd.train
    model, batches = C.loop_model()
    x = batches[0].contiguous(memory_format=torch.channels_last)
    model.eval()                                           # no EMA update: both calls see the same quantiser
    T.stats.update(conv_down_hip=0, conv_down_fallbacks=0, conv1x1_hip=0)
    out_h, rec_h, (vq_h,) = T.step(model, x, conv_down="hip")
    assert (T.stats["conv_down_hip"], T.stats["conv_down_fallbacks"], T.stats["conv1x1_hip"]) == (4, 0, 0)
    out_t, rec_t, (vq_t,) = T.step(model, x)
    assert torch.equal(out_h, out_t) and torch.equal(rec_h, rec_t) and torch.equal(vq_h, vq_t)
    out_b, _, _ = T.step(model, x, conv1x1="hip", conv_down="hip")
    assert torch.equal(out_b, out_t) and T.stats["conv_down_hip"] == 8 and T.stats["conv1x1_hip"] > 0
    (rec_h + vq_h).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_abi_errors_before_any_hip_call(amd):
    L = amd._lib
    lib = L.lib()
    one = ctypes.c_void_p(4096)
    odd = ctypes.c_void_p(4096 + 8)
    fwd, bwd = lib.vqae_conv_down_train_forward_f32, lib.vqae_conv_down_train_backward_f32

    def f(x=one, a=one, b=one, pre=2, w=one, lay=1, B=2, H=4, W=6, ci=8, co=16, y=one, ws=one):
        return fwd(x, a, b, pre, w, lay, B, H, W, ci, co, y, ws, None)

    def r(g=one, x=one, a=one, b=one, pre=2, w=one, lay=1, B=2, H=4, W=6, ci=8, co=16, gx=one, gw=one, ga=one, gb=one, ws=one):
        return bwd(g, x, a, b, pre, w, lay, B, H, W, ci, co, gx, gw, ga, gb, ws, None)

    INVALID, UNSUPPORTED = -1, -2
    # null pointers
    for kw in ({"x": None}, {"a": None}, {"b": None}, {"b": None, "pre": 1}, {"w": None}, {"y": None}, {"ws": None, "lay": 0}):
        assert f(**kw) == INVALID, kw
    with pytest.raises(AssertionError):
        L.check(f(x=None))
    for kw in ({"g": None}, {"x": None}, {"a": None}, {"b": None}, {"w": None}, {"ws": None}):
        assert r(**kw) == INVALID, kw
    # misaligned pointers: tensors 16 bytes, the workspace 8
    for kw in ({"x": odd}, {"w": odd}, {"y": odd}, {"ws": ctypes.c_void_p(4100), "lay": 0}):
        assert f(**kw) == INVALID, kw
    for kw in ({"g": odd}, {"x": odd}, {"w": odd}, {"gx": odd}, {"gw": odd}, {"ws": ctypes.c_void_p(4100)}):
        assert r(**kw) == INVALID, kw
    # pre, w_layout, sizes
    for kw in ({"pre": 3}, {"pre": -1}, {"lay": 2}, {"lay": -1}, {"B": 0}, {"H": 0}, {"W": 0}, {"B": -1}, {"H": -2},
               {"B": 2 ** 40, "H": 2, "W": 2}):
        assert f(**kw) == INVALID, kw
        assert r(**kw) == INVALID, kw
    # channel counts outside the rule, odd H / W
    for ci, co in ((12, 8), (8, 264), (8, 12), (264, 8), (0, 8), (8, 4)):
        assert lib.vqae_conv_down_train_supported(ci, co) == 0 and not amd.ops.conv_down_train_supported(ci, co)
        assert f(ci=ci, co=co) == UNSUPPORTED and r(ci=ci, co=co) == UNSUPPORTED
        assert lib.vqae_conv_down_train_workspace_bytes(2, 4, 6, ci, co) == 0
    with pytest.raises(NotImplementedError):
        L.check(f(ci=12))
    for kw in ({"H": 5}, {"W": 7}, {"H": 1}, {"W": 1}):
        assert f(**kw) == UNSUPPORTED and r(**kw) == UNSUPPORTED, kw
    assert lib.vqae_conv_down_train_workspace_bytes(2, 5, 6, 8, 16) == 0
    assert lib.vqae_conv_down_train_workspace_bytes(0, 4, 6, 8, 16) == 0
    assert lib.vqae_conv_down_train_workspace_bytes(2 ** 40, 2, 2, 8, 16) == 0
    # answers that need no GPU
    for ci, co in ((8, 8), (8, 16), (24, 40), (256, 256), (128, 8)):
        assert lib.vqae_conv_down_train_supported(ci, co) == 1 and amd.ops.conv_down_train_supported(ci, co)
        for B, H, W in ((1, 2, 2), (3, 14, 98), (16, 256, 256), (2 ** 19, 2048, 2048)):
            n = lib.vqae_conv_down_train_workspace_bytes(B, H, W, ci, co)
            assert n > 0 and n % 8 == 0
            # bounded whatever the number of rows: the documented 16 MiB of partials + 1 MiB of weight + the scalar rows
            assert n <= (16 << 20) + (1 << 20) + 4096 * 16 + 256
        assert (lib.vqae_conv_down_train_workspace_bytes(2 ** 19, 2048, 2048, ci, co)
                == lib.vqae_conv_down_train_workspace_bytes(2 ** 10, 2048, 2048, ci, co))
    R = lib.vqae_conv_down_train_wgrad_run()
    assert R >= 64 and R == amd.ops.conv_down_train_wgrad_run()
    with pytest.raises(amd._lib.VqaeHipError):
        amd.ops.conv_down_train_forward(torch.zeros(1, 2, 2, 8), torch.zeros(8, 8, 2, 2))
