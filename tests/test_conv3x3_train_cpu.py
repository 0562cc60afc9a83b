"""CPU: the trainable circular 3x3 conv node of vqae_amd.train (conv3x3 / _Conv3x3Fn) through its plain-torch restatement -- the
same forward and the same hand-derived backward the Circ3x3 policy of csrc/conv_train.hip implements
(tests/test_conv3x3_train_gpu.py runs the kernels).

  * torch.autograd.gradcheck of the restatement in fp64 for pre = 0 (u = x), 1 (u = x + b) and 2 (u = ELU(x + a) + b), for a
    contiguous and a channels_last weight, at H x W = 4 x 5 and at the wrap cases 1 x 3, 2 x 1, 1 x 1, 2 x 2 (at H = 1 all three kh
    read the same row), and with a frozen input or weight;
  * every 'same' / 'out' fixture case under conv3x3="hip" on CPU tensors: the forward is the "torch" route's bit for bit (the
    restatement calls the same F.conv2d on the same circularly padded u); the gradients differ by fp32 re-association only --
    the fused node folds a conv_transpose and forms g_w as one matmul on unfolded patches where the torch route has the
    convolution's own backward, the same products in another order -- so ||hip - torch|| / ||g64|| <= 4 e_ref and
    dist(hip, g64) <= 4 e_ref per tensor group, e_ref the fixture's own fp32-to-fp64 distance (the bound and its reasoning are
    tests/test_conv1x1_train_cpu.py's);
  * a block of branch width 4 takes the fall-back and is counted; the default keyword is the parent's graph bit for bit on
    every fixture case; an invalid keyword raises ValueError;
  * the C ABI's errors that are returned before any HIP call.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import fixup_train_cases as C

BAR = 4.0
CASES = ["same_8_4x6", "same_8_1x1", "same_8_2x2", "sameskip_8_16_3x5", "outskip_8_3_4x4"]
KEYS = ("conv3x3_hip", "conv3x3_fallbacks", "conv1x1_hip", "conv1x1_fallbacks", "conv_down_hip", "conv_down_fallbacks")


def _p(v):
    return torch.tensor([v], dtype=torch.float64, requires_grad=True)


def _weight(co, ci, gen, channels_last):
    w = torch.randn(co, ci, 3, 3, dtype=torch.float64, generator=gen) / (9 * ci) ** 0.5
    if channels_last:
        w = w.contiguous(memory_format=torch.channels_last)
        assert not w.is_contiguous()
    return w.requires_grad_()


def _counts(T):
    return tuple(T.stats[k] for k in KEYS)


def _reset(T):
    T.stats.update({k: 0 for k in KEYS})


def test_fixture_has_the_cases():
    assert set(CASES) <= set(C.block_cases())


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("pre", [0, 1, 2])
@pytest.mark.parametrize("hw", [(4, 5), (1, 3), (2, 1), (1, 1), (2, 2)])
def test_gradcheck_restatement(amd, hw, pre, channels_last):
    T = amd.train
    gen = torch.Generator().manual_seed(pre + 10 * hw[0] + hw[1])
    B, (H, W), Ci, Co = 2, hw, 8, 16
    x = torch.randn(B, H, W, Ci, dtype=torch.float64, generator=gen, requires_grad=True)
    w = _weight(Co, Ci, gen, channels_last)
    if pre == 0:
        assert torch.autograd.gradcheck(lambda x, w: T.conv3x3(x, w), (x, w))
        args = ()
    elif pre == 1:
        assert torch.autograd.gradcheck(lambda x, w, b: T.conv3x3(x, w, None, b), (x, w, _p(-0.2)))
        args = (None, _p(-0.2))
    else:
        assert torch.autograd.gradcheck(lambda x, w, a, b: T.conv3x3(x, w, a, b), (x, w, _p(0.3), _p(-0.2)))
        args = (_p(0.3), _p(-0.2))
    y = T.conv3x3(x, w, *args)
    assert y.shape == (B, H, W, Co)
    u = x if pre == 0 else x + args[1] if pre == 1 else F.elu(x + args[0]) + args[1]
    # bit for bit what the torch route computes (the same F.conv2d on the same channel-last padded u); F.pad lays the padded
    # tensor out differently, and F.conv2d then sums in another order: equal to fp64 rounding
    assert torch.equal(y, F.conv2d(T.to_nchw(T.pad_circular_nhwc(u)), w).permute(0, 2, 3, 1))
    want = F.conv2d(F.pad(u.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="circular"), w).permute(0, 2, 3, 1)
    assert torch.allclose(y, want, rtol=1e-12, atol=1e-12)
    # the hand-derived gradients against autograd's of the stock ops
    g = torch.randn(y.shape, dtype=torch.float64, generator=gen)
    mine = torch.autograd.grad(y, [x, w], g)
    stock = torch.autograd.grad(want, [x, w], g)
    for p, q in zip(mine, stock):
        assert torch.allclose(p, q, rtol=1e-12, atol=1e-12)
    assert mine[1].shape == w.shape and mine[1].stride() == w.stride()   # the weight's own memory format


def test_restatement_frozen_inputs(amd):
    """needs_input_grad is honoured: a frozen weight or input gets no gradient and the other one is unchanged."""
    T = amd.train
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(1, 2, 3, 8, dtype=torch.float64, generator=gen)
    w = torch.randn(8, 8, 3, 3, dtype=torch.float64, generator=gen)
    a, b = _p(0.1), _p(0.2)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    gx, gw = torch.autograd.grad(T.conv3x3(xr, wr, a, b).sum(), [xr, wr])
    (gx1,) = torch.autograd.grad(T.conv3x3(xr, w, a, b).sum(), [xr])
    (gw1,) = torch.autograd.grad(T.conv3x3(x, wr, a, b).sum(), [wr])
    assert torch.equal(gx, gx1) and torch.equal(gw, gw1)
    assert torch.autograd.gradcheck(lambda x: T.conv3x3(x, w, a, b), (xr,))
    assert torch.autograd.gradcheck(lambda w: T.conv3x3(x, w, a, b), (wr,))


@pytest.mark.parametrize("case", CASES)
def test_block_hip_route_on_cpu(amd, case):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    block, x, g, ref = C.block_case(case, PreActFixupResBlock)
    assert block.mode in ("same", "out")
    x = x.contiguous(memory_format=torch.channels_last)
    _reset(T)
    hip = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv3x3="hip"))
    assert _counts(T) == (1, 0, 0, 0, 0, 0)                                # the keywords are independent
    tor = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv3x3="torch"))
    assert _counts(T) == (1, 0, 0, 0, 0, 0)                                # the torch route counts nothing
    assert torch.equal(hip["out"], tor["out"])
    for k, (v64, e_ref) in ref.items():
        d = float((hip[k].double() - tor[k].double()).norm() / v64.double().norm())
        print(f"{case} {k}: |hip - torch| / |g64| {d:.2e}  e_ref {e_ref:.2e}")
        assert d <= BAR * e_ref, (k, d, e_ref)
        assert C.dist(hip[k], v64.reshape(hip[k].shape)) <= BAR * e_ref, k
    every = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv1x1="hip", conv_down="hip", conv3x3="hip"))
    assert torch.equal(every["out"], tor["out"])
    assert T.stats["conv3x3_hip"] == 2 and T.stats["conv1x1_hip"] > 0 and T.stats["conv_down_hip"] == 0
    # a channels_last weight (what the reference trains with): the same node, the gradient in the weight's format
    blk2 = PreActFixupResBlock(block.in_channels, block.out_channels, block.mode, conv3x3="hip")
    blk2.load_state_dict(block.state_dict())
    blk2.branch_conv2.weight.data = blk2.branch_conv2.weight.data.contiguous(memory_format=torch.channels_last)
    cl = C.block_results(blk2, x, g, lambda b, t: b(t))
    assert torch.equal(cl["out"], tor["out"])
    for k, (v64, e_ref) in ref.items():
        assert C.dist(cl[k], v64.reshape(cl[k].shape)) <= BAR * e_ref, k


def test_narrow_branch_takes_the_fallback(amd):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    torch.manual_seed(1)
    gen = torch.Generator().manual_seed(2)
    for cin, cout, mode, want in ((4, 4, "same", (0, 1)), (4, 3, "out", (0, 1)), (8, 8, "same", (1, 0)), (8, 3, "out", (1, 0))):
        block = PreActFixupResBlock(cin, cout, mode, n_layers=4)
        assert block.branch_channels == max(cin, cout)
        x = torch.randn((1, cin, 3, 4), generator=gen)
        _reset(T)
        y = T.block_forward(block, x, conv3x3="hip")
        assert _counts(T)[:2] == want, (cin, cout, mode)                   # the zero-padded 3x3 skip of 'out' is no candidate
        assert torch.equal(y, T.block_forward(block, x)) and y.shape == (1, cout, 3, 4)


def test_default_route_is_torch(amd):
    """With the keyword at its default, or "torch", every fixture case gives the bits of the graph written out with the ops
    the module has always used for a 'same' / 'out' block (fixup_act with the halo, then F.conv2d without padding)."""
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train

    def parent_graph(block, xn):
        x = T.to_nhwc(xn)
        conv = lambda t, w, **kw: T.to_nhwc(F.conv2d(T.to_nchw(t), w, **kw))
        t = conv(T.fixup_act(x, block.bias1a, block.bias1b), block.branch_conv1.weight)
        t = conv(T.fixup_act(t, block.bias2a, block.bias2b, halo=1), block.branch_conv2.weight)
        t = conv(T.fixup_act(t, block.bias3a, block.bias3b), block.branch_conv3.weight)
        if block.skip_conv is None:
            return T.to_nchw(T.fixup_out(t, x, block.scale, block.bias4))
        skip = conv(T.fixup_add(x, block.bias1c), block.skip_conv.weight, padding=1 if block.mode == "out" else 0)
        return T.to_nchw(T.fixup_out(t, skip, block.scale, block.bias4, block.bias1d))

    _reset(T)
    for case in C.block_cases():
        block, x, g, _ = C.block_case(case, PreActFixupResBlock)
        assert (block.conv3x3, block.conv_down, block.conv1x1) == ("torch",) * 3
        d = C.block_results(block, x, g, T.block_forward)
        t = C.block_results(block, x, g, lambda b, v: T.block_forward(b, v, conv3x3="torch"))
        m = C.block_results(block, x, g, lambda b, v: b(v))
        for k in d:
            assert torch.equal(d[k], t[k]) and torch.equal(d[k], m[k]), (case, k)
        if block.mode in ("same", "out"):
            p = C.block_results(block, x, g, parent_graph)
            for k in d:
                assert torch.equal(d[k], p[k]), (case, k)
    assert _counts(T) == (0,) * 6
    with pytest.raises(ValueError):
        T.block_forward(block, x, conv3x3="triton")
    with pytest.raises(ValueError):
        T.block_forward_nhwc(block, x, conv3x3="miopen")
    with pytest.raises(ValueError):
        T.forward_train(None, x, conv3x3="miopen")
    with pytest.raises(ValueError):
        T.step(None, x, conv3x3="")
    with pytest.raises(ValueError):
        PreActFixupResBlock(8, 8, "same", conv3x3="miopen")
    blk = PreActFixupResBlock(8, 8, "same", conv3x3="hip")
    assert (blk.conv3x3, blk.conv1x1, blk.conv_down) == ("hip", "torch", "torch")
    assert functools.partial(PreActFixupResBlock, conv1x1="hip", conv3x3="hip")(8, 8, "same").conv1x1 == "hip"


def test_forward_train_keyword_on_cpu(amd):
    """forward_train / step pass the keyword down: under "hip" the first step's output is the torch route's."""
    T = amd.train
    model, batches = C.loop_model()
    x = batches[0].contiguous(memory_format=torch.channels_last)
    model.eval()                                           # no EMA update: both calls see the same quantiser
    _reset(T)
    out_h, rec_h, (vq_h,) = T.step(model, x, conv3x3="hip")
    n = T.stats["conv3x3_hip"]
    assert n > 0 and _counts(T)[1:] == (0,) * 5
    out_t, rec_t, (vq_t,) = T.step(model, x)
    assert T.stats["conv3x3_hip"] == n
    assert torch.equal(out_h, out_t) and torch.equal(rec_h, rec_t) and torch.equal(vq_h, vq_t)
    out_b, _, _ = T.step(model, x, conv1x1="hip", conv_down="hip", conv3x3="hip")
    assert torch.equal(out_b, out_t) and T.stats["conv3x3_hip"] == 2 * n
    assert T.stats["conv1x1_hip"] > 0 and T.stats["conv_down_hip"] == 4
    (rec_h + vq_h).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_abi_errors_before_any_hip_call(amd):
    L = amd._lib
    lib = L.lib()
    one = ctypes.c_void_p(4096)
    odd = ctypes.c_void_p(4096 + 8)
    fwd, bwd = lib.vqae_conv3x3_train_forward_f32, lib.vqae_conv3x3_train_backward_f32

    def f(x=one, a=one, b=one, pre=2, w=one, lay=1, B=2, H=4, W=5, ci=8, co=16, y=one, ws=one):
        return fwd(x, a, b, pre, w, lay, B, H, W, ci, co, y, ws, None)

    def r(g=one, x=one, a=one, b=one, pre=2, w=one, lay=1, B=2, H=4, W=5, ci=8, co=16, gx=one, gw=one, ga=one, gb=one, ws=one):
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
    # pre, w_layout, geometry
    for kw in ({"pre": 3}, {"pre": -1}, {"lay": 2}, {"lay": -1}, {"B": 0}, {"H": 0}, {"W": 0}, {"B": -1}, {"H": -2}, {"W": -1},
               {"B": 2 ** 40, "H": 1, "W": 1}, {"B": 2 ** 20, "H": 2 ** 10, "W": 2 ** 10}, {"B": 2 ** 62, "H": 4, "W": 4}):
        assert f(**kw) == INVALID, kw
        assert r(**kw) == INVALID, kw
    # channel counts outside the rule
    for ci, co in ((12, 8), (8, 264), (8, 12), (264, 8), (0, 8), (8, 4), (3, 8), (8, 3)):
        assert lib.vqae_conv3x3_train_supported(ci, co) == 0 and not amd.ops.conv3x3_train_supported(ci, co)
        assert f(ci=ci, co=co) == UNSUPPORTED and r(ci=ci, co=co) == UNSUPPORTED
        assert lib.vqae_conv3x3_train_workspace_bytes(2, 4, 5, ci, co) == 0
    with pytest.raises(NotImplementedError):
        L.check(f(ci=12))
    assert lib.vqae_conv3x3_train_workspace_bytes(0, 4, 6, 8, 16) == 0
    assert lib.vqae_conv3x3_train_workspace_bytes(2, 0, 6, 8, 16) == 0
    assert lib.vqae_conv3x3_train_workspace_bytes(2 ** 40, 1, 1, 8, 16) == 0
    # answers that need no GPU
    for ci, co in ((8, 8), (8, 16), (24, 40), (256, 256), (128, 8)):
        assert lib.vqae_conv3x3_train_supported(ci, co) == 1 and amd.ops.conv3x3_train_supported(ci, co)
        for B, H, W in ((1, 1, 1), (3, 7, 49), (16, 256, 256), (2 ** 17, 2048, 2048)):
            n = lib.vqae_conv3x3_train_workspace_bytes(B, H, W, ci, co)
            assert n > 0 and n % 8 == 0
            # the documented bound whatever the number of rows: 32 MiB of partials + two weights of 2.25 MiB + the scalar rows
            assert n <= (32 << 20) + 2 * 9 * (256 * 256 * 4) + 1024 * 16 + 256
        assert (lib.vqae_conv3x3_train_workspace_bytes(2 ** 17, 2048, 2048, ci, co)
                == lib.vqae_conv3x3_train_workspace_bytes(2 ** 10, 2048, 2048, ci, co))
    R = lib.vqae_conv3x3_train_wgrad_run()
    assert R >= 64 and R == amd.ops.conv3x3_train_wgrad_run()
    with pytest.raises(amd._lib.VqaeHipError):
        amd.ops.conv3x3_train_forward(torch.zeros(1, 2, 2, 8), torch.zeros(8, 8, 3, 3))
