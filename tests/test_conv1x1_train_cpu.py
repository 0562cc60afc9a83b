"""CPU: the trainable 1x1 conv node of vqae_amd.train (conv1x1 / _Conv1x1Fn) through its plain-torch restatement -- the same
forward and the same hand-derived backward csrc/conv_train.hip implements (tests/test_conv1x1_train_gpu.py runs the kernels).

  * torch.autograd.gradcheck of the restatement in fp64 for pre = 0 (u = x), 1 (u = x + b) and 2 (u = ELU(x + a) + b);
  * block_forward(..., conv1x1="hip") on CPU tensors against the "torch" route on every case of tests/fixup_train_cases.py:
    the forward is equal (the restatement calls the same F.conv2d on the same u), the gradients differ by fp32
    re-association only.  Bound: the fused node forms g_u = g . w and g_w = g^T . u as matmuls where the torch route has
    the convolution's own backward, i.e. the same products summed in another order.  Two fp32 evaluations of one sum of K
    products are each within (K + 1) u sum|terms| of it (u = 2^-24), and norm-wise every gradient of a block is such a sum
    passed through a few more of them, so each route is at e_ref -- the fixture's own fp32-to-fp64 distance of that
    tensor -- times a small constant from the fp64 value.  The assertion: ||hip - torch|| / ||g64|| <= 4 e_ref per tensor
    (the project's bar for the same products in another order), one-element tensors as one vector;
  * the keyword's default is "torch", bit for bit;
  * the C ABI's errors that are returned before any HIP call.
"""
import ctypes

import pytest
import torch

import fixup_train_cases as C

BAR = 4.0


def _p(v):
    return torch.tensor([v], dtype=torch.float64, requires_grad=True)


@pytest.mark.parametrize("pre", [0, 1, 2])
def test_gradcheck_restatement(amd, pre):
    T = amd.train
    gen = torch.Generator().manual_seed(pre)
    B, H, W, Ci, Co = 2, 2, 3, 8, 16
    x = torch.randn(B, H, W, Ci, dtype=torch.float64, generator=gen, requires_grad=True)
    w = (torch.randn(Co, Ci, 1, 1, dtype=torch.float64, generator=gen) / Ci ** 0.5).requires_grad_()
    if pre == 0:
        assert torch.autograd.gradcheck(lambda x, w: T.conv1x1(x, w), (x, w))
    elif pre == 1:
        assert torch.autograd.gradcheck(lambda x, w, b: T.conv1x1(x, w, None, b), (x, w, _p(-0.2)))
    else:
        assert torch.autograd.gradcheck(lambda x, w, a, b: T.conv1x1(x, w, a, b), (x, w, _p(0.3), _p(-0.2)))
    y = T.conv1x1(x, w, *((_p(0.3), _p(-0.2)) if pre == 2 else (None, _p(-0.2)) if pre == 1 else ()))
    assert y.shape == (B, H, W, Co)


def test_restatement_frozen_inputs(amd):
    """needs_input_grad is honoured: a frozen weight or input gets no gradient and the other one is unchanged."""
    T = amd.train
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(1, 2, 2, 8, dtype=torch.float64, generator=gen)
    w = torch.randn(8, 8, 1, 1, dtype=torch.float64, generator=gen)
    a, b = _p(0.1), _p(0.2)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    gx, gw = torch.autograd.grad(T.conv1x1(xr, wr, a, b).sum(), [xr, wr])
    (gx1,) = torch.autograd.grad(T.conv1x1(xr, w, a, b).sum(), [xr])
    (gw1,) = torch.autograd.grad(T.conv1x1(x, wr, a, b).sum(), [wr])
    assert torch.equal(gx, gx1) and torch.equal(gw, gw1)


@pytest.mark.parametrize("case", C.block_cases())
def test_block_hip_route_equals_torch_route_on_cpu(amd, case):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    block, x, g, ref = C.block_case(case, PreActFixupResBlock)
    x = x.contiguous(memory_format=torch.channels_last)
    T.stats.update(conv1x1_hip=0, conv1x1_fallbacks=0)
    hip = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv1x1="hip"))
    routed, fell = T.stats["conv1x1_hip"], T.stats["conv1x1_fallbacks"]
    tor = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv1x1="torch"))
    assert (T.stats["conv1x1_hip"], T.stats["conv1x1_fallbacks"]) == (routed, fell)      # the torch route counts nothing
    want_hip, want_fall = expected_routes(amd, block)
    assert (routed, fell) == (want_hip, want_fall) and routed >= 1, (case, routed, fell)
    assert torch.equal(hip["out"], tor["out"]), case
    for k, (v64, e_ref) in ref.items():
        d = float((hip[k].double() - tor[k].double()).norm() / v64.double().norm())
        print(f"{case} {k}: |hip - torch| / |g64| {d:.2e}  e_ref {e_ref:.2e}")
        assert d <= BAR * e_ref, (case, k, d, e_ref)
        assert C.dist(hip[k], v64.reshape(hip[k].shape)) <= BAR * e_ref, (case, k)


def expected_routes(amd, block):
    """(fused, fallback) counts of a block under "hip", from its modules: every 1x1, stride-1 conv is one or the other."""
    convs = [block.branch_conv1, block.branch_conv3]
    if block.mode == "up":
        convs.append(block.branch_conv2)
    if block.skip_conv is not None and block.mode in ("up", "same"):
        convs.append(block.skip_conv)
    assert all(c.kernel_size == (1, 1) for c in convs)
    ok = [c.in_channels % 8 == 0 and c.out_channels % 8 == 0 and 8 <= c.in_channels <= 256 and 8 <= c.out_channels <= 256
          for c in convs]
    return sum(ok), len(ok) - sum(ok)


def test_default_route_is_torch(amd):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    for case in C.block_cases():
        block, x, g, _ = C.block_case(case, PreActFixupResBlock)
        d = C.block_results(block, x, g, T.block_forward)
        t = C.block_results(block, x, g, lambda b, v: T.block_forward(b, v, conv1x1="torch"))
        m = C.block_results(block, x, g, lambda b, v: b(v))
        assert block.conv1x1 == "torch"
        for k in d:
            assert torch.equal(d[k], t[k]) and torch.equal(d[k], m[k]), (case, k)
    with pytest.raises(ValueError):
        T.block_forward(block, x, conv1x1="triton")
    with pytest.raises(ValueError):
        PreActFixupResBlock(8, 8, "same", conv1x1="miopen")
    assert PreActFixupResBlock(8, 8, "same", conv1x1="hip").conv1x1 == "hip"


def test_forward_train_keyword_on_cpu(amd):
    """forward_train / step pass the keyword down: under "hip" the first step's output is the torch route's."""
    T = amd.train
    model, batches = C.loop_model()
    x = batches[0].contiguous(memory_format=torch.channels_last)
    model.eval()                                           # no EMA update: both calls see the same quantiser
    T.stats.update(conv1x1_hip=0, conv1x1_fallbacks=0)
    out_h, rec_h, (vq_h,) = T.step(model, x, conv1x1="hip")
    assert T.stats["conv1x1_hip"] > 0
    out_t, rec_t, (vq_t,) = T.step(model, x)
    assert torch.equal(out_h, out_t) and torch.equal(rec_h, rec_t) and torch.equal(vq_h, vq_t)


def test_abi_errors_before_any_hip_call(amd):
    L = amd._lib
    lib = L.lib()
    one = ctypes.c_void_p(4096)
    fwd, bwd = lib.vqae_conv1x1_train_forward_f32, lib.vqae_conv1x1_train_backward_f32
    # null pointers -> VQAE_ERR_INVALID
    for args in ((None, one, one, 2, one, 4, 8, 8, one, None), (one, None, one, 2, one, 4, 8, 8, one, None),
                 (one, one, None, 1, one, 4, 8, 8, one, None), (one, one, one, 2, None, 4, 8, 8, one, None),
                 (one, one, one, 2, one, 4, 8, 8, None, None)):
        assert fwd(*args) == -1
        with pytest.raises(AssertionError):
            L.check(fwd(*args))
    for args in ((None, one, one, one, 2, one, 4, 8, 8, one, one, one, one, one, None),
                 (one, None, one, one, 2, one, 4, 8, 8, one, one, one, one, one, None),
                 (one, one, one, one, 2, None, 4, 8, 8, one, one, one, one, one, None),
                 (one, one, one, one, 2, one, 4, 8, 8, one, one, one, one, None, None)):
        assert bwd(*args) == -1
    # m = 0 -> VQAE_ERR_INVALID
    assert fwd(one, one, one, 2, one, 0, 8, 8, one, None) == -1
    assert bwd(one, one, one, one, 2, one, 0, 8, 8, one, one, one, one, one, None) == -1
    assert fwd(one, one, one, 3, one, 4, 8, 8, one, None) == -1                      # pre outside 0 .. 2
    # cin = 12, cout = 264 -> VQAE_ERR_UNSUPPORTED, and supported() agrees
    for cin, cout in ((12, 8), (8, 264), (8, 12), (264, 8), (0, 8), (8, 4)):
        assert lib.vqae_conv1x1_train_supported(cin, cout) == 0
        assert fwd(one, one, one, 2, one, 4, cin, cout, one, None) == -2
        assert bwd(one, one, one, one, 2, one, 4, cin, cout, one, one, one, one, one, None) == -2
        with pytest.raises(NotImplementedError):
            L.check(fwd(one, one, one, 2, one, 4, cin, cout, one, None))
        assert lib.vqae_conv1x1_train_workspace_bytes(4, cin, cout) == 0
    for cin, cout in ((8, 8), (8, 16), (24, 40), (256, 256), (128, 8)):
        assert lib.vqae_conv1x1_train_supported(cin, cout) == 1
        assert amd.ops.conv1x1_train_supported(cin, cout)
        for m in (1, 129, 65536, 2 ** 31 + 5):
            n = lib.vqae_conv1x1_train_workspace_bytes(m, cin, cout)
            assert n > 0 and n % 8 == 0
        # bounded by the weight's size, not by the number of rows
        assert lib.vqae_conv1x1_train_workspace_bytes(2 ** 31 + 5, cin, cout) == lib.vqae_conv1x1_train_workspace_bytes(2 ** 24, cin, cout)
        assert lib.vqae_conv1x1_train_workspace_bytes(2 ** 31, cin, cout) <= 8 * 256 * 64 * 64 + 8 * cin * cout + 2 ** 15
    r = lib.vqae_conv1x1_train_wgrad_run()
    assert r >= 64 and r == amd.ops.conv1x1_train_wgrad_run()
    with pytest.raises(amd._lib.VqaeHipError):
        amd.ops.conv1x1_train_forward(torch.zeros(1, 2, 2, 8), torch.zeros(8, 8, 1, 1))
