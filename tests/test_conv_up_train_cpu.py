"""CPU: the keyword conv_up of vqae_amd.train and its two Functions (up2_act, fixup_out_up) through their plain-torch
restatements -- the forward and the hand-derived backward csrc/up_train.hip implements (tests/test_conv_up_train_gpu.py runs
the kernels).

  * torch.autograd.gradcheck of both Functions in fp64, inputs away from the ELU kink;
  * both 'up' cases of tests/golden/fixup_train.npz under conv_up="hip" against the fixture's fp64 autograd: every group within
    4 x e_ref, e_ref the larger of the fixture's own fp32 distance and block_forward_torch's on this CPU.  (The commuted order
    sums the same products in another order; it is held to the distance of the two fp32 evaluations of the ORIGINAL order.)
  * integer data: the commuted order equals the original bit for bit, outputs and all gradients -- the taps are multiples of
    2^-8, so where no sum needs more than 24 bits both orders are exact.  With the ranges x in -8 .. 8, weights in -4 .. 4 that
    holds while the resize mixes along ONE axis (1 x 2, 2 x 1, 1 x 1: 8 fractional bits); along two axes (16 fractional bits)
    the ORIGINAL order itself rounds its weight-gradient products, so the 2-D shapes use x, weights in -1 .. 1.  Each case
    first asserts its own premises: every ELU argument is positive (ELU is the identity, ELU' = 1), and the original order in
    fp32 equals itself in fp64 (nothing was rounded);
  * the keyword's plumbing: validation at all six entry points, the default graph, the counters, a whole model.
"""
import copy
import inspect

import pytest
import torch
import torch.nn.functional as F

import fixup_train_cases as C

BAR = 4.0
HW = [(1, 1), (1, 2), (2, 1), (3, 5)]


def _p(v):
    return torch.tensor([v], dtype=torch.float64, requires_grad=True)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", HW, ids=lambda s: "x".join(map(str, s)))
def test_gradcheck_functions(amd, hw, c):
    T = amd.train
    gen = torch.Generator().manual_seed(10 * hw[0] + hw[1] + c)
    low, big = (2, hw[0], hw[1], c), (2, 2 * hw[0], 2 * hw[1], c)
    # up2(t_low) + a stays at least 0.2 from the kink: |t_low| in [1, 1.5] of one sign per channel keeps |up2| >= 1.32 - 0.48
    sign = torch.tensor([1.0, -1.0, 1.0])[:c]
    t_low = ((1 + 0.5 * torch.rand(low, dtype=torch.float64, generator=gen)) * sign).requires_grad_()
    a = _p(0.3)
    assert float((T.bicubic_up2(t_low.detach()) + a.detach()).abs().min()) > 0.2
    assert torch.autograd.gradcheck(T.up2_act, (t_low, a, _p(-0.2)))
    t = torch.randn(big, dtype=torch.float64, generator=gen, requires_grad=True)
    s_low = torch.randn(low, dtype=torch.float64, generator=gen, requires_grad=True)
    assert torch.autograd.gradcheck(T.fixup_out_up, (t, s_low, _p(1.3), _p(0.1), _p(-0.4)))


@pytest.mark.parametrize("hw", HW, ids=lambda s: "x".join(map(str, s)))
def test_restatements_are_the_compositions(amd, hw):
    """On CPU tensors the new nodes are the existing ones composed, bit for bit, forward and backward."""
    T = amd.train
    gen = torch.Generator().manual_seed(3)
    low, big = (2, hw[0], hw[1], 3), (2, 2 * hw[0], 2 * hw[1], 3)
    mk = lambda shape: torch.randn(shape, dtype=torch.float64, generator=gen, requires_grad=True)
    t_low, s_low, t, g = mk(low), mk(low), mk(big), torch.randn(big, dtype=torch.float64, generator=gen)
    ps = [_p(v) for v in (0.3, -0.2, 1.3, 0.1, -0.4)]
    a, b, sc, b4, b1d = ps
    pairs = [(T.up2_act(t_low, a, b), T.fixup_act(T.bicubic_up2(t_low), a, b), [t_low, a, b]),
             (T.fixup_out_up(t, s_low, sc, b4, b1d), T.fixup_out(t, T.bicubic_up2(s_low), sc, b4, b1d), [t, s_low, sc, b4, b1d])]
    for mine, comp, inputs in pairs:
        assert torch.equal(mine, comp)
        for p, q in zip(torch.autograd.grad(mine, inputs, g), torch.autograd.grad(comp, inputs, g)):
            assert torch.equal(p, q)


@pytest.mark.parametrize("case", [c for c in C.block_cases() if c.startswith("up_")])
def test_block_forward_matches_reference(amd, case):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    assert case in ("up_16_8_3x5", "up_16_8_1x2")
    block, x, g, ref = C.block_case(case, PreActFixupResBlock)
    x = x.contiguous(memory_format=torch.channels_last)
    got = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv_up="hip"))
    stock = C.block_results(block, x, g, T.block_forward_torch)
    assert set(got) == set(ref)
    for k, (v64, e_fix) in ref.items():
        e = C.dist(got[k], v64.reshape(got[k].shape))
        e_ref = max(e_fix, C.dist(stock[k], v64.reshape(stock[k].shape)))
        print(f"{case} {k}: e {e:.2e} e_ref {e_ref:.2e} ratio {e / e_ref:.2f}")
        assert e <= BAR * e_ref, (case, k, e, e_ref)
    # in fp64 the commuted order is the reference to fp64 rounding: the same function, not merely a close one
    block, x, g, ref = C.block_case(case, PreActFixupResBlock, dtype=torch.float64)
    got = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv_up="hip"))
    for k, (v64, _) in ref.items():
        assert C.dist(got[k], v64.reshape(got[k].shape)) <= 1e-13, (case, k)


def _integer_block(cin, cout, hw, seed, wmax, xmax, dtype):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    gen = torch.Generator().manual_seed(seed)
    block = PreActFixupResBlock(cin, cout, "up")
    with torch.no_grad():
        for name, p in block.named_parameters():
            if p.numel() == 1:
                p.fill_(1.0 if name == "scale" else 0.0)
            else:
                p.copy_(torch.randint(-wmax, wmax + 1, p.shape, generator=gen).to(p.dtype))
    x = torch.randint(-xmax, xmax + 1, (2, cin, *hw), generator=gen).float() + (xmax + 1)       # shifted positive
    g = torch.randint(-min(xmax, 3), min(xmax, 3) + 1, (2, cout, 2 * hw[0], 2 * hw[1]), generator=gen).float()
    return block.to(dtype), x.to(dtype), g.to(dtype)


def _run(T, block, x, g, **routes):
    x = x.clone().requires_grad_()
    y = T.block_forward(block, x, **routes)
    return [y.detach()] + list(torch.autograd.grad(y, [x] + list(block.parameters()), g))


# (cin, cout, (H, W), seed, |weights| <=, |x| <=): seeds whose conv1 and conv2 outputs are positive everywhere
INTEGER_CASES = [(2, 1, (1, 2), 32, 4, 8), (2, 1, (2, 1), 39, 4, 8), (4, 2, (1, 1), 29, 4, 8), (4, 2, (1, 2), 29, 4, 8),
                 (2, 1, (3, 5), 67, 1, 1), (2, 1, (2, 3), 107, 1, 1)]


@pytest.mark.parametrize("cin,cout,hw,seed,wmax,xmax", INTEGER_CASES)
def test_integer_data_commutes_bit_for_bit(amd, cin, cout, hw, seed, wmax, xmax):
    T = amd.train
    block, x, g = _integer_block(cin, cout, hw, seed, wmax, xmax, torch.float32)
    t = F.conv2d(x, block.branch_conv1.weight)
    t2 = F.conv2d(F.interpolate(t, scale_factor=2, mode="bicubic", align_corners=False), block.branch_conv2.weight)
    assert bool((x > 0).all()) and bool((t > 0).all()) and bool((t2 > 0).all()), "premise: ELU is the identity"
    want = _run(T, block, x, g)
    exact = _run(T, *_integer_block(cin, cout, hw, seed, wmax, xmax, torch.float64))
    assert all(torch.equal(p.double(), q) for p, q in zip(want, exact)), "premise: the original order rounds nothing"
    got = _run(T, block, x, g, conv_up="hip")
    assert len(got) == len(want) == 2 + len(list(block.parameters()))
    for p, q in zip(got, want):
        assert p.shape == q.shape and torch.equal(p, q)
    assert all(float(v.abs().max()) > 0 for v in want[:2])


# ---- the keyword --------------------------------------------------------------------------------------------------------------
def test_invalid_values_raise_everywhere(amd):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    from vqae_amd.model import VQAE
    T = amd.train
    assert T.CONV_UP_ROUTES == T.ROUTES == ("torch", "hip")
    block = PreActFixupResBlock(16, 8, "up")
    x = torch.zeros(1, 16, 2, 2)
    model = VQAE.from_spec(amd.SPECS["tiny"])
    batch = torch.zeros(1, 3, 32, 32)
    calls = [lambda v: T.conv_routes(conv_up=v), lambda v: T.block_forward(block, x, conv_up=v),
             lambda v: T.block_forward_nhwc(block, x.permute(0, 2, 3, 1), conv_up=v),
             lambda v: T.forward_train(model, batch, conv_up=v), lambda v: T.step(model, batch, conv_up=v),
             lambda v: PreActFixupResBlock(16, 8, "up", conv_up=v)]
    for call in calls:
        for bad in ("miopen", None, True):
            with pytest.raises(ValueError):
                call(bad)
    assert T.conv_routes(conv_up="hip")["conv_up"] is True and T.conv_routes()["conv_up"] is False


def test_default_is_todays_graph_and_counters(amd):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    torch.manual_seed(5)
    block = PreActFixupResBlock(16, 8, "up")
    with torch.no_grad():
        for p in block.parameters():
            p.add_(0.1 * torch.randn_like(p))
    assert block.conv_up == "torch"
    assert PreActFixupResBlock(16, 8, "up", conv_up="hip").conv_up == "hip"
    assert list(inspect.signature(PreActFixupResBlock.__init__).parameters)[-2:] == ["conv_up", "kwargs"]    # the last keyword
    assert list(inspect.signature(T.conv_routes).parameters)[-1] == "conv_up"
    x, g = torch.randn(2, 16, 3, 5), torch.randn(2, 8, 6, 10)
    T.stats.update(conv_up_hip=0, conv_up_fallbacks=0)
    plain, explicit, module = _run(T, block, x, g), _run(T, block, x, g, conv_up="torch"), None
    xx = x.clone().requires_grad_()
    y = block(xx)
    module = [y.detach()] + list(torch.autograd.grad(y, [xx] + list(block.parameters()), g))
    for other in (explicit, module):
        assert all(torch.equal(p, q) for p, q in zip(plain, other))
    assert T.stats["conv_up_hip"] == 0 and T.stats["conv_up_fallbacks"] == 0
    hip = _run(T, block, x, g, conv_up="hip")
    assert T.stats["conv_up_hip"] == 2 and T.stats["conv_up_fallbacks"] == 0
    assert all(p.shape == q.shape and torch.allclose(p, q, rtol=1e-3, atol=1e-4) for p, q in zip(hip, plain))
    # other modes ignore the keyword: the same bits, nothing counted
    for mode, cout in (("same", 16), ("down", 32)):
        other = PreActFixupResBlock(16, cout, mode)
        x4 = torch.randn(1, 16, 4, 4)
        assert torch.equal(T.block_forward(other, x4, conv_up="hip"), T.block_forward(other, x4))
    assert T.stats["conv_up_hip"] == 2
    # an 'up' block without a skip_conv (no constructor builds one) is counted and raises as the torch route does
    block.skip_conv = None
    with pytest.raises(Exception) as torch_route:
        T.block_forward(block, x)
    with pytest.raises(type(torch_route.value)):
        T.block_forward(block, x, conv_up="hip")
    assert T.stats["conv_up_fallbacks"] == 1 and T.stats["conv_up_hip"] == 2


def test_forward_train_gives_every_parameter_a_gradient(amd):
    T = amd.train
    model, batches = C.loop_model()
    with torch.no_grad():                                  # Fixup zero-initialises branch_conv3: give every path a signal
        for p in model.parameters():
            if float(p.abs().max()) == 0:
                p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())))
    n_up = sum(1 for m in model.modules() if getattr(m, "mode", None) == "up")
    x = batches[0].contiguous(memory_format=torch.channels_last)
    twin = copy.deepcopy(model)
    T.stats.update(conv_up_hip=0, conv_up_fallbacks=0)
    out, (vq_loss,) = T.forward_train(model, x, conv_up="hip")
    (F.huber_loss(out, x) + vq_loss).backward()
    assert n_up > 0 and T.stats["conv_up_hip"] == 2 * n_up and T.stats["conv_up_fallbacks"] == 0
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    out2, recon, _ = T.step(twin, x, conv_up="hip")      # a copy taken before the first call: the quantiser's EMA moves on
    assert torch.equal(out2, out) and bool(torch.isfinite(recon))


def test_new_symbols_validate_before_any_launch(amd):
    """The error convention of the C ABI for the new entry points, without a GPU (validation precedes every HIP call)."""
    import ctypes
    L = amd._lib
    lib = L.lib()
    one = ctypes.c_void_p(16)
    assert lib.vqae_up_train_workspace_bytes(1, 1, 1, 1) == 16 + 256
    assert lib.vqae_up_train_workspace_bytes(1, 9, 8, 17) == 2 * 1 * 2 * 16 + 256          # tiles: 2 x 1 x 2 channel chunks
    assert lib.vqae_up_train_workspace_bytes(64, 512, 512, 64) == 2048 * 16 + 256          # capped: the workgroups loop
    with pytest.raises(AssertionError):
        L.check(lib.vqae_up2_act_f32(None, one, one, 1, 2, 2, 4, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_up2_act_f32(one, one, one, 1, 0, 2, 4, one, None))
    with pytest.raises(NotImplementedError):
        L.check(lib.vqae_up2_act_f32(one, one, one, 1 << 20, 1 << 10, 1 << 10, 4, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_up2_act_backward_f32(one, None, one, 1, 2, 2, 4, one, one, one, one, None))
    with pytest.raises(AssertionError):                    # workspace not 8-byte aligned
        L.check(lib.vqae_up2_act_backward_f32(one, one, one, 1, 2, 2, 4, one, one, one, ctypes.c_void_p(12), None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_fixup_out_up_f32(one, one, one, one, None, 1, 2, 2, 4, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_fixup_out_up_backward_f32(one, one, one, 1, 2, 2, 4, one, None, one, one, one, one, None))
    with pytest.raises(L.VqaeHipError):
        amd.ops.up2_act(torch.zeros(1, 2, 2, 4), torch.zeros(1), torch.zeros(1))
    with pytest.raises(L.VqaeHipError):
        amd.ops.fixup_out_up(torch.zeros(1, 4, 4, 4), torch.zeros(1, 2, 2, 4), torch.zeros(1), torch.zeros(1), torch.zeros(1))
