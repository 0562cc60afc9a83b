"""CPU: the trainable zero-padded 3x3 conv node of vqae_amd.train (conv3x3z / _Conv3x3zFn) through its plain-torch restatement --
the forward F.conv2d(x + c, w, bias, padding=1) and the hand-derived backward csrc/conv_train_thin.hip implements
(tests/test_conv3x3z_train_gpu.py runs the kernels).

  * torch.autograd.gradcheck of the restatement in fp64 for pre = 0 (u = x) and 1 (u = x + c, c != 0: the zeros are padded BEHIND
    the pre-op), with and without a bias, for a contiguous and a channels_last weight, at H x W = 4 x 5 and at the padding cases
    1 x 3, 2 x 1, 1 x 1, 2 x 2 (every tap but the centre may lie outside), and with a frozen input or weight;
  * every 'out' fixture case (outskip_8_3_4x4) under conv3x3z="hip" on CPU tensors: the forward is the "torch" route's bit for
    bit (the restatement calls the same F.conv2d on the same x + c); the gradients differ by fp32 re-association only, so
    ||hip - torch|| / ||g64|| <= 4 e_ref and dist(hip, g64) <= 4 e_ref per tensor group (the bound and its reasoning are
    tests/test_conv1x1_train_cpu.py's); stats counts 1 node and 0 fall-backs;
  * a stem 3 -> 4 takes the fall-back and is counted; the default keyword is the parent's graph bit for bit on every fixture
    case and on forward_train of spec tiny; an invalid keyword raises ValueError;
  * the C ABI's errors that are returned before any HIP call, and the workspace bound.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import fixup_train_cases as C

BAR = 4.0
KEYS = ("conv3x3z_hip", "conv3x3z_fallbacks", "conv3x3_hip", "conv3x3_fallbacks", "conv1x1_hip", "conv1x1_fallbacks",
        "conv_down_hip", "conv_down_fallbacks")
OUT_CASES = ["outskip_8_3_4x4"]
WS_BOUND = (16 << 20) + (512 << 10) + (16 << 10) + 256        # slots + bias slots + scalar rows + slack: below 16.6 MiB
assert WS_BOUND < 16.6 * 2 ** 20


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
    assert set(OUT_CASES) <= set(C.block_cases())


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("hw", [(4, 5), (1, 3), (2, 1), (1, 1), (2, 2)])
def test_gradcheck_restatement(amd, hw, pre, with_bias, channels_last):
    T = amd.train
    gen = torch.Generator().manual_seed(pre + 10 * hw[0] + hw[1] + 100 * with_bias)
    B, (H, W) = 2, hw
    Ci, Co = (3, 8) if with_bias == channels_last else (8, 3)            # both orientations under every other parameter
    x = torch.randn(B, H, W, Ci, dtype=torch.float64, generator=gen, requires_grad=True)
    w = _weight(Co, Ci, gen, channels_last)
    bias = torch.randn(Co, dtype=torch.float64, generator=gen).requires_grad_() if with_bias else None
    c = _p(0.5) if pre else None
    inputs = [t for t in (x, w, bias, c) if t is not None]

    def f(*ts):
        ts = list(ts)
        xx, ww = ts.pop(0), ts.pop(0)
        bb = ts.pop(0) if with_bias else None
        cc = ts.pop(0) if pre else None
        return T.conv3x3z(xx, ww, bb, cc)

    assert torch.autograd.gradcheck(f, inputs)
    y = f(*inputs)
    assert y.shape == (B, H, W, Co)
    u = x if c is None else x + c
    want = F.conv2d(u.permute(0, 3, 1, 2), w, bias, padding=1).permute(0, 2, 3, 1)
    assert torch.allclose(y, want, rtol=1e-12, atol=1e-12)
    # the padding is zeros, not c: the explicit form
    padded = F.pad(u.permute(0, 3, 1, 2), (1, 1, 1, 1))
    assert torch.allclose(y, F.conv2d(padded, w, bias).permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    g = torch.randn(y.shape, dtype=torch.float64, generator=gen)
    mine = torch.autograd.grad(y, inputs, g)
    stock = torch.autograd.grad(want, inputs, g)
    for p, q in zip(mine, stock):
        assert p.shape == q.shape and torch.allclose(p, q, rtol=1e-12, atol=1e-12)
    assert mine[1].shape == w.shape and mine[1].stride() == w.stride()   # the weight's own memory format


def test_restatement_frozen_inputs(amd):
    """needs_input_grad is honoured: a frozen weight or input gets no gradient and the others are unchanged."""
    T = amd.train
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(1, 2, 3, 8, dtype=torch.float64, generator=gen)
    w = torch.randn(3, 8, 3, 3, dtype=torch.float64, generator=gen)
    bias, c = torch.randn(3, dtype=torch.float64, generator=gen).requires_grad_(), _p(0.5)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    gx, gw, gb, gc = torch.autograd.grad(T.conv3x3z(xr, wr, bias, c).sum(), [xr, wr, bias, c])
    gx1, gb1, gc1 = torch.autograd.grad(T.conv3x3z(xr, w, bias, c).sum(), [xr, bias, c])
    gw1, gb2, gc2 = torch.autograd.grad(T.conv3x3z(x, wr, bias, c).sum(), [wr, bias, c])
    assert torch.equal(gx, gx1) and torch.equal(gw, gw1)
    assert torch.equal(gb, gb1) and torch.equal(gb, gb2) and torch.equal(gc, gc1) and torch.equal(gc, gc2)
    assert torch.autograd.gradcheck(lambda x: T.conv3x3z(x, w, bias, c), (xr,))
    assert torch.autograd.gradcheck(lambda w: T.conv3x3z(x, w, bias, c), (wr,))


@pytest.mark.parametrize("case", OUT_CASES)
def test_block_hip_route_on_cpu(amd, case):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    block, x, g, ref = C.block_case(case, PreActFixupResBlock)
    assert block.mode == "out"
    x = x.contiguous(memory_format=torch.channels_last)
    _reset(T)
    hip = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv3x3z="hip"))
    assert _counts(T) == (1, 0) + (0,) * 6                                 # the keywords are independent
    tor = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv3x3z="torch"))
    assert _counts(T) == (1, 0) + (0,) * 6                                 # the torch route counts nothing
    assert torch.equal(hip["out"], tor["out"])
    for k, (v64, e_ref) in ref.items():
        d = float((hip[k].double() - tor[k].double()).norm() / v64.double().norm())
        print(f"{case} {k}: |hip - torch| / |g64| {d:.2e}  e_ref {e_ref:.2e}")
        assert d <= BAR * e_ref, (k, d, e_ref)
        assert C.dist(hip[k], v64.reshape(hip[k].shape)) <= BAR * e_ref, k
    every = C.block_results(block, x, g, lambda b, t: T.block_forward(b, t, conv1x1="hip", conv_down="hip", conv3x3="hip",
                                                                      conv3x3z="hip"))
    assert torch.equal(every["out"], tor["out"])
    assert T.stats["conv3x3z_hip"] == 2 and T.stats["conv3x3_hip"] == 1 and T.stats["conv1x1_fallbacks"] == 1
    # a channels_last weight (what the reference trains with): the same node, the gradient in the weight's format
    blk2 = PreActFixupResBlock(block.in_channels, block.out_channels, block.mode, conv3x3z="hip")
    blk2.load_state_dict(block.state_dict())
    blk2.skip_conv.weight.data = blk2.skip_conv.weight.data.contiguous(memory_format=torch.channels_last)
    cl = C.block_results(blk2, x, g, lambda b, t: b(t))
    assert torch.equal(cl["out"], tor["out"])
    for k, (v64, e_ref) in ref.items():
        assert C.dist(cl[k], v64.reshape(cl[k].shape)) <= BAR * e_ref, k


def test_other_blocks_have_no_candidate(amd):
    """A 'same', 'down' or 'up' block has no zero-padded conv: under conv3x3z="hip" nothing is counted and the bits are the
    default's."""
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    _reset(T)
    for case in C.block_cases():
        block, x, g, _ = C.block_case(case, PreActFixupResBlock)
        if block.mode == "out":
            continue
        d = C.block_results(block, x, g, T.block_forward)
        h = C.block_results(block, x, g, lambda b, v: T.block_forward(b, v, conv3x3z="hip"))
        for k in d:
            assert torch.equal(d[k], h[k]), (case, k)
    assert _counts(T) == (0,) * 8


def test_narrow_stem_takes_the_fallback(amd):
    """A stem 3 -> 4 (and its out_stem 4 -> 3) is outside the channel rule: the torch route, counted."""
    import vqae_amd
    from vqae_amd.model import VQAE
    T = amd.train
    torch.manual_seed(3)
    spec = vqae_amd.spec.VQAESpec(stem=4, n_down=1, n_pre=1, n_post=1, n_enc=1, num_embeddings=8, projection_dim=0)
    model = VQAE.from_spec(spec).eval()
    x = torch.randn(1, 3, 8, 8).contiguous(memory_format=torch.channels_last)
    _reset(T)
    out_h, _ = T.forward_train(model, x, conv3x3z="hip")
    assert _counts(T)[:2] == (0, 2)
    out_t, _ = T.forward_train(model, x)
    assert torch.equal(out_h, out_t) and _counts(T)[:2] == (0, 2)
    assert not amd.ops.conv3x3z_train_supported(3, 4) and not amd.ops.conv3x3z_train_supported(4, 3)


def test_default_route_is_torch(amd):
    """With the keyword at its default, or "torch", every fixture case gives the bits of the graph written out with the ops
    the module has always used (fixup_add, then F.conv2d with padding 1, for the skip of an 'out' block), and forward_train of
    spec tiny those of the stems written as F.conv2d."""
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train

    def parent_graph(block, xn):
        x = T.to_nhwc(xn)
        conv = lambda t, w, **kw: T.to_nhwc(F.conv2d(T.to_nchw(t), w, **kw))
        t = conv(T.fixup_act(x, block.bias1a, block.bias1b), block.branch_conv1.weight)
        t = conv(T.fixup_act(t, block.bias2a, block.bias2b, halo=1), block.branch_conv2.weight)
        t = conv(T.fixup_act(t, block.bias3a, block.bias3b), block.branch_conv3.weight)
        skip = conv(T.fixup_add(x, block.bias1c), block.skip_conv.weight, padding=1)
        return T.to_nchw(T.fixup_out(t, skip, block.scale, block.bias4, block.bias1d))

    _reset(T)
    for case in C.block_cases():
        block, x, g, _ = C.block_case(case, PreActFixupResBlock)
        assert block.conv3x3z == "torch"
        d = C.block_results(block, x, g, T.block_forward)
        t = C.block_results(block, x, g, lambda b, v: T.block_forward(b, v, conv3x3z="torch"))
        m = C.block_results(block, x, g, lambda b, v: b(v))
        for k in d:
            assert torch.equal(d[k], t[k]) and torch.equal(d[k], m[k]), (case, k)
        if block.mode == "out":
            p = C.block_results(block, x, g, parent_graph)
            for k in d:
                assert torch.equal(d[k], p[k]), (case, k)
    # the whole model: the stems as the parent wrote them
    model, batches = C.loop_model()
    model.eval()
    x = batches[0].contiguous(memory_format=torch.channels_last)
    out, (vq,) = T.forward_train(model, x)
    out_t, (vq_t,) = T.forward_train(model, x, conv3x3z="torch")
    enc, dec = model.encoder, model.decoder
    h = T.to_nhwc(F.conv2d(x, enc.in_stem.weight, enc.in_stem.bias, padding=1))
    for level in enc.down_layers[0].layers:
        for blk in level.layers:
            h = T.block_forward_nhwc(blk, h)
    for blk in enc.pre_enc_layers[0]:
        h = T.block_forward_nhwc(blk, h)
    q, _, vq_p = T._quantize_torch(enc.vq_layers[0], T.to_nchw(h))
    h = T.to_nhwc(q)
    for blk in dec.post_enc_layers[0]:
        h = T.block_forward_nhwc(blk, h)
    for level in dec.up_layers[0].layers:
        for blk in level.layers:
            h = T.block_forward_nhwc(blk, h)
    out_p = F.conv2d(T.to_nchw(h), dec.out_stem.weight, dec.out_stem.bias, padding=1)
    assert torch.equal(out, out_t) and torch.equal(out, out_p) and torch.equal(vq, vq_t) and torch.equal(vq, vq_p)
    grads = lambda o, v: torch.autograd.grad(o.square().mean() + v, list(model.parameters()))
    for p, q in zip(grads(out, vq), grads(out_p, vq_p)):
        assert torch.equal(p, q)
    assert _counts(T) == (0,) * 8
    for call in (lambda: T.block_forward(block, x, conv3x3z="triton"), lambda: T.block_forward_nhwc(block, x, conv3x3z="miopen"),
                 lambda: T.forward_train(None, x, conv3x3z="miopen"), lambda: T.step(None, x, conv3x3z=""),
                 lambda: PreActFixupResBlock(8, 3, "out", conv3x3z="miopen"), lambda: T.conv_routes(conv3x3z=None)):
        with pytest.raises(ValueError):
            call()
    blk = PreActFixupResBlock(8, 3, "out", conv3x3z="hip")
    assert (blk.conv3x3z, blk.conv3x3, blk.conv1x1, blk.conv_down) == ("hip", "torch", "torch", "torch")
    assert T.CONV3X3Z_ROUTES == ("torch", "hip")


def test_forward_train_keyword_on_cpu(amd):
    """forward_train / step pass the keyword down: under "hip" both stems of spec tiny are the fused node, the first step's
    output is the torch route's, and every parameter gets a finite gradient."""
    T = amd.train
    model, batches = C.loop_model()
    x = batches[0].contiguous(memory_format=torch.channels_last)
    model.eval()                                           # no EMA update: both calls see the same quantiser
    _reset(T)
    out_h, rec_h, (vq_h,) = T.step(model, x, conv3x3z="hip")
    assert _counts(T) == (2, 0) + (0,) * 6
    out_t, rec_t, (vq_t,) = T.step(model, x)
    assert T.stats["conv3x3z_hip"] == 2
    assert torch.equal(out_h, out_t) and torch.equal(rec_h, rec_t) and torch.equal(vq_h, vq_t)
    out_b, _, _ = T.step(model, x, conv1x1="hip", conv_down="hip", conv3x3="hip", conv3x3z="hip")
    assert torch.equal(out_b, out_t) and T.stats["conv3x3z_hip"] == 4 and T.stats["conv3x3z_fallbacks"] == 0
    params = list(model.parameters())
    gh = torch.autograd.grad(rec_h + vq_h, params)
    for (k, _), p in zip(model.named_parameters(), gh):
        assert bool(torch.isfinite(p).all()), k            # (their distance to fp64 is test_block_hip_route_on_cpu's subject)
    by_name = dict(zip((k for k, _ in model.named_parameters()), gh))
    for k in ("encoder.in_stem.weight", "encoder.in_stem.bias", "decoder.out_stem.weight", "decoder.out_stem.bias"):
        assert float(by_name[k].abs().max()) > 0, k        # the batch needs no gradient; the stems' parameters have theirs


def test_abi_errors_before_any_hip_call(amd):
    L = amd._lib
    lib = L.lib()
    one = ctypes.c_void_p(4096)
    odd = ctypes.c_void_p(4096 + 8)
    fwd, bwd = lib.vqae_conv3x3z_train_forward_f32, lib.vqae_conv3x3z_train_backward_f32
    err = lambda: lib.vqae_last_error().decode()

    def f(x=one, a=one, b=one, pre=1, w=one, bias=one, lay=1, B=2, H=4, W=5, ci=8, co=3, y=one, ws=one):
        return fwd(x, a, b, pre, w, bias, lay, B, H, W, ci, co, y, ws, None)

    def r(g=one, x=one, a=one, b=one, pre=1, w=one, lay=1, B=2, H=4, W=5, ci=8, co=3, gx=one, gw=one, ga=one, gb=one, gbias=one,
          ws=one):
        return bwd(g, x, a, b, pre, w, lay, B, H, W, ci, co, gx, gw, ga, gb, gbias, ws, None)

    INVALID, UNSUPPORTED = -1, -2
    # null pointers: every required one in turn (a is never read: pre < 2; the bias and the forward's workspace are optional)
    for kw in ({"x": None}, {"b": None}, {"w": None}, {"y": None}):
        assert f(**kw) == INVALID and "null pointer" in err(), kw
    with pytest.raises(AssertionError):
        L.check(f(x=None))
    for kw in ({"g": None}, {"x": None}, {"b": None}, {"w": None}, {"ws": None}):
        assert r(**kw) == INVALID and "null pointer" in err(), kw
    # misaligned pointers: tensors 16 bytes, the workspace 8
    for kw in ({"x": odd}, {"w": odd}, {"bias": odd}, {"y": odd}):
        assert f(**kw) == INVALID and "aligned" in err(), kw
    for kw in ({"g": odd}, {"x": odd}, {"w": odd}, {"gx": odd}, {"gw": odd}, {"gbias": odd}, {"ws": ctypes.c_void_p(4100)}):
        assert r(**kw) == INVALID and "aligned" in err(), kw
    # pre, w_layout, geometry
    for kw in ({"pre": 3}, {"pre": -1}, {"lay": 2}, {"lay": -1}, {"B": 0}, {"H": 0}, {"W": 0}, {"B": -1}, {"H": -2}, {"W": -1},
               {"B": 2 ** 40, "H": 1, "W": 1}, {"B": 2 ** 20, "H": 2 ** 10, "W": 2 ** 10}, {"B": 2 ** 62, "H": 4, "W": 4}):
        assert f(**kw) == INVALID, kw
        assert r(**kw) == INVALID, kw
    assert f(pre=2) == UNSUPPORTED and "pre 2" in err() and r(pre=2) == UNSUPPORTED
    # the order of entry_checks: geometry, pre, w_layout, null pointers, the channel rule, 2^40 rows, alignment
    assert f(B=0, pre=7) == INVALID and "batch 0" in err()
    assert f(pre=7, lay=9) == INVALID and "pre 7" in err()
    assert f(lay=9, x=None) == INVALID and "w_layout 9" in err()
    assert f(x=None, ci=5) == INVALID and "null pointer" in err()
    assert f(ci=5, B=2 ** 40, H=1, W=1) == UNSUPPORTED and "cin 5" in err()
    assert f(B=2 ** 40, H=1, W=1, x=odd) == INVALID and "2^40" in err()
    # channel pairs on both sides of the rule
    no = ((3, 3), (3, 4), (4, 3), (3, 12), (12, 3), (3, 72), (3, 128), (264, 3), (0, 3), (3, 0), (8, 8), (8, 16), (1, 8), (8, 1),
          (2, 8), (4, 8), (8, 4), (-8, 3))
    for ci, co in no:
        assert lib.vqae_conv3x3z_train_supported(ci, co) == 0 and not amd.ops.conv3x3z_train_supported(ci, co), (ci, co)
        assert f(ci=ci, co=co) == UNSUPPORTED and r(ci=ci, co=co) == UNSUPPORTED, (ci, co)
        assert lib.vqae_conv3x3z_train_workspace_bytes(2, 4, 5, ci, co) == 0
    with pytest.raises(NotImplementedError):
        L.check(f(ci=12))
    assert lib.vqae_conv3x3z_train_workspace_bytes(0, 4, 6, 8, 3) == 0
    assert lib.vqae_conv3x3z_train_workspace_bytes(2, 0, 6, 8, 3) == 0
    assert lib.vqae_conv3x3z_train_workspace_bytes(2 ** 40, 1, 1, 8, 3) == 0
    # answers that need no GPU: the whole supported range stays under the stated bound, whatever the number of rows
    yes = [(3, co) for co in range(8, 65, 8)] + [(ci, 3) for ci in range(8, 257, 8)]
    worst = 0
    for ci, co in yes:
        assert lib.vqae_conv3x3z_train_supported(ci, co) == 1 and amd.ops.conv3x3z_train_supported(ci, co), (ci, co)
        for B, H, W in ((1, 1, 1), (3, 7, 49), (16, 256, 256), (8, 512, 512), (2 ** 17, 2048, 2048)):
            n = lib.vqae_conv3x3z_train_workspace_bytes(B, H, W, ci, co)
            assert 0 < n <= WS_BOUND and n % 8 == 0, (ci, co, B, H, W, n)
            worst = max(worst, n)
        assert (lib.vqae_conv3x3z_train_workspace_bytes(2 ** 17, 2048, 2048, ci, co)
                == lib.vqae_conv3x3z_train_workspace_bytes(2 ** 10, 2048, 2048, ci, co))
    print(f"largest conv3x3z workspace over the supported range: {worst} bytes (bound {WS_BOUND})")
    R = lib.vqae_conv3x3z_train_wgrad_run()
    assert R >= 64 and R == amd.ops.conv3x3z_train_wgrad_run()
    with pytest.raises(amd._lib.VqaeHipError):
        amd.ops.conv3x3z_train_forward(torch.zeros(1, 2, 2, 8), torch.zeros(3, 8, 3, 3))
