"""GPU: the trainable circular 3x3 conv kernels (the Circ3x3 policy of csrc/conv_train.hip) behind
vqae_amd.ops.conv3x3_train_* and train.conv3x3.  x [B, H, W, Ci], y [B, H, W, Co], M = B H W rows of a GEMM with K = 9 Ci over
rows gathered with a circular wrap.

Shapes (B, H, W): the wrap cases (1,1,1), (1,1,2), (1,2,1), (1,2,2), (1,1,3), (1,3,1), (2,3,3) (at H = 1 all three kh read the
same row, at H = 2 the taps -1 and +1 read the same one); the tile edges (2,3,5), (1,1,31), (1,4,8), (1,3,11), (1,1,127), (2,8,8),
(1,3,43), (1,1,257), (3,7,49): M = 30, 31, 32, 33, 127, 128, 129, 257 and 2 R + 5 (R = vqae_conv3x3_train_wgrad_run() = 512;
another R takes (1, 1, 2 R + 5)) -- around the 32-row MFMA tile, the 64-row weight-gradient step, the 128-row workgroup tile,
more than one fp32 run; rows of a tile cross image rows and batch entries; and the narrow tall image (1,70,1), where a 64-row
weight-gradient block wraps W at every row -- x (Ci, Co) in {(8,8), (8,16), (16,16), (24,40), (32,64), (64,128), (128,256),
(256,256)} (every tile count of the templates, K and N tails, 32 columns spanning several taps), the last two with M <= 129
only; and (25, 49, 107), M = 2^17 + 3, with (8,8) and (16,8).  Both weight layouts.

Exact: small-integer data with a = 0.5, b = -0.5, so u = ELU(x + a) + b = x and ELU' = 1 without rounding; every partial sum
of every output is an integer below 2^24 (checked from the data), so y, g_x, g_w, g_a, g_b are the exact results whatever
the order of summation: a row, tap or channel dropped, doubled or wrapped to the wrong pixel at any tile or image edge shows.

No stray writes: the library called on interior slices of sentinel-filled buffers.  Run to run: two calls give the same bits.

Element-wise bounds against the fp64 evaluation of the restatement, from the arithmetic alone -- the derivation of
tests/test_conv_down_train_gpu.py with the term counts of this GEMM (u = 2^-24; expm1f / expf taken as <= 4 ulp = 8 u relative; a
sum of K fp32 products accumulated in fp32 in any order is within (K + 1) u sum|terms|; nothing measured).  v = x + a,
e = ELU(v), op = e + b the operand, d = ELU'(v); sums over the 9 Ci gathered columns k = (kh, kw, ci), for g_u over the 9 Co
gathered columns (kh, kw, co) of g against the flipped weight:
    operand   D = u (|v| + 8 |e| + |op|)                     (0 for pre = 0, u |op| for pre = 1)
    y         sum_k D |w| + (9 Ci + 1) u sum_k (|op| + D) |w|
    g_u       G = (9 Co + 1) u sum_{kh,kw,co} |g| |w|
    g_x       G d (1 + 2^-20) + u |g_u| d (|v| + 10)
    g_a, g_b  the sum of the element bounds + u |sum| + 2^-40 sum |terms|      (fp64 sums of fp32 values, rounded once)
    g_w       sum_m |g| D + (min(M, R) + 1) u sum_m |g| (|op| + D) + u |g_w| + 2^-40 sum_m |g| |op|

Op parity: e_dev = ||hip - v64|| / ||v64|| per output <= 4 x e_ref, e_ref the larger of CPU fp32 autograd of
F.conv2d(F.pad(F.elu(x + a) + b, circular), w) and the same on the GPU with stock torch ops; the one-element outputs of all
parity shapes form ONE vector of relative values (tests/fixup_train_cases.py says why).  Blocks and closed loop: the bar and the
e_ref construction of test_fixup_train_gpu.py, under conv3x3="hip" alone and under all three keywords "hip".
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import fixup_train_cases as C
from conftest import record_parity

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -40
BAR = 4.0
PAIRS = [(8, 8), (8, 16), (16, 16), (24, 40), (32, 64), (64, 128), (128, 256), (256, 256)]
WIDE = [(128, 256), (256, 256)]
WRAP = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (1, 2, 2), (1, 1, 3), (1, 3, 1), (2, 3, 3)]
EDGES = [(2, 3, 5), (1, 1, 31), (1, 4, 8), (1, 3, 11), (1, 1, 127), (2, 8, 8), (1, 3, 43), (1, 1, 257)]
TALL = (1, 70, 1)
BIG = (25, 49, 107)
assert BIG[0] * BIG[1] * BIG[2] == 2 ** 17 + 3
BLOCK_CASES = ["same_8_4x6", "same_8_1x1", "same_8_2x2", "sameskip_8_16_3x5", "outskip_8_3_4x4"]
# conv1x1="hip" in these blocks: (fused nodes, fall-backs); branch_conv3 8 -> 3 of the 'out' block falls back
CONV1X1_COUNTS = {"same_8_4x6": (2, 0), "same_8_1x1": (2, 0), "same_8_2x2": (2, 0), "sameskip_8_16_3x5": (3, 0),
                  "outskip_8_3_4x4": (1, 1)}
STATS = ("conv3x3_hip", "conv3x3_fallbacks", "conv1x1_hip", "conv1x1_fallbacks", "conv_down_hip", "conv_down_fallbacks")


def two_runs(amd):
    r = amd.ops.conv3x3_train_wgrad_run()
    return (3, 7, 49) if r == 512 else (1, 1, 2 * r + 5)


def shapes(amd):
    out = []
    for bhw in WRAP + EDGES + [two_runs(amd), TALL]:
        m = bhw[0] * bhw[1] * bhw[2]
        out += [bhw + p for p in PAIRS if not (p in WIDE and m > 129)]
    return out + [BIG + (8, 8), BIG + (16, 8)]


def P(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


def ints(shape, seed, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def patches(t):
    """[B, H, W, C] -> [M, 9 C], column (kh, kw, c) = t[b][(h + kh - 1) mod H][(w + kw - 1) mod W][c]."""
    B, H, W, Cc = t.shape
    ih, iw = torch.arange(-1, H + 1) % H, torch.arange(-1, W + 1) % W
    p = t[:, ih][:, :, iw].unfold(1, 3, 1).unfold(2, 3, 1)                # [B, H, W, C, kh, kw]
    return p.permute(0, 1, 2, 4, 5, 3).reshape(B * H * W, 9 * Cc)


def w2d(w):
    """[Co, Ci, 3, 3] -> [Co, (kh, kw, ci)]."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def wflip(w):
    """[Co, Ci, 3, 3] -> [Ci, (kh, kw, co)] of the flipped kernel: the data gradient is the same gather applied to g."""
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], -1)


def gw_of(mat, co):
    """[Co, (kh, kw, ci)] -> [Co, Ci, 3, 3]."""
    return mat.reshape(co, 3, 3, -1).permute(0, 3, 1, 2)


def dev_w(w, layout):
    w = w.float().cuda().contiguous()
    return w.contiguous(memory_format=torch.channels_last) if layout else w


def within(got, want64, bound64, what):
    got, want64, bound64 = got.detach().double().cpu().reshape(-1), want64.reshape(-1), bound64.reshape(-1)
    assert got.shape == want64.shape, what
    over = (got - want64).abs() - bound64
    assert bool((over <= 0).all()), (what, float(over.max()), float(bound64.max()))
    return float(((got - want64).abs() / bound64.clamp_min(1e-300)).max())


def pre_args(pre, a, b):
    return (None, None) if pre == 0 else (None, b) if pre == 1 else (a, b)


# ---- exact ---------------------------------------------------------------------------------------------------------------------
def test_integer_data_is_exact(amd):
    ops = amd.ops
    a, b = P(0.5), P(-0.5)
    lim = 2 ** 24
    for i, (B, H, W, ci, co) in enumerate(shapes(amd)):
        m = B * H * W
        x, g, w = ints((B, H, W, ci), 3 * i, 1, 4), ints((B, H, W, co), 3 * i + 1, -3, 3), ints((co, ci, 3, 3), 3 * i + 2, -2, 2)
        # the definition: F.conv2d on the circularly padded integers, fp64 of small integers (exact: all below 2^53)
        y64 = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="circular"), w).permute(0, 2, 3, 1).reshape(m, co)
        xs, gs, g2, w2, wf = patches(x), patches(g), g.reshape(m, co), w2d(w), wflip(w)
        assert torch.equal(xs @ w2.t(), y64)                               # the test's own gather is the definition's
        gu64, gw64 = gs @ wf.t(), g2.t() @ xs                              # the hand-computed gradients
        # every partial sum of every output is an integer below 2^24 in any order: the sums of absolute values are
        assert float((xs.abs() @ w2.abs().t()).max()) < lim and float((gs.abs() @ wf.abs().t()).max()) < lim
        assert float((g2.abs().t() @ xs.abs()).max()) < lim and float(gu64.abs().sum()) < 2 ** 53 and abs(float(gu64.sum())) < lim
        gx64 = gu64.reshape(B, H, W, ci)
        xd, gd = x.float().cuda(), g.float().cuda()
        what = (B, H, W, ci, co)
        for layout in (0, 1):
            wd = dev_w(w, layout)
            y = ops.conv3x3_train_forward(xd, wd, a, b)
            g_x, g_w, g_a, g_b = ops.conv3x3_train_backward(gd, xd, wd, a, b)
            assert y.shape == (B, H, W, co) and torch.equal(y.cpu().double().reshape(m, co), y64), (what, layout)
            assert g_x.shape == xd.shape and torch.equal(g_x.cpu().double(), gx64), (what, layout)
            assert g_w.shape == wd.shape and g_w.stride() == wd.stride(), (what, layout)
            assert torch.equal(g_w.cpu().double(), gw_of(gw64, co)), (what, layout)
            assert float(g_a) == float(gu64.sum()) == float(g_b), (what, layout)
        if (B, H, W) in ((1, 3, 11), (1, 3, 43)):           # M = 33, 129: the other two pre-ops and the optional outputs
            y0 = ops.conv3x3_train_forward(xd, wd)
            y1 = ops.conv3x3_train_forward(xd, wd, None, b)                   # u = x - 0.5: multiples of 0.5, still exact
            assert torch.equal(y0.cpu().double().reshape(m, co), y64), what
            assert torch.equal(y1.cpu().double().reshape(m, co), (xs - 0.5) @ w2.t()), what
            gx0, gw0, ga0, gb0 = ops.conv3x3_train_backward(gd, xd, wd)
            assert ga0 is None and gb0 is None and torch.equal(gx0, g_x) and torch.equal(gw0, g_w), what
            gx1, gw1, ga1, gb1 = ops.conv3x3_train_backward(gd, xd, wd, None, b)
            assert ga1 is None and torch.equal(gb1, g_b) and torch.equal(gx1, g_x), what
            assert torch.equal(gw1.cpu().double(), gw_of(g2.t() @ (xs - 0.5), co)), what
            only_x = ops.conv3x3_train_backward(gd, xd, wd, a, b, need_w=False)
            only_w = ops.conv3x3_train_backward(gd, xd, wd, a, b, need_x=False)
            assert only_x[1] is None and torch.equal(only_x[0], g_x) and torch.equal(only_x[2], g_a)
            assert only_w[0] is None and torch.equal(only_w[1], g_w) and torch.equal(only_w[3], g_b)


def test_null_outputs(amd):
    """Each of g_x, g_w, g_a, g_b NULL in turn at the C ABI: the others are the bits of the full call, at two shapes."""
    L, ops = amd._lib, amd.ops
    lib = L.lib()
    a, b = P(0.3), P(-0.2)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    for i, (B, H, W, ci, co) in enumerate([(1, 3, 11, 24, 40), (1, 3, 43, 8, 16)]):
        x, g = rnd((B, H, W, ci), i, 2.0).cuda(), rnd((B, H, W, co), i + 10).cuda()
        wd = dev_w(rnd((co, ci, 3, 3), i + 20, (9 * ci) ** -0.5), i % 2)
        full = ops.conv3x3_train_backward(g, x, wd, a, b)
        ws = torch.empty(lib.vqae_conv3x3_train_workspace_bytes(B, H, W, ci, co), dtype=torch.uint8, device="cuda")
        for skip in range(4):
            outs = [torch.full_like(t, float("nan")) for t in full]
            args = [None if k == skip else outs[k] for k in range(4)]
            L.check(lib.vqae_conv3x3_train_backward_f32(p(g), p(x), p(a), p(b), 2, p(wd), i % 2, B, H, W, ci, co, *map(p, args),
                                                        p(ws), ops._stream()))
            torch.cuda.synchronize()
            for k in range(4):
                if k != skip:
                    assert torch.equal(outs[k], full[k]), (B, H, W, ci, co, skip, k)


# ---- no stray writes -------------------------------------------------------------------------------------------------------------
def test_no_write_outside_the_outputs(amd):
    """y, g_x and g_w as 16-byte-aligned interior slices of sentinel-filled buffers: the sentinel stays on both sides, and every
    element of g_x (pre-filled with NaN) is written."""
    L, ops = amd._lib, amd.ops
    lib = L.lib()
    PAD, SENT = 68, -12345.0                                                     # 68 floats = 17 x 16 bytes
    a, b = P(0.3), P(-0.2)
    for i, (B, H, W, ci, co) in enumerate([(1, 1, 1, 8, 8), (1, 3, 43, 24, 40), two_runs(amd) + (8, 16)]):
        x, g = rnd((B, H, W, ci), i, 2.0).cuda(), rnd((B, H, W, co), i + 10).cuda()
        w = rnd((co, ci, 3, 3), i + 20, (9 * ci) ** -0.5)
        for layout in (0, 1):
            wd = dev_w(w, layout)
            bufs = {k: torch.full((n + 2 * PAD,), SENT, device="cuda") for k, n in
                    (("y", g.numel()), ("g_x", x.numel()), ("g_w", w.numel()))}
            inner = {k: v[PAD:-PAD] for k, v in bufs.items()}
            assert all(t.data_ptr() % 16 == 0 for t in inner.values())
            inner["g_x"].fill_(float("nan"))
            g_a, g_b = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
            ws = torch.empty(lib.vqae_conv3x3_train_workspace_bytes(B, H, W, ci, co), dtype=torch.uint8, device="cuda")
            p = lambda t: ctypes.c_void_p(t.data_ptr())
            L.check(lib.vqae_conv3x3_train_forward_f32(p(x), p(a), p(b), 2, p(wd), layout, B, H, W, ci, co, p(inner["y"]),
                                                       p(ws), ops._stream()))
            L.check(lib.vqae_conv3x3_train_backward_f32(p(g), p(x), p(a), p(b), 2, p(wd), layout, B, H, W, ci, co,
                                                        p(inner["g_x"]), p(inner["g_w"]), p(g_a), p(g_b), p(ws), ops._stream()))
            torch.cuda.synchronize()
            what = (B, H, W, ci, co, layout)
            for k, v in bufs.items():
                assert bool((v[:PAD] == SENT).all()) and bool((v[-PAD:] == SENT).all()), (k,) + what
                assert bool(torch.isfinite(v[PAD:-PAD]).all()), (k,) + what
            want = ops.conv3x3_train_backward(g, x, wd, a, b)
            assert torch.equal(inner["y"].reshape(B, H, W, co), ops.conv3x3_train_forward(x, wd, a, b)), what
            assert torch.equal(inner["g_x"].reshape(x.shape), want[0]), what
            assert torch.equal(inner["g_w"], want[1].as_strided((w.numel(),), (1,))), what


# ---- run to run ------------------------------------------------------------------------------------------------------------------
def test_runs_are_bit_identical(amd):
    ops = amd.ops
    cases = [(1, 3, 43, 24, 40), (1, 1, 257, 64, 128), two_runs(amd) + (16, 16), (2, 16, 32, 128, 256), BIG + (8, 8)]
    for i, (B, H, W, ci, co) in enumerate(cases):
        x, g = rnd((B, H, W, ci), i, 2.0).cuda(), rnd((B, H, W, co), i + 10).cuda()
        w = dev_w(rnd((co, ci, 3, 3), i + 20, (9 * ci) ** -0.5), i % 2)
        a, b = P(0.3), P(-0.2)
        run = lambda: [ops.conv3x3_train_forward(x, w, a, b)] + list(ops.conv3x3_train_backward(g, x, w, a, b))
        for p, q in zip(run(), run()):
            assert torch.equal(p, q), (B, H, W, ci, co)


def test_gradients_repeat_through_autograd(amd):
    """Under conv1x1="hip", conv3x3="hip" no conv of a 'same' block is MIOpen's: every gradient of same_8_4x6 repeats."""
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    cls = functools.partial(PreActFixupResBlock, conv1x1="hip", conv3x3="hip")
    block, x, g, _ = C.block_case("same_8_4x6", cls, device="cuda")
    x = x.contiguous(memory_format=torch.channels_last).requires_grad_()
    grads = []
    for _ in range(2):
        block.zero_grad(set_to_none=True)
        x.grad = None
        block(x).backward(g)
        grads.append(dict({k: p.grad.clone() for k, p in block.named_parameters()}, input=x.grad.clone()))
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
    assert float(grads[0]["branch_conv2.weight"].abs().max()) > 0


# ---- element-wise bounds against the fp64 restatement ------------------------------------------------------------------------------
def test_elementwise_bounds(amd):
    T, ops = amd.train, amd.ops
    R = ops.conv3x3_train_wgrad_run()
    pick = [(1, 1, 1), (1, 2, 2), (2, 3, 3), (1, 3, 11), (1, 3, 43), (1, 1, 257), two_runs(amd), TALL, BIG]
    todo = [s + (2,) for s in shapes(amd) if s[:3] in pick]
    todo += [(1, 3, 43, ci, co, pre) for (ci, co) in PAIRS[::2] for pre in (0, 1)]
    worst = {"y": 0.0, "g_x": 0.0, "g_w": 0.0, "g_a": 0.0, "g_b": 0.0}
    for i, (B, H, W, ci, co, pre) in enumerate(todo):
        m = B * H * W
        x, g, w = rnd((B, H, W, ci), i, 2.0), rnd((B, H, W, co), i + 1000), rnd((co, ci, 3, 3), i + 2000, (9 * ci) ** -0.5)
        a, b = pre_args(pre, P(0.25 - 0.01 * (i % 7)), P(-0.125 + 0.02 * (i % 5)))
        x64, g64, w64, wf64 = x.double(), g.double(), w2d(w.double()), wflip(w.double())
        a64 = a.double().cpu() if a is not None else None
        b64 = b.double().cpu() if b is not None else None
        if pre == 2:
            v = x64 + a64
            e, d = F.elu(v), T.elu_grad(v)
            op = e + b64
            D = U * (v.abs() + 8 * e.abs() + op.abs())
        else:
            v, d = x64, torch.ones_like(x64)
            op = x64 if pre == 0 else x64 + b64
            D = torch.zeros_like(x64) if pre == 0 else U * op.abs()
        what = (B, H, W, ci, co, pre)
        opg, Ds, wabs, g2 = patches(op), patches(D), w64.abs(), g64.reshape(m, co)
        gabs = g2.abs()
        xd, gd, wd = x.cuda(), g.cuda(), dev_w(w, i % 2)
        y = ops.conv3x3_train_forward(xd, wd, a, b)
        by = Ds @ wabs.t() + (9 * ci + 1) * U * ((opg.abs() + Ds) @ wabs.t())
        worst["y"] = max(worst["y"], within(y, opg @ w64.t(), by, ("y",) + what))
        g_x, g_w, g_a, g_b = ops.conv3x3_train_backward(gd, xd, wd, a, b)
        gu64 = (patches(g64) @ wf64.t()).reshape(B, H, W, ci)
        G = ((9 * co + 1) * U * (patches(g64.abs()) @ wf64.abs().t())).reshape(B, H, W, ci)
        gx64 = gu64 * d
        bx = G * d * (1 + 2.0 ** -20) + (U * gu64.abs() * d * (v.abs() + 10) if pre == 2 else 0)
        worst["g_x"] = max(worst["g_x"], within(g_x, gx64, bx, ("g_x",) + what))
        if pre == 2:
            ba = bx.sum() + U * gx64.sum().abs() + TINY * gx64.abs().sum()
            worst["g_a"] = max(worst["g_a"], within(g_a, gx64.sum(), ba, ("g_a",) + what))
        if pre >= 1:
            bb = G.sum() + U * gu64.sum().abs() + TINY * gu64.abs().sum()
            worst["g_b"] = max(worst["g_b"], within(g_b, gu64.sum(), bb, ("g_b",) + what))
        gw64 = g2.t() @ opg
        bw = gabs.t() @ Ds + (min(m, R) + 1) * U * (gabs.t() @ (opg.abs() + Ds)) + U * gw64.abs() + TINY * (gabs.t() @ opg.abs())
        worst["g_w"] = max(worst["g_w"], within(g_w, gw_of(gw64, co), gw_of(bw, co), ("g_w",) + what))
    record_parity("conv3x3_train_bounds", wgrad_run=R, cases=len(todo),
                  **{f"worst_fraction_of_bound_{k}": v for k, v in worst.items()})


# ---- the op against torch's own conv and autograd ---------------------------------------------------------------------------------
def _stock(x, w, a, b, g, device, dtype):
    x, w, a, b = (t.detach().to(device=device, dtype=dtype).requires_grad_() for t in (x, w, a, b))
    y = F.conv2d(F.pad(F.elu(x.permute(0, 3, 1, 2) + a) + b, (1, 1, 1, 1), mode="circular"), w)
    gs = torch.autograd.grad(y, [x, w, a, b], g.to(device=device, dtype=dtype).permute(0, 3, 1, 2))
    return [y.detach().permute(0, 2, 3, 1)] + list(gs)


def test_op_parity(amd):
    ops = amd.ops
    names = ("y", "g_x", "g_w")
    rel = {"hip": [], "cpu": [], "gpu": []}
    fails = []
    cases = [(1, 1, 257, 24, 40), two_runs(amd) + (64, 128), (2, 16, 32, 128, 256), (1, 3, 43, 256, 256), (4, 32, 32, 16, 16)]
    for i, (B, H, W, ci, co) in enumerate(cases):
        x, g, w = rnd((B, H, W, ci), i + 50, 2.0), rnd((B, H, W, co), i + 60), rnd((co, ci, 3, 3), i + 70, (9 * ci) ** -0.5)
        a, b = torch.tensor([0.21]), torch.tensor([-0.13])
        v64 = _stock(x, w, a, b, g, "cpu", torch.float64)
        cpu = _stock(x, w, a, b, g, "cpu", torch.float32)
        gpu = _stock(x, w, a, b, g, "cuda", torch.float32)
        ad, bd, wd = a.cuda(), b.cuda(), dev_w(w, i % 2)
        y = ops.conv3x3_train_forward(x.cuda(), wd, ad, bd)
        g_x, g_w, g_a, g_b = ops.conv3x3_train_backward(g.cuda(), x.cuda(), wd, ad, bd)
        hip = [y, g_x, g_w, g_a, g_b]
        shape = (B, H, W, ci, co)
        for k, name in enumerate(names):
            e_dev, e_cpu, e_gpu = (C.dist(t[k], v64[k]) for t in (hip, cpu, gpu))
            print(f"conv3x3_train_op {shape} {name}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
            record_parity("conv3x3_train_op", shape=list(shape), w_layout=i % 2, tensor=name, e_dev=e_dev, e_ref_cpu32=e_cpu,
                          e_ref_stock_gpu=e_gpu)
            if not e_dev <= BAR * max(e_cpu, e_gpu):
                fails.append((shape, name, e_dev, e_cpu, e_gpu))
        for k in (3, 4):
            for tag, t in (("hip", hip), ("cpu", cpu), ("gpu", gpu)):
                rel[tag].append(float(t[k].double().cpu().reshape(())) / float(v64[k]))
    one = torch.ones(len(rel["hip"]), dtype=torch.float64)
    e_dev, e_cpu, e_gpu = (C.dist(torch.tensor(rel[t], dtype=torch.float64), one) for t in ("hip", "cpu", "gpu"))
    print(f"conv3x3_train_op scalars: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
    record_parity("conv3x3_train_op", tensor="scalars", e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
    if not e_dev <= BAR * max(e_cpu, e_gpu):
        fails.append(("scalars", e_dev, e_cpu, e_gpu))
    assert not fails, fails


# ---- the blocks and the whole model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("routes", [("torch", "torch", "hip"), ("hip", "hip", "hip")], ids=["conv3x3", "all"])
@pytest.mark.parametrize("case", BLOCK_CASES)
def test_block_parity_hip_route(amd, case, routes):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    cls = functools.partial(PreActFixupResBlock, conv1x1=routes[0], conv_down=routes[1], conv3x3=routes[2])
    block, x, g, ref = C.block_case(case, cls, device="cuda")
    assert (block.conv1x1, block.conv_down, block.conv3x3) == routes
    T.stats.update({k: 0 for k in STATS})
    got = C.block_results(block, x.contiguous(memory_format=torch.channels_last), g, lambda b, t: b(t))
    counts = tuple(T.stats[k] for k in STATS)
    stock = C.block_results(block, x, g, T.block_forward_torch)
    torch.cuda.synchronize()
    assert counts[:2] == (1, 0), counts
    assert counts[2:4] == (CONV1X1_COUNTS[case] if routes[0] == "hip" else (0, 0)) and counts[4:] == (0, 0), counts
    assert set(got) == set(ref)
    fails = []
    for k, (v64, e_cpu) in ref.items():
        e_dev, e_gpu = C.dist(got[k], v64.reshape(got[k].shape)), C.dist(stock[k], v64.reshape(stock[k].shape))
        print(f"conv3x3_train_block {case} {routes} {k}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
        record_parity("conv3x3_train_block", case=case, conv1x1=routes[0], conv_down=routes[1], conv3x3=routes[2], tensor=k,
                      e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
        assert bool(torch.isfinite(got[k]).all())
        if not e_dev <= BAR * max(e_cpu, e_gpu):
            fails.append((k, e_dev, e_cpu, e_gpu))
    assert not fails, fails


def test_closed_loop_hip_routes(amd):
    """The fixture's three steps with forward_train(conv1x1="hip", conv_down="hip", conv3x3="hip") + FusedAdamW on spec tiny:
    the recorded codes exactly; losses, all parameters and the quantiser's buffers (one vector each) within 4 x e_ref, as
    test_whole_model_closed_loop."""
    from test_fixup_train_gpu import _run_loop, _stock_forward
    T = amd.train
    z = C.fixture()
    T.stats.update({k: 0 for k in STATS})
    fused = lambda m, x: T.forward_train(m, x, return_indices=True, conv1x1="hip", conv_down="hip", conv3x3="hip")
    model, sd0, losses, idxs = _run_loop(amd, fused, amd.FusedAdamW, True)
    assert T.stats["conv3x3_hip"] > 0 and T.stats["conv3x3_hip"] % 3 == 0 and T.stats["conv3x3_fallbacks"] == 0
    assert T.stats["conv_down_hip"] == 3 * 4 and T.stats["conv_down_fallbacks"] == 0
    assert T.stats["conv1x1_hip"] > 0 and T.stats["conv1x1_fallbacks"] == 0
    smodel, ssd0, slosses, sidxs = _run_loop(amd, _stock_forward(amd), torch.optim.AdamW, False)
    for i in range(3):
        assert torch.equal(idxs[i].to(torch.int16), torch.from_numpy(z["loop/idx"][i])), f"step {i}: codes differ"
    stock_idx_ok = all(torch.equal(sidxs[i].to(torch.int16), torch.from_numpy(z["loop/idx"][i])) for i in range(3))
    e, e_cpu = C.loss_distances(losses)
    rows = [("losses", e, e_cpu, C.loss_distances(slosses)[0] if stock_idx_ok else 0.0)]
    mine, stock = C.loop_final_groups(model, sd0), C.loop_final_groups(smodel, ssd0)
    for tag, (got, want, e32) in mine.items():
        rows.append((tag, C.dist(got, want), e32, C.dist(stock[tag][0], want) if stock_idx_ok else 0.0))
    fails = []
    for tag, e_dev, e_cpu, e_gpu in rows:
        print(f"conv3x3_train_loop {tag}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
        record_parity("conv3x3_train_loop", tensor=tag, e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
        if not e_dev <= BAR * max(e_cpu, e_gpu):
            fails.append((tag, e_dev, e_cpu, e_gpu))
    assert not fails, fails
