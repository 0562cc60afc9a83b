"""GPU: the trainable 2x2, stride-2 conv kernels (csrc/conv_train.hip) behind vqae_amd.ops.conv_down_train_* and
train.conv_down.  x [B, 2 OH, 2 OW, Ci], y [B, OH, OW, Co], M = B OH OW rows of a GEMM with K = 4 Ci.

Shapes: (B, OH, OW) in {(1,1,1), (1,1,2), (2,3,5), (1,1,31), (1,4,8), (1,3,11), (1,1,127), (2,8,8), (1,3,43), (1,1,257),
(3,7,49)}: M = 1, 2, 30, 31, 32, 33, 127, 128, 129, 257 and 2 R + 5 (R = vqae_conv_down_train_wgrad_run() = 512; another R
takes (1, 1, 2 R + 5)) -- around the 32-row MFMA tile, the 64-row weight-gradient step, the 128-row workgroup tile, more than
one fp32 run; rows of a tile cross image rows and batch entries -- x (Ci, Co) in {(8,8), (8,16), (16,16), (24,40), (32,64),
(64,128), (128,256), (256,256)} (every tile count of the templates, K and N tails, one to four column pieces of the data
gradient), the last two with M <= 129 only; and (25, 49, 107), M = 2^17 + 3, with (8,8) and (16,8).  Both weight layouts.

Exact: small-integer data with a = 0.5, b = -0.5, so u = ELU(x + a) + b = x and ELU' = 1 without rounding; every partial sum
of every output is an integer below 2^24 (checked from the data), so y, g_x, g_w, g_a, g_b are the exact results whatever
the order of summation: a row, tap or channel counted twice or not at all at any tile edge shows.

No stray writes: the library called on interior slices of sentinel-filled buffers.  Run to run: two calls give the same bits.

Element-wise bounds against the fp64 evaluation of the restatement, from the arithmetic alone -- the derivation of
tests/test_conv1x1_train_gpu.py with the term counts of this GEMM (u = 2^-24; expm1f / expf taken as <= 4 ulp = 8 u relative; a
sum of K fp32 products accumulated in fp32 in any order is within (K + 1) u sum|terms|; nothing measured).  v = x + a,
e = ELU(v), op = e + b the operand, d = ELU'(v); sums over the 4 Ci gathered columns k = (kh, kw, ci):
    operand   D = u (|v| + 8 |e| + |op|)                     (0 for pre = 0, u |op| for pre = 1)
    y         sum_k D |w| + (4 Ci + 1) u sum_k (|op| + D) |w|
    g_u       G = (Co + 1) u sum_co |g| |w|
    g_x       G d (1 + 2^-20) + u |g_u| d (|v| + 10)
    g_a, g_b  the sum of the element bounds + u |sum| + 2^-40 sum |terms|      (fp64 sums of fp32 values, rounded once)
    g_w       sum_m |g| D + (min(M, R) + 1) u sum_m |g| (|op| + D) + u |g_w| + 2^-40 sum_m |g| |op|

Op parity: e_dev = ||hip - v64|| / ||v64|| per output <= 4 x e_ref, e_ref the larger of CPU fp32 autograd of
F.conv2d(F.elu(x + a) + b, w, stride=2) and the same on the GPU with stock torch ops; the one-element outputs of all parity
shapes form ONE vector of relative values (tests/fixup_train_cases.py says why).  Block and closed loop: the bar and the e_ref
construction of test_fixup_train_gpu.py, under conv_down="hip" and under both keywords "hip".
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
SMALL = [(1, 1, 1), (1, 1, 2), (2, 3, 5), (1, 1, 31), (1, 4, 8), (1, 3, 11), (1, 1, 127), (2, 8, 8), (1, 3, 43), (1, 1, 257)]
BIG = (25, 49, 107)
assert BIG[0] * BIG[1] * BIG[2] == 2 ** 17 + 3


def two_runs(amd):
    r = amd.ops.conv_down_train_wgrad_run()
    return (3, 7, 49) if r == 512 else (1, 1, 2 * r + 5)


def shapes(amd):
    out = []
    for bhw in SMALL + [two_runs(amd)]:
        m = bhw[0] * bhw[1] * bhw[2]
        out += [bhw + p for p in PAIRS if not (p in WIDE and m > 129)]
    return out + [BIG + (8, 8), BIG + (16, 8)]


def P(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


def ints(shape, seed, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def s2d(t):
    """[B, 2 OH, 2 OW, C] -> [M, 4 C], column (kh, kw, c)."""
    B, H, W, Cc = t.shape
    return t.reshape(B, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4 * Cc)


def d2s(m, B, OH, OW):
    Cc = m.shape[-1] // 4
    return m.reshape(B, OH, OW, 2, 2, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * OH, 2 * OW, Cc)


def w2d(w):
    """[Co, Ci, 2, 2] -> [Co, (kh, kw, ci)]."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def gw_of(mat, co):
    """[Co, (kh, kw, ci)] -> [Co, Ci, 2, 2]."""
    return mat.reshape(co, 2, 2, -1).permute(0, 3, 1, 2)


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
    for i, (B, OH, OW, ci, co) in enumerate(shapes(amd)):
        m = B * OH * OW
        x, g, w = ints((B, 2 * OH, 2 * OW, ci), 3 * i, 1, 4), ints((B, OH, OW, co), 3 * i + 1, -3, 3), ints((co, ci, 2, 2), 3 * i + 2, -2, 2)
        xs, g2, w2 = s2d(x), g.reshape(m, co), w2d(w)
        y64, gu64, gw64 = xs @ w2.t(), g2 @ w2, g2.t() @ xs                 # fp64 of small integers: exact (all below 2^53)
        # every partial sum of every output is an integer below 2^24 in any order: the sums of absolute values are
        assert float((xs.abs() @ w2.abs().t()).max()) < lim and float((g2.abs() @ w2.abs()).max()) < lim
        assert float((g2.abs().t() @ xs.abs()).max()) < lim and float(gu64.abs().sum()) < 2 ** 53 and abs(float(gu64.sum())) < lim
        gx64 = d2s(gu64, B, OH, OW)
        xd, gd = x.float().cuda(), g.float().cuda()
        what = (B, OH, OW, ci, co)
        for layout in (0, 1):
            wd = dev_w(w, layout)
            y = ops.conv_down_train_forward(xd, wd, a, b)
            g_x, g_w, g_a, g_b = ops.conv_down_train_backward(gd, xd, wd, a, b)
            assert y.shape == (B, OH, OW, co) and torch.equal(y.cpu().double().reshape(m, co), y64), (what, layout)
            assert g_x.shape == xd.shape and torch.equal(g_x.cpu().double(), gx64), (what, layout)
            assert g_w.shape == wd.shape and g_w.stride() == wd.stride(), (what, layout)
            assert torch.equal(g_w.cpu().double(), gw_of(gw64, co)), (what, layout)
            assert float(g_a) == float(gu64.sum()) == float(g_b), (what, layout)
        if (B, OH, OW) in ((1, 3, 11), (1, 3, 43)):         # M = 33, 129: the other two pre-ops and the optional outputs
            y0 = ops.conv_down_train_forward(xd, wd)
            y1 = ops.conv_down_train_forward(xd, wd, None, b)                 # u = x - 0.5: multiples of 0.5, still exact
            assert torch.equal(y0.cpu().double().reshape(m, co), y64), what
            assert torch.equal(y1.cpu().double().reshape(m, co), (xs - 0.5) @ w2.t()), what
            gx0, gw0, ga0, gb0 = ops.conv_down_train_backward(gd, xd, wd)
            assert ga0 is None and gb0 is None and torch.equal(gx0, g_x) and torch.equal(gw0, g_w), what
            gx1, gw1, ga1, gb1 = ops.conv_down_train_backward(gd, xd, wd, None, b)
            assert ga1 is None and torch.equal(gb1, g_b) and torch.equal(gx1, g_x), what
            assert torch.equal(gw1.cpu().double(), gw_of(g2.t() @ (xs - 0.5), co)), what
            only_x = ops.conv_down_train_backward(gd, xd, wd, a, b, need_w=False)
            only_w = ops.conv_down_train_backward(gd, xd, wd, a, b, need_x=False)
            assert only_x[1] is None and torch.equal(only_x[0], g_x) and torch.equal(only_x[2], g_a)
            assert only_w[0] is None and torch.equal(only_w[1], g_w) and torch.equal(only_w[3], g_b)


# ---- no stray writes -------------------------------------------------------------------------------------------------------------
def test_no_write_outside_the_outputs(amd):
    """y, g_x and g_w as 16-byte-aligned interior slices of sentinel-filled buffers: the sentinel stays on both sides, and every
    element of g_x (pre-filled with NaN) is written."""
    L, ops = amd._lib, amd.ops
    lib = L.lib()
    PAD, SENT = 68, -12345.0                                                     # 68 floats = 17 x 16 bytes
    a, b = P(0.3), P(-0.2)
    for i, (B, OH, OW, ci, co) in enumerate([(1, 1, 1, 8, 8), (1, 3, 43, 24, 40), two_runs(amd) + (8, 16)]):
        x, g = rnd((B, 2 * OH, 2 * OW, ci), i, 2.0).cuda(), rnd((B, OH, OW, co), i + 10).cuda()
        w = rnd((co, ci, 2, 2), i + 20, (4 * ci) ** -0.5)
        for layout in (0, 1):
            wd = dev_w(w, layout)
            bufs = {k: torch.full((n + 2 * PAD,), SENT, device="cuda") for k, n in
                    (("y", g.numel()), ("g_x", x.numel()), ("g_w", w.numel()))}
            inner = {k: v[PAD:-PAD] for k, v in bufs.items()}
            assert all(t.data_ptr() % 16 == 0 for t in inner.values())
            inner["g_x"].fill_(float("nan"))
            g_a, g_b = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
            ws = torch.empty(lib.vqae_conv_down_train_workspace_bytes(B, 2 * OH, 2 * OW, ci, co), dtype=torch.uint8, device="cuda")
            p = lambda t: ctypes.c_void_p(t.data_ptr())
            L.check(lib.vqae_conv_down_train_forward_f32(p(x), p(a), p(b), 2, p(wd), layout, B, 2 * OH, 2 * OW, ci, co, p(inner["y"]),
                                                         p(ws), ops._stream()))
            L.check(lib.vqae_conv_down_train_backward_f32(p(g), p(x), p(a), p(b), 2, p(wd), layout, B, 2 * OH, 2 * OW, ci, co,
                                                          p(inner["g_x"]), p(inner["g_w"]), p(g_a), p(g_b), p(ws), ops._stream()))
            torch.cuda.synchronize()
            what = (B, OH, OW, ci, co, layout)
            for k, v in bufs.items():
                assert bool((v[:PAD] == SENT).all()) and bool((v[-PAD:] == SENT).all()), (k,) + what
                assert bool(torch.isfinite(v[PAD:-PAD]).all()), (k,) + what
            want = ops.conv_down_train_backward(g, x, wd, a, b)
            assert torch.equal(inner["y"].reshape(B, OH, OW, co), ops.conv_down_train_forward(x, wd, a, b)), what
            assert torch.equal(inner["g_x"].reshape(x.shape), want[0]), what
            assert torch.equal(inner["g_w"], want[1].as_strided((w.numel(),), (1,))), what


# ---- run to run ------------------------------------------------------------------------------------------------------------------
def test_runs_are_bit_identical(amd):
    ops = amd.ops
    cases = [(1, 3, 43, 24, 40), (1, 1, 257, 64, 128), two_runs(amd) + (16, 16), (2, 16, 32, 128, 256), BIG + (8, 8)]
    for i, (B, OH, OW, ci, co) in enumerate(cases):
        x, g = rnd((B, 2 * OH, 2 * OW, ci), i, 2.0).cuda(), rnd((B, OH, OW, co), i + 10).cuda()
        w = dev_w(rnd((co, ci, 2, 2), i + 20, (4 * ci) ** -0.5), i % 2)
        a, b = P(0.3), P(-0.2)
        run = lambda: [ops.conv_down_train_forward(x, w, a, b)] + list(ops.conv_down_train_backward(g, x, w, a, b))
        for p, q in zip(run(), run()):
            assert torch.equal(p, q), (B, OH, OW, ci, co)


def test_gradients_repeat_through_autograd(amd):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    torch.manual_seed(3)
    block = PreActFixupResBlock(16, 32, "down", n_layers=4, conv1x1="hip", conv_down="hip").cuda()
    with torch.no_grad():
        torch.nn.init.normal_(block.branch_conv3.weight, std=0.1)
    x = rnd((3, 16, 18, 22), 9).cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    g = rnd((3, 32, 9, 11), 10).cuda().contiguous(memory_format=torch.channels_last)
    grads = []
    for _ in range(2):
        block.zero_grad(set_to_none=True)
        x.grad = None
        block(x).backward(g)
        grads.append(dict({k: p.grad.clone() for k, p in block.named_parameters()}, input=x.grad.clone()))
    for k in grads[0]:                                      # under both keywords no conv of a 'down' block is MIOpen's
        assert torch.equal(grads[0][k], grads[1][k]), k
    assert float(grads[0]["branch_conv2.weight"].abs().max()) > 0 and float(grads[0]["skip_conv.weight"].abs().max()) > 0


# ---- element-wise bounds against the fp64 restatement ------------------------------------------------------------------------------
def test_elementwise_bounds(amd):
    T, ops = amd.train, amd.ops
    R = ops.conv_down_train_wgrad_run()
    big_m = [(1, 3, 11), (1, 3, 43), (1, 1, 257), two_runs(amd), BIG]
    todo = [s + (2,) for s in shapes(amd) if s[:3] in big_m]
    todo += [(1, 3, 43, ci, co, pre) for (ci, co) in PAIRS[::2] for pre in (0, 1)]
    worst = {"y": 0.0, "g_x": 0.0, "g_w": 0.0, "g_a": 0.0, "g_b": 0.0}
    for i, (B, OH, OW, ci, co, pre) in enumerate(todo):
        m = B * OH * OW
        x, g, w = rnd((B, 2 * OH, 2 * OW, ci), i, 2.0), rnd((B, OH, OW, co), i + 1000), rnd((co, ci, 2, 2), i + 2000, (4 * ci) ** -0.5)
        a, b = pre_args(pre, P(0.25 - 0.01 * (i % 7)), P(-0.125 + 0.02 * (i % 5)))
        x64, g64, w64 = x.double(), g.double().reshape(m, co), w2d(w.double())
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
        what = (B, OH, OW, ci, co, pre)
        opg, Ds, wabs, gabs = s2d(op), s2d(D), w64.abs(), g64.abs()
        xd, gd, wd = x.cuda(), g.cuda(), dev_w(w, i % 2)
        y = ops.conv_down_train_forward(xd, wd, a, b)
        by = Ds @ wabs.t() + (4 * ci + 1) * U * ((opg.abs() + Ds) @ wabs.t())
        worst["y"] = max(worst["y"], within(y, opg @ w64.t(), by, ("y",) + what))
        g_x, g_w, g_a, g_b = ops.conv_down_train_backward(gd, xd, wd, a, b)
        gu64 = d2s(g64 @ w64, B, OH, OW)
        G = d2s((co + 1) * U * (gabs @ wabs), B, OH, OW)
        gx64 = gu64 * d
        bx = G * d * (1 + 2.0 ** -20) + (U * gu64.abs() * d * (v.abs() + 10) if pre == 2 else 0)
        worst["g_x"] = max(worst["g_x"], within(g_x, gx64, bx, ("g_x",) + what))
        if pre == 2:
            ba = bx.sum() + U * gx64.sum().abs() + TINY * gx64.abs().sum()
            worst["g_a"] = max(worst["g_a"], within(g_a, gx64.sum(), ba, ("g_a",) + what))
        if pre >= 1:
            bb = G.sum() + U * gu64.sum().abs() + TINY * gu64.abs().sum()
            worst["g_b"] = max(worst["g_b"], within(g_b, gu64.sum(), bb, ("g_b",) + what))
        gw64 = g64.t() @ opg
        bw = gabs.t() @ Ds + (min(m, R) + 1) * U * (gabs.t() @ (opg.abs() + Ds)) + U * gw64.abs() + TINY * (gabs.t() @ opg.abs())
        worst["g_w"] = max(worst["g_w"], within(g_w, gw_of(gw64, co), gw_of(bw, co), ("g_w",) + what))
    record_parity("conv_down_train_bounds", wgrad_run=R, cases=len(todo),
                  **{f"worst_fraction_of_bound_{k}": v for k, v in worst.items()})


# ---- the op against torch's own conv and autograd ---------------------------------------------------------------------------------
def _stock(x, w, a, b, g, device, dtype):
    x, w, a, b = (t.detach().to(device=device, dtype=dtype).requires_grad_() for t in (x, w, a, b))
    y = F.conv2d(F.elu(x.permute(0, 3, 1, 2) + a) + b, w, stride=2)
    gs = torch.autograd.grad(y, [x, w, a, b], g.to(device=device, dtype=dtype).permute(0, 3, 1, 2))
    return [y.detach().permute(0, 2, 3, 1)] + list(gs)


def test_op_parity(amd):
    ops = amd.ops
    names = ("y", "g_x", "g_w")
    rel = {"hip": [], "cpu": [], "gpu": []}
    fails = []
    cases = [(1, 1, 257, 24, 40), two_runs(amd) + (64, 128), (2, 16, 32, 128, 256), (1, 3, 43, 256, 256), (4, 32, 32, 16, 16)]
    for i, (B, OH, OW, ci, co) in enumerate(cases):
        x, g, w = rnd((B, 2 * OH, 2 * OW, ci), i + 50, 2.0), rnd((B, OH, OW, co), i + 60), rnd((co, ci, 2, 2), i + 70, (4 * ci) ** -0.5)
        a, b = torch.tensor([0.21]), torch.tensor([-0.13])
        v64 = _stock(x, w, a, b, g, "cpu", torch.float64)
        cpu = _stock(x, w, a, b, g, "cpu", torch.float32)
        gpu = _stock(x, w, a, b, g, "cuda", torch.float32)
        ad, bd, wd = a.cuda(), b.cuda(), dev_w(w, i % 2)
        y = ops.conv_down_train_forward(x.cuda(), wd, ad, bd)
        g_x, g_w, g_a, g_b = ops.conv_down_train_backward(g.cuda(), x.cuda(), wd, ad, bd)
        hip = [y, g_x, g_w, g_a, g_b]
        shape = (B, OH, OW, ci, co)
        for k, name in enumerate(names):
            e_dev, e_cpu, e_gpu = (C.dist(t[k], v64[k]) for t in (hip, cpu, gpu))
            print(f"conv_down_train_op {shape} {name}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
            record_parity("conv_down_train_op", shape=list(shape), w_layout=i % 2, tensor=name, e_dev=e_dev, e_ref_cpu32=e_cpu,
                          e_ref_stock_gpu=e_gpu)
            if not e_dev <= BAR * max(e_cpu, e_gpu):
                fails.append((shape, name, e_dev, e_cpu, e_gpu))
        for k in (3, 4):
            for tag, t in (("hip", hip), ("cpu", cpu), ("gpu", gpu)):
                rel[tag].append(float(t[k].double().cpu().reshape(())) / float(v64[k]))
    one = torch.ones(len(rel["hip"]), dtype=torch.float64)
    e_dev, e_cpu, e_gpu = (C.dist(torch.tensor(rel[t], dtype=torch.float64), one) for t in ("hip", "cpu", "gpu"))
    print(f"conv_down_train_op scalars: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
    record_parity("conv_down_train_op", tensor="scalars", e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
    if not e_dev <= BAR * max(e_cpu, e_gpu):
        fails.append(("scalars", e_dev, e_cpu, e_gpu))
    assert not fails, fails


# ---- the block and the whole model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("routes", [("torch", "hip"), ("hip", "hip")], ids=["conv_down", "both"])
def test_down_block_parity_hip_route(amd, routes):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    case = "down_8_16_4x6"
    cls = functools.partial(PreActFixupResBlock, conv1x1=routes[0], conv_down=routes[1])
    block, x, g, ref = C.block_case(case, cls, device="cuda")
    assert (block.conv1x1, block.conv_down) == routes
    T.stats.update(conv_down_hip=0, conv_down_fallbacks=0, conv1x1_hip=0, conv1x1_fallbacks=0)
    got = C.block_results(block, x.contiguous(memory_format=torch.channels_last), g, lambda b, t: b(t))
    counts = tuple(T.stats[k] for k in ("conv_down_hip", "conv_down_fallbacks", "conv1x1_hip", "conv1x1_fallbacks"))
    stock = C.block_results(block, x, g, T.block_forward_torch)
    torch.cuda.synchronize()
    assert counts == (2, 0, 2 if routes[0] == "hip" else 0, 0), counts
    assert set(got) == set(ref)
    fails = []
    for k, (v64, e_cpu) in ref.items():
        e_dev, e_gpu = C.dist(got[k], v64.reshape(got[k].shape)), C.dist(stock[k], v64.reshape(stock[k].shape))
        print(f"conv_down_train_block {case} {routes} {k}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
        record_parity("conv_down_train_block", case=case, conv1x1=routes[0], conv_down=routes[1], tensor=k, e_dev=e_dev,
                      e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
        assert bool(torch.isfinite(got[k]).all())
        if not e_dev <= BAR * max(e_cpu, e_gpu):
            fails.append((k, e_dev, e_cpu, e_gpu))
    assert not fails, fails


def test_closed_loop_hip_routes(amd):
    """The fixture's three steps with forward_train(conv1x1="hip", conv_down="hip") + FusedAdamW on spec tiny (its two 'down'
    blocks are 8 -> 16 and 16 -> 32): the recorded codes exactly; losses, all parameters and the quantiser's buffers (one vector
    each) within 4 x e_ref, as test_whole_model_closed_loop."""
    from test_fixup_train_gpu import _run_loop, _stock_forward
    T = amd.train
    z = C.fixture()
    T.stats.update(conv_down_hip=0, conv_down_fallbacks=0, conv1x1_hip=0, conv1x1_fallbacks=0)
    fused = lambda m, x: T.forward_train(m, x, return_indices=True, conv1x1="hip", conv_down="hip")
    model, sd0, losses, idxs = _run_loop(amd, fused, amd.FusedAdamW, True)
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
        print(f"conv_down_train_loop {tag}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
        record_parity("conv_down_train_loop", tensor=tag, e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
        if not e_dev <= BAR * max(e_cpu, e_gpu):
            fails.append((tag, e_dev, e_cpu, e_gpu))
    assert not fails, fails
