"""GPU: the trainable zero-padded 3x3 conv kernels with a 3-channel side (csrc/conv_train_thin.hip) behind
vqae_amd.ops.conv3x3z_train_* and train.conv3x3z.  x [B, H, W, Ci], y [B, H, W, Co] = bias + conv3x3(uz, w), u = x + c, uz = u
inside the image and 0 outside (F.conv2d(x + c, w, bias, padding=1)); M = B H W rows.

Shapes (B, H, W): the padding cases (1,1,1), (1,1,2), (1,2,1), (1,2,2), (1,1,3), (1,3,1), (2,3,3), where every tap but the centre may
lie outside; the tile edges (2,3,5), (1,1,31), (1,4,8), (1,3,11), (1,1,127), (2,8,8), (1,3,43), (1,1,257) -- around the 8 x 32 pixel
tile (several tiles per image row, tiles crossing batch entries) and the sub-lane split of a weight-gradient run; a shape with
more than two fp32 runs, (3,7,49) = 2 R + 5 rows for R = vqae_conv3x3z_train_wgrad_run() = 512 (another R takes (1,1,2 R + 5));
the narrow tall (1,70,1); x (Ci, Co) in {(3,8), (3,16), (3,32), (3,64), (8,3), (16,3), (64,3), (256,3)}, the last two with M <= 129
only; and (25,49,107), M = 2^17 + 3, with (3,8) and (8,3).  Both weight layouts.  Every case runs with c = 0.5 != 0: padding
shifted by c shows at every image edge.

Exact: integer x, w, g, bias in -3 .. 3 and c = 0.5, so every term of every output is a multiple of 1/2 and every sum of absolute
terms is below 2^23 (asserted from the data; 9 M < 2^21 at 2^17 + 3 rows): y, g_x, g_w, g_bias are the exact results whatever the
order of summation, g_c (fp64 sums, rounded once) whenever the sum fits fp32, which is asserted too.  The reference is fp64
F.conv2d(..., padding=1) and its fp64 autograd.

No stray writes: the library called on interior slices of sentinel-filled buffers.  Run to run: two calls give the same bits.

Element-wise bounds against the fp64 evaluation of the restatement, from the arithmetic alone -- the derivation of
tests/test_conv_down_train_gpu.py with the term counts of these direct convs (u = 2^-24; a sum of n fp32 terms accumulated in
fp32 in any order, with or without fused multiply-adds, is within (n + 1) u sum|terms|; nothing measured).  op = x + c the
operand inside the image (one rounding: D = u |op|; D = 0 for pre = 0), 0 outside; sums over the taps inside the image:
    y         n = 9 Ci + 1 terms (the bias is one):   sum D |w| + (9 Ci + 2) u (sum (|op| + D) |w| + |bias|)
    g_x       n = 9 Co terms:                          G = (9 Co + 1) u sum_{kh,kw,co} |g| |w|
    g_c       sum G + u |sum g_x| + 2^-40 sum |g_x|                       (fp64 sums of fp32 values, rounded once)
    g_w       n = min(M, R) + 1:   sum_m |g| D + (min(M, R) + 1) u sum_m |g| (|op| + D) + u |g_w| + 2^-40 sum_m |g| |op|
    g_bias    n = min(M, R) + 1:   (min(M, R) + 1) u sum_m |g| + u |g_bias| + 2^-40 sum_m |g|
(g_w, g_bias: fp32 over a run of at most R rows, the runs in fp64, one rounding at the end.)

Op parity: e_dev = ||hip - v64|| / ||v64|| per output <= 4 x e_ref, e_ref the larger of CPU fp32 autograd of
F.conv2d(x + c, w, bias, padding=1) and the same on the GPU with stock torch ops; the one-element outputs (g_c) of all parity
shapes form ONE vector of relative values (tests/fixup_train_cases.py says why).  Blocks and closed loop: the bar and the e_ref
construction of test_fixup_train_gpu.py, under conv3x3z="hip" alone and under all four keywords "hip".

Whole-step determinism: two deep copies of a model, one batch, all four keywords "hip", step + backward: every .grad is
bit-identical between the copies, for spec tiny and spec tinyP.
"""
import copy
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
PAIRS = [(3, 8), (3, 16), (3, 32), (3, 64), (8, 3), (16, 3), (64, 3), (256, 3)]
WIDE = [(64, 3), (256, 3)]
PADDING = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (1, 2, 2), (1, 1, 3), (1, 3, 1), (2, 3, 3)]
EDGES = [(2, 3, 5), (1, 1, 31), (1, 4, 8), (1, 3, 11), (1, 1, 127), (2, 8, 8), (1, 3, 43), (1, 1, 257)]
TALL = (1, 70, 1)
BIG = (25, 49, 107)
assert BIG[0] * BIG[1] * BIG[2] == 2 ** 17 + 3
ALL4 = dict(conv1x1="hip", conv_down="hip", conv3x3="hip", conv3x3z="hip")
STATS = ("conv3x3z_hip", "conv3x3z_fallbacks", "conv3x3_hip", "conv3x3_fallbacks", "conv1x1_hip", "conv1x1_fallbacks",
         "conv_down_hip", "conv_down_fallbacks")


def three_runs(amd):
    r = amd.ops.conv3x3z_train_wgrad_run()
    return (3, 7, 49) if r == 512 else (1, 1, 2 * r + 5)


def shapes_of(amd, pair):
    out = [s for s in PADDING + EDGES + [three_runs(amd), TALL] if not (pair in WIDE and s[0] * s[1] * s[2] > 129)]
    return out + ([BIG] if pair in ((3, 8), (8, 3)) else [])


def P(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


def ints(shape, seed, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def dev_w(w, layout):
    w = w.float().cuda().contiguous()
    return w.contiguous(memory_format=torch.channels_last) if layout else w


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def conv64(x, w, bias, c, g, device="cpu", dtype=torch.float64):
    """F.conv2d(x + c, w, bias, padding=1) and its autograd in `dtype` on `device` -> {y, g_x, g_w, g_bias, g_c} (channel-last)."""
    t = lambda v: None if v is None else v.detach().to(device=device, dtype=dtype).requires_grad_()
    x, w, bias, c = t(x), t(w), t(bias), t(c)
    y = F.conv2d(nchw(x if c is None else x + c), w, bias, padding=1)
    wrt = {"g_x": x, "g_w": w, "g_bias": bias, "g_c": c}
    wrt = {k: v for k, v in wrt.items() if v is not None}
    gs = torch.autograd.grad(y, list(wrt.values()), nchw(g.to(device=device, dtype=dtype)))
    out = dict(zip(wrt, gs), y=nhwc(y.detach()))
    if "g_c" in out:
        out["g_c"] = out["g_c"].reshape(1)
    return out


def taps_w(a, gabs):
    """sum_m gabs[m][co] az[m + tap][ci] as a [Co, Ci, 3, 3] tensor (az = a inside the image, 0 outside), in fp64: the weight
    gradient of the zero-padded conv, which is linear in the weight."""
    w0 = torch.zeros(gabs.shape[-1], a.shape[-1], 3, 3, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(F.conv2d(nchw(a), w0, padding=1), w0, nchw(gabs))[0]


def taps_x(gabs, wabs):
    """sum_{tap,co} gabs[p - tap][co] wabs[co][ci][tap] over the positions inside the image, [B, H, W, Ci]."""
    return nhwc(F.conv_transpose2d(nchw(gabs), wabs, padding=1))


def within(got, want64, bound64, what):
    got, want64, bound64 = got.detach().double().cpu().reshape(-1), want64.reshape(-1), bound64.reshape(-1)
    assert got.shape == want64.shape, what
    over = (got - want64).abs() - bound64
    assert bool((over <= 0).all()), (what, float(over.max()), float(bound64.max()))
    return float(((got - want64).abs() / bound64.clamp_min(1e-300)).max())


def same(got, want64):
    return got.shape == want64.shape and torch.equal(got.detach().cpu().double(), want64)


# ---- exact ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_integer_data_is_exact(amd, pair):
    ops = amd.ops
    ci, co = pair
    c = P(0.5)
    lim = 2.0 ** 23
    for i, (B, H, W) in enumerate(shapes_of(amd, pair)):
        x, g = ints((B, H, W, ci), 4 * i), ints((B, H, W, co), 4 * i + 1)
        w, bias = ints((co, ci, 3, 3), 4 * i + 2), ints((co,), 4 * i + 3)
        want = conv64(x, w, bias, c.cpu(), g)
        u = x + 0.5
        # every sum of absolute terms is a multiple of 1/2 below 2^23: exact in fp32 in any order, fused or not
        sums = (nhwc(F.conv2d(nchw(u.abs()), w.abs(), bias.abs(), padding=1)), taps_x(g.abs(), w.abs()), taps_w(u.abs(), g.abs()),
                g.abs().sum((0, 1, 2)))
        for s in sums:
            assert float(s.max()) < lim and bool((2 * s == (2 * s).round()).all()), (B, H, W, pair)
        assert abs(float(want["g_c"])) < 2 ** 24 and float(want["g_x"].abs().sum()) < 2 ** 53
        xd, gd, bd = x.float().cuda(), g.float().cuda(), bias.float().cuda()
        what = (B, H, W, ci, co)
        for layout in (0, 1):
            wd = dev_w(w, layout)
            y = ops.conv3x3z_train_forward(xd, wd, bd, c)
            g_x, g_w, g_bias, g_c = ops.conv3x3z_train_backward(gd, xd, wd, c, need_bias=True)
            assert same(y, want["y"]), (what, layout)
            assert same(g_x, want["g_x"]), (what, layout)
            assert g_w.shape == wd.shape and g_w.stride() == wd.stride() and same(g_w, want["g_w"]), (what, layout)
            assert same(g_bias, want["g_bias"]) and same(g_c, want["g_c"]), (what, layout)
        if (B, H, W) in ((1, 3, 11), (1, 3, 43)):               # the other pre-op, no bias, and each optional output left out
            w0 = conv64(x, w, None, None, g)
            assert same(ops.conv3x3z_train_forward(xd, wd), w0["y"]), what
            gx0, gw0, gb0, gc0 = ops.conv3x3z_train_backward(gd, xd, wd)
            assert gb0 is None and gc0 is None and same(gx0, w0["g_x"]) and same(gw0, w0["g_w"]), what
            assert torch.equal(gx0, g_x)                                        # the data gradient does not see c
            only_x = ops.conv3x3z_train_backward(gd, xd, wd, c, need_w=False)
            only_w = ops.conv3x3z_train_backward(gd, xd, wd, c, need_x=False)
            only_b = ops.conv3x3z_train_backward(gd, xd, wd, c, need_x=False, need_w=False, need_bias=True)
            assert only_x[1] is None and only_x[2] is None and torch.equal(only_x[0], g_x) and torch.equal(only_x[3], g_c)
            assert only_w[0] is None and only_w[2] is None and torch.equal(only_w[1], g_w) and torch.equal(only_w[3], g_c)
            assert only_b[0] is None and only_b[1] is None and torch.equal(only_b[2], g_bias) and torch.equal(only_b[3], g_c)


def test_null_outputs(amd):
    """Each of g_x, g_w, g_b (= g_c), g_bias NULL in turn at the C ABI: the others are the bits of the full call, at two shapes."""
    L, ops = amd._lib, amd.ops
    lib = L.lib()
    c = P(0.5)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    for i, (B, H, W, ci, co) in enumerate([(1, 3, 11, 3, 16), (1, 3, 43, 16, 3)]):
        x, g = rnd((B, H, W, ci), i, 2.0).cuda(), rnd((B, H, W, co), i + 10).cuda()
        wd = dev_w(rnd((co, ci, 3, 3), i + 20, (9 * ci) ** -0.5), i % 2)
        g_x, g_w, g_bias, g_c = ops.conv3x3z_train_backward(g, x, wd, c, need_bias=True)
        full = [g_x, g_w, g_c, g_bias]
        ws = torch.empty(lib.vqae_conv3x3z_train_workspace_bytes(B, H, W, ci, co), dtype=torch.uint8, device="cuda")
        for skip in range(4):
            outs = [torch.full_like(t, float("nan")) for t in full]
            a = [None if k == skip else outs[k] for k in range(4)]
            L.check(lib.vqae_conv3x3z_train_backward_f32(p(g), p(x), None, p(c), 1, p(wd), i % 2, B, H, W, ci, co, p(a[0]), p(a[1]),
                                                         None, p(a[2]), p(a[3]), p(ws), ops._stream()))
            torch.cuda.synchronize()
            for k in range(4):
                if k != skip:
                    assert torch.equal(outs[k], full[k]), (B, H, W, ci, co, skip, k)


# ---- no stray writes -------------------------------------------------------------------------------------------------------------
def test_no_write_outside_the_outputs(amd):
    """y, g_x, g_w and g_bias as 16-byte-aligned interior slices of sentinel-filled buffers: the sentinel stays on both sides, and
    every element of g_x (pre-filled with NaN) is written."""
    L, ops = amd._lib, amd.ops
    lib = L.lib()
    PAD, SENT = 68, -12345.0                                                     # 68 floats = 17 x 16 bytes
    c = P(0.5)
    for i, (B, H, W, ci, co) in enumerate([(1, 1, 1, 3, 8), (1, 3, 43, 16, 3), three_runs(amd) + (3, 16)]):
        x, g = rnd((B, H, W, ci), i, 2.0).cuda(), rnd((B, H, W, co), i + 10).cuda()
        w, bias = rnd((co, ci, 3, 3), i + 20, (9 * ci) ** -0.5), rnd((co,), i + 30).cuda()
        nb = -(-co // 4) * 4                                                     # the buffer keeps the far sentinel aligned
        for layout in (0, 1):
            wd = dev_w(w, layout)
            bufs = {k: torch.full((n + 2 * PAD,), SENT, device="cuda") for k, n in
                    (("y", g.numel()), ("g_x", x.numel()), ("g_w", w.numel()), ("g_bias", nb))}
            inner = {k: v[PAD:-PAD] for k, v in bufs.items()}
            inner["g_bias"] = inner["g_bias"][:co]
            assert all(t.data_ptr() % 16 == 0 for t in inner.values())
            inner["g_x"].fill_(float("nan"))
            g_c = torch.empty(1, device="cuda")
            ws = torch.empty(lib.vqae_conv3x3z_train_workspace_bytes(B, H, W, ci, co), dtype=torch.uint8, device="cuda")
            p = lambda t: ctypes.c_void_p(t.data_ptr())
            L.check(lib.vqae_conv3x3z_train_forward_f32(p(x), None, p(c), 1, p(wd), p(bias), layout, B, H, W, ci, co, p(inner["y"]),
                                                        None, ops._stream()))
            L.check(lib.vqae_conv3x3z_train_backward_f32(p(g), p(x), None, p(c), 1, p(wd), layout, B, H, W, ci, co, p(inner["g_x"]),
                                                         p(inner["g_w"]), None, p(g_c), p(inner["g_bias"]), p(ws), ops._stream()))
            torch.cuda.synchronize()
            what = (B, H, W, ci, co, layout)
            for k, v in bufs.items():
                n = inner[k].numel()
                assert bool((v[:PAD] == SENT).all()) and bool((v[PAD + n:] == SENT).all()), (k,) + what
                assert bool(torch.isfinite(v[PAD:PAD + n]).all()), (k,) + what
            want = ops.conv3x3z_train_backward(g, x, wd, c, need_bias=True)
            assert torch.equal(inner["y"].reshape(B, H, W, co), ops.conv3x3z_train_forward(x, wd, bias, c)), what
            assert torch.equal(inner["g_x"].reshape(x.shape), want[0]), what
            assert torch.equal(inner["g_w"], want[1].as_strided((w.numel(),), (1,))), what
            assert torch.equal(inner["g_bias"], want[2]) and torch.equal(g_c, want[3]), what


# ---- run to run ------------------------------------------------------------------------------------------------------------------
def test_runs_are_bit_identical(amd):
    ops = amd.ops
    cases = [(1, 3, 43, 3, 32), (1, 1, 129, 256, 3), three_runs(amd) + (16, 3), (2, 16, 32, 3, 64), BIG + (8, 3)]
    for i, (B, H, W, ci, co) in enumerate(cases):
        x, g = rnd((B, H, W, ci), i, 2.0).cuda(), rnd((B, H, W, co), i + 10).cuda()
        w, bias = dev_w(rnd((co, ci, 3, 3), i + 20, (9 * ci) ** -0.5), i % 2), rnd((co,), i + 30).cuda()
        c = P(0.5)
        run = lambda: [ops.conv3x3z_train_forward(x, w, bias, c)] + list(ops.conv3x3z_train_backward(g, x, w, c, need_bias=True))
        for p, q in zip(run(), run()):
            assert torch.equal(p, q), (B, H, W, ci, co)


# ---- element-wise bounds against the fp64 restatement ------------------------------------------------------------------------------
def test_elementwise_bounds(amd):
    ops = amd.ops
    R = ops.conv3x3z_train_wgrad_run()
    pick = [(1, 1, 1), (1, 2, 2), (2, 3, 3), (1, 3, 11), (1, 3, 43), (1, 1, 257), three_runs(amd), TALL, BIG]
    todo = [s + p + (1,) for p in PAIRS for s in shapes_of(amd, p) if s in pick]
    todo += [(1, 3, 43) + p + (0,) for p in PAIRS[::2]]
    worst = {"y": 0.0, "g_x": 0.0, "g_w": 0.0, "g_bias": 0.0, "g_c": 0.0}
    for i, (B, H, W, ci, co, pre) in enumerate(todo):
        m = B * H * W
        x, g = rnd((B, H, W, ci), i, 2.0), rnd((B, H, W, co), i + 1000)
        w, bias = rnd((co, ci, 3, 3), i + 2000, (9 * ci) ** -0.5), rnd((co,), i + 3000)
        c = P(0.5 - 0.01 * (i % 7)) if pre else None
        c64 = c.cpu() if pre else None
        want = conv64(x, w, bias, c64, g)
        x64, g64, w64, b64 = x.double(), g.double(), w.double(), bias.double()
        op = x64 + c64.double() if pre else x64
        D = U * op.abs() if pre else torch.zeros_like(x64)
        gabs, wabs = g64.abs(), w64.abs()
        what = (B, H, W, ci, co, pre)
        xd, gd, wd, bd = x.cuda(), g.cuda(), dev_w(w, i % 2), bias.cuda()
        y = ops.conv3x3z_train_forward(xd, wd, bd, c)
        by = nhwc(F.conv2d(nchw(D), wabs, padding=1)) + (9 * ci + 2) * U * nhwc(F.conv2d(nchw(op.abs() + D), wabs, b64.abs(), padding=1))
        worst["y"] = max(worst["y"], within(y, want["y"], by, ("y",) + what))
        g_x, g_w, g_bias, g_c = ops.conv3x3z_train_backward(gd, xd, wd, c, need_bias=True)
        G = (9 * co + 1) * U * taps_x(gabs, wabs)
        worst["g_x"] = max(worst["g_x"], within(g_x, want["g_x"], G, ("g_x",) + what))
        if pre:
            bc = G.sum() + U * want["g_x"].sum().abs() + TINY * want["g_x"].abs().sum()
            worst["g_c"] = max(worst["g_c"], within(g_c, want["g_c"], bc, ("g_c",) + what))
        n = min(m, R) + 1
        bw = taps_w(D, gabs) + n * U * taps_w(op.abs() + D, gabs) + U * want["g_w"].abs() + TINY * taps_w(op.abs(), gabs)
        worst["g_w"] = max(worst["g_w"], within(g_w, want["g_w"], bw, ("g_w",) + what))
        sg = gabs.sum((0, 1, 2))
        bb = n * U * sg + U * want["g_bias"].abs() + TINY * sg
        worst["g_bias"] = max(worst["g_bias"], within(g_bias, want["g_bias"], bb, ("g_bias",) + what))
    record_parity("conv3x3z_train_bounds", wgrad_run=R, cases=len(todo),
                  **{f"worst_fraction_of_bound_{k}": v for k, v in worst.items()})


# ---- the op against torch's own conv and autograd ---------------------------------------------------------------------------------
def test_op_parity(amd):
    ops = amd.ops
    names = ("y", "g_x", "g_w", "g_bias")
    rel = {"hip": [], "cpu": [], "gpu": []}
    fails = []
    cases = [(1, 1, 257, 3, 32), three_runs(amd) + (64, 3), (2, 16, 32, 3, 64), (1, 3, 43, 256, 3), (4, 32, 32, 16, 3),
             (4, 32, 32, 3, 16), (2, 64, 64, 8, 3), (2, 64, 64, 3, 8)]
    for i, (B, H, W, ci, co) in enumerate(cases):
        x, g = rnd((B, H, W, ci), i + 50, 2.0), rnd((B, H, W, co), i + 60)
        w, bias, c = rnd((co, ci, 3, 3), i + 70, (9 * ci) ** -0.5), rnd((co,), i + 80), torch.tensor([0.21])
        v64 = conv64(x, w, bias, c, g)
        cpu = conv64(x, w, bias, c, g, "cpu", torch.float32)
        gpu = conv64(x, w, bias, c, g, "cuda", torch.float32)
        cd, wd = c.cuda(), dev_w(w, i % 2)
        hip = {"y": ops.conv3x3z_train_forward(x.cuda(), wd, bias.cuda(), cd)}
        hip["g_x"], hip["g_w"], hip["g_bias"], hip["g_c"] = ops.conv3x3z_train_backward(g.cuda(), x.cuda(), wd, cd, need_bias=True)
        shape = (B, H, W, ci, co)
        for name in names:
            e_dev, e_cpu, e_gpu = (C.dist(t[name], v64[name]) for t in (hip, cpu, gpu))
            print(f"conv3x3z_train_op {shape} {name}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
            record_parity("conv3x3z_train_op", shape=list(shape), w_layout=i % 2, tensor=name, e_dev=e_dev, e_ref_cpu32=e_cpu,
                          e_ref_stock_gpu=e_gpu)
            if not e_dev <= BAR * max(e_cpu, e_gpu):
                fails.append((shape, name, e_dev, e_cpu, e_gpu))
        for tag, t in (("hip", hip), ("cpu", cpu), ("gpu", gpu)):
            rel[tag].append(float(t["g_c"].double().cpu().reshape(())) / float(v64["g_c"]))
    one = torch.ones(len(rel["hip"]), dtype=torch.float64)
    e_dev, e_cpu, e_gpu = (C.dist(torch.tensor(rel[t], dtype=torch.float64), one) for t in ("hip", "cpu", "gpu"))
    print(f"conv3x3z_train_op scalars: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
    record_parity("conv3x3z_train_op", tensor="scalars", e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
    if not e_dev <= BAR * max(e_cpu, e_gpu):
        fails.append(("scalars", e_dev, e_cpu, e_gpu))
    assert not fails, fails


# ---- the block and the whole model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("routes", [("torch", "torch", "torch", "hip"), ("hip", "hip", "hip", "hip")], ids=["conv3x3z", "all"])
def test_block_parity_hip_route(amd, routes):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    case = "outskip_8_3_4x4"
    cls = functools.partial(PreActFixupResBlock, conv1x1=routes[0], conv_down=routes[1], conv3x3=routes[2], conv3x3z=routes[3])
    block, x, g, ref = C.block_case(case, cls, device="cuda")
    assert (block.conv1x1, block.conv_down, block.conv3x3, block.conv3x3z) == routes
    T.stats.update({k: 0 for k in STATS})
    got = C.block_results(block, x.contiguous(memory_format=torch.channels_last), g, lambda b, t: b(t))
    counts = tuple(T.stats[k] for k in STATS)
    stock = C.block_results(block, x, g, T.block_forward_torch)
    torch.cuda.synchronize()
    # branch_conv3 8 -> 3 stays a counted conv1x1 fall-back
    assert counts == ((1, 0, 1, 0, 1, 1, 0, 0) if routes[0] == "hip" else (1, 0, 0, 0, 0, 0, 0, 0)), counts
    assert set(got) == set(ref)
    fails = []
    for k, (v64, e_cpu) in ref.items():
        e_dev, e_gpu = C.dist(got[k], v64.reshape(got[k].shape)), C.dist(stock[k], v64.reshape(stock[k].shape))
        print(f"conv3x3z_train_block {case} {routes} {k}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
        record_parity("conv3x3z_train_block", case=case, conv1x1=routes[0], conv_down=routes[1], conv3x3=routes[2],
                      conv3x3z=routes[3], tensor=k, e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
        assert bool(torch.isfinite(got[k]).all())
        if not e_dev <= BAR * max(e_cpu, e_gpu):
            fails.append((k, e_dev, e_cpu, e_gpu))
    assert not fails, fails


def test_closed_loop_hip_routes(amd):
    """The fixture's three steps with forward_train under all four keywords "hip" + FusedAdamW on spec tiny: the recorded codes
    exactly; losses, all parameters and the quantiser's buffers (one vector each) within 4 x e_ref, as
    test_whole_model_closed_loop."""
    from test_fixup_train_gpu import _run_loop, _stock_forward
    T = amd.train
    z = C.fixture()
    T.stats.update({k: 0 for k in STATS})
    fused = lambda m, x: T.forward_train(m, x, return_indices=True, **ALL4)
    model, sd0, losses, idxs = _run_loop(amd, fused, amd.FusedAdamW, True)
    assert T.stats["conv3x3z_hip"] == 3 * 2 and T.stats["conv3x3z_fallbacks"] == 0               # both stems, three steps
    assert T.stats["conv3x3_hip"] > 0 and T.stats["conv3x3_fallbacks"] == 0
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
        print(f"conv3x3z_train_loop {tag}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
        record_parity("conv3x3z_train_loop", tensor=tag, e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
        if not e_dev <= BAR * max(e_cpu, e_gpu):
            fails.append((tag, e_dev, e_cpu, e_gpu))
    assert not fails, fails


def _train_model(amd, name):
    """A vqae_amd.model.VQAE mirror of spec `name` in train mode with the oracle's seeded parameters (no zero-initialised
    branch: every parameter has a gradient) and a calibrated codebook, on the GPU."""
    from oracle import vqae_oracle as O
    from vqae_amd.model import VQAE
    spec = O.SPECS[name]
    p = O.calibrate_codebook(O.make_patches(2, 32, 99), O.make_params(spec, 7), spec)
    model = VQAE.from_spec(amd.SPECS[name])
    model.load_state_dict(p, strict=False)
    vq = model.encoder.vq_layers[0]
    with torch.no_grad():
        vq.embed_avg.copy_(vq.embed)
        vq.cluster_size.fill_(1.0)
        vq.first_pass.fill_(0)
    return model.cuda().train(), O.make_patches(2, 32, 3).cuda().contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("name", ["tiny", "tinyP"])
def test_whole_step_is_bit_identical(amd, name):
    """The point of the fourth node: with all four keywords "hip" no conv of a step is MIOpen's, and two runs of step + backward
    on two deep copies of a model give the same bits in every .grad."""
    T = amd.train
    model, x = _train_model(amd, name)
    grads, outs = [], []
    T.stats.update({k: 0 for k in STATS})
    for m in (copy.deepcopy(model), copy.deepcopy(model)):
        out, recon, (vq_loss,) = T.step(m, x, **ALL4)
        (recon + vq_loss).backward()
        torch.cuda.synchronize()
        outs.append((out.detach(), recon.detach(), vq_loss.detach()))
        grads.append({k: p.grad for k, p in m.named_parameters()})
    assert T.stats["conv3x3z_hip"] == 4 and all(T.stats[k] == 0 for k in STATS if k.endswith("fallbacks")), dict(T.stats)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert all(v is not None for v in grads[0].values())
    differ = [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]
    assert not differ, differ
    for k in ("encoder.in_stem.weight", "encoder.in_stem.bias", "decoder.out_stem.weight", "decoder.out_stem.bias"):
        assert float(grads[0][k].abs().max()) > 0, k
