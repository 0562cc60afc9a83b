"""GPU: the trainable 1x1 conv kernels (csrc/conv_train.hip) behind vqae_amd.ops.conv1x1_train_* and train.conv1x1.

Shapes: M in {1, 2, 31, 32, 33, 127, 128, 129, 257, 2 R + 5, 2^17 + 3} (R = vqae_conv1x1_train_wgrad_run(); around the 32-row
MFMA tile, the 64-row weight-gradient step, the 128-row workgroup tile, more than one fp32 run, more than one run per
workgroup) x (Ci, Co) in {(8,8), (8,16), (16,8), (24,40), (32,32), (64,128), (128,128), (256,256)} (every tile count of the
templates, K and N tails); the two large M with (8,8) and (16,8) only, (256,256) with M <= 129 only.

Exact: small-integer data with a = 0.5, b = -0.5, so u = ELU(x + a) + b = x and ELU' = 1 without rounding; every partial sum
of every output is an integer below 2^24 (checked from the data), so y, g_x, g_w, g_a, g_b are the int64 results whatever
the order of summation: a row or column counted twice or not at all at any tile edge shows.

Run to run: two calls give the same bits.

Element-wise bounds against the fp64 evaluation of the CPU restatement, from the arithmetic alone (u = 2^-24; expm1f / expf
taken as <= 4 ulp = 8 u relative, as in test_fixup_train_gpu.py; a sum of K fp32 products accumulated in fp32 in any order
is within (K + 1) u sum|terms|; nothing measured).  v = x + a, e = ELU(v), op = e + b the operand, d = ELU'(v):
    operand   D = u (|v| + 8 |e| + |op|)                     test_fixup_train_gpu.py's activation forward (0 for pre = 0, u |op| for pre = 1)
    y         sum_ci D |w| + (Ci + 1) u sum_ci (|op| + D) |w|
    g_u       G = (Co + 1) u sum_co |g| |w|
    g_x       G d (1 + 2^-20) + u |g_u| d (|v| + 10)          that file's activation backward: rounding of v through exp, expf, the product
    g_a, g_b  the sum of the element bounds + u |sum| + 2^-40 sum |terms|      (fp64 sums of fp32 values, rounded once)
    g_w       sum_m |g| D + (min(M, R) + 1) u sum_m |g| (|op| + D) + u |g_w| + 2^-40 sum_m |g| |op|
              (each fp32 run has at most R rows; the runs are added in fp64 and rounded once)

Op parity: e_dev = ||hip - v64|| / ||v64|| per output <= 4 x e_ref, e_ref the larger of CPU fp32 autograd of
F.conv2d(F.elu(x + a) + b, w) and the same on the GPU with stock torch ops.  The two one-element outputs of all parity shapes
form ONE vector of relative values, for the reason tests/fixup_train_cases.py gives.  Blocks and the closed loop: the bar and
the e_ref construction of test_fixup_train_gpu.py, under conv1x1="hip".
"""
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
PAIRS = [(8, 8), (8, 16), (16, 8), (24, 40), (32, 32), (64, 128), (128, 128), (256, 256)]
SMALL_M = [1, 2, 31, 32, 33, 127, 128, 129, 257]


def shapes(amd):
    r = amd.ops.conv1x1_train_wgrad_run()
    out = [(m, ci, co) for m in SMALL_M for (ci, co) in PAIRS if not ((ci, co) == (256, 256) and m > 129)]
    return out + [(m, ci, co) for m in (2 * r + 5, 2 ** 17 + 3) for (ci, co) in ((8, 8), (16, 8))]


def P(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


def ints(shape, seed, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed))


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


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
    for i, (m, ci, co) in enumerate(shapes(amd)):
        x, g, w = ints((m, ci), 3 * i, 1, 4), ints((m, co), 3 * i + 1, -3, 3), ints((co, ci), 3 * i + 2, -2, 2)
        y64, gu64, gw64 = x @ w.t(), g @ w, g.t() @ x
        # every partial sum of every output is an integer below 2^24 in any order: the sums of absolute values are
        assert int((x.abs() @ w.abs().t()).max()) < lim and int((g.abs() @ w.abs()).max()) < lim
        assert int((g.abs().t() @ x.abs()).max()) < lim and int(gu64.abs().sum()) < 2 ** 53 and abs(int(gu64.sum())) < lim
        xd, gd, wd = x.float().cuda(), g.float().cuda(), w.float().reshape(co, ci, 1, 1).cuda()
        y = ops.conv1x1_train_forward(xd, wd, a, b)
        g_x, g_w, g_a, g_b = ops.conv1x1_train_backward(gd, xd, wd, a, b)
        what = (m, ci, co)
        assert torch.equal(y.cpu().to(torch.int64), y64) and torch.equal(y.cpu(), y64.float()), what
        assert torch.equal(g_x.cpu(), gu64.float()), what
        assert g_w.shape == wd.shape and torch.equal(g_w.cpu().reshape(co, ci), gw64.float()), what
        assert float(g_a) == float(gu64.sum()) == float(g_b), what
        if m in (33, 129):                                  # the other two pre-ops and the optional outputs
            y0 = ops.conv1x1_train_forward(xd, wd)
            y1 = ops.conv1x1_train_forward(xd, wd, None, b)                   # u = x - 0.5: multiples of 0.5, still exact
            assert torch.equal(y0.cpu(), y64.float()) and torch.equal(y1.cpu().double(), (x.double() - 0.5) @ w.double().t()), what
            gx0, gw0, ga0, gb0 = ops.conv1x1_train_backward(gd, xd, wd)
            assert ga0 is None and gb0 is None and torch.equal(gx0, g_x) and torch.equal(gw0, g_w), what
            gx1, gw1, ga1, gb1 = ops.conv1x1_train_backward(gd, xd, wd, None, b)
            assert ga1 is None and torch.equal(gb1, g_b) and torch.equal(gx1, g_x), what
            assert torch.equal(gw1.cpu().reshape(co, ci).double(), g.double().t() @ (x.double() - 0.5)), what
            only_x = ops.conv1x1_train_backward(gd, xd, wd, a, b, need_w=False)
            only_w = ops.conv1x1_train_backward(gd, xd, wd, a, b, need_x=False)
            assert only_x[1] is None and torch.equal(only_x[0], g_x) and torch.equal(only_x[2], g_a)
            assert only_w[0] is None and torch.equal(only_w[1], g_w) and torch.equal(only_w[3], g_b)


def test_runs_are_bit_identical(amd):
    ops = amd.ops
    r = ops.conv1x1_train_wgrad_run()
    for i, (m, ci, co) in enumerate([(129, 24, 40), (257, 64, 128), (2 * r + 5, 16, 8), (1024, 128, 128), (2 ** 17 + 3, 8, 8)]):
        x, g, w = rnd((m, ci), i, 2.0).cuda(), rnd((m, co), i + 10).cuda(), rnd((co, ci, 1, 1), i + 20, ci ** -0.5).cuda()
        a, b = P(0.3), P(-0.2)
        run = lambda: [ops.conv1x1_train_forward(x, w, a, b)] + list(ops.conv1x1_train_backward(g, x, w, a, b))
        for p, q in zip(run(), run()):
            assert torch.equal(p, q), (m, ci, co)


# ---- element-wise bounds against the fp64 restatement ------------------------------------------------------------------------------
def test_elementwise_bounds(amd):
    T, ops = amd.train, amd.ops
    R = ops.conv1x1_train_wgrad_run()
    todo = [(m, ci, co, 2) for (m, ci, co) in shapes(amd) if m in (33, 129, 257, 2 * R + 5, 2 ** 17 + 3)]
    todo += [(129, ci, co, pre) for (ci, co) in PAIRS for pre in (0, 1)]
    worst = {"y": 0.0, "g_x": 0.0, "g_w": 0.0, "g_a": 0.0, "g_b": 0.0}
    for i, (m, ci, co, pre) in enumerate(todo):
        x, g, w = rnd((m, ci), i, 2.0), rnd((m, co), i + 1000), rnd((co, ci), i + 2000, ci ** -0.5)
        a, b = pre_args(pre, P(0.25 - 0.01 * (i % 7)), P(-0.125 + 0.02 * (i % 5)))
        x64, g64, w64 = x.double(), g.double(), w.double()
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
        what = (m, ci, co, pre)
        xd, gd, wd = x.cuda(), g.cuda(), w.reshape(co, ci, 1, 1).cuda()
        y = ops.conv1x1_train_forward(xd, wd, a, b)
        by = D @ w64.abs().t() + (ci + 1) * U * ((op.abs() + D) @ w64.abs().t())
        worst["y"] = max(worst["y"], within(y, op @ w64.t(), by, ("y",) + what))
        g_x, g_w, g_a, g_b = ops.conv1x1_train_backward(gd, xd, wd, a, b)
        gu64 = g64 @ w64
        G = (co + 1) * U * (g64.abs() @ w64.abs())
        gx64 = gu64 * d
        bx = G * d * (1 + 2.0 ** -20) + (U * gu64.abs() * d * (v.abs() + 10) if pre == 2 else 0)
        worst["g_x"] = max(worst["g_x"], within(g_x, gx64, bx, ("g_x",) + what))
        if pre == 2:
            ba = bx.sum() + U * gx64.sum().abs() + TINY * gx64.abs().sum()
            worst["g_a"] = max(worst["g_a"], within(g_a, gx64.sum(), ba, ("g_a",) + what))
        if pre >= 1:
            bb = G.sum() + U * gu64.sum().abs() + TINY * gu64.abs().sum()
            worst["g_b"] = max(worst["g_b"], within(g_b, gu64.sum(), bb, ("g_b",) + what))
        gw64 = g64.t() @ op
        gabs = g64.abs().t()
        bw = gabs @ D + (min(m, R) + 1) * U * (gabs @ (op.abs() + D)) + U * gw64.abs() + TINY * (gabs @ op.abs())
        worst["g_w"] = max(worst["g_w"], within(g_w, gw64, bw, ("g_w",) + what))
    record_parity("conv1x1_train_bounds", wgrad_run=R, cases=len(todo),
                  **{f"worst_fraction_of_bound_{k}": v for k, v in worst.items()})


# ---- the op against torch's own conv and autograd ---------------------------------------------------------------------------------
def _stock(x, w, a, b, g, device, dtype):
    x, w, a, b = (t.detach().to(device=device, dtype=dtype).requires_grad_() for t in (x, w, a, b))
    m, ci = x.shape
    y = F.conv2d(F.elu(x.t().reshape(1, ci, m, 1) + a) + b, w)                  # NCHW [1, Ci, M, 1]
    gs = torch.autograd.grad(y, [x, w, a, b], g.to(device=device, dtype=dtype).t().reshape(1, -1, m, 1))
    return [y.reshape(-1, m).t()] + list(gs)


def test_op_parity(amd):
    ops = amd.ops
    R = ops.conv1x1_train_wgrad_run()
    names = ("y", "g_x", "g_w")
    rel = {"hip": [], "cpu": [], "gpu": []}
    fails = []
    for i, (m, ci, co) in enumerate([(257, 24, 40), (2 * R + 5, 64, 128), (1024, 128, 128), (129, 256, 256), (4096, 16, 16)]):
        x, g, w = rnd((m, ci), i + 50, 2.0), rnd((m, co), i + 60), rnd((co, ci, 1, 1), i + 70, ci ** -0.5)
        a, b = torch.tensor([0.21]), torch.tensor([-0.13])
        v64 = _stock(x, w, a, b, g, "cpu", torch.float64)
        cpu = _stock(x, w, a, b, g, "cpu", torch.float32)
        gpu = _stock(x, w, a, b, g, "cuda", torch.float32)
        ad, bd = a.cuda(), b.cuda()
        y = ops.conv1x1_train_forward(x.cuda(), w.cuda(), ad, bd)
        g_x, g_w, g_a, g_b = ops.conv1x1_train_backward(g.cuda(), x.cuda(), w.cuda(), ad, bd)
        hip = [y, g_x, g_w, g_a, g_b]
        for k, name in enumerate(names):
            e_dev, e_cpu, e_gpu = (C.dist(t[k], v64[k].reshape(t[k].shape)) for t in (hip, cpu, gpu))
            print(f"conv1x1_train_op {(m, ci, co)} {name}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
            record_parity("conv1x1_train_op", shape=[m, ci, co], tensor=name, e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
            if not e_dev <= BAR * max(e_cpu, e_gpu):
                fails.append(((m, ci, co), name, e_dev, e_cpu, e_gpu))
        for k in (3, 4):
            for tag, t in (("hip", hip), ("cpu", cpu), ("gpu", gpu)):
                rel[tag].append(float(t[k].double().cpu().reshape(())) / float(v64[k]))
    one = torch.ones(len(rel["hip"]), dtype=torch.float64)
    e_dev, e_cpu, e_gpu = (C.dist(torch.tensor(rel[t], dtype=torch.float64), one) for t in ("hip", "cpu", "gpu"))
    print(f"conv1x1_train_op scalars: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
    record_parity("conv1x1_train_op", tensor="scalars", e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
    if not e_dev <= BAR * max(e_cpu, e_gpu):
        fails.append(("scalars", e_dev, e_cpu, e_gpu))
    assert not fails, fails


# ---- blocks and the whole model ----------------------------------------------------------------------------------------------------
def _expected_routes(block):
    convs = [block.branch_conv1, block.branch_conv3]
    if block.mode == "up":
        convs.append(block.branch_conv2)
    if block.skip_conv is not None and block.mode in ("up", "same"):
        convs.append(block.skip_conv)
    ok = [c.in_channels % 8 == 0 and c.out_channels % 8 == 0 and 8 <= c.in_channels <= 256 and 8 <= c.out_channels <= 256
          for c in convs]
    return sum(ok), len(ok) - sum(ok)


@pytest.mark.parametrize("case", C.block_cases())
def test_block_parity_hip_route(amd, case):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    block, x, g, ref = C.block_case(case, functools.partial(PreActFixupResBlock, conv1x1="hip"), device="cuda")
    assert block.conv1x1 == "hip"
    T.stats.update(conv1x1_hip=0, conv1x1_fallbacks=0)
    got = C.block_results(block, x.contiguous(memory_format=torch.channels_last), g, lambda b, t: b(t))
    routed, fell = T.stats["conv1x1_hip"], T.stats["conv1x1_fallbacks"]
    stock = C.block_results(block, x, g, T.block_forward_torch)
    torch.cuda.synchronize()
    want_hip, want_fall = _expected_routes(block)
    assert (routed, fell) == (want_hip, want_fall) and routed >= 1, (case, routed, fell, want_hip, want_fall)
    if case == "outskip_8_3_4x4":
        assert fell == 1                                   # branch_conv3, 8 -> 3 (its 3x3 skip conv is no 1x1 candidate)
    assert set(got) == set(ref)
    fails = []
    for k, (v64, e_cpu) in ref.items():
        e_dev, e_gpu = C.dist(got[k], v64.reshape(got[k].shape)), C.dist(stock[k], v64.reshape(stock[k].shape))
        print(f"conv1x1_train_block {case} {k}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
        record_parity("conv1x1_train_block", case=case, tensor=k, e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
        assert bool(torch.isfinite(got[k]).all())
        if not e_dev <= BAR * max(e_cpu, e_gpu):
            fails.append((k, e_dev, e_cpu, e_gpu))
    assert not fails, fails


def test_closed_loop_hip_route(amd):
    """The fixture's three steps with forward_train(conv1x1="hip") + FusedAdamW: the recorded codes exactly; losses, all
    parameters and the quantiser's buffers (one vector each) within 4 x e_ref, as test_whole_model_closed_loop."""
    from test_fixup_train_gpu import _run_loop, _stock_forward
    T = amd.train
    z = C.fixture()
    T.stats.update(conv1x1_hip=0, conv1x1_fallbacks=0)
    fused = lambda m, x: T.forward_train(m, x, return_indices=True, conv1x1="hip")
    model, sd0, losses, idxs = _run_loop(amd, fused, amd.FusedAdamW, True)
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
        print(f"conv1x1_train_loop {tag}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
        record_parity("conv1x1_train_loop", tensor=tag, e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
        if not e_dev <= BAR * max(e_cpu, e_gpu):
            fails.append((tag, e_dev, e_cpu, e_gpu))
    assert not fails, fails


def test_weight_gradients_repeat_through_autograd(amd):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    torch.manual_seed(3)
    block = PreActFixupResBlock(32, 32, "same", n_layers=4, conv1x1="hip").cuda()
    with torch.no_grad():
        torch.nn.init.normal_(block.branch_conv3.weight, std=0.1)
    x = rnd((3, 32, 17, 19), 9).cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    g = rnd((3, 32, 17, 19), 10).cuda().contiguous(memory_format=torch.channels_last)
    grads = []
    for _ in range(2):
        block.zero_grad(set_to_none=True)
        x.grad = None
        block(x).backward(g)
        grads.append({k: p.grad.clone() for k, p in block.named_parameters()})
    for k in ("branch_conv1.weight", "branch_conv3.weight", "bias3a", "bias3b"):
        assert torch.equal(grads[0][k], grads[1][k]), k
    assert float(grads[0]["branch_conv1.weight"].abs().max()) > 0
