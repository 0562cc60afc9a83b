"""GPU: the fused training ops of a Fixup block (csrc/fixup_train.hip behind vqae_amd.train's autograd Functions).

Exact, no tolerance: the halo is F.pad(circular) of the interior; g_t is torch's g * scale; the skip / plain-mode input
gradient is the incoming tensor; with small-integer data every scalar gradient is the integer sum (every element counted
once, for element counts around the 4-wide groups and the 256-thread workgroups, 2^20 + 3, and C in {1, 3, 4, 8, 20}); two
runs of every op give the same bits.

Element-wise bounds against the fp64 evaluation of the CPU restatement on the same inputs, from the kernels' arithmetic
alone (u = 2^-24; expm1f / expf taken as <= 4 ulp = 8 u relative; nothing measured).  v = x + a, e = ELU(v), d = ELU'(v):
    act forward      u (|v| + 8 |e| + |y|)           rounding of v through a slope <= 1, expm1f, the add of b
    act backward     u F d (|v| + 10 + 8 h)          F = sum of |g| over the pixel's images (h = 1 with a halo: up to 8
                                                     fp32 adds of the fold); rounding of v through exp (relative |v| u),
                                                     expf, the product
    g_a, g_b         sum of the element bounds of g_x (of the fold: 8 h u F) + u |sum| + 2^-40 sum |terms|   (fp64 sums of
                                                     fp32 values, rounded once)
    out forward      4 u (|t s| + |b4| + |skip| + |b1d|)     four roundings of partial sums
    g_scale, g_bias  u |sum| + 2^-40 sum |terms|     exact products summed in fp64, rounded once
    bicubic forward  10 u A,  A = |up|(|x + pb|)     rounding of x + pb, 2 x (product + 3 adds) (+1 spare)
    bicubic backward 17 u A', A' = |up|^T(|g|)       2 x (product + 7 adds) (+1 spare); the weights are exact
    g_pre_bias       sum of 17 u A' + u |sum| + 2^-40 sum |g_x|

Block and whole-model bar: e_dev = ||hip - g64|| / ||g64|| <= 4 x e_ref per tensor (one-element tensors as one vector,
tests/fixup_train_cases.py), e_ref the larger of the fixture's fp32 CPU distance and the distance of the same block written
with stock torch ops (train.block_forward_torch: F.elu, F.pad, F.interpolate, the same F.conv2d) on the same GPU, so that
MIOpen's own summation order is not charged to the new kernels.  Run-to-run identity is claimed for the new ops only.
"""
import pytest
import torch
import torch.nn.functional as F

import fixup_train_cases as C
from conftest import record_parity

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -40
BAR = 4.0
HW = [(1, 1), (1, 2), (2, 1), (2, 3), (3, 3), (4, 5), (7, 9)]
CS = [1, 3, 4, 8, 20]
SHAPES = [(b, h, w, c) for (h, w) in HW for c in CS for b in (1, 2)]
COUNTS = [1, 3, 4, 5, 255, 256, 257, 2 ** 20 + 3]
INT_SHAPES = [(1, 1, n, 1) for n in COUNTS] + [(2, 5, 7, c) for c in CS]


def P(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def ints(shape, seed, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def d64(*ts):
    return [t.detach().double().cpu() if t is not None else None for t in ts]


def within(got, want64, bound64, what):
    got, want64, bound64 = got.detach().double().cpu().reshape(-1), want64.reshape(-1), bound64.reshape(-1)
    assert got.shape == want64.shape, what
    over = (got - want64).abs() - bound64
    assert bool((over <= 0).all()), (what, float(over.max()), float(bound64.max()))
    return float(((got - want64).abs() / bound64.clamp_min(1e-300)).max())


# ---- exact properties -------------------------------------------------------------------------------------------------------
def test_halo_is_circular_pad(amd):
    T = amd.train
    for i, shape in enumerate(SHAPES):
        x, a, b = rnd(shape, i, 2.0).cuda(), P(0.25), P(-0.125)
        y, inner = T.fixup_act(x, a, b, halo=1), T.fixup_act(x, a, b)
        want = F.pad(inner.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="circular").permute(0, 2, 3, 1)
        assert y.shape == (shape[0], shape[1] + 2, shape[2] + 2, shape[3]) and torch.equal(y, want), shape


def test_identity_gradients_and_g_t(amd):
    T, ops = amd.train, amd.ops
    for i, shape in enumerate(SHAPES[::3] + [(1, 1, 2 ** 20 + 3, 1)]):
        t, skip, g = (rnd(shape, 10 * i + k).cuda() for k in range(3))
        scale = P(0.8125 + i / 64)
        g_t, g_scale, g_bias = ops.fixup_out_backward(g, t, scale)
        assert torch.equal(g_t, g * scale), shape
        tt, ss = t.clone().requires_grad_(), skip.clone().requires_grad_()
        y = T.fixup_out(tt, ss, scale, P(0.1), P(0.2))
        gt, gs = torch.autograd.grad(y, [tt, ss], g)
        assert torch.equal(gs, g) and torch.equal(gt, g * scale), shape
        gx, _, _ = ops.fixup_act_backward(g, None, None, act=False)
        assert gx is g
        xx = t.clone().requires_grad_()
        (gp,) = torch.autograd.grad(T.fixup_add(xx, P(0.3)), [xx], g)
        assert torch.equal(gp, g), shape


@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_sums_are_exact(amd, shape):
    """Small-integer g and t: every scalar gradient is the integer sum, so every element is counted exactly once."""
    ops = amd.ops
    g, t = ints(shape, 1, -3, 3), ints(shape, 2, -4, 4)
    gd, td = g.cuda(), t.cuda()
    _, g_scale, g_bias = ops.fixup_out_backward(gd, td, P(1.5))
    assert float(g_scale) == float((g.double() * t.double()).sum()) and float(g_bias) == float(g.double().sum())
    _, _, g_c = ops.fixup_act_backward(gd, None, None, act=False)
    assert float(g_c) == float(g.double().sum())
    x = ints(shape, 3, 1, 4).cuda()                       # x + a > 0 everywhere: ELU' = 1 and g_a = g_b = sum g
    g_x, g_a, g_b = ops.fixup_act_backward(gd, x, P(0.5))
    assert torch.equal(g_x, gd) and float(g_a) == float(g.double().sum()) == float(g_b)
    B, H, W, Cc = shape
    gh = ints((B, H + 2, W + 2, Cc), 4, -3, 3)
    g_x, g_a, g_b = ops.fixup_act_backward(gh.cuda(), x, P(0.5), halo=1)
    assert torch.equal(g_x.cpu(), amd.train.fold_circular_nhwc(gh))
    assert float(g_a) == float(gh.double().sum()) == float(g_b)
    gu = ints((B, 2 * H, 2 * W, Cc), 5, -3, 3)            # the taps are multiples of 2^-8: g_x is exact, and sums to sum g
    g_x, g_pb = ops.bicubic_up2_backward(gu.cuda())
    if W <= 512:                                          # the restatement's operator is a dense [2W, W] matrix
        assert torch.equal(g_x.cpu().double(), amd.train._bicubic_up2_adjoint_torch(gu.double()))
    assert float(g_pb) == float(gu.double().sum())


def test_runs_are_bit_identical(amd):
    ops = amd.ops
    for i, shape in enumerate(SHAPES[1::4] + [(1, 3, 2 ** 18 + 1, 4), (1, 1, 2 ** 20 + 3, 1)]):
        B, H, W, Cc = shape
        x, g, t = rnd(shape, i).cuda(), rnd(shape, i + 100).cuda(), rnd(shape, i + 200).cuda()
        gh, gu = rnd((B, H + 2, W + 2, Cc), i + 300).cuda(), rnd((B, 2 * H, 2 * W, Cc), i + 400).cuda()
        a, b = P(0.3), P(-0.2)

        def run():
            out = [ops.fixup_act(x, a, b), ops.fixup_act(x, a, b, halo=1), ops.fixup_act(x, None, b)]
            out += ops.fixup_act_backward(g, x, a) + ops.fixup_act_backward(gh, x, a, halo=1)
            out += ops.fixup_act_backward(g, None, None, act=False)[2:]
            out += [ops.fixup_out(t, x, a, b, a)] + list(ops.fixup_out_backward(g, t, a))
            out += [ops.bicubic_up2_bias(x, a)] + list(ops.bicubic_up2_backward(gu))
            return out

        for p, q in zip(run(), run()):
            assert torch.equal(p, q), shape


def test_bicubic_forward_is_the_inference_kernel(amd):
    """Where both apply (C % 4 == 0) the training forward gives the bits of vqae_bicubic_up2_f32, pre_bias included."""
    for i, shape in enumerate([s for s in SHAPES if s[3] % 4 == 0]):
        x = rnd(shape, i).cuda()
        assert torch.equal(amd.ops.bicubic_up2_bias(x), amd.ops.bicubic_up2(x)), shape
        assert torch.equal(amd.ops.bicubic_up2_bias(x, P(0.37)), amd.ops.bicubic_up2(x, float(P(0.37)))), shape


# ---- element-wise bounds against the fp64 restatement -------------------------------------------------------------------------
def test_act_bounds(amd):
    T, ops = amd.train, amd.ops
    worst = 0.0
    for i, shape in enumerate(SHAPES):
        B, H, W, Cc = shape
        x, a, b = rnd(shape, i, 2.0), P(0.25 - 0.01 * (i % 7)), P(-0.125 + 0.02 * (i % 5))
        x64, a64, b64 = d64(x, a, b)
        v = x64 + a64
        e, d = F.elu(v), T.elu_grad(v)
        for halo in (0, 1):
            y = ops.fixup_act(x.cuda(), a, b, halo)
            y64 = T.fixup_act(x64, a64, b64, halo)
            bound = U * (v.abs() + 8 * e.abs() + (e + b64).abs())
            worst = max(worst, within(y, y64, T.pad_circular_nhwc(bound) if halo else bound, ("act fwd", shape, halo)))
            g = rnd(y.shape, 1000 + i)
            g64 = g.double()
            g_x, g_a, g_b = ops.fixup_act_backward(g.cuda(), x.cuda(), a, halo)
            fold, fabs = (T.fold_circular_nhwc(g64), T.fold_circular_nhwc(g64.abs())) if halo else (g64, g64.abs())
            gx64 = fold * d
            bx = U * fabs * d * (v.abs() + 10 + 8 * halo)
            worst = max(worst, within(g_x, gx64, bx, ("act bwd", shape, halo)))
            ba = bx.sum() + U * gx64.sum().abs() + TINY * gx64.abs().sum()
            bb = 8 * halo * U * fabs.sum() + U * fold.sum().abs() + TINY * fabs.sum()
            worst = max(worst, within(g_a, gx64.sum(), ba, ("g_a", shape, halo)), within(g_b, fold.sum(), bb, ("g_b", shape, halo)))
        c = ops.fixup_act(x.cuda(), None, b)
        assert torch.equal(c, x.cuda() + b)
    record_parity("fixup_train_act_bounds", worst_fraction_of_bound=worst, shapes=len(SHAPES))


def test_out_bounds(amd):
    ops = amd.ops
    worst = 0.0
    for i, shape in enumerate(SHAPES):
        t, skip, g = rnd(shape, i), rnd(shape, i + 50), rnd(shape, i + 99)
        sc, b4, b1d = P(0.8 + 0.01 * (i % 9)), P(0.07), P(-0.11)
        t64, s64, g64, sc64, b464, b1d64 = d64(t, skip, g, sc, b4, b1d)
        for bd, bd64 in ((b1d, b1d64), (None, None)):
            y = ops.fixup_out(t.cuda(), skip.cuda(), sc, b4, bd)
            y64 = (t64 * sc64 + b464) + (s64 if bd is None else s64 + bd64)
            m = (t64 * sc64).abs() + b464.abs() + s64.abs() + (0 if bd is None else bd64.abs())
            worst = max(worst, within(y, y64, 4 * U * m, ("out fwd", shape)))
        _, g_scale, g_bias = ops.fixup_out_backward(g.cuda(), t.cuda(), sc)
        gs, gb = (g64 * t64).sum(), g64.sum()
        worst = max(worst, within(g_scale, gs, U * gs.abs() + TINY * (g64 * t64).abs().sum(), ("g_scale", shape)),
                    within(g_bias, gb, U * gb.abs() + TINY * g64.abs().sum(), ("g_bias", shape)))
    record_parity("fixup_train_out_bounds", worst_fraction_of_bound=worst, shapes=len(SHAPES))


def test_bicubic_bounds_and_adjoint(amd):
    """Forward and backward against the fp64 restatement, the backward also against fp64 CPU autograd of F.interpolate, and
    the inner-product identity <up(x), g> = <x, up^T(g)> on the device results in fp64."""
    T, ops = amd.train, amd.ops
    worst = 0.0
    for i, shape in enumerate(SHAPES):
        B, H, W, Cc = shape
        x, g, pb = rnd(shape, i), rnd((B, 2 * H, 2 * W, Cc), i + 77), P(0.3)
        x64, g64, pb64 = d64(x, g, pb)
        ah, aw = T.up2_matrix(H).abs(), T.up2_matrix(W).abs()
        up_abs = lambda v: torch.einsum("oh,bhwc->bowc", ah, torch.einsum("pw,bhwc->bhpc", aw, v))
        adj_abs = lambda v: torch.einsum("pw,bhpc->bhwc", aw, torch.einsum("oh,bowc->bhwc", ah, v))
        for bias, bias64 in ((pb, pb64), (None, None)):
            y = ops.bicubic_up2_bias(x.cuda(), bias)
            v64 = x64 if bias is None else x64 + bias64
            worst = max(worst, within(y, T._bicubic_up2_torch(x64, bias64), 10 * U * up_abs(v64.abs()), ("bicubic fwd", shape)))
        g_x, g_pb = ops.bicubic_up2_backward(g.cuda())
        xr = x64.clone().requires_grad_()
        ref = F.interpolate(xr.permute(0, 3, 1, 2), scale_factor=2, mode="bicubic", align_corners=False).permute(0, 2, 3, 1)
        (gx_auto,) = torch.autograd.grad(ref, [xr], g64)
        bx = 17 * U * adj_abs(g64.abs())
        worst = max(worst, within(g_x, T._bicubic_up2_adjoint_torch(g64), bx, ("bicubic bwd", shape)))
        within(g_x, gx_auto, bx + 1e-13, ("bicubic bwd vs autograd", shape))
        gx64 = g_x.double().cpu()
        worst = max(worst, within(g_pb, gx64.sum(), U * gx64.sum().abs() + TINY * gx64.abs().sum(), ("g_pre_bias", shape)))
        within(g_pb, gx_auto.sum(), bx.sum() + U * gx_auto.sum().abs() + TINY * gx_auto.abs().sum(), ("g_pre_bias vs autograd", shape))
        y = ops.bicubic_up2_bias(x.cuda()).double().cpu()
        lhs, rhs = (y * g64).sum(), (x64 * gx64).sum()
        assert abs(float(lhs - rhs)) <= float((10 * U * up_abs(x64.abs()) * g64.abs()).sum() + (bx * x64.abs()).sum()), shape
    record_parity("fixup_train_bicubic_bounds", worst_fraction_of_bound=worst, shapes=len(SHAPES))


# ---- blocks and the whole model against the reference's autograd -----------------------------------------------------------------
@pytest.mark.parametrize("case", C.block_cases())
def test_block_parity(amd, case):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    block, x, g, ref = C.block_case(case, PreActFixupResBlock, device="cuda")
    got = C.block_results(block, x.contiguous(memory_format=torch.channels_last), g, lambda b, t: b(t))
    stock = C.block_results(block, x, g, amd.train.block_forward_torch)
    torch.cuda.synchronize()
    assert set(got) == set(ref)
    fails = []
    for k, (v64, e_cpu) in ref.items():
        e_dev, e_gpu = C.dist(got[k], v64.reshape(got[k].shape)), C.dist(stock[k], v64.reshape(stock[k].shape))
        e_ref = max(e_cpu, e_gpu)
        print(f"fixup_train_block {case} {k}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
        record_parity("fixup_train_block", case=case, tensor=k, e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
        assert bool(torch.isfinite(got[k]).all())
        if not e_dev <= BAR * e_ref:
            fails.append((k, e_dev, e_ref))
    assert not fails, fails


def _run_loop(amd, forward, make_opt, channels_last):
    z = C.fixture()
    model, batches = C.loop_model(device="cuda")
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = make_opt(model.parameters(), lr=float(z["loop/lr"]))
    losses, idxs = [], []
    for x in batches:
        if channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        out, vq_losses, (idx,) = forward(model, x)
        recon = F.huber_loss(input=out, target=x)
        opt.zero_grad()
        (recon + sum(vq_losses)).backward()
        opt.step()
        losses += [float(recon), float(vq_losses[0])]
        idxs.append(idx.cpu())
    return model, sd0, losses, idxs


def _stock_forward(amd):
    """VQAE.forward with stock torch ops on NCHW tensors (the blocks by train.block_forward_torch), the quantiser mirror as is."""
    bft = amd.train.block_forward_torch

    def forward(model, x):
        enc, dec = model.encoder, model.decoder
        h = F.conv2d(x, enc.in_stem.weight, enc.in_stem.bias, padding=1)
        for level in enc.down_layers[0].layers:
            for blk in level.layers:
                h = bft(blk, h)
        for blk in enc.pre_enc_layers[0]:
            h = bft(blk, h)
        h, idx, vq_loss = enc.vq_layers[0](h)
        for blk in dec.post_enc_layers[0]:
            h = bft(blk, h)
        for level in dec.up_layers[0].layers:
            for blk in level.layers:
                h = bft(blk, h)
        return F.conv2d(h, dec.out_stem.weight, dec.out_stem.bias, padding=1), (vq_loss,), (idx,)
    return forward


def test_whole_model_closed_loop(amd):
    """step()'s forward + vqae_amd.FusedAdamW for the fixture's three steps: the recorded codes exactly; the six losses (one
    vector), all parameters (one vector) and the quantiser's buffers (one vector) within 4 x e_ref, e_ref the larger of the
    fp32 reference run's distance and that of the stock-torch model + torch.optim.AdamW on the same GPU."""
    z = C.fixture()
    fused = lambda m, x: amd.train.forward_train(m, x, return_indices=True)
    model, sd0, losses, idxs = _run_loop(amd, fused, amd.FusedAdamW, True)
    smodel, ssd0, slosses, sidxs = _run_loop(amd, _stock_forward(amd), torch.optim.AdamW, False)
    for i in range(3):
        assert torch.equal(idxs[i].to(torch.int16), torch.from_numpy(z["loop/idx"][i])), f"step {i}: codes differ"
    stock_idx_ok = all(torch.equal(sidxs[i].to(torch.int16), torch.from_numpy(z["loop/idx"][i])) for i in range(3))
    e, e_cpu = C.loss_distances(losses)
    e_gpu = C.loss_distances(slosses)[0] if stock_idx_ok else 0.0
    rows = [("losses", e, e_cpu, e_gpu)]
    mine, stock = C.loop_final_groups(model, sd0), C.loop_final_groups(smodel, ssd0)
    for tag, (got, want, e32) in mine.items():
        rows.append((tag, C.dist(got, want), e32, C.dist(stock[tag][0], want) if stock_idx_ok else 0.0))
    fails = []
    for tag, e_dev, e_cpu, e_gpu in rows:
        print(f"fixup_train_loop {tag}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
        record_parity("fixup_train_loop", tensor=tag, e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
        if not e_dev <= BAR * max(e_cpu, e_gpu):
            fails.append((tag, e_dev, e_cpu, e_gpu))
    assert not fails, fails
