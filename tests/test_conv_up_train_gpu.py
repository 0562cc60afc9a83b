"""GPU: the 'up' blocks in the commuted order, conv_up="hip" (csrc/up_train.hip behind vqae_amd.train.up2_act / fixup_out_up).

A workgroup of csrc/up_train.hip owns T x T low-resolution pixels x K channels (T = 8, K = 16) and loops over its tiles once there
are more than 2048 of them.  The shapes put H and W on 1, 2, 3, T - 1, T, T + 1 and 2 T + 1 (one tile, a partial one, two
tiles and a part, windows that clamp on both sides at once) and C on 1, 3 (scalar path), 4, 8, 20 = K + 4, K (16-byte path,
a partial channel chunk), B on 1 and 2.

Exact, no tolerance.  The new kernels evaluate the expressions of ft_bicubic_fwd, ft_act_fwd_flat / ft_act_bwd_flat,
ft_out_fwd / ft_out_bwd and ft_bicubic_bwd in their order, so every tensor they write equals the composition of the existing
ops bit for bit: y of both forwards, g_t_low, g_t, g_s_low.  No existing kernel had to change for that.  The same holds with
every pointer one float off a 16-byte boundary (the scalar path), every output lies inside a poisoned buffer whose guard bands
stay untouched, and two runs give the same bits.  On small-integer data every scalar gradient is the integer sum, at 1 .. 257
low-resolution pixels and at 2^20 + 3 (131073 tiles: the tile loop).

Scalar gradients against the composition.  Both sides add the SAME fp32 numbers (g_v, g, the exact products g t) in fp64 in
different orders and round once: |ours - theirs| <= 2 (u |S| + 2^-40 sum |terms|), u = 2^-24 -- one fp32 rounding and one
fp64 reordering term per side, the terms of tests/test_fixup_train_gpu.py.

Element-wise bounds against the fp64 evaluation of the CPU restatement on the same inputs, from the arithmetic alone (expm1f /
expf taken as <= 8 u relative, as in tests/test_fixup_train_gpu.py; nothing measured).  A = |up2|(|t_low|), v = up2(t_low),
w = v + a, e = ELU(w), d = ELU'(w):
    v                     10 u A                                   that file's bicubic forward bound
    up2_act forward       u (10 A + |w| + 8 |e| + |y|)             v through a slope <= 1, the add of a, expm1f, the add of b
    g_v = g d             u |g| d (10 A + |w| + 10)                v and the add of a through exp (relative), expf, the product (+1)
    g_t_low = up2^T g_v   |up2|^T(bound of g_v) + 17 u |up2|^T(|g_v|)   that file's bicubic backward bound on top
    g_a                   sum of the bounds of g_v + u |sum| + 2^-40 sum |g_v|;      g_b: u |sum| + 2^-40 sum |g|
    fixup_out_up forward  10 u A_s + 4 u (|t s| + |b4| + |up2(s_low)| + |b1d|)       four roundings of partial sums
    g_t                   u |g s|;       g_s_low: 17 u |up2|^T(|g|);       g_scale, g_bias: u |sum| + 2^-40 sum |terms|

Blocks and the closed loop: the bar and the e_ref construction of tests/test_fixup_train_gpu.py (4 x the larger of the fixture's
fp32 distance and the stock-torch block's on the same GPU), under conv_up="hip" with conv1x1 "torch" and "hip".  Whole-step
determinism: all five keywords "hip", two deep copies, every .grad bit-identical, on specs tiny and tinyP.
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import fixup_train_cases as C
from conftest import record_parity

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -40
BAR = 4.0
T_, K_ = 8, 16
HS = [1, 2, 3, T_ - 1, T_, T_ + 1, 2 * T_ + 1]
CS = [1, 3, 4, 8, 20, K_, K_ + 4]
SHAPES = [(b, h, w, c) for c in sorted(set(CS)) for h in HS for w in HS for b in (1, 2)]
SMALL = [(b, h, w, c) for c in sorted(set(CS)) for (h, w) in ((1, 1), (1, 2), (2, 1), (3, 3), (T_ - 1, T_ + 1), (T_ + 1, 3))
         for b in (1, 2)]
COUNTS = [1, 3, 4, 5, 255, 256, 257, 2 ** 20 + 3]
POISON = 7.0e37
GUARD = 64                                              # floats: 256 bytes, so an offset of 0 keeps 16-byte alignment


def P(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def ints(shape, seed, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def up_shape(shape):
    return (shape[0], 2 * shape[1], 2 * shape[2], shape[3])


def within(got, want64, bound64, what):
    got, want64, bound64 = got.detach().double().cpu().reshape(-1), want64.reshape(-1), bound64.reshape(-1)
    assert got.shape == want64.shape, what
    over = (got - want64).abs() - bound64
    assert bool((over <= 0).all()), (what, float(over.max()), float(bound64.max()))
    return float(((got - want64).abs() / bound64.clamp_min(1e-300)).max())


def composition(ops, t_low, s_low, t, g, a, b, sc, b4, b1d):
    """The existing ops the new nodes fuse -> every tensor and scalar they produce."""
    v = ops.bicubic_up2_bias(t_low)
    y_act = ops.fixup_act(v, a, b)
    g_v, g_a, g_b = ops.fixup_act_backward(g, v, a)
    g_t_low, _ = ops.bicubic_up2_backward(g_v, want_bias=False)
    y_out = ops.fixup_out(t, ops.bicubic_up2_bias(s_low), sc, b4, b1d)
    g_t, g_scale, g_bias = ops.fixup_out_backward(g, t, sc)
    g_s_low, _ = ops.bicubic_up2_backward(g, want_bias=False)
    return dict(y_act=y_act, g_t_low=g_t_low, g_a=g_a, g_b=g_b, y_out=y_out, g_t=g_t, g_s_low=g_s_low, g_scale=g_scale,
                g_bias=g_bias, g_v=g_v)


def fused(ops, t_low, s_low, t, g, a, b, sc, b4, b1d):
    g_t_low, g_a, g_b = ops.up2_act_backward(g, t_low, a)
    g_t, g_s_low, g_scale, g_bias = ops.fixup_out_up_backward(g, t, sc)
    return dict(y_act=ops.up2_act(t_low, a, b), g_t_low=g_t_low, g_a=g_a, g_b=g_b,
                y_out=ops.fixup_out_up(t, s_low, sc, b4, b1d), g_t=g_t, g_s_low=g_s_low, g_scale=g_scale, g_bias=g_bias)


TENSORS = ("y_act", "g_t_low", "y_out", "g_t", "g_s_low")
SCALARS = ("g_a", "g_b", "g_scale", "g_bias")


def data(shape, seed):
    big = up_shape(shape)
    return dict(t_low=rnd(shape, seed, 1.5).cuda(), s_low=rnd(shape, seed + 1).cuda(), t=rnd(big, seed + 2).cuda(),
                g=rnd(big, seed + 3).cuda(), a=P(0.25 - 0.01 * (seed % 7)), b=P(-0.125 + 0.02 * (seed % 5)),
                sc=P(0.8125 + (seed % 9) / 64), b4=P(0.07), b1d=P(-0.11))


def scalar_terms(comp, d):
    """name -> (sum of |terms|) of each scalar gradient, in fp64."""
    g64, t64 = d["g"].double(), d["t"].double()
    return {"g_a": float(comp["g_v"].double().abs().sum()), "g_b": float(g64.abs().sum()),
            "g_scale": float((g64 * t64).abs().sum()), "g_bias": float(g64.abs().sum())}


# ---- exact properties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", sorted(set(CS)))
def test_fusion_equals_composition(amd, c):
    """Every tensor bit for bit; every scalar gradient within two roundings and two reordering terms of the composition's."""
    ops = amd.ops
    worst = 0.0
    for i, shape in enumerate(s for s in SHAPES if s[3] == c):
        d = data(shape, 31 * i + c)
        comp, mine = composition(ops, **d), fused(ops, **d)
        for k in TENSORS:
            assert mine[k].shape == comp[k].shape and torch.equal(mine[k], comp[k]), (k, shape)
        terms = scalar_terms(comp, d)
        for k in SCALARS:
            s = float(comp[k].double())
            bound = 2 * (U * abs(s) + TINY * terms[k])
            err = abs(float(mine[k].double()) - s)
            assert err <= bound, (k, shape, err, bound)
            worst = max(worst, err / max(bound, 1e-300))
    record_parity("conv_up_train_scalars_vs_composition", c=c, worst_fraction_of_bound=worst)


# ---- the C ABI on buffers of our own: guard bands, and every pointer one float off a 16-byte boundary ---------------------------
class Arena:
    """Tensors inside poisoned buffers: `off` floats past a 16-byte boundary, GUARD poisoned floats on either side."""

    def __init__(self, off):
        self.off, self.bufs = off, []

    def place(self, shape, src=None):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * GUARD + self.off,), POISON, dtype=torch.float32, device="cuda")
        view = buf[GUARD + self.off:GUARD + self.off + n].view(shape)
        assert view.data_ptr() % 16 == 4 * self.off
        if src is not None:
            view.copy_(src)
        self.bufs.append((buf, n, src is None))
        return view

    def check(self, what):
        for buf, n, is_output in self.bufs:
            lo, hi = buf[:GUARD + self.off], buf[GUARD + self.off + n:]
            assert bool((lo == POISON).all()) and bool((hi == POISON).all()), what
            if is_output:
                assert not bool((buf[GUARD + self.off:GUARD + self.off + n] == POISON).any()), (what, "unwritten output")


def raw(amd, shape, d, off):
    """The four entries through ctypes on Arena tensors -> the dict of `fused`."""
    L, lib = amd._lib, amd._lib.lib()
    B, H, W, Cc = shape
    big = up_shape(shape)
    ar = Arena(off)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    t_low, s_low, t, g = (ar.place(x.shape, x) for x in (d["t_low"], d["s_low"], d["t"], d["g"]))
    a, b, sc, b4, b1d = (ar.place((1,), d[k]) for k in ("a", "b", "sc", "b4", "b1d"))
    out = {k: ar.place(big) for k in ("y_act", "y_out", "g_t")}
    out.update({k: ar.place(shape) for k in ("g_t_low", "g_s_low")})
    out.update({k: ar.place((1,)) for k in ("g_a", "g_b", "g_scale", "g_bias", "g_bias1d")})
    ws = torch.empty(lib.vqae_up_train_workspace_bytes(B, H, W, Cc), dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.vqae_up2_act_f32(p(t_low), p(a), p(b), B, H, W, Cc, p(out["y_act"]), st))
    L.check(lib.vqae_up2_act_backward_f32(p(g), p(t_low), p(a), B, H, W, Cc, p(out["g_t_low"]), p(out["g_a"]), p(out["g_b"]),
                                          p(ws), st))
    L.check(lib.vqae_fixup_out_up_f32(p(t), p(s_low), p(sc), p(b4), p(b1d), B, H, W, Cc, p(out["y_out"]), st))
    L.check(lib.vqae_fixup_out_up_backward_f32(p(g), p(t), p(sc), B, H, W, Cc, p(out["g_t"]), p(out["g_s_low"]),
                                               p(out["g_scale"]), p(out["g_bias"]), p(out["g_bias1d"]), p(ws), st))
    torch.cuda.synchronize()
    ar.check((shape, off))
    assert torch.equal(out["g_bias"], out["g_bias1d"])
    return out


@pytest.mark.parametrize("off", [0, 1])
def test_no_write_outside_the_outputs(amd, off):
    """Every output inside a larger poisoned buffer: the guard bands are untouched and every output element is written.
    off = 1: every pointer one float past a 16-byte boundary, so C % 4 == 0 takes the scalar path too; same bits."""
    for i, shape in enumerate(SMALL + [(1, 2 * T_ + 1, T_ + 1, K_ + 4)]):
        d = data(shape, 500 + i)
        got, want = raw(amd, shape, d, off), fused(amd.ops, **d)
        for k in TENSORS + SCALARS:
            assert torch.equal(got[k].contiguous(), want[k]), (k, shape, off)


def test_runs_are_bit_identical(amd):
    for i, shape in enumerate(SMALL[::5] + [(2, 2 * T_ + 1, 2 * T_ + 1, K_ + 4), (1, 3, 2 ** 15 + 1, 4)]):
        d = data(shape, 900 + i)
        one, two = fused(amd.ops, **d), fused(amd.ops, **d)
        for k in TENSORS + SCALARS:
            assert torch.equal(one[k], two[k]), (k, shape)


@pytest.mark.parametrize("shape", [(1, 1, n, 1) for n in COUNTS] + [(2, 5, 7, c) for c in (1, 3, 4, 8, 20)],
                         ids=lambda s: "x".join(map(str, s)))
def test_integer_sums_are_exact(amd, shape):
    """Small-integer data: every scalar gradient is the integer sum, so every output element is counted exactly once -- with
    one tile, with many, and with more tiles than workgroups.  t_low in 1 .. 4 keeps up2(t_low) + 1/2 > 0 (the taps' negative
    mass is 0.32 of 1.32), so ELU' = 1 and g_a = g_b = sum g; g_t_low and g_s_low are then the exact adjoint of g."""
    ops, T = amd.ops, amd.train
    big = up_shape(shape)
    g, t, t_low = ints(big, 1, -3, 3), ints(big, 2, -4, 4), ints(shape, 3, 1, 4)
    gd = g.cuda()
    g_t_low, g_a, g_b = ops.up2_act_backward(gd, t_low.cuda(), P(0.5))
    g_t, g_s_low, g_scale, g_bias = ops.fixup_out_up_backward(gd, t.cuda(), P(1.5))
    total = float(g.double().sum())
    assert float(g_a) == total == float(g_b) == float(g_bias)
    assert float(g_scale) == float((g.double() * t.double()).sum())
    assert torch.equal(g_t.cpu(), g * 1.5) and torch.equal(g_t_low, g_s_low)
    if shape[2] <= 512:                                   # the restatement's operator is a dense [2W, W] matrix
        assert torch.equal(g_s_low.cpu().double(), T._bicubic_up2_adjoint_torch(g.double()))
    else:
        assert float(g_s_low.double().sum()) == total     # the adjoint's columns sum to 1, exactly on this data


# ---- element-wise bounds against the fp64 restatement -------------------------------------------------------------------------
def test_bounds_against_fp64(amd):
    T, ops = amd.train, amd.ops
    worst = {}

    def note(k, frac):
        worst[k] = max(worst.get(k, 0.0), frac)

    for i, shape in enumerate(SMALL):
        B, H, W, Cc = shape
        d = data(shape, 700 + i)
        mine = fused(ops, **d)
        t_low, s_low, t, g, a, b, sc, b4, b1d = (d[k].double().cpu() for k in ("t_low", "s_low", "t", "g", "a", "b", "sc", "b4", "b1d"))
        ah, aw = T.up2_matrix(H).abs(), T.up2_matrix(W).abs()
        up_abs = lambda x: torch.einsum("oh,bhwc->bowc", ah, torch.einsum("pw,bhwc->bhpc", aw, x))
        adj_abs = lambda x: torch.einsum("pw,bhpc->bhwc", aw, torch.einsum("oh,bowc->bhwc", ah, x))
        A = up_abs(t_low.abs())
        w = T._bicubic_up2_torch(t_low, None) + a
        e, dd = F.elu(w), T.elu_grad(w)
        y = e + b
        note("up2_act", within(mine["y_act"], T.up2_act(t_low, a, b), U * (10 * A + w.abs() + 8 * e.abs() + y.abs()), ("y_act", shape)))
        g_v = g * dd
        b_gv = U * g.abs() * dd * (10 * A + w.abs() + 10)
        note("g_t_low", within(mine["g_t_low"], T._bicubic_up2_adjoint_torch(g_v), adj_abs(b_gv) + 17 * U * adj_abs(g_v.abs()),
                               ("g_t_low", shape)))
        note("g_a", within(mine["g_a"], g_v.sum(), b_gv.sum() + U * g_v.sum().abs() + TINY * g_v.abs().sum(), ("g_a", shape)))
        note("g_b", within(mine["g_b"], g.sum(), U * g.sum().abs() + TINY * g.abs().sum(), ("g_b", shape)))
        vs = T._bicubic_up2_torch(s_low, None)
        m = (t * sc).abs() + b4.abs() + vs.abs() + b1d.abs()
        note("fixup_out_up", within(mine["y_out"], T.fixup_out_up(t, s_low, sc, b4, b1d), 10 * U * up_abs(s_low.abs()) + 4 * U * m,
                                    ("y_out", shape)))
        note("g_t", within(mine["g_t"], g * sc, U * (g * sc).abs(), ("g_t", shape)))
        note("g_s_low", within(mine["g_s_low"], T._bicubic_up2_adjoint_torch(g), 17 * U * adj_abs(g.abs()), ("g_s_low", shape)))
        gs = (g * t).sum()
        note("g_scale", within(mine["g_scale"], gs, U * gs.abs() + TINY * (g * t).abs().sum(), ("g_scale", shape)))
        note("g_bias", within(mine["g_bias"], g.sum(), U * g.sum().abs() + TINY * g.abs().sum(), ("g_bias", shape)))
    record_parity("conv_up_train_bounds", shapes=len(SMALL), **{"worst_fraction_" + k: v for k, v in worst.items()})


# ---- blocks and the whole model against the reference's autograd -----------------------------------------------------------------
@pytest.mark.parametrize("conv1x1", ["torch", "hip"])
@pytest.mark.parametrize("case", [c for c in C.block_cases() if c.startswith("up_")])
def test_block_parity(amd, case, conv1x1):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    cls = lambda ci, co, mode: PreActFixupResBlock(ci, co, mode, conv1x1=conv1x1, conv_up="hip")
    block, x, g, ref = C.block_case(case, cls, device="cuda")
    T.stats.update(conv_up_hip=0, conv_up_fallbacks=0, conv1x1_hip=0, conv1x1_fallbacks=0)
    got = C.block_results(block, x.contiguous(memory_format=torch.channels_last), g, lambda b, t: b(t))
    assert T.stats["conv_up_hip"] == 2 and T.stats["conv_up_fallbacks"] == 0
    assert T.stats["conv1x1_hip"] == (4 if conv1x1 == "hip" else 0) and T.stats["conv1x1_fallbacks"] == 0
    stock = C.block_results(block, x, g, T.block_forward_torch)
    torch.cuda.synchronize()
    assert set(got) == set(ref)
    fails = []
    for k, (v64, e_cpu) in ref.items():
        e_dev, e_gpu = C.dist(got[k], v64.reshape(got[k].shape)), C.dist(stock[k], v64.reshape(stock[k].shape))
        e_ref = max(e_cpu, e_gpu)
        print(f"conv_up_train_block {case} conv1x1={conv1x1} {k}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
        record_parity("conv_up_train_block", case=case, conv1x1=conv1x1, tensor=k, e_dev=e_dev, e_ref_cpu32=e_cpu,
                      e_ref_stock_gpu=e_gpu)
        assert bool(torch.isfinite(got[k]).all())
        if not e_dev <= BAR * e_ref:
            fails.append((k, e_dev, e_ref))
    assert not fails, fails


def test_whole_model_closed_loop(amd):
    """The fixture's three steps with conv_up="hip" + vqae_amd.FusedAdamW: the recorded codes exactly; losses, parameters and
    buffers within 4 x e_ref, measured as tests/test_fixup_train_gpu.py::test_whole_model_closed_loop measures them."""
    import test_fixup_train_gpu as base
    z = C.fixture()
    fwd = lambda m, x: amd.train.forward_train(m, x, return_indices=True, conv_up="hip")
    amd.train.stats.update(conv_up_hip=0, conv_up_fallbacks=0)
    model, sd0, losses, idxs = base._run_loop(amd, fwd, amd.FusedAdamW, True)
    assert amd.train.stats["conv_up_hip"] > 0 and amd.train.stats["conv_up_fallbacks"] == 0
    smodel, ssd0, slosses, sidxs = base._run_loop(amd, base._stock_forward(amd), torch.optim.AdamW, False)
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
        print(f"conv_up_train_loop {tag}: e_dev {e_dev:.3e} e_ref cpu {e_cpu:.3e} stock-gpu {e_gpu:.3e}")
        record_parity("conv_up_train_loop", tensor=tag, e_dev=e_dev, e_ref_cpu32=e_cpu, e_ref_stock_gpu=e_gpu)
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
    """All five keywords "hip": two runs of step + backward on two deep copies of a model give the same bits in every .grad."""
    T = amd.train
    model, x = _train_model(amd, name)
    all5 = dict(conv1x1="hip", conv_down="hip", conv3x3="hip", conv3x3z="hip", conv_up="hip")
    n_up = sum(1 for m in model.modules() if getattr(m, "mode", None) == "up")
    grads, outs = [], []
    T.stats.update({k: 0 for k in T.stats})
    for m in (copy.deepcopy(model), copy.deepcopy(model)):
        out, recon, (vq_loss,) = T.step(m, x, **all5)
        (recon + vq_loss).backward()
        torch.cuda.synchronize()
        outs.append((out.detach(), recon.detach(), vq_loss.detach()))
        grads.append({k: p.grad for k, p in m.named_parameters()})
    assert n_up > 0 and T.stats["conv_up_hip"] == 2 * 2 * n_up, dict(T.stats)
    assert all(T.stats[k] == 0 for k in T.stats if k.endswith("fallbacks")), dict(T.stats)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in grads[0].values())
    differ = [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]
    assert not differ, differ
