"""GPU: the 16-bit-I/O forms of the element-wise Fixup training nodes (csrc/fixup_train_io.hip behind ops.*_io and
vqae_amd.train's Functions under torch.autocast).

Yardstick: the composition of the existing fp32 ops on up-cast inputs with torch's casts around them --
    forward   ops.fixup_act(x.float(), ...).to(T)
    backward  ops.fixup_act_backward(g.float(), x.float(), ...), g_x.to(x.dtype)
and the same pattern for `out` (g_skip: g.to(skip's dtype)).  No test runs the fp32 Functions on 16-bit tensors.

Tensors: every output tensor equals the yardstick BIT FOR BIT (NaNs by position), for every (input, output) dtype combination
of bf16 and of f16; fp32 -> fp32 equals the _f32 entry point.  The entry points are called on views inside larger buffers:
the base pointers sit on the natural alignment (the vector path) or one element off it (the scalar path), and the GUARD
elements around every output must stay untouched.
Data: `special` plants +-inf, NaN, values that overflow f16 behind the ELU, f16 subnormals and signed zeros in random data.

Sums (g_a, g_b, g_scale, g_bias): the kernels keep the fp32 kernels' element order, so on aligned bases every sum EQUALS the
yardstick's bit for bit (asserted; NaN by position on special data).  One element off the alignment the kernel takes the
scalar path while the yardstick's fresh fp32 copies take the vector path: two fp64 summation orders rounded once, within
2 n 2^-53 sum|v| + 1 ulp32 of each other (sum|v| in fp64 on the host), and exactly equal on integer-valued data.

Blocks and the step: under bf16 and f16 autocast, against train.block_forward_torch under the same autocast: distance to the
fixture's fp64 values <= 4 x the stock route's, the training suite's bar.  Measured ratios e_dev / e_ref on an MI355X:
0.62 .. 1.41 under bf16, 0.47 .. 1.50 under f16 (profiles/fixup_train16_parity_report.jsonl).
"""
import ctypes

import pytest
import torch

import fixup_train_cases as C
from conftest import record_parity

pytestmark = pytest.mark.gpu

BAR = 4.0
F32 = torch.float32
T16 = [torch.bfloat16, torch.float16]
IDS = {torch.bfloat16: "bf16", torch.float16: "f16"}
COUNTS = [1, 3, 4, 5, 7, 8, 9, 1023, 2 ** 20 + 3]          # the last: more than one grid stride of 1024 x 256 x 4 elements
HALO_SHAPES = [(b, h, w, c) for h in (1, 2, 3, 5) for w in (1, 2, 3, 5) for c in (1, 3, 8) for b in (1, 2)]
GUARD = 8                                                   # elements; 8 keeps a view on 16 bytes, 9 puts it one element off
SENTINEL = 1984.0                                           # exact in bf16 and f16


def combos(T):
    """(input dtype, output dtype) with one 16-bit type T at least once."""
    return [(F32, T), (T, F32), (T, T)]


def P(v):
    return torch.tensor([v], dtype=F32, device="cuda")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def special(shape, seed, dtype):
    """Random data with +-inf, NaN, f16 overflow behind the ELU, f16 subnormals and signed zeros planted (where n allows)."""
    v = torch.randn(shape, generator=gen(seed)) * 3.0
    flat = v.reshape(-1)
    plant = [float("inf"), float("-inf"), float("nan"), 65504.0, 1.0e5, -1.0e5, 6.0e-8, -3.0e-7, 5.0e-6, 0.0, -0.0, 65519.0]
    pos = torch.randperm(flat.numel(), generator=gen(seed + 1))[:len(plant)]
    for p, val in zip(pos.tolist(), plant):
        flat[p] = val
    return v.to(dtype)


def rnd(shape, seed, dtype):
    return torch.randn(shape, generator=gen(seed)).to(dtype)


def ints(shape, seed, dtype, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).to(dtype)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same(got, want, what):
    """Equal dtype, shape and bits; NaNs by position."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    n_got, n_want = got.isnan(), want.isnan()
    assert torch.equal(n_got, n_want), (what, "NaN positions")
    zero = torch.zeros((), dtype=got.dtype, device=got.device)
    assert torch.equal(bits(torch.where(n_got, zero, got)), bits(torch.where(n_want, zero, want))), what


def ulp32(v):
    v = torch.as_tensor(float(v), dtype=F32).abs()
    return float(torch.nextafter(v, torch.tensor(float("inf"))) - v)


def sum_close(got, want, n, abs_terms64, what):
    """Two fp64 summation orders of the same n fp32 terms, each rounded to fp32 once."""
    bound = 2.0 * n * 2.0 ** -53 * float(abs_terms64) + ulp32(want)
    assert abs(float(got) - float(want)) <= bound, (what, float(got), float(want), bound)


class Banded:
    """A tensor as a view inside a larger buffer of SENTINEL: `off` elements past a 16-byte boundary, GUARD elements on
    either side."""

    def __init__(self, shape, dtype, off, src=None):
        n = 1
        for s in shape:
            n *= s
        lead = GUARD + off
        self.buf = torch.full((lead + n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.view = self.buf[lead:lead + n].view(shape)
        self.lead, self.n = lead, n
        if src is not None:
            self.view.copy_(src)

    def intact(self):
        return bool((self.buf[:self.lead] == SENTINEL).all()) and bool((self.buf[self.lead + self.n:] == SENTINEL).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Lib:
    """The four entry points on raw views (ops.*_io allocates its own, aligned outputs)."""

    def __init__(self, amd):
        self.L, self.ops, self.train = amd._lib, amd.ops, amd.train
        self.lib = amd._lib.lib()

    def code(self, dtype):
        return {F32: self.L.DT_F32, torch.bfloat16: self.L.DT_BF16, torch.float16: self.L.DT_F16}[dtype]

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ws(self, n):
        return torch.empty(self.lib.vqae_fixup_train_workspace_bytes(int(n)), dtype=torch.uint8, device="cuda")

    def act(self, x, a, b, halo, dy, off):
        """-> y (a clone), the guards checked.  a None: the plain mode."""
        B, H, W, Cc = x.shape
        xb = Banded(x.shape, x.dtype, off, x)
        yb = Banded((B, H + 2 * halo, W + 2 * halo, Cc), dy, off)
        self.L.check(self.lib.vqae_fixup_act_io(_p(xb.view), self.code(x.dtype), _p(a), _p(b), int(a is not None), halo, B, H, W,
                                                Cc, _p(yb.view), self.code(dy), self.stream()))
        assert yb.intact() and xb.intact(), ("act guards", x.shape, x.dtype, dy, off)
        return yb.view.clone()

    def act_backward(self, g, x, a, halo, dx, off):
        """-> (g_x | None, g_a | None, g_b).  x, a None: the plain mode, dx the forward's input dtype."""
        act = a is not None
        B, H, W, Cc = g.shape[0], g.shape[1] - 2 * halo, g.shape[2] - 2 * halo, g.shape[3]
        gb = Banded(g.shape, g.dtype, off, g)
        xb = Banded(x.shape, dx, off, x) if act else None
        write = act or dx != g.dtype
        gxb = Banded((B, H, W, Cc), dx, off) if write else None
        sums = torch.full((2 * GUARD + 2,), SENTINEL, dtype=F32, device="cuda")
        g_a, g_b = sums[GUARD:GUARD + 1], sums[GUARD + 1:GUARD + 2]
        self.L.check(self.lib.vqae_fixup_act_backward_io(
            _p(gb.view), self.code(g.dtype), _p(xb.view) if act else None, self.code(dx), _p(a), int(act), halo, B, H, W, Cc,
            _p(gxb.view) if write else None, _p(g_a) if act else None, _p(g_b), _p(self.ws(g.numel())), self.stream()))
        assert gb.intact() and (gxb is None or gxb.intact()), ("act backward guards", g.shape, g.dtype, dx, off)
        assert bool((sums[:GUARD] == SENTINEL).all()) and bool((sums[GUARD + 2:] == SENTINEL).all())
        assert act or float(sums[GUARD]) == SENTINEL
        return gxb.view.clone() if write else None, g_a.clone() if act else None, g_b.clone()

    def out(self, t, skip, scale, b4, b1d, off):
        tb, sb = Banded(t.shape, t.dtype, off, t), Banded(skip.shape, skip.dtype, off, skip)
        yb = Banded(t.shape, F32, off)
        self.L.check(self.lib.vqae_fixup_out_io(_p(tb.view), self.code(t.dtype), _p(sb.view), self.code(skip.dtype), _p(scale),
                                                _p(b4), _p(b1d), t.numel(), _p(yb.view), self.L.DT_F32, self.stream()))
        assert yb.intact(), ("out guards", t.shape, t.dtype, skip.dtype, off)
        return yb.view.clone()

    def out_backward(self, g, t, scale, ds, off):
        """-> (g_t, g_skip | None, g_scale, g_bias)."""
        gb, tb = Banded(g.shape, F32, off, g), Banded(t.shape, t.dtype, off, t)
        gtb = Banded(t.shape, t.dtype, off)
        gsb = Banded(t.shape, ds, off) if ds != F32 else None
        sums = torch.full((2 * GUARD + 2,), SENTINEL, dtype=F32, device="cuda")
        g_scale, g_bias = sums[GUARD:GUARD + 1], sums[GUARD + 1:GUARD + 2]
        self.L.check(self.lib.vqae_fixup_out_backward_io(
            _p(gb.view), _p(tb.view), self.code(t.dtype), _p(scale), g.numel(), _p(gtb.view), _p(gsb.view) if gsb else None,
            self.code(ds), _p(g_scale), _p(g_bias), None, _p(self.ws(g.numel())), self.stream()))
        assert gtb.intact() and (gsb is None or gsb.intact()), ("out backward guards", t.shape, t.dtype, ds, off)
        assert bool((sums[:GUARD] == SENTINEL).all()) and bool((sums[GUARD + 2:] == SENTINEL).all())
        return gtb.view.clone(), gsb.view.clone() if gsb else None, g_scale.clone(), g_bias.clone()


@pytest.fixture(scope="module")
def lib(amd):
    return Lib(amd)


# ---- act / plain -----------------------------------------------------------------------------------------------------------------
def check_act(lib, shape, halo, dx, dy, off, kind, seed, a, b):
    """One (shape, dtypes, base offset, data kind) of act (a given) or plain (a None): forward and backward against the
    yardstick."""
    ops = lib.ops
    B, H, W, Cc = shape
    gshape = (B, H + 2 * halo, W + 2 * halo, Cc)
    n = B * H * W * Cc
    make = {"special": special, "random": rnd, "ints": ints}[kind]
    x = (ints(shape, seed, dx, 1, 4) if kind == "ints" else make(shape, seed, dx)).cuda()   # ints: x + a > 0, ELU' = 1
    g = make(gshape, seed + 7, dy).cuda()
    what = (shape, halo, IDS.get(dx, "f32"), IDS.get(dy, "f32"), off, kind, "act" if a is not None else "plain")
    y = lib.act(x, a, b, halo, dy, off)
    same(y, ops.fixup_act(x.float(), a, b, halo).to(dy), ("forward",) + what)
    if a is not None:
        g_x, g_a, g_b = lib.act_backward(g, x, a, halo, dx, off)
        w_x, w_a, w_b = ops.fixup_act_backward(g.float(), x.float(), a, halo)
        same(g_x, w_x.to(dx), ("g_x",) + what)
        fold = lib.train.fold_circular_nhwc(g.double()) if halo else g.double()          # the terms of g_b
        terms = ((w_x.double().abs().sum(), g_a, w_a, "g_a"), (fold.abs().sum(), g_b, w_b, "g_b"))
    else:
        g_x, _, g_b = lib.act_backward(g, None, None, 0, dx, off)
        _, _, w_b = ops.fixup_act_backward(g.float(), None, None, act=False)
        assert (g_x is None) == (dx == dy)
        if g_x is not None:
            same(g_x, g.to(dx), ("plain g_x",) + what)
        terms = ((g.double().abs().sum(), g_b, w_b, "g_c"),)
    for abs_sum, got, want, name in terms:
        if off == 0 or kind == "ints":
            same(got, want, (name,) + what)                 # the element order is kept; integer data sums exactly in any order
        elif kind == "random":
            sum_close(got, want, n, abs_sum, (name,) + what)
    if kind == "ints":
        gs = float(g.double().sum())
        assert float(g_b) == gs and (a is None or float(g_a) == gs), what


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_act_flat(lib, T, n):
    shape = (1, 1, n, 1)
    kinds = ("special", "random", "ints") if n < 2 ** 20 else ("special", "random")
    for i, (dx, dy) in enumerate(combos(T)):
        for off in (0, 1):
            for kind in kinds:
                check_act(lib, shape, 0, dx, dy, off, kind, 100 * i + n % 97, P(0.25), P(-0.125))
                check_act(lib, shape, 0, dx, dy, off, kind, 100 * i + n % 97 + 3, None, P(0.375))
            # a = b = 0: ELU(x) = x for small x, so f16 subnormal results are written; c = 0: y = x cast
            check_act(lib, shape, 0, dx, dy, off, "special", 100 * i + 50, P(0.0), P(0.0))
            check_act(lib, shape, 0, dx, dy, off, "special", 100 * i + 51, None, P(0.0))


@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_act_halo(lib, T):
    """H or W <= 2: the fold collects up to 9 images of a pixel.  C = 8 on an aligned base takes the 4-channel path."""
    for i, shape in enumerate(HALO_SHAPES):
        for j, (dx, dy) in enumerate(combos(T)):
            off = (i + j) % 2
            for kind in ("special", "random", "ints"):
                check_act(lib, shape, 1, dx, dy, off, kind, 10 * i + j, P(0.25), P(-0.125))
            check_act(lib, shape, 1, dx, dy, 1 - off, "random", 10 * i + j + 5, P(-0.5), P(0.0625))


def test_fp32_combination_is_the_f32_entry_point(lib):
    ops = lib.ops
    a, b, sc = P(0.25), P(-0.125), P(0.8125)
    for shape in [(1, 1, 9, 1), (1, 1, 1023, 1), (2, 2, 3, 8), (1, 5, 1, 3)]:
        x, t = special(shape, 1, F32).cuda(), rnd(shape, 2, F32).cuda()
        for halo in (0, 1):
            g = rnd((shape[0], shape[1] + 2 * halo, shape[2] + 2 * halo, shape[3]), 3, F32).cuda()
            same(lib.act(x, a, b, halo, F32, 0), ops.fixup_act(x, a, b, halo), ("act", shape, halo))
            for got, want in zip(lib.act_backward(g, t, a, halo, F32, 0), ops.fixup_act_backward(g, t, a, halo)):
                same(got, want, ("act backward", shape, halo))
        same(lib.act(x, None, b, 0, F32, 0), ops.fixup_act(x, None, b), ("plain", shape))
        g = rnd(shape, 4, F32).cuda()
        g_x, _, g_c = lib.act_backward(g, None, None, 0, F32, 0)
        assert g_x is None
        same(g_c, ops.fixup_act_backward(g, None, None, act=False)[2], ("plain backward", shape))
        same(lib.out(t, x, sc, a, b, 0), ops.fixup_out(t, x, sc, a, b), ("out", shape))
        g_t, g_skip, g_scale, g_bias = lib.out_backward(g, t, sc, F32, 0)
        assert g_skip is None
        for got, want in zip((g_t, g_scale, g_bias), ops.fixup_out_backward(g, t, sc)):
            same(got, want, ("out backward", shape))


# ---- out -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_out_flat(lib, T, n):
    ops = lib.ops
    shape = (1, 1, n, 1)
    sc, b4, b1d = P(0.8125), P(0.07), P(-0.11)
    kinds = ("special", "random", "ints") if n < 2 ** 20 else ("special", "random")
    for i, (dt, ds) in enumerate([(T, F32), (F32, T), (T, T)]):
        for off in (0, 1):
            for kind in kinds:
                make = {"special": special, "random": rnd, "ints": ints}[kind]
                t, skip = make(shape, 10 * i + 1, dt).cuda(), make(shape, 10 * i + 2, ds).cuda()
                g = make(shape, 10 * i + 3, F32).cuda()
                what = (n, IDS.get(dt, "f32"), IDS.get(ds, "f32"), off, kind)
                for bd in (b1d, None):
                    same(lib.out(t, skip, sc, b4, bd, off), ops.fixup_out(t.float(), skip.float(), sc, b4, bd), ("out",) + what)
                g_t, g_skip, g_scale, g_bias = lib.out_backward(g, t, sc, ds, off)
                w_t, w_scale, w_bias = ops.fixup_out_backward(g, t.float(), sc)
                same(g_t, w_t.to(dt), ("g_t",) + what)
                assert (g_skip is None) == (ds == F32)
                if g_skip is not None:
                    same(g_skip, g.to(ds), ("g_skip",) + what)
                if off == 0 or kind == "ints":
                    same(g_scale, w_scale, ("g_scale",) + what)
                    same(g_bias, w_bias, ("g_bias",) + what)
                elif kind == "random":
                    sum_close(g_scale, w_scale, n, (g.double() * t.double()).abs().sum(), ("g_scale",) + what)
                    sum_close(g_bias, w_bias, n, g.double().abs().sum(), ("g_bias",) + what)
                if kind == "ints":
                    assert float(g_scale) == float((g.double() * t.double()).sum()) and float(g_bias) == float(g.double().sum())


# ---- the wrappers, run to run ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_ops_wrappers_and_repeatability(amd, T):
    """ops.*_io (what train.py calls) against the yardstick, and two runs of each give the same bits."""
    ops = amd.ops
    a, b, sc = P(0.3), P(-0.2), P(0.9)
    for i, shape in enumerate([(2, 3, 5, 8), (1, 2, 2, 3), (1, 1, 2 ** 20 + 3, 1)]):
        B, H, W, Cc = shape
        x32, g32, t32 = (rnd(shape, 10 * i + k, F32).cuda() for k in range(3))
        gh32 = rnd((B, H + 2, W + 2, Cc), 10 * i + 4, F32).cuda()

        def run():
            out = []
            for dx, dy in combos(T):
                x, g, gh = x32.to(dx), g32.to(dy), gh32.to(dy)
                out += [ops.fixup_act_io(x, a, b, 0, dy), ops.fixup_act_io(x, a, b, 1, dy), ops.fixup_act_io(x, None, b, 0, dy)]
                out += ops.fixup_act_backward_io(g, x, a) + ops.fixup_act_backward_io(gh, x, a, 1)
                out += ops.fixup_act_backward_io(g, None, None, act=False, x_dtype=dx)[::2]
                out += [ops.fixup_out_io(t32.to(dx), x32.to(dy), sc, a, b)] + list(ops.fixup_out_backward_io(g32, t32.to(dx), sc, dy))
            return out

        def yardstick():
            out = []
            for dx, dy in combos(T):
                x, g, gh = x32.to(dx), g32.to(dy), gh32.to(dy)
                out += [ops.fixup_act(x.float(), a, b, h).to(dy) for h in (0, 1)] + [ops.fixup_act(x.float(), None, b).to(dy)]
                for gg, h in ((g, 0), (gh, 1)):
                    w_x, w_a, w_b = ops.fixup_act_backward(gg.float(), x.float(), a, h)
                    out += [w_x.to(dx), w_a, w_b]
                out += [g if dx == dy else g.to(dx), ops.fixup_act_backward(g.float(), None, None, act=False)[2]]
                t = t32.to(dx)
                w_t, w_scale, w_bias = ops.fixup_out_backward(g32, t.float(), sc)
                out += [ops.fixup_out(t.float(), x32.to(dy).float(), sc, a, b), w_t.to(dx), g32.to(dy), w_scale, w_bias]
            return out

        first, second, want = run(), run(), yardstick()
        assert len(first) == len(want)
        for k, (p, q, w) in enumerate(zip(first, second, want)):
            same(p, q, ("run to run", shape, k))
            same(p, w, ("wrapper", shape, k))


# ---- blocks and the step under autocast ---------------------------------------------------------------------------------------
BLOCK_CASES = [c for c in C.block_cases() if c.startswith(("same", "down", "out"))]


@pytest.mark.parametrize("case", BLOCK_CASES)
@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_block_parity_under_autocast(amd, T, case):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    Tr = amd.train
    block, x, g, ref = C.block_case(case, PreActFixupResBlock, device="cuda")

    def under(forward):
        def run(blk, t):
            with torch.autocast("cuda", dtype=T):
                return forward(blk, t)
        return run

    before = dict(Tr.stats)
    got = C.block_results(block, x.contiguous(memory_format=torch.channels_last), g, under(lambda b, t: b(t)))
    stock = C.block_results(block, x, g, under(Tr.block_forward_torch))
    torch.cuda.synchronize()
    assert Tr.stats["io16_hip"] > before["io16_hip"] and Tr.stats["io16_fallbacks"] == before["io16_fallbacks"]
    assert set(got) == set(ref) and all(v.dtype == F32 for v in got.values())
    fails = []
    for k, (v64, _) in ref.items():
        e_dev, e_ref = C.dist(got[k], v64.reshape(got[k].shape)), C.dist(stock[k], v64.reshape(stock[k].shape))
        print(f"fixup_train16_block {IDS[T]} {case} {k}: e_dev {e_dev:.3e} e_ref {e_ref:.3e} ratio {e_dev / e_ref:.3f}")
        record_parity("fixup_train16_block", dtype=IDS[T], case=case, tensor=k, e_dev=e_dev, e_ref_stock_autocast=e_ref,
                      ratio=e_dev / e_ref)
        assert bool(torch.isfinite(got[k]).all())
        if not e_dev <= BAR * e_ref:
            fails.append((k, e_dev, e_ref))
    assert not fails, fails


@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_whole_step_under_autocast(amd, T):
    """One step + backward + FusedAdamW on spec tiny, batch 2, 32 x 32: bf16 as it is, f16 with a GradScaler."""
    Tr = amd.train
    model, batches = C.loop_model(device="cuda")
    x = batches[0].contiguous(memory_format=torch.channels_last)
    opt = amd.FusedAdamW(model.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10, enabled=T == torch.float16)
    n_up = sum(1 for m in model.modules() if getattr(m, "mode", None) == "up")
    before = dict(Tr.stats)
    with torch.autocast("cuda", dtype=T):
        out, recon, vq_losses = Tr.step(model, x)
        loss = recon + sum(vq_losses)
    opt.zero_grad()
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(gr is not None and gr.dtype == F32 for gr in grads.values()), [k for k, gr in grads.items() if gr is None]
    # f16: an overflow of the scaled gradients passes through the nodes as inf, and the scaler then skips the step
    finite = all(bool(torch.isfinite(gr).all()) for gr in grads.values())
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(recon)) and all(bool(torch.isfinite(v)) for v in vq_losses)
    assert finite or T == torch.float16
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert Tr.stats["io16_hip"] > before["io16_hip"]
    assert n_up > 0 and Tr.stats["io16_fallbacks"] - before["io16_fallbacks"] == 2 * n_up      # each 'up' block's two bicubic_up2
    record_parity("fixup_train16_step", dtype=IDS[T], recon=float(recon.detach()), vq=float(vq_losses[0].detach()),
                  grads_finite=finite,
                  io16_hip=Tr.stats["io16_hip"] - before["io16_hip"],
                  io16_fallbacks=Tr.stats["io16_fallbacks"] - before["io16_fallbacks"])
