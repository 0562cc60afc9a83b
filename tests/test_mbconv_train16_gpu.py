"""GPU: the 16-bit-I/O forms of the MBConv training nodes (csrc/mbconv_train_io.hip behind ops.*_io and vqae_amd.train_mbconv's
Functions under torch.autocast).

Yardstick: the existing fp32 op on up-cast inputs with torch's casts around it --
    ops.bn_act_train_forward(x.float(), ...): y.to(T); mean, invstd, pool, the running statistics as they are
    ops.bn_act_train_backward(g.float(), x.float(), ...): g_x.to(T); g_gamma, g_beta as they are
    ops.dwconv_train_forward(x.float(), w.to(T).float(), mode).to(T), and the same taps in the backward; g_w as it is
    ops.se_scale_forward(x.float(), gate.float()).to(T); g_x.to(T), g_gate as it is (cast once more for a 16-bit gate)
for T = bf16 and f16.  Every tensor output equals the yardstick BIT FOR BIT (NaNs by position) and every sum equals it bit for
bit, the running statistics after the in-place update included: the kernels keep the fp32 kernels' element-to-thread order and
sum the unrounded fp32 terms.  The entry points are called through ctypes on views inside larger buffers of a sentinel value:
outputs, gradients, sums and workspaces leave their guard bands intact.
Data: random, and `special`: +-inf, NaN, values that overflow f16 behind SiLU, f16 subnormals, signed zeros (for bn_act the
non-finite plants sit in ONE channel, so the others stay informative; the -0 / subnormal products of se_scale are what the
conversion pin of Io16::rnd exists for).
Independent of the project's fp32 kernels: on small integers the 16-bit depthwise forward, data gradient and weight gradient
equal F.conv2d(groups=) / F.conv_transpose2d and their autograd in fp64 exactly.

Blocks and the step: the seven cases of tests/golden/mbconv_train.npz under bf16 and f16 autocast against
train_mbconv.block_forward_torch under the same autocast on the same GPU: distance to the fixture's fp64 values <= 4 x the
stock route's, per tensor group.  Measured ratios e_dev / e_ref on an MI355X: 0.24 .. 1.54 under bf16, 0.51 .. 2.79 under f16
(profiles/mbconv_train16_parity_report.jsonl).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import mbconv_train_cases as C
from conftest import record_parity

pytestmark = pytest.mark.gpu

BAR = 4.0
F32 = torch.float32
T16 = [torch.bfloat16, torch.float16]
IDS = {torch.bfloat16: "bf16", torch.float16: "f16"}
GUARD = 8                                   # elements; keeps a view on 16 bytes
SENTINEL = 1984.0                           # exact in bf16 and f16
BN_C = [4, 8, 36, 260, 1024]                # 260: C4 = 65, 3 pixel lanes and 61 idle threads; 1024: one pixel lane
BN_M = [2, 3, 255, 256, 257, 513]           # rows around one and two strips of 256
BN_M_BIG = 16385                            # at C = 4: the first row count where a finishing lane adds two partial rows
DW_E = [4, 8, 36]
DW_HW = [(h, w) for h in (1, 2, 3, 5) for w in (1, 2, 3, 5)] + [(1, 255), (1, 256), (1, 257)]
SE_SHAPES = [(b, hw, c) for b in (1, 3) for hw in (1, 255, 256, 257) for c in (4, 36)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, dtype, scale=1.0):
    return (torch.randn(shape, generator=gen(seed)) * scale).to(dtype).cuda()


def ints(shape, seed, dtype, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).to(dtype).cuda()


PLANTS = [float("inf"), float("-inf"), float("nan"), 65504.0, 1.0e5, -1.0e5, 6.0e-8, -3.0e-7, 5.0e-6, 0.0, -0.0, 65519.0]


def special(shape, seed, dtype):
    """Random data with +-inf, NaN, f16 overflow, f16 subnormals and signed zeros planted anywhere (where n allows)."""
    v = torch.randn(shape, generator=gen(seed)) * 3.0
    flat = v.reshape(-1)
    pos = torch.randperm(flat.numel(), generator=gen(seed + 1))[:len(PLANTS)]
    for p, val in zip(pos.tolist(), PLANTS):
        flat[p] = val
    return v.to(dtype).cuda()


def special_rows(M, Cc, seed, dtype):
    """[M, C] for bn_act: the non-finite plants in channel 1 only; subnormals and signed zeros in channel 3; the rest random."""
    v = torch.randn(M, Cc, generator=gen(seed)) * 3.0
    rows = torch.randperm(M, generator=gen(seed + 1)).tolist()
    for r, val in zip(rows[:3], (float("inf"), float("-inf"), float("nan"))):
        v[r, 1] = val
    for r, val in zip(rows[:6], (6.0e-8, -3.0e-7, 5.0e-6, 0.0, -0.0, 6.0e-5)):
        v[r, 3] = val
    return v.to(dtype).cuda()


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def same(got, want, what):
    """Equal dtype, shape and bits; NaNs by position."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    n_got, n_want = got.isnan(), want.isnan()
    assert torch.equal(n_got, n_want), (what, "NaN positions")
    zero = torch.zeros((), dtype=got.dtype, device=got.device)
    assert torch.equal(bits(torch.where(n_got, zero, got)), bits(torch.where(n_want, zero, want))), what


class Banded:
    """A tensor as a view inside a larger buffer of SENTINEL: `off` elements past a 16-byte boundary, GUARD elements on
    either side."""

    def __init__(self, shape, dtype, off=0, src=None):
        n = 1
        for s in shape:
            n *= s
        lead = GUARD + off
        self.buf = torch.full((lead + n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.view = self.buf[lead:lead + n].view(shape)
        self.lead, self.n = lead, n
        if src is not None:
            self.view.copy_(src.reshape(shape))

    def intact(self):
        return bool((self.buf[:self.lead] == SENTINEL).all()) and bool((self.buf[self.lead + self.n:] == SENTINEL).all())


class Workspace:
    """`n_bytes` of workspace between two bands of 0xA5 bytes."""
    BAND = 64

    def __init__(self, n_bytes):
        self.n = max(int(n_bytes), 8)
        self.buf = torch.full((2 * self.BAND + self.n,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.buf[self.BAND:self.BAND + self.n]
        assert self.view.data_ptr() % 8 == 0

    def intact(self):
        return bool((self.buf[:self.BAND] == 0xA5).all()) and bool((self.buf[self.BAND + self.n:] == 0xA5).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Lib:
    """The six entry points on raw views inside guard bands (ops.*_io allocates its own, aligned outputs).  Every method
    returns clones and asserts the bands."""

    def __init__(self, amd):
        self.L, self.ops = amd._lib, amd.ops
        self.lib = amd._lib.lib()

    def code(self, dtype):
        return {F32: self.L.DT_F32, torch.bfloat16: self.L.DT_BF16, torch.float16: self.L.DT_F16}[dtype]

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def bn_forward(self, x, gamma, beta, rm, rv, training, silu, want_pool, off=0, momentum=0.1, eps=1e-5):
        """x [B, H, W, C] -> (y, mean, invstd, pool | None); rm, rv updated in place."""
        B, H, W, Cc = x.shape
        xb, yb = Banded(x.shape, x.dtype, off, x), Banded(x.shape, x.dtype, off)
        stat = Banded((2, Cc), torch.float64)
        pool = Banded((B, Cc), F32) if want_pool else None
        ws = Workspace(self.lib.vqae_bn_act_train_workspace_bytes(B, H * W, Cc))
        self.L.check(self.lib.vqae_bn_act_train_forward_io(
            _p(xb.view), _p(gamma), _p(beta), _p(rm), _p(rv), int(training), momentum, eps, int(silu), B, H * W, Cc, _p(yb.view),
            _p(stat.view[0]), _p(stat.view[1]), _p(pool.view) if pool else None, _p(ws.view), self.code(x.dtype), self.stream()))
        assert xb.intact() and yb.intact() and stat.intact() and ws.intact() and (pool is None or pool.intact()), \
            ("bn forward guards", x.shape, x.dtype, off)
        assert torch.equal(bits(xb.view), bits(x))
        return yb.view.clone(), stat.view[0].clone(), stat.view[1].clone(), pool.view.clone() if pool else None

    def bn_backward(self, g, x, mean, invstd, gamma, beta, training, silu, g_pool, off=0):
        """-> (g_x, g_gamma, g_beta)."""
        B, H, W, Cc = x.shape
        gb, xb, gxb = Banded(g.shape, g.dtype, off, g), Banded(x.shape, x.dtype, off, x), Banded(x.shape, x.dtype, off)
        sums = Banded((2, Cc), F32)
        ws = Workspace(self.lib.vqae_bn_act_train_workspace_bytes(B, H * W, Cc))
        self.L.check(self.lib.vqae_bn_act_train_backward_io(
            _p(gb.view), _p(xb.view), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(g_pool), int(training), int(silu), B, H * W,
            Cc, _p(gxb.view), _p(sums.view), _p(ws.view), self.code(x.dtype), self.stream()))
        assert gb.intact() and xb.intact() and gxb.intact() and sums.intact() and ws.intact(), \
            ("bn backward guards", x.shape, x.dtype, off)
        return gxb.view.clone(), sums.view[1].clone(), sums.view[0].clone()

    def dw_forward(self, x, w, mode, off=0):
        B, H, W, Cc = x.shape
        Ho, Wo = self.ops._dw_out_shape(mode, H, W)
        xb, yb = Banded(x.shape, x.dtype, off, x), Banded((B, Ho, Wo, Cc), x.dtype, off)
        self.L.check(self.lib.vqae_dwconv_train_forward_io(_p(xb.view), _p(w), mode, B, H, W, Cc, _p(yb.view), self.code(x.dtype),
                                                           self.stream()))
        assert xb.intact() and yb.intact(), ("dw forward guards", x.shape, x.dtype, mode, off)
        return yb.view.clone()

    def dw_backward(self, g, x, w, mode, need_x, need_w, off=0):
        B, H, W, Cc = x.shape
        gb, xb = Banded(g.shape, g.dtype, off, g), Banded(x.shape, x.dtype, off, x)
        gxb = Banded(x.shape, x.dtype, off) if need_x else None
        gw = Banded(tuple(w.shape), F32) if need_w else None
        ws = Workspace(self.lib.vqae_dwconv_train_workspace_bytes(B, H, W, Cc, mode)) if need_w else None
        self.L.check(self.lib.vqae_dwconv_train_backward_io(
            _p(gb.view), _p(xb.view), _p(w), mode, B, H, W, Cc, _p(gxb.view) if need_x else None, _p(gw.view) if need_w else None,
            _p(ws.view) if need_w else None, self.code(x.dtype), self.stream()))
        assert gb.intact() and xb.intact() and (gxb is None or gxb.intact()) and (gw is None or gw.intact()) \
            and (ws is None or ws.intact()), ("dw backward guards", x.shape, x.dtype, mode, off)
        return gxb.view.clone() if need_x else None, gw.view.clone() if need_w else None

    def se_forward(self, x, gate, off=0, gate_off=0):
        B, H, W, Cc = x.shape
        xb, yb = Banded(x.shape, x.dtype, off, x), Banded(x.shape, x.dtype, off)
        gtb = Banded(gate.shape, gate.dtype, gate_off, gate)
        self.L.check(self.lib.vqae_se_scale_forward_io(_p(xb.view), _p(gtb.view), B, H * W, Cc, _p(yb.view), self.code(x.dtype),
                                                       self.code(gate.dtype), self.stream()))
        assert xb.intact() and yb.intact() and gtb.intact(), ("se forward guards", x.shape, x.dtype, gate.dtype, off)
        return yb.view.clone()

    def se_backward(self, g, x, gate, off=0, gate_off=0):
        B, H, W, Cc = x.shape
        gb, xb, gxb = Banded(g.shape, g.dtype, off, g), Banded(x.shape, x.dtype, off, x), Banded(x.shape, x.dtype, off)
        gtb, ggb = Banded(gate.shape, gate.dtype, gate_off, gate), Banded(gate.shape, gate.dtype, gate_off)
        ws = Workspace(self.lib.vqae_se_scale_workspace_bytes(B, H * W, Cc))
        self.L.check(self.lib.vqae_se_scale_backward_io(
            _p(gb.view), _p(xb.view), _p(gtb.view), B, H * W, Cc, _p(gxb.view), _p(ggb.view), _p(ws.view), self.code(x.dtype),
            self.code(gate.dtype), self.stream()))
        assert gb.intact() and xb.intact() and gxb.intact() and gtb.intact() and ggb.intact() and ws.intact(), \
            ("se backward guards", x.shape, x.dtype, gate.dtype, off)
        return gxb.view.clone(), ggb.view.clone()


@pytest.fixture(scope="module")
def lib(amd):
    return Lib(amd)


def split_rows(M):
    """M rows as (B, H, W): one image, and B = M's smallest prime factor where it has one below M."""
    out = [(1, 1, M)]
    for b in (2, 3, 5):
        if M % b == 0:
            out.append((b, 1, M // b))
            break
    return out


# ---- bn_act --------------------------------------------------------------------------------------------------------------------
def check_bn(lib, T, shape, kind, seed, off=0):
    """All modes of bn_act on one shape and one kind of data: forward and backward against the yardstick, bit for bit."""
    ops = lib.ops
    B, H, W, Cc = shape
    M = B * H * W
    if kind == "special":
        x, g = special_rows(M, Cc, seed, T).reshape(shape), special_rows(M, Cc, seed + 2, T).reshape(shape)
    else:
        x, g = rnd(shape, seed, T, 2.0) + 0.5, rnd(shape, seed + 2, T)
    gamma, beta = rnd((Cc,), seed + 4, F32), rnd((Cc,), seed + 5, F32)
    if kind == "special":
        gamma[2], gamma[3], beta[3] = 3.0e4, 1.0, 0.0            # channel 2 overflows f16 behind SiLU; 3 keeps the subnormals
    g_pool = rnd((B, Cc), seed + 6, F32)
    rm0, rv0 = rnd((Cc,), seed + 7, F32), rnd((Cc,), seed + 8, F32).abs() + 0.5
    for training in (True, False):
        if training and M < 2:
            continue
        for silu in (True, False):
            for pooled in (False, True):
                what = (IDS[T], shape, kind, "train" if training else "eval", silu, pooled, off)
                rm, rv, rm_w, rv_w = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
                y, mean, invstd, pool = lib.bn_forward(x, gamma, beta, rm, rv, training, silu, pooled, off)
                w_y, w_mean, w_invstd, w_pool = ops.bn_act_train_forward(x.float(), gamma, beta, rm_w, rv_w, training, 0.1, 1e-5,
                                                                         silu, pooled)
                same(y, w_y.to(T), what + ("y",))
                same(mean, w_mean, what + ("mean",))
                same(invstd, w_invstd, what + ("invstd",))
                same(rm, rm_w, what + ("running_mean",))
                same(rv, rv_w, what + ("running_var",))
                if pooled:
                    same(pool, w_pool, what + ("pool",))
                if not training:
                    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
                gx, gg, gb = lib.bn_backward(g, x, mean, invstd, gamma, beta, training, silu, g_pool if pooled else None, off)
                w_gx, w_gg, w_gb = ops.bn_act_train_backward(g.float(), x.float(), w_mean, w_invstd, gamma, beta, training, silu,
                                                             g_pool if pooled else None)
                same(gx, w_gx.to(T), what + ("g_x",))
                same(gg, w_gg, what + ("g_gamma",))
                same(gb, w_gb, what + ("g_beta",))
                if kind == "random":
                    assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(gx.float()).all()), what
                elif Cc > 4:                                     # the plants of channels 1 .. 3 leave the others finite
                    assert bool(torch.isfinite(y.float()[..., 4:]).all()) and bool(torch.isfinite(gg[4:]).all()), what


@pytest.mark.parametrize("Cc", BN_C)
@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_bn_act_bit_for_bit(lib, T, Cc):
    seed = 100 * Cc
    for M in BN_M + ([BN_M_BIG] if Cc == 4 else []):
        for shape in split_rows(M):
            for kind in ("random", "special"):
                seed += 10
                check_bn(lib, T, shape + (Cc,), kind, seed)


# ---- dwconv --------------------------------------------------------------------------------------------------------------------
def dw_x_shape(mode, L, h, w):
    """The x extents of a case: the stride-2 conv reads an even image, twice the listed extents."""
    return (2 * h, 2 * w) if mode == L.DW_DOWN else (h, w)


def check_dw(lib, T, mode, shape, kind, seed, off=0):
    ops, L = lib.ops, lib.L
    B, H, W, Cc = shape
    Ho, Wo = ops._dw_out_shape(mode, H, W)
    k = 3 if mode == L.DW_SAME else 2
    make = special if kind == "special" else (lambda s, sd, dt: rnd(s, sd, dt))
    x, g = make(shape, seed, T), make((B, Ho, Wo, Cc), seed + 2, T)
    w = rnd((Cc, 1, k, k), seed + 4, F32)
    w_t = w.to(T).float()                                        # the taps as autocast casts them
    what = (IDS[T], mode, shape, kind, off)
    same(lib.dw_forward(x, w, mode, off), ops.dwconv_train_forward(x.float(), w_t, mode).to(T), what + ("y",))
    for need_x, need_w in ((True, True), (True, False), (False, True)):
        gx, gw = lib.dw_backward(g, x, w, mode, need_x, need_w, off)
        w_gx, w_gw = ops.dwconv_train_backward(g.float(), x.float(), w_t, mode, need_x, need_w)
        if need_x:
            same(gx, w_gx.to(T), what + ("g_x", need_w))
        if need_w:
            same(gw, w_gw, what + ("g_w", need_x))


@pytest.mark.parametrize("mode", ["same", "down", "up"])
@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_dwconv_bit_for_bit(lib, amd, T, mode):
    m = amd.train_mbconv.DW_MODES[mode]
    seed = 7000 + 1000 * m
    for e in DW_E:
        for h, w in DW_HW:
            H, W = dw_x_shape(m, lib.L, h, w)
            kinds = ("random", "special") if (e == 4 or h * w >= 255) else ("random",)
            for kind in kinds:
                seed += 10
                check_dw(lib, T, m, (2, H, W, e), kind, seed)
    if mode == "up":                                             # the OUTPUT pixels around the strip: 4 x 64 = 256, 260
        for w in (64, 65):
            check_dw(lib, T, m, (2, 1, w, 8), "random", seed + w)


@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_dwconv_on_integers_equals_fp64_conv(lib, amd, T):
    """x, g in -3 .. 3, taps in -2 .. 2: every output and data-gradient sum is at most 54 in magnitude, exact in bf16 and f16,
    and the weight gradient is an exact fp32 integer.  The references are torch's convs and their autograd in fp64 on the CPU:
    no kernel of this project."""
    L = lib.L
    for mode in (L.DW_SAME, L.DW_DOWN, L.DW_UP):
        for e, (h, w) in ((4, (3, 5)), (8, (1, 1)), (36, (2, 3)), (8, (1, 257))):
            H, W = dw_x_shape(mode, L, h, w)
            k = 3 if mode == L.DW_SAME else 2
            x = ints((2, H, W, e), 31 + e, T)
            wt = ints((e, 1, k, k), 32 + e, F32, -2, 2)
            x64 = x.double().cpu().permute(0, 3, 1, 2).requires_grad_()
            w64 = wt.double().cpu().requires_grad_()
            if mode == L.DW_SAME:
                y64 = F.conv2d(F.pad(x64, (1, 1, 1, 1), mode="circular"), w64, groups=e)
            elif mode == L.DW_DOWN:
                y64 = F.conv2d(x64, w64, stride=2, groups=e)
            else:
                y64 = F.conv_transpose2d(x64, w64, stride=2, groups=e)
            g = ints(tuple(y64.permute(0, 2, 3, 1).shape), 33 + e, T)
            gx64, gw64 = torch.autograd.grad(y64, [x64, w64], g.double().cpu().permute(0, 3, 1, 2))
            y = lib.dw_forward(x, wt, mode)
            gx, gw = lib.dw_backward(g, x, wt, mode, True, True)
            assert y.dtype == T and gx.dtype == T and gw.dtype == F32
            assert torch.equal(y.double().cpu(), y64.detach().permute(0, 2, 3, 1)), (IDS[T], mode, e, h, w)
            assert torch.equal(gx.double().cpu(), gx64.permute(0, 2, 3, 1)), (IDS[T], mode, e, h, w)
            assert torch.equal(gw.double().cpu(), gw64), (IDS[T], mode, e, h, w)


# ---- se_scale ------------------------------------------------------------------------------------------------------------------
def make_gate(B, Cc, seed, dtype):
    gate = torch.rand(B, Cc, generator=gen(seed))
    flat = gate.reshape(-1)
    for i, v in enumerate((0.0, -0.0, 1.0, 0.5, 2.0 ** -10, -0.25)[:flat.numel()]):
        flat[i] = v
    return gate.to(dtype).cuda()


@pytest.mark.parametrize("gate_T", [False, True], ids=["gate32", "gate16"])
@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_se_scale_bit_for_bit(lib, T, gate_T):
    """With special data: -0 x gate, f16-subnormal products and overflowing products must round as torch's cast of the fp32
    product does (the conversion pin of Io16::rnd)."""
    ops = lib.ops
    seed = 500
    for B, hw, Cc in SE_SHAPES:
        for kind in ("random", "special"):
            seed += 10
            shape = (B, 1, hw, Cc)
            make = special if kind == "special" else (lambda s, sd, dt: rnd(s, sd, dt))
            x, g = make(shape, seed, T), make(shape, seed + 2, T)
            gate = make_gate(B, Cc, seed + 4, T if gate_T else F32)
            what = (IDS[T], shape, kind, gate.dtype)
            same(lib.se_forward(x, gate), ops.se_scale_forward(x.float(), gate.float()).to(T), what + ("y",))
            gx, gg = lib.se_backward(g, x, gate)
            w_gx, w_gg = ops.se_scale_backward(g.float(), x.float(), gate.float())
            same(gx, w_gx.to(T), what + ("g_x",))
            same(gg, w_gg.to(gate.dtype), what + ("g_gate",))


def test_se_scale_signed_zero_and_subnormal_products(lib):
    """The case the pin exists for, spelt out: -0 x 0.5 stays -0, and an f16 product is the rounding of the fp32 product, not of
    the exact one."""
    T = torch.float16
    x = torch.tensor([-0.0, 0.0, 6.0e-8, -6.0e-8, 3.0e-5, 1.0009765625, -0.0, 5.0e-6], dtype=T).cuda().reshape(1, 1, 2, 4)
    gate = torch.tensor([0.5, -0.5, 0.5, 0.5], dtype=F32).cuda().reshape(1, 4) * torch.tensor(1.0009765625).cuda()
    y = lib.se_forward(x, gate)
    want = (x.float() * gate.reshape(1, 1, 1, 4)).to(T)
    same(y, want, "products")
    assert bool(torch.signbit(y.reshape(-1)[0])) and float(y.reshape(-1)[0]) == 0.0              # -0 x 0.5 = -0


# ---- memory: offsets, refusals, fp32 forwarding ---------------------------------------------------------------------------------
@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_views_8_bytes_off_a_16_byte_base(lib, T):
    """A 16-bit view 4 elements (8 bytes) past a 16-byte boundary is accepted and correct, for every node."""
    L = lib.L
    check_bn(lib, T, (3, 1, 171, 36), "random", 41, off=4)
    check_bn(lib, T, (1, 1, 257, 8), "special", 42, off=4)
    for mode in (L.DW_SAME, L.DW_DOWN, L.DW_UP):
        H, W = dw_x_shape(mode, L, 3, 5)
        check_dw(lib, T, mode, (2, H, W, 36), "random", 43 + mode, off=4)
    x, g = rnd((3, 1, 257, 36), 44, T), rnd((3, 1, 257, 36), 45, T)
    for gate, gate_off in ((make_gate(3, 36, 46, T), 4), (make_gate(3, 36, 46, F32), 0)):
        same(lib.se_forward(x, gate, 4, gate_off), lib.ops.se_scale_forward(x.float(), gate.float()).to(T), "se y")
        gx, gg = lib.se_backward(g, x, gate, 4, gate_off)
        w_gx, w_gg = lib.ops.se_scale_backward(g.float(), x.float(), gate.float())
        same(gx, w_gx.to(T), "se g_x")
        same(gg, w_gg.to(gate.dtype), "se g_gate")


@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_misaligned_views_and_mixed_types_are_refused(lib, T):
    """One element (2 bytes) off: VQAE_ERR_INVALID, nothing written.  bf16 beside f16: VQAE_ERR_UNSUPPORTED."""
    L = lib.L
    other = torch.float16 if T == torch.bfloat16 else torch.bfloat16
    x, g = rnd((2, 2, 3, 8), 51, T), rnd((2, 2, 3, 8), 52, T)
    v = rnd((8,), 53, F32)
    w = rnd((8, 1, 3, 3), 54, F32)
    st = torch.zeros(8, dtype=torch.float64, device="cuda")
    with pytest.raises(AssertionError, match="aligned"):
        lib.bn_forward(x, v, v, None, None, True, True, False, off=1)
    with pytest.raises(AssertionError, match="aligned"):
        lib.bn_backward(g, x, st, st, v, v, True, True, None, off=1)
    with pytest.raises(AssertionError, match="aligned"):
        lib.dw_forward(x, w, L.DW_SAME, off=1)
    with pytest.raises(AssertionError, match="aligned"):
        lib.dw_backward(g, x, w, L.DW_SAME, True, True, off=1)
    with pytest.raises(AssertionError, match="aligned"):
        lib.se_forward(x, make_gate(2, 8, 55, F32), off=1)
    with pytest.raises(AssertionError, match="aligned"):
        lib.se_backward(g, x, make_gate(2, 8, 55, T), off=0, gate_off=1)
    with pytest.raises(NotImplementedError, match="16-bit"):
        lib.se_forward(x, make_gate(2, 8, 55, other))
    with pytest.raises(NotImplementedError, match="16-bit"):
        lib.se_backward(g, x, make_gate(2, 8, 55, other))
    with pytest.raises(AssertionError, match="one dtype"):
        lib.ops.bn_act_train_backward_io(g.to(other), x, st, st, v, v, True)
    with pytest.raises(AssertionError, match="one dtype"):
        lib.ops.dwconv_train_backward_io(g.to(other), x, w, L.DW_SAME)
    torch.cuda.synchronize()


def test_all_fp32_io_calls_are_the_f32_entries(lib):
    ops, L = lib.ops, lib.L
    x, g = rnd((3, 1, 257, 36), 61, F32, 2.0), rnd((3, 1, 257, 36), 62, F32)
    gamma, beta, g_pool = rnd((36,), 63, F32), rnd((36,), 64, F32), rnd((3, 36), 65, F32)
    rm, rv, rm_w, rv_w = (torch.zeros(36, device="cuda"), torch.ones(36, device="cuda"), torch.zeros(36, device="cuda"),
                          torch.ones(36, device="cuda"))
    got = ops.bn_act_train_forward_io(x, gamma, beta, rm, rv, True, 0.1, 1e-5, True, True)
    want = ops.bn_act_train_forward(x, gamma, beta, rm_w, rv_w, True, 0.1, 1e-5, True, True)
    for k, (p, q) in enumerate(zip(got + (rm, rv), want + (rm_w, rv_w))):
        same(p, q, ("bn forward", k))
    for p, q in zip(ops.bn_act_train_backward_io(g, x, got[1], got[2], gamma, beta, True, True, g_pool),
                    ops.bn_act_train_backward(g, x, got[1], got[2], gamma, beta, True, True, g_pool)):
        same(p, q, "bn backward")
    y = lib.bn_forward(x, gamma, beta, None, None, True, True, False)[0]          # and through the banded ctypes path
    same(y, want[0], "bn forward, banded")
    for mode, k, xs in ((L.DW_SAME, 3, (2, 3, 5, 36)), (L.DW_DOWN, 2, (2, 6, 10, 36)), (L.DW_UP, 2, (2, 3, 5, 36))):
        xd, w = rnd(xs, 66, F32), rnd((36, 1, k, k), 67, F32)
        yd = ops.dwconv_train_forward_io(xd, w, mode)
        same(yd, ops.dwconv_train_forward(xd, w, mode), ("dw forward", mode))
        gd = rnd(tuple(yd.shape), 68, F32)
        for p, q in zip(ops.dwconv_train_backward_io(gd, xd, w, mode), ops.dwconv_train_backward(gd, xd, w, mode)):
            same(p, q, ("dw backward", mode))
    gate = make_gate(3, 36, 69, F32)
    same(ops.se_scale_forward_io(x, gate), ops.se_scale_forward(x, gate), "se forward")
    for p, q in zip(ops.se_scale_backward_io(g, x, gate), ops.se_scale_backward(g, x, gate)):
        same(p, q, "se backward")


@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_wrappers_run_to_run(lib, T):
    """ops.*_io (the path the Functions take): two runs give the same bits, and the bits of the banded calls above."""
    ops, L = lib.ops, lib.L
    x, g = special_rows(3 * 257, 36, 71, T).reshape(3, 1, 257, 36), rnd((3, 1, 257, 36), 72, T)
    gamma, beta, g_pool = rnd((36,), 73, F32), rnd((36,), 74, F32), rnd((3, 36), 75, F32)
    w3, w2 = rnd((36, 1, 3, 3), 76, F32), rnd((36, 1, 2, 2), 77, F32)
    xq, gq = rnd((2, 6, 10, 36), 78, T), rnd((2, 3, 5, 36), 79, T)

    def run():
        rm, rv = torch.zeros(36, device="cuda"), torch.ones(36, device="cuda")
        y, mean, invstd, pool = ops.bn_act_train_forward_io(x, gamma, beta, rm, rv, True, 0.1, 1e-5, True, True)
        out = [y, mean, invstd, pool, rm, rv]
        out += ops.bn_act_train_backward_io(g, x, mean, invstd, gamma, beta, True, True, g_pool)
        out += [ops.dwconv_train_forward_io(x, w3, L.DW_SAME), ops.dwconv_train_forward_io(xq, w2, L.DW_DOWN),
                ops.dwconv_train_forward_io(gq, w2, L.DW_UP)]
        out += ops.dwconv_train_backward_io(g, x, w3, L.DW_SAME) + ops.dwconv_train_backward_io(gq, xq, w2, L.DW_DOWN)
        out += ops.dwconv_train_backward_io(xq, gq, w2, L.DW_UP)
        for gate in (make_gate(3, 36, 80, F32), make_gate(3, 36, 80, T)):
            out += [ops.se_scale_forward_io(x, gate)] + list(ops.se_scale_backward_io(g, x, gate))
        return out

    first, second = run(), run()
    for k, (p, q) in enumerate(zip(first, second)):
        same(p, q, ("run to run", k))
    assert first[0].dtype == T and first[3].dtype == F32 and first[6].dtype == T and first[7].dtype == F32
    rm, rv = torch.zeros(36, device="cuda"), torch.ones(36, device="cuda")
    banded = lib.bn_forward(x, gamma, beta, rm, rv, True, True, True)
    for k, (p, q) in enumerate(zip(first[:4], banded)):
        same(p, q, ("wrapper against banded", k))


# ---- blocks and the step under autocast -----------------------------------------------------------------------------------------
def results(block, x, g, forward):
    """mbconv_train_cases.block_results with the upstream gradient cast to the output's dtype (16-bit under autocast)."""
    x = x.detach().clone().requires_grad_()
    params = dict(block.named_parameters())
    y = forward(block, x)
    grads = torch.autograd.grad(y, [x] + list(params.values()), g.to(y.dtype))
    res = {"out": y.detach(), "input": grads[0]}
    res.update(dict(zip(params, grads[1:])))
    bnames = [k for k in block.state_dict() if k.endswith(("running_mean", "running_var"))]
    res.update({k: block.state_dict()[k].detach().clone() for k in bnames})
    assert all(res[k].dtype == F32 for k in list(params) + bnames), "parameter gradients and running statistics are fp32"
    return C.result_groups({k: v.float() for k, v in res.items()}, list(params), bnames)


@pytest.mark.parametrize("case", C.block_cases())
@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_block_parity_under_autocast(amd, T, case, monkeypatch):
    from vqae_amd.layers.mbconv_train import MBConv
    Tm = amd.train_mbconv

    def under(forward):
        def run(blk, t):
            with torch.autocast("cuda", dtype=T):
                return forward(blk, t)
        return run

    block, x, g, ref = C.block_case(case, MBConv, device="cuda")
    stock = results(block, x, g, under(Tm.block_forward_torch))
    block, x, g, ref = C.block_case(case, MBConv, device="cuda")
    node_out, saved = [], []
    for name in ("bn_act", "dwconv", "se_scale"):
        def wrap(*a, _f=getattr(Tm, name), _n=name, **k):
            out = _f(*a, **k)
            node_out.append((_n, a[0].dtype, (out[0] if isinstance(out, tuple) else out).dtype))
            return out
        monkeypatch.setattr(Tm, name, wrap)
    before = dict(Tm.stats, **Tm.io16_stats)
    leaf = lambda t: t.is_leaf and t.requires_grad                        # the parameters and the input: fp32 by design
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append((t.dim(), t.dtype, leaf(t))), t)[1], lambda t: t):
        got = results(block, x.contiguous(memory_format=torch.channels_last), g, under(Tm.block_forward))
    torch.cuda.synchronize()
    delta = {k: v - before[k] for k, v in dict(Tm.stats, **Tm.io16_stats).items()}
    small_bn = 1 if block.branch[8].num_features % 4 else 0               # the 3-channel BatchNorm of the 'out' block
    assert delta["bn_fallbacks"] == small_bn and delta["io16_fallbacks"] == small_bn and delta["dwconv_fallbacks"] == 0
    assert delta["io16_hip"] == 5 - small_bn and delta["bn_hip"] == 3 - small_bn and delta["dwconv_hip"] == 1
    assert [n for n, *_ in node_out] == ["bn_act", "dwconv", "bn_act", "se_scale", "bn_act"]
    assert all(din == T and dout == T for _, din, dout in node_out), node_out
    acts = [dt for dim, dt, is_leaf in saved if dim == 4 and not is_leaf]
    assert len(acts) >= 8 and all(dt == T for dt in acts), saved           # every saved activation is 16-bit
    assert set(got) == set(ref)
    fails = []
    for k, (v64, _) in ref.items():
        e_dev, e_ref = C.dist(got[k], v64.reshape(got[k].shape)), C.dist(stock[k], v64.reshape(stock[k].shape))
        print(f"mbconv_train16_block {IDS[T]} {case} {k}: e_dev {e_dev:.3e} e_ref {e_ref:.3e} ratio {e_dev / e_ref:.3f}")
        record_parity("mbconv_train16_block", dtype=IDS[T], case=case, tensor=k, e_dev=e_dev, e_ref_stock_autocast=e_ref,
                      ratio=e_dev / e_ref)
        assert bool(torch.isfinite(got[k]).all())
        if not e_dev <= BAR * e_ref:
            fails.append((k, e_dev, e_ref))
    assert not fails, fails


@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_target_module_gives_block_forward_bits(amd, T):
    from vqae_amd.layers.mbconv_train import MBConv
    Tm = amd.train_mbconv
    for case in C.block_cases():
        block, x, _, _ = C.block_case(case, MBConv, device="cuda")
        twin, _, _, _ = C.block_case(case, MBConv, device="cuda")
        x = x.contiguous(memory_format=torch.channels_last)
        with torch.autocast("cuda", dtype=T):
            y_mod, y_fn = block(x), Tm.block_forward(twin, x)
            y16 = block(x.to(T))
        same(y_mod, y_fn, (case, "module against block_forward"))
        assert y16.dtype == T                                               # a 16-bit residual stream stays 16-bit
        for (k, p), (_, q) in zip(block.state_dict().items(), twin.state_dict().items()):
            if k.endswith(("running_mean", "running_var")):
                assert p.dtype == F32 and not torch.equal(p, q)             # block ran twice, twin once
    torch.cuda.synchronize()


@pytest.mark.parametrize("T", T16, ids=IDS.get)
def test_whole_step_under_autocast(amd, T):
    """One train_mbconv.step + backward + FusedAdamW on spec tinyM, batch 2, 32 x 32: bf16 as it is, f16 with a GradScaler."""
    from vqae_amd.layers.conv_block import MBConv as Mirror
    Tm, ops = amd.train_mbconv, amd.ops
    model, batches = C.loop_model(device="cuda")
    x = batches[0].contiguous(memory_format=torch.channels_last)
    opt = amd.FusedAdamW(model.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10, enabled=T == torch.float16)
    blocks = [m for m in model.modules() if isinstance(m, Mirror)]
    n_se = sum(1 for b in blocks if ops.bn_act_train_supported(b.expanded))
    stats0 = {k: v.detach().clone() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    before = dict(Tm.stats, **Tm.io16_stats)
    with torch.autocast("cuda", dtype=T):
        out, recon, vq_losses = Tm.step(model, x)
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
    now = model.state_dict()
    assert stats0 and all(now[k].dtype == F32 and not torch.equal(now[k], v) for k, v in stats0.items())
    delta = {k: v - before[k] for k, v in dict(Tm.stats, **Tm.io16_stats).items()}
    assert len(blocks) > 0 and delta["bn_hip"] + delta["bn_fallbacks"] == 3 * len(blocks)
    assert delta["io16_hip"] == delta["bn_hip"] + delta["dwconv_hip"] + n_se             # every fused node ran a 16-bit form
    assert delta["io16_fallbacks"] == delta["bn_fallbacks"] + delta["dwconv_fallbacks"] + (len(blocks) - n_se)
    record_parity("mbconv_train16_step", dtype=IDS[T], recon=float(recon.detach()), vq=float(vq_losses[0].detach()),
                  grads_finite=finite, io16_hip=delta["io16_hip"], io16_fallbacks=delta["io16_fallbacks"])
