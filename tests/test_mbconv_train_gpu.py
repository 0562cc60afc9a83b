"""GPU: the fused HIP nodes of the MBConv training path (csrc/mbconv_train.hip behind vqae_amd.train_mbconv).

  * bn_act against torch's F.batch_norm + F.silu in fp64 at the edges of its reduction geometry (R rows per workgroup, FIN
    partial rows per lane of the finishing launch), inside 4 x the distance of fp32 torch on the same inputs; a constant input;
    eval mode;
  * dwconv exact on integer data in all three modes at the small extents and around the strip of R output pixels, and inside
    the bar on random data; se_scale;
  * no node writes outside its outputs (guard bands around every buffer the op wrappers allocate);
  * two runs give the same bits: each node, and a whole tinyM step + backward;
  * the fixture's block cases and closed loop (tests/golden/mbconv_train.npz) inside the bar, the loop's codes exactly;
  * the trainable module layers.mbconv_train.MBConv.
"""
import contextlib
import copy

import pytest
import torch
import torch.nn.functional as F

import mbconv_train_cases as C
from conftest import record_parity

pytestmark = pytest.mark.gpu
BAR = 4.0
DEV = "cuda"


def _check(test, tag, got, r32, r64):
    """got, r32, r64: {name: tensor}; every group inside BAR x fp32 torch's own distance to the fp64 result.  The groups are
    those of mbconv_train_cases.grouped: a tensor of fewer than 8 numbers (the per-channel results at C = 4) joins the case's
    vector "small", because the distance of a few fp32 numbers to their fp64 values is chance and no yardstick."""
    got, r32, r64 = ({k: v.detach() for k, v in C.grouped(d).items()} for d in (got, r32, r64))
    for k, v64 in r64.items():
        e, e_ref = C.dist(got[k], v64), C.dist(r32[k], v64)
        record_parity(test, case=tag, tensor=k, e=e, e_ref=e_ref, ratio=e / e_ref if e_ref else None)
        assert torch.isfinite(got[k]).all(), (tag, k)
        assert e <= BAR * e_ref, (tag, k, e, e_ref)


# ---- bn_act --------------------------------------------------------------------------------------------------------------
def _bn_inputs(B, H, W, Cc, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    return dict(x=(1.5 * r(B, H, W, Cc) + 0.5), gamma=0.5 + torch.rand(Cc, generator=gen), beta=0.3 * r(Cc),
                rm=0.3 * r(Cc), rv=0.5 + torch.rand(Cc, generator=gen), g=r(B, H, W, Cc), gp=r(B, Cc))


def _bn_torch(inp, dtype, training, silu, momentum=0.1, eps=1e-5):
    """F.batch_norm (+ F.silu) and autograd on the device in `dtype` -> the seven results.  The yardstick sees a plain contiguous
    NCHW tensor, torch's default layout: a permuted [1, C, H, 1] view has strides that read as either memory format."""
    t = {k: v.to(DEV, dtype) for k, v in inp.items()}
    x, ga, be = (t[k].requires_grad_() for k in ("x", "gamma", "beta"))
    y = F.batch_norm(x.permute(0, 3, 1, 2).contiguous(), t["rm"], t["rv"], ga, be, training, momentum, eps).permute(0, 2, 3, 1)
    y = F.silu(y) if silu else y
    pool = y.sum((1, 2))
    g_x, g_ga, g_be = torch.autograd.grad([y, pool], [x, ga, be], [t["g"], t["gp"]])
    return dict(y=y.detach(), pool=pool.detach(), g_x=g_x, g_gamma=g_ga, g_beta=g_be, running_mean=t["rm"], running_var=t["rv"])


def _bn_ours(amd, inp, training, silu, momentum=0.1, eps=1e-5):
    t = {k: v.to(DEV) for k, v in inp.items()}
    x, ga, be = (t[k].requires_grad_() for k in ("x", "gamma", "beta"))
    y, pool = amd.train_mbconv._BnActFn.apply(x, ga, be, t["rm"], t["rv"], training, momentum, eps, silu, True)
    g_x, g_ga, g_be = torch.autograd.grad([y, pool], [x, ga, be], [t["g"], t["gp"]])
    return dict(y=y.detach(), pool=pool.detach(), g_x=g_x, g_gamma=g_ga, g_beta=g_be, running_mean=t["rm"], running_var=t["rv"])


def _bn_shapes(amd):
    """[B, H, W] with M = B H W rows at the edges of the reduction geometry.  R: the rows one workgroup reduces in the statistics
    pass (and the pixels of one strip of the pooled pass); FIN: the partial rows one lane of the finishing launch adds are
    FIN apart, so FIN R + 1 rows are the first M at which a lane adds two."""
    R, FIN = amd._lib.MBT_ROWS, amd._lib.MBT_FIN_LANES
    assert (R, FIN) == (256, 64)
    shapes = [(2, 1, 1), (3, 1, 1), (3, 5, 17), (2, 8, 16), (1, 257, 1), (3, 9, 19), (5, 29, 113)]
    assert [b * h * w for b, h, w in shapes] == [2, 3, R - 1, R, R + 1, 2 * R + 1, FIN * R + 1]
    return shapes


@pytest.mark.parametrize("channels", [4, 8, 36, 260])
def test_bn_act_training_against_fp64(amd, channels):
    for B, H, W in _bn_shapes(amd):
        for silu in (False, True):
            inp = _bn_inputs(B, H, W, channels, seed=B * H * W + channels + silu)
            r64, r32 = _bn_torch(inp, torch.float64, True, silu), _bn_torch(inp, torch.float32, True, silu)
            got = _bn_ours(amd, inp, True, silu)
            _check("mbconv_train_bn_act", f"C{channels}_M{B * H * W}_{'silu' if silu else 'id'}", got, r32, r64)


@pytest.mark.parametrize("channels", [4, 36])
def test_bn_act_eval_mode(amd, channels):
    """Eval mode: the running statistics normalise, inside the bar, and both buffers keep their bits."""
    for B, H, W in ((3, 1, 1), (3, 9, 19)):
        inp = _bn_inputs(B, H, W, channels, seed=17 + channels)
        r64, r32 = _bn_torch(inp, torch.float64, False, True), _bn_torch(inp, torch.float32, False, True)
        got = _bn_ours(amd, inp, False, True)
        for k in ("running_mean", "running_var"):
            assert torch.equal(got.pop(k).cpu(), inp["rm" if k == "running_mean" else "rv"]), k
            r32.pop(k), r64.pop(k)
        _check("mbconv_train_bn_act_eval", f"C{channels}_M{B * H * W}", got, r32, r64)


def test_bn_act_constant_input(amd):
    """Variance 0 (every channel a constant): finite, and torch's result.  x - mean is exactly 0, so y = act(beta) and the blended
    running mean are single roundings (two ulps: torch blends with momentum in fp32, the kernel in fp64); pool and g_beta are
    sums of M = R + 1 terms, equal to M 2^-24 of their size; g_gamma = sum d xhat is exactly 0 with xhat = 0.
    torch's OWN fp32 variance of a constant is not 0 (measured on the MI355X: 1.7e-5 at x = 25.9, a third of an ulp of x^2 = 670:
    the rounding of E[x^2] - mean^2), so its running variance is off by momentum times that, and its invstd -- hence its g_x -- is
    that rounding noise against eps = 1e-5: the running variance is compared with torch's within momentum x 4 ulps of x^2 and
    with torch's fp64 result to two ulps, and g_x with the fp64 result, whose variance is 0 to 1e-13."""
    R = amd._lib.MBT_ROWS
    inp = _bn_inputs(1, R + 1, 1, 8, seed=5)
    inp["x"] = torch.full_like(inp["x"], 3.7) * torch.arange(1, 9)
    for silu in (False, True):
        want, got = _bn_torch(inp, torch.float32, True, silu), _bn_ours(amd, inp, True, silu)
        exact = _bn_torch(inp, torch.float64, True, silu)
        for k, v in got.items():
            assert torch.isfinite(v).all(), k
        for k in ("y", "running_mean"):
            torch.testing.assert_close(got[k], want[k], rtol=2 * 2.0 ** -23, atol=0)
        torch.testing.assert_close(got["running_var"], want["running_var"], rtol=2 * 2.0 ** -23,
                                   atol=0.1 * 4 * 2.0 ** -23 * float(inp["x"].max()) ** 2)
        torch.testing.assert_close(got["running_var"], exact["running_var"].float(), rtol=2 * 2.0 ** -23, atol=0)
        for k in ("pool", "g_beta"):
            torch.testing.assert_close(got[k], want[k], rtol=(R + 1) * 2.0 ** -24, atol=(R + 1) * 2.0 ** -24)
        assert float(got["g_gamma"].abs().max()) == 0.0
        assert C.dist(got["g_x"], exact["g_x"]) <= 1e-5


def test_bn_act_refusals_and_fallback(amd):
    T = amd.train_mbconv
    bn = torch.nn.BatchNorm2d(8).to(DEV).train()
    with pytest.raises(ValueError):
        T.bn_act(torch.zeros(1, 1, 1, 8, device=DEV), bn)
    before = dict(T.stats)
    bn3 = torch.nn.BatchNorm2d(3).to(DEV).train()
    x = torch.randn(2, 4, 4, 3, device=DEV, requires_grad=True)
    y = T.bn_act(x, bn3)
    y.sum().backward()
    want = torch.nn.BatchNorm2d(3).to(DEV).train()(x.detach().permute(0, 3, 1, 2).contiguous()).permute(0, 2, 3, 1)
    torch.testing.assert_close(y.detach(), want, rtol=1e-5, atol=1e-5)
    assert T.stats["bn_fallbacks"] == before["bn_fallbacks"] + 1 and T.stats["bn_hip"] == before["bn_hip"]
    assert int(bn3.num_batches_tracked) == 1 and not amd.ops.bn_act_train_supported(3)


# ---- dwconv --------------------------------------------------------------------------------------------------------------
def _dw_torch(x, w, g, mode):
    """F.conv2d(groups=) / F.conv_transpose2d and autograd -> (y, g_x, g_w), NHWC."""
    x, w = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    xc, e = x.permute(0, 3, 1, 2), x.shape[-1]
    if mode == "same":
        y = F.conv2d(F.pad(xc, (1, 1, 1, 1), mode="circular"), w, groups=e)
    elif mode == "down":
        y = F.conv2d(xc, w, stride=2, groups=e)
    else:
        y = F.conv_transpose2d(xc, w, stride=2, groups=e)
    y = y.permute(0, 2, 3, 1)
    g_x, g_w = torch.autograd.grad(y, [x, w], g)
    return dict(y=y.detach(), g_x=g_x, g_w=g_w)


def _dw_ours(amd, x, w, g, mode):
    x, w = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    y = amd.train_mbconv.dwconv(x, w, mode)
    g_x, g_w = torch.autograd.grad(y, [x, w], g)
    return dict(y=y.detach(), g_x=g_x, g_w=g_w)


def _dw_case(mode, B, H, W, e, seed, integers):
    gen = torch.Generator().manual_seed(seed)
    k = 3 if mode == "same" else 2
    Ho, Wo = {"same": (H, W), "down": (H // 2, W // 2), "up": (2 * H, 2 * W)}[mode]
    if integers:
        draw = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
        return draw(-3, 3, B, H, W, e), draw(-2, 2, e, 1, k, k), draw(-3, 3, B, Ho, Wo, e)
    return torch.randn(B, H, W, e, generator=gen), torch.randn(e, 1, k, k, generator=gen), torch.randn(B, Ho, Wo, e, generator=gen)


# The kernels walk strips of R = 256 pixels (of the output; the weight gradient of "up" of the input): one pixel count below,
# at and above the strip, besides every H, W of {1, 2, 3, 5} (doubled for the stride-2 mode, which needs even extents).
SMALL = [(h, w) for h in (1, 2, 3, 5) for w in (1, 2, 3, 5)]
DW_EXTENTS = {"same": SMALL + [(15, 17), (16, 16), (1, 257), (257, 1)],
              "down": [(2 * h, 2 * w) for h, w in SMALL] + [(30, 34), (32, 32), (2, 514)],
              "up": SMALL + [(7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (1, 257)]}


@pytest.mark.parametrize("mode", ["same", "down", "up"])
@pytest.mark.parametrize("e", [4, 8, 36])
def test_dwconv_exact_on_integers(amd, mode, e):
    """Small integers in x, w and g: every fp32 sum is exact, so forward, data gradient and weight gradient equal the fp64 ones."""
    before = amd.train_mbconv.stats["dwconv_hip"]
    for i, (H, W) in enumerate(DW_EXTENTS[mode]):
        x, w, g = (t.to(DEV) for t in _dw_case(mode, 2, H, W, e, seed=100 * e + i, integers=True))
        want = _dw_torch(x.double(), w.double(), g.double(), mode)
        got = _dw_ours(amd, x, w, g, mode)
        for k in want:
            assert got[k].shape == want[k].shape and torch.equal(got[k].double(), want[k]), (mode, e, H, W, k)
    assert amd.train_mbconv.stats["dwconv_hip"] == before + len(DW_EXTENTS[mode])


@pytest.mark.parametrize("mode", ["same", "down", "up"])
def test_dwconv_random_inside_the_bar(amd, mode):
    for e, (H, W) in ((8, (6, 10)), (36, (18, 30))):
        x, w, g = (t.to(DEV) for t in _dw_case(mode, 3, H, W, e, seed=e, integers=False))
        r64, r32 = _dw_torch(x.double(), w.double(), g.double(), mode), _dw_torch(x, w, g, mode)
        _check("mbconv_train_dwconv", f"{mode}_e{e}_{H}x{W}", _dw_ours(amd, x, w, g, mode), r32, r64)


def test_dwconv_fallback_route(amd):
    """Odd extents under stride 2 and a channel count outside the rule take F.conv2d / F.conv_transpose2d, and are counted."""
    T = amd.train_mbconv
    before = dict(T.stats)
    for mode, shape in (("down", (1, 5, 4, 8)), ("up", (1, 2, 3, 6))):
        x, w, g = (t.to(DEV) for t in _dw_case(mode, *shape[:3], shape[3], seed=1, integers=True))
        want, got = _dw_torch(x, w, g, mode), _dw_ours(amd, x, w, g, mode)
        for k in want:
            assert torch.equal(got[k], want[k]), (mode, k)
    assert T.stats["dwconv_fallbacks"] == before["dwconv_fallbacks"] + 2 and T.stats["dwconv_hip"] == before["dwconv_hip"]


# ---- se_scale ------------------------------------------------------------------------------------------------------------
def _se_case(B, H, W, c, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, W, c, generator=gen).to(DEV), torch.rand(B, c, generator=gen).to(DEV),
            torch.randn(B, H, W, c, generator=gen).to(DEV))


def _se(fn, x, gate, g):
    x, gate = x.detach().clone().requires_grad_(), gate.detach().clone().requires_grad_()
    y = fn(x, gate)
    g_x, g_gate = torch.autograd.grad(y, [x, gate], g)
    return dict(y=y.detach(), g_x=g_x, g_gate=g_gate)


@pytest.mark.parametrize("channels", [4, 36, 260])
def test_se_scale(amd, channels):
    stock = lambda x, gate: x * gate.reshape(gate.shape[0], 1, 1, -1)
    for B, H, W in ((2, 1, 1), (3, 15, 17), (2, 16, 16), (2, 1, 257), (2, 64, 257)):
        x, gate, g = _se_case(B, H, W, channels, seed=channels + H)
        r64, r32 = _se(stock, x.double(), gate.double(), g.double()), _se(stock, x, gate, g)
        got = _se(amd.train_mbconv.se_scale, x, gate, g)
        assert torch.equal(got["y"], r32["y"]) and torch.equal(got["g_x"], r32["g_x"])      # one product each
        _check("mbconv_train_se_scale", f"C{channels}_{B}x{H}x{W}", {"g_gate": got["g_gate"]}, r32, {"g_gate": r64["g_gate"]})


# ---- guard bands ---------------------------------------------------------------------------------------------------------
GUARD = 64


class _GuardedTorch:
    """Stands in for the `torch` module inside vqae_amd.ops: every buffer the op wrappers allocate (outputs, gradients,
    workspaces) lies between two bands of a sentinel."""

    def __init__(self):
        self.bands = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=torch.float32, device=None):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(int(s) for s in size)
        n = 1
        for s in shape:
            n *= int(s)
        sentinel = 0xA5 if dtype == torch.uint8 else -777.25
        full = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=device)
        self.bands.append((full, n, sentinel))
        return full[GUARD:GUARD + n].view(shape)

    def empty_like(self, t):
        return self.empty(tuple(t.shape), dtype=t.dtype, device=t.device)

    def intact(self):
        return all(bool((full[:GUARD] == s).all()) and bool((full[GUARD + n:] == s).all()) for full, n, s in self.bands)


@contextlib.contextmanager
def _guarded(amd):
    stand_in = _GuardedTorch()
    real, amd.ops.torch = amd.ops.torch, stand_in
    try:
        yield stand_in
    finally:
        amd.ops.torch = real


def test_no_write_outside_the_outputs(amd):
    with _guarded(amd) as guard:
        for channels, (B, H, W) in ((4, (2, 1, 1)), (36, (2, 5, 3)), (260, (1, 17, 16)), (8, (3, 16, 16))):
            for training in (True, False):
                _bn_ours(amd, _bn_inputs(B, H, W, channels, seed=3), training, True)
            for mode in ("same", "down", "up"):
                h, w = (2 * H, 2 * W) if mode == "down" else (H, W)
                x, wt, g = (t.to(DEV) for t in _dw_case(mode, B, h, w, channels, seed=4, integers=False))
                _dw_ours(amd, x, wt, g, mode)
            _se(amd.train_mbconv.se_scale, *_se_case(B, H, W, channels, seed=5))
        torch.cuda.synchronize()
        # per shape: 2 x (4 forward + 3 backward) of bn_act, 3 x (1 + 3) of dwconv, 1 + 3 of se_scale
        assert len(guard.bands) == 4 * (2 * 7 + 3 * 4 + 4) and guard.intact()


# ---- run to run ----------------------------------------------------------------------------------------------------------
def _equal(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_nodes_bit_identical_run_to_run(amd):
    inp = _bn_inputs(5, 29, 113, 36, seed=9)
    assert _equal(_bn_ours(amd, inp, True, True), _bn_ours(amd, inp, True, True))
    for mode in ("same", "down", "up"):
        x, w, g = (t.to(DEV) for t in _dw_case(mode, 3, 34, 30, 36, seed=2, integers=False))
        assert _equal(_dw_ours(amd, x, w, g, mode), _dw_ours(amd, x, w, g, mode)), mode
    case = _se_case(3, 33, 31, 36, seed=8)
    assert _equal(_se(amd.train_mbconv.se_scale, *case), _se(amd.train_mbconv.se_scale, *case))


def test_step_bit_identical_run_to_run(amd):
    """Two runs of a whole tinyM step + backward: the output, the running statistics and the gradients the three new nodes
    produce (BatchNorm weights and biases, the depthwise weights; the SE Linears' follow from pool and g_gate) -- the dense convs'
    own weight gradients are MIOpen's and not part of the claim.  MIOpen's default choice for the dense 1x1 conv 128 -> 32 on
    2 x 8 x 8 does not repeat its own FORWARD bits (measured: the first op of a step to differ between two runs, every op
    before it equal), so the step runs under torch.backends.cudnn.deterministic, which pins the dense convs' algorithms."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        _step_twice(amd)
    finally:
        torch.backends.cudnn.deterministic = was


def _step_twice(amd):
    def run():
        model, batches = C.loop_model(DEV)
        x = batches[0].contiguous(memory_format=torch.channels_last)
        out, recon, (vq_loss,) = amd.train_mbconv.step(model, x)
        (recon + vq_loss).backward()
        res = {"out": out.detach()}
        for k, p in model.named_parameters():
            if ".branch.1." in k or ".branch.4." in k or ".branch.8." in k or ".branch.3." in k:
                res["grad:" + k] = p.grad
        res.update({k: v for k, v in model.state_dict().items() if "running_" in k})
        return res
    a, b = run(), run()
    assert len(a) > 100 and _equal(a, b), [k for k in a if not torch.equal(a[k], b[k])]


# ---- the fixture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.block_cases())
def test_block_forward_matches_reference(amd, case):
    from vqae_amd.layers.mbconv_train import MBConv
    T = amd.train_mbconv
    block, x, g, ref = C.block_case(case, MBConv, DEV)
    x = x.contiguous(memory_format=torch.channels_last)
    before = dict(T.stats)
    got = C.block_results(block, x, g, T.block_forward)
    assert set(got) == set(ref)
    for k, (v64, e_ref) in ref.items():
        e = C.dist(got[k], v64)
        record_parity("mbconv_train_block", case=case, tensor=k, e=e, e_ref=e_ref, ratio=e / e_ref)
        assert e <= BAR * e_ref, (case, k, e, e_ref)
    took = {k: T.stats[k] - before[k] for k in before}
    out3 = case.startswith("outskip")                      # the 3-channel last BatchNorm takes the torch restatement
    assert took == {"bn_hip": 2 if out3 else 3, "bn_fallbacks": 1 if out3 else 0, "dwconv_hip": 1, "dwconv_fallbacks": 0}, took


def test_closed_loop_reproduces_fixture(amd):
    same, losses, groups = C.closed_loop(amd, DEV)
    assert all(same), same
    e, e_ref = C.loss_distances(losses)
    record_parity("mbconv_train_loop", tensor="losses", e=e, e_ref=e_ref, ratio=e / e_ref)
    assert e <= BAR * e_ref, (e, e_ref)
    for tag, (got, want, e32) in groups.items():
        e = C.dist(got, want)
        record_parity("mbconv_train_loop", tensor=tag, e=e, e_ref=e32, ratio=e / e32)
        assert e <= BAR * e32, (tag, e, e32)


def test_trainable_module(amd):
    """layers.mbconv_train.MBConv loads a reference state dict by its own names (block_case asserts the names), equals the
    inference mirror bit for bit in .eval() under no_grad, and trains in .train()."""
    from vqae_amd.layers.conv_block import MBConv as Mirror
    from vqae_amd.layers.mbconv_train import MBConv
    block, x, g, _ = C.block_case("down_8_16_4x6", MBConv, DEV)
    mirror = Mirror(8, 16, "down", **C.block_kwargs()).to(DEV)
    mirror.load_state_dict(block.state_dict())
    with torch.no_grad():
        assert torch.equal(block.eval()(x), mirror.eval()(x))
    y = block.train()(x)
    assert y.requires_grad and y.shape == (2, 16, 2, 3)
    y.backward(g)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in block.parameters())
    with torch.no_grad():                                   # the running statistics moved: the inference form follows them
        mirror.load_state_dict(block.state_dict())
        assert torch.equal(block.eval()(x), mirror.eval()(x))
    with pytest.raises(NotImplementedError):
        mirror.train()(x)
    twin = copy.deepcopy(block).train()
    want = amd.train_mbconv.block_forward_torch(twin, x)
    torch.testing.assert_close(block.train()(x), want, rtol=1e-4, atol=1e-5)
