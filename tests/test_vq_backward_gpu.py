"""GPU: the backward of both quantiser mirrors (csrc/vq_backward.hip behind vqae_amd.layers.vq's autograd Functions).

Parity bar, per gradient tensor, against the reference's own autograd (tests/golden/vq_backward.npz):
    ||hip - g64|| / ||g64||  <=  4 x ||g32 - g64|| / ||g64||
g32 / g64 being the reference's fp32 and fp64 runs on the same inputs with the same indices: the project's margin for device
code that sums the same products in another order (test_classifier_train_gpu.py).

Shape bar, against projected_backward_reference / backward_reference in fp64 on the device, element by element, from the
kernel's arithmetic alone (u = 2^-24, nothing measured).  M_z = |g_out| |W_out| + |s| |z - q| bounds the terms of g_z:
    g_z      (4 S + 8) u M_z     a lane's 4 S-term fma chain (S = 1 slab for C <= 128, 2 above), 5 levels of cross-lane adds,
                                 then the rounding of s, of z - q, of the product and of the sum
    g_x      (4 S + 16) u M_z |W_in|                       g_z's error through an 8-term fma chain
    g_W_in, g_b_in   (4 S + 9) u sum_n M_z |x|  (|x| = 1 for the bias): fp32 g_z, exact products, fp64 sums, one rounding
    g_W_out, g_b_out 2 u sum_n |g_out| |q|      exact products summed in fp64, rounded to fp32 once
    plain    4 u (|g_out| + |s| |x - q|)"""
import copy

import pytest
import torch
from torch import nn

from conftest import record_parity
from test_vq_backward_cpu import (GRAD_NAMES, PLAIN, PROJ4, PROJ8, PROJ16, bfx, load_case, projected_inputs, rel, rows,  # noqa: F401
                                  unrows)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DECAY, ALPHA = 0.99, 1e-5


def mirror(case, train):
    """The mirror of the case's reference module with its recorded state, on the device."""
    from vqae_amd.layers.vq import EMAVectorQuantizer, ProjectedEMAVectorQuantizer2d
    sd = case["sd"]
    K, D = sd["embed"].shape
    if "proj_in.weight" in sd:
        m = ProjectedEMAVectorQuantizer2d(K, sd["proj_in.weight"].shape[1], case["cc"], DECAY, ALPHA, projection_dim=D)
    else:
        m = EMAVectorQuantizer(K, D, case["cc"], DECAY, ALPHA)
    m.load_state_dict(sd)
    return m.cuda().train(train)


def module_grads(m, case):
    x = case["x"].cuda().requires_grad_()
    out, idx, loss = m(x)
    grads = torch.autograd.grad([out, loss], [x] + list(m.parameters()), [case["g_out"].cuda(), case["g_loss"].cuda()])
    torch.cuda.synchronize()
    return idx.cpu(), [g.cpu() for g in grads]


def check_parity(test, name, mode, got, case):
    g32, g64 = case["grads"](mode)
    assert len(got) == len(g64)
    worst = 0.0
    for nm, g, a, b in zip(GRAD_NAMES, got, g32, g64):
        assert g.shape == b.shape and g.dtype == torch.float32 and bool(torch.isfinite(g).all())
        e, e_ref = rel(g, b), rel(a, b)
        print(f"{test} {name} {mode} {nm}: e_dev {e:.3e} e_ref {e_ref:.3e}")
        record_parity(test, case=name, mode=mode, tensor=nm, e_dev=e, e_ref=e_ref)
        worst = max(worst, e / e_ref if e_ref > 0 else (0.0 if e == 0 else float("inf")))
    return worst


# ---- parity with the reference's autograd -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PROJ8)
def test_projected_kernel_parity(amd, bfx, name):
    """The C entry on the fixture's indices: z = proj_in(x) rounded from fp64, q = embed[idx]; against the eval-mode and the
    train-mode record."""
    case = load_case(bfx, name)
    g_out, x, z, q, g_loss, w_in, w_out = (t.float().cuda() for t in projected_inputs(case, torch.float64))
    got = amd.ops.vq_projected_backward(g_out, x, z, q, g_loss, w_in, w_out, case["cc"])
    torch.cuda.synchronize()
    got = [unrows(got[0].cpu(), case["x"].shape)] + [g.cpu().reshape(r.shape) for g, r in zip(got[1:], case["grads"]("eval")[1][1:])]
    for mode in ("eval", "train"):
        assert check_parity("vq_backward_kernel", name, mode, got, case) <= 4


def forward_refused(name, mode):
    """Shapes the mirrors' FORWARD has always refused (vqae_conv2d_f32 takes input channels in multiples of 8): the unfused
    route -- training mode, or projection_dim != 8 -- at C = 12, and projection_dim = 4 (proj_out's input) in either mode.
    Their fixture gradients are checked below the module: test_projected_kernel_parity (C = 12; the train-mode record
    equals the eval-mode one) and test_fallback_parity_on_device (P = 4)."""
    return name in PROJ4 or (name == "proj_2x12x3x5" and mode == "train")


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("name", PLAIN + PROJ8 + PROJ4 + PROJ16)
def test_module_parity_and_saved_lookup(amd, bfx, name, mode):
    """The mirrors' own forward + backward: their indices are the fixture's, their gradients within the bar in eval AND in
    train mode.  Train mode is the saved-tensor trap: _update_ema has rewritten `embed` by the time backward runs, and the
    fixture's train-mode gradients (which the generator found equal to the eval-mode ones, vq.py:130-133) need the lookup in
    the codebook as it was before.  proj16 takes the backward composed from torch matmuls (projection_dim != 8)."""
    case = load_case(bfx, name)
    m = mirror(case, mode == "train")
    if forward_refused(name, mode):
        with pytest.raises(NotImplementedError):
            m(case["x"].cuda().requires_grad_())
        return
    before = m.embed.clone()
    idx, got = module_grads(m, case)
    assert torch.equal(idx, case["idx"]), int((idx != case["idx"]).sum())
    assert torch.equal(m.embed, before) == (mode == "eval")         # train mode did move the codebook under the saved q
    assert case["train_equals_eval"]
    assert check_parity("vq_backward_module", name, mode, got, case) <= 4


@pytest.mark.parametrize("name", PROJ4 + PROJ16)
def test_fallback_parity_on_device(amd, bfx, name):
    """projected_backward_reference in fp32 on the device -- the backward of the shapes the fused kernel does not take -- on
    the fixture's indices, at the same bar."""
    from vqae_amd.layers.vq import projected_backward_reference
    case = load_case(bfx, name)
    g_out, x, z, q, g_loss, w_in, w_out = (t.float().cuda() for t in projected_inputs(case, torch.float64))
    got = projected_backward_reference(g_out, x, z, q, g_loss, case["cc"], w_in, w_out)
    got = [unrows(got[0].cpu(), case["x"].shape)] + [g.cpu().reshape(r.shape) for g, r in zip(got[1:], case["grads"]("eval")[1][1:])]
    for mode in ("eval", "train"):
        assert check_parity("vq_backward_fallback", name, mode, got, case) <= 4


# ---- shapes, at the C level -----------------------------------------------------------------------------------------------------
def shape_inputs(N, C, seed, K=37):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    x, g_out = r(N, C) * 1.3 + 0.2, r(N, C) * 0.7
    w_in, b_in, w_out = r(8, C) / C ** 0.5, r(8) * 0.1, r(C, 8) * 0.4
    z = (x.double() @ w_in.double().t() + b_in.double()).float()
    embed = r(K, 8)
    q = embed[torch.randint(0, K, (N,), generator=g)]
    return [t.cuda() for t in (g_out, x, z, q, torch.tensor(0.8), w_in, w_out)]


def projected_bounds(g_out, x, z, q, g_loss, cc, w_in, w_out):
    """The elementwise bounds of the module docstring, fp64 on the device, in the order of the five outputs."""
    from vqae_amd.layers.vq import projected_backward_reference
    C = x.shape[1]
    S = 1 if C <= 128 else 2
    d = lambda t: t.double().abs()
    zero_loss = g_loss is None
    gl = torch.zeros((), dtype=torch.float64, device=x.device) if zero_loss else d(g_loss)
    go = torch.zeros_like(x).double() if g_out is None else d(g_out)
    m_x, m_w_in, m_b_in, _, m_b_out = projected_backward_reference(go, d(x), d(z.double() - q.double()), torch.zeros_like(q).double(),
                                                                   gl, cc, d(w_in), d(w_out))
    m_w_out = go.t() @ d(q)
    return ((4 * S + 16) * U * m_x, (4 * S + 9) * U * m_w_in, (4 * S + 9) * U * m_b_in, 2 * U * m_w_out, 2 * U * m_b_out)


def check_shapes(amd, args, cc, tag, want=(True,) * 5):
    from vqae_amd.layers.vq import projected_backward_reference
    g_out, x, z, q, g_loss, w_in, w_out = args
    got = amd.ops.vq_projected_backward(g_out, x, z, q, g_loss, w_in, w_out, cc, want)
    dd = lambda t: None if t is None else t.double()
    ref = projected_backward_reference(dd(g_out), dd(x), dd(z), dd(q), dd(g_loss), cc, dd(w_in), dd(w_out))
    bounds = projected_bounds(g_out, x, z, q, g_loss, cc, w_in, w_out)
    worst = 0.0
    for nm, g, r, b, on in zip(GRAD_NAMES, got, ref, bounds, want):
        if not on:
            assert g is None
            continue
        assert g.shape == r.shape and bool(torch.isfinite(g).all()), (tag, nm)
        err = (g.double() - r).abs()
        assert bool((err <= b).all()), (tag, nm, float((err / b.clamp_min(1e-300)).max()))
        if bool((b > 0).any()):
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    return worst


@pytest.mark.parametrize("C", [4, 12, 64, 128, 256])
def test_projected_kernel_shapes(amd, C):
    """One row, less than a step (15), ragged steps in 3 workgroups (561 = 3 x 192 - 15) and 6 workgroups with a ragged last
    one (1500 = 5 x 256 + 220, 220 = 27 x 8 + 4); C below a lane quad's reach (4, 12), half a slab, one slab, two slabs."""
    for N in (1, 15, 561, 1500):
        worst = check_shapes(amd, shape_inputs(N, C, 1000 * C + N), 0.25, (N, C))
        record_parity("vq_backward_shapes", N=N, C=C, worst_err_over_bound=worst)


@pytest.mark.parametrize("C", [12, 128, 256])
def test_projected_kernel_null_arguments(amd, C):
    """NULL g_out / g_loss are zero upstream gradients; NULL outputs are skipped and leave the others' bits alone."""
    N = 561
    args = shape_inputs(N, C, 77 + C)
    full = amd.ops.vq_projected_backward(*args, 0.25)
    no_out = list(args)
    no_out[0] = None
    check_shapes(amd, no_out, 0.25, "g_out=None")
    got = amd.ops.vq_projected_backward(*no_out, 0.25)
    assert not got[3].any() and not got[4].any()
    no_loss = list(args)
    no_loss[4] = None
    check_shapes(amd, no_loss, 0.25, "g_loss=None")
    neither = list(args)
    neither[0] = neither[4] = None
    assert all(not g.any() for g in amd.ops.vq_projected_backward(*neither, 0.25))
    for want in ((True, False, False, False, False), (False, True, True, False, False), (False, False, False, True, True),
                 (False,) * 5):
        got = amd.ops.vq_projected_backward(*args, 0.25, want)
        for g, f, on in zip(got, full, want):
            assert (g is None) if not on else torch.equal(g, f), want


def test_projected_kernel_edges(amd):
    """N = 0 writes zeros over whatever the buffers held; unsupported projection_dim / channels raise as the forward does."""
    L, ops = amd._lib, amd.ops
    C = 12
    bufs = [torch.full(s, float("nan"), device="cuda") for s in ((8, C), (8,), (C, 8), (C,))]
    e = torch.zeros(0, C, device="cuda")
    e8 = torch.zeros(0, 8, device="cuda")
    w = torch.zeros(C, 8, device="cuda")
    ws = torch.empty(L.lib().vqae_vq_projected_backward_workspace_bytes(0, C), dtype=torch.uint8, device="cuda")
    L.check(L.lib().vqae_vq_projected_backward_f32(None, ops._p(e), ops._p(e8), ops._p(e8), None, ops._p(w), ops._p(w), 0, C, 8, 0.25,
                                                   None, *[ops._p(b) for b in bufs], ops._p(ws), ops._stream()))
    torch.cuda.synchronize()
    assert all(not b.any() for b in bufs)
    got = ops.vq_projected_backward(None, e, e8, e8, None, w.t().contiguous(), w, 0.25)
    assert got[0].shape == (0, C) and all(not g.any() for g in got[1:])
    for C, P in ((6, 8), (12, 4), (12, 16), (260, 8)):
        x = torch.zeros(4, C, device="cuda")
        zq = torch.zeros(4, P, device="cuda")
        with pytest.raises(NotImplementedError):
            ops.vq_projected_backward(x, x, zq, zq, torch.ones((), device="cuda"), torch.zeros(P, C, device="cuda"),
                                      torch.zeros(C, P, device="cuda"), 0.25)


@pytest.mark.parametrize("D", [1, 5, 8, 130])
def test_plain_kernel_shapes(amd, D):
    """vqae_vq_backward_f32 on 16-byte vectors (N D % 4 == 0) and on the scalar path, with NULL g_q / g_loss."""
    from vqae_amd.layers.vq import backward_reference
    for N in (1, 15, 1025, 40000):
        g = torch.Generator().manual_seed(N + D)
        x, q, g_q = (torch.randn(N, D, generator=g).cuda() for _ in range(3))
        g_loss = torch.tensor(-1.25).cuda()
        for gq, gl in ((g_q, g_loss), (None, g_loss), (g_q, None), (None, None)):
            got = amd.ops.vq_backward(gq, x, q, gl, 0.25)
            ref = backward_reference(None if gq is None else gq.double(), x.double(), q.double(), None if gl is None else gl.double(), 0.25)
            s = 0.0 if gl is None else abs(float(gl)) * 0.25 * 2 / (N * D)
            bound = 4 * U * ((0 if gq is None else gq.double().abs()) + s * (x.double() - q.double()).abs())
            assert bool(((got.double() - ref).abs() <= bound).all()), (N, D, gq is None, gl is None)
            if gl is None and gq is not None:
                assert torch.equal(got, gq)


# ---- determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [128, 256])
def test_projected_kernel_bit_identical_run_to_run(amd, C):
    args = shape_inputs(5000, C, 9 + C)
    a = amd.ops.vq_projected_backward(*args, 0.25)
    for _ in range(3):
        b = amd.ops.vq_projected_backward(*args, 0.25)
        assert all(torch.equal(s, t) for s, t in zip(a, b))


# ---- nothing else moved -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", ["plain_2x12x3x5", "plain_1x5x2x3x4", "proj_3x128x8x8", "proj_1x64x33x17", "proj16_2x16x3x5"])
def test_grad_forward_equals_no_grad_forward(amd, bfx, name, train):
    """Values, indices, loss and the three buffers of the grad-requiring forward are bit-equal to the no-grad forward of a
    clone; the no-grad call returns tensors without a grad_fn, the other one tensors with one."""
    case = load_case(bfx, name)
    m0 = mirror(case, train)
    m1 = copy.deepcopy(m0)
    x = case["x"].cuda()
    with torch.no_grad():
        out0, idx0, loss0 = m0(x)
    assert out0.grad_fn is None and loss0.grad_fn is None and not out0.requires_grad
    out1, idx1, loss1 = m1(x.clone().requires_grad_())
    assert out1.grad_fn is not None and loss1.grad_fn is not None and not idx1.requires_grad
    assert torch.equal(out0, out1) and torch.equal(idx0, idx1) and torch.equal(loss0, loss1)
    for b in ("embed", "embed_avg", "cluster_size"):
        assert torch.equal(getattr(m0, b), getattr(m1, b)), b
    assert torch.equal(m1.embed, mirror(case, train).embed) == (not train)
    if not list(m0.parameters()):                       # the plain quantiser: an input without grad takes the old path
        out2, _, loss2 = copy.deepcopy(m0).eval()(x)
        assert out2.grad_fn is None and loss2.grad_fn is None


def test_autocast_gradient_is_fp32_cast_back(amd, bfx):
    """A bf16 input: the mirror computes in fp32 (as it always did) and returns the fp32 gradient rounded to bf16."""
    case = load_case(bfx, "proj_2x12x3x5")
    m = mirror(case, False)
    xb = case["x"].cuda().bfloat16()
    ga, gb = [], []
    for x, dst in ((xb.float().requires_grad_(), ga), (xb.clone().requires_grad_(), gb)):
        out, _, loss = m(x)
        dst.extend(torch.autograd.grad([out, loss], [x] + list(m.parameters()), [case["g_out"].cuda(), case["g_loss"].cuda()]))
    assert gb[0].dtype == torch.bfloat16 and torch.equal(gb[0], ga[0].bfloat16())
    assert all(torch.equal(a, b) for a, b in zip(ga[1:], gb[1:]))


# ---- the use case -----------------------------------------------------------------------------------------------------------------
class Loop(nn.Module):
    def __init__(self, vq):
        super().__init__()
        self.enc, self.vq, self.dec = nn.Conv2d(3, 16, 1), vq, nn.Conv2d(16, 3, 1)

    def forward(self, x):
        q, idx, vq_loss = self.vq(self.enc(x))
        return self.dec(q), idx, vq_loss


def test_closed_loop_trains_like_the_reference(amd, bfx):
    """Stock torch convs around the mirror, 3 SGD steps in train mode: the reference's indices at every step, losses and
    final parameters / buffers within 4 x the distance of the reference's fp32 run from its fp64 run."""
    from vqae_amd.layers.vq import ProjectedEMAVectorQuantizer2d
    t = lambda k: torch.from_numpy(bfx[k])
    model = Loop(ProjectedEMAVectorQuantizer2d(64, 16, 0.25, DECAY, ALPHA, projection_dim=8))
    model.load_state_dict({k[len("loop/sd0/"):]: t(k) for k in bfx.files if k.startswith("loop/sd0/")})
    model = model.cuda().train()
    x, target = t("loop/x").float().cuda(), t("loop/target").float().cuda()
    opt = torch.optim.SGD(model.parameters(), lr=float(bfx["loop/lr"]))
    l32, l64 = bfx["loop/loss32"].astype("float64"), bfx["loop/loss64"]
    for step in range(3):
        rec, idx, vq_loss = model(x[step])
        loss = torch.nn.functional.mse_loss(rec, target[step]) + vq_loss
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert torch.equal(idx.cpu(), t("loop/idx")[step].long()), step
        e, e_ref = abs(float(loss.detach()) - l64[step]) / abs(l64[step]), abs(l32[step] - l64[step]) / abs(l64[step])
        print(f"closed loop step {step}: loss {float(loss.detach()):.9g} e_dev {e:.3e} e_ref {e_ref:.3e}")
        record_parity("vq_backward_closed_loop_loss", step=step, e_dev=e, e_ref=e_ref)
        assert e <= 4 * e_ref, (step, e, e_ref)
    for k, v in model.state_dict().items():
        if v.dim() == 0:
            continue
        e, e_ref = rel(v.cpu(), t(f"loop/final64/{k}")), rel(t(f"loop/final32/{k}"), t(f"loop/final64/{k}"))
        print(f"closed loop final {k}: e_dev {e:.3e} e_ref {e_ref:.3e}")
        record_parity("vq_backward_closed_loop_final", tensor=k, e_dev=e, e_ref=e_ref)
        assert e <= 4 * e_ref, (k, e, e_ref)
