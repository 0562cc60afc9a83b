"""GPU: the fused multi-tensor optimiser step (csrc/optim.hip) through FusedAdam / FusedAdamW / FusedLamb, through SAM over
them and through the raw C ABI.

Accuracy.  The measure is make_classifier_optim_golden.measure: per tensor ||dp_test - dp_64|| / ||dp_64|| over the steps, worst
tensor.  The bar is test_classifier_optim_gpu.py's: d <= 2 * y, d the device's distance to the fp64 record and y that of an
fp32 run of the reference's classes (the fixture) or of their mirrors / torch's Adam and AdamW on the CPU (at test time) on the
same gradients; p, exp_avg and exp_avg_sq are held to it separately.  All comparisons but the closed loop are open-loop: truth,
yardstick and device see the same gradient bits.  Every figure is recorded through record_parity.

Shapes.  The fixture's eleven tensors (2 064 numbers) and a list around the kernel's two bounds, C = VQAE_OPTIM_CHUNK and S =
VQAE_OPTIM_SMALL: S, S + 1, C - 1, C, C + 1, 2 C + 5 elements, a (40, 24, 3, 3) weight, a channels_last (16, 8, 3, 3) weight, a
(7,) view one float into a buffer (4-byte aligned only) and 300 scalars, a third of them zero.

Measured on an MI355X (device over yardstick, the 23 comparisons of this file; profiles/optim_parity_report.jsonl, DESIGN.md
section 15): p 0.46 - 1.02, exp_avg 0.53 - 1.88 (adaptive SAM + LAMB on the large list; Adam on the fixture 1.76), exp_avg_sq
0.53 - 1.03."""
import ctypes
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, record_parity

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_optim_golden as G  # noqa: E402
from test_optim_multi_cpu import CASES, LR, N, RHO, T, fused, hyper, mirror, record  # noqa: E402

pytestmark = pytest.mark.gpu

BIG_CASES = ("adamw", "lamb", "sam_adamw", "asam_lamb")


@pytest.fixture(scope="module")
def mfx():
    return load_golden("optim_multi")


# ---- tensor lists ----------------------------------------------------------------------------------------------------------------
def big_list(amd, steps=T, seed=4100):
    """-> (weights fp32, layouts, grads [steps][n] fp64): the list around the kernel's bounds"""
    C, S = amd._lib.OPTIM_CHUNK, amd._lib.OPTIM_SMALL
    shapes = [(S,), (S + 1,), (C - 1,), (C,), (C + 1,), (2 * C + 5,), (40, 24, 3, 3), (16, 8, 3, 3), (7,)] + [(1,)] * 300
    layouts = ["plain"] * 7 + ["channels_last", "view"] + ["plain"] * 300
    rs = np.random.RandomState(seed)
    ws = []
    for i, s in enumerate(shapes):
        w = rs.standard_normal(s) * ((1.6 / (s[1] * 9) ** 0.5) if len(s) == 4 else 1.0)
        if s == (1,) and i % 3 == 0:
            w[:] = 0.0
        ws.append(w.astype(np.float32))
    grads = [[rs.standard_normal(s) * 0.1 for s in shapes] for _ in range(steps)]
    return ws, layouts, grads


def fixture_list(steps=T):
    ws, grads = G.problem(steps=steps)
    return ws, ["plain"] * N, grads


def make_params(ws, layouts, dtype, device):
    ps = []
    for w, lay in zip(ws, layouts):
        t = torch.from_numpy(w).to(device=device, dtype=dtype).clone()        # (never the numpy array's own memory)
        if lay == "channels_last":
            t = t.contiguous(memory_format=torch.channels_last)
        elif lay == "view":
            buf = torch.zeros(t.numel() + 9, dtype=dtype, device=device)
            buf[1:1 + t.numel()].copy_(t)
            t = buf[1:1 + t.numel()]
        p = torch.nn.Parameter(t)
        assert p.stride() == t.stride() and p.data_ptr() == t.data_ptr()
        ps.append(p)
    return ps


def feed(ps, layouts, gs, dtype, device, scale=1.0, step=0, none=()):
    for i, (p, lay, g) in enumerate(zip(ps, layouts, gs)):
        if i in none:
            p.grad = None
            continue
        t = torch.from_numpy(scale * g).to(device=device, dtype=dtype)
        if lay == "channels_last" and step % 2 == 0:                # the parameter's strides on even steps, other strides on odd
            t = t.contiguous(memory_format=torch.channels_last)
        p.grad = t


def final(ps, opt, sam):
    """-> (p, exp_avg, exp_avg_sq, steps) as logical numpy arrays, through state_dict()"""
    torch.cuda.synchronize()
    sd = (opt.base_optimizer if sam else opt).state_dict()["state"]
    p = [q.detach().cpu().numpy() for q in ps]
    m = [sd[i]["exp_avg"].detach().cpu().numpy() if i in sd else np.zeros_like(p[i]) for i in range(len(ps))]
    v = [sd[i]["exp_avg_sq"].detach().cpu().numpy() if i in sd else np.zeros_like(p[i]) for i in range(len(ps))]
    return p, m, v, [int(sd[i]["step"]) if i in sd else 0 for i in range(len(ps))]


def run_list(make_opt, prob, dtype, device, sam, none_at=lambda s: (), before_step=None):
    ws, layouts, grads = prob
    ps = make_params(ws, layouts, dtype, device)
    opt = make_opt(ps)
    for s, gs in enumerate(grads):
        if before_step is not None:
            before_step(s, opt, ps)
        feed(ps, layouts, gs, dtype, device, 1.0, s, none_at(s))
        if sam:
            opt.first_step()
            feed(ps, layouts, gs, dtype, device, 0.9, s, none_at(s))
            opt.second_step()
        else:
            opt.step()
    return final(ps, opt, sam) if device == "cuda" else final_cpu(ps, opt, sam)


def final_cpu(ps, opt, sam):
    sd = (opt.base_optimizer if sam else opt).state_dict()["state"]
    p = [q.detach().numpy().copy() for q in ps]
    m = [sd[i]["exp_avg"].numpy().copy() if i in sd else np.zeros_like(p[i]) for i in range(len(ps))]
    v = [sd[i]["exp_avg_sq"].numpy().copy() if i in sd else np.zeros_like(p[i]) for i in range(len(ps))]
    return p, m, v, [int(sd[i]["step"]) if i in sd else 0 for i in range(len(ps))]


def held_to_yardstick(test, what, got, truth, ref32, ws):
    """got = (p, m, v) of the device; truth / ref32 the fp64 / fp32 runs: each of p, m, v within 2 x its yardstick"""
    zero = [np.zeros_like(w) for w in ws]
    figs = {}
    for name, a, t, r, start in zip(("p", "exp_avg", "exp_avg_sq"), got, truth, ref32, (ws, zero, zero)):
        figs[name] = (G.measure(a, t, start), G.measure(r, t, start))
    record_parity(test, case=what, **{k: {"device": d, "yardstick": y, "ratio": (d / y if y > 0 else None)}
                                      for k, (d, y) in figs.items()})
    for name, (d, y) in figs.items():
        assert d <= 2 * y, f"{what} {name}: {d:.3e} from the fp64 run, the fp32 run of the reference's code {y:.3e}"


def same_bits(a, b):
    for x, y in zip(a[:3], b[:3]):
        for s, t in zip(x, y):
            assert np.array_equal(np.ascontiguousarray(s).view(np.uint32), np.ascontiguousarray(t).view(np.uint32))


_memo = {}


def big_runs(amd, case):
    """fp64 truth and fp32 yardstick of the mirrors on the CPU, and one device run, of a case on the big list (computed once)"""
    if case not in _memo:
        kind, wd, adaptive = CASES[case]
        prob = big_list(amd)
        sam = adaptive is not None
        _memo[case] = (prob,
                       run_list(lambda ps: mirror(amd, ps, kind, wd, adaptive), prob, torch.float64, "cpu", sam),
                       run_list(lambda ps: mirror(amd, ps, kind, wd, adaptive), prob, torch.float32, "cpu", sam),
                       run_list(lambda ps: fused(amd, ps, kind, wd, adaptive), prob, torch.float32, "cuda", sam))
    return _memo[case]


# ---- the raw C ABI -----------------------------------------------------------------------------------------------------------------
class Raw:
    """A vqae_optim over device tensors, driven through the C ABI; one param group."""

    def __init__(self, amd, ws, kind, wd, adaptive, lr=LR):
        self.L = L = amd._lib
        self.lib = L.lib()
        self.ps = [torch.from_numpy(np.ascontiguousarray(w, np.float32)).cuda() for w in ws]
        self.n = n = len(ws)
        self.cfg = L.ClassifierOptimConfig(L.OPTIM_KINDS[kind], lr, 0.9, 0.999, G.EPS[kind], wd, -1.0 if adaptive is None else RHO,
                                           int(bool(adaptive)))
        self.h = ctypes.c_void_p()
        L.check(self.lib.vqae_optim_create(n, (ctypes.c_int64 * n)(*[p.numel() for p in self.ps]), (ctypes.c_int * n)(),
                                           1, ctypes.byref(self.cfg), ctypes.byref(self.h)))
        self.sam = adaptive is not None
        self.pp = (ctypes.c_void_p * n)(*[p.data_ptr() for p in self.ps])

    def ptrs(self, gs, scale=1.0):
        keep = [None if g is None else torch.from_numpy(scale * np.asarray(g, np.float64)).float().cuda() for g in gs]
        return keep, (ctypes.c_void_p * self.n)(*[None if t is None else t.data_ptr() for t in keep])

    def step(self, gs):
        if self.sam:
            keep, gp = self.ptrs(gs)
            self.L.check(self.lib.vqae_optim_sam_first(self.h, self.pp, gp, None))
        keep2, gp = self.ptrs(gs, 0.9 if self.sam else 1.0)
        self.L.check(self.lib.vqae_optim_step(self.h, self.pp, gp, None))
        torch.cuda.synchronize()

    def state(self):
        tot = sum(p.numel() for p in self.ps)
        m, v, steps = np.empty(tot, np.float32), np.empty(tot, np.float32), (ctypes.c_int64 * self.n)()
        self.L.check(self.lib.vqae_optim_export(self.h, m.ctypes.data, v.ctypes.data, steps, None))
        cut = np.cumsum([p.numel() for p in self.ps])[:-1]
        shapes = [tuple(p.shape) for p in self.ps]
        return ([a.reshape(s) for a, s in zip(np.split(m, cut), shapes)], [a.reshape(s) for a, s in zip(np.split(v, cut), shapes)],
                list(steps))

    def weights(self):
        return [p.cpu().numpy() for p in self.ps]

    def close(self):
        self.lib.vqae_optim_destroy(self.h)


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_fixture_through_the_classes(amd, mfx, case):
    kind, wd, adaptive = CASES[case]
    prob = fixture_list()
    p, m, v, steps = run_list(lambda ps: fused(amd, ps, kind, wd, adaptive), prob, torch.float32, "cuda", adaptive is not None)
    assert steps == [T] * N
    held_to_yardstick("optim_multi_fixture_classes", case, (p, m, v), record(mfx, case, "64"), record(mfx, case, "32"), prob[0])


@pytest.mark.parametrize("case", list(CASES))
def test_fixture_through_the_c_abi(amd, mfx, case):
    kind, wd, adaptive = CASES[case]
    ws, grads = G.problem()
    d = Raw(amd, ws, kind, wd, adaptive)
    try:
        for gs in grads:
            d.step(gs)
        m, v, steps = d.state()
        assert steps == [T] * N
        held_to_yardstick("optim_multi_fixture_abi", case, (d.weights(), m, v), record(mfx, case, "64"), record(mfx, case, "32"), ws)
    finally:
        d.close()


# ---- 2. the list around the bounds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BIG_CASES)
def test_large_list(amd, case):
    prob, truth, ref32, dev = big_runs(amd, case)
    assert dev[3] == [T] * len(prob[0])
    held_to_yardstick("optim_multi_large_list", case, dev[:3], truth[:3], ref32[:3], prob[0])


# ---- 3. tensors without a gradient --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lamb", "sam_adamw"])
def test_none_gradients(amd, case):
    kind, wd, adaptive = CASES[case]
    sam = adaptive is not None
    prob = big_list(amd)
    idle = (10, 0, 5)                                              # a scalar, a small tensor, the three-chunk tensor
    assert prob[0][10].size == 1 and prob[0][10][0] != 0 and prob[0][0].size == amd._lib.OPTIM_SMALL
    assert prob[0][5].size > 2 * amd._lib.OPTIM_CHUNK

    def none_at(s):
        return idle if s in (2, 3, 4) else ()

    snaps = {}

    def snap(s, opt, ps):
        if s in (2, 5):
            torch.cuda.synchronize()
            snaps[s] = [ps[i].detach().cpu().numpy().copy() for i in idle]

    truth = run_list(lambda ps: mirror(amd, ps, kind, wd, adaptive), prob, torch.float64, "cpu", sam, none_at)
    ref32 = run_list(lambda ps: mirror(amd, ps, kind, wd, adaptive), prob, torch.float32, "cpu", sam, none_at)
    dev = run_list(lambda ps: fused(amd, ps, kind, wd, adaptive), prob, torch.float32, "cuda", sam, none_at, snap)
    for a, b in zip(snaps[2], snaps[5]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))            # bit-unchanged over steps 3 - 5
    want = [T - 3 if i in idle else T for i in range(len(prob[0]))]
    assert dev[3] == want and truth[3] == want
    held_to_yardstick("optim_multi_none_gradients", case, dev[:3], truth[:3], ref32[:3], prob[0])


# ---- 4. moving addresses -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lamb", "sam_adamw"])
def test_moving_gradient_addresses(amd, case):
    kind, wd, adaptive = CASES[case]
    sam = adaptive is not None
    ws, layouts, grads = big_list(amd, steps=4)
    outs, seen = [], set()
    for moving in (True, False):
        ps = make_params(ws, layouts, torch.float32, "cuda")
        opt = fused(amd, ps, kind, wd, adaptive)
        junk = []
        for s, gs in enumerate(grads):
            for scale in ((1.0, 0.9) if sam else (1.0,)):
                if moving or s == 0 and scale == 1.0:
                    junk.append(torch.empty(1000 * (len(junk) + 1) + 3, device="cuda"))     # shifts what the allocator hands out
                    feed(ps, layouts, gs, torch.float32, "cuda", scale)
                    if moving:
                        seen.add(ps[5].grad.data_ptr())
                        junk.append(ps[5].grad)                                              # keeps the address from coming back
                else:
                    for p, g in zip(ps, gs):
                        p.grad.copy_(torch.from_numpy(scale * g).to(device="cuda", dtype=torch.float32))
                if not sam:
                    opt.step()
                elif scale == 1.0:
                    opt.first_step()
                else:
                    opt.second_step()
        outs.append(final(ps, opt, sam))
    assert len(seen) == len(grads) * (2 if sam else 1)             # every table named another address
    same_bits(outs[0], outs[1])


# ---- 5. the table ring ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lamb", "asam_lamb"])
def test_ring_of_tables(amd, case):
    """32 steps enqueued back to back (more tables than the ring has slots, different gradients each) equal the same steps
    with a synchronisation after each."""
    kind, wd, adaptive = CASES[case]
    sam = adaptive is not None
    ws, layouts, grads = fixture_list(steps=32)
    dev_grads = [[torch.from_numpy(g).float().cuda() for g in gs] for gs in grads]
    dev_grads2 = [[torch.from_numpy(0.9 * g).float().cuda() for g in gs] for gs in grads]
    outs = []
    for sync in (False, True):
        ps = make_params(ws, layouts, torch.float32, "cuda")
        opt = fused(amd, ps, kind, wd, adaptive)
        torch.cuda.synchronize()
        for gs, gs2 in zip(dev_grads, dev_grads2):
            for p, g in zip(ps, gs):
                p.grad = g
            if sam:
                opt.first_step()
                for p, g in zip(ps, gs2):
                    p.grad = g
                opt.second_step()
            else:
                opt.step()
            if sync:
                torch.cuda.synchronize()
        outs.append(final(ps, opt, sam))
    assert outs[0][3] == [32] * N
    same_bits(outs[0], outs[1])


# ---- 6. determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BIG_CASES)
def test_two_runs_give_the_same_bits(amd, case):
    kind, wd, adaptive = CASES[case]
    prob, _, _, first = big_runs(amd, case)
    again = run_list(lambda ps: fused(amd, ps, kind, wd, adaptive), prob, torch.float32, "cuda", adaptive is not None)
    same_bits(first, again)


# ---- 7. param groups and an lr schedule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_two_param_groups_and_lr_schedule(amd, kind):
    from vqae_amd.optim import FusedAdamW, FusedLamb, Lamb
    prob = fixture_list()

    def make(cls):
        def f(ps):
            return cls([dict(params=ps[:6], lr=LR, weight_decay=0.01), dict(params=ps[6:], lr=2 * LR, weight_decay=0.0)],
                       **hyper(kind, 0.3, lr=7.0))
        return f

    def halve(s, opt, ps):
        if s == 4:
            for g in opt.param_groups:
                g["lr"] = 0.5 * g["lr"]

    cpu_cls = {"adamw": torch.optim.AdamW, "lamb": Lamb}[kind]
    dev_cls = {"adamw": FusedAdamW, "lamb": FusedLamb}[kind]
    truth = run_list(make(cpu_cls), prob, torch.float64, "cpu", False, before_step=halve)
    ref32 = run_list(make(cpu_cls), prob, torch.float32, "cpu", False, before_step=halve)
    dev = run_list(make(dev_cls), prob, torch.float32, "cuda", False, before_step=halve)
    one_lr = run_list(lambda ps: cpu_cls(ps, **hyper(kind, 0.01)), prob, torch.float64, "cpu", False)
    assert G.measure(one_lr[0], truth[0], prob[0]) > 1e-2          # the groups and the schedule matter
    held_to_yardstick("optim_multi_param_groups", kind, dev[:3], truth[:3], ref32[:3], prob[0])


# ---- 8. state round trip on the device --------------------------------------------------------------------------------------------------
def test_state_round_trip_on_the_device(amd):
    """4 steps FusedLamb -> state_dict -> Lamb on the same device tensors for 2 -> back -> 2, against 8 uninterrupted steps."""
    from vqae_amd.optim import FusedLamb, Lamb
    ws, layouts, grads = fixture_list()
    rs = np.random.RandomState(77)
    ws = ws + [(rs.standard_normal((16, 8, 3, 3)) * 0.18).astype(np.float32)]
    layouts = layouts + ["channels_last"]
    grads = [gs + [rs.standard_normal((16, 8, 3, 3)) * 0.1] for gs in grads]
    prob = (ws, layouts, grads)
    truth = run_list(lambda ps: Lamb(ps, **hyper("lamb", 0.01)), prob, torch.float64, "cpu", False)
    ref32 = run_list(lambda ps: Lamb(ps, **hyper("lamb", 0.01)), prob, torch.float32, "cpu", False)
    ps = make_params(ws, layouts, torch.float32, "cuda")

    def steps(opt, lo, hi):
        for s in range(lo, hi):
            feed(ps, layouts, grads[s], torch.float32, "cuda", 1.0, s)
            opt.step()

    a = FusedLamb(ps, **hyper("lamb", 0.01))
    steps(a, 0, 4)
    sd = a.state_dict()
    for k, p in enumerate(ps):
        assert tuple(sd["state"][k]["exp_avg"].shape) == tuple(p.shape) and sd["state"][k]["step"] == 4
    logical = Lamb([torch.nn.Parameter(torch.from_numpy(w).clone()) for w in ws], **hyper("lamb", 0.01))   # 4 mirror steps
    for s in range(4):
        for q, g in zip(logical.param_groups[0]["params"], grads[s]):
            q.grad = torch.from_numpy(g).float()
        logical.step()
    want = logical.state_dict()["state"][len(ws) - 1]["exp_avg"].numpy()
    got = sd["state"][len(ws) - 1]["exp_avg"].cpu().numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5 * np.abs(want).max()      # channels_last, compared logically
    b = Lamb(ps, lr=99.0)
    b.load_state_dict(sd)
    steps(b, 4, 6)
    c = FusedLamb(ps, lr=99.0)
    c.load_state_dict(b.state_dict())
    steps(c, 6, 8)
    dev = final(ps, c, False)
    assert dev[3] == [8] * len(ws)
    held_to_yardstick("optim_multi_state_round_trip", "lamb", dev[:3], truth[:3], ref32[:3], ws)


# ---- 9. closed loop -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lamb", "sam_adamw"])
def test_closed_loop(amd, case):
    kind, wd, adaptive = CASES[case]
    sam = adaptive is not None
    gen = torch.Generator().manual_seed(11)
    x, y = torch.randn(16, 6, generator=gen, dtype=torch.float64), torch.randn(16, 3, generator=gen, dtype=torch.float64)

    def loop(make_opt, dtype, device):
        torch.manual_seed(12)
        net = torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.ELU(), torch.nn.Linear(8, 8), torch.nn.ELU(), torch.nn.Linear(8, 3))
        net = net.to(device=device, dtype=dtype)
        xs, ys = x.to(device=device, dtype=dtype), y.to(device=device, dtype=dtype)
        ps = list(net.parameters())
        start = [p.detach().cpu().numpy().copy() for p in ps]
        opt = make_opt(ps)

        def closure():
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(net(xs), ys)
            loss.backward()
            return loss

        for _ in range(8):
            if sam:
                closure()
                opt.step(closure)
            else:
                opt.step(closure)
        out = final(ps, opt, sam) if device == "cuda" else final_cpu(ps, opt, sam)
        return out, start

    truth, start = loop(lambda ps: mirror(amd, ps, kind, wd, adaptive), torch.float64, "cpu")
    ref32, start32 = loop(lambda ps: mirror(amd, ps, kind, wd, adaptive), torch.float32, "cpu")
    dev, _ = loop(lambda ps: fused(amd, ps, kind, wd, adaptive), torch.float32, "cuda")
    assert all(np.array_equal(a.astype(np.float32), b) for a, b in zip(start, start32))
    held_to_yardstick("optim_multi_closed_loop", case, dev[:3], truth[:3], ref32[:3], start32)


# ---- 10. non-finite gradients, run-time errors ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_non_finite_gradient(amd, kind):
    """A nan gradient element is not an error: it turns its own p / m / v to nan and spreads exactly as far as it does in
    torch.  Under LAMB that is through ||u|| into the trust ratio of its tensor -- where lamb.py:106-114 then finds
    `u_norm > 0` false and takes the ratio 1 -- so the mirror on the CPU says which elements are nan afterwards, and the two
    more steps that follow let the nan parameter reach ||p|| too.  No other tensor changes by a bit."""
    ws, layouts, grads = fixture_list(steps=4)
    bad = [g.copy() for g in grads[1]]
    bad[9][2, 1, 0, 2] = np.nan
    probs = [(ws, layouts, grads), (ws, layouts, [grads[0], bad] + grads[2:])]
    clean, hit = (run_list(lambda ps: fused(amd, ps, kind, 0.01, None), pr, torch.float32, "cuda", False) for pr in probs)
    torch_side = run_list(lambda ps: mirror(amd, ps, kind, 0.01, None), probs[1], torch.float32, "cpu", False)
    for k in range(3):                                              # p, m, v
        for i in range(N):
            a, b = clean[k][i], hit[k][i]
            assert np.array_equal(np.isnan(b), np.isnan(torch_side[k][i])), (k, i)
            if i != 9:
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            else:
                assert np.isnan(b[2, 1, 0, 2])


def test_runtime_errors(amd):
    ws, grads = G.problem(steps=1)
    plain = Raw(amd, ws, "adamw", 0.01, None)
    sam = Raw(amd, ws, "adamw", 0.01, False)
    try:
        lib = plain.lib
        keep, gp = plain.ptrs(grads[0])
        assert lib.vqae_optim_sam_first(plain.h, plain.pp, gp, None) == -1                 # created without SAM
        assert b"without SAM" in lib.vqae_last_error()
        assert lib.vqae_optim_step(plain.h, None, gp, None) == -1
        assert lib.vqae_optim_step(plain.h, plain.pp, None, None) == -1
        holed = (ctypes.c_void_p * N)(*[None if i == 3 else p.data_ptr() for i, p in enumerate(plain.ps)])
        assert lib.vqae_optim_step(plain.h, holed, gp, None) == -1 and b"parameter 3" in lib.vqae_last_error()
        assert lib.vqae_optim_sam_first(sam.h, sam.pp, gp, None) == 0
        assert lib.vqae_optim_sam_first(sam.h, sam.pp, gp, None) == -1                     # twice in a row
        tot = sum(w.size for w in ws)
        z, steps = np.zeros(tot, np.float32), (ctypes.c_int64 * N)()
        assert lib.vqae_optim_import(sam.h, z.ctypes.data, z.ctypes.data, steps, None) == -1    # a climb is pending
        assert b"first step" in lib.vqae_last_error()
        assert lib.vqae_optim_step(sam.h, sam.pp, gp, None) == 0
        assert lib.vqae_optim_sam_first(sam.h, sam.pp, gp, None) == 0                      # ... and fine again after the step
        assert lib.vqae_optim_step(sam.h, sam.pp, gp, None) == 0
        assert lib.vqae_optim_import(sam.h, z.ctypes.data, z.ctypes.data, steps, None) == 0
        steps[2] = -1
        assert lib.vqae_optim_import(sam.h, z.ctypes.data, z.ctypes.data, steps, None) == -1
        other = plain.L.ClassifierOptimConfig(2, LR, 0.9, 0.999, 1e-8, 0.01, -1.0, 0)
        assert lib.vqae_optim_set(plain.h, ctypes.byref(other)) == -1                      # the kind does not change
        torch.cuda.synchronize()
        assert all(np.isfinite(w).all() for w in sam.weights())
        # fp64 parameters on the device are refused by the classes, before any launch
        from vqae_amd.optim import FusedLamb
        p = torch.nn.Parameter(torch.ones(3, dtype=torch.float64, device="cuda"))
        p.grad = torch.ones_like(p)
        with pytest.raises(TypeError):
            FusedLamb([p]).step()
    finally:
        plain.close()
        sam.close()
