"""GPU: the optimiser step on the classifier's device image (csrc/classifier_optim.hip) through the C ABI and through
ClassifierTrainer.

Accuracy.  The measure is test_classifier_optim_cpu's: per tensor ||dp_test - dp_64|| / ||dp_64|| over the T steps, worst
tensor; the yardstick is the same measure for an fp32 run of the reference's classes (from the fixture) or of their mirrors
(at test time) on the SAME gradients, and the device, another fp32 rounding of the same recurrences, may be 2 x the yardstick
away; exp_avg and exp_avg_sq are held to the same measure and bound.  Every comparison is open-loop: truth, yardstick and
device see the same gradient bits.  Where the gradients come from vqae_classifier_loss_grad (the end-to-end test) they are
the trainer's own, recorded as it runs, because a hand loop's gradients differ from the trainer's from the second step on
(its weights differ in the last bit), and that difference is not the optimiser's.

Measured on an MI355X (device next to yardstick; every line is recorded through record_parity, DESIGN.md section 11 has the
table): fixture variant dp -- Adam 8.70e-7 / 8.74e-7, AdamW 8.99e-6 / 9.01e-6, LAMB wd 0 9.08e-7 / 8.98e-7, LAMB 1.118e-6 /
1.116e-6, SAM + AdamW 8.98e-6 / 8.97e-6, adaptive SAM + LAMB 1.06e-6 / 1.11e-6; the moments between 0.9 and 1.6 x theirs
(worst: exp_avg_sq under SAM, 3.16e-7 / 2.02e-7).  K 2048, E 8, C 16: AdamW 8.52e-6 / 8.53e-6, LAMB 1.11e-6 / 1.13e-6,
adaptive SAM + LAMB 1.07e-6 / 1.13e-6.  Trainer end to end: 2.77e-6 / 2.77e-6, 1.16e-6 / 1.13e-6, 3.42e-6 / 3.42e-6."""
import ctypes
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, record_parity

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_classifier_optim_golden as G  # noqa: E402
from test_classifier_optim_cpu import CASES, LR, POS_WEIGHT, RHO, T, hyper, make_trainer, mirror, run_mirror  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("embedding.weight", "in_conv.weight", "in_conv.bias", "hidden_conv1.weight", "hidden_conv1.bias", "out_conv.weight",
         "out_conv.bias")
SMALL = (256, 1, 8)              # 993 numbers: one launch
LARGE = (2048, 8, 16)            # 20 017 numbers: partial sums and a second launch, E > 1, the 30-wide tile


@pytest.fixture(scope="module")
def ofx():
    return load_golden("classifier_optim")


@pytest.fixture(scope="module")
def large():
    """weights and gradients of the large variant (generated once)"""
    return G.problem(G.shapes_of(*LARGE), T, seed=3100)


class Dev:
    """A vqae_classifier and a vqae_classifier_optim on it, driven through the C ABI."""

    def __init__(self, amd, dims, ws, kind, wd, adaptive, lr=LR):
        from vqae_amd.classifier import NativeClassifier
        self.L = L = amd._lib
        self.lib = L.lib()
        self.shapes = [tuple(w.shape) for w in ws]
        self.nat = NativeClassifier(dims[0], dims[1], dims[2], 1, self.named(ws))
        self.cfg = L.ClassifierOptimConfig(L.OPTIM_KINDS[kind], lr, 0.9, 0.999, G.EPS[kind], wd, -1.0 if adaptive is None else RHO,
                                           int(bool(adaptive)))
        self.h = ctypes.c_void_p()
        L.check(self.lib.vqae_classifier_optim_create(self.nat._h, ctypes.byref(self.cfg), ctypes.byref(self.h)))
        self.sam = adaptive is not None

    @staticmethod
    def named(ws):
        return {"layers." + n: torch.from_numpy(np.ascontiguousarray(w, np.float32)) for n, w in zip(NAMES, ws)}

    @staticmethod
    def pack(gs, scale=1.0):
        return torch.from_numpy(np.concatenate([(scale * np.asarray(g, np.float64)).ravel() for g in gs])).cuda()

    def step(self, gs):
        g = self.pack(gs)
        if self.sam:
            self.L.check(self.lib.vqae_classifier_optim_sam_first(self.h, g.data_ptr(), None))
            g = self.pack(gs, 0.9)
        self.L.check(self.lib.vqae_classifier_optim_step(self.h, g.data_ptr(), None))

    def run(self, grads):
        for gs in grads:
            self.step(gs)
        torch.cuda.synchronize()
        return self

    def weights(self):
        outs = [np.empty(s, np.float32) for s in self.shapes]
        ptrs = (ctypes.c_void_p * 7)(*[o.ctypes.data for o in outs])
        self.L.check(self.lib.vqae_classifier_download(self.nat._h, ptrs, None))
        return outs

    def state(self):
        n = sum(int(np.prod(s)) for s in self.shapes)
        m, v, step = np.empty(n, np.float32), np.empty(n, np.float32), ctypes.c_int64()
        self.L.check(self.lib.vqae_classifier_optim_export(self.h, m.ctypes.data, v.ctypes.data, ctypes.byref(step), None))
        cut = np.cumsum([int(np.prod(s)) for s in self.shapes])[:-1]
        return ([a.reshape(s) for a, s in zip(np.split(m, cut), self.shapes)],
                [a.reshape(s) for a, s in zip(np.split(v, cut), self.shapes)], step.value)

    def image(self):
        img = np.empty(self.lib.vqae_classifier_image_floats(self.nat._h), np.float32)
        self.L.check(self.lib.vqae_classifier_image(self.nat._h, img.ctypes.data, None))
        return img

    def close(self):
        self.lib.vqae_classifier_optim_destroy(self.h)
        self.nat.close()


def held_to_yardstick(test, what, got, truth, ref32, ws):
    """got = (p, m, v) of the device; truth / ref32 the fp64 / fp32 runs: each of p, m, v within 2 x its yardstick"""
    zero = [np.zeros_like(w) for w in ws]
    figs = {}
    for name, a, t, r, start in zip(("p", "exp_avg", "exp_avg_sq"), got, truth, ref32, (ws, zero, zero)):
        figs[name] = (G.measure(a, t, start), G.measure(r, t, start))
    record_parity(test, case=what, **{k: {"device": d, "yardstick": y} for k, (d, y) in figs.items()})
    for name, (d, y) in figs.items():
        assert d <= 2 * y, f"{what} {name}: {d:.3e} from the fp64 run, the reference's own fp32 run {y:.3e}"


# ---- 1. trajectories ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_trajectory_fixture_variant(amd, ofx, case):
    ws, grads = G.problem()
    kind, wd, adaptive = CASES[case]
    d = Dev(amd, SMALL, ws, kind, wd, adaptive).run(grads)
    try:
        m, v, step = d.state()
        assert step == T
        truth, ref32 = ([[ofx[f"{case}/{n}{tag}_{i}"] for i in range(7)] for n in "pmv"] for tag in ("64", "32"))
        held_to_yardstick("classifier_optim_trajectory", case, (d.weights(), m, v), truth, ref32, ws)
    finally:
        d.close()


@pytest.mark.parametrize("case", ["adamw", "lamb", "asam_lamb"])
def test_trajectory_large_variant(amd, large, case):
    ws, grads = large
    kind, wd, adaptive = CASES[case]
    truth = run_mirror(amd, case, ws, grads, torch.float64)
    ref32 = run_mirror(amd, case, ws, grads, torch.float32)
    d = Dev(amd, LARGE, ws, kind, wd, adaptive).run(grads)
    try:
        m, v, step = d.state()
        assert step == T
        held_to_yardstick("classifier_optim_trajectory_large", case, (d.weights(), m, v), truth, ref32, ws)
    finally:
        d.close()


# ---- 2. / 3. the packed image is the weights; staleness ------------------------------------------------------------------------
def image_layout(K, E, C):
    """offset and PyTorch -> image packing of the seven blocks, as include/vqae_hip.h states them"""
    numel = (K * E, C * E * 9, C, C * C * 9, C, C * 9, 1)
    offs, o = [], 0
    for n in numel:
        offs.append(o)
        o += -(-n // 16) * 16
    return numel, offs, o


def pack_image(ws, K, E, C):
    numel, offs, total = image_layout(K, E, C)
    img = np.zeros(total, np.float32)
    for w, n, o in zip(ws, numel, offs):
        img[o:o + n] = (w.reshape(w.shape[0], -1).T if w.ndim == 4 else w).ravel()        # [cout][cin*9] -> [cin*9][cout]
    return img


def grid(K, seed=8):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.randint(0, K, (2, 37, 45)).astype(np.uint8 if K <= 256 else np.int32)).cuda()


@pytest.mark.parametrize("dims", [(256, 1, 8), (256, 1, 16), (2048, 8, 16)], ids=["E1C8", "E1C16", "E8C16"])
def test_image_is_the_weights_and_staleness(amd, dims):
    from vqae_amd.classifier import NativeClassifier
    K, E, C = dims
    ws, grads = G.problem(G.shapes_of(K, E, C), T, seed=3200 + C + E)
    codes = grid(K)
    d = Dev(amd, dims, ws, "lamb", 0.01, None)
    try:
        before = d.nat.forward(codes)[0].clone()
        d.run(grads)
        # (3a) a forward after the steps reads the stepped image, not a re-upload of the host copy ...
        after = d.nat.forward(codes)[0]
        stepped = d.weights()
        fresh = NativeClassifier(K, E, C, 1, Dev.named(stepped))
        want = fresh.forward(codes)[0]
        assert not torch.equal(after, before)
        assert torch.equal(after, want)                         # ... (2) bit-equal to a handle made from the downloaded weights
        img = d.image()
        assert np.array_equal(img, pack_image(stepped, K, E, C))                # the permutation, and the padding still 0
        numel, offs, total = image_layout(K, E, C)
        pad = np.ones(total, bool)
        for n, o in zip(numel, offs):
            pad[o:o + n] = False
        assert pad.sum() == total - sum(numel) and not img[pad].any()
        assert all(np.abs(a - b).max() > 0 for a, b in zip(stepped, ws))       # every tensor moved
        # (3b) vqae_classifier_update after a step wins
        other, _ = G.problem(G.shapes_of(K, E, C), 0, seed=77)
        other[2] = other[2] + 0.25
        d.nat.update(Dev.named(other))
        got_b = d.nat.forward(codes)[0]
        fresh_b = NativeClassifier(K, E, C, 1, Dev.named(other))
        assert torch.equal(got_b, fresh_b.forward(codes)[0])
        # (3c) ... and the next step continues from those weights with the moments and the step count kept
        extra = G.problem(G.shapes_of(K, E, C), 1, seed=78)[1][0]
        d.step(extra)
        torch.cuda.synchronize()
        m, v, step = d.state()
        assert step == T + 1
        res = {}
        for tag, dt in (("64", torch.float64), ("32", torch.float32)):
            ps = [torch.nn.Parameter(torch.from_numpy(w).to(dt).clone()) for w in ws]
            opt = mirror(amd, ps, "lamb", 0.01, None)
            for gs in grads + [extra]:
                if gs is extra:
                    for p, w in zip(ps, other):
                        p.data.copy_(torch.from_numpy(w))
                for p, g in zip(ps, gs):
                    p.grad = torch.from_numpy(g).to(dt)
                opt.step()
            res[tag] = ([p.detach().numpy() for p in ps], [opt.state[p]["exp_avg"].numpy() for p in ps],
                        [opt.state[p]["exp_avg_sq"].numpy() for p in ps])
        zero = [np.zeros_like(w) for w in ws]
        for name, a, start, i in (("p", d.weights(), other, 0), ("exp_avg", m, zero, 1), ("exp_avg_sq", v, zero, 2)):
            dev, yard = G.measure(a, res["64"][i], start), G.measure(res["32"][i], res["64"][i], start)
            record_parity("classifier_optim_update_then_step", dims=list(dims), what=name, device=dev, yardstick=yard)
            assert dev <= 2 * yard, (name, dev, yard)
        fresh.close()
        fresh_b.close()
    finally:
        d.close()


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [SMALL, LARGE], ids=["one_launch", "two_launches"])
@pytest.mark.parametrize("case", ["lamb", "asam_lamb", "sam_adamw"])
def test_two_runs_give_the_same_bits(amd, dims, case):
    ws, grads = G.problem(G.shapes_of(*dims), 6, seed=3300)
    kind, wd, adaptive = CASES[case]
    outs = []
    for _ in range(2):
        d = Dev(amd, dims, ws, kind, wd, adaptive).run(grads)
        try:
            m, v, _ = d.state()
            outs.append((d.weights(), m, v))
        finally:
            d.close()
    for a, b in zip(outs[0], outs[1]):
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------
def build_clf(K, E, C, seed=3400):
    from vqae_amd.classifier import CNNClassifier
    from vqae_amd.classifier_train import _params
    clf = CNNClassifier(K, E, C, 1)
    ws, _ = G.problem(G.shapes_of(K, E, C), 0, seed=seed)
    ws[2] = ws[2] + 0.1                                          # (biases away from 0: every gradient is alive)
    with torch.no_grad():
        for p, w in zip(_params(clf), ws):
            p.copy_(torch.from_numpy(w))
    return clf


@pytest.mark.parametrize("case", ["adamw", "lamb", "sam_adamw"])
def test_trainer_end_to_end(amd, case):
    from vqae_amd.classifier_train import _params, loss_and_grads, smooth_targets
    kind, wd, adaptive = CASES[case]
    steps = 8
    codes = grid(256)
    mask = torch.from_numpy(np.random.RandomState(9).randint(0, 3, (2, 37, 45)).astype(np.uint8)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(3)
    t1 = [smooth_targets(mask, 0.2, gen) for _ in range(steps)]
    t2 = [smooth_targets(mask, 0.2, gen) for _ in range(steps)]
    clf = build_clf(256, 1, 8)
    ws = [p.detach().numpy().copy() for p in _params(clf)]
    tr = make_trainer(amd, clf, kind, wd, adaptive)
    first = loss_and_grads(build_clf(256, 1, 8), codes, mask, pos_weight=POS_WEIGHT, target=t1[0])
    tr._ensure("cuda")
    seen, orig = [], tr.native.loss_grad

    def recording(*a, **k):                                       # the trainer's own gradients, as its optimiser reads them
        out = orig(*a, **k)
        seen.append(out[1].clone())
        return out

    tr.native.loss_grad = recording
    outs = [tr.step(codes, mask, pos_weight=POS_WEIGHT, target=t1[s], target2=t2[s]) for s in range(steps)]
    tr.native.loss_grad = orig
    assert all(loss.is_cuda and stats.is_cuda and loss.dtype == torch.float64 and tuple(stats.shape) == (2, 6) for loss, stats in outs)
    torch.cuda.synchronize()
    # the first step's return values are loss_and_grads' on the same weights, bit for bit (with SAM: the first pass)
    assert float(outs[0][0]) == first["loss_sum"]
    assert outs[0][1].sum(0).tolist()[:5] == [first[k] for k in ("tp", "fp", "fn", "tn", "n_valid")]
    passes = 2 if adaptive is not None else 1
    assert len(seen) == steps * passes
    cut = np.cumsum([w.size for w in ws])[:-1]
    rec = [[a.reshape(w.shape) for a, w in zip(np.split(g.cpu().numpy(), cut), ws)] for g in seen]
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        ps = [torch.nn.Parameter(torch.from_numpy(w).to(dt).clone()) for w in ws]
        opt = mirror(amd, ps, kind, wd, adaptive)
        for s in range(steps):
            for p, g in zip(ps, rec[s * passes]):
                p.grad = torch.from_numpy(g).to(dt)
            if adaptive is None:
                opt.step()
            else:
                opt.first_step()
                for p, g in zip(ps, rec[s * passes + 1]):
                    p.grad = torch.from_numpy(g).to(dt)
                opt.second_step()
        res[tag] = [p.detach().numpy() for p in ps]
    got = [w.numpy() for w in tr.weights()]
    dev, yard = G.measure(got, res["64"], ws), G.measure(res["32"], res["64"], ws)
    record_parity("classifier_optim_trainer", case=case, device=dev, yardstick=yard)
    assert dev <= 2 * yard, (case, dev, yard)
    # the module takes the weights on request only
    assert all(np.array_equal(p.detach().numpy(), w) for p, w in zip(_params(clf), ws))
    tr.sync_to_module()
    assert all(np.array_equal(p.detach().numpy(), w) for p, w in zip(_params(clf), got))
    assert torch.equal(clf(codes), tr.native.forward(codes)[0])
    tr.close()


# ---- 6. state round trip --------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_with_torch_adamw(amd, ofx):
    """Open loop on the fixture's gradients (the trainer's loss_grad is replaced by one that hands them out): 4 trainer steps
    -> state_dict -> torch.optim.AdamW for 4 more, and 4 AdamW steps -> load_state_dict -> 4 trainer steps, each against the
    fp64 trajectory of 8 steps, next to 8 trainer steps."""
    from vqae_amd.classifier_train import _params
    ws, grads = G.problem(steps=8)
    codes = grid(256)
    mask = torch.ones((2, 37, 45), dtype=torch.uint8, device="cuda")

    def trainer_with(clf, feed):
        tr = make_trainer(amd, clf, "adamw", 0.01, None)
        tr._ensure("cuda")
        orig = tr.native.loss_grad
        it = iter(feed)

        def fed(*a, **k):
            loss, g, stats = orig(*a, **k)
            return loss, Dev.pack(next(it)), stats

        tr.native.loss_grad = fed
        return tr

    def module():
        clf = build_clf(256, 1, 8)
        with torch.no_grad():
            for p, w in zip(_params(clf), ws):
                p.copy_(torch.from_numpy(w))
        return clf

    truth = G.run(lambda ps: torch.optim.AdamW(ps, **hyper("adamw", 0.01)), ws, grads, torch.float64, False)[0]
    ref32 = G.run(lambda ps: torch.optim.AdamW(ps, **hyper("adamw", 0.01)), ws, grads, torch.float32, False)[0]
    yard = G.measure(ref32, truth, ws)
    figs = {}
    # eight trainer steps
    tr = trainer_with(module(), grads)
    for _ in range(8):
        tr.step(codes, mask)
    figs["trainer"] = G.measure([w.numpy() for w in tr.weights()], truth, ws)
    tr.close()
    # trainer -> torch
    a = module()
    tr = trainer_with(a, grads[:4])
    for _ in range(4):
        tr.step(codes, mask)
    sd = tr.state_dict()
    assert float(sd["state"][0]["step"]) == 4 and tuple(sd["state"][3]["exp_avg"].shape) == (8, 8, 3, 3)
    tr.sync_to_module()
    tr.close()
    opt = torch.optim.AdamW(_params(a), lr=99.0)
    opt.load_state_dict(sd)
    for gs in grads[4:]:
        for p, g in zip(_params(a), gs):
            p.grad = torch.from_numpy(g).float()
        opt.step()
    figs["trainer_then_torch"] = G.measure([p.detach().numpy() for p in _params(a)], truth, ws)
    # torch -> trainer
    b = module()
    opt = torch.optim.AdamW(_params(b), **hyper("adamw", 0.01))
    for gs in grads[:4]:
        for p, g in zip(_params(b), gs):
            p.grad = torch.from_numpy(g).float()
        opt.step()
    tr = trainer_with(b, grads[4:])
    tr.hyper["lr"] = 99.0
    tr.load_state_dict(opt.state_dict())
    for _ in range(4):
        tr.step(codes, mask)
    figs["torch_then_trainer"] = G.measure([w.numpy() for w in tr.weights()], truth, ws)
    tr.close()
    record_parity("classifier_optim_state_round_trip", yardstick=yard, **figs)
    for k, v in figs.items():
        assert v <= 2 * yard, (k, v, yard)


# ---- 7. errors at run time ------------------------------------------------------------------------------------------------------------
def test_runtime_errors_and_non_finite_gradients(amd):
    ws, grads = G.problem(steps=2)
    plain = Dev(amd, SMALL, ws, "adamw", 0.01, None)
    sam = Dev(amd, SMALL, ws, "adamw", 0.01, False)
    try:
        lib = plain.lib
        g = Dev.pack(grads[0])
        assert lib.vqae_classifier_optim_sam_first(plain.h, g.data_ptr(), None) == -1          # created without SAM
        assert b"without SAM" in lib.vqae_last_error()
        assert lib.vqae_classifier_optim_step(plain.h, None, None) == -1                       # null gradients
        assert lib.vqae_classifier_optim_sam_first(sam.h, None, None) == -1
        assert lib.vqae_classifier_optim_sam_first(sam.h, g.data_ptr(), None) == 0
        assert lib.vqae_classifier_optim_sam_first(sam.h, g.data_ptr(), None) == -1            # twice in a row
        assert lib.vqae_classifier_optim_step(sam.h, g.data_ptr(), None) == 0
        assert lib.vqae_classifier_optim_sam_first(sam.h, g.data_ptr(), None) == 0             # ... and fine again after the step
        assert lib.vqae_classifier_optim_step(sam.h, g.data_ptr(), None) == 0
        bad = plain.L.ClassifierOptimConfig(2, LR, 0.9, 0.999, 1e-8, 0.01, -1.0, 0)
        assert lib.vqae_classifier_optim_set(plain.h, ctypes.byref(bad)) == -1                 # the kind does not change
        # a non-finite gradient is not an error: it propagates into its own element, as in torch
        gs = [x.copy() for x in grads[1]]
        gs[3][2, 1, 0, 2] = np.nan
        gs[0][5, 0] = np.inf
        plain.step(gs)
        torch.cuda.synchronize()
        w = plain.weights()
        assert np.isnan(w[3][2, 1, 0, 2]) and np.isnan(w[0][5, 0])
        w[3][2, 1, 0, 2] = 0.0
        w[0][5, 0] = 0.0
        assert all(np.isfinite(x).all() for x in w)
    finally:
        plain.close()
        sam.close()
