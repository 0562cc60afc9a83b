"""CPU: the fused multi-tensor optimisers (FusedAdam / FusedAdamW / FusedLamb, SAM over them) on CPU tensors, where they run
torch's Adam / AdamW and the `Lamb` mirror, against the reference's recorded trajectories; the create-time validation of the C
ABI (vqae_optim_*) without a GPU; the Python errors; state_dict round trips with `Lamb` and torch.optim.AdamW.

tests/golden/optim_multi.npz holds what the reference's own vq_ae.optim.lamb.Lamb, vq_ae.optim.sam.SAM and torch's Adam / AdamW
gave after T = 8 steps on eleven tensors shaped like an auto-encoder's parameter list, in fp32 and in fp64, see
tests/golden/make_optim_golden.py (whose `problem()` regenerates weights and gradients here).  Measure and bars are those of
test_classifier_optim_cpu.py: fp64 runs retrace the record to 1e-12 of its largest value, fp32 runs lie within 2 x the
reference's own fp32 distance to the fp64 record.  No kernel is launched here; test_optim_multi_gpu.py imports the helpers."""
import copy
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_optim_golden as G  # noqa: E402   (problem(), measure(), the case table; imports no reference code)

CASES = G.CASES
LR, RHO, T = G.LR, G.RHO, G.T
N = len(G.SHAPES)


@pytest.fixture(scope="module")
def mfx():
    return load_golden("optim_multi")


def hyper(kind, wd, lr=LR):
    return dict(lr=lr, betas=(0.9, 0.999), eps=G.EPS[kind], weight_decay=wd)


def fused(amd, ps, kind, wd, adaptive, how="class"):
    """The fused optimiser of a case: FusedAdam / FusedAdamW / FusedLamb, or SAM around one (by class or by conf dict)."""
    from vqae_amd.optim import SAM, FusedAdam, FusedAdamW, FusedLamb
    cls = {"adam": FusedAdam, "adamw": FusedAdamW, "lamb": FusedLamb}[kind]
    if adaptive is None:
        return cls(ps, **hyper(kind, wd))
    if how == "conf":
        return SAM(ps, dict(hyper(kind, wd), _target_="vqae_amd.optim." + cls.__name__, params=None), rho=RHO, adaptive=adaptive)
    if how == "factory":
        return SAM(ps, lambda groups, **kw: cls(groups, **kw), rho=RHO, adaptive=adaptive, **hyper(kind, wd))
    return SAM(ps, cls, rho=RHO, adaptive=adaptive, **hyper(kind, wd))


def mirror(amd, ps, kind, wd, adaptive, lr=LR):
    """The torch-side optimiser of a case: torch.optim.Adam / AdamW, the Lamb mirror, or the SAM mirror around one."""
    from vqae_amd.optim import SAM, Lamb
    cls = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "lamb": Lamb}[kind]
    if adaptive is None:
        return cls(ps, **hyper(kind, wd, lr))
    return SAM(ps, cls, rho=RHO, adaptive=adaptive, **hyper(kind, wd, lr))


def record(mfx, case, tag):
    return [[mfx[f"{case}/{n}{tag}_{i}"] for i in range(N)] for n in "pmv"]


def test_fixture_matches_its_problem(mfx):
    ws, grads = G.problem()
    assert [str(c) for c in mfx["cases"]] == list(CASES) and int(mfx["T"]) == T == len(grads)
    assert [tuple(w.shape) for w in ws] == list(G.SHAPES) and sum(w.size for w in ws) == 2064
    for i, w in enumerate(ws):
        assert np.array_equal(mfx[f"w_{i}"], w)
    assert ws[0][0] == 0 and ws[1][0] == 1 and ws[2][0] == np.float32(0.3) and not ws[4].any()
    assert not any(g[8][128:].any() for g in grads) and all(g[8][:128].all() for g in grads)
    zero = [np.zeros_like(w) for w in ws]
    for case in CASES:                                            # the yardsticks are alive for p, m and v
        for a, b, start in zip(record(mfx, case, "32"), record(mfx, case, "64"), (ws, zero, zero)):
            assert G.measure(a, b, start) > 0


@pytest.mark.parametrize("case,how", [(c, h) for c in CASES for h in (("class", "conf", "factory") if CASES[c][2] is not None
                                                                         else ("class",))])
def test_cpu_path_retraces_reference_fp64(amd, mfx, case, how):
    kind, wd, adaptive = CASES[case]
    ws, grads = G.problem()
    got = G.run(lambda ps: fused(amd, ps, kind, wd, adaptive, how), ws, grads, torch.float64, adaptive is not None)
    for name, arrs, want in zip("pmv", got, record(mfx, case, "64")):
        for i, (a, w) in enumerate(zip(arrs, want)):
            assert a.dtype == np.float64 and a.shape == w.shape
            assert np.abs(a - w).max() <= 1e-12 * max(np.abs(w).max(), 1e-300), (case, name, i)
    assert abs(got[0][0][0]) > 0                                  # the bias that started at 0 moved: trust ratio 1


@pytest.mark.parametrize("case", list(CASES))
def test_cpu_path_fp32_within_the_yardstick(amd, mfx, case):
    kind, wd, adaptive = CASES[case]
    ws, grads = G.problem()
    got = G.run(lambda ps: fused(amd, ps, kind, wd, adaptive), ws, grads, torch.float32, adaptive is not None)
    zero = [np.zeros_like(w) for w in ws]
    for name, a, t, r, start in zip("pmv", got, record(mfx, case, "64"), record(mfx, case, "32"), (ws, zero, zero)):
        d, y = G.measure(a, t, start), G.measure(r, t, start)
        assert d <= 2 * y, (case, name, d, y)


def test_resolve_inside_sam_conf(amd):
    from vqae_amd.optim import SAM, FusedAdamW, FusedLamb, _resolve
    assert _resolve("vqae_amd.optim.FusedLamb") is FusedLamb and _resolve("vqae_amd.optim.FusedAdamW") is FusedAdamW
    assert amd.FusedLamb is FusedLamb and amd.FusedAdam is amd.optim.FusedAdam
    p = [torch.nn.Parameter(torch.ones(3))]
    s = SAM(p, {"_target_": "vqae_amd.optim.FusedLamb", "lr": 1e-2, "betas": [0.9, 0.99], "params": None}, rho=0.1, adaptive=True)
    assert isinstance(s.base_optimizer, FusedLamb) and s.param_groups is s.base_optimizer.param_groups
    g = s.param_groups[0]
    assert g["rho"] == 0.1 and g["adaptive"] and g["betas"] == (0.9, 0.99) and g["eps"] == 1e-6
    cfg = s.base_optimizer._configs()[0]                          # rho and adaptive reach the C ABI from the groups
    assert (cfg.kind, cfg.sam_rho, cfg.sam_adaptive, cfg.beta2) == (2, 0.1, 1, 0.99)
    assert FusedLamb(p)._configs()[0].sam_rho == -1.0


# ---- the C ABI, before any HIP call --------------------------------------------------------------------------------------------
def test_abi_validation_without_gpu(amd):
    L = amd._lib
    lib = L.lib()
    names = ("vqae_optim_create", "vqae_optim_destroy", "vqae_optim_set", "vqae_optim_step", "vqae_optim_sam_first",
             "vqae_optim_export", "vqae_optim_import")
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "vqae_hip.h")).read()
    for name in names:
        assert name in L.SYMBOLS and getattr(lib, name) and name + "(" in header, name
    assert f"VQAE_OPTIM_CHUNK = {L.OPTIM_CHUNK}" in header and f"VQAE_OPTIM_SMALL = {L.OPTIM_SMALL}" in header
    assert L.OPTIM_CHUNK % 4 == 0 and L.OPTIM_SMALL == 64

    def cfg(kind=2, lr=1e-3, b1=0.9, b2=0.999, eps=1e-6, wd=0.01, rho=-1.0, adaptive=0):
        return L.ClassifierOptimConfig(kind, lr, b1, b2, eps, wd, rho, adaptive)

    def create(numel=(1, 5, 70), group_of=(0, 0, 1), groups=None, n=None, ng=None, null=None):
        groups = [cfg(), cfg(lr=1e-2)] if groups is None else groups
        n = len(numel) if n is None else n
        ng = len(groups) if ng is None else ng
        o = ctypes.c_void_p()
        args = [n, (ctypes.c_int64 * len(numel))(*numel), (ctypes.c_int * len(group_of))(*group_of), ng,
                (L.ClassifierOptimConfig * len(groups))(*groups), ctypes.byref(o)]
        if null is not None:
            args[null] = None
        rc = lib.vqae_optim_create(*args)
        assert not o.value
        return rc, lib.vqae_last_error()

    for null in (1, 2, 4, 5):
        assert create(null=null)[0] == -1
    rc, msg = create(n=0)
    assert rc == -1 and b"n_tensors" in msg
    rc, msg = create(numel=(1, 0, 70))
    assert rc == -1 and b"numel" in msg
    assert create(numel=(1, -3, 70))[0] == -1
    for bad in ((0, 2, 1), (0, -1, 1)):
        rc, msg = create(group_of=bad)
        assert rc == -1 and b"group" in msg
    words = {"kind": b"kind", "lr": b"learning rate", "eps": b"epsilon", "b1": b"beta", "b2": b"beta", "wd": b"weight_decay",
             "rho": b"rho"}
    for bad in (dict(kind=3), dict(kind=-1), dict(lr=-1e-3), dict(eps=-1e-8), dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0),
                dict(b2=-0.5), dict(wd=-0.01), dict(lr=float("nan")), dict(rho=float("nan"))):
        rc, msg = create(groups=[cfg(), cfg(**bad)])              # per group: the second one is checked too
        assert rc == -1 and words[next(iter(bad))] in msg, (bad, msg)
    rc, msg = create(groups=[cfg(kind=2), cfg(kind=1)])
    assert rc == -1 and b"kind" in msg
    rc, msg = create(groups=[cfg(rho=0.05), cfg()])
    assert rc == -1 and b"SAM" in msg
    rc, msg = create(numel=(2 ** 30, 2 ** 30, 5), group_of=(0, 0, 0))
    assert rc == -2 and b"2^31" in msg
    assert create(numel=(2 ** 31,), group_of=(0,))[0] == -2
    with pytest.raises(NotImplementedError):
        L.check(create(numel=(2 ** 31 - 1, 1), group_of=(0, 0))[0])
    # the other entry points refuse null handles and arrays before touching anything
    one = ctypes.c_void_p(16)                                     # never dereferenced: validation fails first
    arr = (ctypes.c_void_p * 1)(16)
    good = cfg()
    assert lib.vqae_optim_step(None, arr, arr, None) == -1
    assert lib.vqae_optim_sam_first(None, arr, arr, None) == -1
    assert lib.vqae_optim_set(None, ctypes.byref(good)) == -1
    assert lib.vqae_optim_export(None, one, one, (ctypes.c_int64 * 1)(), None) == -1
    assert lib.vqae_optim_import(None, one, one, (ctypes.c_int64 * 1)(), None) == -1
    assert b"null" in lib.vqae_last_error()
    lib.vqae_optim_destroy(None)


# ---- the Python errors -----------------------------------------------------------------------------------------------------------
def test_constructor_defaults_and_errors(amd):
    from vqae_amd.optim import SAM, FusedAdam, FusedAdamW, FusedLamb, Lamb
    p = [torch.nn.Parameter(torch.ones(3))]
    keys = ("lr", "betas", "eps", "weight_decay")
    for cls, ref in ((FusedAdam, torch.optim.Adam), (FusedAdamW, torch.optim.AdamW), (FusedLamb, Lamb)):
        assert {k: cls(p).defaults[k] for k in keys} == {k: ref(p).defaults[k] for k in keys}
        for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1))):
            with pytest.raises(ValueError):
                cls(p, **bad)
            with pytest.raises(ValueError):
                ref(p, **bad)
        with pytest.raises(TypeError):
            cls([torch.nn.Parameter(torch.ones(3, dtype=torch.float16))])
        with pytest.raises(ValueError):
            cls([torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(3, device="meta"))])
    assert set(FusedAdamW(p).param_groups[0]) == set(torch.optim.AdamW(p).param_groups[0])
    assert FusedAdamW(p).param_groups[0]["decoupled_weight_decay"] and not FusedAdam(p).param_groups[0]["decoupled_weight_decay"]
    for cls in (FusedAdam, FusedAdamW):
        with pytest.raises(ValueError):
            cls(p, weight_decay=-1.0)
        for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
            with pytest.raises(NotImplementedError):
                cls(p, **{flag: True})
        opt = cls(p)
        opt.param_groups[0]["amsgrad"] = True                     # (what a loaded state_dict could bring)
        p[0].grad = torch.ones(3)
        with pytest.raises(NotImplementedError):
            opt.step()
    with pytest.raises(ValueError):
        SAM(p, FusedLamb, rho=-1.0)
    for cls in (FusedAdamW, FusedLamb):                           # sparse gradients: as torch and the mirror raise
        e = torch.nn.Parameter(torch.ones(4, 2))
        opt = cls([e])
        e.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.ones(1, 2), (4, 2))
        with pytest.raises(RuntimeError):
            opt.step()


# ---- state ---------------------------------------------------------------------------------------------------------------------
def _feed(ps, gs, dtype=torch.float32):
    for p, g in zip(ps, gs):
        p.grad = torch.from_numpy(g).to(dtype)


@pytest.mark.parametrize("kind", ["lamb", "adamw"])
def test_state_dict_round_trips_with_the_torch_side(amd, kind):
    """4 fused steps -> state_dict -> Lamb / torch.optim.AdamW for 4 more, and the other way round: both bit-equal to 8 steps
    of the torch side alone (on CPU tensors the fused classes run that very code)."""
    ws, grads = G.problem()

    def params():
        return [torch.nn.Parameter(torch.from_numpy(w).clone()) for w in ws]

    def steps(opt, ps, which):
        for gs in which:
            _feed(ps, gs)
            opt.step()

    ref = params()
    steps(mirror(amd, ref, kind, 0.01, None), ref, grads)
    for first, second in ((fused, mirror), (mirror, fused)):
        ps = params()
        a = first(amd, ps, kind, 0.01, None)
        steps(a, ps, grads[:4])
        sd = a.state_dict()
        assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == list(range(N))
        assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"] and float(sd["state"][9]["step"]) == 4
        assert tuple(sd["state"][9]["exp_avg"].shape) == (8, 8, 3, 3)
        assert isinstance(sd["state"][0]["step"], int) == (kind == "lamb")
        b = second(amd, ps, kind, 0.5, None) if second is fused else mirror(amd, ps, kind, 0.5, None, lr=99.0)
        b.load_state_dict(sd)
        assert b.param_groups[0]["lr"] == LR and b.param_groups[0]["weight_decay"] == 0.01
        steps(b, ps, grads[4:])
        for p, q in zip(ps, ref):
            assert torch.equal(p.detach(), q.detach())


def test_deepcopy_pickle_and_add_param_group(amd):
    from vqae_amd.optim import FusedLamb
    ws, grads = G.problem()
    ps = [torch.nn.Parameter(torch.from_numpy(w).clone()) for w in ws]
    opt = FusedLamb(ps[:6], **hyper("lamb", 0.01))
    _feed(ps, grads[0])
    opt.step()
    opt.add_param_group(dict(params=ps[6:], lr=0.5 * LR))          # the state of the first six is kept
    assert len(opt.param_groups) == 2 and opt.state_dict()["state"][5]["step"] == 1
    _feed(ps, grads[1])
    opt.step()
    sd = opt.state_dict()
    assert [sd["state"][i]["step"] for i in (0, 5, 6, 10)] == [2, 2, 1, 1]
    twin = copy.deepcopy(opt)
    back = pickle.loads(pickle.dumps(opt))
    for other in (twin, back):
        assert type(other) is FusedLamb and other.param_groups[1]["lr"] == 0.5 * LR
        qs = [p for g in other.param_groups for p in g["params"]]
        assert all(q is not p and torch.equal(q, p) for q, p in zip(qs, ps))
        _feed(qs, grads[2])
        other.step()
    _feed(ps, grads[2])
    opt.step()
    for other in (twin, back):
        for q, p in zip([p for g in other.param_groups for p in g["params"]], ps):
            assert torch.equal(q.detach(), p.detach())
        assert other.state_dict()["state"][10]["step"] == 2


def test_none_gradients_on_the_cpu_path(amd):
    """What the GPU test holds the kernels to: a tensor without a gradient does not move and its step does not advance."""
    ws, grads = G.problem(steps=3)
    ps = [torch.nn.Parameter(torch.from_numpy(w).clone()) for w in ws]
    opt = fused(amd, ps, "lamb", 0.01, True)
    for s, gs in enumerate(grads):
        _feed(ps, gs)
        if s == 1:
            ps[1].grad = ps[9].grad = None
        before = [p.detach().clone() for p in ps]
        opt.first_step()
        opt.second_step()
        if s == 1:
            assert torch.equal(ps[1], before[1]) and torch.equal(ps[9], before[9]) and not torch.equal(ps[2], before[2])
    sd = opt.base_optimizer.state_dict()
    assert [sd["state"][i]["step"] for i in (0, 1, 9)] == [3, 2, 2]
