"""CPU: the optimisers of the slide classifier -- the Lamb and SAM mirrors against the reference's recorded trajectories, the
C ABI's create-time validation, ClassifierTrainer on CPU tensors against a hand-written loop of loss_and_grads + mirror, its
state_dict against torch.optim.AdamW, and train_hdf5 with a trainer / with the SAM mirror.

tests/golden/classifier_optim.npz holds what the reference's own vq_ae.optim.lamb.Lamb, vq_ae.optim.sam.SAM and torch's Adam /
AdamW gave after T = 16 steps on the shipped variant's seven tensors, in fp32 and in fp64, see
tests/golden/make_classifier_optim_golden.py (whose `problem()` regenerates weights and gradients here).  The accuracy measure
is, per tensor, ||dp_test - dp_64|| / ||dp_64|| with dp the change over the T steps, worst tensor; the yardstick of a case is
that measure for the reference's own fp32 run.  No kernel is launched here; test_classifier_optim_gpu.py imports the helpers."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_classifier_optim_golden as G  # noqa: E402   (problem(), measure(), the case table; imports no reference code)

CASES = G.CASES
LR, RHO, T = G.LR, G.RHO, G.T
POS_WEIGHT = 40.4858


@pytest.fixture(scope="module")
def ofx():
    return load_golden("classifier_optim")


@pytest.fixture(scope="module")
def tfx():
    return load_golden("classifier_train")


def hyper(kind, wd):
    return dict(lr=LR, betas=(0.9, 0.999), eps=G.EPS[kind], weight_decay=wd)


def mirror(amd, ps, kind, wd, adaptive, as_conf=False):
    """The torch-side optimiser of a case: torch.optim.Adam / AdamW, the Lamb mirror, or the SAM mirror around one."""
    from vqae_amd.optim import SAM, Lamb
    cls = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "lamb": Lamb}[kind]
    if adaptive is None:
        return cls(ps, **hyper(kind, wd))
    if as_conf:
        target = {"adam": "torch.optim.Adam", "adamw": "torch.optim.AdamW", "lamb": "vq_ae.optim.lamb.Lamb"}[kind]
        return SAM(ps, dict(hyper(kind, wd), _target_=target, params=None), rho=RHO, adaptive=adaptive)
    return SAM(ps, cls, rho=RHO, adaptive=adaptive, **hyper(kind, wd))


def run_mirror(amd, case, ws, grads, dtype, as_conf=False):
    kind, wd, adaptive = CASES[case]
    return G.run(lambda ps: mirror(amd, ps, kind, wd, adaptive, as_conf), ws, grads, dtype, adaptive is not None)


def test_fixture_matches_its_problem(ofx):
    ws, grads = G.problem()
    assert [str(c) for c in ofx["cases"]] == list(CASES) and int(ofx["T"]) == T == len(grads)
    for i, w in enumerate(ws):
        assert np.array_equal(ofx[f"w_{i}"], w)
    assert not ws[2].any() and not ws[4].any() and not ws[6].any()            # the zero-norm tensors
    assert not any(g[0][128:].any() for g in grads) and all(g[0][:128].all() for g in grads)


@pytest.mark.parametrize("case", list(CASES))
def test_mirrors_retrace_reference_fp64(amd, ofx, case):
    ws, grads = G.problem()
    got = run_mirror(amd, case, ws, grads, torch.float64, as_conf=True)
    for name, arrs in zip("pmv", got):
        for i, a in enumerate(arrs):
            want = ofx[f"{case}/{name}64_{i}"]
            assert a.dtype == np.float64 and a.shape == want.shape
            assert np.abs(a - want).max() <= 1e-12 * np.abs(want).max(), (case, name, i)
    # the biases started at 0 and moved: LAMB's trust ratio 1 branch was taken on the first step
    assert np.abs(got[0][2]).min() > 0
    # rows 128 .. 255 of the table saw no gradient: no momentum, decay (or nothing) only -- but for Adam, whose decay IS gradient
    assert case == "adam" or (not got[1][0][128:].any() and not got[2][0][128:].any())


def test_mirror_fp32_is_the_yardstick(amd, ofx):
    """The mirrors in fp32 give the reference's own fp32 run (same ops, same order) on this build of torch, to rounding."""
    ws, grads = G.problem()
    for case in CASES:
        got = run_mirror(amd, case, ws, grads, torch.float32)
        truth = [ofx[f"{case}/p64_{i}"] for i in range(7)]
        ref = G.measure([ofx[f"{case}/p32_{i}"] for i in range(7)], truth, ws)
        assert G.measure(got[0], truth, ws) <= 2 * ref, case


def test_sam_constructor_forms(amd):
    from vqae_amd.optim import SAM, Lamb
    p = [torch.nn.Parameter(torch.ones(3))]
    a = SAM(p, {"_target_": "vq_ae.optim.lamb.Lamb", "lr": 1e-2, "betas": [0.9, 0.99], "params": None}, rho=0.1, adaptive=True)
    assert isinstance(a.base_optimizer, Lamb) and a.param_groups is a.base_optimizer.param_groups
    assert a.param_groups[0]["rho"] == 0.1 and a.param_groups[0]["adaptive"] and a.param_groups[0]["betas"] == (0.9, 0.99)
    b = SAM(p, {"_target_": "torch.optim.SGD", "lr": 0.5}, lr=0.25)
    assert isinstance(b.base_optimizer, torch.optim.SGD) and b.param_groups[0]["lr"] == 0.25
    c = SAM(p, lambda groups, **kw: torch.optim.SGD(groups, **kw), lr=0.5)
    with pytest.raises(AssertionError):
        c.step()
    p[0].grad = torch.ones(3)

    def closure():
        assert float(p[0].data[0]) > 1.0                       # evaluated at the climbed point
        p[0].grad = torch.full((3,), 0.5)

    c.step(closure)                                            # back to w = 1, then SGD with the closure's gradient
    assert torch.equal(p[0].data, torch.full((3,), 0.75))
    with pytest.raises(ValueError):
        SAM(p, torch.optim.SGD, rho=-1.0, lr=0.1)
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1))):
        with pytest.raises(ValueError):
            Lamb(p, **bad)


# ---- the C ABI, before any HIP call ------------------------------------------------------------------------------------------
def test_abi_create_validation_without_gpu(amd):
    from test_classifier_cpu import _tensors
    L = amd._lib
    lib = L.lib()
    names = ("vqae_classifier_optim_create", "vqae_classifier_optim_destroy", "vqae_classifier_optim_set", "vqae_classifier_optim_step",
             "vqae_classifier_optim_sam_first", "vqae_classifier_download", "vqae_classifier_optim_export",
             "vqae_classifier_optim_import")
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "vqae_hip.h")).read()
    for name in names:
        assert name in L.SYMBOLS and getattr(lib, name) and name + "(" in header, name
    h, h3, o = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    keep, arr, n = _tensors(L)
    assert lib.vqae_classifier_create(256, 1, 8, 1, arr, n, ctypes.byref(h)) == 0
    keep3, arr3, n3 = _tensors(L, E=4, NO=3)
    assert lib.vqae_classifier_create(256, 4, 8, 3, arr3, n3, ctypes.byref(h3)) == 0
    one = ctypes.c_void_p(16)                     # never dereferenced: validation fails first
    try:
        def cfg(kind=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, rho=-1.0, adaptive=0):
            return L.ClassifierOptimConfig(kind, lr, b1, b2, eps, wd, rho, adaptive)

        create = lib.vqae_classifier_optim_create
        good = cfg()
        assert create(None, ctypes.byref(good), ctypes.byref(o)) == -1
        assert create(h, None, ctypes.byref(o)) == -1
        assert create(h, ctypes.byref(good), None) == -1
        for bad in (dict(kind=3), dict(kind=-1), dict(lr=-1e-3), dict(eps=-1e-8), dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0),
                    dict(b2=-0.5), dict(wd=-0.01), dict(lr=float("nan")), dict(rho=float("nan"))):
            c = cfg(**bad)
            assert create(h, ctypes.byref(c), ctypes.byref(o)) == -1 and not o.value, bad
        assert b"beta" in lib.vqae_last_error() or b"rho" in lib.vqae_last_error()
        assert create(h3, ctypes.byref(good), ctypes.byref(o)) == -2 and not o.value            # n_out != 1
        assert b"n_out" in lib.vqae_last_error()
        with pytest.raises(NotImplementedError):
            L.check(create(h3, ctypes.byref(good), ctypes.byref(o)))
        # the other entry points refuse null handles before touching anything
        assert lib.vqae_classifier_optim_step(None, one, None) == -1
        assert lib.vqae_classifier_optim_sam_first(None, one, None) == -1
        assert lib.vqae_classifier_optim_set(None, ctypes.byref(good)) == -1
        assert lib.vqae_classifier_optim_export(None, one, one, None, None) == -1
        assert lib.vqae_classifier_optim_import(None, one, one, 0, None) == -1
        assert lib.vqae_classifier_download(None, None, None) == -1
        lib.vqae_classifier_optim_destroy(None)
        # download without a device: the host image, un-permuted (no HIP call)
        outs = [np.zeros(k, np.float32) for k in (256, 72, 8, 576, 8, 72, 1)]
        ptrs = (ctypes.c_void_p * 7)(*[a.ctypes.data for a in outs])
        assert lib.vqae_classifier_download(h, ptrs, None) == 0
        assert all((a == 1).all() for a in outs)
    finally:
        lib.vqae_classifier_destroy(h)
        lib.vqae_classifier_destroy(h3)


def test_download_inverts_the_packing_without_gpu(amd, tfx):
    from test_classifier_train_cpu import build
    from vqae_amd.classifier import NativeClassifier
    from vqae_amd.classifier_train import _params
    L = amd._lib
    for variant in ("E1C8O1", "E1C16O1", "E4C8O1"):
        clf = build(tfx, variant)
        ls = clf.layers
        dims = (256, ls.embedding.embedding_dim, ls.in_conv.out_channels, 1)
        nat = NativeClassifier(*dims, {"layers." + n: p for n, p in ls.named_parameters()})
        outs = [np.zeros(tuple(p.shape), np.float32) for p in _params(clf)]
        ptrs = (ctypes.c_void_p * 7)(*[a.ctypes.data for a in outs])
        L.check(L.lib().vqae_classifier_download(nat._h, ptrs, None))
        for a, p in zip(outs, _params(clf)):
            assert np.array_equal(a, p.detach().numpy()), variant
        nat.close()


# ---- ClassifierTrainer on CPU tensors ------------------------------------------------------------------------------------------
TRAINER_CASES = {"adamw": ("adamw", 0.01, None), "lamb": ("lamb", 0.01, None), "sam_adamw": ("adamw", 0.01, False),
                 "asam_lamb": ("lamb", 0.01, True)}


def make_trainer(amd, clf, kind, wd, adaptive, device=None):
    from vqae_amd.optim import ClassifierTrainer
    return ClassifierTrainer(clf, kind, sam_rho=None if adaptive is None else RHO, sam_adaptive=bool(adaptive), device=device,
                             **hyper(kind, wd))


def hand_loop(amd, clf, kind, wd, adaptive, batches, steps, targets=None, targets2=None):
    """loss_and_grads + mirror on `clf` itself, cycling through `batches` -> the first-pass result dict of every step"""
    from vqae_amd.classifier_train import _params, loss_and_grads
    opt = mirror(amd, _params(clf), kind, wd, adaptive)
    out = []
    for s in range(steps):
        codes, mask = batches[s % len(batches)]
        t1 = None if targets is None else targets[s]
        t2 = t1 if targets2 is None else targets2[s]
        out.append(loss_and_grads(clf, codes, mask, pos_weight=POS_WEIGHT, target=t1))
        if adaptive is None:
            opt.step()
        else:
            opt.first_step(zero_grad=True)
            loss_and_grads(clf, codes, mask, pos_weight=POS_WEIGHT, target=t2)
            opt.second_step(zero_grad=True)
    return out, opt


@pytest.mark.parametrize("case", list(TRAINER_CASES))
def test_trainer_cpu_equals_hand_loop(amd, tfx, case):
    from test_classifier_train_cpu import build
    from vqae_amd.classifier_train import _params, smooth_targets
    kind, wd, adaptive = TRAINER_CASES[case]
    codes = torch.from_numpy(tfx["codes_2x7x5"])
    mask = torch.from_numpy(tfx["mask_2x7x5"])
    gen = torch.Generator().manual_seed(5)
    t1 = [smooth_targets(mask, 0.3, gen) for _ in range(4)]
    t2 = [smooth_targets(mask, 0.3, gen) for _ in range(4)]
    clf, twin = build(tfx, "E1C8O1"), build(tfx, "E1C8O1")
    before = [p.detach().clone() for p in _params(clf)]
    tr = make_trainer(amd, clf, kind, wd, adaptive)
    assert tr.device is None
    got = [tr.step(codes, mask, pos_weight=POS_WEIGHT, target=t1[s], target2=t2[s], check=True) for s in range(4)]
    assert tr.device == "cpu"
    want, _ = hand_loop(amd, twin, kind, wd, adaptive, [(codes, mask)], 4, t1, t2)
    for (loss, stats), w in zip(got, want):
        assert loss.dtype == torch.float64 and tuple(loss.shape) == (1,) and tuple(stats.shape) == (1, 6)
        assert float(loss) == w["loss_sum"]                                     # SAM: the FIRST pass's loss
        assert stats[0].tolist() == [w["tp"], w["fp"], w["fn"], w["tn"], w["n_valid"], w["loss_sum"]]
    for p, b in zip(_params(clf), before):
        assert torch.equal(p, b)                                                # the module is the trainer's only on request
    for w, q in zip(tr.weights(), _params(twin)):
        assert torch.equal(w, q.detach())
    assert tr.sync_to_module() is clf
    for p, q in zip(_params(clf), _params(twin)):
        assert torch.equal(p, q)
    with pytest.raises(ValueError):
        tr.step(codes, mask[:, :3], pos_weight=POS_WEIGHT)
    with pytest.raises(ValueError):
        tr.step(codes, mask + 2, pos_weight=POS_WEIGHT, check=True)


def test_trainer_arguments(amd, tfx):
    from test_classifier_train_cpu import build
    from vqae_amd.optim import ClassifierTrainer
    clf = build(tfx, "E1C8O1")
    for bad in (dict(optimizer="sgd"), dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(weight_decay=-1.0),
                dict(sam_rho=-0.1)):
        with pytest.raises(ValueError):
            ClassifierTrainer(clf, **bad)
    assert ClassifierTrainer(clf, "adamw").hyper == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    assert ClassifierTrainer(clf, "lamb").hyper == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0)
    tr = ClassifierTrainer(clf, "lamb", device="cpu")
    tr.set_lr(0.5)
    assert tr._opt.param_groups[0]["lr"] == 0.5 and tr.state_dict()["param_groups"][0]["lr"] == 0.5
    with pytest.raises(ValueError):
        tr.set_lr(-1.0)


def test_trainer_state_dict_round_trips_with_torch_adamw(amd, tfx):
    from test_classifier_train_cpu import build
    from vqae_amd.classifier_train import _params, loss_and_grads
    codes = torch.from_numpy(tfx["codes_2x7x5"])
    mask = torch.from_numpy(tfx["mask_2x7x5"])
    # eight trainer steps ...
    ref = build(tfx, "E1C8O1")
    tr8 = make_trainer(amd, ref, "adamw", 0.01, None, device="cpu")
    for _ in range(8):
        tr8.step(codes, mask, pos_weight=POS_WEIGHT)
    want = tr8.weights()
    # ... equal four trainer steps, then four of torch.optim.AdamW from the trainer's state_dict ...
    a = build(tfx, "E1C8O1")
    tr = make_trainer(amd, a, "adamw", 0.01, None, device="cpu")
    for _ in range(4):
        tr.step(codes, mask, pos_weight=POS_WEIGHT)
    sd = tr.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == list(range(7))
    assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"] and float(sd["state"][3]["step"]) == 4
    assert sd["param_groups"][0]["params"] == list(range(7)) and sd["param_groups"][0]["lr"] == LR
    tr.sync_to_module()
    opt = torch.optim.AdamW(_params(a), lr=123.0)
    opt.load_state_dict(sd)
    for _ in range(4):
        loss_and_grads(a, codes, mask, pos_weight=POS_WEIGHT)
        opt.step()
    for p, w in zip(_params(a), want):
        assert torch.equal(p.detach(), w)
    # ... and four of torch.optim.AdamW, then four trainer steps from ITS state_dict (loaded before the first step)
    b = build(tfx, "E1C8O1")
    opt = torch.optim.AdamW(_params(b), **hyper("adamw", 0.01))
    for _ in range(4):
        loss_and_grads(b, codes, mask, pos_weight=POS_WEIGHT)
        opt.step()
    tr = make_trainer(amd, b, "adamw", 0.5, None)
    tr.load_state_dict(opt.state_dict())
    assert tr.hyper["weight_decay"] == 0.01 and float(tr.state_dict()["state"][6]["step"]) == 4
    for _ in range(4):
        tr.step(codes, mask, pos_weight=POS_WEIGHT)
    for w, v in zip(tr.weights(), want):
        assert torch.equal(w, v)
    with pytest.raises(ValueError):
        tr.load_state_dict({"state": {}, "param_groups": [dict(sd["param_groups"][0], params=[0, 1])]})


def three_slide_groups(seed=6):
    rs = np.random.RandomState(seed)
    shapes = {"normal_001": (12, 15), "tumor_001": (14, 11), "normal_002": (9, 13)}
    return {"images": {k: rs.randint(0, 256, s).astype(np.uint8) for k, s in shapes.items()},
            "masks": {k + "_mask": rs.randint(0, 3, s).astype(np.uint8) for k, s in shapes.items()}}


@pytest.mark.parametrize("how", ["trainer", "trainer_sam", "sam_mirror"])
def test_train_hdf5_with_trainer_and_sam_cpu(amd, tfx, tmp_path, how):
    """normal_001 + tumor_001 train as one batch per epoch, normal_002 validates; label smoothing draws one target per pass."""
    from test_classifier_train_cpu import build
    from vqae_amd import hdf5
    from vqae_amd.classifier_train import (_params, collate_random_crop, loss_and_grads, smooth_targets, torch_loss_grad,
                                           train_hdf5)
    groups = three_slide_groups()
    path = hdf5.write_hdf5(tmp_path / "enc.hdf5", groups)
    seed, ls, epochs = 13, 0.2, 3
    kind, wd, adaptive = ("lamb", 0.01, None) if how == "trainer" else ("adamw", 0.01, False)
    clf, twin = build(tfx, "E1C8O1"), build(tfx, "E1C8O1")
    kw = dict(epochs=epochs, batch_size=2, train_frac=0.5, pos_weight=POS_WEIGHT, seed=seed, label_smoothing=ls, forward_fn=clf)
    if how == "sam_mirror":
        hist = train_hdf5(clf, path, mirror(amd, _params(clf), kind, wd, adaptive), grad_fn=torch_loss_grad, **kw)
    else:
        tr = make_trainer(amd, clf, kind, wd, adaptive, device="cpu")
        hist = train_hdf5(clf, path, tr, **kw)
        with pytest.raises(ValueError):
            train_hdf5(twin, path, tr, **kw)                                    # a trainer of another module
    rng = np.random.RandomState(seed)
    gen = torch.Generator().manual_seed(seed)
    opt = mirror(amd, _params(twin), kind, wd, adaptive)
    pair = [(groups["images"][k], groups["masks"][k + "_mask"]) for k in ("normal_001", "tumor_001")]
    for ep in range(epochs):
        codes, mask = collate_random_crop(pair, rng)
        mask = mask.to(torch.uint8)
        want = loss_and_grads(twin, codes, mask, pos_weight=POS_WEIGHT, target=smooth_targets(mask, ls, gen))
        if adaptive is None:
            opt.step()
        else:
            opt.first_step(zero_grad=True)
            loss_and_grads(twin, codes, mask, pos_weight=POS_WEIGHT, target=smooth_targets(mask, ls, gen))
            opt.second_step(zero_grad=True)
        step, = hist[ep]["steps"]
        assert step["stems"] == ["normal_001", "tumor_001"] and step["shape"] == tuple(codes.shape)
        assert {k: step[k] for k in want} == want, (ep, step, want)
        assert hist[ep]["train"]["loss"] == want["loss_sum"] / want["n_valid"]
    for p, q in zip(_params(clf), _params(twin)):
        assert torch.equal(p, q)                                                # the module holds the trained weights
    assert hist[-1]["val"]["n_valid"] == int((groups["masks"]["normal_002_mask"] != 0).sum())
