"""CPU: the multi-class route of the slide classifier -- nn.CrossEntropyLoss over the stored mask bytes as class indices.

tests/golden/classifier_ce.npz holds what the reference's own CNNClassifier.step + torch.nn.CrossEntropyLoss + autograd gave
in fp32 and (after .double()) in fp64, see tests/golden/make_classifier_ce_golden.py.  The accuracy measure is
test_classifier_train_cpu's: e(G) = max over the seven tensors of max|G - G64| / max|G64|; e_ref of a variant is e of the
reference's own fp32 gradients, maximised over every recorded grid and case, and an fp32 evaluation that sums the same
products in another order may be 4 x e_ref away.  The loss may differ from fp64 by what a logit error e_logit allows:
-log p_c moves by at most 2 * e_logit under a logit perturbation of e_logit and the target distribution sums to 1, so
|loss_sum - loss_sum64| <= 2 * max(w) * e_logit * N + 1e-6 * |loss_sum64| (the second term is loss_bound's).
No kernel is launched here; test_classifier_ce_gpu.py imports the helpers below."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_classifier_train_cpu import e_of, grads_of, params

VARIANTS = {"E1C8O3": (1, 8, 3), "E1C16O2": (1, 16, 2), "E4C8O4": (4, 8, 4)}
GRIDS = ("2x7x5", "2x37x70", "4x64x96")
EXTRA_GRID = "2x37x70"
CASES = [(g, c) for g in GRIDS for c in ("ones_sum", "cam_mean")] + [(EXTRA_GRID, "cam_sum")]
CAM = [0.0, 0.0247, 0.9753]


@pytest.fixture(scope="module")
def cfx():
    return load_golden("classifier_ce")


def build(cfx, variant, dtype=torch.float32):
    from vqae_amd.classifier import CNNClassifier
    E, C, NO = VARIANTS[variant]
    m = CNNClassifier(256, E, C, NO)
    pre = variant + "/layers."
    m.load_state_dict({k[len(variant) + 1:]: torch.from_numpy(cfx[k]) for k in cfx.files if k.startswith(pre)}, strict=True)
    return m.to(dtype)


@pytest.fixture(scope="module")
def cmodels(cfx):
    return {v: build(cfx, v) for v in VARIANTS}


@pytest.fixture(scope="module")
def cmodels64(cfx):
    return {v: build(cfx, v, torch.float64) for v in VARIANTS}


def recorded(cfx, variant, grid, case, tag):
    return [cfx[f"{variant}/{grid}/{case}/g{tag}_{i}"] for i in range(7)]


def e_ref(cfx, variant):
    """e of the reference's own fp32 gradients, maximised over every recorded grid and case"""
    return max(e_of(recorded(cfx, variant, g, c, "32"), recorded(cfx, variant, g, c, "64")) for g, c in CASES)


def case_kw(cfx, variant, case):
    no = VARIANTS[variant][2]
    if case == "ones_sum":
        return dict(reduction="sum")
    return dict(class_weight=cfx[f"weight_{no}"].tolist(), label_smoothing=float(cfx["label_smoothing"]),
                reduction="mean" if case == "cam_mean" else "sum")


def case_inputs(cfx, variant, grid, case):
    no = VARIANTS[variant][2]
    return torch.from_numpy(cfx[f"codes_{grid}"]), torch.from_numpy(cfx[f"labels_{no}_{grid}"]), case_kw(cfx, variant, case)


def ce_loss_bound(class_weight, e_logit, n, loss_sum64):
    return 2.0 * (max(class_weight) if class_weight is not None else 1.0) * e_logit * n + 1e-6 * abs(loss_sum64)


def test_the_reference_weights_are_the_recorded_ones(cfx):
    assert cfx["weight_3"].tolist() == CAM and float(cfx["label_smoothing"]) == 0.001
    assert all(cfx[f"weight_{no}"][0] == 0 for no in (2, 3, 4))
    for v in VARIANTS:
        assert max(e_of(recorded(cfx, v, g, c, "32"), recorded(cfx, v, g, c, "64")) for g, c in CASES) == e_ref(cfx, v) > 0


# ---- the restatement against the reference's recorded logits, loss and gradients --------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_restatement_fp64_reproduces_the_reference(cfx, cmodels64, variant):
    from vqae_amd.classifier_train import ce_loss_and_grads
    m = cmodels64[variant]
    no = VARIANTS[variant][2]
    lg = m(torch.from_numpy(cfx["codes_2x7x5"]))
    want = cfx[f"{variant}/2x7x5/logits64"]
    assert lg.dtype == torch.float64 and float((lg - torch.from_numpy(want)).abs().max()) <= 1e-12 * np.abs(want).max()
    for grid, case in CASES:
        codes, labels, kw = case_inputs(cfx, variant, grid, case)
        res = ce_loss_and_grads(m, codes, labels, **kw)
        loss64 = float(cfx[f"{variant}/{grid}/{case}/loss64"])
        assert abs(res["loss"] - loss64) <= 1e-12 * abs(loss64), (variant, grid, case)
        assert all(p.grad.dtype == torch.float64 and p.grad.shape == p.shape for p in params(m))
        assert e_of(grads_of(m), recorded(cfx, variant, grid, case, "64")) <= 1e-12, (variant, grid, case)
        # the returned sums restate the loss: (1 - eps) * nll + (eps / NO) * smooth, over sum w[y] for 'mean'
        scale = res["weight_sum"] if kw["reduction"] == "mean" else 1.0
        assert abs(res["loss_sum"] / scale - loss64) <= 1e-12 * abs(loss64)
        assert res["confusion"].shape == (no, no) and int(res["confusion"].sum()) == labels.numel() and res["n_bad"] == 0
        w = kw.get("class_weight") or [1.0] * no
        cnt = np.bincount(labels.numpy().ravel(), minlength=no)
        assert abs(res["weight_sum"] - float(np.dot(cnt, w))) <= 1e-12 * max(1.0, res["weight_sum"])
        assert res["confusion"][0, 1:].sum() == 0 and res["confusion"][0, 0] == cnt[0]        # the background hack
        assert res["recall"][0] == 1.0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_restatement_fp32_within_the_bound(cfx, cmodels, cmodels64, variant):
    from vqae_amd.classifier_train import ce_loss_and_grads
    m = cmodels[variant]
    tol = 4 * e_ref(cfx, variant)
    for grid, case in CASES:
        codes, labels, kw = case_inputs(cfx, variant, grid, case)
        res = ce_loss_and_grads(m, codes, labels, **kw)
        assert all(p.grad.dtype == torch.float32 for p in params(m))
        e = e_of(grads_of(m), recorded(cfx, variant, grid, case, "64"))
        print(f"{variant} {grid} {case}: e = {e:.3e}, 4 e_ref = {tol:.3e}")
        assert e <= tol, (variant, grid, case, e, tol)
        e_logit = float((m(codes).double() - cmodels64[variant](codes)).abs().max())
        loss64 = float(cfx[f"{variant}/{grid}/{case}/loss64"])
        scale = res["weight_sum"] if kw["reduction"] == "mean" else 1.0
        assert abs(res["loss"] - loss64) * scale <= ce_loss_bound(kw.get("class_weight"), e_logit, labels.numel(), loss64 * scale)


def test_formulas_of_the_loss_and_its_logit_gradient():
    """The closed forms the kernel evaluates, against torch in fp64."""
    import torch.nn.functional as F
    torch.manual_seed(0)
    for no, w, eps in ((3, CAM, 0.001), (2, None, 0.0), (4, [0.0, 0.05, 0.25, 0.7], 0.3)):
        x = torch.randn(2, no, 5, 7, dtype=torch.float64, requires_grad=True)
        y = torch.randint(0, no, (2, 5, 7))
        wt = None if w is None else torch.tensor(w, dtype=torch.float64)
        loss = F.cross_entropy(x, y, weight=wt, label_smoothing=eps, reduction="sum")
        g, = torch.autograd.grad(loss, x)
        wv = torch.ones(no, dtype=torch.float64) if wt is None else wt
        p = torch.softmax(x.detach(), 1)
        lp = torch.log_softmax(x.detach(), 1)
        onehot = F.one_hot(y, no).movedim(-1, 1).double()
        wy = wv[y][:, None]
        nll = -(wy[:, 0] * lp.gather(1, y[:, None])[:, 0]).sum()
        smooth = -(lp * wv[None, :, None, None]).sum()
        assert abs(float(loss.detach()) - float((1 - eps) * nll + eps / no * smooth)) <= 1e-13 * float(loss.detach())
        want = (1 - eps) * wy * (p - onehot) + eps / no * (wv.sum() * p - wv[None, :, None, None])
        assert float((g - want).abs().max()) <= 1e-15
        mean = F.cross_entropy(x, y, weight=wt, label_smoothing=eps, reduction="mean")
        assert abs(float(mean.detach()) - float(loss.detach()) / float(wv[y].sum())) <= 1e-13 * abs(float(mean.detach()))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("vqae_classifier_ce_workspace_bytes", "vqae_classifier_forward_ce", "vqae_classifier_ce_train_workspace_bytes",
               "vqae_classifier_loss_grad_ce", "vqae_classifier_optim_create_ce")


def test_new_symbols_everywhere(amd):
    import os
    from conftest import ROOT
    L = amd._lib
    header = open(os.path.join(ROOT, "include", "vqae_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s in L.SYMBOLS and hasattr(L.lib(), s) and s + "(" in header, s
    assert "VQAE_CE_STATS_K = 20" in header and L.CE_STATS_K == 20
    assert (L.CE_WEIGHT_SUM, L.CE_NLL_SUM, L.CE_SMOOTH_SUM, L.CE_N_BAD) == (16, 17, 18, 19)


def _handle(L, E, C, NO, K=256):
    from test_classifier_cpu import _tensors
    keep, arr, n = _tensors(L, E=E, C=C, NO=NO, K=K)
    h = ctypes.c_void_p()
    assert L.lib().vqae_classifier_create(K, E, C, NO, arr, n, ctypes.byref(h)) == 0
    return h


def test_abi_argument_validation_without_gpu(amd):
    L = amd._lib
    lib = L.lib()
    INVALID, UNSUPPORTED = -1, -2
    one = ctypes.c_void_p(16)                     # never dereferenced: validation fails (or batch == 0 returns) first
    h1, h3 = _handle(L, 1, 8, 1), _handle(L, 4, 8, 3)
    U8 = L.IDX_U8
    w3 = (ctypes.c_float * 3)(*CAM)

    def wv(*v):
        return (ctypes.c_float * len(v))(*v)

    try:
        fwd = lib.vqae_classifier_forward_ce
        #   (c, codes, dt, B, h, w, logits, prob, class, labels, weight, eps, stats, ws, stream)
        assert fwd(None, one, U8, 1, 4, 4, one, None, None, None, None, 0.0, None, None, None) == INVALID      # null classifier
        assert fwd(h3, None, U8, 1, 4, 4, one, None, None, None, None, 0.0, None, None, None) == INVALID       # null codes
        assert fwd(h3, one, U8, 1, 4, 4, None, None, None, None, None, 0.0, None, None, None) == INVALID       # no output
        assert fwd(h3, one, U8, 1, 4, 4, None, None, None, one, w3, 0.0, None, one, None) == INVALID           # labels are no output
        assert fwd(h3, one, U8, 1, 4, 4, one, None, None, None, w3, 0.0, one, one, None) == INVALID            # stats without labels
        assert fwd(h3, one, U8, 1, 4, 4, one, None, None, one, w3, 0.0, one, None, None) == INVALID            # ... without workspace
        assert fwd(h3, one, 7, 1, 4, 4, one, None, None, None, None, 0.0, None, None, None) == INVALID         # bad dtype
        assert fwd(h3, one, U8, 1, 0, 4, one, None, None, None, None, 0.0, None, None, None) == INVALID        # h < 1
        assert fwd(h3, one, U8, 1, 4, 0, one, None, None, None, None, 0.0, None, None, None) == INVALID
        assert fwd(h3, one, U8, -1, 4, 4, one, None, None, None, None, 0.0, None, None, None) == INVALID
        for bad in (wv(0.0, -1.0, 1.0), wv(0.0, float("nan"), 1.0), wv(0.0, float("inf"), 1.0)):
            assert fwd(h3, one, U8, 1, 4, 4, None, None, one, None, bad, 0.0, None, None, None) == INVALID     # weight
        for eps in (-0.1, 1.5, float("nan")):
            assert fwd(h3, one, U8, 1, 4, 4, None, None, one, None, w3, eps, None, None, None) == INVALID      # label_smoothing
        assert fwd(h1, one, U8, 1, 4, 4, one, None, None, None, None, 0.0, None, None, None) == UNSUPPORTED    # n_out == 1
        assert b"n_out" in lib.vqae_last_error()
        assert fwd(h3, one, U8, 70000, 4, 4, one, None, None, None, None, 0.0, None, None, None) == UNSUPPORTED
        assert fwd(h3, one, U8, 0, 4, 4, one, one, one, one, w3, 1.0, one, one, None) == 0                     # empty batch
        ws = lib.vqae_classifier_ce_workspace_bytes
        assert ws(h3, 0, 4, 4) == 0 and ws(h3, 1, 0, 4) == 0 and ws(None, 1, 4, 4) == 0 and ws(h1, 1, 4, 4) == 0
        assert ws(h3, 1, 1, 1) >= 20 * 8 and ws(h3, 1, 1, 1) % 256 == 0
        assert ws(h3, 3, 6144, 12288) >= 3 * (6144 // 14) * (12288 // 62) * 20 * 8

        lg = lib.vqae_classifier_loss_grad_ce
        #  (c, codes, dt, B, h, w, labels, weight, eps, reduction, grads, stats, loss, ws, stream)
        ok = [h3, one, U8, 1, 4, 4, one, w3, 0.001, 1, one, one, one, one, None]
        for i in (0, 1, 6, 10, 11, 12, 13):                                      # each required pointer in turn
            args = list(ok)
            args[i] = None
            assert lg(*args) == INVALID, i
        for i, v in ((2, 7), (3, -1), (4, 0), (5, 0), (8, -0.5), (8, 1.01), (8, float("nan")), (9, 2), (9, -1),
                     (7, wv(1.0, 1.0, -2.0)), (7, wv(1.0, float("nan"), 1.0))):
            args = list(ok)
            args[i] = v
            assert lg(*args) == INVALID, (i, v)
        args = list(ok)
        args[0] = h1
        assert lg(*args) == UNSUPPORTED                                          # the BCE entry points own n_out == 1
        args = list(ok)
        args[3] = 70000
        assert lg(*args) == UNSUPPORTED
        tws = lib.vqae_classifier_ce_train_workspace_bytes
        assert tws(h3, 0, 4, 4) == 0 and tws(None, 1, 4, 4) == 0 and tws(h1, 1, 4, 4) == 0
        assert tws(h3, 2, 37, 70) >= ws(h3, 2, 37, 70) + 2 * 3 * 37 * 70 * 4 + 256 * 4 * 8

        # the entry points that were there keep their answers for n_out == 3, the new ones refuse n_out == 1
        assert lib.vqae_classifier_forward(h3, one, U8, 1, 4, 4, one, one, None, 1.0, None, None, None) == INVALID
        assert lib.vqae_classifier_forward(h3, one, U8, 1, 4, 4, one, None, one, 1.0, one, one, None) == INVALID
        assert lib.vqae_classifier_loss_grad(h3, one, U8, 1, 4, 4, one, None, 1.0, 0, one, one, one, one, None) == UNSUPPORTED
        assert lib.vqae_classifier_train_workspace_bytes(h3, 1, 4, 4) == 0
        cfg = L.ClassifierOptimConfig(L.OPTIM_KINDS["adamw"], 1e-3, 0.9, 0.999, 1e-8, 0.01, -1.0, 0)
        o = ctypes.c_void_p()
        assert lib.vqae_classifier_optim_create(h3, ctypes.byref(cfg), ctypes.byref(o)) == UNSUPPORTED and not o.value
        assert lib.vqae_classifier_optim_create_ce(h1, ctypes.byref(cfg), ctypes.byref(o)) == UNSUPPORTED and not o.value
        assert lib.vqae_classifier_optim_create_ce(None, ctypes.byref(cfg), ctypes.byref(o)) == INVALID
        assert lib.vqae_classifier_optim_create_ce(h3, None, ctypes.byref(o)) == INVALID
        assert lib.vqae_classifier_optim_create_ce(h3, ctypes.byref(cfg), None) == INVALID
        bad = L.ClassifierOptimConfig(L.OPTIM_KINDS["adamw"], -1.0, 0.9, 0.999, 1e-8, 0.01, -1.0, 0)
        assert lib.vqae_classifier_optim_create_ce(h3, ctypes.byref(bad), ctypes.byref(o)) == INVALID
    finally:
        lib.vqae_classifier_destroy(h1)
        lib.vqae_classifier_destroy(h3)


def test_python_layer_refusals(cfx, cmodels, amd):
    from vqae_amd.classifier import CNNClassifier, classify_slide
    from vqae_amd.classifier_train import ce_loss_and_grads, loss_and_grads
    from vqae_amd.optim import ClassifierTrainer
    m = cmodels["E1C8O3"]
    one = CNNClassifier(256, 1, 8, 1)
    codes, labels, kw = case_inputs(cfx, "E1C8O3", "2x7x5", "cam_mean")
    with pytest.raises(ValueError):
        ce_loss_and_grads(one, codes, labels)                                    # n_out == 1 is the BCE route's
    with pytest.raises(ValueError):
        classify_slide(one, codes[0], labels[0], loss="ce", forward_fn=one)
    with pytest.raises(ValueError):
        ClassifierTrainer(one, loss="ce")
    with pytest.raises(ValueError):
        loss_and_grads(m, codes, labels)                                         # ... and the BCE route still refuses n_out == 3
    with pytest.raises(ValueError):
        ClassifierTrainer(m)
    with pytest.raises(ValueError):
        classify_slide(m, codes[0], labels[0], forward_fn=m)
    with pytest.raises(ValueError):
        classify_slide(m, codes[0], labels[0], loss="nll", forward_fn=m)
    bad = labels.clone()
    bad[0, 0, 0] = 3
    with pytest.raises(ValueError):
        ce_loss_and_grads(m, codes, bad, **kw)                                   # a label >= NO
    with pytest.raises(ValueError):
        classify_slide(m, codes[0], bad[0], loss="ce", forward_fn=m)
    with pytest.raises(ValueError):
        ce_loss_and_grads(m, codes, torch.zeros_like(labels), **kw)              # 'mean' over a zero weight sum (w[0] = 0)
    r = ce_loss_and_grads(m, codes, torch.zeros_like(labels), **dict(kw, reduction="sum"))
    assert r["weight_sum"] == 0.0 and r["loss"] > 0                              # ... whose smoothing term is still there
    assert any(bool(p.grad.any()) for p in params(m))
    for k, v in (("class_weight", [1.0, 1.0]), ("class_weight", [1.0, -1.0, 1.0]), ("class_weight", [1.0, float("nan"), 1.0]),
                 ("label_smoothing", -0.1), ("label_smoothing", 1.5), ("reduction", "none")):
        with pytest.raises(ValueError):
            ce_loss_and_grads(m, codes, labels, **dict(kw, **{k: v}))
    with pytest.raises(ValueError):
        ce_loss_and_grads(m, codes, labels[:, :5], **kw)
    with pytest.raises(TypeError):
        ce_loss_and_grads(m, codes, labels.float(), **kw)
    with pytest.raises(IndexError):
        ce_loss_and_grads(m, torch.full((2, 7, 5), 256, dtype=torch.int32), labels, **kw)
    tr = ClassifierTrainer(m, loss="ce", class_weight=CAM, label_smoothing=0.001, device="cpu")
    with pytest.raises(ValueError):
        tr.step(codes, labels, target=torch.zeros(2, 7, 5))
    with pytest.raises(ValueError):
        tr.step(codes, bad, check=True)
    # an injected gradient function replaces the restatement
    seen = []

    def grad_fn(clf, c, k, class_weight, label_smoothing, reduction):
        seen.append((tuple(c.shape), k.dtype, class_weight, label_smoothing, reduction))
        return [torch.full_like(p, 2.0) for p in params(clf)], (np.array([[1, 2, 0], [0, 3, 1], [1, 0, 4]]), 5.0, 6.0, 9.0, 0), 1.5

    r = ce_loss_and_grads(m, codes, labels, grad_fn=grad_fn, **kw)
    assert seen == [((2, 7, 5), torch.uint8, CAM, 0.001, "mean")]
    assert r["loss"] == 1.5 and r["weight_sum"] == 5.0 and r["confusion"].tolist() == [[3, 0, 0], [0, 3, 1], [1, 0, 4]]
    assert abs(r["loss_sum"] - (0.999 * 6.0 + 0.001 / 3 * 9.0)) <= 1e-15
    assert all(bool((p.grad == 2).all()) for p in params(m))


def test_background_hack_and_scores():
    from vqae_amd.classifier import apply_background_hack, ce_summary
    raw = np.array([[5, 2, 3], [1, 7, 2], [0, 4, 6]])
    hacked = apply_background_hack(raw)
    assert hacked.tolist() == [[10, 0, 0], [1, 7, 2], [0, 4, 6]] and raw[0, 1] == 2           # a copy
    s = ce_summary(raw, 12.5, 20.0, 66.0, 3, 0.1)
    assert s["confusion"].tolist() == hacked.tolist() and s["n_bad"] == 3 and s["weight_sum"] == 12.5
    assert s["precision"] == [10 / 11, 7 / 11, 6 / 8] and s["recall"] == [1.0, 7 / 10, 6 / 10]
    assert abs(s["loss_sum"] - (0.9 * 20.0 + 0.1 / 3 * 66.0)) <= 1e-14 and abs(s["loss"] - s["loss_sum"] / 12.5) <= 1e-15
    s = ce_summary(raw, 0.0, 0.0, 0.0, 0, 0.0, hack=False)
    assert s["confusion"].tolist() == raw.tolist() and s["precision"][0] == 5 / 6 and s["recall"][0] == 5 / 10
    assert np.isnan(s["loss"])
    s = ce_summary(np.array([[0, 0], [0, 0]]), 0.0, 0.0, 0.0, 0, 0.0)
    assert all(np.isnan(v) for v in s["precision"] + s["recall"])


# ---- the HDF5 drivers over the restatement ------------------------------------------------------------------------------------
def _archive(tmp_path, no):
    from vqae_amd import hdf5
    rs = np.random.RandomState(31)
    images = {"normal_001": rs.randint(0, 256, (20, 33)).astype(np.uint8), "normal_002": rs.randint(0, 256, (24, 30)).astype(np.uint8),
              "tumor_001": rs.randint(0, 256, (22, 31)).astype(np.uint8), "tumor_002": rs.randint(0, 256, (21, 35)).astype(np.uint8)}
    masks = {k + "_mask": (v % no).astype(np.uint8) for k, v in images.items()}
    return images, masks, hdf5.write_hdf5(tmp_path / "enc.hdf5", {"images": images, "masks": masks})


def test_classify_hdf5_cpu(cfx, cmodels, cmodels64, tmp_path):
    from vqae_amd import hdf5
    from vqae_amd.classifier import classify_hdf5, classify_slide
    clf = cmodels["E1C8O3"]
    images, masks, path = _archive(tmp_path, 3)
    out_path = tmp_path / "pred.hdf5"
    res = classify_hdf5(clf, path, out_path, forward_fn=clf, loss="ce", class_weight=CAM, label_smoothing=0.001)
    assert list(res["slides"]) == sorted(images)
    pred = hdf5.read_hdf5(out_path)["predictions"]
    total = np.zeros((3, 3), np.int64)
    for stem, codes in images.items():
        x = clf(torch.from_numpy(codes.astype(np.int64)))[0].double()
        cls = x.argmax(0).numpy()
        assert pred[stem].dtype == np.uint8 and np.array_equal(pred[stem], cls), stem
        lab = masks[stem + "_mask"]
        conf = np.zeros((3, 3), np.int64)
        np.add.at(conf, (lab.ravel(), cls.ravel()), 1)
        conf[0] = [conf[0].sum(), 0, 0]
        s = res["slides"][stem]
        assert s["confusion"].tolist() == conf.tolist()
        want = torch.nn.functional.cross_entropy(x[None], torch.from_numpy(lab.astype(np.int64))[None],
                                                 weight=torch.tensor(CAM, dtype=torch.float64), label_smoothing=0.001)
        assert abs(s["loss"] - float(want)) <= 1e-12 * float(want)
        total += conf
    assert res["pooled"]["confusion"].tolist() == total.tolist()
    assert abs(res["pooled"]["loss_sum"] - sum(s["loss_sum"] for s in res["slides"].values())) <= 1e-9
    raw = classify_slide(clf, images["tumor_001"], masks["tumor_001_mask"], forward_fn=clf, loss="ce", background_hack=False,
                         prob=True, logits=True)
    assert raw["confusion"][0, 1:].sum() > 0 and raw["prob"].shape == (3, 22, 31) and raw["prob"].dtype == np.uint8
    assert raw["logits"].shape == (3, 22, 31) and np.array_equal(raw["class"], raw["logits"].argmax(0))
    srt = np.sort(raw["prob"].astype(int), 0)
    clear = srt[-1] > srt[-2]                                                    # (two classes may round to the same level)
    assert clear.mean() > 0.9 and np.array_equal(raw["prob"].argmax(0)[clear], raw["class"][clear])
    assert np.abs(raw["prob"].astype(int).sum(0) - 255).max() <= 2
    only = classify_slide(clf, images["tumor_001"], forward_fn=clf, loss="ce")
    assert set(only) == {"class"} and np.array_equal(only["class"], raw["class"])
    # the default loss keeps today's behaviour
    with pytest.raises(ValueError):
        classify_hdf5(clf, path, forward_fn=clf)


def test_train_hdf5_cpu(cfx, tmp_path):
    from vqae_amd.classifier_train import ce_loss_and_grads, torch_ce_loss_grad, train_hdf5
    from vqae_amd.optim import SAM, ClassifierTrainer
    images, masks, path = _archive(tmp_path, 3)
    kw = dict(epochs=2, batch_size=2, seed=4, train_frac=0.5, reduction="mean", aligned_crops=True, class_weight=CAM,
              label_smoothing=0.001)
    clf = build(cfx, "E1C8O3")
    hist = train_hdf5(clf, path, torch.optim.Adam(clf.parameters(), lr=0.02), grad_fn=torch_ce_loss_grad, forward_fn=clf, **kw)
    assert len(hist) == 2 and [s["stems"] for s in hist[0]["steps"]] == [["normal_001", "tumor_001"]]
    st = hist[0]["steps"][0]
    assert st["shape"] == (2, 20, 31) and st["confusion"].shape == (3, 3) and int(st["confusion"].sum()) == 2 * 20 * 31
    assert hist[1]["steps"][0]["loss"] < st["loss"]
    assert int(hist[0]["val"]["confusion"].sum()) == 24 * 30 + 21 * 35 and np.isfinite(hist[0]["val"]["loss"])
    assert hist[0]["train"]["confusion"].tolist() == st["confusion"].tolist()
    # the first step is ce_loss_and_grads on the same crop
    again = build(cfx, "E1C8O3")
    r = ce_loss_and_grads(again, torch.from_numpy(images["normal_001"][None, :20, :31].copy()),
                          torch.from_numpy(masks["normal_001_mask"][None, :20, :31].copy()), class_weight=CAM, label_smoothing=0.001)
    assert np.isfinite(r["loss"])
    # a trainer on CPU tensors gives the same first-epoch losses as the hand loop with the same optimiser
    a, b = build(cfx, "E1C8O3"), build(cfx, "E1C8O3")
    tr = ClassifierTrainer(a, "adamw", lr=0.02, loss="ce", class_weight=CAM, label_smoothing=0.001, device="cpu")
    h_tr = train_hdf5(a, path, tr, forward_fn=a, **dict(kw, class_weight=None, label_smoothing=0.0))
    h_pt = train_hdf5(b, path, torch.optim.AdamW(b.parameters(), lr=0.02), grad_fn=torch_ce_loss_grad, forward_fn=b, **kw)
    for x, y in zip(h_tr, h_pt):
        assert abs(x["steps"][0]["loss"] - y["steps"][0]["loss"]) <= 1e-6 * abs(y["steps"][0]["loss"])
        assert x["steps"][0]["confusion"].tolist() == y["steps"][0]["confusion"].tolist()
    for p, q in zip(params(a), params(b)):
        assert float((p - q).abs().max()) <= 1e-6
    # SAM: two passes per batch
    c = build(cfx, "E1C8O3")
    calls = []

    def counting(*args):
        calls.append(1)
        return torch_ce_loss_grad(*args)

    sam = SAM(list(c.parameters()), torch.optim.AdamW, rho=0.05, lr=0.01)
    train_hdf5(c, path, sam, grad_fn=counting, forward_fn=c, **dict(kw, epochs=1))
    assert len(calls) == 2
    # pos_weight is required for n_out == 1 only
    from vqae_amd.classifier import CNNClassifier
    one = CNNClassifier()
    with pytest.raises(ValueError):
        train_hdf5(one, path, torch.optim.Adam(one.parameters()), epochs=1, batch_size=2, seed=1)
    with pytest.raises(ValueError):
        train_hdf5(a, path, ClassifierTrainer(build(cfx, "E1C8O3"), loss="ce", device="cpu"), **kw)      # another classifier's trainer
