"""CPU: the slide classifier's module mirror, its torch restatement, the C ABI's argument validation and the HDF5 driver.

tests/golden/classifier.npz holds what the reference's own validation_nn.model.CNNClassifier computed (fp32 and, after
.double(), fp64) for three variants on four small grids, each a batch of two slides so that every convolution of the
reference runs on ATen's oneDNN route (the single-image route is not reproducible between machines to the 1e-6 asked
below); see tests/golden/make_classifier_golden.py.  No kernel is launched here; test_classifier_gpu.py imports the
helpers below."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

VARIANTS = {"E1C8O1": (1, 8, 1), "E4C8O3": (4, 8, 3), "E1C16O1": (1, 16, 1)}
GRIDS = ("1x1", "2x3", "7x5", "2x37x70")
POS_WEIGHTS = (1.0, 40.4858)


@pytest.fixture(scope="module")
def fx():
    return load_golden("classifier")


def variant_state(fx, variant):
    """the reference's state_dict of a variant, names as the reference spells them"""
    pre = variant + "/layers."
    return {k[len(variant) + 1:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(pre)}


def build(fx, variant, num_embeddings=256):
    from vqae_amd.classifier import CNNClassifier
    E, C, NO = VARIANTS[variant]
    m = CNNClassifier(num_embeddings, E, C, NO)
    sd = variant_state(fx, variant)
    sd["layers.0.weight"] = sd["layers.0.weight"][:num_embeddings]
    m.load_state_dict(sd, strict=True)
    return m


@pytest.fixture(scope="module")
def models(fx):
    return {v: build(fx, v) for v in VARIANTS}


def err_ref(fx, variant):
    """max |ref32 - f64| of the reference itself over all grids of a variant"""
    return max(float(np.abs(fx[f"{variant}/ref32_{g}"].astype(np.float64) - fx[f"{variant}/f64_{g}"]).max()) for g in GRIDS)


def confusion(logit, mask):
    """numpy counts over mask != 0 with target mask - 1 and prediction logit > 0 -> (tp, fp, fn, tn)"""
    v = mask != 0
    t = (mask[v] - 1).astype(bool)
    p = logit[v] > 0
    return int((p & t).sum()), int((p & ~t).sum()), int((~p & t).sum()), int((~p & ~t).sum())


def two_slide_groups(seed=3):
    """the archive of the end-to-end tests: a uint8 slide with a mask and a uint16 slide without one, keys out of order"""
    rs = np.random.RandomState(seed)
    return {"images": {"tumor_002": rs.randint(0, 256, (33, 35)).astype(np.uint16),
                       "normal_001": rs.randint(0, 256, (40, 70)).astype(np.uint8)},
            "masks": {"normal_001_mask": rs.randint(0, 3, (40, 70)).astype(np.uint8)}}


# ---- the module mirror ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_restatement_matches_reference(fx, models, variant):
    m = models[variant]
    for g in GRIDS:
        codes = torch.from_numpy(fx[f"codes_{g}"])[:, None]
        out = m(codes)
        ref = torch.from_numpy(fx[f"{variant}/ref32_{g}"])
        assert out.dtype == torch.float32 and out.shape == ref.shape
        assert float((out - ref).abs().max()) <= 1e-6, (variant, g)
    # the other input forms
    c = torch.from_numpy(fx["codes_7x5"])
    assert torch.equal(m(c), m(c[:, None]))
    alone = m(c[0])                                                      # [H,W]: one slide, outside its batch
    assert alone.shape == m(c)[:1].shape and float((alone - m(c)[:1]).abs().max()) <= 1e-6
    assert torch.equal(m(c.to(torch.int32)), m(c)) and torch.equal(m(c.to(torch.int64)), m(c))
    if hasattr(torch, "uint16"):
        assert torch.equal(m(c.to(torch.uint16)), m(c))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_state_dict_names_and_shapes(fx, models, variant):
    want = {k: tuple(v.shape) for k, v in variant_state(fx, variant).items()}
    got = {k: tuple(v.shape) for k, v in models[variant].state_dict().items()}
    assert got == want
    assert [n for n, _ in models[variant].layers.named_children()] == [
        "embedding", "flatten_after_embedding", "in_conv", "act1", "hidden_conv1", "act2", "out_conv"]
    for k, v in variant_state(fx, variant).items():
        assert torch.equal(models[variant].state_dict()[k], v), k


def test_checkpoint_round_trip(fx, models, tmp_path):
    from vqae_amd.classifier import CNNClassifier
    from vqae_amd.model import load_lightning_state_dict
    sd = variant_state(fx, "E1C8O1")
    path = tmp_path / "epoch=1-step=10.ckpt"
    torch.save({"state_dict": sd, "epoch": 1, "global_step": 10}, path)
    m = CNNClassifier()
    m.load_state_dict(load_lightning_state_dict(str(path)), strict=True)
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v), k
    # cnn_classifier.yaml's own layer names load too
    named = {"layers." + n: p.detach().clone() for n, p in models["E1C8O1"].layers.named_parameters()}
    assert "layers.in_conv.weight" in named
    m2 = CNNClassifier()
    m2.load_state_dict(named, strict=True)
    c = torch.from_numpy(fx["codes_7x5"])
    assert torch.equal(m2(c), models["E1C8O1"](c)) and torch.equal(m(c), m2(c))
    with pytest.raises(RuntimeError):
        CNNClassifier().load_state_dict({k: v for k, v in sd.items() if k != "layers.6.bias"}, strict=True)


def test_inference_only_and_structure():
    from torch import nn
    from vqae_amd.classifier import CNNClassifier
    m = CNNClassifier()
    assert not m.training and not m.layers.in_conv.training
    assert m.eval() is m
    with pytest.raises(NotImplementedError):
        m.train()
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 1, 4, 4, requires_grad=True))
    with pytest.raises(TypeError):
        with torch.no_grad():
            m(torch.zeros(1, 1, 4, 4))
    with pytest.raises(IndexError):
        m(torch.full((1, 1, 4, 4), 256, dtype=torch.int32))
    with pytest.raises(IndexError):
        m(torch.full((4, 4), -1, dtype=torch.int64))

    def stack(**kw):
        mods = dict(embedding=nn.Embedding(256, 1), flatten=m.layers.flatten_after_embedding,
                    in_conv=nn.Conv2d(1, 8, 3, padding=1), act1=nn.ELU(), hidden_conv1=nn.Conv2d(8, 8, 3, padding=1),
                    act2=nn.ELU(), out_conv=nn.Conv2d(8, 1, 3, padding=1))
        mods.update(kw)
        return nn.Sequential(*mods.values())

    CNNClassifier(layers=stack(), optim=None, loss_f=None)                  # the reference's constructor arguments
    for bad in (dict(in_conv=nn.Conv2d(1, 8, 5, padding=2)), dict(act1=nn.ReLU()), dict(act2=nn.ELU(alpha=0.5)),
                dict(out_conv=nn.Conv2d(8, 1, 3, padding=1, bias=False)),
                dict(hidden_conv1=nn.Conv2d(8, 8, 3, padding=1, padding_mode="circular")),
                dict(extra=nn.Conv2d(1, 1, 3, padding=1))):
        with pytest.raises(NotImplementedError):
            CNNClassifier(layers=stack(**bad))


# ---- the C ABI, before any HIP call -----------------------------------------------------------------
def _tensors(L, E=1, C=8, NO=1, K=256, drop=None, resize=None):
    shapes = {"layers.embedding.weight": K * E, "layers.in_conv.weight": C * E * 9, "layers.in_conv.bias": C,
              "layers.hidden_conv1.weight": C * C * 9, "layers.hidden_conv1.bias": C,
              "layers.out_conv.weight": NO * C * 9, "layers.out_conv.bias": NO}
    keep, items = [], []
    for name, n in shapes.items():
        if name == drop:
            continue
        a = np.ones(n + (1 if name == resize else 0), np.float32)
        keep.append(a)
        items.append(L.Tensor(name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size))
    return keep, (L.Tensor * len(items))(*items), len(items)


def test_abi_argument_validation_without_gpu(amd):
    L = amd._lib
    lib = L.lib()
    h = ctypes.c_void_p()
    for args in ((256, 9, 8, 1), (256, 0, 8, 1), (256, 1, 12, 1), (256, 1, 8, 5), (256, 1, 8, 0), (70000, 1, 8, 1), (0, 1, 8, 1)):
        keep, arr, n = _tensors(L)
        assert lib.vqae_classifier_create(*args, arr, n, ctypes.byref(h)) == -2, args         # VQAE_ERR_UNSUPPORTED
        assert not h.value
    keep, arr, n = _tensors(L, drop="layers.hidden_conv1.bias")
    assert lib.vqae_classifier_create(256, 1, 8, 1, arr, n, ctypes.byref(h)) == -5             # VQAE_ERR_NOT_FOUND
    assert b"hidden_conv1.bias" in lib.vqae_last_error()
    with pytest.raises(KeyError):
        L.check(-5)
    keep, arr, n = _tensors(L, resize="layers.in_conv.weight")
    assert lib.vqae_classifier_create(256, 1, 8, 1, arr, n, ctypes.byref(h)) == -1             # VQAE_ERR_INVALID
    assert lib.vqae_classifier_create(256, 1, 8, 1, arr, n, None) == -1

    one = ctypes.c_void_p(16)                     # never dereferenced: validation fails (or batch == 0 returns) first
    keep, arr, n = _tensors(L)
    assert lib.vqae_classifier_create(256, 1, 8, 1, arr, n, ctypes.byref(h)) == 0 and h.value   # no HIP call in create
    keep3, arr3, n3 = _tensors(L, E=4, NO=3)
    h3 = ctypes.c_void_p()
    assert lib.vqae_classifier_create(256, 4, 8, 3, arr3, n3, ctypes.byref(h3)) == 0
    try:
        fwd = lib.vqae_classifier_forward
        U8 = L.IDX_U8
        assert fwd(None, one, U8, 1, 4, 4, one, None, None, 1.0, None, None, None) == -1          # null classifier
        assert fwd(h, None, U8, 1, 4, 4, one, None, None, 1.0, None, None, None) == -1            # null codes
        assert fwd(h, one, U8, 1, 4, 4, None, None, None, 1.0, None, None, None) == -1            # no output at all
        assert fwd(h, one, U8, 1, 4, 4, None, None, one, 1.0, None, one, None) == -1              # a mask is not an output
        assert fwd(h, one, U8, 1, 4, 4, one, None, None, 1.0, one, one, None) == -1               # stats without a mask
        assert fwd(h, one, U8, 1, 4, 4, one, None, one, 1.0, one, None, None) == -1               # stats without workspace
        assert fwd(h3, one, U8, 1, 4, 4, one, one, None, 1.0, None, None, None) == -1             # heat with n_out = 3
        assert fwd(h3, one, U8, 1, 4, 4, one, None, one, 1.0, one, one, None) == -1               # stats with n_out = 3
        assert fwd(h, one, U8, 1, 0, 4, one, None, None, 1.0, None, None, None) == -1             # h < 1
        assert fwd(h, one, U8, 1, 4, 0, one, None, None, 1.0, None, None, None) == -1             # w < 1
        assert fwd(h, one, U8, -1, 4, 4, one, None, None, 1.0, None, None, None) == -1
        assert fwd(h, one, 7, 1, 4, 4, one, None, None, 1.0, None, None, None) == -1              # bad index dtype
        assert fwd(h, one, U8, 1, 4, 4, None, None, one, -1.0, one, one, None) == -1              # negative pos_weight
        with pytest.raises(AssertionError):
            L.check(fwd(h, one, U8, 1, 4, 4, None, None, None, 1.0, None, None, None))
        assert fwd(h, one, U8, 70000, 4, 4, one, None, None, 1.0, None, None, None) == -2
        assert fwd(h, one, U8, 0, 4, 4, one, None, None, 1.0, None, None, None) == 0              # empty batch: VQAE_OK
        assert fwd(h, one, U8, 0, 4, 4, None, one, one, 1.0, one, one, None) == 0
        ws = lib.vqae_classifier_workspace_bytes
        assert ws(h, 0, 4, 4) == 0 and ws(h, 1, 0, 4) == 0 and ws(None, 1, 4, 4) == 0
        assert ws(h, 1, 1, 1) >= 6 * 8 and ws(h, 1, 1, 1) % 256 == 0
        assert ws(h, 3, 6144, 12288) >= 3 * (6144 // 14) * (12288 // 62) * 6 * 8
    finally:
        lib.vqae_classifier_destroy(h)
        lib.vqae_classifier_destroy(h3)
        lib.vqae_classifier_destroy(None)


def test_ops_refuse_cpu_tensors(amd, models):
    nat = models["E1C8O1"].native()                # building the handle needs no GPU
    with pytest.raises(amd._lib.VqaeHipError):
        nat.forward(torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(amd._lib.VqaeHipError):
        amd.ops.classifier_forward(nat._h, torch.zeros(1, 4, 4, dtype=torch.uint8))


# ---- the HDF5 driver over an injected forward ---------------------------------------------------------
def test_classify_hdf5_cpu(amd, models, tmp_path):
    from vqae_amd import hdf5
    from vqae_amd.classifier import classify_hdf5, classify_slide
    clf = models["E1C8O1"]
    groups = two_slide_groups()
    path = hdf5.write_hdf5(tmp_path / "enc.hdf5", groups)
    out_path = tmp_path / "pred.hdf5"
    pw = POS_WEIGHTS[1]
    res = classify_hdf5(clf, path, out_path, forward_fn=clf, pos_weight=pw)
    assert list(res["slides"]) == ["normal_001", "tumor_002"]                   # sorted key order
    assert res["slides"]["tumor_002"] == {}                                     # no mask: a map, no scores
    pred = hdf5.read_hdf5(out_path)["predictions"]
    assert sorted(pred) == ["normal_001", "tumor_002"]

    for stem, codes in groups["images"].items():
        x = clf(torch.from_numpy(codes.astype(np.int64)))[0, 0].double().numpy()
        heat = np.rint(255.0 / (1.0 + np.exp(-x)))
        assert pred[stem].dtype == np.uint8 and pred[stem].shape == codes.shape
        assert np.array_equal(pred[stem], heat.astype(np.uint8)), stem
    mask = groups["masks"]["normal_001_mask"]
    x = clf(torch.from_numpy(groups["images"]["normal_001"]))[0, 0].double().numpy()
    tp, fp, fn, tn = confusion(x, mask)
    s = res["slides"]["normal_001"]
    assert (s["tp"], s["fp"], s["fn"], s["tn"], s["n_valid"]) == (tp, fp, fn, tn, int((mask != 0).sum()))
    assert tp and fp and fn and tn
    assert s["precision"] == tp / (tp + fp) and s["recall"] == tp / (tp + fn)
    v = mask != 0
    t = (mask[v] - 1).astype(np.float64)
    sp = lambda z: np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))             # noqa: E731
    loss = float((pw * t * sp(-x[v]) + (1 - t) * sp(x[v])).sum())
    assert abs(s["loss"] - loss / v.sum()) <= 1e-12 * loss / v.sum()
    assert res["pooled"] == {k: s[k] for k in res["pooled"]}                    # one scored slide: pooled = that slide

    only = classify_hdf5(clf, path, names=["tumor_002"], forward_fn=clf)
    assert list(only["slides"]) == ["tumor_002"] and only["out_path"] is None
    assert only["pooled"]["n_valid"] == 0 and np.isnan(only["pooled"]["precision"]) and np.isnan(only["pooled"]["recall"])
    with pytest.raises(KeyError):
        classify_hdf5(clf, path, names=["absent"], forward_fn=clf)

    # an all-background mask: no valid code
    z = classify_slide(clf, groups["images"]["normal_001"], np.zeros((40, 70), np.uint8), forward_fn=clf, logits=True)
    assert z["n_valid"] == 0 and z["tp"] == z["fp"] == z["fn"] == z["tn"] == 0
    assert np.isnan(z["precision"]) and np.isnan(z["recall"]) and np.isnan(z["loss"])
    assert z["logits"].shape == (1, 40, 70) and z["logits"].dtype == np.float32

    # a stored uint16 code outside the table
    bad = groups["images"]["tumor_002"].copy()
    bad[5, 7] = 256
    bad_path = hdf5.write_hdf5(tmp_path / "bad.hdf5", {"images": {"s": bad}})
    with pytest.raises(IndexError):
        classify_hdf5(clf, bad_path, forward_fn=clf)
    with pytest.raises(ValueError):
        classify_slide(clf, groups["images"]["normal_001"], np.zeros((4, 4), np.uint8), forward_fn=clf)
    with pytest.raises(ValueError):
        classify_slide(clf, groups["images"]["normal_001"], np.full((40, 70), 3, np.uint8), forward_fn=clf)
    with pytest.raises(ValueError):
        classify_slide(models["E4C8O3"], groups["images"]["normal_001"], forward_fn=models["E4C8O3"])
