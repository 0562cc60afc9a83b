"""CPU: training the slide classifier -- the torch restatement of loss and gradients against the reference's recorded ones,
the `.grad` / optimiser contract, the dataset helpers against the reference's recorded outputs, the HDF5 training driver
over an injected gradient function, and the C ABI's argument validation.

tests/golden/classifier_train.npz holds what the reference's own CNNClassifier.step + Camelyon16BCELoss + autograd gave, in
fp32 and (after .double()) in fp64, see tests/golden/make_classifier_train_golden.py.  The accuracy measure is the relative
error of the worst tensor, e(G) = max over the seven tensors of max|G - G64| / max|G64|; e_ref of a variant is e of the
reference's own fp32 gradients, maximised over the fixture grids and pos_weights, and an fp32 evaluation that sums the same
products in another order may be 4 x e_ref away (the margin DESIGN.md section 11 grants the forward for the same reason).
No kernel is launched here; test_classifier_train_gpu.py imports the helpers below."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

VARIANTS = {"E1C8O1": (1, 8, 1), "E1C16O1": (1, 16, 1), "E4C8O1": (4, 8, 1)}
GRIDS = ("2x7x5", "2x37x70", "4x64x96")
POS_WEIGHTS = (1.0, 40.4858)
EXTRA_GRID = "2x37x70"
CASES = [(g, c) for g in GRIDS for c in ("pw0", "pw1")] + [(EXTRA_GRID, "mean"), (EXTRA_GRID, "soft")]
CASE_ARGS = {"pw0": dict(pos_weight=POS_WEIGHTS[0]), "pw1": dict(pos_weight=POS_WEIGHTS[1]),
             "mean": dict(pos_weight=POS_WEIGHTS[1], reduction="mean"), "soft": dict(pos_weight=POS_WEIGHTS[1])}


@pytest.fixture(scope="module")
def tfx():
    return load_golden("classifier_train")


def build(tfx, variant, dtype=torch.float32):
    from vqae_amd.classifier import CNNClassifier
    E, C, NO = VARIANTS[variant]
    m = CNNClassifier(256, E, C, NO)
    pre = variant + "/layers."
    m.load_state_dict({k[len(variant) + 1:]: torch.from_numpy(tfx[k]) for k in tfx.files if k.startswith(pre)}, strict=True)
    return m.to(dtype)


def as_double(clf):
    """a copy of the classifier in fp64: the yardstick of the tests without a recorded gradient"""
    from vqae_amd.classifier import CNNClassifier
    ls = clf.layers
    m = CNNClassifier(ls.embedding.num_embeddings, ls.embedding.embedding_dim, ls.in_conv.out_channels, ls.out_conv.out_channels)
    m.load_state_dict(clf.state_dict(), strict=True)
    return m.double()


@pytest.fixture(scope="module")
def tmodels(tfx):
    return {v: build(tfx, v) for v in VARIANTS}


@pytest.fixture(scope="module")
def tmodels64(tfx):
    return {v: build(tfx, v, torch.float64) for v in VARIANTS}


def params(clf):
    from vqae_amd.classifier_train import _params
    return _params(clf)


def grads_of(clf):
    return [p.grad.detach().double().cpu().numpy().copy() for p in params(clf)]


def e_of(G, G64):
    """relative error of the worst tensor"""
    return max(float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max()) for a, b in zip(G, G64))


def recorded(tfx, variant, grid, case, tag):
    return [tfx[f"{variant}/{grid}/{case}/g{tag}_{i}"] for i in range(7)]


def e_ref(tfx, variant):
    """e of the reference's own fp32 gradients, maximised over the fixture grids and pos_weights"""
    return max(e_of(recorded(tfx, variant, g, c, "32"), recorded(tfx, variant, g, c, "64")) for g in GRIDS for c in ("pw0", "pw1"))


def case_inputs(tfx, grid, case):
    codes, mask = torch.from_numpy(tfx[f"codes_{grid}"]), torch.from_numpy(tfx[f"mask_{grid}"])
    kw = dict(CASE_ARGS[case])
    if case == "soft":
        kw["target"] = torch.from_numpy(tfx["soft_target"])
    return codes, mask, kw


def loss_bound(pos_weight, e_logit, n_valid, loss64):
    return max(1.0, pos_weight) * e_logit * n_valid + 1e-6 * abs(loss64)


# ---- the restatement against the reference's recorded loss and gradients ----------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_restatement_fp64_reproduces_the_reference(tfx, tmodels64, variant):
    from vqae_amd.classifier_train import loss_and_grads
    m = tmodels64[variant]
    for grid, case in CASES:
        codes, mask, kw = case_inputs(tfx, grid, case)
        res = loss_and_grads(m, codes, mask, **kw)
        loss64 = float(tfx[f"{variant}/{grid}/{case}/loss64"])
        assert abs(res["loss"] - loss64) <= 1e-12 * abs(loss64), (variant, grid, case)
        assert all(p.grad.dtype == torch.float64 and p.grad.shape == p.shape for p in params(m))
        assert e_of(grads_of(m), recorded(tfx, variant, grid, case, "64")) <= 1e-12, (variant, grid, case)
        assert res["n_valid"] == int((mask != 0).sum())
        assert res["tp"] + res["fp"] + res["fn"] + res["tn"] == res["n_valid"]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_restatement_fp32_within_the_bound(tfx, tmodels, tmodels64, variant):
    from vqae_amd.classifier_train import loss_and_grads
    m = tmodels[variant]
    tol = 4 * e_ref(tfx, variant)
    for grid, case in CASES:
        codes, mask, kw = case_inputs(tfx, grid, case)
        res = loss_and_grads(m, codes, mask, **kw)
        assert all(p.grad.dtype == torch.float32 for p in params(m))
        e = e_of(grads_of(m), recorded(tfx, variant, grid, case, "64"))
        print(f"{variant} {grid} {case}: e = {e:.3e}, 4 e_ref = {tol:.3e}")
        assert e <= tol, (variant, grid, case, e, tol)
        e_logit = float((m(codes).double() - tmodels64[variant](codes)).abs().max())
        n = res["n_valid"]
        loss64 = float(tfx[f"{variant}/{grid}/{case}/loss64"])
        scale = n if case == "mean" else 1
        assert abs(res["loss"] - loss64) * scale <= loss_bound(kw["pos_weight"], e_logit, n, loss64 * scale), (variant, grid, case)


# ---- .grad, accumulation, the optimiser ---------------------------------------------------------------------------------
def test_grad_contract_and_optimizer_step(tfx):
    from vqae_amd.classifier_train import loss_and_grads
    m = build(tfx, "E1C8O1", torch.float64)
    codes, mask, kw = case_inputs(tfx, "2x7x5", "pw1")
    assert all(p.grad is None for p in m.parameters())
    r1 = loss_and_grads(m, codes, mask, **kw)
    g1 = grads_of(m)
    loss_and_grads(m, codes[:, None], mask, accumulate=True, **kw)           # [B,1,H,W] codes
    assert e_of(grads_of(m), [2 * g for g in g1]) <= 1e-13                   # (the host's fp64 sums are not ordered run to run)
    loss_and_grads(m, codes, mask, **kw)                                      # without accumulate: overwritten
    assert e_of(grads_of(m), g1) <= 1e-13
    one = loss_and_grads(m, codes[0], mask[0], **kw)                          # [H,W]: one slide
    two = loss_and_grads(m, codes[1], mask[1], accumulate=True, **kw)
    assert abs(one["loss"] + two["loss"] - r1["loss"]) <= 1e-12 * r1["loss"]
    assert e_of(grads_of(m), g1) <= 1e-12                                     # the batch's gradient is the sum of its slides'
    assert one["loss"] == one["loss_sum"] and one["n_valid"] + two["n_valid"] == r1["n_valid"]

    # an optimiser step: the next call sees the new weights, and descends
    loss_and_grads(m, codes, mask, **kw)
    before = [p.detach().clone() for p in params(m)]
    opt = torch.optim.SGD(m.parameters(), lr=1e-4)
    opt.step()
    for p, b, g in zip(params(m), before, g1):
        assert torch.allclose(p.detach(), b - 1e-4 * torch.from_numpy(g), rtol=1e-14, atol=0)
    r2 = loss_and_grads(m, codes, mask, **kw)
    assert r2["loss"] < r1["loss"]
    assert e_of(grads_of(m), g1) > 1e-6                                       # other weights, other gradients
    with pytest.raises(NotImplementedError):                                  # the mirror itself stays inference-only
        m.train()

    # mean = sum / n_valid of the whole batch, loss and gradients
    s = loss_and_grads(m, codes, mask, **kw)
    gs = grads_of(m)
    mn = loss_and_grads(m, codes, mask, reduction="mean", **kw)
    assert abs(mn["loss"] - s["loss"] / s["n_valid"]) <= 1e-14 * mn["loss"] and mn["loss_sum"] == pytest.approx(s["loss_sum"], rel=1e-14)
    assert e_of(grads_of(m), [g / s["n_valid"] for g in gs]) <= 1e-13


def test_errors_and_empty_masks(tfx, tmodels):
    from vqae_amd.classifier import CNNClassifier
    from vqae_amd.classifier_train import loss_and_grads
    m = tmodels["E1C8O1"]
    codes, mask, kw = case_inputs(tfx, "2x7x5", "pw0")
    with pytest.raises(IndexError):
        loss_and_grads(m, torch.full((1, 7, 5), 256, dtype=torch.int32), mask[:1])
    with pytest.raises(IndexError):
        loss_and_grads(m, torch.full((1, 7, 5), -1, dtype=torch.int64), mask[:1])
    with pytest.raises(ValueError):
        loss_and_grads(CNNClassifier(256, 4, 8, 3), codes, mask)              # n_out != 1
    with pytest.raises(ValueError):
        loss_and_grads(m, codes, mask[:, :5])
    with pytest.raises(ValueError):
        loss_and_grads(m, codes, torch.full_like(mask, 3))
    with pytest.raises(ValueError):
        loss_and_grads(m, codes, mask, reduction="none")
    with pytest.raises(ValueError):
        loss_and_grads(m, codes, mask, pos_weight=-1.0)
    with pytest.raises(ValueError):
        loss_and_grads(m, codes, mask, target=torch.full(mask.shape, 1.5))
    with pytest.raises(TypeError):
        loss_and_grads(m, codes.float(), mask)
    zero = torch.zeros_like(mask)
    with pytest.raises(ValueError):
        loss_and_grads(m, codes, zero, reduction="mean")
    r = loss_and_grads(m, codes, zero)
    assert r["loss"] == 0.0 and r["loss_sum"] == 0.0 and r["n_valid"] == 0
    assert all(p.grad is not None and not p.grad.any() for p in params(m))
    # an injected gradient function replaces the restatement
    seen = []

    def grad_fn(clf, c, k, target, pos_weight, reduction):
        seen.append((tuple(c.shape), k.dtype, target, pos_weight, reduction))
        return [torch.full_like(p, 2.0) for p in params(clf)], (1, 2, 3, 4, 5.0)

    r = loss_and_grads(m, codes, mask, pos_weight=3.0, grad_fn=grad_fn)
    assert seen == [((2, 7, 5), torch.uint8, None, 3.0, "sum")]
    assert (r["tp"], r["fp"], r["fn"], r["tn"], r["n_valid"], r["loss"]) == (1, 2, 3, 4, 10, 5.0)
    assert all(bool((p.grad == 2).all()) for p in params(m))


# ---- the helpers of the data path ------------------------------------------------------------------------------------------
def test_smooth_targets():
    from vqae_amd.classifier_train import smooth_targets
    mask = torch.from_numpy(np.random.RandomState(0).randint(0, 3, (3, 17, 23)).astype(np.uint8))
    for ls in (0.3, 2.5):
        got = smooth_targets(mask, ls, torch.Generator().manual_seed(5))
        noise = torch.randn(mask.shape, generator=torch.Generator().manual_seed(5))
        want = (1 - ((1 + (mask.float() - 1) + noise * ls) % 2)).abs()
        assert got.dtype == torch.float32 and torch.equal(got, want)
        assert float(got.min()) >= 0 and float(got.max()) <= 1
    hard = smooth_targets(mask, 0.0)
    valid = mask != 0
    assert torch.equal(hard[valid], (mask[valid] - 1).float())                # no smoothing: the hard targets


def test_split_and_collate_equal_the_reference(tfx):
    from vqae_amd.classifier_train import collate_random_crop, embeddings_split
    keys = [str(k) for k in tfx["split/keys"]]
    shuffled = [keys[i] for i in np.random.RandomState(2).permutation(len(keys))]
    for frac in (0.9, 0.5, 0.1):
        for mode in ("train", "validation"):
            assert embeddings_split(shuffled, mode, frac) == [str(k) for k in tfx[f"split/{frac}/{mode}"]], (frac, mode)
    assert embeddings_split(shuffled, "test", 0.9) == [str(k) for k in tfx["split/test"]]
    with pytest.raises(ValueError):
        embeddings_split(keys, "val", 0.9)

    batch = [(tfx[f"collate/img_{i}"], tfx[f"collate/msk_{i}"]) for i in range(3)]
    img, msk = collate_random_crop(batch, np.random.RandomState(int(tfx["collate/seed"])))
    assert tuple(img.shape) == (3, 7, 8)
    assert np.array_equal(img.numpy(), tfx["collate/out_img"]) and np.array_equal(msk.numpy(), tfx["collate/out_msk"])
    assert img.dtype == torch.int32 and msk.dtype == torch.int64
    # aligned=True: the mask is cut where its grid is cut
    pairs = [(a, a.astype(np.int64) + 1000) for a, _ in batch]
    i2, m2 = collate_random_crop(pairs, np.random.RandomState(3), aligned=True)
    assert torch.equal(i2.long() + 1000, m2)
    i3, m3 = collate_random_crop(pairs, np.random.RandomState(3))
    assert torch.equal(i3, i2) and not torch.equal(i3.long() + 1000, m3)      # the reference's own, independent draws


def four_slide_groups(seed=4):
    rs = np.random.RandomState(seed)
    shapes = {"normal_001": (20, 31), "tumor_001": (26, 24), "normal_002": (18, 22), "tumor_002": (25, 25), "test_001": (9, 9)}
    return {"images": {k: rs.randint(0, 256, s).astype(np.uint8) for k, s in shapes.items()},
            "masks": {k + "_mask": rs.randint(0, 3, s).astype(np.uint8) for k, s in shapes.items()}}


def test_train_hdf5_cpu(amd, tfx, tmp_path):
    from vqae_amd import hdf5
    from vqae_amd.classifier import classify_hdf5
    from vqae_amd.classifier_train import collate_random_crop, loss_and_grads, torch_loss_grad, train_hdf5
    groups = four_slide_groups()
    path = hdf5.write_hdf5(tmp_path / "enc.hdf5", groups)
    pw, seed, lr = POS_WEIGHTS[1], 11, 1e-5
    clf = build(tfx, "E1C8O1")
    seen = []

    def grad_fn(c, codes, mask, target, pos_weight, reduction):
        seen.append((codes.clone(), mask.clone()))
        return torch_loss_grad(c, codes, mask, target, pos_weight, reduction)

    hist = train_hdf5(clf, path, torch.optim.SGD(clf.parameters(), lr=lr), epochs=2, batch_size=2, train_frac=0.5,
                      pos_weight=pw, seed=seed, grad_fn=grad_fn, forward_fn=clf)
    # the walk: normal_001 + tumor_001 train (one batch per epoch), normal_002 + tumor_002 validate; crops from RandomState(seed)
    assert [e["epoch"] for e in hist] == [0, 1] and len(seen) == 2
    twin = build(tfx, "E1C8O1")
    opt = torch.optim.SGD(twin.parameters(), lr=lr)
    rng = np.random.RandomState(seed)
    pair = [(groups["images"][k], groups["masks"][k + "_mask"]) for k in ("normal_001", "tumor_001")]
    for ep in range(2):
        codes, mask = collate_random_crop(pair, rng)
        assert tuple(codes.shape) == (2, 20, 24)
        assert torch.equal(seen[ep][0], codes) and torch.equal(seen[ep][1], mask.to(torch.uint8))
        want = loss_and_grads(twin, codes, mask, pos_weight=pw)
        opt.step()
        step, = hist[ep]["steps"]
        assert step["stems"] == ["normal_001", "tumor_001"] and step["shape"] == (2, 20, 24)
        assert {k: step[k] for k in want} == want
        assert hist[ep]["train"]["loss"] == want["loss_sum"] / want["n_valid"]
        assert hist[ep]["train"]["tp"] == want["tp"] and hist[ep]["train"]["n_valid"] == want["n_valid"]
    for p, q in zip(clf.parameters(), twin.parameters()):
        assert torch.equal(p, q)
    val = classify_hdf5(clf, path, names=["normal_002", "tumor_002"], forward_fn=clf, pos_weight=pw)["pooled"]
    assert hist[1]["val"].keys() == val.keys()
    for k, v in val.items():
        assert hist[1]["val"][k] == v or (np.isnan(v) and np.isnan(hist[1]["val"][k])), k
    assert hist[1]["train"]["loss"] < hist[0]["train"]["loss"]
    with pytest.raises(KeyError):
        train_hdf5(clf, hdf5.write_hdf5(tmp_path / "nomask.hdf5", {"images": groups["images"]}), None, epochs=1, batch_size=2,
                   pos_weight=pw, seed=0, grad_fn=grad_fn, forward_fn=clf)


# ---- the C ABI, before any HIP call ------------------------------------------------------------------------------------------
def test_abi_argument_validation_without_gpu(amd):
    from test_classifier_cpu import _tensors
    L = amd._lib
    lib = L.lib()
    for name in ("vqae_classifier_update", "vqae_classifier_grad_floats", "vqae_classifier_train_workspace_bytes",
                 "vqae_classifier_loss_grad"):
        assert name in L.SYMBOLS and getattr(lib, name)
    one = ctypes.c_void_p(16)                     # never dereferenced: validation fails first
    h, h3 = ctypes.c_void_p(), ctypes.c_void_p()
    keep, arr, n = _tensors(L)
    assert lib.vqae_classifier_create(256, 1, 8, 1, arr, n, ctypes.byref(h)) == 0
    keep3, arr3, n3 = _tensors(L, E=4, NO=3)
    assert lib.vqae_classifier_create(256, 4, 8, 3, arr3, n3, ctypes.byref(h3)) == 0
    try:
        upd = lib.vqae_classifier_update
        assert upd(h, arr, n) == 0                                            # no HIP call: fine without a device
        assert upd(None, arr, n) == -1 and upd(h, None, n) == -1
        k2, a2, n2 = _tensors(L, drop="layers.out_conv.bias")
        assert upd(h, a2, n2) == -5 and b"out_conv.bias" in lib.vqae_last_error()
        k2, a2, n2 = _tensors(L, resize="layers.embedding.weight")
        assert upd(h, a2, n2) == -1
        assert upd(h, arr3, n3) == -1                                         # another variant's shapes
        assert lib.vqae_classifier_grad_floats(h) == 256 + 72 + 8 + 576 + 8 + 72 + 1
        assert lib.vqae_classifier_grad_floats(h3) == 1024 + 288 + 8 + 576 + 8 + 216 + 3
        assert lib.vqae_classifier_grad_floats(None) == 0
        ws = lib.vqae_classifier_train_workspace_bytes
        assert ws(h, 0, 4, 4) == 0 and ws(h, 1, 0, 4) == 0 and ws(None, 1, 4, 4) == 0 and ws(h3, 1, 4, 4) == 0
        assert ws(h, 2, 37, 70) >= lib.vqae_classifier_workspace_bytes(h, 2, 37, 70) + 2 * 37 * 70 * 4 + 256 * 8 + 737 * 8
        assert ws(h, 1, 6144, 12288) <= lib.vqae_classifier_workspace_bytes(h, 1, 6144, 12288) + 6144 * 12288 * 4 + (16 << 20)

        lg = lib.vqae_classifier_loss_grad
        U8 = L.IDX_U8

        def call(c=h, codes=one, dt=U8, B=1, H=4, W=4, mask=one, target=None, pw=1.0, red=0, grads=one, stats=one, loss=one, wsp=one):
            return lg(c, codes, dt, B, H, W, mask, target, pw, red, grads, stats, loss, wsp, None)

        for null in ("c", "codes", "mask", "grads", "stats", "loss", "wsp"):
            assert call(**{null: None}) == -1, null
        assert call(dt=7) == -1 and call(H=0) == -1 and call(W=0) == -1 and call(B=-1) == -1
        assert call(pw=-1.0) == -1 and call(pw=float("nan")) == -1 and call(pw=float("inf")) == -1
        assert call(red=2) == -1
        with pytest.raises(AssertionError):
            L.check(call(red=-1))
        assert call(c=h3) == -2 and b"n_out" in lib.vqae_last_error()          # VQAE_ERR_UNSUPPORTED
        assert call(B=70000) == -2
        with pytest.raises(NotImplementedError):
            L.check(call(c=h3, target=one))
    finally:
        lib.vqae_classifier_destroy(h)
        lib.vqae_classifier_destroy(h3)


def test_ops_refuse_cpu_tensors(amd, tmodels):
    nat = tmodels["E1C8O1"].native()
    z = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(amd._lib.VqaeHipError):
        amd.ops.classifier_loss_grad(nat._h, z, z)
    with pytest.raises(amd._lib.VqaeHipError):
        nat.loss_grad(z, z)
