"""CPU: the host side of vqae_amd.code_stats -- the numpy restatement of the histogram kernel, the figures the reference's
loss YAMLs derive from its committed counts (tests/golden/code_marginals.npz holds those arrays verbatim), the archive
driver with the host path as hist_fn, and the C ABI's argument validation (which runs before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from code_stats_archive import small_archive
from conftest import load_golden


@pytest.fixture(scope="module")
def marginals():
    return load_golden("code_marginals")


# ---- host restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32, np.int64])
@pytest.mark.parametrize("K", [3, 256])
def test_host_histogram_equals_bincount(amd, dtype, K):
    from vqae_amd import code_stats as S
    rng = np.random.RandomState(K)
    codes = rng.randint(0, K, (3, 7, 13)).astype(dtype)
    mask = rng.randint(0, 3, (3, 7, 13)).astype(np.uint8)
    hist, bad = S.host_code_histogram(torch.from_numpy(codes), None, num_embeddings=K)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (3, 1, K) and not bad.any()
    for b in range(3):
        assert np.array_equal(hist[b, 0].numpy(), np.bincount(codes[b].ravel().astype(np.int64), minlength=K))
    hist, bad = S.host_code_histogram(torch.from_numpy(codes), torch.from_numpy(mask), num_embeddings=K)
    assert tuple(hist.shape) == (3, 3, K) and not bad.any()
    for b in range(3):
        want = np.bincount(mask[b].ravel().astype(np.int64) * K + codes[b].ravel().astype(np.int64), minlength=3 * K)
        assert np.array_equal(hist[b].numpy().ravel(), want)
    pooled, _ = S.host_code_histogram(torch.from_numpy(codes), torch.from_numpy(mask), num_embeddings=K, pooled=True)
    assert np.array_equal(pooled[0].numpy(), hist.numpy().sum(0))

    res = S.code_histogram(codes[0], mask[0], num_embeddings=K)
    assert res["joint"].dtype == np.int64 and res["joint"].shape == (3, K)
    assert np.array_equal(res["joint"].sum(0), res["codes"]) and np.array_equal(res["joint"].sum(1), res["labels"])
    assert np.array_equal(res["codes"], np.bincount(codes[0].ravel().astype(np.int64), minlength=K))
    assert np.array_equal(res["labels"], np.bincount(mask[0].ravel(), minlength=3))
    assert res["n"] == 7 * 13 and res["dead"] == int((res["codes"] == 0).sum())
    assert res["perplexity"] == S.perplexity(res["codes"])
    res1 = S.code_histogram(torch.from_numpy(codes[0]), num_embeddings=K)
    assert res1["joint"].shape == (1, K) and np.array_equal(res1["codes"], res["codes"]) and res1["labels"].tolist() == [91]


def test_host_histogram_bad_counts_and_errors(amd):
    from vqae_amd import code_stats as S
    K = 16
    codes = np.arange(40, dtype=np.int32).reshape(1, 40) % K
    mask = (np.arange(40) % 3).astype(np.uint8).reshape(1, 40)
    codes[0, [0, 5]] = (K, -1)                   # bad codes, whatever their label
    mask[0, [5, 7, 9]] = (255, 3, 200)           # position 5 already counts as a bad code
    hist, bad = S.host_code_histogram(torch.from_numpy(codes), torch.from_numpy(mask), num_embeddings=K)
    assert bad.tolist() == [[2, 2]]
    assert int(hist.sum()) + 2 + 2 == 40
    keep = np.ones(40, bool)
    keep[[0, 5, 7, 9]] = False
    assert np.array_equal(hist[0].numpy().ravel(), np.bincount(mask[0, keep].astype(np.int64) * K + codes[0, keep], minlength=3 * K))
    # accumulate
    out, bd = torch.full((1, 3, K), 2 ** 40, dtype=torch.int64), torch.ones((1, 2), dtype=torch.int64)
    o2, b2 = S.host_code_histogram(torch.from_numpy(codes), torch.from_numpy(mask), num_embeddings=K, out=out, bad=bd)
    assert o2 is out and b2 is bd and torch.equal(out, hist + 2 ** 40) and bd.tolist() == [[3, 3]]

    with pytest.raises(IndexError):
        S.code_histogram(codes[0], mask[0], num_embeddings=K)
    codes[0, [0, 5]] = 1
    with pytest.raises(ValueError, match="0 .background., 1 .tissue. and 2 .cancer."):
        S.code_histogram(codes[0], mask[0], num_embeddings=K)
    with pytest.raises(ValueError):
        S.code_histogram(codes[0], mask[0, :39], num_embeddings=K)
    with pytest.raises(TypeError):
        S.code_histogram(codes[0].astype(np.float32), num_embeddings=K)


# ---- the reference's figures, from its committed counts -------------------------------------------------------------------
def test_class_weights_reproduce_reference_yamls(amd, marginals):
    from vqae_amd.code_stats import class_weights
    val = marginals["histogram_val"]
    assert val.dtype == np.int64 and val.shape == (3,)
    w = class_weights(val, decimals=4)
    assert w["ce_weight"].tolist() == [0, 0.0247, 0.9753]                 # cross_entropy_camelyon16_embeddings.yaml `weight`
    assert round(w["pos_weight"], 4) == 40.4858                           # bce_with_logits_loss_camelyon16_embeddings.yaml
    assert w["pos_weight"] == 1 / round(float(val[2]) / float(val[1] + val[2]), 4)
    rec = w["reciprocal"]
    assert rec[2] == 125.0 and round(rec[0], 3) == 1.476 and round(rec[1], 4) == 3.1786   # the commented alternative
    for name, want in (("histogram_val", 40.4117), ("histogram_train", 51.6132), ("histogram_test", 27.3592)):
        c = marginals[name]
        u = class_weights(c)
        assert u["pos_weight"] == pytest.approx(want, rel=1e-4)
        assert u["pos_weight"] == (float(c[1]) + float(c[2])) / float(c[2])
        assert np.allclose(u["marginal"], c / c.sum(), rtol=1e-15) and abs(u["marginal"].sum() - 1) < 1e-12
        assert np.allclose(u["foreground"], c[1:] / c[1:].sum(), rtol=1e-15)
        assert u["ce_weight"][0] == 0 and u["ce_weight"][1] == u["foreground"][1] and u["ce_weight"][2] == u["foreground"][0]
        assert np.allclose(u["reciprocal"], c.sum() / c, rtol=1e-15)
    z = class_weights([10, 5, 0])
    assert z["pos_weight"] == float("inf") and z["reciprocal"][2] == float("inf")
    with pytest.raises(ValueError):
        class_weights([1, 2])


def test_perplexity_of_reference_marginal(amd, marginals):
    from vqae_amd.code_stats import perplexity
    c = marginals["embedding_idx_histogram_256_validation"]
    assert c.dtype == np.int64 and c.shape == (256,)
    p = c.astype(np.float64) / np.float64(c.sum())
    want = float(np.exp(-np.sum(p * np.log(p + 1e-10))))                  # vq.py:135-136 in fp64
    got = perplexity(c)
    assert got == pytest.approx(want, rel=1e-9)
    assert got == pytest.approx(23.0816, abs=5e-5)
    assert int((c == 0).sum()) == 0
    assert perplexity(np.full(64, 7)) == pytest.approx(64.0, rel=1e-7)
    assert perplexity([5, 0, 0]) == pytest.approx(1.0, rel=1e-7)
    for k in (128, 256, 512, 1024):                                       # the reference's marginals: one code holds 45-48 %
        for s in ("train", "validation", "test"):
            a = marginals[f"embedding_idx_histogram_{k}_{s}"]
            assert a.shape == (k,) and a.sum() == marginals["histogram_val" if s == "validation" else f"histogram_{s}"].sum()


# ---- the archive driver on the host path ----------------------------------------------------------------------------------
def test_histogram_hdf5_host_path(amd, tmp_path):
    from vqae_amd import code_stats as S
    images, masks = small_archive(tmp_path / "enc.hdf5")
    path = str(tmp_path / "enc.hdf5")
    K = 512                                                              # max code 299 -> next power of two

    def want(stem):
        return np.bincount(masks[stem + "_mask"].ravel().astype(np.int64) * K + images[stem].ravel().astype(np.int64),
                           minlength=3 * K).reshape(3, K)

    allr = S.histogram_hdf5(path, hist_fn=S.host_code_histogram)
    assert allr["num_embeddings"] == K and allr["stems"] == sorted(images) and allr["split"] is None and allr["files"] == []
    seen = []
    for split, short in (("train", "train"), ("validation", "val"), ("test", "test")):
        out_dir = tmp_path / "out"
        r = S.histogram_hdf5(path, split=split, train_frac=0.5, num_embeddings=K, out_dir=str(out_dir),
                             hist_fn=S.host_code_histogram)
        assert r["stems"] == amd.embeddings_split(images.keys(), split, 0.5) and list(r["slides"]) == r["stems"]
        seen += r["stems"]
        for s in r["stems"]:
            assert np.array_equal(r["slides"][s]["joint"], want(s))
            assert r["slides"][s]["n"] == images[s].size
            assert np.array_equal(r["slides"][s]["joint"], allr["slides"][s]["joint"])
        pj = sum(r["slides"][s]["joint"] for s in r["stems"])
        assert np.array_equal(r["pooled"]["joint"], pj) and r["pooled"]["n"] == sum(images[s].size for s in r["stems"])
        assert np.array_equal(r["pooled"]["codes"], pj.sum(0)) and np.array_equal(r["pooled"]["labels"], pj.sum(1))
        names = [f"embedding_idx_histogram_{K}_{split}.npy", f"histogram_{short}.npy", f"joint_histogram_{K}_{split}.npy"]
        assert [os.path.basename(f) for f in r["files"]] == names
        for f, shape, arr in zip(r["files"], ((K,), (3,), (3, K)), (pj.sum(0), pj.sum(1), pj)):
            a = np.load(f)
            assert a.dtype == np.int64 and a.shape == shape and np.array_equal(a, arr)
            h = a / a.sum()                                              # the plotting scripts' normalisation
            assert np.isfinite(h).all() and abs(h.sum() - 1) < 1e-12
        assert S.pos_weight_hdf5(path, split, 0.5, hist_fn=S.host_code_histogram) == \
            S.class_weights(r["pooled"]["labels"])["pos_weight"]
    assert sorted(seen) == sorted(images)                               # train + validation + test partition the archive
    assert len(set(seen)) == len(seen)
    assert np.array_equal(allr["pooled"]["joint"], sum(want(s) for s in images))


def test_histogram_hdf5_missing_mask_and_bad_codes(amd, tmp_path):
    from vqae_amd import code_stats as S
    images, masks = small_archive(tmp_path / "enc.hdf5", with_all_masks=False)
    path = str(tmp_path / "enc.hdf5")
    with pytest.raises(KeyError, match="tumor_002_mask"):
        S.histogram_hdf5(path, hist_fn=S.host_code_histogram)
    with pytest.raises(KeyError):
        S.histogram_hdf5(path, names=["no_such_slide"], hist_fn=S.host_code_histogram)
    r = S.histogram_hdf5(path, names=["tumor_002", "tumor_001"], num_embeddings=512, hist_fn=S.host_code_histogram)
    assert r["stems"] == ["tumor_001", "tumor_002"]
    bare = r["slides"]["tumor_002"]
    assert bare["joint"] is None and bare["labels"] is None
    assert np.array_equal(bare["codes"], np.bincount(images["tumor_002"].ravel(), minlength=512))
    assert np.array_equal(r["pooled"]["codes"], bare["codes"] + r["slides"]["tumor_001"]["codes"])
    assert np.array_equal(r["pooled"]["joint"], r["slides"]["tumor_001"]["joint"])
    with pytest.raises(IndexError, match="images/"):                     # codes up to 299 in a 256-row table
        S.histogram_hdf5(path, names=["tumor_001", "normal_002"], num_embeddings=256, hist_fn=S.host_code_histogram)


# ---- C ABI: validation before any HIP call --------------------------------------------------------------------------------
def test_code_histogram_abi_errors_without_gpu(amd):
    L = amd._lib
    lib = L.lib()
    one = ctypes.c_void_p(16)                    # never dereferenced: validation fails first

    def call(codes=one, idx=L.IDX_U8, mask=one, batch=1, n=64, K=256, nl=3, hist=one, bad=one, ws=one):
        return lib.vqae_code_histogram(codes, idx, mask, batch, n, K, nl, 0, 0, hist, bad, ws, None)

    invalid = [dict(codes=None), dict(hist=None), dict(ws=None), dict(mask=None, nl=3), dict(idx=7), dict(idx=-1), dict(n=0),
               dict(n=-5), dict(batch=-1)]
    for kw in invalid:
        assert call(**kw) == -1, kw
        assert lib.vqae_last_error().startswith(b"code_histogram:"), kw
        with pytest.raises(AssertionError):
            L.check(call(**kw))
    unsupported = [dict(K=0), dict(K=65537), dict(nl=0, mask=None), dict(nl=9), dict(batch=65536)]
    for kw in unsupported:
        assert call(**kw) == -2, kw
        assert lib.vqae_last_error().startswith(b"code_histogram:"), kw
        with pytest.raises(NotImplementedError):
            L.check(call(**kw))
    wb = lib.vqae_code_histogram_workspace_bytes
    assert wb(0, 4096, 256, 3) == 0
    sizes = [wb(b, 4096, 256, 3) for b in (1, 2, 16, 17, 1000, 65535)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] >= 65535 * 16


def test_ops_code_histogram_refuses_cpu_tensors(amd):
    with pytest.raises(amd._lib.VqaeHipError):
        amd.ops.code_histogram(torch.zeros((1, 8), dtype=torch.uint8), num_embeddings=4)
