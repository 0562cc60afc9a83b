"""GPU: the reconstruction-metrics kernel (csrc/recon_metrics.hip) against the fp64 restatement of the contract
(tests/test_metrics_cpu.py), its bitwise invariance, the on-the-fly uint8 target, and the end-to-end figures of the
native forward against the reference's recorded outputs; validate() against a hand loop."""
import numpy as np
import pytest
import torch

from conftest import load_golden, record_parity
from test_metrics_cpu import ref_metrics, torchmetrics_ssim
from test_model_gpu import golden_params

pytestmark = pytest.mark.gpu

SCALARS = ("mse", "huber", "psnr", "ssim", "pred_min", "pred_max", "target_min", "target_max")


def _rng(seed):
    return np.random.default_rng(seed)


def _case(name):
    """(pred, target) fp32 NCHW on the host."""
    r = _rng(CASES.index(name))
    n = lambda *s: torch.from_numpy(r.standard_normal(s).astype(np.float32))
    if name == "random":
        t = n(3, 3, 40, 52)
        return t + 0.3 * n(3, 3, 40, 52), t
    if name == "const_pred":                      # sigma_p = 0
        return torch.full((2, 3, 24, 24), 0.25), n(2, 3, 24, 24)
    if name == "const_target":                    # sigma_t = 0, r_t = 0 -> psnr -inf
        return n(2, 3, 24, 24), torch.full((2, 3, 24, 24), -0.5)
    if name == "equal":                           # p = t: ssim 1, psnr inf
        t = n(2, 3, 30, 30)
        return t.clone(), t
    if name == "outlier":                         # one pixel dominates the range
        t = n(2, 3, 32, 32)
        p = t + 0.1 * n(2, 3, 32, 32)
        p[0, 1, 7, 9] = 900.0
        t[1, 2, 30, 3] = -700.0
        return p, t
    if name == "straddle_delta":                  # |d| on both sides of delta = 1
        t = n(2, 3, 28, 28)
        d = torch.from_numpy(r.uniform(0.5, 1.5, (2, 3, 28, 28)).astype(np.float32))
        sign = torch.from_numpy(np.where(r.random((2, 3, 28, 28)) < 0.5, -1, 1).astype(np.float32))
        return t + sign * d, t
    if name == "h11_w13":
        t = n(2, 3, 11, 13)
        return t + 0.2 * n(2, 3, 11, 13), t
    if name == "nonsquare":
        t = n(2, 3, 24, 150)
        return t + 0.2 * n(2, 3, 24, 150), t
    if name == "b1":
        t = n(1, 3, 64, 64)
        return 0.8 * t + 0.1 * n(1, 3, 64, 64), t
    if name == "b257":
        t = n(257, 3, 12, 16)
        return t + 0.2 * n(257, 3, 12, 16), t
    raise KeyError(name)


CASES = ["random", "const_pred", "const_target", "equal", "outlier", "straddle_delta", "h11_w13", "nonsquare", "b1",
         "b257"]


def _check(name, got, want, tm_ssim, layout):
    g = {k: got[k].cpu().numpy() for k in SCALARS}
    for k in ("pred_min", "pred_max", "target_min", "target_max"):
        assert np.array_equal(g[k], want[k]), k
    rel = lambda a, b: np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    mse_err = float(np.max(np.where(want["mse"] == 0, np.abs(g["mse"]), rel(g["mse"], want["mse"]))))
    hub_err = float(np.max(np.where(want["huber"] == 0, np.abs(g["huber"]), rel(g["huber"], want["huber"]))))
    finite = np.isfinite(want["psnr"])
    assert np.array_equal(g["psnr"][~finite], want["psnr"][~finite])
    psnr_err = float(np.max(np.abs(g["psnr"][finite] - want["psnr"][finite]), initial=0.0))
    ssim_err = np.abs(g["ssim"] - want["ssim"])
    tm_err = np.abs(tm_ssim - want["ssim"])
    record_parity("recon_metrics_vs_fp64", case=name, layout=layout, batch=int(len(g["mse"])), mse_rel=mse_err,
                  huber_rel=hub_err, psnr_abs_db=psnr_err, ssim_abs_max=float(ssim_err.max()),
                  ssim_torch_fp32_abs_max=float(tm_err.max()))
    assert mse_err <= 2e-6 and hub_err <= 2e-6, (mse_err, hub_err)
    assert psnr_err <= 1e-4, psnr_err
    assert np.all(ssim_err <= 1.25 * tm_err + 1e-6), (ssim_err.max(), tm_err.max())


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_fp64_restatement(amd, name):
    from vqae_amd.metrics import recon_metrics
    p, t = _case(name)
    want = ref_metrics(p, t)
    tm = torchmetrics_ssim(p, t)
    got = recon_metrics(p.cuda(), t.cuda(), "NCHW")
    _check(name, got, want, tm, "NCHW")
    nhwc = lambda x: x.permute(0, 2, 3, 1).contiguous().cuda()
    got2 = recon_metrics(nhwc(p), nhwc(t), "NHWC")
    _check(name, got2, want, tm, "NHWC")


def test_bitwise_invariance_across_runs_and_batches(amd):
    from vqae_amd.metrics import recon_metrics_raw
    r = _rng(7)
    t = torch.from_numpy(r.standard_normal((257, 3, 40, 36)).astype(np.float32)).cuda()
    p = t + 0.3 * torch.from_numpy(r.standard_normal((257, 3, 40, 36)).astype(np.float32)).cuda()
    a = recon_metrics_raw(p, t)
    b = recon_metrics_raw(p, t)
    assert torch.equal(a, b)
    k = 17
    batch_p, batch_t = p.clone(), t.clone()
    batch_p[200], batch_t[200] = p[k], t[k]
    alone = recon_metrics_raw(p[k:k + 1].clone(), t[k:k + 1].clone())
    inside = recon_metrics_raw(batch_p, batch_t)
    assert torch.equal(alone[0], inside[200]) and torch.equal(alone[0], a[k])


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
def test_u8_target_equals_fp32_target(amd, layout):
    from vqae_amd.extract_embeddings import SyntheticSlideDataset
    from vqae_amd.metrics import recon_metrics
    raw = SyntheticSlideDataset([(2, 3)], patch_size=(40, 48), seed=3, raw=True)
    f32 = SyntheticSlideDataset([(2, 3)], patch_size=(40, 48), seed=3, raw=False)
    u8 = torch.stack([raw[i][0] for i in range(6)]).cuda()
    tgt = torch.stack([f32[i][0] for i in range(6)]).cuda()                  # NCHW fp32
    pred = tgt + 0.2 * torch.randn(tgt.shape, generator=torch.Generator().manual_seed(5)).cuda()
    if layout == "NHWC":
        pred, tgt = pred.permute(0, 2, 3, 1).contiguous(), tgt.permute(0, 2, 3, 1).contiguous()
    a = recon_metrics(pred, u8, layout)
    b = recon_metrics(pred, tgt, layout)
    want = ref_metrics(*(x.permute(0, 3, 1, 2) if layout == "NHWC" else x for x in (pred.cpu(), tgt.cpu())))
    tm = torchmetrics_ssim(*(x.permute(0, 3, 1, 2) if layout == "NHWC" else x for x in (pred.cpu(), tgt.cpu())))
    _check("u8_target", a, want, tm, layout)
    bitwise = all(torch.equal(a[k], b[k]) for k in SCALARS)
    record_parity("recon_metrics_u8_vs_f32_target", layout=layout, bitwise=bitwise)
    for k in SCALARS:
        assert torch.allclose(a[k], b[k], rtol=2e-6, atol=0), k


@pytest.mark.parametrize("name", ["tiny", "tinyP", "tinyM"])
def test_native_forward_metrics_match_reference_output(amd, oracle, name):
    from vqae_amd.metrics import recon_metrics
    g = load_golden(f"model_{name}")
    _, p = golden_params(oracle, name, g)
    nat = amd.NativeVQAE(amd.SPECS[name], p)
    x = torch.from_numpy(g["x"])
    out, _, _ = nat.forward(x.cuda())
    got = recon_metrics(out, x.cuda())
    ref = ref_metrics(torch.from_numpy(g["tap:out"]), x)
    ssim_d = float(np.abs(got["ssim"].cpu().numpy() - ref["ssim"]).max())
    mse_mean = float(got["mse"].mean())
    rel = abs(mse_mean - float(g["recon_mse"])) / float(g["recon_mse"])
    record_parity("recon_metrics_native_forward", model=name, ssim_vs_ref_out=ssim_d, mse_mean=mse_mean,
                  recon_mse_ref=float(g["recon_mse"]), mse_rel=rel)
    assert ssim_d <= 1e-4 and rel <= 1e-4


def test_cfg_b_mean_mse_equals_fixture(amd, oracle):
    from vqae_amd.metrics import recon_metrics
    g = load_golden("model_B")
    _, p = golden_params(oracle, "B", g)
    x = oracle.make_patches(int(g["batch"]), 256, 0)
    nat = amd.NativeVQAE(amd.SPECS["B"], p)
    out, _, _ = nat.forward(x.cuda())
    got = recon_metrics(out, x.cuda())
    mse_mean = float(got["mse"].mean())
    rel = abs(mse_mean - float(g["recon_mse"])) / float(g["recon_mse"])
    record_parity("recon_metrics_cfg_B", mse_mean=mse_mean, recon_mse_ref=float(g["recon_mse"]), mse_rel=rel,
                  ssim=got["ssim"].cpu().tolist())
    assert rel <= 1e-4


@pytest.mark.parametrize("raw", [True, False])
def test_validate_equals_hand_loop(amd, oracle, raw):
    from vqae_amd.extract_embeddings import SyntheticSlideDataset
    from vqae_amd.metrics import psnr_from, recon_metrics
    from vqae_amd.validate import validate
    g = load_golden("model_tiny")
    _, p = golden_params(oracle, "tiny", g)
    nat = amd.NativeVQAE(amd.SPECS["tiny"], p)
    ds = SyntheticSlideDataset([(2, 2), (1, 3)], patch_size=32, seed=1, raw=raw)
    res = validate(nat, ds, batch_size=3, autocast_dtype=None)
    rows, losses = [], []
    for b0 in range(0, len(ds), 3):
        imgs = torch.stack([ds[i][0] for i in range(b0, min(b0 + 3, len(ds)))]).cuda()
        if raw:
            q, _, loss = nat.encode_u8(imgs, want_q=True)
            out = nat.decode(q)
        else:
            out, _, loss = nat.forward(imgs)
        r = recon_metrics(out, imgs)
        rows.append(torch.stack([r["mse"], r["huber"], psnr_from(r["mse"], r["pred_min"], r["pred_max"]), r["ssim"]], 1))
        losses += [float(loss)] * imgs.shape[0]
    want = torch.cat(rows).cpu().numpy()
    record_parity("validate_vs_hand_loop", raw=raw, n=res["n_images"], ssim=res["val_StructuralSimilarityIndexMeasure"],
                  psnr=res["val_PeakSignalNoiseRatio"], mse=res["val_MeanSquaredError"])
    assert res["n_images"] == len(ds)
    for i, k in enumerate(("mse", "huber", "psnr", "ssim")):
        assert np.array_equal(res[k], want[:, i]), k
    assert np.allclose(res["encoding_loss"], np.asarray(losses), rtol=0, atol=0)
    assert res["val_StructuralSimilarityIndexMeasure"] == float(want[:, 3].mean())


def test_metric_collection_dropin(amd):
    """metrics(batch, out) as model.py:92 calls it: torchmetrics' argument order (PSNR on the range of `out`), means over the
    batch; update / compute / reset accumulate over batches."""
    from vqae_amd.metrics import ReconMetrics
    r = _rng(11)
    x = torch.from_numpy(r.standard_normal((5, 3, 24, 28)).astype(np.float32))
    out = 0.7 * x + 0.2 * torch.from_numpy(r.standard_normal((5, 3, 24, 28)).astype(np.float32))
    m = ReconMetrics()
    first = m(x[:3].cuda(), out[:3].cuda())
    m.update(x[3:].cuda(), out[3:].cuda())
    want = ref_metrics(x, out)                      # preds = batch, target = reconstruction
    assert set(first) == set(ReconMetrics.KEYS)
    np.testing.assert_allclose(float(first["MeanSquaredError"]), want["mse"][:3].mean(), rtol=2e-6)
    np.testing.assert_allclose(float(first["PeakSignalNoiseRatio"]), want["psnr"][:3].mean(), rtol=0, atol=1e-4)
    tot = m.compute()
    np.testing.assert_allclose(float(tot["MeanSquaredError"]), want["mse"].mean(), rtol=2e-6)
    np.testing.assert_allclose(float(tot["PeakSignalNoiseRatio"]), want["psnr"].mean(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(float(tot["StructuralSimilarityIndexMeasure"]), want["ssim"].mean(), rtol=0, atol=1e-6)
    m.reset()
    assert m._n == 0
