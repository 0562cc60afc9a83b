"""CPU: the reconstruction-metrics contract (metrics.py, include/vqae_hip.h section 4) restated in fp64 and checked
against independent facts, the new ABI entry points' argument validation, and the host logic of validate() sharded
under gloo (world 2 and 3) with the forward and the metrics injected.  tests/test_metrics_gpu.py holds the kernel to
the restatement below."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

WIN, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03


# ---- fp64 restatement of the contract -----------------------------------------------------------------------------------
def gauss_taps(dtype=torch.float64):
    """torchmetrics 0.8.2 `_gaussian(11, 1.5)` in `dtype`: exp(-(k / 1.5)^2 / 2), k = -5 .. 5, normalised to sum 1."""
    k = torch.arange((1 - WIN) / 2, (1 + WIN) / 2, 1.0, dtype=dtype)
    g = torch.exp(-((k / SIGMA) ** 2) / 2)
    return g / g.sum()


def valid_filter(x, g):
    """Separable 11x11 Gaussian moments at the valid centres: x [..., H, W] -> [..., H-10, W-10]."""
    x = x.unfold(-1, WIN, 1) @ g                  # horizontal
    return x.unfold(-2, WIN, 1) @ g               # vertical


def ref_metrics(p, t, delta=1.0):
    """Per-image metrics of p, t [B, C, H, W] (any float dtype; evaluated in fp64) -> dict of fp64 numpy [B]."""
    p, t = torch.as_tensor(p).double(), torch.as_tensor(t).double()
    if p.shape[-1] < WIN or p.shape[-2] < WIN:
        raise ValueError("image smaller than the SSIM window")
    B = p.shape[0]
    d = (p - t).reshape(B, -1)
    ad = d.abs()
    mse = (d * d).mean(1)
    huber = torch.where(ad < delta, 0.5 * d * d, delta * (ad - 0.5 * delta)).mean(1)
    pf, tf = p.reshape(B, -1), t.reshape(B, -1)
    rt = tf.max(1).values - tf.min(1).values
    rp = pf.max(1).values - pf.min(1).values
    psnr = 10 * torch.log10(rt * rt / mse)
    r = torch.maximum(rp, rt).reshape(B, 1, 1, 1)
    c1, c2 = (K1 * r) ** 2, (K2 * r) ** 2
    g = gauss_taps()
    mp_, mt = valid_filter(p, g), valid_filter(t, g)
    epp, ett, ept = valid_filter(p * p, g), valid_filter(t * t, g), valid_filter(p * t, g)
    spp, stt, spt = epp - mp_ * mp_, ett - mt * mt, ept - mp_ * mt
    s = ((2 * mp_ * mt + c1) * (2 * spt + c2)) / ((mp_ * mp_ + mt * mt + c1) * (spp + stt + c2))
    ssim = s.reshape(B, -1).mean(1)
    out = {"mse": mse, "huber": huber, "psnr": psnr, "ssim": ssim, "pred_min": pf.min(1).values,
           "pred_max": pf.max(1).values, "target_min": tf.min(1).values, "target_max": tf.max(1).values}
    return {k: v.numpy() for k, v in out.items()}


def torchmetrics_ssim(p, t, dtype=torch.float32):
    """SSIM per image in torchmetrics 0.8.2's op order (`_ssim_compute`): reflect pad 5, one grouped 2-D conv of the
    stacked (p, t, pp, tt, pt) with the outer-product window, un-centred moments, crop 5, mean."""
    p, t = torch.as_tensor(p).to(dtype), torch.as_tensor(t).to(dtype)
    B, C = p.shape[:2]
    g = gauss_taps(dtype)
    w2 = torch.matmul(g[:, None], g[None, :]).expand(C, 1, WIN, WIN)
    r = torch.maximum(p.reshape(B, -1).max(1).values - p.reshape(B, -1).min(1).values,
                      t.reshape(B, -1).max(1).values - t.reshape(B, -1).min(1).values).reshape(B, 1, 1, 1)
    c1, c2 = torch.pow(K1 * r, 2), torch.pow(K2 * r, 2)
    pad = (WIN - 1) // 2
    pp_, tp_ = F.pad(p, (pad,) * 4, mode="reflect"), F.pad(t, (pad,) * 4, mode="reflect")
    inp = torch.cat((pp_, tp_, pp_ * pp_, tp_ * tp_, pp_ * tp_))
    o = F.conv2d(inp, w2, groups=C).split(B)
    mu_p_sq, mu_t_sq, mu_pt = o[0].pow(2), o[1].pow(2), o[0] * o[1]
    sp, st, spt = o[2] - mu_p_sq, o[3] - mu_t_sq, o[4] - mu_pt
    upper, lower = 2 * spt + c2, sp + st + c2
    s = ((2 * mu_pt + c1) * upper) / ((mu_p_sq + mu_t_sq + c1) * lower)
    s = s[..., pad:-pad, pad:-pad]
    return s.reshape(B, -1).double().mean(1).numpy()


# ---- the restatement against independent facts ---------------------------------------------------------------------------
def _imgs(seed, shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape))


def test_identity_ssim_one_psnr_inf():
    x = _imgs(0, (3, 3, 20, 17))
    m = ref_metrics(x, x)
    np.testing.assert_allclose(m["ssim"], 1.0, rtol=0, atol=1e-14)
    assert np.all(np.isposinf(m["psnr"])) and np.all(m["mse"] == 0) and np.all(m["huber"] == 0)


def test_gaussian_taps_closed_form():
    g = gauss_taps().numpy()
    k = np.arange(-5, 6)
    want = np.exp(-k.astype(np.float64) ** 2 / (2 * 1.5 ** 2))
    np.testing.assert_allclose(g, want / want.sum(), rtol=1e-15, atol=0)
    assert abs(g.sum() - 1) < 1e-15 and np.allclose(g, g[::-1], rtol=0, atol=0)


def test_separable_equals_direct_2d_window():
    x = _imgs(1, (2, 3, 15, 19))
    g = gauss_taps()
    w2 = torch.outer(g, g)
    direct = torch.empty(2, 3, 5, 9, dtype=torch.float64)
    for i in range(5):
        for j in range(9):
            direct[:, :, i, j] = (x[:, :, i:i + WIN, j:j + WIN] * w2).sum((-1, -2))
    assert float((valid_filter(x, g) - direct).abs().max()) <= 1e-12


def test_valid_crop_equals_reflect_pad_conv_crop():
    p, t = _imgs(2, (2, 3, 24, 31)), _imgs(3, (2, 3, 24, 31))
    want = torchmetrics_ssim(p, t, dtype=torch.float64)
    got = ref_metrics(p, t)["ssim"]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_huber_matches_torch_huber_loss():
    p, t = _imgs(4, (2, 3, 12, 12)) * 2, _imgs(5, (2, 3, 12, 12))
    got = ref_metrics(p, t)["huber"]
    want = [float(torch.nn.HuberLoss(delta=1.0)(p[i], t[i])) for i in range(2)]
    np.testing.assert_allclose(got, want, rtol=1e-14)


# ---- ABI --------------------------------------------------------------------------------------------------------------
def test_recon_metrics_abi_exported_and_validated(amd):
    L = amd._lib
    lib = L.lib()
    for name in ("vqae_recon_metrics_workspace_bytes", "vqae_recon_metrics_f32"):
        assert name in L.SYMBOLS and getattr(lib, name).argtypes == L.SYMBOLS[name][1]
    assert lib.vqae_recon_metrics_workspace_bytes(4, 3, 512, 512) > 0
    assert lib.vqae_recon_metrics_workspace_bytes(4, 3, 10, 512) == 0
    one = __import__("ctypes").c_void_p(16)           # never dereferenced: validation fails first
    args = lambda h, w, pred=one, tgt=one, u8=None, out=one, ws=one, c=3, delta=1.0, layout=L.LAYOUT_NCHW: (
        pred, tgt, u8, None, None, 2, c, h, w, layout, delta, out, ws, None)
    with pytest.raises(ValueError):                    # torchmetrics: image smaller than the window
        L.check(lib.vqae_recon_metrics_f32(*args(10, 32)))
    with pytest.raises(ValueError):
        L.check(lib.vqae_recon_metrics_f32(*args(32, 10)))
    assert b"11" in lib.vqae_last_error()
    with pytest.raises(AssertionError):
        L.check(lib.vqae_recon_metrics_f32(*args(32, 32, pred=None)))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_recon_metrics_f32(*args(32, 32, out=None)))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_recon_metrics_f32(*args(32, 32, ws=None)))
    with pytest.raises(AssertionError):                # both targets
        L.check(lib.vqae_recon_metrics_f32(*args(32, 32, u8=one)))
    with pytest.raises(AssertionError):                # neither
        L.check(lib.vqae_recon_metrics_f32(*args(32, 32, tgt=None)))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_recon_metrics_f32(*args(32, 32, delta=0.0)))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_recon_metrics_f32(*args(32, 32, layout=7)))
    with pytest.raises(NotImplementedError):           # a uint8 target has the 3 channels of the normalisation
        L.check(lib.vqae_recon_metrics_f32(*args(32, 32, tgt=None, u8=one, c=4)))


def test_recon_metrics_refuses_cpu_tensors(amd):
    from vqae_amd.metrics import recon_metrics
    with pytest.raises(amd._lib.VqaeHipError):
        recon_metrics(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


# ---- validate() host logic under gloo -----------------------------------------------------------------------------------
class _Items(torch.utils.data.Dataset):
    """Seeded fp32 images [3, 12, 14]; records which indices were read."""

    def __init__(self, n):
        self.n, self.reads = n, []

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        self.reads.append(int(i))
        return _imgs(100 + i, (3, 12, 14)).float(), torch.zeros(1), i


def _cpu_forward(imgs):
    out = imgs * 0.75 + 0.1 * torch.sin(imgs * 3)
    return out, (imgs * imgs).mean()                  # the batch mean, as the native forward's commitment loss


def _cpu_metrics(out, imgs):
    m = ref_metrics(out, imgs)
    psnr = 10 * np.log10((m["pred_max"] - m["pred_min"]) ** 2 / m["mse"])      # range of the reconstruction
    return torch.from_numpy(np.stack([m["mse"], m["huber"], psnr, m["ssim"]], 1))


def _run_validate(n, bs):
    from vqae_amd.validate import validate
    ds = _Items(n)
    res = validate(None, ds, batch_size=bs, device="cpu", forward_fn=_cpu_forward, metrics_fn=_cpu_metrics)
    return res, ds.reads


def _validate_worker(rank, ws, port, cases, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        import vqae_amd  # noqa: F401
        q.put((rank, True, [_run_validate(n, bs) for n, bs in cases]))
    except Exception:
        import traceback
        q.put((rank, False, traceback.format_exc()))
    dist.destroy_process_group()


_CASES = [(11, 4), (7, 2), (5, 8), (2, 4)]             # ragged shares; shares of 1 and 0 on some ranks


def _assert_same(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        if k in ("encoding_loss", "val_encoding_loss_0"):
            continue                                    # batch-share means: composition depends on the world size
        if isinstance(v, np.ndarray):
            assert v.dtype == got[k].dtype and np.array_equal(got[k], v), k
        else:
            assert got[k] == v, (k, got[k], v)


def test_validate_single_process_matches_per_image_restatement(amd):
    res, reads = _run_validate(11, 4)
    assert res["n_images"] == 11 and sorted(reads) == list(range(11))
    ds = _Items(11)
    imgs = torch.stack([ds[i][0] for i in range(11)])
    out, _ = _cpu_forward(imgs)
    want = _cpu_metrics(out, imgs).numpy()
    for i, k in enumerate(("mse", "huber", "psnr", "ssim")):
        np.testing.assert_allclose(res[k], want[:, i], rtol=1e-13, atol=0)
    assert res["val_MeanSquaredError"] == float(res["mse"].mean())
    assert res["val_recon_loss"] == float(res["huber"].mean())
    assert res["val_PeakSignalNoiseRatio"] == float(res["psnr"].mean())
    assert res["val_StructuralSimilarityIndexMeasure"] == float(res["ssim"].mean())
    # val_encoding_loss_0: the batch losses weighted by batch size
    losses = [float((imgs[b:b + 4].double() ** 2).mean()) for b in range(0, 11, 4)]
    want_loss = sum(l * min(4, 11 - b) for l, b in zip(losses, range(0, 11, 4))) / 11
    assert abs(res["val_encoding_loss_0"] - want_loss) <= 1e-6 * abs(want_loss)


@pytest.mark.parametrize("ws", [2, 3])
def test_validate_sharded_gloo_equals_world1(amd, ws):
    """Every rank returns the world-1 dict (the per-image rows are gathered back into dataset order), and each rank's
    loader read only its share of every batch."""
    want = [_run_validate(n, bs) for n, bs in _CASES]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29400 + ws * 40 + os.getpid() % 40
    procs = [ctx.Process(target=_validate_worker, args=(r, ws, port, _CASES, q)) for r in range(ws)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(60)
    assert all(r[1] for r in res), [r[2] for r in res if not r[1]]
    from vqae_amd.dist import shard_range
    for ci, (n, bs) in enumerate(_CASES):
        w_res = want[ci][0]
        for rank, _, runs in res:
            got, reads = runs[ci]
            _assert_same(got, w_res)
            assert abs(got["val_encoding_loss_0"] - w_res["val_encoding_loss_0"]) <= 1e-6 * abs(w_res["val_encoding_loss_0"])
            mine = []
            for b0 in range(0, n, bs):
                lo, hi = shard_range(min(bs, n - b0), rank, ws)
                mine += list(range(b0 + lo, b0 + hi))
            assert sorted(reads) == mine, (rank, reads, mine)
        # all ranks hold identical encoding-loss rows too
        for _, _, runs in res[1:]:
            assert np.array_equal(runs[ci][0]["encoding_loss"], res[0][2][ci][0]["encoding_loss"])
