"""On-device reconstruction metrics: MSE, Huber, PSNR and SSIM per image, one HIP call for all of them
(csrc/recon_metrics.hip, `vqae_recon_metrics_f32`).

The contract restates the metrics the reference's validation logs (VQAE.shared_step, vq_ae/model.py:82-93;
conf/model/loss_f/huber.yaml; conf/model/metrics/{mse,psnr,ssim}.yaml) with the semantics of torchmetrics 0.8.2, the
version the reference pins, and of torch.nn.HuberLoss.  For one image, prediction p and target t [C, H, W],
N = C*H*W, d = p - t:

    mse   = sum d^2 / N
    huber = sum h(d) / N,   h(d) = 0.5 d^2 if |d| < delta else delta (|d| - 0.5 delta),   delta = 1.0
    psnr  = 10 log10(r_t^2 / mse),   r_t = max t - min t       (PeakSignalNoiseRatio, data_range=None; mse = 0 -> +inf)
    ssim  = mean over C x (H-10) x (W-10) of
            s = ((2 mu_p mu_t + c1)(2 s_pt + c2)) / ((mu_p^2 + mu_t^2 + c1)(s_p^2 + s_t^2 + c2))
            with r = max(max p - min p, max t - min t), c1 = (0.01 r)^2, c2 = (0.03 r)^2, the moments mu_p, mu_t, E[pp], E[tt],
            E[pt] over the 11x11 window g (x) g, g_k ~ exp(-k^2 / (2 * 1.5^2)), k = -5..5, sum 1, and the un-centred
            s_p^2 = E[pp] - mu_p^2, s_t^2 = E[tt] - mu_t^2, s_pt = E[pt] - mu_p mu_t.  torchmetrics pads by reflection and crops
            the pad again, so only the valid window centres count; H < 11 or W < 11 raises ValueError.

A dataset value is the mean of the per-image values (scripts/extract_validation_metrics/eval.py:29 validates with batch
size 1, and Lightning's epoch value is the mean of the steps), so data ranges are per image, never per batch.  The metrics
are evaluated in fp32 with fp64 sums on the fp32 reconstruction; eval.py also runs the metric evaluation itself under
fp16 autocast, which is not reproduced.

Argument order: `recon_metrics(pred, target)` takes the reconstruction as `pred`.  The reference calls its collection as
`self.metrics(batch, out)` (model.py:92), i.e. torchmetrics' `preds` is the input and `target` the reconstruction, so its
PSNR takes the data range of the reconstruction.  `ReconMetrics` and validate.py keep that order; MSE and SSIM are
symmetric, PSNR is recomputed from the same MSE and the other range column.
"""
import ctypes
from typing import Dict

import torch

from . import _lib as L
from . import ops
from .extract_embeddings import MEAN, STD

NAMES = L.METRIC_NAMES            # columns of the kernel's per-image rows (VQAE_METRIC_*)


def _norm255(mean, std):
    """(mean * 255, 1 / (std * 255)) in fp32, as SyntheticSlideDataset(raw=False) and the u8 encoder compute them."""
    import numpy as np
    m = np.asarray(mean, np.float32) * np.float32(255)
    inv = np.float32(1) / (np.asarray(std, np.float32) * np.float32(255))
    return (ctypes.c_float * 3)(*m.tolist()), (ctypes.c_float * 3)(*inv.tolist())


def recon_metrics_raw(pred, target, layout="NCHW", huber_delta=1.0, mean=MEAN, std=STD) -> torch.Tensor:
    """The kernel's [B, 8] fp64 rows (columns NAMES) on the device.  pred: fp32 [B,C,H,W] (layout 'NCHW') or [B,H,W,C]
    ('NHWC'); target: fp32 in the same layout, or uint8 NHWC [B,H,W,3] normalised on the fly with (mean, std)."""
    ops._need_gpu(pred, target)
    if layout not in ("NCHW", "NHWC"):
        raise AssertionError(f"layout must be 'NCHW' or 'NHWC', got {layout!r}")
    assert pred.dtype == torch.float32 and pred.dim() == 4, (pred.dtype, tuple(pred.shape))
    pred = pred.contiguous()
    target = target.contiguous()
    if layout == "NCHW":
        B, C, H, W = pred.shape
    else:
        B, H, W, C = pred.shape
    u8 = target.dtype == torch.uint8
    if u8:
        assert tuple(target.shape) == (B, H, W, C), f"uint8 target must be NHWC {(B, H, W, C)}, got {tuple(target.shape)}"
    else:
        assert target.dtype == torch.float32 and target.shape == pred.shape, (target.dtype, tuple(target.shape))
    lib = L.lib()
    out = torch.empty((B, len(NAMES)), dtype=torch.float64, device=pred.device)
    ws = torch.empty(max(1, int(lib.vqae_recon_metrics_workspace_bytes(B, C, H, W))), dtype=torch.uint8,
                     device=pred.device)
    m, s = _norm255(mean, std) if u8 else (None, None)
    L.check(lib.vqae_recon_metrics_f32(ops._p(pred), None if u8 else ops._p(target), ops._p(target) if u8 else None, m, s,
                                       B, C, H, W, L.LAYOUT_NCHW if layout == "NCHW" else L.LAYOUT_NHWC,
                                       float(huber_delta), ops._p(out), ops._p(ws), ops._stream()))
    return out


def recon_metrics(pred, target, layout="NCHW", huber_delta=1.0, mean=MEAN, std=STD) -> Dict[str, torch.Tensor]:
    """Per-image metrics of the reconstruction `pred` against `target`, one HIP call: {'mse', 'huber', 'psnr', 'ssim',
    'pred_min', 'pred_max', 'target_min', 'target_max'} -> fp64 tensors [B] on the device.  A uint8 NHWC `target`
    (raw patches) is normalised on the device with (mean, std), the reference's transform (camelyon16_transforms.yaml)."""
    out = recon_metrics_raw(pred, target, layout, huber_delta, mean, std)
    return {n: out[:, i] for i, n in enumerate(NAMES)}


def psnr_from(mse, lo, hi):
    """10 log10((hi - lo)^2 / mse) in fp64 (torchmetrics 0.8.2 PeakSignalNoiseRatio with data_range=None)."""
    r = hi - lo
    return 10.0 * torch.log10(r * r / mse)


class ReconMetrics:
    """Drop-in for the reference's `metrics=` argument (a torchmetrics.MetricCollection of MeanSquaredError,
    PeakSignalNoiseRatio and StructuralSimilarityIndexMeasure; model.py:91-93, eval.py:25-31): `metrics(preds, target)`
    returns {'MeanSquaredError', 'PeakSignalNoiseRatio', 'StructuralSimilarityIndexMeasure'} of that batch (mean over its
    images) from ONE kernel call and accumulates the per-image values; `compute()` returns the mean over every image
    updated so far, summed across ranks under torch.distributed; `reset()` clears.

    As in torchmetrics, PSNR takes the data range of `target` -- the reference passes (batch, out), so that is the
    reconstruction.  Either argument may be the uint8 NHWC raw patch batch; the other is then fp32 NCHW."""

    KEYS = ("MeanSquaredError", "PeakSignalNoiseRatio", "StructuralSimilarityIndexMeasure")

    def __init__(self, huber_delta=1.0, mean=MEAN, std=STD):
        self.huber_delta, self.mean, self.std = huber_delta, mean, std
        self.reset()

    def reset(self):
        self._sum = None
        self._n = 0

    def rows(self, preds, target):
        """[B, 3] fp64 per-image (mse, psnr, ssim) in the torchmetrics argument order."""
        swap = preds.dtype == torch.uint8                 # the kernel normalises a uint8 operand only as its target
        pred_k, tgt_k = (target, preds) if swap else (preds, target)
        r = recon_metrics(pred_k, tgt_k, "NCHW", self.huber_delta, self.mean, self.std)
        lo, hi = (r["pred_min"], r["pred_max"]) if swap else (r["target_min"], r["target_max"])
        return torch.stack([r["mse"], psnr_from(r["mse"], lo, hi), r["ssim"]], 1)

    def update(self, preds, target):
        rows = self.rows(preds, target)
        s = rows.sum(0)
        self._sum = s if self._sum is None else self._sum + s
        self._n += rows.shape[0]
        return rows

    def __call__(self, preds, target):
        rows = self.update(preds, target)
        return dict(zip(self.KEYS, rows.mean(0)))

    forward = __call__

    def compute(self):
        s = self._sum if self._sum is not None else torch.zeros(3, dtype=torch.float64)
        tot = torch.cat([s.reshape(3), torch.tensor([float(self._n)], dtype=torch.float64, device=s.device)])
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            if dist.get_backend() == "gloo" and tot.is_cuda:
                host = tot.cpu()
                dist.all_reduce(host)
                tot = host.to(tot.device)
            else:
                dist.all_reduce(tot)
        return dict(zip(self.KEYS, tot[:3] / tot[3]))
