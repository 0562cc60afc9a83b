"""Dataset-level validation of a checkpoint: mirror of scripts/extract_validation_metrics/eval.py:13-45, which runs
`trainer.validate` under fp16 autocast with validation batch size 1 and logs, per step, VQAE.shared_step's
`val_recon_loss` (Huber, loss_f/huber.yaml), `val_encoding_loss_0` and the torchmetrics collection (model.py:82-93).

Here the forward runs on the HIP path in batches and the metrics come from one kernel call per batch (metrics.py); the
per-image values are what eval.py's batch-1 steps log, and every dataset value is their mean over the images (Lightning's
epoch mean of equally weighted steps).  The commitment loss is the forward's batch mean, weighted by the batch size.
"""
import contextlib
from typing import Callable, Optional

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import dist as vdist
from .extract_embeddings import _REF_AUTOCAST, ShardBatchSampler, _collate
from .metrics import psnr_from, recon_metrics

COLUMNS = ("mse", "huber", "psnr", "ssim", "encoding_loss")     # per-image rows, in this order


def _native(model):
    if hasattr(model, "with_dtype"):                               # NativeVQAE
        return model
    if hasattr(model, "native"):                                   # vqae_amd.model.VQAE mirror
        return model.native()
    raise TypeError("validate: model must be a NativeVQAE or a vqae_amd.model.VQAE")


def default_forward(model, autocast_dtype=_REF_AUTOCAST) -> Callable:
    """imgs on the device -> (out fp32 NCHW, commitment loss of the batch).  fp32 NCHW items run VQAE.forward; uint8 NHWC
    items (raw patches) run encode_u8(want_q=True) -> decode, normalised on the device."""
    nat = _native(model).with_dtype(autocast_dtype)

    def fwd(imgs):
        if imgs.dtype == torch.uint8:
            q, _, loss = nat.encode_u8(imgs, want_q=True)
            return nat.decode(q), loss
        out, _, loss = nat.forward(imgs.float(), "NCHW", want_idx=False)
        return out, loss
    return fwd


def default_metrics(huber_delta=1.0) -> Callable:
    """(out, imgs) -> [b, 4] fp64 (mse, huber, psnr, ssim) per image, one kernel call; a uint8 batch goes to the kernel as
    it is.  PSNR takes the range of the reconstruction: the reference logs `self.metrics(batch, out)` (model.py:92), and
    torchmetrics' PSNR tracks the range of its second argument."""
    def met(out, imgs):
        r = recon_metrics(out, imgs, "NCHW", huber_delta)
        return torch.stack([r["mse"], r["huber"], psnr_from(r["mse"], r["pred_min"], r["pred_max"]), r["ssim"]], 1)
    return met


def validate(model, dataset, batch_size=64, *, autocast_dtype=_REF_AUTOCAST, huber_delta=1.0, num_workers=0,
             device=None, shard=True, forward_fn: Optional[Callable] = None, metrics_fn: Optional[Callable] = None):
    """Score a model's reconstructions of `dataset` (items (img, ...) with img fp32 [3,H,W] or uint8 [H,W,3]).

    model: a NativeVQAE or a vqae_amd.model.VQAE mirror (as run_eval takes them); the forward runs with the convolutions
    in `autocast_dtype` (torch.float16 = eval.py's autocast, torch.bfloat16, or None for fp32).
    Returns {'val_recon_loss', 'val_encoding_loss_0', 'val_MeanSquaredError', 'val_PeakSignalNoiseRatio',
    'val_StructuralSimilarityIndexMeasure'} (floats, means over images), the per-image arrays COLUMNS in dataset order
    (numpy fp64; 'encoding_loss' holds the loss of the batch share an image was evaluated in) and 'n_images'.

    Under torch.distributed each rank loads and evaluates only its contiguous share of every batch (ShardBatchSampler; a
    share may be empty), then the small per-image rows are all-gathered, so every rank returns the same dict.
    forward_fn(imgs) -> (out, loss) and metrics_fn(out, imgs) -> [b, 4] replace the HIP forward / metrics kernel (the CPU
    tests of the host logic; the product default has no CPU fallback)."""
    device = torch.device(device) if device is not None else torch.device("cuda")
    rank, ws = vdist.world() if shard else (0, 1)
    fwd = forward_fn or default_forward(model, autocast_dtype)
    met = metrics_fn or default_metrics(huber_delta)
    n_items = len(dataset)
    sampler = ShardBatchSampler(n_items, batch_size, rank, ws)
    dl = DataLoader(dataset, batch_sampler=sampler, collate_fn=_collate, num_workers=num_workers,
                    pin_memory=device.type == "cuda")
    parts = []
    ctx = torch.inference_mode() if forward_fn is None else contextlib.nullcontext()
    with ctx:
        for collated in dl:
            if collated is None:                                   # empty share of a short last batch
                continue
            imgs = collated[0].to(device, non_blocking=True)
            out, loss = fwd(imgs)
            rows = met(out, imgs).to(torch.float64)
            parts.append(torch.cat([rows, torch.as_tensor(loss, dtype=torch.float64, device=rows.device)
                                    .reshape(1, 1).expand(rows.shape[0], 1)], 1))
    mine = torch.cat(parts, 0) if parts else torch.zeros((0, len(COLUMNS)), dtype=torch.float64, device=device)
    if ws > 1 and torch.distributed.get_backend() == "gloo":
        mine = mine.cpu()
    gathered = vdist.all_gather_ragged(mine.contiguous()) if ws > 1 else [mine]
    # rank r holds its shares of batches 0, 1, ... back to back: interleave them into dataset order
    offs, order = [0] * ws, []
    for b0 in range(0, n_items, batch_size):
        nb = min(batch_size, n_items - b0)
        for r in range(ws):
            lo, hi = vdist.shard_range(nb, r, ws)
            order.append(gathered[r][offs[r]: offs[r] + hi - lo])
            offs[r] += hi - lo
    allrows = (torch.cat(order, 0) if order else mine[:0]).cpu().numpy()
    res = {name: np.ascontiguousarray(allrows[:, i]) for i, name in enumerate(COLUMNS)}
    mean = lambda a: float(a.mean()) if a.size else float("nan")
    res.update({"val_recon_loss": mean(res["huber"]), "val_encoding_loss_0": mean(res["encoding_loss"]),
                "val_MeanSquaredError": mean(res["mse"]), "val_PeakSignalNoiseRatio": mean(res["psnr"]),
                "val_StructuralSimilarityIndexMeasure": mean(res["ssim"]), "n_images": int(allrows.shape[0])})
    return res
