#!/usr/bin/env python3
"""Validation throughput on one GPU, on a resident batch: images/s of the full forward alone and of forward + the
reconstruction-metrics kernels (metrics.recon_metrics), and the metrics kernels' own time and algorithmic bandwidth.
Prints one JSON line per config.

    python tools/bench_validate.py [--batch 256 --steps 20 --warmup 3 --configs A:bf16,A:f16,B:f32]

Algorithmic bytes of the metrics: pass 1 reads the prediction and the fp32 target once, pass 2 (SSIM) reads both again;
the SSIM pass's halo re-reads are not counted.  The fraction is of 6.3 TB/s, the rate a float4 copy reaches on the MI355X."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vqae_amd  # noqa: E402
from vqae_amd.metrics import recon_metrics_raw  # noqa: E402

COPY_TBPS = 6.3


def timed(fn, steps):
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps            # ms per step


def run(cfg, dtype, batch, steps, warmup):
    from oracle import vqae_oracle as O
    size = 512 if cfg == "A" else 256
    params = O.make_params(O.SPECS[cfg], 0)
    nat = vqae_amd.NativeVQAE(vqae_amd.SPECS[cfg], params, compute_dtype=None if dtype == "f32" else dtype)
    nat.reserve(batch, size, size)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((batch, 3, size, size), generator=g, device="cuda")
    nat.calibrate_codebook(x[:8], params["encoder.vq_layers.0.embed"])
    out = torch.empty_like(x)

    def fwd():
        nonlocal out
        out = nat.forward(x, "NCHW", want_idx=False)[0]

    def fwd_metrics():
        fwd()
        recon_metrics_raw(out, x)

    for _ in range(warmup):
        fwd_metrics()
    ms_fwd = timed(fwd, steps)
    ms_both = timed(fwd_metrics, steps)
    ms_met = timed(lambda: recon_metrics_raw(out, x), steps)
    rows = recon_metrics_raw(out, x).cpu()
    gbytes = 2 * 2 * x.numel() * 4 / 1e9             # two passes x (prediction + target)
    return {"config": cfg, "dtype": dtype, "batch": batch, "image": [3, size, size], "steps": steps,
            "forward_images_per_s": round(batch / ms_fwd * 1e3, 1),
            "forward_plus_metrics_images_per_s": round(batch / ms_both * 1e3, 1),
            "ratio": round(ms_fwd / ms_both, 4),
            "metrics_ms": round(ms_met, 4), "metrics_algorithmic_GB": round(gbytes, 3),
            "metrics_GB_per_s": round(gbytes / ms_met * 1e3, 1),
            "fraction_of_copy_rate": round(gbytes / ms_met * 1e3 / (COPY_TBPS * 1e3), 4),
            "mean_mse": float(rows[:, 0].mean()), "mean_ssim": float(rows[:, 3].mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="A:bf16,A:f16,B:f32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_validate.py needs a GPU")
    t0 = time.time()
    for item in args.configs.split(","):
        cfg, dt = item.split(":")
        print(json.dumps(run(cfg, dt, args.batch, args.steps, args.warmup)), flush=True)
        torch.cuda.empty_cache()
    print(f"# {time.time() - t0:.1f} s", file=sys.stderr)


if __name__ == "__main__":
    main()
