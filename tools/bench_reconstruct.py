#!/usr/bin/env python3
"""Cost of the way back to pixels on one GPU, on resident code tiles: cfg B at batch 256 in fp32 and f16,

    decode_indices     codes -> fp32 NHWC reconstruction (the yardstick: unchanged by the pixel path)
    decode_indices_u8  codes -> uint8 NHWC pixels (the same decoder + vqae_pixels_u8)

timed in one process, the two alternating round by round (the median round counts), and the pixel kernel alone beside a
device-to-device copy that moves the same number of bytes.  Writes one JSON record.

    python tools/bench_reconstruct.py [--batch 256 --steps 10 --rounds 7 --warmup 2 --out profiles/reconstruct.json]

Requirement: decode_indices_u8 <= 1.03 x decode_indices in the same run.  The added pass moves 15 B per pixel (12 read,
3 written), 0.25 GB at this size, next to a decoder step of tens of milliseconds.  The pixel kernel's share of the copy
rate is recorded without a bar; at this size its 0.25 GB partly live in the 256 MB Infinity Cache, and so does the copy's."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vqae_amd  # noqa: E402

LIMIT = 1.03


def timed(fn, steps):
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps            # ms per call


def alternate(fns, steps, rounds):
    """{name: [ms per call, one per round]}: every round times each function in turn"""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, steps))
    return out


def run_decode(cfg, dtype, batch, size, steps, rounds, warmup):
    from oracle import vqae_oracle as O
    spec = vqae_amd.SPECS[cfg]
    nat = vqae_amd.NativeVQAE(spec, O.make_params(O.SPECS[cfg], 0), compute_dtype=None if dtype == "f32" else dtype)
    nat.reserve(batch, size, size)
    q = size // nat.factor
    idx = torch.from_numpy(np.random.RandomState(0).randint(0, spec.num_embeddings, size=(batch, q, q)).astype(np.uint8)).cuda()
    fns = {"decode_indices": lambda: nat.decode_indices(idx, "NHWC"), "decode_indices_u8": lambda: nat.decode_indices_u8(idx)}
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ms = alternate(fns, steps, rounds)
    a, b = statistics.median(ms["decode_indices"]), statistics.median(ms["decode_indices_u8"])
    nat.close()
    return {"dtype": dtype, "decode_indices_ms": round(a, 4), "decode_indices_u8_ms": round(b, 4), "ratio": round(b / a, 4),
            "tiles_per_s_u8": round(batch / b * 1e3, 1),
            "rounds_ms": {k: [round(v, 4) for v in vs] for k, vs in ms.items()}}


def run_pixels(batch, size, steps, rounds, warmup):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((batch, size, size, 3), generator=g, device="cuda") * 2.0
    npix = batch * size * size
    moved = 15 * npix                                # 12 B read + 3 B written per pixel
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda").random_()
    dst = torch.empty_like(src)
    fns = {"pixels_u8": lambda: vqae_amd.ops.pixels_u8(x, "NHWC"), "copy": lambda: dst.copy_(src)}
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ms = alternate(fns, steps, rounds)
    p, c = statistics.median(ms["pixels_u8"]), statistics.median(ms["copy"])
    return {"pixels": npix, "bytes_moved": moved, "pixels_u8_ms": round(p, 4), "copy_ms": round(c, 4),
            "pixels_u8_GB_per_s": round(moved / p / 1e6, 1), "copy_GB_per_s": round(moved / c / 1e6, 1),
            "share_of_copy_rate": round(c / p, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", default="f32,f16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruct.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reconstruct.py needs a GPU")
    size = 512 if args.config == "A" else 256
    rec = {"tool": "tools/bench_reconstruct.py", "device": torch.cuda.get_device_name(0), "config": args.config,
           "batch": args.batch, "tile_pixels": [size, size, 3], "steps": args.steps, "rounds": args.rounds,
           "timing": "HIP events around `steps` calls; the variants alternate round by round; median round",
           "decode": [run_decode(args.config, dt, args.batch, size, args.steps, args.rounds, args.warmup)
                      for dt in args.dtypes.split(",")]}
    torch.cuda.empty_cache()
    rec["pixel_kernel"] = run_pixels(args.batch, size, 5 * args.steps, args.rounds, args.warmup)
    rec["limit_ratio"] = LIMIT
    rec["limit_met"] = all(d["ratio"] <= LIMIT for d in rec["decode"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    if not rec["limit_met"]:
        raise SystemExit(f"decode_indices_u8 is slower than {LIMIT} x decode_indices")


if __name__ == "__main__":
    main()
