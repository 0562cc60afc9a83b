#!/usr/bin/env python3
"""Cost of the way back to pixels on one GPU, on resident code tiles: cfg B at batch 256 in fp32 and f16,

    decode_indices     codes -> fp32 NHWC reconstruction (the yardstick: unchanged by the pixel path)
    decode_indices_u8  codes -> uint8 NHWC pixels (the same decoder + vqae_pixels_u8)

timed in one process, the two alternating round by round (the median round counts), and the pixel kernel alone beside a
device-to-device copy that moves the same number of bytes.  Writes one JSON record.

    python tools/bench_reconstruct.py [--batch 256 --steps 10 --rounds 7 --warmup 2 --out profiles/reconstruct.json]
                                      [--levels 1,3,5,6 --levels-out profiles/reconstruct_levels.json]

Requirement: decode_indices_u8 <= 1.03 x decode_indices in the same run.  The added pass moves 15 B per pixel (12 read,
3 written), 0.25 GB at this size, next to a decoder step of tens of milliseconds.  The pixel kernel's share of the copy
rate is recorded without a bar; at this size its 0.25 GB partly live in the 256 MB Infinity Cache, and so does the copy's.

--levels (empty: none) adds the overview levels of vqae_pixels_u8_level to the same rounds and writes a second record:
decode_indices_u8(level=L) next to decode_indices under the same 1.03 limit, and each level's kernel alone next to the
level-0 kernel on the same tensor.  A level reads the same 12 B per pixel and writes 3 / 4^L B, at most 12.75 of level 0's 15 B,
so levels 1, 3 and 5 must be no slower than level 0; the margin is the spread the run itself shows for level 0 (its slowest
round over its median round).  Other levels are recorded without a bar."""
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
BARRED_LEVELS = (1, 3, 5)               # kernel alone: no slower than level 0 within level 0's own spread


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


def run_decode(cfg, dtype, batch, size, steps, rounds, warmup, levels=()):
    """(the record of the level-0 path, the record of the levels or None); all variants alternate in the same rounds"""
    from oracle import vqae_oracle as O
    spec = vqae_amd.SPECS[cfg]
    nat = vqae_amd.NativeVQAE(spec, O.make_params(O.SPECS[cfg], 0), compute_dtype=None if dtype == "f32" else dtype)
    nat.reserve(batch, size, size)
    q = size // nat.factor
    idx = torch.from_numpy(np.random.RandomState(0).randint(0, spec.num_embeddings, size=(batch, q, q)).astype(np.uint8)).cuda()
    fns = {"decode_indices": lambda: nat.decode_indices(idx, "NHWC"), "decode_indices_u8": lambda: nat.decode_indices_u8(idx)}
    for lv in levels:
        fns[f"level_{lv}"] = lambda lv=lv: nat.decode_indices_u8(idx, level=lv)
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ms = alternate(fns, steps, rounds)
    a, b = statistics.median(ms["decode_indices"]), statistics.median(ms["decode_indices_u8"])
    nat.close()
    rec = {"dtype": dtype, "decode_indices_ms": round(a, 4), "decode_indices_u8_ms": round(b, 4), "ratio": round(b / a, 4),
           "tiles_per_s_u8": round(batch / b * 1e3, 1),
           "rounds_ms": {k: [round(v, 4) for v in ms[k]] for k in ("decode_indices", "decode_indices_u8")}}
    if not levels:
        return rec, None
    lev = {"dtype": dtype, "decode_indices_ms": round(a, 4), "levels": []}
    for lv in levels:
        m = statistics.median(ms[f"level_{lv}"])
        lev["levels"].append({"level": lv, "decode_indices_u8_ms": round(m, 4), "ratio": round(m / a, 4),
                              "rounds_ms": [round(v, 4) for v in ms[f"level_{lv}"]]})
    return rec, lev


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


def run_pixel_levels(batch, size, levels, steps, rounds, warmup):
    """every level's kernel alone beside the level-0 kernel, on the tensor of run_pixels"""
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((batch, size, size, 3), generator=g, device="cuda") * 2.0
    npix = batch * size * size
    fns = {0: lambda: vqae_amd.ops.pixels_u8(x, "NHWC")}
    for lv in levels:
        fns[lv] = lambda lv=lv: vqae_amd.ops.pixels_u8(x, "NHWC", level=lv)
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ms = alternate(fns, steps, rounds)
    base = statistics.median(ms[0])
    spread = max(ms[0]) / base
    rec = {"pixels": npix, "level_0_ms": round(base, 4), "level_0_rounds_ms": [round(v, 4) for v in ms[0]],
           "level_0_spread": round(spread, 4), "barred_levels": [lv for lv in levels if lv in BARRED_LEVELS], "levels": []}
    for lv in levels:
        m = statistics.median(ms[lv])
        moved = 12 * npix + 3 * npix // 4 ** lv
        row = {"level": lv, "ms": round(m, 4), "ratio_to_level_0": round(m / base, 4), "bytes_moved": moved,
               "GB_per_s": round(moved / m / 1e6, 1), "rounds_ms": [round(v, 4) for v in ms[lv]]}
        if lv in BARRED_LEVELS:
            row["bar_met"] = bool(m <= base * spread)
        rec["levels"].append(row)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", default="f32,f16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruct.json"))
    ap.add_argument("--levels", default="1,3,5,6", help="overview levels to time as well (empty: none)")
    ap.add_argument("--levels-out", default=os.path.join(ROOT, "profiles", "reconstruct_levels.json"))
    args = ap.parse_args()
    levels = [int(v) for v in args.levels.split(",") if v.strip()]
    if any(not 1 <= lv <= vqae_amd._lib.MAX_PIXEL_LEVEL for lv in levels) or len(set(levels)) != len(levels):
        raise SystemExit(f"--levels {args.levels}: distinct levels 1 .. {vqae_amd._lib.MAX_PIXEL_LEVEL}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_reconstruct.py needs a GPU")
    size = 512 if args.config == "A" else 256
    head = {"tool": "tools/bench_reconstruct.py", "device": torch.cuda.get_device_name(0), "config": args.config,
            "batch": args.batch, "tile_pixels": [size, size, 3], "steps": args.steps, "rounds": args.rounds,
            "timing": "HIP events around `steps` calls; the variants alternate round by round; median round"}
    decode = [run_decode(args.config, dt, args.batch, size, args.steps, args.rounds, args.warmup, levels)
              for dt in args.dtypes.split(",")]
    rec = dict(head, decode=[d for d, _ in decode])
    torch.cuda.empty_cache()
    rec["pixel_kernel"] = run_pixels(args.batch, size, 5 * args.steps, args.rounds, args.warmup)
    rec["limit_ratio"] = LIMIT
    rec["limit_met"] = all(d["ratio"] <= LIMIT for d in rec["decode"])
    records = [(args.out, rec)]
    if levels:
        lev = dict(head, levels=levels, decode=[d for _, d in decode])
        torch.cuda.empty_cache()
        lev["pixel_kernel"] = run_pixel_levels(args.batch, size, levels, 5 * args.steps, args.rounds, args.warmup)
        lev["limit_ratio"] = LIMIT
        lev["limit_met"] = all(row["ratio"] <= LIMIT for d in lev["decode"] for row in d["levels"])
        lev["kernel_bars_met"] = all(row.get("bar_met", True) for row in lev["pixel_kernel"]["levels"])
        records.append((args.levels_out, lev))
    for path, r in records:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")
        print(json.dumps(r))
    if not rec["limit_met"]:
        raise SystemExit(f"decode_indices_u8 is slower than {LIMIT} x decode_indices")
    if levels and not lev["limit_met"]:
        raise SystemExit(f"decode_indices_u8 at a level is slower than {LIMIT} x decode_indices")
    if levels and not lev["kernel_bars_met"]:
        raise SystemExit("a level's kernel is slower than the level-0 kernel beyond level 0's own spread")


if __name__ == "__main__":
    main()
