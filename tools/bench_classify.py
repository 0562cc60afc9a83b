#!/usr/bin/env python3
"""Cost of the slide classifier on resident uint8 code grids, one GPU, the shipped variant (K 256, E 1, C 8, n_out 1):

    (a) fused_logits      vqae_classifier_forward, logits only
    (b) fused_heat_stats  vqae_classifier_forward, uint8 heat + masked stats, no logits
    (c) stock             the same layers as torch modules on the same device (nn.Embedding -> permute -> Conv2d -> ELU ->
                          Conv2d -> ELU -> Conv2d) on int64 codes, in the default and in the channels_last memory format,
                          the faster of the two

at 1024 x 1024, 4096 x 4096 and 6144 x 12288 codes, in one process: HIP events around `steps` calls, the variants alternating
round by round, the median round reported with the fastest and slowest.  The bar is (a) < (c) at every size; no ratio is
fixed in advance.

Besides the times the record holds, per size, what the kernel executes and moves, computed from shapes:
  flop_executed   2 * 9 * (E*C over the tile + 2, C*C over the tile + 1, C*n_out over the tile) per 14 x 62 tile, halo
                  recompute included, and flop_algorithmic = 1440 per code;
  share_of_fp32_vector_peak = flop_executed / time / 157.3 TFLOP/s;
  hbm_bytes       codes read once plus the outputs written once (a: 1 + 4 B per code; b: 1 + 1 + 1 B), and
                  hbm_bytes_with_halo, which counts the (14 + 6) x (62 + 6) codes every tile loads.

    python tools/bench_classify.py [--sizes 1024x1024,4096x4096,6144x12288 --steps 20 --rounds 5 --out profiles/classify.json]
"""
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
from vqae_amd.classifier import CNNClassifier  # noqa: E402

PEAK_FP32_VECTOR = 157.3e12
TH, TW = 14, 62                      # csrc/classifier.hip: the tile of the C = 8, E <= 6 geometry
K, E, C, NO = 256, 1, 8, 1


def timed(fn, steps):
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps            # ms per call


def counts(h, w):
    tiles = -(-h // TH) * -(-w // TW)
    per_tile = 2 * 9 * ((TH + 4) * (TW + 4) * E * C + (TH + 2) * (TW + 2) * C * C + TH * TW * C * NO)
    return {"tiles": tiles, "flop_executed": tiles * per_tile, "flop_algorithmic": h * w * 2 * 9 * (E * C + C * C + C * NO),
            "halo_code_bytes": tiles * (TH + 6) * (TW + 6)}


def run_size(clf, stock, h, w, steps, stock_steps, rounds, warmup):
    rs = np.random.RandomState(0)
    codes = torch.from_numpy(rs.randint(0, K, (1, h, w)).astype(np.uint8)).cuda()
    mask = torch.from_numpy(rs.randint(0, 3, (1, h, w)).astype(np.uint8)).cuda()
    codes64 = codes[:, None].long()
    nat = clf.native()
    fns = {"fused_logits": (lambda: nat.forward(codes), steps),
           "fused_heat_stats": (lambda: nat.forward(codes, logits=False, heat=True, mask=mask, pos_weight=40.4858), steps)}
    for name, mod in stock.items():
        fns["stock_" + name] = (lambda mod=mod: mod(codes64), stock_steps)
    with torch.no_grad():
        for _ in range(warmup):
            for fn, _ in fns.values():
                fn()
        # the two paths agree before anything is timed
        diff = float((nat.forward(codes)[0] - stock["default"](codes64)).abs().max())
        ms = {k: [] for k in fns}
        for _ in range(rounds):
            for k, (fn, n) in fns.items():
                ms[k].append(timed(fn, n))
    c = counts(h, w)
    rec = {"h": h, "w": w, "codes": h * w, "max_abs_diff_fused_vs_stock": diff, **c}
    for k, v in ms.items():
        rec[k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    a, b = rec["fused_logits"]["ms_median"], rec["fused_heat_stats"]["ms_median"]
    best = min(stock, key=lambda n: rec["stock_" + n]["ms_median"])
    cms = rec["stock_" + best]["ms_median"]
    rec["stock_best"] = best
    rec["stock_over_fused_logits"] = round(cms / a, 2)
    rec["bar_met"] = bool(a < cms)
    for k, t, out_bytes in (("fused_logits", a, 4 * NO), ("fused_heat_stats", b, 2)):      # b: mask read + heat written
        rec[k]["share_of_fp32_vector_peak"] = round(c["flop_executed"] / (t * 1e-3) / PEAK_FP32_VECTOR, 4)
        rec[k]["tflops_executed"] = round(c["flop_executed"] / (t * 1e-3) / 1e12, 2)
        rec[k]["hbm_bytes"] = h * w * (1 + out_bytes)
        rec[k]["hbm_bytes_with_halo"] = c["halo_code_bytes"] + h * w * out_bytes
        rec[k]["GB_per_s"] = round(rec[k]["hbm_bytes"] / t / 1e6, 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024x1024,4096x4096,6144x12288")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--stock-steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classify.py needs a GPU")
    torch.manual_seed(0)
    clf = CNNClassifier(K, E, C, NO)
    with torch.no_grad():
        for m in clf.layers:
            if isinstance(m, torch.nn.Conv2d):
                m.weight.normal_(0.0, 1.6 / (m.in_channels * 9) ** 0.5)
                m.bias.normal_(0.0, 0.3)
    import copy
    stock = {"default": copy.deepcopy(clf.layers).cuda().eval(),
             "channels_last": copy.deepcopy(clf.layers).cuda().eval().to(memory_format=torch.channels_last)}
    rec = {"tool": "tools/bench_classify.py", "device": torch.cuda.get_device_name(0), "variant": {"K": K, "E": E, "C": C, "n_out": NO},
           "tile": [TH, TW], "steps": args.steps, "stock_steps": args.stock_steps, "rounds": args.rounds,
           "timing": "HIP events around `steps` calls; the variants alternate round by round; median (min, max) round",
           "peak_fp32_vector_flops": PEAK_FP32_VECTOR, "sizes": []}
    for s in args.sizes.split(","):
        h, w = (int(v) for v in s.split("x"))
        rec["sizes"].append(run_size(clf, stock, h, w, args.steps, args.stock_steps, args.rounds, args.warmup))
        torch.cuda.empty_cache()
    rec["bar"] = "fused_logits < stock at every size"
    rec["bar_met"] = all(r["bar_met"] for r in rec["sizes"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    if not rec["bar_met"]:
        raise SystemExit("the fused call is not faster than the stock modules at every size")


if __name__ == "__main__":
    main()
