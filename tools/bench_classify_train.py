#!/usr/bin/env python3
"""Cost of one training step's loss and gradients of the slide classifier on resident uint8 code grids and masks, one GPU,
the shipped variant (K 256, E 1, C 8, n_out 1), pos_weight 40.4858, reduction 'sum':

    (a) fused_loss_grad   one vqae_classifier_loss_grad call: loss, stats and the seven gradients (csrc/classifier_train.hip)
    (b) stock             forward + BCEWithLogits over the valid codes (what Camelyon16BCELoss computes) + backward() of the
                          same layers as torch modules on the same device on int64 codes, in the default and in the
                          channels_last memory format, the faster of the two
    (c) fused_forward     vqae_classifier_forward with stats only: an inference step, for the ratio (a) / (c)

at 1024 x 1024, 4096 x 4096 and 6144 x 12288 codes, in one process: HIP events around `steps` whole steps, the variants
alternating round by round, the median round reported with the fastest and slowest.  The bar is (a) < (b) at every size; no
ratio is fixed in advance.  The peak device memory of one step of (a) and of (b) is recorded as well
(torch.cuda.max_memory_allocated over the step, above what is resident before it).
The first stock step at a new size includes MIOpen's kernel search for the three convolutions' forward, backward-data and
backward-weights problems: 21 s at 1024 x 1024 and 166 s (+ 95 s channels_last) at 4096 x 4096 were seen, more beyond.
--stock-max-codes N leaves the stock modules out above N codes (the record then says so and the bar is judged on the sizes
that have both).

Besides the times the record holds, per size, what (a) executes and moves, computed from shapes:
  flop_executed   the forward launch (as tools/bench_classify.py counts it) plus, per 14 x 62 tile of the backward launch,
                  2 * 9 * (E*C on tile+3, C*C on tile+2 [recompute]; C on tile+2 [dB]; C*C on tile+1 [dA]; C + C*C + 2*E*C
                  on the tile [the three weight correlations and dE0]);
  hbm_bytes       forward: code 1 + mask 1 read, dL/dlogit 4 written; backward: code 1 + dL/dlogit 4 read: 11 B per code,
                  and hbm_bytes_with_halo, which counts the (14+6) x (62+6) codes the forward and the (14+8) x (62+8) codes
                  plus (14+6) x (62+6) dL/dlogit values the backward load per tile.

    python tools/bench_classify_train.py [--sizes ... --steps 10 --rounds 5 --out profiles/classify_train.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vqae_amd  # noqa: E402,F401
from vqae_amd.classifier import CNNClassifier  # noqa: E402

PEAK_FP32_VECTOR = 157.3e12
TH, TW = 14, 62                      # the tile of the C = 8, E <= 6 geometry, forward and backward
K, E, C, NO = 256, 1, 8, 1
POS_WEIGHT = 40.4858


def note(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def timed(fn, steps):
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps            # ms per step


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def counts(h, w):
    tiles = -(-h // TH) * -(-w // TW)
    fwd = 2 * 9 * ((TH + 4) * (TW + 4) * E * C + (TH + 2) * (TW + 2) * C * C + TH * TW * C * NO)
    bwd = 2 * 9 * ((TH + 6) * (TW + 6) * E * C + (TH + 4) * (TW + 4) * (C * C + C) + (TH + 2) * (TW + 2) * C * C
                   + TH * TW * (C + C * C + 2 * E * C))
    halo = (TH + 6) * (TW + 6) + (TH + 8) * (TW + 8) + 4 * (TH + 6) * (TW + 6)
    return {"tiles": tiles, "flop_executed": tiles * (fwd + bwd), "flop_executed_forward": tiles * fwd,
            "hbm_bytes": 11 * h * w, "hbm_bytes_with_halo": tiles * halo + 5 * h * w}


def stock_step(mod, codes64, valid, target, pw):
    def step():
        for p in mod.parameters():
            p.grad = None
        out = mod(codes64)
        loss = F.binary_cross_entropy_with_logits(out[valid][None], target, pos_weight=pw, reduction="sum")
        loss.backward()
        return loss
    return step


def run_size(clf, stock, h, w, steps, stock_steps, rounds, warmup):
    rs = np.random.RandomState(0)
    codes = torch.from_numpy(rs.randint(0, K, (1, h, w)).astype(np.uint8)).cuda()
    mask = torch.from_numpy(rs.randint(0, 3, (1, h, w)).astype(np.uint8)).cuda()
    codes64 = codes[:, None].long()
    valid = (mask != 0)[:, None]
    target = (mask[:, None][valid] - 1).float()[None]
    pw = torch.tensor(POS_WEIGHT, device="cuda")
    nat = clf.native()
    fns = {"fused_loss_grad": (lambda: nat.loss_grad(codes, mask, pos_weight=POS_WEIGHT), steps),
           "fused_forward": (lambda: nat.forward(codes, logits=False, mask=mask, pos_weight=POS_WEIGHT), steps)}
    for name, mod in stock.items():
        fns["stock_" + name] = (stock_step(mod, codes64, valid, target, pw), stock_steps)
    for i in range(warmup):
        for k, (fn, _) in fns.items():
            t0 = time.time()
            fn()
            torch.cuda.synchronize()
            note(f"{h}x{w} warm-up {i} {k}: {time.time() - t0:.3f} s")      # (the first stock step includes MIOpen's kernel search)
    grad_diff = loss_diff = None
    if stock:                                                       # the two paths agree before anything is timed
        loss_a, packed, _ = nat.loss_grad(codes, mask, pos_weight=POS_WEIGHT)
        loss_b = fns["stock_default"][0]()
        gb = torch.cat([p.grad.flatten() for p in stock["default"].parameters()]).double()
        grad_diff = float((packed - gb).abs().max() / gb.abs().max())
        loss_diff = abs(float(loss_a) - float(loss_b.detach())) / abs(float(loss_b.detach()))
        del packed, gb, loss_b
    ms = {k: [] for k in fns}
    for r in range(rounds):
        for k, (fn, n) in fns.items():
            ms[k].append(timed(fn, n))
        note(f"{h}x{w} round {r}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in ms.items()))
    c = counts(h, w)
    rec = {"h": h, "w": w, "codes": h * w, "rel_grad_diff_fused_vs_stock": grad_diff, "rel_loss_diff_fused_vs_stock": loss_diff, **c}
    if not stock:
        rec["stock"] = "not run (--stock-max-codes)"
    for k, v in ms.items():
        rec[k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    a, f = rec["fused_loss_grad"]["ms_median"], rec["fused_forward"]["ms_median"]
    rec["train_over_inference_step"] = round(a / f, 2)
    if stock:
        best = min(stock, key=lambda n: rec["stock_" + n]["ms_median"])
        bms = rec["stock_" + best]["ms_median"]
        rec["stock_best"] = best
        rec["stock_over_fused"] = round(bms / a, 2)
        rec["bar_met"] = bool(a < bms)
    rec["fused_loss_grad"]["tflops_executed"] = round(c["flop_executed"] / (a * 1e-3) / 1e12, 2)
    rec["fused_loss_grad"]["share_of_fp32_vector_peak"] = round(c["flop_executed"] / (a * 1e-3) / PEAK_FP32_VECTOR, 4)
    rec["fused_loss_grad"]["GB_per_s"] = round(c["hbm_bytes"] / a / 1e6, 1)
    for mod in stock.values():
        for p in mod.parameters():
            p.grad = None
    rec["peak_bytes_fused"] = peak_bytes(fns["fused_loss_grad"][0])
    if stock:
        rec["peak_bytes_stock"] = peak_bytes(fns["stock_" + best][0])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024x1024,4096x4096,6144x12288")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--stock-steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stock-max-codes", type=int, default=0, help="leave the stock modules out above this many codes (0: never)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify_train.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classify_train.py needs a GPU")
    torch.manual_seed(0)
    clf = CNNClassifier(K, E, C, NO)
    with torch.no_grad():
        for m in clf.layers:
            if isinstance(m, torch.nn.Conv2d):
                m.weight.normal_(0.0, 1.6 / (m.in_channels * 9) ** 0.5)
                m.bias.normal_(0.0, 0.3)
    stock = {"default": copy.deepcopy(clf.layers).cuda(),
             "channels_last": copy.deepcopy(clf.layers).cuda().to(memory_format=torch.channels_last)}
    for mod in stock.values():
        for p in mod.parameters():
            p.requires_grad_(True)
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    rec = {"tool": "tools/bench_classify_train.py", "device": torch.cuda.get_device_name(0),
           "variant": {"K": K, "E": E, "C": C, "n_out": NO}, "pos_weight": POS_WEIGHT, "reduction": "sum", "tile": [TH, TW],
           "steps": args.steps, "stock_steps": args.stock_steps, "rounds": args.rounds,
           "timing": "HIP events around `steps` whole steps; the variants alternate round by round; median (min, max) round",
           "peak_fp32_vector_flops": PEAK_FP32_VECTOR, "sizes": []}
    rec["bar"] = "fused_loss_grad < stock at every size"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for h, w in sizes:
        with_stock = not args.stock_max_codes or h * w <= args.stock_max_codes
        rec["sizes"].append(run_size(clf, stock if with_stock else {}, h, w, args.steps, args.stock_steps, args.rounds, args.warmup))
        torch.cuda.empty_cache()
        rec["bar_met"] = all(r["bar_met"] for r in rec["sizes"] if "bar_met" in r)
        with open(args.out, "w") as f:                              # after every size: a long run leaves what it has
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))
    if not rec.get("bar_met", True):
        raise SystemExit("the fused step is not faster than the stock modules at every size")


if __name__ == "__main__":
    main()
