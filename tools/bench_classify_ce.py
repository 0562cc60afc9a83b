#!/usr/bin/env python3
"""Cost of the multi-class route of the slide classifier on resident uint8 code grids and labels, one GPU, the shipped stack
with three outputs (K 256, E 1, C 8, n_out 3), class weights [0, 0.0247, 0.9753], label smoothing 0.001, reduction 'mean':

    (a) fused_forward_ce    one vqae_classifier_forward_ce call: the uint8 class map and the stats rows (confusion counts, loss)
    (b) fused_loss_grad_ce  one vqae_classifier_loss_grad_ce call: loss, stats and the seven gradients
    (c) fused_train_step    ClassifierTrainer(loss='ce').step: (b) plus the AdamW step on the device image
    (d) stock               forward + F.cross_entropy + backward() of the same layers as torch modules on int64 codes and
                            labels, for the sizes up to --stock-max-codes (the first step at a new size includes MIOpen's
                            kernel search, minutes at 4096 x 4096; the record says which sizes have it)
    (e) bce_loss_grad       the n_out = 1 step of tools/bench_classify_train.py (vqae_classifier_loss_grad, pos_weight
                            40.4858, 'sum') on the same build, for the ratio (b) / (e)

at 1024 x 1024, 4096 x 4096 and 6144 x 12288 codes, in one process: HIP events around `steps` whole steps, the variants
alternating round by round, the median round reported with the fastest and slowest.  No ratio is fixed in advance.

The one timing condition of the multi-class work is on the n_out = 1 step, which shares its kernels' source: it must not be
slower than the commit before.  --bce-parent / --bce-this take records written by tools/bench_classify_train.py on the two
builds on one machine (several repeats each); their fused_loss_grad medians go into this record, and per size the verdict is
    median of this build's repeats <= median of the parent's repeats + (slowest - fastest of the parent's repeats).

    python tools/bench_classify_ce.py [--sizes ... --steps 10 --rounds 5 --out profiles/classify_ce.json]
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
from vqae_amd.optim import ClassifierTrainer  # noqa: E402

K, E, C, NO = 256, 1, 8, 3
WEIGHT = [0.0, 0.0247, 0.9753]
SMOOTH = 0.001
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


def make(n_out):
    torch.manual_seed(0)
    clf = CNNClassifier(K, E, C, n_out)
    with torch.no_grad():
        for m in clf.layers:
            if isinstance(m, torch.nn.Conv2d):
                m.weight.normal_(0.0, 1.6 / (m.in_channels * 9) ** 0.5)
                m.bias.normal_(0.0, 0.3)
    return clf


def run_size(clf3, clf1, trainer, stock, h, w, steps, stock_steps, rounds, warmup):
    rs = np.random.RandomState(0)
    codes = torch.from_numpy(rs.randint(0, K, (1, h, w)).astype(np.uint8)).cuda()
    labels = torch.from_numpy(rs.randint(0, 3, (1, h, w)).astype(np.uint8)).cuda()
    nat3, nat1 = clf3.native(), clf1.native()
    kw = dict(weight=WEIGHT, label_smoothing=SMOOTH)
    fns = {"fused_forward_ce": (lambda: nat3.forward_ce(codes, cls=True, labels=labels, **kw), steps),
           "fused_loss_grad_ce": (lambda: nat3.loss_grad_ce(codes, labels, reduction="mean", **kw), steps),
           "fused_train_step": (lambda: trainer.step(codes, labels, reduction="mean"), steps),
           "bce_loss_grad": (lambda: nat1.loss_grad(codes, labels, pos_weight=POS_WEIGHT), steps)}
    if stock is not None:
        codes64, labels64 = codes[:, None].long(), labels.long()
        wt = torch.tensor(WEIGHT, device="cuda")

        def stock_step():
            for p in stock.parameters():
                p.grad = None
            loss = F.cross_entropy(stock(codes64), labels64, weight=wt, label_smoothing=SMOOTH)
            loss.backward()
            return loss

        fns["stock"] = (stock_step, stock_steps)
    for i in range(warmup):
        for k, (fn, _) in fns.items():
            t0 = time.time()
            fn()
            torch.cuda.synchronize()
            note(f"{h}x{w} warm-up {i} {k}: {time.time() - t0:.3f} s")
    grad_diff = loss_diff = None
    if stock is not None:                                           # the two paths agree before anything is timed
        loss_a, packed, _ = nat3.loss_grad_ce(codes, labels, reduction="mean", **kw)
        loss_b = fns["stock"][0]()
        gb = torch.cat([p.grad.flatten() for p in stock.parameters()]).double()
        grad_diff = float((packed - gb).abs().max() / gb.abs().max())
        loss_diff = abs(float(loss_a) - float(loss_b.detach())) / abs(float(loss_b.detach()))
        del packed, gb, loss_b
    ms = {k: [] for k in fns}
    for r in range(rounds):
        for k, (fn, n) in fns.items():
            ms[k].append(timed(fn, n))
        note(f"{h}x{w} round {r}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in ms.items()))
    rec = {"h": h, "w": w, "codes": h * w, "rel_grad_diff_fused_vs_stock": grad_diff, "rel_loss_diff_fused_vs_stock": loss_diff}
    if stock is None:
        rec["stock"] = "not run (--stock-max-codes)"
    for k, v in ms.items():
        rec[k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    a = rec["fused_loss_grad_ce"]["ms_median"]
    rec["fused_loss_grad_ce"]["ns_per_code"] = round(a * 1e6 / (h * w), 3)
    rec["ce_over_bce_loss_grad"] = round(a / rec["bce_loss_grad"]["ms_median"], 3)
    rec["train_over_forward_ce"] = round(a / rec["fused_forward_ce"]["ms_median"], 2)
    if stock is not None:
        rec["stock_over_fused"] = round(rec["stock"]["ms_median"] / a, 2)
        for p in stock.parameters():
            p.grad = None
    return rec


def bce_condition(parent_files, this_files):
    """fused_loss_grad medians of bench_classify_train.py records of the two builds -> per size the repeats and the verdict"""
    def load(files):
        per = {}
        for f in files:
            for s in json.load(open(f))["sizes"]:
                per.setdefault(f"{s['h']}x{s['w']}", []).append(s["fused_loss_grad"]["ms_median"])
        return per
    parent, this = load(parent_files), load(this_files)
    out = {"rule": "median(this) <= median(parent) + (max(parent) - min(parent)) over the repeats' medians, per size", "sizes": {}}
    for size in parent:
        p, t = parent[size], this.get(size, [])
        rec = {"parent_ms": p, "this_ms": t, "parent_median": statistics.median(p), "parent_spread": round(max(p) - min(p), 4)}
        if t:
            rec["this_median"] = statistics.median(t)
            rec["not_slower"] = bool(rec["this_median"] <= rec["parent_median"] + rec["parent_spread"])
        out["sizes"][size] = rec
    out["not_slower"] = all(r.get("not_slower", False) for r in out["sizes"].values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024x1024,4096x4096,6144x12288")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--stock-steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stock-max-codes", type=int, default=4096 * 4096, help="leave the stock modules out above this many codes")
    ap.add_argument("--bce-parent", nargs="*", default=[], help="bench_classify_train.py records of the parent commit's build")
    ap.add_argument("--bce-this", nargs="*", default=[], help="... and of this build, same machine")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify_ce.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classify_ce.py needs a GPU")
    clf3, clf1 = make(NO), make(1)
    trainer = ClassifierTrainer(make(NO), "adamw", lr=1e-3, loss="ce", class_weight=WEIGHT, label_smoothing=SMOOTH)
    stock = copy.deepcopy(clf3.layers).cuda()
    for p in stock.parameters():
        p.requires_grad_(True)
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    rec = {"tool": "tools/bench_classify_ce.py", "device": torch.cuda.get_device_name(0),
           "variant": {"K": K, "E": E, "C": C, "n_out": NO}, "class_weight": WEIGHT, "label_smoothing": SMOOTH, "reduction": "mean",
           "bce_variant": {"K": K, "E": E, "C": C, "n_out": 1, "pos_weight": POS_WEIGHT, "reduction": "sum"},
           "steps": args.steps, "stock_steps": args.stock_steps, "rounds": args.rounds,
           "timing": "HIP events around `steps` whole steps; the variants alternate round by round; median (min, max) round",
           "sizes": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for h, w in sizes:
        with_stock = h * w <= args.stock_max_codes
        rec["sizes"].append(run_size(clf3, clf1, trainer, stock if with_stock else None, h, w, args.steps, args.stock_steps,
                                     args.rounds, args.warmup))
        torch.cuda.empty_cache()
        with open(args.out, "w") as f:                              # after every size: a long run leaves what it has
            json.dump(rec, f, indent=1)
            f.write("\n")
    if args.bce_parent:
        rec["n_out_1_step_vs_parent"] = bce_condition(args.bce_parent, args.bce_this)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))
    if args.bce_parent and not rec["n_out_1_step_vs_parent"]["not_slower"]:
        raise SystemExit("the n_out = 1 step is slower than the parent's beyond the spread of the parent's own repeats")


if __name__ == "__main__":
    main()
