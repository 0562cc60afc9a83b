#!/usr/bin/env python3
"""Cost of one whole training step of the slide classifier -- loss, gradients AND the optimiser -- on resident uint8 code
grids and masks, one GPU, the shipped variant (K 256, E 1, C 8, n_out 1), pos_weight 40.4858, reduction 'sum':

    (a) the host-side step   loss_and_grads (fused HIP backward, stats read back, gradients sliced into `.grad`) +
                             optimizer.step() of torch.optim.AdamW, or of the Lamb mirror, over the module's parameters;
                             the next call re-packs and uploads the stepped weights.  Parameters in HBM (`cuda`) and on the
                             host (`cpu`), both.
    (b) the device step      ClassifierTrainer.step with AdamW, LAMB and SAM + AdamW (two loss_grad passes): loss_grad and the
                             optimiser kernel on the handle's own weight image, nothing read back.

at 256 x 256, 1024 x 1024 and 4096 x 4096 codes, in one process and one run: wall-clock time of `steps` steps between two
device synchronisations (the host-side step blocks inside; HIP events would not see the host's share; `--steps` at
4096 x 4096, up to 20 x as many on the smaller grids so that a window lasts a tenth of a second or more), the variants
alternating round by round after a warm-up, the median round reported with the fastest and slowest.  The bar: (b) is not
slower than (a) with the same optimiser at any size, against the faster placement of (a); no ratio is fixed in advance.
At every size the optimiser kernel alone is timed too (HIP events around `steps` vqae_classifier_optim_step calls on a
resident gradient) for its share of a device step.

    python tools/bench_classify_optim.py [--sizes ... --steps 20 --rounds 7 --out profiles/classify_optim.json]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vqae_amd  # noqa: E402,F401
from vqae_amd import _lib as L, ops  # noqa: E402
from vqae_amd.classifier import CNNClassifier  # noqa: E402
from vqae_amd.classifier_train import loss_and_grads  # noqa: E402
from vqae_amd.optim import ClassifierTrainer, Lamb  # noqa: E402

K, E, C, NO = 256, 1, 8, 1
POS_WEIGHT = 40.4858
HYPER = dict(lr=1e-5, betas=(0.9, 0.999))


def note(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def wall(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps              # ms per step


def events(fn, steps):
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps


def host_step(clf, opt, codes, mask):
    def step():
        opt.zero_grad(set_to_none=True)
        loss_and_grads(clf, codes, mask, pos_weight=POS_WEIGHT)
        opt.step()
    return step


def make(seed_clf, where):
    clf = copy.deepcopy(seed_clf)
    return clf.cuda() if where == "cuda" else clf


def run_size(seed_clf, h, w, steps, rounds, warmup):
    rs = np.random.RandomState(0)
    codes = torch.from_numpy(rs.randint(0, K, (1, h, w)).astype(np.uint8)).cuda()
    mask = torch.from_numpy(rs.randint(0, 3, (1, h, w)).astype(np.uint8)).cuda()
    fns, keep = {}, []
    for where in ("cuda", "cpu"):
        for name, cls, kw in (("adamw", torch.optim.AdamW, dict(weight_decay=0.01)), ("lamb", Lamb, {})):
            clf = make(seed_clf, where)
            fns[f"host_{name}_{where}"] = host_step(clf, cls(clf.parameters(), **HYPER, **kw), codes, mask)
            keep.append(clf)
    trainers = {"adamw": ClassifierTrainer(make(seed_clf, "cpu"), "adamw", **HYPER),
                "lamb": ClassifierTrainer(make(seed_clf, "cpu"), "lamb", **HYPER),
                "sam_adamw": ClassifierTrainer(make(seed_clf, "cpu"), "adamw", sam_rho=0.05, **HYPER)}
    for name, tr in trainers.items():
        fns["device_" + name] = (lambda tr=tr: tr.step(codes, mask, pos_weight=POS_WEIGHT))
    for i in range(warmup):
        for k, fn in fns.items():
            t0 = time.time()
            fn()
            torch.cuda.synchronize()
            note(f"{h}x{w} warm-up {i} {k}: {time.time() - t0:.3f} s")
    ms = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            ms[k].append(wall(fn, steps))
        note(f"{h}x{w} round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in ms.items()))
    rec = {"h": h, "w": w, "codes": h * w}
    for k, v in ms.items():
        rec[k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    # the optimiser kernel alone, on a resident gradient
    lib = L.lib()
    for name in ("adamw", "lamb"):
        tr = trainers[name]
        g = torch.zeros(lib.vqae_classifier_grad_floats(tr.native._h), dtype=torch.float64, device="cuda")
        one = (lambda tr=tr, g=g: L.check(lib.vqae_classifier_optim_step(tr._opt_h, ops._p(g), ops._stream())))
        one()
        t = statistics.median(events(one, steps) for _ in range(rounds))
        rec[f"optim_kernel_{name}"] = {"ms_median": round(t, 5), "share_of_device_step": round(t / rec["device_" + name]["ms_median"], 4)}
    for name in ("adamw", "lamb"):
        best = min(rec[f"host_{name}_cuda"]["ms_median"], rec[f"host_{name}_cpu"]["ms_median"])
        rec[f"host_over_device_{name}"] = round(best / rec["device_" + name]["ms_median"], 2)
    rec["sam_over_plain_adamw"] = round(rec["device_sam_adamw"]["ms_median"] / rec["device_adamw"]["ms_median"], 2)
    rec["bar_met"] = bool(rec["host_over_device_adamw"] >= 1.0 and rec["host_over_device_lamb"] >= 1.0)
    for tr in trainers.values():
        tr.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256x256,1024x1024,4096x4096")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify_optim.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classify_optim.py needs a GPU")
    torch.manual_seed(0)
    clf = CNNClassifier(K, E, C, NO)
    with torch.no_grad():
        for m in clf.layers:
            if isinstance(m, torch.nn.Conv2d):
                m.weight.normal_(0.0, 1.6 / (m.in_channels * 9) ** 0.5)
                m.bias.normal_(0.0, 0.3)
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    rec = {"tool": "tools/bench_classify_optim.py", "device": torch.cuda.get_device_name(0),
           "variant": {"K": K, "E": E, "C": C, "n_out": NO}, "pos_weight": POS_WEIGHT, "reduction": "sum", "hyper": HYPER,
           "steps_at_4096x4096": args.steps, "rounds": args.rounds,
           "timing": "wall clock of `steps` whole steps between two device synchronisations; the variants alternate round by "
                     "round; median (min, max) round.  optim_kernel_*: HIP events around `steps` optimiser steps alone",
           "bar": "device_<opt> <= the faster of host_<opt>_cuda / host_<opt>_cpu at every size", "sizes": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for h, w in sizes:
        steps = min(400, max(args.steps, args.steps * (4096 * 4096) // (h * w)))      # small grids: more steps, a window of >= 0.1 s
        rec["sizes"].append(dict(run_size(clf, h, w, steps, args.rounds, args.warmup), steps=steps))
        torch.cuda.empty_cache()
        rec["bar_met"] = all(r["bar_met"] for r in rec["sizes"])
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))
    if not rec["bar_met"]:
        raise SystemExit("the device step is slower than the host-side step somewhere")


if __name__ == "__main__":
    main()
