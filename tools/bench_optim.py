#!/usr/bin/env python3
"""Cost of one optimiser step over the parameter list of an auto-encoder, one GPU: the fused multi-tensor step
(FusedAdamW, FusedLamb, SAM over FusedLamb; csrc/optim.hip) next to what it replaces --

    FusedAdamW       against torch.optim.AdamW in its default form (foreach on device tensors) and with fused=True where
                     the installed torch offers it;
    FusedLamb        against the `Lamb` mirror (per-tensor torch ops, two blocking norm reads per tensor);
    SAM(FusedLamb)   against SAM(Lamb), first_step + second_step;
    copy floor       a device-to-device copy that moves the bytes the step must: 28 B per element for Adam (read g, p, m, v,
                     write p, m, v), 40 B per element for LAMB (its second launch reads p, m, v and writes p again)

-- on the parameters of vqae_amd.model.VQAE.from_spec(SPECS["A"]) and SPECS["B"] with seeded values and gradients (the same
gradients every step; no forward or backward runs).  HIP events around `steps` steps (fewer for the mirrors, whose step takes
a thousand times longer), after a warm-up, the variants alternating round by round; the median round with the fastest and the
slowest.  The events see the host's share too: a mirror step blocks inside, and the device idles meanwhile.

    python tools/bench_optim.py [--specs A,B --steps 20 --rounds 7 --out profiles/optim.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vqae_amd  # noqa: E402,F401
from vqae_amd import _lib as L  # noqa: E402
from vqae_amd.model import VQAE  # noqa: E402
from vqae_amd.optim import SAM, FusedAdamW, FusedLamb, Lamb  # noqa: E402
from vqae_amd.spec import SPECS  # noqa: E402

HYPER = dict(lr=1e-4, betas=(0.9, 0.999), weight_decay=0.01)


def note(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def events(fn, steps):
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps                          # ms per step


def params_of(shapes, gen):
    ps = []
    for s in shapes:
        p = torch.nn.Parameter((torch.randn(s, generator=gen) * 0.1).cuda())
        p.grad = (torch.randn(s, generator=gen) * 0.01).cuda()
        ps.append(p)
    return ps


def sam_step(opt):
    def step():
        opt.first_step()
        opt.second_step()
    return step


def run_spec(name, steps, slow_steps, rounds, warmup):
    model = VQAE.from_spec(SPECS[name])
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    del model
    numel = [int(torch.Size(s).numel()) for s in shapes]
    total = sum(numel)
    n_small = sum(1 for k in numel if k <= L.OPTIM_SMALL)
    n_chunks = sum(-(-k // L.OPTIM_CHUNK) for k in numel if k > L.OPTIM_SMALL)
    gen = torch.Generator().manual_seed(0)
    fns, slow = {}, set()
    fns["fused_adamw"] = FusedAdamW(params_of(shapes, gen), **HYPER).step
    fns["torch_adamw"] = torch.optim.AdamW(params_of(shapes, gen), **HYPER).step
    try:
        fns["torch_adamw_fused"] = torch.optim.AdamW(params_of(shapes, gen), fused=True, **HYPER).step
    except (RuntimeError, TypeError, ValueError) as e:
        note(f"torch.optim.AdamW(fused=True) is not offered here: {e}")
    fns["fused_lamb"] = FusedLamb(params_of(shapes, gen), **HYPER).step
    fns["mirror_lamb"] = Lamb(params_of(shapes, gen), **HYPER).step
    fns["sam_fused_lamb"] = sam_step(SAM(params_of(shapes, gen), FusedLamb, rho=0.05, **HYPER))
    fns["sam_mirror_lamb"] = sam_step(SAM(params_of(shapes, gen), Lamb, rho=0.05, **HYPER))
    slow.update(("mirror_lamb", "sam_mirror_lamb"))
    for bpe, key in ((28, "copy_adam"), (40, "copy_lamb")):         # a copy reads and writes: half the bytes each way
        src = torch.empty(total * bpe // 8, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)
        fns[key] = (lambda src=src, dst=dst: dst.copy_(src))
    for i in range(warmup):
        for k, fn in fns.items():
            t0 = time.time()
            fn()
            torch.cuda.synchronize()
            note(f"{name} warm-up {i} {k}: {time.time() - t0:.4f} s")
    ms = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            ms[k].append(events(fn, slow_steps if k in slow else steps))
        note(f"{name} round {r}: " + ", ".join(f"{k} {v[-1]:.4f}" for k, v in ms.items()))
    rec = {"spec": name, "tensors": len(shapes), "elements": total, "small_tensors": n_small, "chunked_tensors": len(shapes) - n_small,
           "chunks": n_chunks, "workgroups_first_launch": n_chunks + -(-n_small // 4),
           "launches_per_step": {"fused_adamw": 1, "fused_lamb": 3, "sam_fused_lamb": 6,
                                 "note": "plus one table upload per call (two for SAM's first + second step)"},
           "steps": steps, "steps_mirrors": slow_steps}
    for k, v in ms.items():
        rec[k] = {"ms_median": round(statistics.median(v), 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5)}
    med = lambda k: rec[k]["ms_median"]
    rec["mirror_over_fused_lamb"] = round(med("mirror_lamb") / med("fused_lamb"), 1)
    rec["mirror_over_fused_sam_lamb"] = round(med("sam_mirror_lamb") / med("sam_fused_lamb"), 1)
    rec["torch_over_fused_adamw"] = round(med("torch_adamw") / med("fused_adamw"), 2)
    if "torch_adamw_fused" in rec:
        rec["torch_fused_over_fused_adamw"] = round(med("torch_adamw_fused") / med("fused_adamw"), 2)
    rec["fused_adamw_over_copy"] = round(med("fused_adamw") / med("copy_adam"), 2)
    rec["fused_lamb_over_copy"] = round(med("fused_lamb") / med("copy_lamb"), 2)
    rec["sam_fused_lamb_over_copy"] = round(med("sam_fused_lamb") / med("copy_lamb"), 2)
    # the bar: faster than the mirrors by more than the spread of the mirrors' own repeats
    rec["bar_met"] = bool(rec["fused_lamb"]["ms_max"] < rec["mirror_lamb"]["ms_min"] - (rec["mirror_lamb"]["ms_max"] - rec["mirror_lamb"]["ms_min"])
                          and rec["sam_fused_lamb"]["ms_max"] < rec["sam_mirror_lamb"]["ms_min"]
                          - (rec["sam_mirror_lamb"]["ms_max"] - rec["sam_mirror_lamb"]["ms_min"]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--specs", default="A,B")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--slow-steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs a GPU")
    rec = {"tool": "tools/bench_optim.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hyper": HYPER,
           "rounds": args.rounds,
           "timing": "HIP events around `steps` steps (steps_mirrors for the mirrors); the variants alternate round by round; "
                     "median (min, max) round, ms per step",
           "bar": "fused_lamb and sam_fused_lamb below mirror_lamb and sam_mirror_lamb by more than the mirrors' own spread",
           "specs": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.specs.split(","):
        rec["specs"].append(run_spec(name, args.steps, args.slow_steps, args.rounds, args.warmup))
        torch.cuda.empty_cache()
        rec["bar_met"] = all(r["bar_met"] for r in rec["specs"])
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))
    if not rec["bar_met"]:
        raise SystemExit("the fused step is not faster than the mirrors by more than their spread")


if __name__ == "__main__":
    main()
