#!/usr/bin/env python3
"""Times the backward of the projected quantiser (csrc/vq_backward.hip) on one GPU, at the bottleneck's shapes:

    (1) fused      ops.vq_projected_backward: all five gradients in one pass over g_out and x (+ the partial-row reduction)
         fused_pass_only: the same launch asked for g_x alone, i.e. without the second launch that adds the partial rows
    (2) torch      the same gradients from layers.vq.projected_backward_reference with stock torch ops, fp32, same GPU
    (3) copy       a device-to-device copy that moves the fused pass's compulsory traffic, 3 N C 4 bytes (g_out and x read,
                   g_x written): 1.5 N C floats read and as many written -- the floor
    (4) module     ProjectedEMAVectorQuantizer2d forward + backward (grad path) next to its no-grad forward, eval (fused
                   forward) and train (conv -> lookup -> EMA update -> conv)

Device events around `reps` back-to-back calls; the variants alternate inside every round (one process, same data), and the
JSON keeps the median and the minimum over rounds.  Rates are the algorithmic bytes 3 N C 4 over the time.

    python tools/bench_vq_backward.py [--shapes 262144x128,65536x256 --reps 20 --rounds 7 --out profiles/vq_backward.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vqae_amd  # noqa: E402
from vqae_amd.layers.vq import ProjectedEMAVectorQuantizer2d, projected_backward_reference  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per call


def bench_shape(N, C, reps, rounds):
    ops = vqae_amd.ops
    g = torch.Generator().manual_seed(N + C)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    x, g_out = r(N, C), r(N, C)
    w_in, b_in, w_out = r(8, C) / C ** 0.5, r(8) * 0.1, r(C, 8) * 0.4
    z = x @ w_in.t() + b_in
    q = r(256, 8)[torch.randint(0, 256, (N,), generator=g).cuda()]
    g_loss = torch.tensor(1.0).cuda()
    src, dst = r(N * C * 3 // 2), torch.empty(N * C * 3 // 2, device="cuda")
    side = int(round((N // 256) ** 0.5)) if N % 256 == 0 and int(round((N // 256) ** 0.5)) ** 2 == N // 256 else None
    B, H, W = (256, side, side) if side else (1, N // 64, 64)
    xin = r(B, C, H, W)
    gin = r(B, C, H, W)
    mods = {}
    for mode in ("eval", "train"):
        torch.manual_seed(1)
        m = ProjectedEMAVectorQuantizer2d(256, C, 0.25, 0.99, 1e-5, projection_dim=8).cuda().train(mode == "train")
        m.first_pass.mul_(0)
        mods[mode] = m

    def fwd_bwd(m):
        xi = xin.requires_grad_()
        out, _, loss = m(xi)
        torch.autograd.backward([out, loss], [gin, g_loss])
        xi.grad = None
        for p in m.parameters():
            p.grad = None

    def fwd(m):
        with torch.no_grad():
            m(xin)

    fns = {"fused": lambda: ops.vq_projected_backward(g_out, x, z, q, g_loss, w_in, w_out, 0.25),
           "fused_pass_only": lambda: ops.vq_projected_backward(g_out, x, z, q, g_loss, w_in, w_out, 0.25, (True, False, False, False, False)),
           "torch": lambda: projected_backward_reference(g_out, x, z, q, g_loss, 0.25, w_in, w_out),
           "copy": lambda: dst.copy_(src)}
    for mode, m in mods.items():
        fns[f"module_{mode}_fwd_bwd"] = (lambda m=m: fwd_bwd(m))
        fns[f"module_{mode}_fwd_no_grad"] = (lambda m=m: fwd(m))
    got = ops.vq_projected_backward(g_out, x, z, q, g_loss, w_in, w_out, 0.25)
    ref = projected_backward_reference(g_out.double(), x.double(), z.double(), q.double(), g_loss.double(), 0.25, w_in.double(),
                                       w_out.double())
    err = [float((a.double() - b).norm() / b.norm()) for a, b in zip(got, ref)]
    ref32 = projected_backward_reference(g_out, x, z, q, g_loss, 0.25, w_in, w_out)
    err32 = [float((a.double() - b).norm() / b.norm()) for a, b in zip(ref32, ref)]
    del ref, ref32
    for fn in fns.values():                            # every shape the window uses, warmed
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            samples[k].append(timed(fn, reps))
    byts = 3.0 * N * C * 4
    res = {"N": N, "C": C, "module_input": [B, C, H, W], "algorithmic_bytes": byts, "reps": reps, "rounds": rounds,
           "rel_l2_vs_fp64_fused": err, "rel_l2_vs_fp64_torch_fp32": err32, "us": {}}
    for k, v in samples.items():
        res["us"][k] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2)}
    med = lambda k: res["us"][k]["median"]
    res["fused_TBps_algorithmic"] = round(byts / med("fused") * 1e-6, 3)
    res["copy_TBps"] = round(byts / med("copy") * 1e-6, 3)
    res["ratio_fused_over_copy"] = round(med("fused") / med("copy"), 3)
    res["ratio_torch_over_fused"] = round(med("torch") / med("fused"), 3)
    for mode in mods:
        res[f"ratio_module_{mode}_fwd_bwd_over_fwd"] = round(med(f"module_{mode}_fwd_bwd") / med(f"module_{mode}_fwd_no_grad"), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="262144x128,65536x256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vq_backward.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vq_backward needs a GPU: there is no CPU timing"
    out = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for s in args.shapes.split(","):
        N, C = (int(v) for v in s.split("x"))
        res = bench_shape(N, C, args.reps, args.rounds)
        print(json.dumps(res))
        out["shapes"].append(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
