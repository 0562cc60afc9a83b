#!/usr/bin/env python3
"""Times the training path of the Fixup mirrors (vqae_amd.train, csrc/fixup_train.hip) on one GPU against the same block
written with stock torch ops (train.block_forward_torch: F.elu, F.pad, F.interpolate); both sides use the same F.conv2d.

    blocks    forward + backward of one 'same' block at cfg B's trunk (C = 128, 32 x 32) and at its C = 16, 256 x 256 level:
              the two sides alternate inside every round after a warm-up; median, min and max over the rounds of each side,
              torch.cuda.max_memory_allocated of one forward + backward of each side, and how many of train.py's layout
              checks copied (a conv result that did not come back channels_last)
    kernels   every new kernel against a device-to-device copy of its algorithmic bytes per element: activation forward 8
              (read x, write y), backward 12 (read g and x, write g_x), output op 12 / 12, plain-mode sum 4, bicubic 20 per
              input element either way (1 + 4 floats)
    step      a whole train.step + backward of cfg B (256 x 256 patches) at --step-batch, fused against the stock-torch
              forward of the same mirror; nothing is read back inside the timed window
    launches  (--launches) kernel launches per block forward + backward of each side, from rocprofv3 --kernel-trace runs of
              this script's --child mode: two runs per side that differ by 10 iterations, so warm-up launches cancel

    python tools/bench_fixup_train.py [--rounds 9 --reps 10 --step-batch 16 --launches --out profiles/fixup_train.json]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vqae_amd  # noqa: E402
from vqae_amd import ops, train  # noqa: E402
from vqae_amd.layers.fixup_train import PreActFixupResBlock  # noqa: E402

BLOCK_SHAPES = {"trunk_C128_32x32": (64, 128, 32, 32), "level_C16_256x256": (16, 16, 256, 256)}   # (batch, C, H, W)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per call


def summary(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def make_block(C):
    torch.manual_seed(C)
    blk = PreActFixupResBlock(C, C, "same", n_layers=100).cuda()
    with torch.no_grad():
        for k, p in blk.named_parameters():
            if p.numel() == 1:
                p.fill_(0.9 if k == "scale" else 0.03)
        torch.nn.init.normal_(blk.branch_conv3.weight, std=0.5 / C ** 0.5)
    return blk


def block_sides(name):
    B, C, H, W = BLOCK_SHAPES[name]
    blk = make_block(C)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, C, H, W, generator=gen).cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    g = torch.randn(B, C, H, W, generator=gen).cuda().contiguous(memory_format=torch.channels_last)
    xs, gs = x.detach().contiguous().requires_grad_(), g.contiguous()          # the stock side in torch's default layout

    def run(forward, xi, gi):
        forward(blk, xi).backward(gi)
        xi.grad = None
        for p in blk.parameters():
            p.grad = None

    return blk, {"fused": lambda: run(train.block_forward, x, g), "stock": lambda: run(train.block_forward_torch, xs, gs),
                 "stock_channels_last": lambda: run(train.block_forward_torch, x, g)}


def bench_block(name, reps, rounds):
    blk, sides = block_sides(name)
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            samples[k].append(timed(fn, reps))
    res = {"shape_BCHW": list(BLOCK_SHAPES[name]), "reps": reps, "rounds": rounds, "us": {k: summary(v) for k, v in samples.items()},
           "max_memory_allocated_MiB": {}}
    for k, fn in sides.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        res["max_memory_allocated_MiB"][k] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    train.stats.update(layout_checks=0, layout_copies=0)
    sides["fused"]()
    res["fused_layout_checks"], res["fused_layout_copies"] = train.stats["layout_checks"], train.stats["layout_copies"]
    res["ratio_stock_over_fused"] = round(res["us"]["stock"]["median"] / res["us"]["fused"]["median"], 3)
    return res


def bench_kernels(reps, rounds):
    out = {}
    for name, (B, C, H, W) in BLOCK_SHAPES.items():
        gen = torch.Generator().manual_seed(2)
        r = lambda *s: torch.randn(*s, generator=gen).cuda()
        x, g, t = r(B, H, W, C), r(B, H, W, C), r(B, H, W, C)
        gh = r(B, H + 2, W + 2, C)
        xq, gu = r(B, H // 2, W // 2, C), r(B, H, W, C)           # bicubic: the op's OUTPUT has the level's size
        a, b = (torch.tensor([v]).cuda() for v in (0.03, -0.02))
        n = x.numel()
        fns = {"act_fwd": (8 * n, lambda: ops.fixup_act(x, a, b)),
               "act_fwd_halo": (8 * n, lambda: ops.fixup_act(x, a, b, halo=1)),
               "act_bwd": (12 * n, lambda: ops.fixup_act_backward(g, x, a)),
               "act_bwd_halo": (12 * n, lambda: ops.fixup_act_backward(gh, x, a, halo=1)),
               "plain_bwd": (4 * n, lambda: ops.fixup_act_backward(g, None, None, act=False)),
               "out_fwd": (12 * n, lambda: ops.fixup_out(t, x, a, b)),
               "out_bwd": (12 * n, lambda: ops.fixup_out_backward(g, t, a)),
               "bicubic_fwd": (20 * xq.numel(), lambda: ops.bicubic_up2_bias(xq, a)),
               "bicubic_fwd_inference_kernel": (20 * xq.numel(), lambda: ops.bicubic_up2(xq)),
               "bicubic_bwd": (20 * xq.numel(), lambda: ops.bicubic_up2_backward(gu))}
        copies = {}
        for byts in sorted({v[0] for v in fns.values()}):
            src, dst = torch.empty(byts // 8, device="cuda"), torch.empty(byts // 8, device="cuda")
            copies[byts] = (lambda s=src, d=dst: d.copy_(s))
        for fn in [v[1] for v in fns.values()] + list(copies.values()):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in list(fns) + [f"copy_{b}" for b in copies]}
        for _ in range(rounds):
            for k, (_, fn) in fns.items():
                samples[k].append(timed(fn, reps))
            for byts, fn in copies.items():
                samples[f"copy_{byts}"].append(timed(fn, reps))
        res = {}
        for k, (byts, _) in fns.items():
            med, cp = statistics.median(samples[k]), statistics.median(samples[f"copy_{byts}"])
            res[k] = {"algorithmic_bytes": byts, "us": summary(samples[k]), "copy_us": summary(samples[f"copy_{byts}"]),
                      "TBps_algorithmic": round(byts / med * 1e-6, 3), "ratio_over_copy": round(med / cp, 3)}
        out[name] = res
    return out


def stock_forward(model, x):
    """VQAE.forward of the mirror with stock torch ops on NCHW tensors: train.block_forward_torch blocks, the same quantiser."""
    enc, dec, bft = model.encoder, model.decoder, train.block_forward_torch
    h = F.conv2d(x, enc.in_stem.weight, enc.in_stem.bias, padding=1)
    for level in enc.down_layers[0].layers:
        for blk in level.layers:
            h = bft(blk, h)
    for blk in enc.pre_enc_layers[0]:
        h = bft(blk, h)
    h, _, vq_loss = enc.vq_layers[0](h)
    for blk in dec.post_enc_layers[0]:
        h = bft(blk, h)
    for level in dec.up_layers[0].layers:
        for blk in level.layers:
            h = bft(blk, h)
    return F.conv2d(h, dec.out_stem.weight, dec.out_stem.bias, padding=1), (vq_loss,)


def bench_step(batch, reps, rounds):
    from oracle import vqae_oracle as O
    from vqae_amd.model import VQAE
    spec = O.SPECS["B"]
    model = VQAE.from_spec(vqae_amd.SPECS["B"])
    p = O.make_params(spec, 0)
    vq = "encoder.vq_layers.0."
    p.update({vq + "embed_avg": p[vq + "embed"].clone(), vq + "cluster_size": torch.ones(spec.num_embeddings),
              vq + "first_pass": torch.as_tensor(0)})
    model.load_state_dict(p)
    model = model.cuda().train()
    x = O.make_patches(batch, 256, 0).cuda()
    xcl = x.contiguous(memory_format=torch.channels_last)

    def run(forward, xi):
        out, (vq_loss,) = forward(model, xi)
        (F.huber_loss(input=out, target=xi) + vq_loss).backward()
        for q in model.parameters():
            q.grad = None

    sides = {"fused": lambda: run(train.forward_train, xcl), "stock": lambda: run(stock_forward, x)}
    for fn in sides.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            samples[k].append(timed(fn, reps) / 1e3)             # ms
    res = {"spec": "B", "batch": batch, "patch": 256, "reps": reps, "rounds": rounds, "ms": {k: summary(v) for k, v in samples.items()},
           "max_memory_allocated_GiB": {}}
    for k, fn in sides.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        res["max_memory_allocated_GiB"][k] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    res["ratio_stock_over_fused"] = round(res["ms"]["stock"]["median"] / res["ms"]["fused"]["median"], 3)
    return res


def child(side, name, iters):
    _, sides = block_sides(name)
    for _ in range(iters):
        sides[side]()
    torch.cuda.synchronize()


def count_launches(side, name, iters, workdir):
    d = os.path.join(workdir, f"{side}_{name}_{iters}")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "--child", side, "--child-shape", name, "--child-iters", str(iters)],
                   check=True, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rows = 0
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += sum(1 for _ in csv.reader(f)) - 1
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--step-batch", type=int, default=16)
    ap.add_argument("--step-reps", type=int, default=2)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-shape", default="trunk_C128_32x32")
    ap.add_argument("--child-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixup_train.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fixup_train needs a GPU: there is no CPU timing"
    if args.child:
        return child(args.child, args.child_shape, args.child_iters)
    out = {"device": torch.cuda.get_device_name(0), "blocks": {}, "kernels": None, "step": None, "launches_per_block_fwd_bwd": None}
    for name in BLOCK_SHAPES:
        out["blocks"][name] = bench_block(name, args.reps, args.rounds)
        print(json.dumps({name: out["blocks"][name]}))
    out["kernels"] = bench_kernels(args.reps, args.rounds)
    print(json.dumps({"kernels": out["kernels"]}))
    if not args.no_step:
        out["step"] = bench_step(args.step_batch, args.step_reps, args.step_rounds)
        print(json.dumps({"step": out["step"]}))
    if args.launches:
        with tempfile.TemporaryDirectory() as wd:
            out["launches_per_block_fwd_bwd"] = {
                side: (count_launches(side, "trunk_C128_32x32", 15, wd) - count_launches(side, "trunk_C128_32x32", 5, wd)) / 10
                for side in ("fused", "stock")}
        print(json.dumps({"launches_per_block_fwd_bwd": out["launches_per_block_fwd_bwd"]}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
