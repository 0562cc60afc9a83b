#!/usr/bin/env python3
"""Times the keyword conv_up of vqae_amd.train on one GPU: conv_up="hip" (an 'up' block's conv2 and skip_conv at low resolution,
the bicubic x2 inside the two fused ops of csrc/up_train.hip) against conv_up="torch" (the order train.py has always built) in
the same process.  The method is tools/bench_fixup_train.py's: HIP events around `reps` calls, the sides alternating inside
every round after a warm-up, median (min - max) over the rounds.

    kernels   the four entries of csrc/up_train.hip at cfg B's three 'up' levels, batch 16, against the composition of existing ops
              each replaces, against the stand-alone bicubic pair at the same shape, and against a device copy of the algorithmic
              bytes (stated per record: every tensor an entry must read or write, once)
    blocks    forward + backward of one 'up' block at cfg B's three levels (128 -> 64 from 32^2, 64 -> 32 from 64^2, 32 -> 16 from
              128^2), batch 16, under conv1x1 "torch" and "hip", with torch.cuda.max_memory_allocated of one call of each side;
              --launches: kernel launches per call from rocprofv3 --kernel-trace runs of this script's --child mode (two runs per
              side that differ by 10 iterations)
    step      a whole train.step + backward of cfg B (256 x 256 patches) at --step-batch: all keywords "torch", conv_up alone,
              the other four "hip", all five "hip", with peak memory

    python tools/bench_conv_up_train.py [--rounds 9 --reps 10 --step-batch 16 --launches --out profiles/conv_up_train.json]
"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vqae_amd  # noqa: E402
from vqae_amd import ops, train  # noqa: E402
from vqae_amd.layers.conv_block import PreActFixupResBlock  # noqa: E402
from bench_conv_train import alternate, peak_of  # noqa: E402

LEVELS = {"B_up0_128_64_32x32": (16, 128, 64, 32), "B_up1_64_32_64x64": (16, 64, 32, 64), "B_up2_32_16_128x128": (16, 32, 16, 128)}
OTHER4 = ("conv1x1", "conv_down", "conv3x3", "conv3x3z")


def bench_kernels(reps, rounds):
    out = {}
    P = lambda v: torch.tensor([v]).cuda()
    for level, (B, cin, cout, H) in LEVELS.items():
        for entry, C in (("up2_act", cin), ("fixup_out_up", cout)):
            gen = torch.Generator().manual_seed(C + H)
            low, big = torch.randn(B, H, H, C, generator=gen).cuda(), torch.randn(B, 2 * H, 2 * H, C, generator=gen).cuda()
            g = torch.randn(B, 2 * H, 2 * H, C, generator=gen).cuda()
            a, b, sc = P(0.03), P(-0.02), P(0.9)
            n_low, n_out = low.numel(), g.numel()
            if entry == "up2_act":
                v = ops.bicubic_up2_bias(low)
                fns = {"hip_fwd": lambda: ops.up2_act(low, a, b),
                       "composition_fwd": lambda: ops.fixup_act(ops.bicubic_up2_bias(low), a, b),
                       "hip_bwd": lambda: ops.up2_act_backward(g, low, a),
                       "composition_bwd": lambda: ops.bicubic_up2_backward(ops.fixup_act_backward(g, v, a)[0], want_bias=False)}
                byts = {"fwd": 4 * (n_low + n_out), "bwd": 4 * (n_out + 2 * n_low)}
                what = {"fwd": "read t_low, write y", "bwd": "read g and t_low, write g_t_low"}
            else:
                fns = {"hip_fwd": lambda: ops.fixup_out_up(big, low, sc, a, b),
                       "composition_fwd": lambda: ops.fixup_out(big, ops.bicubic_up2_bias(low), sc, a, b),
                       "hip_bwd": lambda: ops.fixup_out_up_backward(g, big, sc),
                       "composition_bwd": lambda: (ops.fixup_out_backward(g, big, sc), ops.bicubic_up2_backward(g, want_bias=False))}
                byts = {"fwd": 4 * (2 * n_out + n_low), "bwd": 4 * (3 * n_out + n_low)}
                what = {"fwd": "read t and s_low, write y", "bwd": "read g and t, write g_t and g_s_low"}
            # the stand-alone pair the fused entries stand in for, against its own bytes (low + out elements, both ways)
            fns["bicubic_fwd"] = lambda: ops.bicubic_up2_bias(low)
            fns["bicubic_bwd"] = lambda: ops.bicubic_up2_backward(g, want_bias=False)
            byts["bicubic"] = 4 * (n_low + n_out)
            for d, n in byts.items():
                src, dst = torch.empty(n // 8, device="cuda"), torch.empty(n // 8, device="cuda")
                fns["copy_" + d] = (lambda src=src, dst=dst: dst.copy_(src))
            us = alternate(fns, reps, rounds, 3)
            res = {"batch": B, "H_low": H, "C": C, "us": us, "algorithmic_bytes": byts, "bytes_counted": what}
            for d in ("fwd", "bwd"):
                hip, comp, cp = (us[f"{side}_{d}"]["median"] for side in ("hip", "composition", "copy"))
                res[d] = {"composition_over_hip": round(comp / hip, 3), "hip_over_copy": round(hip / cp, 3),
                          "composition_over_copy": round(comp / cp, 3),
                          "bicubic_alone_over_its_copy": round(us["bicubic_" + d]["median"] / us["copy_bicubic"]["median"], 3)}
            out[f"{level}/{entry}"] = res
            print(json.dumps({f"{level}/{entry}": res}), flush=True)
            del low, big, g, fns
            torch.cuda.empty_cache()
    return out


def block_sides(level, conv1x1):
    B, cin, cout, H = LEVELS[level]
    torch.manual_seed(cin)
    blk = PreActFixupResBlock(cin, cout, "up", n_layers=100).cuda()
    with torch.no_grad():
        for k, p in blk.named_parameters():
            if p.numel() == 1:
                p.fill_(0.9 if k == "scale" else 0.03)
        torch.nn.init.normal_(blk.branch_conv3.weight, std=0.5 / cout ** 0.5)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, cin, H, H, generator=gen).cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    g = torch.randn(B, cout, 2 * H, 2 * H, generator=gen).cuda().contiguous(memory_format=torch.channels_last)

    def run(conv_up):
        train.block_forward(blk, x, conv1x1=conv1x1, conv_up=conv_up).backward(g)
        x.grad = None
        for p in blk.parameters():
            p.grad = None

    return {"hip": lambda: run("hip"), "torch": lambda: run("torch")}


def bench_block(level, conv1x1, reps, rounds):
    sides = block_sides(level, conv1x1)
    B, cin, cout, H = LEVELS[level]
    res = {"batch_cin_cout_H": [B, cin, cout, H], "conv1x1": conv1x1, "reps": reps, "rounds": rounds,
           "us": alternate(sides, reps, rounds, 3),
           "max_memory_allocated_MiB": {k: round(peak_of(fn, 2 ** 20), 1) for k, fn in sides.items()}}
    train.stats.update(conv_up_hip=0, conv_up_fallbacks=0)
    sides["hip"]()
    res.update(hip_nodes=train.stats["conv_up_hip"], hip_fallbacks=train.stats["conv_up_fallbacks"])
    t, h = res["us"]["torch"], res["us"]["hip"]
    res["ratio_torch_over_hip"] = round(t["median"] / h["median"], 3)
    res["hip_slower_than_torch_by_more_than_torch_spread"] = bool(h["median"] - t["median"] > t["max"] - t["min"])
    return res


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
    x = O.make_patches(batch, 256, 0).cuda().contiguous(memory_format=torch.channels_last)

    def run(routes):
        out, recon, (vq_loss,) = train.step(model, x, **routes)
        (recon + vq_loss).backward()
        for q in model.parameters():
            q.grad = None

    four = dict.fromkeys(OTHER4, "hip")
    sides = {"all_torch": lambda: run({}), "conv_up_hip": lambda: run({"conv_up": "hip"}), "other_four_hip": lambda: run(four),
             "all_five_hip": lambda: run({**four, "conv_up": "hip"})}
    res = {"spec": "B", "batch": batch, "patch": 256, "reps": reps, "rounds": rounds, "ms": alternate(sides, reps, rounds, 2, 1e-3),
           "max_memory_allocated_GiB": {k: round(peak_of(fn, 2 ** 30, above_allocated=False), 2) for k, fn in sides.items()}}
    ms = {k: v["median"] for k, v in res["ms"].items()}
    res["ratio_all_torch_over_conv_up_hip"] = round(ms["all_torch"] / ms["conv_up_hip"], 3)
    res["ratio_other_four_hip_over_all_five_hip"] = round(ms["other_four_hip"] / ms["all_five_hip"], 3)
    return res


def count_launches(side, level, conv1x1, iters, workdir):
    import csv
    import glob
    import subprocess
    d = os.path.join(workdir, f"{side}_{iters}")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "--child", side, "--child-level", level, "--child-conv1x1", conv1x1,
                    "--child-iters", str(iters)], check=True, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
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
    ap.add_argument("--step-rounds", type=int, default=9)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-level", default=next(iter(LEVELS)))
    ap.add_argument("--child-conv1x1", default="hip")
    ap.add_argument("--child-iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv_up_train needs a GPU: there is no CPU timing"
    if args.child:
        fn = block_sides(args.child_level, args.child_conv1x1)[args.child]
        for _ in range(args.child_iters):
            fn()
        return torch.cuda.synchronize()
    out = {"device": torch.cuda.get_device_name(0), "tile": {"low_res_pixels_per_axis": 8, "channels": 16},
           "kernels": bench_kernels(args.reps, args.rounds), "blocks": {}, "step": None, "launches_per_block_fwd_bwd": None}
    for level in LEVELS:
        for conv1x1 in ("torch", "hip"):
            res = bench_block(level, conv1x1, args.reps, args.rounds)
            out["blocks"][f"{level}/conv1x1={conv1x1}"] = res
            print(json.dumps({f"{level}/conv1x1={conv1x1}": res}), flush=True)
            torch.cuda.empty_cache()
    if not args.no_step:
        out["step"] = bench_step(args.step_batch, args.step_reps, args.step_rounds)
        print(json.dumps({"step": out["step"]}), flush=True)
    if args.launches:
        level = next(iter(LEVELS))
        with tempfile.TemporaryDirectory() as wd:
            out["launches_per_block_fwd_bwd"] = {
                f"conv1x1={c}": {s: (count_launches(s, level, c, 15, wd) - count_launches(s, level, c, 5, wd)) / 10
                                 for s in ("hip", "torch")} for c in ("torch", "hip")}
        print(json.dumps({"launches_per_block_fwd_bwd": out["launches_per_block_fwd_bwd"]}), flush=True)
    path = args.out or os.path.join(ROOT, "profiles", "conv_up_train.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
