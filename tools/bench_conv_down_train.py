#!/usr/bin/env python3
"""Times the trainable 2x2, stride-2 conv kernels (csrc/conv_train.hip, the conv_down="hip" route of vqae_amd.train) on
one GPU against the "torch" route -- fixup_act / fixup_add of csrc/fixup_train.hip in front of F.conv2d(stride=2), which is what
train.py ran before the keyword existed.  The method is tools/bench_conv1x1_train.py's: HIP events around `reps` calls, the
sides alternating inside every round after a warm-up, median (min - max) over the rounds.

    ops       forward and backward at the two convs of each 'down' block of cfg B at batch 16, 256 x 256 patches (branch_conv2
              behind ELU(x + a) + b: 32 -> 32 at 256^2, 64 -> 64 at 128^2, 128 -> 128 at 64^2; skip_conv behind x + c: 16 -> 32,
              32 -> 64, 64 -> 128) and at cfg C's 256 -> 256 conv (64^2): the fused node against the torch route's ops for the
              same work (fixup_act + F.conv2d forward; aten.convolution_backward + fixup_act_backward), and against a device
              copy of the algorithmic bytes (forward 4 (4 Ci + Co) B per output row, backward 4 (Co + 8 Ci) B)
    block     forward + backward of cfg B's first 'down' block (16 -> 32, batch 16, 256^2), "hip" against "torch", with
              torch.cuda.max_memory_allocated of one call of each side; --launches: kernel launches per call from rocprofv3
              --kernel-trace runs of this script's --child mode (two runs per side that differ by 10 iterations)
    step      a whole train.step + backward of cfg B (256 x 256 patches) at --step-batch under the four combinations of
              conv1x1 and conv_down, with peak memory

    python tools/bench_conv_down_train.py [--rounds 9 --reps 10 --step-batch 16 --launches --out profiles/conv_down_train.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vqae_amd  # noqa: E402
from vqae_amd import ops, train  # noqa: E402
from vqae_amd.layers.conv_block import PreActFixupResBlock  # noqa: E402
from bench_fixup_train import summary, timed  # noqa: E402

# (name, batch, H = W of the input, Ci, Co, pre)
OP_SHAPES = [("B_down0_branch", 16, 256, 32, 32, 2), ("B_down0_skip", 16, 256, 16, 32, 1),
             ("B_down1_branch", 16, 128, 64, 64, 2), ("B_down1_skip", 16, 128, 32, 64, 1),
             ("B_down2_branch", 16, 64, 128, 128, 2), ("B_down2_skip", 16, 64, 64, 128, 1),
             ("C_down2_branch", 16, 64, 256, 256, 2)]
BLOCK = (16, 16, 32, 256)                        # batch, cin, cout, H = W
ROUTES = ("hip", "torch")
MFMA_PEAK = 157.3e12


def bench_ops(reps, rounds):
    out = {}
    for (name, B, H, ci, co, pre) in OP_SHAPES:
        gen = torch.Generator().manual_seed(ci + co)
        x = torch.randn(B, H, H, ci, generator=gen).cuda()
        g = torch.randn(B, H // 2, H // 2, co, generator=gen).cuda()
        # channels_last, what the reference trains in (w_layout 1); the block and the step below hold contiguous weights (0)
        w = (torch.randn(co, ci, 2, 2, generator=gen) / (4 * ci) ** 0.5).cuda().contiguous(memory_format=torch.channels_last)
        a, b = (torch.tensor([v]).cuda() for v in (0.03, -0.02))
        a = a if pre == 2 else None
        u = ops.fixup_act(x, a, b)
        un, gn = u.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2)
        m = B * (H // 2) ** 2

        def torch_fwd():
            return F.conv2d(ops.fixup_act(x, a, b).permute(0, 3, 1, 2), w, stride=2)

        def torch_bwd():
            g_u, g_w, _ = torch.ops.aten.convolution_backward(gn, un, w, None, [2, 2], [0, 0], [1, 1], False, [0, 0], 1,
                                                              [True, True, False])
            g_u = g_u.permute(0, 2, 3, 1).contiguous()
            return (ops.fixup_act_backward(g_u, x, a) if pre == 2 else ops.fixup_act_backward(g_u, None, None, act=False)), g_w

        fb, bb = 4 * (4 * ci + co) * m, 4 * (co + 8 * ci) * m
        copies = {}
        for byts in (fb, bb):
            src, dst = torch.empty(byts // 8, device="cuda"), torch.empty(byts // 8, device="cuda")
            copies[byts] = (lambda s=src, d=dst: d.copy_(s))
        fns = {"hip_fwd": lambda: ops.conv_down_train_forward(x, w, a, b), "torch_fwd": torch_fwd,
               "hip_bwd": lambda: ops.conv_down_train_backward(g, x, w, a, b), "torch_bwd": torch_bwd,
               "hip_bwd_data_only": lambda: ops.conv_down_train_backward(g, x, w, a, b, need_w=False),
               "hip_bwd_weight_only": lambda: ops.conv_down_train_backward(g, x, w, a, b, need_x=False),
               "copy_fwd": copies[fb], "copy_bwd": copies[bb]}
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                samples[k].append(timed(fn, reps))
        med = {k: statistics.median(v) for k, v in samples.items()}
        res = {"batch": B, "H": H, "Ci": ci, "Co": co, "pre": pre, "rows": m, "w_layout": 1,
               "us": {k: summary(v) for k, v in samples.items()}, "algorithmic_bytes": {"fwd": fb, "bwd": bb}}
        for d, flop in (("fwd", 2.0 * m * 4 * ci * co), ("bwd", 4.0 * m * 4 * ci * co)):
            res[d] = {"torch_over_hip": round(med[f"torch_{d}"] / med[f"hip_{d}"], 3),
                      "hip_over_copy": round(med[f"hip_{d}"] / med[f"copy_{d}"], 3),
                      "torch_over_copy": round(med[f"torch_{d}"] / med[f"copy_{d}"], 3),
                      "hip_mfma_peak_fraction": round(flop / (med[f"hip_{d}"] * 1e-6) / MFMA_PEAK, 4)}
        out[name] = res
        print(json.dumps({name: res}), flush=True)
        del x, g, u, un, gn, copies, fns
        torch.cuda.empty_cache()
    return out


def block_sides():
    B, cin, cout, H = BLOCK
    torch.manual_seed(cin)
    blk = PreActFixupResBlock(cin, cout, "down", n_layers=100).cuda()
    with torch.no_grad():
        for k, p in blk.named_parameters():
            if p.numel() == 1:
                p.fill_(0.9 if k == "scale" else 0.03)
        torch.nn.init.normal_(blk.branch_conv3.weight, std=0.5 / cout ** 0.5)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, cin, H, H, generator=gen).cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    g = torch.randn(B, cout, H // 2, H // 2, generator=gen).cuda().contiguous(memory_format=torch.channels_last)

    def run(route):
        train.block_forward(blk, x, conv_down=route).backward(g)
        x.grad = None
        for p in blk.parameters():
            p.grad = None

    return {r: (lambda r=r: run(r)) for r in ROUTES}


def peak_of(fn, unit):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / unit


def bench_block(reps, rounds):
    sides = block_sides()
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            samples[k].append(timed(fn, reps))
    res = {"batch_cin_cout_H": list(BLOCK), "reps": reps, "rounds": rounds, "us": {k: summary(v) for k, v in samples.items()},
           "max_memory_allocated_MiB": {k: round(peak_of(fn, 2 ** 20), 1) for k, fn in sides.items()}}
    train.stats.update(conv_down_hip=0, conv_down_fallbacks=0)
    sides["hip"]()
    res["hip_nodes"], res["hip_fallbacks"] = train.stats["conv_down_hip"], train.stats["conv_down_fallbacks"]
    res["ratio_torch_over_hip"] = round(res["us"]["torch"]["median"] / res["us"]["hip"]["median"], 3)
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

    def run(c1, cd):
        out, recon, (vq_loss,) = train.step(model, x, conv1x1=c1, conv_down=cd)
        (recon + vq_loss).backward()
        for q in model.parameters():
            q.grad = None

    sides = {f"conv1x1={c1},conv_down={cd}": (lambda c1=c1, cd=cd: run(c1, cd)) for c1 in ("torch", "hip") for cd in ("torch", "hip")}
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
    train.stats.update(conv_down_hip=0, conv_down_fallbacks=0)
    sides["conv1x1=torch,conv_down=hip"]()
    res["hip_nodes"], res["hip_fallbacks"] = train.stats["conv_down_hip"], train.stats["conv_down_fallbacks"]
    base = res["ms"]["conv1x1=torch,conv_down=torch"]["median"]
    res["ratio_of_default_over"] = {k: round(base / v["median"], 3) for k, v in res["ms"].items()}
    return res


def child(route, iters):
    sides = block_sides()
    for _ in range(iters):
        sides[route]()
    torch.cuda.synchronize()


def count_launches(route, iters, workdir):
    d = os.path.join(workdir, f"{route}_{iters}")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "--child", route, "--child-iters", str(iters)],
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
    ap.add_argument("--no-block", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_down_train.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv_down_train needs a GPU: there is no CPU timing"
    if args.child:
        return child(args.child, args.child_iters)
    out = {"device": torch.cuda.get_device_name(0), "wgrad_run_rows": ops.conv_down_train_wgrad_run(), "ops": None, "block": None,
           "step": None, "launches_per_block_fwd_bwd": None}
    out["ops"] = bench_ops(args.reps, args.rounds)
    if not args.no_block:
        out["block"] = bench_block(args.reps, args.rounds)
        print(json.dumps({"block": out["block"]}), flush=True)
    if not args.no_step:
        out["step"] = bench_step(args.step_batch, args.step_reps, args.step_rounds)
        print(json.dumps({"step": out["step"]}), flush=True)
    if args.launches:
        with tempfile.TemporaryDirectory() as wd:
            out["launches_per_block_fwd_bwd"] = {r: (count_launches(r, 15, wd) - count_launches(r, 5, wd)) / 10 for r in ROUTES}
        print(json.dumps({"launches_per_block_fwd_bwd": out["launches_per_block_fwd_bwd"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
