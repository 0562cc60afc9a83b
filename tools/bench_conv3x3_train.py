#!/usr/bin/env python3
"""Times the trainable circular 3x3 conv kernels (the Circ3x3 policy of csrc/conv_train.hip, the conv3x3="hip" route of
vqae_amd.train) on one GPU against the "torch" route -- fixup_act(..., halo=1) of csrc/fixup_train.hip in front of F.conv2d,
which is what train.py ran before the keyword existed.  The method is tools/bench_conv_down_train.py's: HIP events around `reps`
calls, the sides alternating inside every round after a warm-up, median (min - max) over the rounds.

    ops       forward and backward of branch_conv2 behind ELU(x + a) + b at cfg B's trunk shape (C = 128, 32^2, batch 64), at a
              high-resolution 'same' shape (C = 16, 256^2, batch 16) and at cfg C's C = 256 (32^2, batch 64): the fused node against
              the torch route's ops for the same work (fixup_act with halo + F.conv2d forward; aten.convolution_backward +
              fixup_act_backward), with the data-only and weight-only backward calls
    block     forward + backward of one 'same' block (C = 128, batch 64, 32^2) under all three keywords "hip" against all "torch",
              with torch.cuda.max_memory_allocated of one call of each side; --launches: kernel launches per call from rocprofv3
              --kernel-trace runs of this script's --child mode (two runs per side that differ by 10 iterations)
    step      a whole train.step + backward of cfg B (256 x 256 patches) at --step-batch under the eight combinations of
              conv1x1, conv_down and conv3x3, with peak memory

    python tools/bench_conv3x3_train.py [--rounds 9 --reps 10 --step-batch 16 --launches --out profiles/conv3x3_train.json]

`--existing-nodes PARENT.json NEW.json` adds the two lists of sha256 digests of the conv1x1 / conv_down nodes' outputs (one made
with the parent's build of the library, one with this one) under "existing_nodes" and states whether they are equal.
"""
import argparse
import csv
import glob
import itertools
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
from bench_fixup_train import make_block, summary, timed  # noqa: E402
from bench_conv_down_train import peak_of  # noqa: E402

# (name, batch, H = W, Ci, Co)
OP_SHAPES = [("B_trunk_128", 64, 32, 128, 128), ("hires_same_16", 16, 256, 16, 16), ("C_trunk_256", 64, 32, 256, 256)]
BLOCK = (64, 128, 32)                            # batch, C, H = W
SIDES = {"hip": dict(conv1x1="hip", conv_down="hip", conv3x3="hip"), "torch": dict(conv1x1="torch", conv_down="torch", conv3x3="torch")}
MFMA_PEAK = 157.3e12


def bench_ops(reps, rounds):
    out = {}
    for (name, B, H, ci, co) in OP_SHAPES:
        gen = torch.Generator().manual_seed(ci + co)
        x = torch.randn(B, H, H, ci, generator=gen).cuda()
        g = torch.randn(B, H, H, co, generator=gen).cuda()
        # channels_last, what the reference trains in (w_layout 1); the block and the step below hold contiguous weights (0)
        w = (torch.randn(co, ci, 3, 3, generator=gen) / (9 * ci) ** 0.5).cuda().contiguous(memory_format=torch.channels_last)
        a, b = (torch.tensor([v]).cuda() for v in (0.03, -0.02))
        un, gn = ops.fixup_act(x, a, b, 1).permute(0, 3, 1, 2), g.permute(0, 3, 1, 2)
        m = B * H * H

        def torch_fwd():
            return F.conv2d(ops.fixup_act(x, a, b, 1).permute(0, 3, 1, 2), w)

        def torch_bwd():
            g_u, g_w, _ = torch.ops.aten.convolution_backward(gn, un, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                              [True, True, False])
            return ops.fixup_act_backward(g_u.permute(0, 2, 3, 1).contiguous(), x, a, 1), g_w

        fns = {"hip_fwd": lambda: ops.conv3x3_train_forward(x, w, a, b), "torch_fwd": torch_fwd,
               "hip_bwd": lambda: ops.conv3x3_train_backward(g, x, w, a, b), "torch_bwd": torch_bwd,
               "hip_bwd_data_only": lambda: ops.conv3x3_train_backward(g, x, w, a, b, need_w=False),
               "hip_bwd_weight_only": lambda: ops.conv3x3_train_backward(g, x, w, a, b, need_x=False)}
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                samples[k].append(timed(fn, reps))
        med = {k: statistics.median(v) for k, v in samples.items()}
        res = {"batch": B, "H": H, "Ci": ci, "Co": co, "pre": 2, "rows": m, "w_layout": 1,
               "us": {k: summary(v) for k, v in samples.items()}}
        for d, flop in (("fwd", 2.0 * m * 9 * ci * co), ("bwd", 4.0 * m * 9 * ci * co)):
            res[d] = {"torch_over_hip": round(med[f"torch_{d}"] / med[f"hip_{d}"], 3),
                      "hip_mfma_peak_fraction": round(flop / (med[f"hip_{d}"] * 1e-6) / MFMA_PEAK, 4)}
        out[name] = res
        print(json.dumps({name: res}), flush=True)
        del x, g, un, gn, fns
        torch.cuda.empty_cache()
    return out


def block_sides():
    B, C, H = BLOCK
    blk = make_block(C)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, C, H, H, generator=gen).cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    g = torch.randn(B, C, H, H, generator=gen).cuda().contiguous(memory_format=torch.channels_last)

    def run(routes):
        train.block_forward(blk, x, **routes).backward(g)
        x.grad = None
        for p in blk.parameters():
            p.grad = None

    return {k: (lambda r=r: run(r)) for k, r in SIDES.items()}


def alternate(sides, reps, rounds, warm, scale=1.0):
    for fn in sides.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            samples[k].append(timed(fn, reps) * scale)
    return {k: summary(v) for k, v in samples.items()}


def bench_block(reps, rounds):
    sides = block_sides()
    res = {"batch_C_H": list(BLOCK), "mode": "same", "reps": reps, "rounds": rounds, "us": alternate(sides, reps, rounds, 3),
           "max_memory_allocated_MiB": {k: round(peak_of(fn, 2 ** 20), 1) for k, fn in sides.items()}}
    train.stats.update(conv3x3_hip=0, conv3x3_fallbacks=0)
    sides["hip"]()
    res["hip_nodes"], res["hip_fallbacks"] = train.stats["conv3x3_hip"], train.stats["conv3x3_fallbacks"]
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

    def run(**routes):
        out, recon, (vq_loss,) = train.step(model, x, **routes)
        (recon + vq_loss).backward()
        for q in model.parameters():
            q.grad = None

    sides = {}
    for c1, cd, c3 in itertools.product(("torch", "hip"), repeat=3):
        sides[f"conv1x1={c1},conv_down={cd},conv3x3={c3}"] = (lambda r=dict(conv1x1=c1, conv_down=cd, conv3x3=c3): run(**r))
    res = {"spec": "B", "batch": batch, "patch": 256, "reps": reps, "rounds": rounds, "ms": alternate(sides, reps, rounds, 2, 1e-3),
           "max_memory_allocated_GiB": {}}
    for k, fn in sides.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        res["max_memory_allocated_GiB"][k] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    train.stats.update(conv3x3_hip=0, conv3x3_fallbacks=0)
    sides["conv1x1=torch,conv_down=torch,conv3x3=hip"]()
    res["hip_nodes"], res["hip_fallbacks"] = train.stats["conv3x3_hip"], train.stats["conv3x3_fallbacks"]
    base = res["ms"]["conv1x1=torch,conv_down=torch,conv3x3=torch"]["median"]
    res["ratio_of_default_over"] = {k: round(base / v["median"], 3) for k, v in res["ms"].items()}
    return res


def child(side, iters):
    sides = block_sides()
    for _ in range(iters):
        sides[side]()
    torch.cuda.synchronize()


def count_launches(side, iters, workdir):
    d = os.path.join(workdir, f"{side}_{iters}")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "--child", side, "--child-iters", str(iters)],
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
    ap.add_argument("--existing-nodes", nargs=2, metavar=("PARENT_JSON", "NEW_JSON"), default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv3x3_train.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv3x3_train needs a GPU: there is no CPU timing"
    if args.child:
        return child(args.child, args.child_iters)
    out = {"device": torch.cuda.get_device_name(0), "wgrad_run_rows": ops.conv3x3_train_wgrad_run(), "ops": None, "block": None,
           "step": None, "launches_per_block_fwd_bwd": None, "existing_nodes": None}
    out["ops"] = bench_ops(args.reps, args.rounds)
    if not args.no_block:
        out["block"] = bench_block(args.reps, args.rounds)
        print(json.dumps({"block": out["block"]}), flush=True)
    if not args.no_step:
        out["step"] = bench_step(args.step_batch, args.step_reps, args.step_rounds)
        print(json.dumps({"step": out["step"]}), flush=True)
    if args.launches:
        with tempfile.TemporaryDirectory() as wd:
            out["launches_per_block_fwd_bwd"] = {s: (count_launches(s, 15, wd) - count_launches(s, 5, wd)) / 10 for s in SIDES}
        print(json.dumps({"launches_per_block_fwd_bwd": out["launches_per_block_fwd_bwd"]}), flush=True)
    if args.existing_nodes:
        parent, new = (json.load(open(p)) for p in args.existing_nodes)
        out["existing_nodes"] = {"what": "sha256 of y, g_x, g_w, g_a, g_b of conv1x1_train_* and conv_down_train_* at the op shapes of "
                                         "profiles/conv_train_refactor.json, parent build and this build, same seeded inputs",
                                 "equal": parent == new, "parent": parent, "new": new}
        print(json.dumps({"existing_nodes_equal": parent == new, "cases": len(new)}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
