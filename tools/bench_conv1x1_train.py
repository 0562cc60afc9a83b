#!/usr/bin/env python3
"""Times the trainable 1x1 conv kernels (csrc/conv_train.hip, the conv1x1="hip" route of vqae_amd.train) on one GPU
against the "torch" route -- the fused element-wise ops of csrc/fixup_train.hip around F.conv2d, which is what train.py ran
before the keyword existed.  The method is tools/bench_fixup_train.py's: HIP events around `reps` calls, the sides
alternating inside every round after a warm-up, median (min - max) over the rounds.

    ops       forward and backward of ELU(x + a) + b -> 1x1 conv at (M, Ci, Co) = (65536, 128, 128), (1048576, 16, 16),
              (262144, 64, 64): the fused node against the torch route's ops for the same work (fixup_act + F.conv2d forward;
              aten.convolution_backward + fixup_act_backward), against a device copy of the algorithmic bytes (forward
              4 (Ci + Co) B per row, backward 4 (Co + 2 Ci) B per row) and as a fraction of the fp32 MFMA peak (157.3 TFLOP/s;
              forward 2 M Ci Co flop, backward 4 M Ci Co)
    blocks    forward + backward of one 'same' block, "hip" against "torch", at the two shapes of bench_fixup_train.py, with
              torch.cuda.max_memory_allocated of one call of each side; --launches: kernel launches per call from
              rocprofv3 --kernel-trace runs of this script's --child mode (two runs per side that differ by 10 iterations)
    step      a whole train.step + backward of cfg B (256 x 256 patches) at --step-batch, "hip" against "torch"
    check     whether the "torch" side of blocks and step lies within the min - max spread profiles/fixup_train.json
              recorded for the same code ("fused" there)

    python tools/bench_conv1x1_train.py [--rounds 9 --reps 10 --step-batch 16 --launches --out profiles/conv1x1_train.json]
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
from bench_fixup_train import BLOCK_SHAPES, make_block, summary, timed  # noqa: E402

OP_SHAPES = [(65536, 128, 128), (1048576, 16, 16), (262144, 64, 64)]
MFMA_PEAK = 157.3e12
ROUTES = ("hip", "torch")


def bench_ops(reps, rounds):
    out = {}
    for (m, ci, co) in OP_SHAPES:
        gen = torch.Generator().manual_seed(ci)
        # [B, H, W, C] with B H W = m, as the blocks hand it over; the torch route sees its NCHW-shaped view
        x = torch.randn(m // 1024, 32, 32, ci, generator=gen).cuda()
        g = torch.randn(m // 1024, 32, 32, co, generator=gen).cuda()
        w = (torch.randn(co, ci, 1, 1, generator=gen) / ci ** 0.5).cuda()
        a, b = (torch.tensor([v]).cuda() for v in (0.03, -0.02))
        u = ops.fixup_act(x, a, b)
        un, gn = u.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2)

        def torch_fwd():
            return F.conv2d(ops.fixup_act(x, a, b).permute(0, 3, 1, 2), w)

        def torch_bwd():
            g_u, g_w, _ = torch.ops.aten.convolution_backward(gn, un, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                              [True, True, False])
            return ops.fixup_act_backward(g_u.permute(0, 2, 3, 1).contiguous(), x, a), g_w

        fb, bb = 4 * (ci + co) * m, 4 * (co + 2 * ci) * m
        copies = {}
        for byts in (fb, bb):
            src, dst = torch.empty(byts // 8, device="cuda"), torch.empty(byts // 8, device="cuda")
            copies[byts] = (lambda s=src, d=dst: d.copy_(s))
        fns = {"hip_fwd": lambda: ops.conv1x1_train_forward(x, w, a, b), "torch_fwd": torch_fwd,
               "hip_bwd": lambda: ops.conv1x1_train_backward(g, x, w, a, b), "torch_bwd": torch_bwd,
               "hip_bwd_data_only": lambda: ops.conv1x1_train_backward(g, x, w, a, b, need_w=False),
               "hip_bwd_weight_only": lambda: ops.conv1x1_train_backward(g, x, w, a, b, need_x=False),
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
        res = {"us": {k: summary(v) for k, v in samples.items()}, "algorithmic_bytes": {"fwd": fb, "bwd": bb}}
        for d, flop in (("fwd", 2.0 * m * ci * co), ("bwd", 4.0 * m * ci * co)):
            res[d] = {"torch_over_hip": round(med[f"torch_{d}"] / med[f"hip_{d}"], 3),
                      "hip_over_copy": round(med[f"hip_{d}"] / med[f"copy_{d}"], 3),
                      "torch_over_copy": round(med[f"torch_{d}"] / med[f"copy_{d}"], 3),
                      "hip_mfma_peak_fraction": round(flop / (med[f"hip_{d}"] * 1e-6) / MFMA_PEAK, 4),
                      "torch_mfma_peak_fraction": round(flop / (med[f"torch_{d}"] * 1e-6) / MFMA_PEAK, 4)}
        out[f"M{m}_Ci{ci}_Co{co}"] = res
        print(json.dumps({f"M{m}_Ci{ci}_Co{co}": res}))
    return out


def block_sides(name):
    B, C, H, W = BLOCK_SHAPES[name]
    blk = make_block(C)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, C, H, W, generator=gen).cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    g = torch.randn(B, C, H, W, generator=gen).cuda().contiguous(memory_format=torch.channels_last)

    def run(route):
        train.block_forward(blk, x, conv1x1=route).backward(g)
        x.grad = None
        for p in blk.parameters():
            p.grad = None

    return {r: (lambda r=r: run(r)) for r in ROUTES}


def bench_block(name, reps, rounds):
    sides = block_sides(name)
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
    train.stats.update(conv1x1_hip=0, conv1x1_fallbacks=0)
    sides["hip"]()
    res["hip_nodes"], res["hip_fallbacks"] = train.stats["conv1x1_hip"], train.stats["conv1x1_fallbacks"]
    res["ratio_torch_over_hip"] = round(res["us"]["torch"]["median"] / res["us"]["hip"]["median"], 3)
    t = res["us"]["torch"]
    res["hip_slower_than_torch_by_more_than_torch_spread"] = bool(res["us"]["hip"]["median"] - t["median"] > t["max"] - t["min"])
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

    def run(route):
        out, recon, (vq_loss,) = train.step(model, x, conv1x1=route)
        (recon + vq_loss).backward()
        for q in model.parameters():
            q.grad = None

    sides = {r: (lambda r=r: run(r)) for r in ROUTES}
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
    train.stats.update(conv1x1_hip=0, conv1x1_fallbacks=0)
    sides["hip"]()
    res["hip_nodes"], res["hip_fallbacks"] = train.stats["conv1x1_hip"], train.stats["conv1x1_fallbacks"]
    res["ratio_torch_over_hip"] = round(res["ms"]["torch"]["median"] / res["ms"]["hip"]["median"], 3)
    return res


def check_against_recorded(out):
    """The "torch" route is the code profiles/fixup_train.json timed as "fused": inside that file's min - max spread?"""
    path = os.path.join(ROOT, "profiles", "fixup_train.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        old = json.load(f)
    res = {}
    for name, blk in out["blocks"].items():
        o = old["blocks"][name]["us"]["fused"]
        now = blk["us"]["torch"]["median"]
        res[name] = {"torch_route_median_us": now, "recorded_us": o, "within_recorded_spread": bool(o["min"] <= now <= o["max"])}
    if out.get("step") and old.get("step") and out["step"]["batch"] == old["step"]["batch"]:
        o = old["step"]["ms"]["fused"]
        now = out["step"]["ms"]["torch"]["median"]
        res["step"] = {"torch_route_median_ms": now, "recorded_ms": o, "within_recorded_spread": bool(o["min"] <= now <= o["max"])}
    return res


def child(route, name, iters):
    sides = block_sides(name)
    for _ in range(iters):
        sides[route]()
    torch.cuda.synchronize()


def count_launches(route, name, iters, workdir):
    d = os.path.join(workdir, f"{route}_{name}_{iters}")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "--child", route, "--child-shape", name, "--child-iters", str(iters)],
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
    ap.add_argument("--no-blocks", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-shape", default="trunk_C128_32x32")
    ap.add_argument("--child-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv1x1_train.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv1x1_train needs a GPU: there is no CPU timing"
    if args.child:
        return child(args.child, args.child_shape, args.child_iters)
    out = {"device": torch.cuda.get_device_name(0), "wgrad_run_rows": ops.conv1x1_train_wgrad_run(), "ops": None, "blocks": {},
           "step": None, "launches_per_block_fwd_bwd": None}
    out["ops"] = bench_ops(args.reps, args.rounds)
    if not args.no_blocks:
        for name in BLOCK_SHAPES:
            out["blocks"][name] = bench_block(name, args.reps, args.rounds)
            print(json.dumps({name: out["blocks"][name]}))
    if not args.no_step:
        out["step"] = bench_step(args.step_batch, args.step_reps, args.step_rounds)
        print(json.dumps({"step": out["step"]}))
    out["torch_route_against_fixup_train_json"] = check_against_recorded(out)
    print(json.dumps({"torch_route_against_fixup_train_json": out["torch_route_against_fixup_train_json"]}))
    if args.launches:
        with tempfile.TemporaryDirectory() as wd:
            out["launches_per_block_fwd_bwd"] = {
                r: (count_launches(r, "trunk_C128_32x32", 15, wd) - count_launches(r, "trunk_C128_32x32", 5, wd)) / 10
                for r in ROUTES}
        print(json.dumps({"launches_per_block_fwd_bwd": out["launches_per_block_fwd_bwd"]}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
