#!/usr/bin/env python3
"""Times one trainable conv node of csrc/conv_train.hip (--node conv1x1 | conv_down | conv3x3: the keyword of vqae_amd.train of
the same name at "hip") on one GPU against the "torch" route -- the fused element-wise ops of csrc/fixup_train.hip around
F.conv2d, which is what train.py ran before the keyword existed.  The method is tools/bench_fixup_train.py's: HIP events around
`reps` calls, the sides alternating inside every round after a warm-up, median (min - max) over the rounds.

    ops       forward and backward of the node's op shapes (NODES below): the fused node against the torch route's ops for the
              same work (fixup_act + F.conv2d forward; aten.convolution_backward + fixup_act_backward), with the data-only and
              weight-only backward calls, against a device copy of the algorithmic bytes (forward 4 (s^2 Ci + Co) B per output
              row, backward 4 (Co + 2 s^2 Ci) B, s the stride) and as a fraction of the fp32 MFMA peak (157.3 TFLOP/s; forward
              2 M k^2 Ci Co flop, backward twice that).  Weights of more than one tap are channels_last, what the reference
              trains in (w_layout 1); the blocks and the step hold contiguous weights (0).
    blocks    forward + backward of the node's blocks, its "hip" side against all keywords at "torch", with
              torch.cuda.max_memory_allocated of one call of each side; --launches: kernel launches per call from rocprofv3
              --kernel-trace runs of this script's --child mode (two runs per side that differ by 10 iterations)
    step      a whole train.step + backward of cfg B (256 x 256 patches) at --step-batch under the eight combinations of conv1x1,
              conv_down and conv3x3, with peak memory
    check     (conv1x1) whether the all-"torch" side of blocks and step lies within the min - max spread profiles/fixup_train.json
              recorded for the same code ("fused" there)

    python tools/bench_conv_train.py --node conv3x3 [--rounds 9 --reps 10 --step-batch 16 --launches --out profiles/conv3x3_train.json]

--node conv3x3z times the zero-padded 3x3 node with a 3-channel side of csrc/conv_train_thin.hip (the stems, the skip_conv of an
'out' block) in the same way, with what differs stated in its record: the torch route is F.conv2d(x, w, bias, padding=1) on the
NCHW-shaped view and aten.convolution_backward, the layout copy of its result included (train._conv); in_stem shapes time the
backward without a data gradient (the batch needs none) on both sides; there is no block record (no shipped config has an 'out'
block); the step is cfg B under all four keywords "hip", under the other three alone, and under all "torch", with peak memory
and, with --launches, kernel launches per step.

    python tools/bench_conv_train.py --node conv3x3z [--launches --out profiles/conv3x3z_train.json]
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
from vqae_amd.layers.conv_block import PreActFixupResBlock  # noqa: E402
from bench_fixup_train import summary, timed  # noqa: E402

MFMA_PEAK = 157.3e12
KEYWORDS = ("conv1x1", "conv_down", "conv3x3")
# k, stride: the kernel;  halo: of the torch route's activation;  ops: (name, batch, H = W of the input, Ci, Co, pre);
# blocks: name -> (mode, batch, cin, cout, H = W), written under "blocks" by name, or, a node with one block, as "block";
# hip: the keywords of the "hip" side of blocks;  block_key: the block's shape under the key the node's recorded profile has
NODES = {
    "conv1x1": dict(k=1, stride=1, halo=0,
                    ops=[("M65536_Ci128_Co128", 64, 32, 128, 128, 2), ("M1048576_Ci16_Co16", 1024, 32, 16, 16, 2),
                         ("M262144_Ci64_Co64", 256, 32, 64, 64, 2)],
                    blocks={"trunk_C128_32x32": ("same", 64, 128, 128, 32), "level_C16_256x256": ("same", 16, 16, 16, 256)},
                    hip=("conv1x1",), block_key=lambda B, ci, co, H: {"shape_BCHW": [B, ci, H, H]}),
    "conv_down": dict(k=2, stride=2, halo=0,
                      ops=[("B_down0_branch", 16, 256, 32, 32, 2), ("B_down0_skip", 16, 256, 16, 32, 1),
                           ("B_down1_branch", 16, 128, 64, 64, 2), ("B_down1_skip", 16, 128, 32, 64, 1),
                           ("B_down2_branch", 16, 64, 128, 128, 2), ("B_down2_skip", 16, 64, 64, 128, 1),
                           ("C_down2_branch", 16, 64, 256, 256, 2)],
                      blocks={"block": ("down", 16, 16, 32, 256)},
                      hip=("conv_down",), block_key=lambda B, ci, co, H: {"batch_cin_cout_H": [B, ci, co, H]}),
    "conv3x3": dict(k=3, stride=1, halo=1,
                    ops=[("B_trunk_128", 64, 32, 128, 128, 2), ("hires_same_16", 16, 256, 16, 16, 2), ("C_trunk_256", 64, 32, 256, 256, 2)],
                    blocks={"block": ("same", 64, 128, 128, 32)},
                    hip=KEYWORDS, block_key=lambda B, ci, co, H: {"batch_C_H": [B, ci, H], "mode": "same"}),
    # ops: (name, batch, H = W, Ci, Co, whether the input needs a gradient); its own record (bench_ops_z, bench_step_z)
    "conv3x3z": dict(k=3, stride=1, halo=0,
                     ops=[("in_stem_3_16_256", 16, 256, 3, 16, False), ("out_stem_16_3_256", 16, 256, 16, 3, True),
                          ("in_stem_3_8_512", 8, 512, 3, 8, False), ("out_stem_8_3_512", 8, 512, 8, 3, True)],
                     blocks={}, hip=KEYWORDS + ("conv3x3z",), block_key=None),
}


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


def peak_of(fn, unit, above_allocated=True):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated() if above_allocated else 0
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / unit


def node_counts(node, fn):
    train.stats.update({node + "_hip": 0, node + "_fallbacks": 0})
    fn()
    return {"hip_nodes": train.stats[node + "_hip"], "hip_fallbacks": train.stats[node + "_fallbacks"]}


def bench_ops_z(reps, rounds):
    out = {}
    for (name, B, H, ci, co, need_x) in NODES["conv3x3z"]["ops"]:
        gen = torch.Generator().manual_seed(ci + co)
        x, g = torch.randn(B, H, H, ci, generator=gen).cuda(), torch.randn(B, H, H, co, generator=gen).cuda()
        w = (torch.randn(co, ci, 3, 3, generator=gen) / (9 * ci) ** 0.5).cuda().contiguous(memory_format=torch.channels_last)
        bias = torch.randn(co, generator=gen).cuda()
        xn, gn = x.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2)
        m = B * H * H

        def torch_fwd():
            return train.to_nhwc(F.conv2d(xn, w, bias, padding=1))

        def torch_bwd():
            g_x, g_w, g_bias = torch.ops.aten.convolution_backward(gn, xn, w, [co], [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                                   [need_x, True, True])
            return (train.to_nhwc(g_x) if need_x else None), g_w, g_bias

        byts = {"fwd": 4 * (ci + co) * m, "bwd": 4 * (co + ci + (ci if need_x else 0)) * m}
        fns = {"hip_fwd": lambda: ops.conv3x3z_train_forward(x, w, bias), "torch_fwd": torch_fwd,
               "hip_bwd": lambda: ops.conv3x3z_train_backward(g, x, w, None, need_x, True, True), "torch_bwd": torch_bwd,
               "hip_bwd_weight_only": lambda: ops.conv3x3z_train_backward(g, x, w, None, False, True, True)}
        if need_x:
            fns["hip_bwd_data_only"] = lambda: ops.conv3x3z_train_backward(g, x, w, None, True, False, False)
        for d, n in byts.items():
            src, dst = torch.empty(n // 8, device="cuda"), torch.empty(n // 8, device="cuda")
            fns["copy_" + d] = (lambda src=src, dst=dst: dst.copy_(src))
        us = alternate(fns, reps, rounds, 3)
        res = {"batch": B, "H": H, "Ci": ci, "Co": co, "pre": 0, "bias": True, "data_gradient": bool(need_x), "rows": m, "w_layout": 1,
               "us": us, "algorithmic_bytes": byts}
        for d in ("fwd", "bwd"):
            hip, tor, cp = (us[f"{side}_{d}"]["median"] for side in ("hip", "torch", "copy"))
            res[d] = {"torch_over_hip": round(tor / hip, 3), "hip_over_copy": round(hip / cp, 3), "torch_over_copy": round(tor / cp, 3)}
        out[name] = res
        print(json.dumps({name: res}), flush=True)
        del x, g, xn, gn, fns
        torch.cuda.empty_cache()
    return out


def step_model_z(batch):
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

    three = dict.fromkeys(KEYWORDS, "hip")
    return {"all_hip": lambda: run({**three, "conv3x3z": "hip"}), "three_hip_conv3x3z_torch": lambda: run(three), "all_torch": lambda: run({})}


def bench_step_z(batch, reps, rounds):
    sides = step_model_z(batch)
    res = {"spec": "B", "batch": batch, "patch": 256, "reps": reps, "rounds": rounds, "ms": alternate(sides, reps, rounds, 2, 1e-3),
           "max_memory_allocated_GiB": {k: round(peak_of(fn, 2 ** 30, above_allocated=False), 2) for k, fn in sides.items()}}
    res.update(node_counts("conv3x3z", sides["all_hip"]))
    base = res["ms"]["all_torch"]["median"]
    res["ratio_of_all_torch_over"] = {k: round(base / v["median"], 3) for k, v in res["ms"].items()}
    return res


def count_step_launches(side, batch, iters, workdir):
    d = os.path.join(workdir, f"{side}_{iters}")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "--node", "conv3x3z", "--child", side, "--child-iters", str(iters), "--step-batch",
                    str(batch)], check=True, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rows = 0
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += sum(1 for _ in csv.reader(f)) - 1
    return rows


def main_z(args):
    if args.child:
        fn = step_model_z(args.step_batch)[args.child]
        for _ in range(args.child_iters):
            fn()
        return torch.cuda.synchronize()
    out = {"device": torch.cuda.get_device_name(0), "wgrad_run_rows": ops.conv3x3z_train_wgrad_run(), "ops": None, "step": None,
           "launches_per_step_fwd_bwd": None}
    out["ops"] = bench_ops_z(args.reps, args.rounds)
    if not args.no_step:
        out["step"] = bench_step_z(args.step_batch, args.step_reps, args.step_rounds)
        print(json.dumps({"step": out["step"]}), flush=True)
    if args.launches:
        with tempfile.TemporaryDirectory() as wd:
            out["launches_per_step_fwd_bwd"] = {
                s: (count_step_launches(s, 2, 4, wd) - count_step_launches(s, 2, 2, wd)) / 2 for s in ("all_hip", "all_torch")}
        print(json.dumps({"launches_per_step_fwd_bwd": out["launches_per_step_fwd_bwd"]}), flush=True)
    path = args.out or os.path.join(ROOT, "profiles", "conv3x3z_train.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def bench_ops(node, reps, rounds):
    rec, out = NODES[node], {}
    k, s, halo = rec["k"], rec["stride"], rec["halo"]
    fwd, bwd = getattr(ops, node + "_train_forward"), getattr(ops, node + "_train_backward")
    for (name, B, H, ci, co, pre) in rec["ops"]:
        gen = torch.Generator().manual_seed(ci + co)
        # [B, H, W, C], as the blocks hand it over; the torch route sees its NCHW-shaped view
        x = torch.randn(B, H, H, ci, generator=gen).cuda()
        g = torch.randn(B, H // s, H // s, co, generator=gen).cuda()
        w = (torch.randn(co, ci, k, k, generator=gen) / (k * k * ci) ** 0.5).cuda().contiguous(memory_format=torch.channels_last)
        a, b = (torch.tensor([v]).cuda() for v in (0.03, -0.02))
        a = a if pre == 2 else None
        un, gn = ops.fixup_act(x, a, b, halo).permute(0, 3, 1, 2), g.permute(0, 3, 1, 2)
        m = B * (H // s) ** 2

        def torch_fwd():
            return F.conv2d(ops.fixup_act(x, a, b, halo).permute(0, 3, 1, 2), w, stride=s)

        def torch_bwd():
            g_u, g_w, _ = torch.ops.aten.convolution_backward(gn, un, w, None, [s, s], [0, 0], [1, 1], False, [0, 0], 1,
                                                              [True, True, False])
            g_u = g_u.permute(0, 2, 3, 1).contiguous()
            return (ops.fixup_act_backward(g_u, x, a, halo) if pre == 2 else ops.fixup_act_backward(g_u, None, None, act=False)), g_w

        byts = {"fwd": 4 * (s * s * ci + co) * m, "bwd": 4 * (co + 2 * s * s * ci) * m}
        fns = {"hip_fwd": lambda: fwd(x, w, a, b), "torch_fwd": torch_fwd, "hip_bwd": lambda: bwd(g, x, w, a, b), "torch_bwd": torch_bwd,
               "hip_bwd_data_only": lambda: bwd(g, x, w, a, b, need_w=False), "hip_bwd_weight_only": lambda: bwd(g, x, w, a, b, need_x=False)}
        for d, n in byts.items():
            src, dst = torch.empty(n // 8, device="cuda"), torch.empty(n // 8, device="cuda")
            fns["copy_" + d] = (lambda src=src, dst=dst: dst.copy_(src))
        us = alternate(fns, reps, rounds, 3)
        res = {"batch": B, "H": H, "Ci": ci, "Co": co, "pre": pre, "rows": m, "w_layout": int(k > 1), "us": us, "algorithmic_bytes": byts}
        for d, flop in (("fwd", 2.0 * m * k * k * ci * co), ("bwd", 4.0 * m * k * k * ci * co)):
            hip, tor, cp = (us[f"{side}_{d}"]["median"] for side in ("hip", "torch", "copy"))
            res[d] = {"torch_over_hip": round(tor / hip, 3), "hip_over_copy": round(hip / cp, 3), "torch_over_copy": round(tor / cp, 3),
                      "hip_mfma_peak_fraction": round(flop / (hip * 1e-6) / MFMA_PEAK, 4),
                      "torch_mfma_peak_fraction": round(flop / (tor * 1e-6) / MFMA_PEAK, 4)}
        out[name] = res
        print(json.dumps({name: res}), flush=True)
        del x, g, un, gn, fns
        torch.cuda.empty_cache()
    return out


def block_sides(node, name):
    mode, B, cin, cout, H = NODES[node]["blocks"][name]
    torch.manual_seed(cin)
    blk = PreActFixupResBlock(cin, cout, mode, n_layers=100).cuda()
    with torch.no_grad():
        for k, p in blk.named_parameters():
            if p.numel() == 1:
                p.fill_(0.9 if k == "scale" else 0.03)
        torch.nn.init.normal_(blk.branch_conv3.weight, std=0.5 / cout ** 0.5)
    gen = torch.Generator().manual_seed(1)
    OH = H // 2 if mode == "down" else H
    x = torch.randn(B, cin, H, H, generator=gen).cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    g = torch.randn(B, cout, OH, OH, generator=gen).cuda().contiguous(memory_format=torch.channels_last)

    def run(routes):
        train.block_forward(blk, x, **routes).backward(g)
        x.grad = None
        for p in blk.parameters():
            p.grad = None

    return {"hip": lambda: run({kw: "hip" for kw in NODES[node]["hip"]}), "torch": lambda: run({})}


def bench_block(node, name, reps, rounds):
    sides = block_sides(node, name)
    res = {**NODES[node]["block_key"](*NODES[node]["blocks"][name][1:]), "reps": reps, "rounds": rounds,
           "us": alternate(sides, reps, rounds, 3),
           "max_memory_allocated_MiB": {k: round(peak_of(fn, 2 ** 20), 1) for k, fn in sides.items()}, **node_counts(node, sides["hip"])}
    t, h = res["us"]["torch"], res["us"]["hip"]
    res["ratio_torch_over_hip"] = round(t["median"] / h["median"], 3)
    res["hip_slower_than_torch_by_more_than_torch_spread"] = bool(h["median"] - t["median"] > t["max"] - t["min"])
    return res


def bench_step(node, batch, reps, rounds):
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

    label = lambda routes: ",".join(f"{kw}={routes[kw]}" for kw in KEYWORDS)
    combos = [dict(zip(KEYWORDS, c)) for c in itertools.product(("torch", "hip"), repeat=3)]
    sides = {label(r): (lambda r=r: run(r)) for r in combos}
    res = {"spec": "B", "batch": batch, "patch": 256, "reps": reps, "rounds": rounds, "ms": alternate(sides, reps, rounds, 2, 1e-3),
           "max_memory_allocated_GiB": {k: round(peak_of(fn, 2 ** 30, above_allocated=False), 2) for k, fn in sides.items()}}
    res.update(node_counts(node, sides[label({kw: "hip" if kw == node else "torch" for kw in KEYWORDS})]))
    base = res["ms"][label(dict.fromkeys(KEYWORDS, "torch"))]["median"]
    res["ratio_of_default_over"] = {k: round(base / v["median"], 3) for k, v in res["ms"].items()}
    return res


def check_against_recorded(out):
    """All keywords at "torch" is the code profiles/fixup_train.json timed as "fused": inside that file's min - max spread?"""
    path = os.path.join(ROOT, "profiles", "fixup_train.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        old = json.load(f)
    res = {}
    for name, blk in out["blocks"].items():
        o, now = old["blocks"][name]["us"]["fused"], blk["us"]["torch"]["median"]
        res[name] = {"torch_route_median_us": now, "recorded_us": o, "within_recorded_spread": bool(o["min"] <= now <= o["max"])}
    if out.get("step") and old.get("step") and out["step"]["batch"] == old["step"]["batch"]:
        o, now = old["step"]["ms"]["fused"], out["step"]["ms"][",".join(kw + "=torch" for kw in KEYWORDS)]["median"]
        res["step"] = {"torch_route_median_ms": now, "recorded_ms": o, "within_recorded_spread": bool(o["min"] <= now <= o["max"])}
    return res


def child(node, side, name, iters):
    sides = block_sides(node, name)
    for _ in range(iters):
        sides[side]()
    torch.cuda.synchronize()


def count_launches(node, side, name, iters, workdir):
    d = os.path.join(workdir, f"{side}_{iters}")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "--node", node, "--child", side, "--child-shape", name, "--child-iters", str(iters)],
                   check=True, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rows = 0
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += sum(1 for _ in csv.reader(f)) - 1
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--node", choices=sorted(NODES), required=True)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--step-batch", type=int, default=16)
    ap.add_argument("--step-reps", type=int, default=2)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-blocks", "--no-block", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-shape", default=None)
    ap.add_argument("--child-iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv_train needs a GPU: there is no CPU timing"
    if args.node == "conv3x3z":
        return main_z(args)
    node, blocks = args.node, NODES[args.node]["blocks"]
    first = next(iter(blocks))
    if args.child:
        return child(node, args.child, args.child_shape or first, args.child_iters)
    many = list(blocks) != ["block"]
    out = {"device": torch.cuda.get_device_name(0), "wgrad_run_rows": getattr(ops, node + "_train_wgrad_run")(), "ops": None,
           **({"blocks": {}} if many else {"block": None}), "step": None, "launches_per_block_fwd_bwd": None}
    out["ops"] = bench_ops(node, args.reps, args.rounds)
    if not args.no_blocks:
        for name in blocks:
            res = bench_block(node, name, args.reps, args.rounds)
            if many:
                out["blocks"][name] = res
            else:
                out["block"] = res
            print(json.dumps({name: res}), flush=True)
    if not args.no_step:
        out["step"] = bench_step(node, args.step_batch, args.step_reps, args.step_rounds)
        print(json.dumps({"step": out["step"]}), flush=True)
    if node == "conv1x1":
        out["torch_route_against_fixup_train_json"] = check_against_recorded(out)
        print(json.dumps({"torch_route_against_fixup_train_json": out["torch_route_against_fixup_train_json"]}), flush=True)
    if args.launches:
        with tempfile.TemporaryDirectory() as wd:
            out["launches_per_block_fwd_bwd"] = {
                s: (count_launches(node, s, first, 15, wd) - count_launches(node, s, first, 5, wd)) / 10 for s in ("hip", "torch")}
        print(json.dumps({"launches_per_block_fwd_bwd": out["launches_per_block_fwd_bwd"]}), flush=True)
    path = args.out or os.path.join(ROOT, "profiles", node + "_train.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
