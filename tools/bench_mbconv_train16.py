#!/usr/bin/env python3
"""Times the 16-bit-I/O nodes of the MBConv training path (csrc/mbconv_train_io.hip, vqae_amd.train_mbconv under
torch.autocast) on one GPU, under bf16 autocast, batch 16, at the levels of spec `BM` on 128 x 128 patches that
tools/bench_mbconv_train.py uses (16 ch at 128^2, 32 at 64^2, 64 at 32^2; the nodes see the expanded channels).

    nodes     every node, forward and backward, against its yardstick composition: the existing fp32 op on up-cast inputs
              with torch's casts around it (ops.bn_act_train_forward(x.float(), ...)[0].to(T); the backward on g.float(),
              x.float() and g_x.to(T); the depthwise taps as w.to(T).float()) -- the cast kernels are part of the yardstick, as
              they are part of a step without the 16-bit forms.  A device-to-device copy of the node's own bytes (what it must
              read and write) runs in the same rounds.  The sides alternate inside every round after a warm-up; median, min
              and max over the rounds.
    blocks    forward + backward of one block per level and mode, train_mbconv.block_forward against
              train_mbconv.block_forward_torch under the same autocast, with torch.cuda.max_memory_allocated; and, with
              --parent-tree DIR (a checkout of the parent commit with its library built), against THAT tree's
              train_mbconv.block_forward under the same autocast, loaded into this process beside the current package
    step      a whole train_mbconv.step + backward of `BM` (128 x 128 patches, --step-batch): the same three sides
    launches  (--launches) kernel launches per block forward + backward of each side, from rocprofv3 --kernel-trace runs of
              this script's --child mode: two runs per side that differ by 10 iterations, so warm-up launches cancel

    python tools/bench_mbconv_train16.py [--rounds 5 --reps 10 --step-batch 8 --parent-tree DIR --launches
                                          --out profiles/mbconv_train16.json]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vqae_amd  # noqa: E402
from vqae_amd import _lib as L  # noqa: E402
from vqae_amd import ops, train_mbconv  # noqa: E402
from bench_mbconv_train import BATCH, BLOCK_SHAPES, LEVELS, make_block, stock_forward, summary, timed  # noqa: E402

T = torch.bfloat16
JUDGED = ("C16_128x128", "C32_64x64")            # the two largest levels: a node slower than its yardstick there is reported


def load_parent(tree):
    """The package of another checkout as `vqae_amd_parent`, its own libvqae_hip.so beside it -> the package.  Its blocks and
    models are built from ITS classes (its train_mbconv checks a block's class), with the current side's state dict."""
    d = os.path.join(os.path.abspath(tree), "2d-vq-ae-2_amd")
    assert os.path.exists(os.path.join(d, "libvqae_hip.so")), f"{d}: build the parent's library first (build.sh)"
    spec = importlib.util.spec_from_file_location("vqae_amd_parent", os.path.join(d, "__init__.py"),
                                                  submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["vqae_amd_parent"] = mod
    spec.loader.exec_module(mod)
    for sub in ("train_mbconv", "layers.mbconv_train", "model"):
        importlib.import_module("vqae_amd_parent." + sub)
    return mod


def node_sides(C, S, B=BATCH):
    """{node: (its own bytes, the 16-bit form, the yardstick composition)} on e = the expanded channels of a C-channel block."""
    e = make_block("same", C, C).expanded
    gen = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=gen).cuda()
    x32, g32 = r(B, S, S, e), r(B, S, S, e)
    xq32 = r(B, S // 2, S // 2, e)
    x, g, xq = x32.to(T), g32.to(T), xq32.to(T)
    gamma, beta, rm, rv = 0.5 + torch.rand(e).cuda(), r(e), r(e), 0.5 + torch.rand(e).cuda()
    gate, g_pool = torch.rand(B, e).cuda().to(T), r(B, e)
    w3, w2 = r(e, 1, 3, 3), r(e, 1, 2, 2)
    _, mean, invstd, _ = ops.bn_act_train_forward(x32, gamma, beta, None, None, True, 0.1, 1e-5, True, True)
    n = x.numel()
    fw, bw = ops.bn_act_train_forward, ops.bn_act_train_backward
    fwi, bwi = ops.bn_act_train_forward_io, ops.bn_act_train_backward_io
    dwf, dwb, dwfi, dwbi = ops.dwconv_train_forward, ops.dwconv_train_backward, ops.dwconv_train_forward_io, ops.dwconv_train_backward_io

    def bwd_y(gp):
        return lambda: bw(g.float(), x.float(), mean, invstd, gamma, beta, True, True, gp)[0].to(T)

    def dw_y(gg, xx, w, mode):
        def run():
            g_x, g_w = dwb(gg.float(), xx.float(), w.to(T).float(), mode)
            return g_x.to(T), g_w
        return run

    def se_bwd_y():
        g_x, g_gate = ops.se_scale_backward(g.float(), x.float(), gate.float())
        return g_x.to(T), g_gate.to(T)

    return e, {
        # bytes per element: x twice (statistics, apply) + y
        "bn_act_fwd": (6 * n, lambda: fwi(x, gamma, beta, rm, rv, True, 0.1, 1e-5, True, False),
                       lambda: fw(x.float(), gamma, beta, rm, rv, True, 0.1, 1e-5, True, False)[0].to(T)),
        "bn_act_fwd_pool": (6 * n, lambda: fwi(x, gamma, beta, rm, rv, True, 0.1, 1e-5, True, True),
                            lambda: fw(x.float(), gamma, beta, rm, rv, True, 0.1, 1e-5, True, True)[0].to(T)),
        "bn_act_fwd_eval": (4 * n, lambda: fwi(x, gamma, beta, rm, rv, False, 0.1, 1e-5, True, False),
                            lambda: fw(x.float(), gamma, beta, rm, rv, False, 0.1, 1e-5, True, False)[0].to(T)),
        # g and x twice (sums, apply) + g_x
        "bn_act_bwd": (10 * n, lambda: bwi(g, x, mean, invstd, gamma, beta, True, True), bwd_y(None)),
        "bn_act_bwd_pool": (10 * n, lambda: bwi(g, x, mean, invstd, gamma, beta, True, True, g_pool), bwd_y(g_pool)),
        "dwconv_same_fwd": (4 * n, lambda: dwfi(x, w3, L.DW_SAME), lambda: dwf(x.float(), w3.to(T).float(), L.DW_SAME).to(T)),
        "dwconv_same_bwd": (8 * n, lambda: dwbi(g, x, w3, L.DW_SAME), dw_y(g, x, w3, L.DW_SAME)),
        "dwconv_down_fwd": (5 * n // 2, lambda: dwfi(x, w2, L.DW_DOWN), lambda: dwf(x.float(), w2.to(T).float(), L.DW_DOWN).to(T)),
        "dwconv_down_bwd": (5 * n, lambda: dwbi(xq, x, w2, L.DW_DOWN), dw_y(xq, x, w2, L.DW_DOWN)),
        "dwconv_up_fwd": (5 * n // 2, lambda: dwfi(xq, w2, L.DW_UP), lambda: dwf(xq.float(), w2.to(T).float(), L.DW_UP).to(T)),
        "dwconv_up_bwd": (5 * n, lambda: dwbi(g, xq, w2, L.DW_UP), dw_y(g, xq, w2, L.DW_UP)),
        "se_scale_fwd": (4 * n, lambda: ops.se_scale_forward_io(x, gate),
                         lambda: ops.se_scale_forward(x.float(), gate.float()).to(T)),
        "se_scale_bwd": (6 * n, lambda: ops.se_scale_backward_io(g, x, gate), se_bwd_y)}


def bench_nodes(reps, rounds):
    out = {}
    for C, S in LEVELS:
        e, sides = node_sides(C, S)
        copies = {}
        for byts in sorted({v[0] for v in sides.values()}):
            src, dst = (torch.empty(byts // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
            copies[byts] = (lambda s=src, d=dst: d.copy_(s))
        for _, fused, yard in sides.values():
            for _ in range(3):
                fused(), yard()
        for fn in copies.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        samples = {k: {"io16": [], "yardstick": [], "copy": []} for k in sides}
        for _ in range(rounds):
            for k, (byts, fused, yard) in sides.items():
                samples[k]["io16"].append(timed(fused, reps))
                samples[k]["yardstick"].append(timed(yard, reps))
                samples[k]["copy"].append(timed(copies[byts], reps))
        level = f"C{C}_{S}x{S}"
        res = {"shape_BHWC": [BATCH, S, S, e]}
        for k, (byts, _, _) in sides.items():
            med = {s: statistics.median(v) for s, v in samples[k].items()}
            res[k] = {"own_bytes": byts, "us": {s: summary(v) for s, v in samples[k].items()},
                      "TBps_own_bytes": round(byts / med["io16"] * 1e-6, 3),
                      "ratio_yardstick_over_io16": round(med["yardstick"] / med["io16"], 3),
                      "ratio_io16_over_copy": round(med["io16"] / med["copy"], 3)}
        res["slower_than_yardstick"] = [k for k in sides if res[k]["ratio_yardstick_over_io16"] < 1.0]
        res["judged"] = level in JUDGED
        out[level] = res
    return out


def block_sides(name, parent):
    mode, cin, cout, S = BLOCK_SHAPES[name]
    blk = make_block(mode, cin, cout)
    So = {"same": S, "down": S // 2, "up": 2 * S}[mode]
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(BATCH, cin, S, S, generator=gen).cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    g = torch.randn(BATCH, cout, So, So, generator=gen).cuda().contiguous(memory_format=torch.channels_last)

    def run(forward):
        with torch.autocast("cuda", dtype=T):
            y = forward(blk, x)
        y.backward(g.to(y.dtype))
        x.grad = None
        for p in blk.parameters():
            p.grad = None

    sides = {"fused": lambda: run(train_mbconv.block_forward), "stock": lambda: run(train_mbconv.block_forward_torch)}
    if parent is not None:
        conf = parent.model.default_confs(parent.SPECS["BM"])["encoder_conf"]["conv_block_conf"]
        twin = parent.layers.mbconv_train.MBConv(cin, cout, mode, **{k: v for k, v in conf.items() if not k.startswith("_")})
        twin.load_state_dict(blk.state_dict())
        twin = twin.cuda().train()

        def run_parent():
            with torch.autocast("cuda", dtype=T):
                y = parent.train_mbconv.block_forward(twin, x)
            y.backward(g.to(y.dtype))
            x.grad = None
            for p in twin.parameters():
                p.grad = None

        sides["parent"] = run_parent
    return sides


def bench_block(name, parent, reps, rounds):
    sides = block_sides(name, parent)
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            samples[k].append(timed(fn, reps))
    res = {"mode_cin_cout_extent": list(BLOCK_SHAPES[name]), "batch": BATCH, "reps": reps, "rounds": rounds,
           "us": {k: summary(v) for k, v in samples.items()}, "max_memory_allocated_MiB": {}}
    for k, fn in sides.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        res["max_memory_allocated_MiB"][k] = round((torch.cuda.max_memory_allocated() - start) / 2 ** 20, 1)
    for k in sides:
        if k != "fused":
            res[f"ratio_{k}_over_fused"] = round(res["us"][k]["median"] / res["us"]["fused"]["median"], 3)
    return res


def bench_step(batch, parent, reps, rounds, patch=128):
    from oracle import vqae_oracle as O
    from vqae_amd.model import VQAE
    spec = O.SPECS["BM"]
    model = VQAE.from_spec(vqae_amd.SPECS["BM"])
    p = O.make_params(spec, 0)
    vq = "encoder.vq_layers.0."
    p.update({vq + "embed_avg": p[vq + "embed"].clone(), vq + "cluster_size": torch.ones(spec.num_embeddings),
              vq + "first_pass": torch.as_tensor(0)})
    p.update({k: torch.as_tensor(1) for k in model.state_dict() if k.endswith("num_batches_tracked")})
    model.load_state_dict(p)
    model = model.cuda().train()
    x = O.make_patches(batch, patch, 0).cuda()
    xcl = x.contiguous(memory_format=torch.channels_last)

    def run(forward, xi, m=model):
        with torch.autocast("cuda", dtype=T):
            out, (vq_loss,) = forward(m, xi)
            loss = F.huber_loss(input=out, target=xi) + vq_loss
        loss.backward()
        for q in m.parameters():
            q.grad = None

    sides = {"fused": lambda: run(train_mbconv.forward_train, xcl), "stock": lambda: run(stock_forward, x)}
    if parent is not None:
        twin = parent.model.VQAE.from_spec(parent.SPECS["BM"])
        twin.load_state_dict(model.state_dict())
        twin = twin.cuda().train()
        sides["parent"] = lambda: run(parent.train_mbconv.forward_train, xcl, twin)
    train_mbconv.io16_stats.update(io16_hip=0, io16_fallbacks=0)
    sides["fused"]()
    counts = dict(train_mbconv.io16_stats)
    for fn in sides.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            samples[k].append(timed(fn, reps) / 1e3)             # ms
    res = {"spec": "BM", "batch": batch, "patch": patch, "autocast": "bf16", "reps": reps, "rounds": rounds,
           "ms": {k: summary(v) for k, v in samples.items()}, "nodes_per_step": counts, "max_memory_allocated_GiB": {}}
    for k, fn in sides.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        res["max_memory_allocated_GiB"][k] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    for k in sides:
        if k != "fused":
            res[f"ratio_{k}_over_fused"] = round(res["ms"][k]["median"] / res["ms"]["fused"]["median"], 3)
    return res


def child(side, name, iters, parent_tree):
    parent = load_parent(parent_tree) if side == "parent" else None
    sides = block_sides(name, parent)
    for _ in range(iters):
        sides[side]()
    torch.cuda.synchronize()


def count_launches(side, name, iters, workdir, parent_tree):
    import csv
    import glob
    import subprocess
    d = os.path.join(workdir, f"{side}_{name}_{iters}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
           os.path.abspath(__file__), "--child", side, "--child-shape", name, "--child-iters", str(iters)]
    if parent_tree:
        cmd += ["--parent-tree", parent_tree]
    subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rows = 0
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += sum(1 for _ in csv.reader(f)) - 1
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--step-reps", type=int, default=2)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--launch-shape", default="same_C32_64x64")
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-shape", default="same_C32_64x64")
    ap.add_argument("--child-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mbconv_train16.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mbconv_train16 needs a GPU: there is no CPU timing"
    if args.child:
        return child(args.child, args.child_shape, args.child_iters, args.parent_tree)
    parent = load_parent(args.parent_tree) if args.parent_tree else None
    out = {"device": torch.cuda.get_device_name(0), "autocast": "bf16", "parent_measured": parent is not None, "nodes": None,
           "blocks": {}, "step": None, "launches_per_block_fwd_bwd": None}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    out["nodes"] = bench_nodes(args.reps, args.rounds)
    print(json.dumps({"nodes": out["nodes"]}), flush=True)
    save()
    for name in BLOCK_SHAPES:
        out["blocks"][name] = bench_block(name, parent, args.reps, args.rounds)
        print(json.dumps({name: out["blocks"][name]}), flush=True)
    save()
    if not args.no_step:
        out["step"] = bench_step(args.step_batch, parent, args.step_reps, args.step_rounds)
        print(json.dumps({"step": out["step"]}), flush=True)
        save()
    if args.launches:
        sides = ["fused", "stock"] + (["parent"] if parent is not None else [])
        with tempfile.TemporaryDirectory() as wd:
            out["launches_per_block_fwd_bwd"] = {"shape": args.launch_shape, "autocast": "bf16", **{
                side: (count_launches(side, args.launch_shape, 15, wd, args.parent_tree)
                       - count_launches(side, args.launch_shape, 5, wd, args.parent_tree)) / 10 for side in sides}}
        print(json.dumps({"launches": out["launches_per_block_fwd_bwd"]}), flush=True)
        save()


if __name__ == "__main__":
    main()
