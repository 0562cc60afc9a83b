#!/usr/bin/env python3
"""Times the training path of the MBConv mirrors (vqae_amd.train_mbconv, csrc/mbconv_train.hip) on one GPU against the same
block written with stock torch modules' ops (train_mbconv.block_forward_torch: F.batch_norm, F.silu, F.conv2d(groups=), the SE
multiply, autograd's backward); both sides use the same dense F.conv2d / F.conv_transpose2d, in the same process.

    blocks    forward + backward of one block through train_mbconv.block_forward at the three channel levels of spec `BM` on
              128 x 128 patches, batch 16 -- 16 ch at 128^2, 32 at 64^2, 64 at 32^2 -- in the modes same (C -> C), down
              (C -> 2C) and up (2C -> C, input at half the extent): the sides alternate inside every round after a warm-up;
              median, min and max over the rounds, torch.cuda.max_memory_allocated of one forward + backward of each side
    kernels   every new node alone (e = 128 channels, 64 x 64, batch 16) against a device-to-device copy of the bytes it must
              move per element: bn_act forward 12 (x twice, y), backward 20 (g and x twice, g_x), dwconv forward 8, backward 16
              (g_x: g and g_x; g_w: g and x), se_scale forward 8, backward 12
    step      a whole train_mbconv.step + backward of `BM` (128 x 128 patches) at --step-batch against the stock-torch forward
              of the same mirror; nothing is read back inside the timed window
    launches  (--launches) kernel launches per block forward + backward of each side, from rocprofv3 --kernel-trace runs of
              this script's --child mode: two runs per side that differ by 10 iterations, so warm-up launches cancel

Every ratio is against the stock side, or the copy, measured in this same run.

    python tools/bench_mbconv_train.py [--rounds 9 --reps 10 --step-batch 8 --launches --out profiles/mbconv_train.json]
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
from vqae_amd import _lib as L  # noqa: E402
from vqae_amd import ops, train_mbconv  # noqa: E402
from vqae_amd.layers.mbconv_train import MBConv  # noqa: E402
from vqae_amd.model import default_confs  # noqa: E402

BATCH = 16
LEVELS = ((16, 128), (32, 64), (64, 32))                   # (channels, extent) of spec BM on 128 x 128 patches
BLOCK_SHAPES = {}                                          # name: (mode, cin, cout, H = W of the input)
for _c, _s in LEVELS:
    BLOCK_SHAPES[f"same_C{_c}_{_s}x{_s}"] = ("same", _c, _c, _s)
    BLOCK_SHAPES[f"down_C{_c}_{_s}x{_s}"] = ("down", _c, 2 * _c, _s)
    BLOCK_SHAPES[f"up_C{2 * _c}_{_s // 2}x{_s // 2}"] = ("up", 2 * _c, _c, _s // 2)


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


def make_block(mode, cin, cout):
    conf = default_confs(vqae_amd.SPECS["BM"])["encoder_conf"]["conv_block_conf"]
    torch.manual_seed(cin + cout)
    blk = MBConv(cin, cout, mode, **{k: v for k, v in conf.items() if not k.startswith("_")}).cuda().train()
    with torch.no_grad():
        blk.branch[8].weight.fill_(0.5)                    # the zero init would make every gradient behind it zero
    return blk


def block_sides(name):
    mode, cin, cout, S = BLOCK_SHAPES[name]
    blk = make_block(mode, cin, cout)
    So = {"same": S, "down": S // 2, "up": 2 * S}[mode]
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(BATCH, cin, S, S, generator=gen).cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    g = torch.randn(BATCH, cout, So, So, generator=gen).cuda().contiguous(memory_format=torch.channels_last)
    xs, gs = x.detach().contiguous().requires_grad_(), g.contiguous()          # the stock side in torch's default layout

    def run(forward, xi, gi):
        forward(blk, xi).backward(gi)
        xi.grad = None
        for p in blk.parameters():
            p.grad = None

    return blk, {"fused": lambda: run(train_mbconv.block_forward, x, g),
                 "stock": lambda: run(train_mbconv.block_forward_torch, xs, gs),
                 "stock_channels_last": lambda: run(train_mbconv.block_forward_torch, x, g)}


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
    res = {"mode_cin_cout_extent": list(BLOCK_SHAPES[name]), "batch": BATCH, "reps": reps, "rounds": rounds,
           "us": {k: summary(v) for k, v in samples.items()}, "max_memory_allocated_MiB": {}}
    for k, fn in sides.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        res["max_memory_allocated_MiB"][k] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    best_stock = min(res["us"]["stock"]["median"], res["us"]["stock_channels_last"]["median"])
    res["ratio_stock_over_fused"] = round(res["us"]["stock"]["median"] / res["us"]["fused"]["median"], 3)
    res["ratio_best_stock_over_fused"] = round(best_stock / res["us"]["fused"]["median"], 3)
    return res


def bench_kernels(reps, rounds, B=BATCH, S=64, e=128):
    gen = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=gen).cuda()
    x, g = r(B, S, S, e), r(B, S, S, e)
    xq, gu = r(B, S // 2, S // 2, e), r(B, S // 2, S // 2, e)
    gamma, beta, rm, rv = 0.5 + torch.rand(e).cuda(), r(e), r(e), 0.5 + torch.rand(e).cuda()
    gate, g_pool = torch.rand(B, e).cuda(), r(B, e)
    w3, w2 = r(e, 1, 3, 3), r(e, 1, 2, 2)
    _, mean, invstd, _ = ops.bn_act_train_forward(x, gamma, beta, None, None, True, 0.1, 1e-5, True, True)
    n = x.numel()
    fns = {"bn_act_fwd": (12 * n, lambda: ops.bn_act_train_forward(x, gamma, beta, rm, rv, True, 0.1, 1e-5, True, False)),
           "bn_act_fwd_pool": (12 * n, lambda: ops.bn_act_train_forward(x, gamma, beta, rm, rv, True, 0.1, 1e-5, True, True)),
           "bn_act_fwd_eval": (8 * n, lambda: ops.bn_act_train_forward(x, gamma, beta, rm, rv, False, 0.1, 1e-5, True, False)),
           "bn_act_bwd": (20 * n, lambda: ops.bn_act_train_backward(g, x, mean, invstd, gamma, beta, True, True)),
           "bn_act_bwd_pool": (20 * n, lambda: ops.bn_act_train_backward(g, x, mean, invstd, gamma, beta, True, True, g_pool)),
           "dwconv_same_fwd": (8 * n, lambda: ops.dwconv_train_forward(x, w3, L.DW_SAME)),
           "dwconv_same_bwd": (16 * n, lambda: ops.dwconv_train_backward(g, x, w3, L.DW_SAME)),
           "dwconv_down_fwd": (5 * n, lambda: ops.dwconv_train_forward(x, w2, L.DW_DOWN)),
           "dwconv_down_bwd": (10 * n, lambda: ops.dwconv_train_backward(gu, x, w2, L.DW_DOWN)),
           "dwconv_up_fwd": (5 * n, lambda: ops.dwconv_train_forward(xq, w2, L.DW_UP)),
           "dwconv_up_bwd": (10 * n, lambda: ops.dwconv_train_backward(g, xq, w2, L.DW_UP)),
           "se_scale_fwd": (8 * n, lambda: ops.se_scale_forward(x, gate)),
           "se_scale_bwd": (12 * n, lambda: ops.se_scale_backward(g, x, gate))}
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
    res = {"shape_BHWC": [B, S, S, e]}
    for k, (byts, _) in fns.items():
        med, cp = statistics.median(samples[k]), statistics.median(samples[f"copy_{byts}"])
        res[k] = {"algorithmic_bytes": byts, "us": summary(samples[k]), "copy_us": summary(samples[f"copy_{byts}"]),
                  "TBps_algorithmic": round(byts / med * 1e-6, 3), "ratio_over_copy": round(med / cp, 3)}
    return res


def stock_forward(model, x):
    """VQAE.forward of the mirror with stock torch ops on NCHW tensors: block_forward_torch blocks, the same quantiser."""
    enc, dec, bft = model.encoder, model.decoder, train_mbconv.block_forward_torch
    pre, post = train_mbconv._blocks(model)
    h = F.conv2d(x, enc.in_stem.weight, enc.in_stem.bias, padding=1)
    for blk in pre:
        h = bft(blk, h)
    h, _, vq_loss = enc.vq_layers[0](h)
    for blk in post:
        h = bft(blk, h)
    return F.conv2d(h, dec.out_stem.weight, dec.out_stem.bias, padding=1), (vq_loss,)


def bench_step(batch, reps, rounds, patch=128):
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

    def run(forward, xi):
        out, (vq_loss,) = forward(model, xi)
        (F.huber_loss(input=out, target=xi) + vq_loss).backward()
        for q in model.parameters():
            q.grad = None

    sides = {"fused": lambda: run(train_mbconv.forward_train, xcl), "stock": lambda: run(stock_forward, x)}
    for fn in sides.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            samples[k].append(timed(fn, reps) / 1e3)             # ms
    res = {"spec": "BM", "batch": batch, "patch": patch, "reps": reps, "rounds": rounds,
           "ms": {k: summary(v) for k, v in samples.items()}, "max_memory_allocated_GiB": {}}
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
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--step-reps", type=int, default=2)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-shape", default="same_C32_64x64")
    ap.add_argument("--child-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mbconv_train.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mbconv_train needs a GPU: there is no CPU timing"
    if args.child:
        return child(args.child, args.child_shape, args.child_iters)
    out = {"device": torch.cuda.get_device_name(0), "blocks": {}, "kernels": None, "step": None, "launches_per_block_fwd_bwd": None}
    for name in BLOCK_SHAPES:
        out["blocks"][name] = bench_block(name, args.reps, args.rounds)
        print(json.dumps({name: out["blocks"][name]}), flush=True)
    out["kernels"] = bench_kernels(args.reps, args.rounds)
    print(json.dumps({"kernels": out["kernels"]}), flush=True)
    if not args.no_step:
        out["step"] = bench_step(args.step_batch, args.step_reps, args.step_rounds)
        print(json.dumps({"step": out["step"]}), flush=True)
    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    write()                                                # the timings are kept even where the profiler runs below fail
    if args.launches:
        with tempfile.TemporaryDirectory() as wd:
            out["launches_per_block_fwd_bwd"] = {
                side: (count_launches(side, args.child_shape, 12, wd) - count_launches(side, args.child_shape, 2, wd)) / 10
                for side in ("fused", "stock")}
        print(json.dumps({"launches_per_block_fwd_bwd": out["launches_per_block_fwd_bwd"]}), flush=True)
        write()


if __name__ == "__main__":
    main()
