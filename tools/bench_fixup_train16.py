#!/usr/bin/env python3
"""Times the 16-bit-I/O nodes of the Fixup training path (csrc/fixup_train_io.hip, vqae_amd.train under torch.autocast) on one
GPU, under bf16 autocast, at cfg B's levels (batch 16: 16 @ 256 x 256, 32 @ 128 x 128, 64 @ 64 x 64, 128 @ 32 x 32).

    nodes     every node, forward and backward, against its yardstick: the existing fp32 op on up-cast inputs with torch's
              casts around it (ops.fixup_act(x.float(), ...).to(T); ops.fixup_act_backward(g.float(), x.float(), ...) and
              g_x.to(x.dtype); the same for `out`) -- the cast kernels are part of the yardstick, as they are part of a step
              without the 16-bit forms.  A device-to-device copy of the node's own bytes (what it must read and write) runs in
              the same rounds.  The sides alternate inside every round after a warm-up; median, min and max over the rounds.
    blocks    forward + backward of one 'same' block (cfg B's trunk, C = 128, 32 x 32) and one 'down' block (16 -> 32 at
              256 x 256), train.block_forward against train.block_forward_torch, both under the same autocast
    step      a whole train.step + backward of cfg B (256 x 256 patches, --step-batch) against the stock-torch forward of the
              same mirror, both under autocast; nothing is read back inside the timed window

    python tools/bench_fixup_train16.py [--rounds 9 --reps 10 --step-batch 16 --out profiles/fixup_train16.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vqae_amd  # noqa: E402
from vqae_amd import ops, train  # noqa: E402
from vqae_amd.layers.fixup_train import PreActFixupResBlock  # noqa: E402
from bench_fixup_train import stock_forward, summary, timed  # noqa: E402

T = torch.bfloat16
F32 = torch.float32
LEVELS = {"C16_256x256": (16, 16, 256, 256), "C32_128x128": (16, 32, 128, 128), "C64_64x64": (16, 64, 64, 64),
          "C128_32x32": (16, 128, 32, 32)}                                            # (batch, C, H, W)
SIZE = {F32: 4, T: 2}


def node_sides(B, C, H, W):
    """{node: (its own bytes, the 16-bit form, the yardstick composition)}."""
    gen = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=gen).cuda()
    x32, g32, t32, gh32 = r(B, H, W, C), r(B, H, W, C), r(B, H, W, C), r(B, H + 2, W + 2, C)
    x16, g16, t16, gh16, s16 = x32.to(T), g32.to(T), t32.to(T), gh32.to(T), g32.to(T)
    a, b = (torch.tensor([v]).cuda() for v in (0.03, -0.02))
    n, nh = x32.numel(), gh32.numel()
    sides = {}

    def act(name, x, dy, halo):
        g = {(T, 0): g16, (T, 1): gh16, (F32, 0): g32, (F32, 1): gh32}[(dy, halo)]
        ny = nh if halo else n
        sides[name + "_fwd"] = (SIZE[x.dtype] * n + SIZE[dy] * ny, lambda: ops.fixup_act_io(x, a, b, halo, dy),
                                lambda: ops.fixup_act(x.float(), a, b, halo).to(dy))
        sides[name + "_bwd"] = (SIZE[dy] * ny + 2 * SIZE[x.dtype] * n, lambda: ops.fixup_act_backward_io(g, x, a, halo),
                                lambda: ops.fixup_act_backward(g.float(), x.float(), a, halo)[0].to(x.dtype))

    act("act_conv_to_conv", x16, T, 0)                     # between two convs: 2 + 2 bytes per element
    act("act_conv_to_conv3x3_halo", x16, T, 1)
    act("act_stream_to_conv", x32, T, 0)                   # the first act of a block: reads the fp32 residual stream
    act("act_conv_to_fp32", x16, F32, 0)                   # in front of bicubic_up2
    sides["add_stream_to_conv_fwd"] = (6 * n, lambda: ops.fixup_act_io(x32, None, b, 0, T),
                                       lambda: ops.fixup_act(x32, None, b).to(T))
    sides["add_stream_to_conv_bwd"] = (6 * n, lambda: ops.fixup_act_backward_io(g16, None, None, act=False, x_dtype=F32),
                                       lambda: ops.fixup_act_backward(g16.float(), None, None, act=False))
    for name, skip in (("out_skip_fp32", x32), ("out_skip_conv", s16)):
        sd = skip.dtype
        sides[name + "_fwd"] = ((2 + SIZE[sd] + 4) * n, lambda skip=skip: ops.fixup_out_io(t16, skip, a, b, b),
                                lambda skip=skip: ops.fixup_out(t16.float(), skip.float(), a, b, b))
        sides[name + "_bwd"] = ((4 + 2 + 2 + (2 if sd == T else 0)) * n,
                                lambda sd=sd: ops.fixup_out_backward_io(g32, t16, a, sd),
                                lambda sd=sd: (ops.fixup_out_backward(g32, t16.float(), a)[0].to(T), g32.to(sd)))
    return sides


def bench_nodes(reps, rounds):
    out = {}
    for level, shape in LEVELS.items():
        sides = node_sides(*shape)
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
        res = {}
        for k, (byts, _, _) in sides.items():
            med = {s: statistics.median(v) for s, v in samples[k].items()}
            res[k] = {"own_bytes": byts, "us": {s: summary(v) for s, v in samples[k].items()},
                      "TBps_own_bytes": round(byts / med["io16"] * 1e-6, 3),
                      "ratio_yardstick_over_io16": round(med["yardstick"] / med["io16"], 3),
                      "ratio_io16_over_copy": round(med["io16"] / med["copy"], 3)}
        out[level] = res
    return out


def make_block(cin, cout, mode):
    torch.manual_seed(cin)
    blk = PreActFixupResBlock(cin, cout, mode, n_layers=100).cuda()
    with torch.no_grad():
        for k, p in blk.named_parameters():
            if p.numel() == 1:
                p.fill_(0.9 if k == "scale" else 0.03)
        torch.nn.init.normal_(blk.branch_conv3.weight, std=0.5 / cout ** 0.5)
    return blk


def bench_blocks(reps, rounds):
    out = {}
    for name, (mode, cin, cout, B, H, W) in {"same_C128_32x32": ("same", 128, 128, 16, 32, 32),
                                             "down_C16_C32_256x256": ("down", 16, 32, 16, 256, 256)}.items():
        blk = make_block(cin, cout, mode)
        gen = torch.Generator().manual_seed(1)
        x = torch.randn(B, cin, H, W, generator=gen).cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
        s = 2 if mode == "down" else 1
        g = torch.randn(B, cout, H // s, W // s, generator=gen).cuda().contiguous(memory_format=torch.channels_last)

        def run(forward):
            with torch.autocast("cuda", dtype=T):
                y = forward(blk, x)
            y.backward(g)
            x.grad = None
            for p in blk.parameters():
                p.grad = None

        sides = {"fused": lambda: run(train.block_forward), "stock": lambda: run(train.block_forward_torch)}
        for fn in sides.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in sides}
        for _ in range(rounds):
            for k, fn in sides.items():
                samples[k].append(timed(fn, reps))
        res = {"mode": mode, "shape_BCHW": [B, cin, H, W], "reps": reps, "rounds": rounds,
               "us": {k: summary(v) for k, v in samples.items()}, "max_memory_allocated_MiB": {}}
        for k, fn in sides.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            res["max_memory_allocated_MiB"][k] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        res["ratio_stock_over_fused"] = round(res["us"]["stock"]["median"] / res["us"]["fused"]["median"], 3)
        out[name] = res
    return out


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
        with torch.autocast("cuda", dtype=T):
            out, (vq_loss,) = forward(model, xi)
            loss = F.huber_loss(input=out, target=xi) + vq_loss
        loss.backward()
        for q in model.parameters():
            q.grad = None

    sides = {"fused": lambda: run(train.forward_train, xcl), "stock": lambda: run(stock_forward, x)}
    train.stats.update(io16_hip=0, io16_fallbacks=0)
    sides["fused"]()
    counts = {"io16_hip": train.stats["io16_hip"], "io16_fallbacks": train.stats["io16_fallbacks"]}
    for fn in sides.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            samples[k].append(timed(fn, reps) / 1e3)             # ms
    res = {"spec": "B", "batch": batch, "patch": 256, "autocast": "bf16", "reps": reps, "rounds": rounds,
           "ms": {k: summary(v) for k, v in samples.items()}, "nodes_per_step": counts, "max_memory_allocated_GiB": {}}
    for k, fn in sides.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        res["max_memory_allocated_GiB"][k] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    res["ratio_stock_over_fused"] = round(res["ms"]["stock"]["median"] / res["ms"]["fused"]["median"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--step-batch", type=int, default=16)
    ap.add_argument("--step-reps", type=int, default=2)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixup_train16.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fixup_train16 needs a GPU: there is no CPU timing"
    out = {"device": torch.cuda.get_device_name(0), "autocast": "bf16", "nodes": None, "blocks": None, "step": None}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    out["nodes"] = bench_nodes(args.reps, args.rounds)
    print(json.dumps({"nodes": out["nodes"]}), flush=True)
    save()
    out["blocks"] = bench_blocks(args.reps, args.rounds)
    print(json.dumps({"blocks": out["blocks"]}), flush=True)
    save()
    if not args.no_step:
        out["step"] = bench_step(args.step_batch, args.step_reps, args.step_rounds)
        print(json.dumps({"step": out["step"]}), flush=True)
        save()


if __name__ == "__main__":
    main()
