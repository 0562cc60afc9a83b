#!/usr/bin/env python3
"""Cost of the exact (label x code) histogram on resident uint8 code grids with their masks, one GPU:

    (a) kernel   vqae_code_histogram adding into a resident int64 table (ops.code_histogram with out= / bad=)
    (b) call     ops.code_histogram as a user calls it: table allocated, zeroed, counted
    (c) stock    torch.bincount(mask.long() * K + codes.long(), minlength=3 * K) on the same device
    (d) copy     a device-to-device copy of as many bytes as (a) reads (2 per code): the HBM floor of one pass

at 1024 x 1024, 4096 x 4096 and 6144 x 12288 codes, K = 256 and 1024, on three inputs each:
    uniform    codes uniform over K, labels uniform over 3
    marginal   codes i.i.d. from the reference's train marginal of that K (one code holds 45-48 %), labels i.i.d. from its
               train label counts (tests/golden/code_marginals.npz)
    runs       the same two marginals in runs of geometric length (mean 48 codes), the spatial structure of a slide
HIP events around `steps` calls after a warm-up, the variants alternating round by round, the median round reported with
the fastest and slowest; (a) and (c) are compared for equality before anything is timed.  The bar: at the largest size
(a) < (c) on all three inputs.  Not a bar, but recorded: (a) over (d), and runs over uniform.

The last record is the wall time of code_stats.histogram_hdf5 on a synthetic archive of a few large slides, device path
against the numpy host path (hist_fn), with the time the device path spends outside the kernel (read, upload).

    python tools/bench_code_stats.py [--sizes 1024x1024,4096x4096,6144x12288 --steps 20 --rounds 5 --out profiles/code_stats.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vqae_amd  # noqa: E402
from vqae_amd import code_stats, hdf5, ops  # noqa: E402

MEAN_RUN = 48


def timed(fn, steps):
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps            # ms per call


def draw(rng, p, n, runs):
    if not runs:
        return rng.choice(len(p), size=n, p=p).astype(np.uint8 if len(p) <= 256 else np.uint16)
    lengths = rng.geometric(1.0 / MEAN_RUN, size=n // 8)
    while lengths.sum() < n:
        lengths = np.concatenate([lengths, rng.geometric(1.0 / MEAN_RUN, size=n // 8)])
    return np.repeat(rng.choice(len(p), size=lengths.size, p=p), lengths)[:n]


def make_input(kind, K, n, z, seed):
    rng = np.random.RandomState(seed)
    if kind == "uniform":
        return rng.randint(0, K, n), rng.randint(0, 3, n)
    pc = z[f"embedding_idx_histogram_{K}_train"].astype(np.float64)
    pl = z["histogram_train"].astype(np.float64)
    return draw(rng, pc / pc.sum(), n, kind == "runs"), draw(rng, pl / pl.sum(), n, kind == "runs")


def run_case(kind, K, h, w, z, steps, stock_steps, rounds, warmup, np_dtype=np.uint8):
    n = h * w
    c, m = make_input(kind, min(K, np.iinfo(np_dtype).max + 1) if kind == "uniform" else K, n, z, seed=K + h)
    # resident grids as stored: uint8 codes where they fit (the K = 1024 marginal needs uint16; a uint8 grid counted into a
    # K = 1024 table holds codes 0 .. 255 only)
    codes = torch.from_numpy(c.astype(np_dtype)).cuda().view(1, n)
    mask = torch.from_numpy(m.astype(np.uint8)).cuda().view(1, n)
    in_bytes = codes.numel() * codes.element_size() + mask.numel()
    src = torch.empty(in_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    out = torch.zeros((1, 3, K), dtype=torch.int64, device="cuda")
    bad = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    codes_i = codes.to(torch.int32) if codes.dtype != torch.uint8 else codes      # torch has no uint16 -> int64 cast on every build

    def stock():
        return torch.bincount((mask.long() * K + codes_i.long()).view(-1), minlength=3 * K)

    fns = {"kernel": (lambda: ops.code_histogram(codes, mask, num_embeddings=K, out=out, bad=bad), steps),
           "call": (lambda: ops.code_histogram(codes, mask, num_embeddings=K), steps),
           "stock": (stock, stock_steps),
           "copy": (lambda: dst.copy_(src), steps)}
    hist, bd = ops.code_histogram(codes, mask, num_embeddings=K)
    equal = bool(torch.equal(hist.view(-1), stock())) and not bool(bd.any())
    for _ in range(warmup):
        for fn, _ in fns.values():
            fn()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (fn, s) in fns.items():
            ms[k].append(timed(fn, s))
    rec = {"input": kind, "K": K, "h": h, "w": w, "codes": n, "code_dtype": str(codes.dtype).replace("torch.", ""),
           "input_bytes": in_bytes, "equal_to_stock": equal, "top_code_share": round(float(hist.sum(1).max()) / n, 4)}
    for k, v in ms.items():
        rec[k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    a = rec["kernel"]["ms_median"]
    rec["kernel"]["GB_per_s"] = round(in_bytes / a / 1e6, 1)
    rec["copy"]["GB_per_s_read"] = round(in_bytes / rec["copy"]["ms_median"] / 1e6, 1)
    rec["stock_over_kernel"] = round(rec["stock"]["ms_median"] / a, 2)
    rec["kernel_over_copy"] = round(a / rec["copy"]["ms_median"], 2)
    rec["bar_met"] = bool(equal and a < rec["stock"]["ms_median"])
    return rec


def bench_archive(n_slides, h, w, K, z):
    """wall time of histogram_hdf5, device path against the numpy host path, on a synthetic archive"""
    images, masks = {}, {}
    for i in range(n_slides):
        c, m = make_input("runs", K, h * w, z, seed=100 + i)
        images[f"slide_{i:03d}"] = c.astype(np.uint8).reshape(h, w)
        masks[f"slide_{i:03d}_mask"] = m.astype(np.uint8).reshape(h, w)
    with tempfile.TemporaryDirectory() as d:
        path = hdf5.write_hdf5(os.path.join(d, "encodings.hdf5"), {"images": images, "masks": masks})
        code_stats.histogram_hdf5(path, num_embeddings=K)                         # warm-up: code objects, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = code_stats.histogram_hdf5(path, num_embeddings=K)
        t1 = time.perf_counter()
        host = code_stats.histogram_hdf5(path, num_embeddings=K, hist_fn=code_stats.host_code_histogram)
        t2 = time.perf_counter()
        r = hdf5.H5Reader(path)
        arrs = [(np.asarray(r["images"][s]), np.asarray(r["masks"][s + "_mask"])) for s in dev["stems"]]
        t3 = time.perf_counter()
        up = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in arrs]
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        out = torch.zeros((1, 3, K), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        for a, b in up:
            ops.code_histogram(a.view(1, -1), b.view(1, -1), num_embeddings=K, pooled=True, out=out)
        torch.cuda.synchronize()
        t6 = time.perf_counter()
    return {"slides": n_slides, "h": h, "w": w, "K": K, "equal": bool(np.array_equal(dev["pooled"]["joint"], host["pooled"]["joint"])),
            "device_path_s": round(t1 - t0, 4), "host_path_s": round(t2 - t1, 4), "host_over_device": round((t2 - t1) / (t1 - t0), 2),
            "read_archive_s": round(t3 - t2, 4), "upload_s": round(t4 - t3, 4), "kernels_s": round(t6 - t5, 5),
            "timing": "host clock around calls that end in a device synchronise (the download); the archive is in the page cache"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024x1024,4096x4096,6144x12288")
    ap.add_argument("--codebooks", default="256,1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--stock-steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--archive", default="3x4096x4096", help="slides x h x w of the synthetic archive ('' skips it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "code_stats.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_code_stats.py needs a GPU")
    z = np.load(os.path.join(ROOT, "tests", "golden", "code_marginals.npz"), allow_pickle=False)
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    rec = {"tool": "tools/bench_code_stats.py", "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "stock_steps": args.stock_steps, "rounds": args.rounds, "mean_run": MEAN_RUN,
           "timing": "HIP events around `steps` calls; the variants alternate round by round; median (min, max) round",
           "cases": []}
    for h, w in sizes:
        for K in (int(k) for k in args.codebooks.split(",")):
            by_kind = {}
            wide = np.uint8 if K <= 256 else np.uint16
            if wide is not np.uint8:                                   # the uint8 grid of the same size into the larger table
                r = run_case("uniform", K, h, w, z, args.steps, args.stock_steps, args.rounds, args.warmup)
                rec["cases"].append(r)
                print(json.dumps(r), flush=True)
            for kind in ("uniform", "marginal", "runs"):
                r = run_case(kind, K, h, w, z, args.steps, args.stock_steps, args.rounds, args.warmup, wide)
                by_kind[kind] = r
                rec["cases"].append(r)
                print(json.dumps(r), flush=True)
                torch.cuda.empty_cache()
            for kind in ("marginal", "runs"):
                by_kind[kind]["over_uniform"] = round(by_kind[kind]["kernel"]["ms_median"] / by_kind["uniform"]["kernel"]["ms_median"], 2)
    big = max(sizes, key=lambda s: s[0] * s[1])
    rec["bar"] = "kernel < stock on all three inputs at the largest size, with equal counts"
    rec["bar_met"] = all(r["bar_met"] for r in rec["cases"] if (r["h"], r["w"]) == big)
    if args.archive:
        ns, h, w = (int(v) for v in args.archive.split("x"))
        rec["archive"] = bench_archive(ns, h, w, 256, z)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "cases"}))
    if not rec["bar_met"]:
        raise SystemExit("the kernel is not faster than torch.bincount on every input at the largest size")


if __name__ == "__main__":
    main()
