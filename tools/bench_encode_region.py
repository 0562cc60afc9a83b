#!/usr/bin/env python3
"""Cost of the way in from an array slide to code grids on one GPU: a synthetic slide at cfg A (512 x 512 tiles, f16), by
default 32 x 64 = 2048 tiles (a 16384 x 32768-pixel canvas, 1.6 GB, and its mask).  Three measurements, one JSON record:

  1. kernels      vqae_cut_pixels_u8 (levels 0 and 1 over every tile of the slide) and vqae_pool_labels_u8 (window 16, the
                  slide's mask) alone, each beside a device-to-device copy that moves the same number of bytes.
  2. resident     encode_region on the resident canvas against encode_u8 on the same tiles cut beforehand, in the same
                  batches.  The cut moves 1.5 MB per tile next to an encoder step of tens of microseconds per tile, so the
                  expectation is a ratio within the spread of the baseline's own repeats; the record says whether it is.  If
                  it is not, the follow-up is reading the tiles from the canvas inside the in-stem (not done here).
  3. end to end   encode_slide from the host array against get_encodings over a SyntheticSlideDataset of the same slide
                  (its tiles sliced from the same host array) with run_eval's default loader, both with their stage tables;
                  the get_encodings repeats run first, before this process holds a large page-locked allocation.
                  A report, not a bar: it depends on the host.

    python tools/bench_encode_region.py [--rows 32 --cols 64 --batch 64 --rounds 7 --out profiles/encode_region.json]

The measurements run in a child process under --time-limit seconds; the parent never opens the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps            # ms per call


def alternate(fns, steps, rounds, warmup):
    """{name: [ms per call, one per round]}: every round times each function in turn"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, steps))
    return out


def _r(values):
    return [round(v, 4) for v in values]


def build_model():
    """cfg A as tools/bench_slide.py builds it: random weights with working residual branches, fp16 handle"""
    import torch
    import vqae_amd
    from vqae_amd.model import VQAE
    spec = vqae_amd.SPECS["A"]
    torch.manual_seed(0)
    model = VQAE.from_spec(spec).eval()
    with torch.no_grad():                           # the reference zero-initialises branch_conv3: make the blocks do work
        for n, p in model.named_parameters():
            if n.endswith("branch_conv3.weight"):
                p.normal_(0.0, 0.5 / p.shape[1] ** 0.5)
    nat = vqae_amd.NativeVQAE(spec, dict(model.state_dict()), compute_dtype="f16")
    return nat, model.state_dict()["encoder.vq_layers.0.embed"]


def run_kernels(canvas, mask, rows, cols, steps, rounds, warmup):
    import torch
    import vqae_amd
    ops = vqae_amd.ops
    rc = torch.tensor([(r, c) for r in range(rows) for c in range(cols)], dtype=torch.int32, device="cuda")
    out = {}
    for level in (0, 1):
        f = 1 << level
        h = 512 // f
        tiles = torch.empty((rows * cols, h, h, 3), dtype=torch.uint8, device="cuda")
        moved = canvas.numel() + tiles.numel()
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda").random_()
        dst = torch.empty_like(src)
        ms = alternate({"cut": lambda: ops.cut_pixels_u8(canvas, rc, h, h, level=level, out=tiles), "copy": lambda: dst.copy_(src)},
                       steps, rounds, warmup)
        k, c = statistics.median(ms["cut"]), statistics.median(ms["copy"])
        out[f"cut_level_{level}"] = {"tiles": rows * cols, "tile": [h, h, 3], "bytes_moved": moved, "ms": round(k, 4),
                                     "copy_ms": round(c, 4), "GB_per_s": round(moved / k / 1e6, 1),
                                     "copy_GB_per_s": round(moved / c / 1e6, 1), "share_of_copy_rate": round(c / k, 4),
                                     "rounds_ms": _r(ms["cut"]), "copy_rounds_ms": _r(ms["copy"])}
        del tiles, src, dst
    moved = mask.numel() + mask.numel() // 256
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda").random_()
    dst = torch.empty_like(src)
    ms = alternate({"pool": lambda: ops.pool_labels_u8(mask, 16), "copy": lambda: dst.copy_(src)}, steps, rounds, warmup)
    k, c = statistics.median(ms["pool"]), statistics.median(ms["copy"])
    out["pool_win_16"] = {"mask": list(mask.shape), "bytes_moved": moved, "ms": round(k, 4), "copy_ms": round(c, 4),
                          "GB_per_s": round(moved / k / 1e6, 1), "copy_GB_per_s": round(moved / c / 1e6, 1),
                          "share_of_copy_rate": round(c / k, 4), "rounds_ms": _r(ms["pool"]), "copy_rounds_ms": _r(ms["copy"])}
    return out


def run_resident(nat, canvas, rows, cols, batch, rounds, warmup):
    import torch
    import vqae_amd
    n = rows * cols
    rc = torch.tensor([(r, c) for r in range(rows) for c in range(cols)], dtype=torch.int32, device="cuda")
    tiles = vqae_amd.ops.cut_pixels_u8(canvas, rc, 512, 512)
    enc = nat.with_dtype(torch.float16)

    def baseline():
        for lo in range(0, n, batch):
            enc.encode_u8(tiles[lo:lo + batch], idx_dtype=torch.uint8)

    def region():
        vqae_amd.encode_region(nat, canvas, None, 32, batch_size=batch)

    ms = alternate({"encode_u8_precut": baseline, "encode_region": region}, 1, rounds, warmup)
    a, b = statistics.median(ms["encode_u8_precut"]), statistics.median(ms["encode_region"])
    lo, hi = min(ms["encode_u8_precut"]) / a, max(ms["encode_u8_precut"]) / a
    ratio = b / a
    # the grids agree with the baseline's codes (bit-exact batch invariance of the encoder)
    grid, _ = vqae_amd.encode_region(nat, canvas, None, 32, batch_size=batch, rows=1)
    want = torch.cat([enc.encode_u8(tiles[c:c + 1], idx_dtype=torch.uint8)[1][0] for c in range(cols)], 1)
    assert torch.equal(grid, want), "encode_region differs from encode_u8 on the pre-cut tiles"
    return {"tiles": n, "batch": batch, "encode_u8_precut_ms": round(a, 3), "encode_region_ms": round(b, 3), "ratio": round(ratio, 4),
            "baseline_spread": [round(lo, 4), round(hi, 4)], "ratio_within_baseline_spread": bool(ratio <= hi),
            "us_per_tile": {"encode_u8_precut": round(a * 1e3 / n, 2), "encode_region": round(b * 1e3 / n, 2)},
            "follow_up_if_outside": "read the tiles from the canvas inside the in-stem instead of cutting them first",
            "rounds_ms": {k: _r(v) for k, v in ms.items()}}


def run_end_to_end(nat, pixels, mask, rows, cols, batch, band_rows, repeats):
    import numpy as np
    import torch
    import vqae_amd
    from vqae_amd.extract_embeddings import StageTimer, SyntheticSlideDataset, get_encodings

    class ArraySlide(SyntheticSlideDataset):
        """the item contract of SyntheticSlideDataset; the tiles are slices of the host array encode_slide reads"""

        def __getitem__(self, index):
            s, r, c = self.locate(index)
            img = torch.from_numpy(pixels[r * 512:(r + 1) * 512, c * 512:(c + 1) * 512])
            lab = torch.from_numpy(mask[r * 512:(r + 1) * 512, c * 512:(c + 1) * 512])[None]
            return img, lab, (s, np.asarray((r, c)), self.image_paths[s], self.mask_paths[s])

    ds = ArraySlide([(rows, cols)], patch_size=512, raw=True, names=["slide_000"])
    out = {"get_encodings": [], "encode_slide": []}
    grids = {}
    # get_encodings first: a process that holds a large torch page-locked allocation -- encode_slide's staging buffers stay in
    # torch's host cache -- slows the ring loader's copies many times over (open observation)
    for _ in range(repeats):
        timer = StageTimer()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = dict(get_encodings(nat, ds, batch_size=batch, timer=timer))            # run_eval's default loader and workers
        dt = time.perf_counter() - t0
        out["get_encodings"].append({"seconds": round(dt, 3), "tiles_per_s": round(rows * cols / dt, 1), "stages": timer.summary()})
        grids["get_encodings"] = (got["images/slide_000"], got["masks/slide_000_mask"])
    for _ in range(repeats):
        timer = StageTimer()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g, l = vqae_amd.encode_slide(nat, pixels, mask, 32, band_rows=band_rows, batch_size=batch, timer=timer)
        dt = time.perf_counter() - t0
        out["encode_slide"].append({"seconds": round(dt, 3), "tiles_per_s": round(rows * cols / dt, 1), "stages": timer.summary()})
        grids["encode_slide"] = (g, l)
    same = all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(grids["encode_slide"], grids["get_encodings"]))
    assert same, "encode_slide and get_encodings differ"
    med = {k: statistics.median(r["seconds"] for r in v) for k, v in out.items()}
    return {"tiles": rows * cols, "batch": batch, "band_rows": band_rows, "host_cores": len(os.sched_getaffinity(0)),
            "loader": "run_eval defaults: ring loader, 6 workers, prefetch 5",
            "order": "every get_encodings repeat before the first encode_slide (no large torch page-locked allocation yet)", "grids_equal": bool(same),
            "median_seconds": {k: round(v, 3) for k, v in med.items()},
            "speedup_encode_slide": round(med["get_encodings"] / med["encode_slide"], 3), "repeats": out}


def child(a):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_encode_region.py needs a GPU")
    g = torch.Generator(device="cuda").manual_seed(1)
    H, W = a.rows * 512, a.cols * 512
    canvas = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    mask = (torch.rand((H, W), device="cuda", generator=g) > 0.995).to(torch.uint8)
    nat, embed = build_model()
    calib = canvas[:512, :2048].reshape(512, 4, 512, 3).permute(1, 0, 2, 3).float()
    import vqae_amd
    mean, std = (torch.tensor(v, device="cuda") * 255 for v in (vqae_amd.ops.MEAN, vqae_amd.ops.STD))
    nat.calibrate_codebook(((calib - mean) / std).permute(0, 3, 1, 2).contiguous(), embed)
    nat.with_dtype(torch.float16).reserve(a.batch, 512, 512)
    rec = {"tool": "tools/bench_encode_region.py", "device": torch.cuda.get_device_name(0), "config": "A", "dtype": "f16",
           "slide": {"tiles": [a.rows, a.cols], "pixels": [H, W, 3]}, "rounds": a.rounds,
           "timing": "1, 2: HIP events, the variants alternate round by round, median round; 3: host clock around the whole call"}
    rec["kernels"] = run_kernels(canvas, mask, a.rows, a.cols, a.steps, a.rounds, a.warmup)
    rec["resident"] = run_resident(nat, canvas, a.rows, a.cols, a.batch, a.rounds, a.warmup)
    pixels, mask_host = canvas.cpu().numpy(), mask.cpu().numpy()
    del canvas, mask
    torch.cuda.empty_cache()
    rec["end_to_end"] = run_end_to_end(nat, pixels, mask_host, a.rows, a.cols, a.batch, a.band_rows, a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--cols", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--band-rows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="kernel calls per timed round (measurement 1)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="end-to-end repeats (measurement 3)")
    ap.add_argument("--time-limit", type=int, default=480, help="seconds the child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_region.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=a.time_limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"bench_encode_region.py: the measurements did not finish in {a.time_limit} s")
    raise SystemExit(rc)


if __name__ == "__main__":
    main()
