#!/usr/bin/env python3
"""Generate tests/golden/code_marginals.npz: the count arrays the reference commits as data under
scripts/create_wsi_histograms/ (it ships no program that produces them), loaded and re-saved verbatim:

  embedding_idx_histogram_{128,256,512,1024}_{train,validation,test}.npy   codes per codebook size and split
  histogram_{train,val,test}.npy                                            [background, tissue, cancer] per split
  camelyon16_mask_histogram_bg_tissue_cancer.npy                            the same labels over the whole dataset

Each array is stored under its file's stem.  tests/test_code_stats_cpu.py, tests/test_code_stats_gpu.py and
tools/bench_code_stats.py read the .npz only.

    python tests/golden/make_code_stats_golden.py --reference /path/to/2D-VQ-AE-2
"""
import argparse
import glob
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of sara-nl/2D-VQ-AE-2")
    a = ap.parse_args()
    src = os.path.join(a.reference, "scripts", "create_wsi_histograms")
    files = sorted(glob.glob(os.path.join(src, "*.npy")))
    if len(files) != 16:
        raise SystemExit(f"expected the sixteen committed count arrays under {src}, found {len(files)}")
    arrays = {os.path.splitext(os.path.basename(f))[0]: np.load(f, allow_pickle=False) for f in files}
    path = os.path.join(HERE, "code_marginals.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB): " +
          ", ".join(f"{k} {v.dtype}{v.shape}" for k, v in arrays.items()))


if __name__ == "__main__":
    main()
