#!/usr/bin/env python3
"""Generate tests/golden/classifier.npz: the reference's own `validation_nn` classifier on small code grids.

Build container only: imports the unmodified reference through _ref_shims (plus a stand-in for `torchmetrics`, which
validation_nn/model.py imports for a type annotation), instantiates validation_nn.model.CNNClassifier around the
reference's SequentialFromKwargs(embedding=nn.Embedding, flatten_after_embedding=FlattenAfterEmbedding(), in_conv=...,
act1=..., hidden_conv1=..., act2=..., out_conv=...) exactly as conf/model/cnn_classifier.yaml composes it, and
utils.train_helpers.Camelyon16BCELoss(reduction='sum', label_smoothing=0).  No arithmetic is shimmed.

Every grid is a batch of two slides.  ATen's conv dispatcher sends a single small image (batch 1, at most 20480 elements,
3x3 kernel) to an im2col + BLAS GEMM, whose fp32 sums differ between machines and thread counts by more than the 1e-6 the
CPU test allows (1.7e-6 on a 7 x 5 grid was seen), and a batch to oneDNN's direct kernels, which the other fp32 fixtures of
this directory already rely on being reproducible.  With a batch of two every nn.Conv2d of the reference takes the oneDNN
route; the package's CPU restatement names that route explicitly (vqae_amd.classifier._conv3x3).

Variants (embedding_dim, hidden, n_out): E1C8O1 (the shipped one), E4C8O3, E1C16O1; num_embeddings = 256.
Weights are procedural and all non-zero: embedding ~ N(0, 1), conv weights ~ N(0, (1.6 / sqrt(fan_in))^2), biases
~ N(0, 0.3^2), from a seeded torch.Generator.

Keys
  variants                      the variant names
  grids                         the grid names: 1x1, 2x3, 7x5, 2x37x70 (each a batch of two slides)
  codes_<grid>   uint8 [B,H,W]  RandomState(0)
  mask_<grid>    uint8 [B,H,W]  labels in {0, 1, 2}
  <variant>/<state-dict name>   the reference module's own state_dict() (names as the reference spells them)
  <variant>/ref32_<grid>        fp32 [B,n_out,H,W]  the reference's forward
  <variant>/f64_<grid>          fp64 [B,n_out,H,W]  the same module after .double()
  <variant>/loss32_<grid>, <variant>/loss64_<grid>   [B,2]  per slide, Camelyon16BCELoss of those logits against the mask
                                with pos_weight 1 and 40.4858 (n_out == 1 variants only)

    python tests/golden/make_classifier_golden.py
"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shims  # noqa: E402

VARIANTS = {"E1C8O1": (1, 8, 1), "E4C8O3": (4, 8, 3), "E1C16O1": (1, 16, 1)}
GRIDS = {"1x1": (2, 1, 1), "2x3": (2, 2, 3), "7x5": (2, 7, 5), "2x37x70": (2, 37, 70)}
POS_WEIGHTS = (1.0, 40.4858)
K = 256


def main():
    _ref_shims.install()
    tm = types.ModuleType("torchmetrics")
    tm.MetricCollection = type("MetricCollection", (), {})
    sys.modules.setdefault("torchmetrics", tm)
    from utils.train_helpers import Camelyon16BCELoss            # noqa: the reference, unmodified
    from validation_nn.layers.misc import FlattenAfterEmbedding, SequentialFromKwargs
    from validation_nn.model import CNNClassifier

    rs = np.random.RandomState(0)
    out = {"variants": np.array(list(VARIANTS)), "grids": np.array(list(GRIDS))}
    for g, shape in GRIDS.items():
        out[f"codes_{g}"] = rs.randint(0, K, size=shape).astype(np.uint8)
    for g, shape in GRIDS.items():
        out[f"mask_{g}"] = rs.randint(0, 3, size=shape).astype(np.uint8)

    for seed, (name, (E, C, NO)) in enumerate(VARIANTS.items()):
        layers = SequentialFromKwargs(
            embedding=nn.Embedding(K, E), flatten_after_embedding=FlattenAfterEmbedding(),
            in_conv=nn.Conv2d(E, C, 3, padding=1), act1=nn.ELU(),
            hidden_conv1=nn.Conv2d(C, C, 3, padding=1), act2=nn.ELU(),
            out_conv=nn.Conv2d(C, NO, 3, padding=1))
        model = CNNClassifier(optim=None, loss_f=None, layers=layers).eval()
        gen = torch.Generator().manual_seed(1000 + seed)
        with torch.no_grad():
            for m in layers:
                if isinstance(m, nn.Embedding):
                    m.weight.copy_(torch.randn(m.weight.shape, generator=gen))
                elif isinstance(m, nn.Conv2d):
                    fan_in = m.in_channels * 9
                    m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (1.6 / fan_in ** 0.5))
                    m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.3)
        for k, v in model.state_dict().items():
            assert bool((v != 0).all()), k
            out[f"{name}/{k}"] = v.numpy().copy()
        model64 = CNNClassifier(optim=None, loss_f=None, layers=SequentialFromKwargs(
            embedding=nn.Embedding(K, E), flatten_after_embedding=FlattenAfterEmbedding(),
            in_conv=nn.Conv2d(E, C, 3, padding=1), act1=nn.ELU(),
            hidden_conv1=nn.Conv2d(C, C, 3, padding=1), act2=nn.ELU(),
            out_conv=nn.Conv2d(C, NO, 3, padding=1))).eval()
        model64.load_state_dict(model.state_dict())
        model64.double()
        for g in GRIDS:
            codes = torch.from_numpy(out[f"codes_{g}"].astype(np.int64))[:, None]
            mask = torch.from_numpy(out[f"mask_{g}"].astype(np.int64))
            with torch.no_grad():
                y32, y64 = model(codes), model64(codes)
            assert y32.dtype == torch.float32 and y64.dtype == torch.float64
            out[f"{name}/ref32_{g}"] = y32.numpy()
            out[f"{name}/f64_{g}"] = y64.numpy()
            if NO == 1:
                l32 = np.zeros((codes.shape[0], 2), np.float32)
                l64 = np.zeros((codes.shape[0], 2), np.float64)
                for j, pw in enumerate(POS_WEIGHTS):
                    f32 = Camelyon16BCELoss(reduction="sum", pos_weight=torch.tensor(pw), label_smoothing=0)
                    f64 = Camelyon16BCELoss(reduction="sum", pos_weight=torch.tensor(pw, dtype=torch.float64), label_smoothing=0)
                    for b in range(codes.shape[0]):
                        l32[b, j] = float(f32(y32[b:b + 1], mask[b:b + 1]))
                        l64[b, j] = float(f64(y64[b:b + 1], mask[b:b + 1]))
                out[f"{name}/loss32_{g}"], out[f"{name}/loss64_{g}"] = l32, l64
        e = max(float(np.abs(out[f"{name}/ref32_{g}"] - out[f"{name}/f64_{g}"]).max()) for g in GRIDS)
        print(f"{name}: max |ref32 - f64| = {e:.3e}; logits std {out[f'{name}/f64_2x37x70'].std():.2f} "
              f"max {np.abs(out[f'{name}/f64_2x37x70']).max():.1f}")
    path = os.path.join(HERE, "classifier.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
