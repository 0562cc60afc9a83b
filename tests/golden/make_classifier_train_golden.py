#!/usr/bin/env python3
"""Generate tests/golden/classifier_train.npz: the reference's own `validation_nn` training step on small code grids.

Build container only: imports the unmodified reference through _ref_shims (plus stand-ins for modules the reference imports
at module top and this script never calls: torchmetrics, albumentations, h5py, wsi_io.imagereader), instantiates
validation_nn.model.CNNClassifier around the reference's SequentialFromKwargs exactly as conf/model/cnn_classifier.yaml
composes it, and utils.train_helpers.Camelyon16BCELoss; `CNNClassifier.step` (model.py:131-139) gives the loss and
torch.autograd.grad over the module's parameters the gradients.  No arithmetic is shimmed.

Every grid is a batch (2 or 4 slides), so every nn.Conv2d of the reference takes ATen's oneDNN route, forward and backward
(see make_classifier_golden.py).  Weights are procedural as there (seeds 2000 + i).

Variants (embedding_dim, hidden, n_out): E1C8O1 (the shipped one), E1C16O1, E4C8O1; num_embeddings = 256.

Keys
  variants, grids, pos_weights
  codes_<grid> uint8 [B,H,W], mask_<grid> uint8 [B,H,W] in {0, 1, 2}      RandomState(1)
  <variant>/<state-dict name>            the reference module's own state_dict()
  <variant>/<grid>/<case>/loss32, loss64     the loss in fp32 and, after .double(), in fp64
  <variant>/<grid>/<case>/g32_<i>, g64_<i>   the gradient of parameter i (the order of module.parameters(): embedding.weight,
                                         in_conv.weight, in_conv.bias, hidden_conv1.weight, .bias, out_conv.weight, .bias)
     cases: pw0, pw1 -- reduction='sum' with pos_weight 1.0 / 40.4858, every grid;
            mean     -- reduction='mean', pos_weight 40.4858, grid 2x37x70;
            soft     -- reduction='sum', pos_weight 40.4858, grid 2x37x70, soft targets `soft_target` (below)
  soft_target  fp32 [2,37,70]  |1 - ((1 + t + N(0,1) * 0.3) mod 2)| (train_helpers.py:133-135) from a seeded generator, rounded
               to multiples of 2^-20.  The loss draws its smoothing noise itself and in the dtype of its input, so the fp32
               and the fp64 run would see different targets; instead the loss gets a FLOATING-POINT target grid 1 + soft
               (0 where the mask is 0) with label_smoothing=0: train_helpers.py:122-131 then uses target - 1 = soft as it
               stands (the rounding makes 1 + soft exact in fp32).
  split/keys                             toy slide names
  split/<frac>/<mode>                    _train_val_split_paths' images output for mode train / validation on the sorted
                                         normal* and tumor* names (camelyon16.py:239-246), and the names with 'test'
  collate/img_<i>, collate/msk_<i>       toy slides of unequal size; collate/seed
  collate/out_img, collate/out_msk       collate_unequal_sized_slides(batch) after np.random.seed(collate/seed)

    python tests/golden/make_classifier_train_golden.py
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

VARIANTS = {"E1C8O1": (1, 8, 1), "E1C16O1": (1, 16, 1), "E4C8O1": (4, 8, 1)}
GRIDS = {"2x7x5": (2, 7, 5), "2x37x70": (2, 37, 70), "4x64x96": (4, 64, 96)}
POS_WEIGHTS = (1.0, 40.4858)
EXTRA_GRID = "2x37x70"
K = 256
SPLIT_KEYS = [f"normal_{i:03d}" for i in (1, 2, 3, 5, 8, 13, 21)] + [f"tumor_{i:03d}" for i in (4, 6, 7, 9, 10)] + \
             ["test_001", "test_002", "test_040"]
SPLIT_FRACS = (0.9, 0.5, 0.1)
COLLATE_SHAPES = ((9, 11), (7, 13), (12, 8))
COLLATE_SEED = 7


def _stand_ins():
    tm = types.ModuleType("torchmetrics")
    tm.MetricCollection = type("MetricCollection", (), {})
    sys.modules.setdefault("torchmetrics", tm)
    al = types.ModuleType("albumentations")
    al.BasicTransform = type("BasicTransform", (), {})
    alp = types.ModuleType("albumentations.pytorch")
    al.pytorch = alp
    sys.modules.setdefault("albumentations", al)
    sys.modules.setdefault("albumentations.pytorch", alp)
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    wi = types.ModuleType("wsi_io")
    wr = types.ModuleType("wsi_io.imagereader")
    wr.ImageReader = type("ImageReader", (), {})
    wi.imagereader = wr
    sys.modules.setdefault("wsi_io", wi)
    sys.modules.setdefault("wsi_io.imagereader", wr)


def main():
    _ref_shims.install()
    _stand_ins()
    from datamodules.camelyon16 import _train_val_split_paths, collate_unequal_sized_slides   # noqa: the reference
    from utils.train_helpers import Camelyon16BCELoss
    from validation_nn.layers.misc import FlattenAfterEmbedding, SequentialFromKwargs
    from validation_nn.model import CNNClassifier

    rs = np.random.RandomState(1)
    out = {"variants": np.array(list(VARIANTS)), "grids": np.array(list(GRIDS)), "pos_weights": np.array(POS_WEIGHTS)}
    for g, shape in GRIDS.items():
        out[f"codes_{g}"] = rs.randint(0, K, size=shape).astype(np.uint8)
    for g, shape in GRIDS.items():
        out[f"mask_{g}"] = rs.randint(0, 3, size=shape).astype(np.uint8)
    gen = torch.Generator().manual_seed(77)
    t = torch.from_numpy(out[f"mask_{EXTRA_GRID}"]).float() - 1
    soft = (1 - ((1 + t + torch.randn(t.shape, generator=gen) * 0.3) % 2)).abs()
    soft = (torch.round(soft * 2 ** 20) / 2 ** 20).clamp(0, 1)
    out["soft_target"] = soft.numpy()

    def stack(E, C, NO):
        return SequentialFromKwargs(
            embedding=nn.Embedding(K, E), flatten_after_embedding=FlattenAfterEmbedding(),
            in_conv=nn.Conv2d(E, C, 3, padding=1), act1=nn.ELU(),
            hidden_conv1=nn.Conv2d(C, C, 3, padding=1), act2=nn.ELU(),
            out_conv=nn.Conv2d(C, NO, 3, padding=1))

    def run(model, dtype, codes, target, pw, reduction):
        model.loss_f = Camelyon16BCELoss(reduction=reduction, pos_weight=torch.tensor(pw, dtype=dtype), label_smoothing=0)
        _, loss = model.step(codes, target)
        grads = torch.autograd.grad(loss, list(model.parameters()))
        assert loss.dtype == dtype and all(g.dtype == dtype for g in grads)
        return float(loss), [g.numpy().copy() for g in grads]

    for seed, (name, (E, C, NO)) in enumerate(VARIANTS.items()):
        model = CNNClassifier(optim=None, loss_f=None, layers=stack(E, C, NO))
        gen = torch.Generator().manual_seed(2000 + seed)
        with torch.no_grad():
            for m in model.layers:
                if isinstance(m, nn.Embedding):
                    m.weight.copy_(torch.randn(m.weight.shape, generator=gen))
                elif isinstance(m, nn.Conv2d):
                    m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (1.6 / (m.in_channels * 9) ** 0.5))
                    m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.3)
        for k, v in model.state_dict().items():
            if k.startswith("layers."):
                out[f"{name}/{k}"] = v.numpy().copy()
        model64 = CNNClassifier(optim=None, loss_f=None, layers=stack(E, C, NO))
        model64.load_state_dict(model.state_dict())
        model64.double()
        for g in GRIDS:
            codes = torch.from_numpy(out[f"codes_{g}"].astype(np.int64))[:, None]
            mask = torch.from_numpy(out[f"mask_{g}"].astype(np.int64))
            cases = {"pw0": (mask, POS_WEIGHTS[0], "sum"), "pw1": (mask, POS_WEIGHTS[1], "sum")}
            if g == EXTRA_GRID:
                cases["mean"] = (mask, POS_WEIGHTS[1], "mean")
                cases["soft"] = (None, POS_WEIGHTS[1], "sum")
            errs = []
            for case, (tgt, pw, red) in cases.items():
                res = {}
                for tag, mdl, dt in (("32", model, torch.float32), ("64", model64, torch.float64)):
                    tg = tgt if tgt is not None else ((1 + soft) * (mask != 0)).to(dt)
                    loss, grads = run(mdl, dt, codes, tg, pw, red)
                    out[f"{name}/{g}/{case}/loss{tag}"] = np.asarray(loss, np.float32 if tag == "32" else np.float64)
                    for i, gr in enumerate(grads):
                        out[f"{name}/{g}/{case}/g{tag}_{i}"] = gr
                    res[tag] = grads
                errs.append(max(float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()) for a, b in zip(res["32"], res["64"])))
            print(f"{name} {g}: e_ref = " + " ".join(f"{c}:{e:.2e}" for c, e in zip(cases, errs)))

    # ---- the dataset's split and the collate function ------------------------------------------------------------------
    out["split/keys"] = np.array(SPLIT_KEYS)
    keys = np.sort(SPLIT_KEYS)
    for frac in SPLIT_FRACS:
        for mode in ("train", "validation"):
            mods = [tuple(zip(*((k, k + "_mask") for k in keys if pat in k))) for pat in ("normal", "tumor")]
            images, masks = _train_val_split_paths(mods, split_frac=frac, mode=mode)
            assert [i + "_mask" for i in images] == list(masks)
            out[f"split/{frac}/{mode}"] = np.array(list(images))
    out["split/test"] = np.array([k for k in keys if "test" in k])
    crs = np.random.RandomState(5)
    batch = []
    for i, shp in enumerate(COLLATE_SHAPES):
        img, msk = crs.randint(0, K, shp).astype(np.int32), crs.randint(0, 3, shp).astype(np.int64)
        out[f"collate/img_{i}"], out[f"collate/msk_{i}"] = img, msk
        batch.append((img, msk))
    out["collate/seed"] = np.asarray(COLLATE_SEED)
    np.random.seed(COLLATE_SEED)
    oi, om = collate_unequal_sized_slides(batch)
    out["collate/out_img"], out["collate/out_msk"] = oi.numpy(), om.numpy()

    path = os.path.join(HERE, "classifier_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
