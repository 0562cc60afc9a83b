#!/usr/bin/env python3
"""Generate tests/golden/classifier_ce.npz: the reference's own `validation_nn` training step with torch.nn.CrossEntropyLoss on
small code grids -- the three-class route of conf/model/loss_f/cross_entropy.yaml and
conf/model/optional_overrides/loss_f/cross_entropy_camelyon16_embeddings.yaml.

Build container only: imports the unmodified reference through _ref_shims plus make_classifier_train_golden's stand-ins,
instantiates validation_nn.model.CNNClassifier around the reference's SequentialFromKwargs exactly as
conf/model/cnn_classifier.yaml composes it, with loss_f = torch.nn.CrossEntropyLoss(weight, label_smoothing, reduction);
`CNNClassifier.step` (model.py:131-139) gives the logits and the loss, torch.autograd.grad over the module's parameters the
gradients.  No arithmetic is shimmed.  Every grid is a batch, so every nn.Conv2d takes ATen's oneDNN route (see
make_classifier_golden.py).  Weights are procedural as there (seeds 2100 + i).

Variants (embedding_dim, hidden, n_out): E1C8O3 (the shipped stack with [background, tissue, cancer] outputs), E1C16O2,
E4C8O4; num_embeddings = 256.

Keys
  variants, grids, label_smoothing
  codes_<grid> uint8 [B,H,W], labels_<n_out>_<grid> uint8 [B,H,W] in 0 .. n_out-1      RandomState(2)
  weight_<n_out>                         the class weights of the cam_* cases: [0, 0.0247, 0.9753] for n_out = 3 (the
                                         reference's override), a fixed vector with a zero first entry for the others
  <variant>/<state-dict name>            the reference module's own state_dict()
  <variant>/2x7x5/logits32, logits64     CNNClassifier.step's first output in fp32 and, after .double(), in fp64 (the smallest
                                         grid only: the logits of the others are 80 % of what the file would then hold)
  <variant>/<grid>/<case>/loss32, loss64
  <variant>/<grid>/<case>/g32_<i>, g64_<i>   the gradient of parameter i (the order of module.parameters())
     cases: ones_sum -- no weight, label_smoothing 0, reduction='sum', every grid;
            cam_mean -- weight_<n_out>, label_smoothing 0.001, reduction='mean', every grid;
            cam_sum  -- the same with reduction='sum', grid 2x37x70
  optim/<kind>/p32_<i>, p64_<i>          E1C8O3 after 8 closed-loop steps (step, backward, optimizer.step) on grid 2x37x70 with
  optim/<kind>/loss32, loss64 [8]        the cam_mean loss: kind adamw = torch.optim.AdamW(lr 1e-2, weight_decay 0.01),
                                         kind lamb = vq_ae.optim.lamb.Lamb(lr 1e-2, weight_decay 0.01); the losses of the steps

    python tests/golden/make_classifier_ce_golden.py
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shims  # noqa: E402
from make_classifier_train_golden import _stand_ins  # noqa: E402

VARIANTS = {"E1C8O3": (1, 8, 3), "E1C16O2": (1, 16, 2), "E4C8O4": (4, 8, 4)}
GRIDS = {"2x7x5": (2, 7, 5), "2x37x70": (2, 37, 70), "4x64x96": (4, 64, 96)}
WEIGHTS = {2: (0.0, 1.0), 3: (0.0, 0.0247, 0.9753), 4: (0.0, 0.05, 0.25, 0.7)}
LABEL_SMOOTHING = 0.001
EXTRA_GRID = "2x37x70"
LOGIT_GRID = "2x7x5"
K = 256
OPTIM_VARIANT, OPTIM_STEPS, OPTIM_LR, OPTIM_WD = "E1C8O3", 8, 1e-2, 0.01


def main():
    _ref_shims.install()
    _stand_ins()
    from validation_nn.layers.misc import FlattenAfterEmbedding, SequentialFromKwargs   # noqa: the reference
    from validation_nn.model import CNNClassifier
    from vq_ae.optim.lamb import Lamb

    rs = np.random.RandomState(2)
    out = {"variants": np.array(list(VARIANTS)), "grids": np.array(list(GRIDS)), "label_smoothing": np.asarray(LABEL_SMOOTHING)}
    for g, shape in GRIDS.items():
        out[f"codes_{g}"] = rs.randint(0, K, size=shape).astype(np.uint8)
    for no in (2, 3, 4):
        out[f"weight_{no}"] = np.asarray(WEIGHTS[no], np.float64)
        for g, shape in GRIDS.items():
            out[f"labels_{no}_{g}"] = rs.randint(0, no, size=shape).astype(np.uint8)

    def stack(E, C, NO):
        return SequentialFromKwargs(
            embedding=nn.Embedding(K, E), flatten_after_embedding=FlattenAfterEmbedding(),
            in_conv=nn.Conv2d(E, C, 3, padding=1), act1=nn.ELU(),
            hidden_conv1=nn.Conv2d(C, C, 3, padding=1), act2=nn.ELU(),
            out_conv=nn.Conv2d(C, NO, 3, padding=1))

    def loss_f(dtype, no, case):
        if case == "ones_sum":
            return nn.CrossEntropyLoss(reduction="sum")
        return nn.CrossEntropyLoss(weight=torch.tensor(WEIGHTS[no], dtype=dtype), label_smoothing=LABEL_SMOOTHING,
                                   reduction="mean" if case == "cam_mean" else "sum")

    def fresh(name, seed, dtype):
        E, C, NO = VARIANTS[name]
        model = CNNClassifier(optim=None, loss_f=None, layers=stack(E, C, NO))
        gen = torch.Generator().manual_seed(2100 + seed)
        with torch.no_grad():
            for m in model.layers:
                if isinstance(m, nn.Embedding):
                    m.weight.copy_(torch.randn(m.weight.shape, generator=gen))
                elif isinstance(m, nn.Conv2d):
                    m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (1.6 / (m.in_channels * 9) ** 0.5))
                    m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.3)
        return model.to(dtype)                                     # (fp32 weights, converted exactly)

    for seed, (name, (E, C, NO)) in enumerate(VARIANTS.items()):
        models = {"32": fresh(name, seed, torch.float32), "64": fresh(name, seed, torch.float64)}
        for k, v in models["32"].state_dict().items():
            if k.startswith("layers."):
                out[f"{name}/{k}"] = v.numpy().copy()
        for g in GRIDS:
            codes = torch.from_numpy(out[f"codes_{g}"].astype(np.int64))[:, None]
            labels = torch.from_numpy(out[f"labels_{NO}_{g}"].astype(np.int64))
            cases = ["ones_sum", "cam_mean"] + (["cam_sum"] if g == EXTRA_GRID else [])
            errs = []
            for case in cases:
                res = {}
                for tag, dt in (("32", torch.float32), ("64", torch.float64)):
                    model = models[tag]
                    model.loss_f = loss_f(dt, NO, case)
                    logits, loss = model.step(codes, labels)
                    grads = torch.autograd.grad(loss, list(model.parameters()))
                    assert loss.dtype == dt and logits.dtype == dt and all(gr.dtype == dt for gr in grads)
                    if g == LOGIT_GRID and case == "ones_sum":
                        out[f"{name}/{g}/logits{tag}"] = logits.detach().numpy().copy()
                    out[f"{name}/{g}/{case}/loss{tag}"] = np.asarray(float(loss.detach()), np.float32 if tag == "32" else np.float64)
                    res[tag] = [gr.numpy().copy() for gr in grads]
                    for i, gr in enumerate(res[tag]):
                        out[f"{name}/{g}/{case}/g{tag}_{i}"] = gr
                errs.append(max(float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()) for a, b in zip(res["32"], res["64"])))
            print(f"{name} {g}: e_ref = " + " ".join(f"{c}:{e:.2e}" for c, e in zip(cases, errs)))

    # ---- eight closed-loop optimiser steps on the shipped three-class stack ----------------------------------------------------
    name = OPTIM_VARIANT
    NO = VARIANTS[name][2]
    seed = list(VARIANTS).index(name)
    codes = torch.from_numpy(out[f"codes_{EXTRA_GRID}"].astype(np.int64))[:, None]
    labels = torch.from_numpy(out[f"labels_{NO}_{EXTRA_GRID}"].astype(np.int64))
    makers = {"adamw": lambda ps: torch.optim.AdamW(ps, lr=OPTIM_LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=OPTIM_WD),
              "lamb": lambda ps: Lamb(ps, lr=OPTIM_LR, betas=(0.9, 0.999), eps=1e-6, weight_decay=OPTIM_WD)}
    for kind, make in makers.items():
        end = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            model = fresh(name, seed, dt)
            model.loss_f = loss_f(dt, NO, "cam_mean")
            start = [p.detach().double().numpy().copy() for p in model.parameters()]
            opt = make(list(model.parameters()))
            losses = []
            for _ in range(OPTIM_STEPS):
                opt.zero_grad()
                _, loss = model.step(codes, labels)
                loss.backward()
                opt.step()
                losses.append(float(loss))
            out[f"optim/{kind}/loss{tag}"] = np.asarray(losses, np.float64)
            end[tag] = [p.detach().numpy().copy() for p in model.parameters()]
            for i, p in enumerate(end[tag]):
                out[f"optim/{kind}/p{tag}_{i}"] = p
        yard = max(float(np.linalg.norm(((a - s) - (b - s)).ravel()) / np.linalg.norm((b - s).ravel()))
                   for a, b, s in zip(end["32"], end["64"], start))
        print(f"optim {kind}: the fp32 run is {yard:.2e} from the fp64 run; losses {out[f'optim/{kind}/loss64'][0]:.4f} -> "
              f"{out[f'optim/{kind}/loss64'][-1]:.4f}")

    path = os.path.join(HERE, "classifier_ce.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
