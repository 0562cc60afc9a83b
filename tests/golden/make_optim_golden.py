#!/usr/bin/env python3
"""Generate tests/golden/optim_multi.npz: the reference's own optimisers on a list of eleven tensors shaped like an
auto-encoder's parameters -- Fixup scalars, short vectors around the 64-element bound, a conv weight, a multi-row vector.

Build container only: imports the unmodified reference through _ref_shims (vq_ae.optim.lamb.Lamb, vq_ae.optim.sam.SAM) exactly
as make_classifier_optim_golden.py does, whose case table, `run` and `measure` are used here.  No arithmetic is shimmed.

The problem (`problem()` below, which the tests import to regenerate it; nothing of it but the weights is stored):
  SHAPES / what starts where:  (1,) = 0 (a Fixup bias: LAMB's zero-norm branch), (1,) = 1 (a Fixup scale), (1,) = 0.3, (3,),
  (8,) = 0, (63,), (64,), (65,), (257,), (8, 8, 3, 3), (1025,) -- 2 064 numbers; the others from torch.Generator(4000), N(0, 1)
  (the conv weight times 1.6 / sqrt(72)); T = 8 steps of fp64 gradients from RandomState(4001), N(0, 1) * 0.1 per element; the
  second half of the (257,) tensor gets exactly 0.  SAM's second pass of a step sees 0.9 x that step's gradients.  The fp32
  runs see every gradient rounded to fp32 once.

Cases, lr, betas, eps, rho: make_classifier_optim_golden.CASES.

Keys
  cases, T, lr
  w_<i>                                          the initial weights, fp32, list order
  <case>/p32_<i>, p64_<i>                        the parameters after T steps of the fp32 / the fp64 run
  <case>/m32_<i>, m64_<i>, v32_<i>, v64_<i>      exp_avg and exp_avg_sq after T steps

    python tests/golden/make_optim_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_classifier_optim_golden as G  # noqa: E402   (CASES, EPS, LR, RHO, run(), measure(); imports no reference code)

T = 8
LR, RHO, CASES, EPS = G.LR, G.RHO, G.CASES, G.EPS
SHAPES = ((1,), (1,), (1,), (3,), (8,), (63,), (64,), (65,), (257,), (8, 8, 3, 3), (1025,))
FIXED = {0: 0.0, 1: 1.0, 2: 0.3, 4: 0.0}            # tensor -> the value it starts at
HALF_ZERO = 8                                       # the tensor whose second half never sees a gradient
measure, run = G.measure, G.run


def problem(steps=T, seed=4000):
    """-> (weights: eleven fp32 arrays, grads: [steps][11] fp64 arrays)"""
    gen = torch.Generator().manual_seed(seed)
    ws = []
    for i, s in enumerate(SHAPES):
        if i in FIXED:
            w = torch.full(s, FIXED[i])
        elif len(s) == 4:
            w = torch.randn(s, generator=gen) * (1.6 / (s[1] * 9) ** 0.5)
        else:
            w = torch.randn(s, generator=gen)
        ws.append(w.numpy().copy())
    rs = np.random.RandomState(seed + 1)
    grads = []
    for _ in range(steps):
        gs = [rs.standard_normal(s) * 0.1 for s in SHAPES]
        gs[HALF_ZERO][SHAPES[HALF_ZERO][0] // 2:] = 0.0
        grads.append(gs)
    return ws, grads


def main():
    import _ref_shims
    _ref_shims.install()
    from vq_ae.optim.lamb import Lamb                         # the reference
    from vq_ae.optim.sam import SAM

    targets = {"adam": "torch.optim.Adam", "adamw": "torch.optim.AdamW", "lamb": "vq_ae.optim.lamb.Lamb"}
    classes = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "lamb": Lamb}
    ws, grads = problem()
    out = {"cases": np.array(list(CASES)), "T": np.asarray(T), "lr": np.asarray(LR)}
    for i, w in enumerate(ws):
        out[f"w_{i}"] = w
    zero = [np.zeros_like(w) for w in ws]
    for case, (kind, wd, adaptive) in CASES.items():
        hyper = dict(lr=LR, betas=(0.9, 0.999), eps=EPS[kind], weight_decay=wd)

        def make(ps):
            if adaptive is None:
                return classes[kind](ps, **hyper)
            return SAM(ps, dict(hyper, _target_=targets[kind], params=None), rho=RHO, adaptive=adaptive)

        res = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            res[tag] = run(make, ws, grads, dt, adaptive is not None)
            for name, arrs in zip("pmv", res[tag]):
                for i, a in enumerate(arrs):
                    out[f"{case}/{name}{tag}_{i}"] = a
        yard = [measure(res["32"][k], res["64"][k], start) for k, start in enumerate((ws, zero, zero))]
        assert all(y > 0 for y in yard), (case, yard)             # the yardsticks of the tests
        print(f"{case}: yardstick p {yard[0]:.2e}  m {yard[1]:.2e}  v {yard[2]:.2e}")
    path = os.path.join(HERE, "optim_multi.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
