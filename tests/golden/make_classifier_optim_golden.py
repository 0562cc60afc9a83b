#!/usr/bin/env python3
"""Generate tests/golden/classifier_optim.npz: the reference's own optimisers on the shipped classifier's seven tensors.

Build container only: imports the unmodified reference through _ref_shims (vq_ae.optim.lamb.Lamb, vq_ae.optim.sam.SAM, whose
`instantiate` of base_optimizer_conf is the shim's) and runs each case for T steps on procedural weights and gradients, once
in fp32 and once in fp64.  No arithmetic is shimmed.  torch.optim.Adam / AdamW are torch's own.

The problem (`problem()` below, which the tests import to regenerate it; nothing of it but the weights is stored):
  variant E1C8O1 at K = 256: embedding.weight [256,1], in_conv.weight [8,1,3,3], .bias [8], hidden_conv1.weight [8,8,3,3],
  .bias [8], out_conv.weight [1,8,3,3], .bias [1] -- 993 numbers; weights from torch.Generator(3000) as in
  make_classifier_train_golden.py, but the three biases start at exactly 0 (LAMB's zero-norm branch: trust ratio 1);
  T = 16 steps of fp64 gradients from RandomState(3001), N(0, 1) * 0.1 per element; table rows 128 .. 255 get exactly 0
  (codes that never occur: they move by decay only).  SAM's second pass of a step sees 0.9 x that step's gradients.
  The fp32 runs see every gradient rounded to fp32 once, as `.grad` of an fp32 parameter holds it.

Cases (lr 1e-2, betas (0.9, 0.999) everywhere; eps 1e-8 for Adam / AdamW, 1e-6 for Lamb: each optimiser's default)
  adam       torch.optim.Adam, weight_decay 0.01          adamw      torch.optim.AdamW, weight_decay 0.01
  lamb_wd0   Lamb, weight_decay 0                          lamb       Lamb, weight_decay 0.01
  sam_adamw  SAM(rho 0.05) over AdamW(weight_decay 0.01)   asam_lamb  SAM(rho 0.05, adaptive) over Lamb(weight_decay 0.01)

Keys
  cases, T, lr
  w_<i>                              the initial weights, fp32, parameter order
  <case>/p32_<i>, p64_<i>            the parameters after T steps of the fp32 / the fp64 run
  <case>/m32_<i>, m64_<i>, v32_<i>, v64_<i>     exp_avg and exp_avg_sq after T steps

    python tests/golden/make_classifier_optim_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

K, E, C, NO = 256, 1, 8, 1
T = 16
LR = 1e-2
RHO = 0.05
SHAPES = ((K, E), (C, E, 3, 3), (C,), (C, C, 3, 3), (C,), (NO, C, 3, 3), (NO,))
CASES = {"adam": ("adam", 0.01, None), "adamw": ("adamw", 0.01, None), "lamb_wd0": ("lamb", 0.0, None),
         "lamb": ("lamb", 0.01, None), "sam_adamw": ("adamw", 0.01, False), "asam_lamb": ("lamb", 0.01, True)}
EPS = {"adam": 1e-8, "adamw": 1e-8, "lamb": 1e-6}


def shapes_of(k, e, c, no=1):
    return ((k, e), (c, e, 3, 3), (c,), (c, c, 3, 3), (c,), (no, c, 3, 3), (no,))


def problem(shapes=SHAPES, steps=T, seed=3000):
    """-> (weights: seven fp32 arrays, grads: [steps][7] fp64 arrays)"""
    gen = torch.Generator().manual_seed(seed)
    ws = []
    for s in shapes:
        if len(s) == 2:
            w = torch.randn(s, generator=gen)
        elif len(s) == 4:
            w = torch.randn(s, generator=gen) * (1.6 / (s[1] * 9) ** 0.5)
        else:
            w = torch.zeros(s)
        ws.append(w.numpy().copy())
    rs = np.random.RandomState(seed + 1)
    grads = []
    for _ in range(steps):
        gs = [rs.standard_normal(s) * 0.1 for s in shapes]
        gs[0][shapes[0][0] // 2:] = 0.0
        grads.append(gs)
    return ws, grads


def run(make_opt, ws, grads, dtype, sam):
    """T steps of an optimiser built by make_opt(params) -> (params, exp_avg, exp_avg_sq) as fp64-or-fp32 arrays"""
    ps = [torch.nn.Parameter(torch.from_numpy(w).to(dtype).clone()) for w in ws]
    opt = make_opt(ps)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g).to(dtype)
        if sam:
            opt.first_step()
            for p, g in zip(ps, gs):
                p.grad = torch.from_numpy(0.9 * g).to(dtype)
            opt.second_step()
        else:
            opt.step()
    base = opt.base_optimizer if sam else opt
    return ([p.detach().numpy().copy() for p in ps], [base.state[p]["exp_avg"].numpy().copy() for p in ps],
            [base.state[p]["exp_avg_sq"].numpy().copy() for p in ps])


def measure(test, truth, start):
    """max over the tensors of ||(test - start) - (truth - start)|| / ||truth - start||, in fp64"""
    worst = 0.0
    for a, b, s in zip(test, truth, start):
        a, b, s = (np.asarray(x, np.float64) for x in (a, b, s))
        d = np.linalg.norm((b - s).ravel())
        worst = max(worst, float(np.linalg.norm(((a - s) - (b - s)).ravel()) / d) if d > 0 else float(np.abs(a - b).max()))
    return worst


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
        zero = [np.zeros_like(w) for w in ws]
        moved = max(float(np.linalg.norm((b - s).ravel()) / np.linalg.norm(s.ravel())) for b, s in zip(res["64"][0], ws)
                    if np.linalg.norm(s.ravel()) > 0)
        print(f"{case}: yardstick p {measure(res['32'][0], res['64'][0], ws):.2e}  m {measure(res['32'][1], res['64'][1], zero):.2e}"
              f"  v {measure(res['32'][2], res['64'][2], zero):.2e}  (parameters moved by up to {moved * 100:.0f} %)")
    path = os.path.join(HERE, "classifier_optim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
