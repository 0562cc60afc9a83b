#!/usr/bin/env python3
"""Generate tests/golden/vq_backward.npz: the gradients of the reference's quantisers, from the reference's own autograd.

Build container only: imports the unmodified reference vq_ae/layers/vq.py through _ref_shims (the file imports only torch)
and records, for seeded inputs and first_pass = 0,
    torch.autograd.grad([out, loss], [x, *parameters], [g_out, g_loss])
once in fp32 and once after .double().  The generator ASSERTS that both runs chose identical indices (a gradient recorded
across an index flip would compare two different functions) and fails otherwise.

Cases
  plain quantiser (K = 64, cc = 0.25, eval): plain_2x6x11 (p = 3), plain_2x12x3x5, plain_1x5x2x3x4 (p = 5)
  projected quantiser (P = 8, K = 256, cc = 0.25), eval and train mode (decay 0.99):
      proj_2x12x3x5, proj_3x128x8x8, proj_1x64x33x17, proj_1x256x4x4
  the fallback (P = 4, K = 64): proj4_2x12x3x5, eval and train mode
  the fallback at a width the mirror's own forward takes (P = 16, K = 64): proj16_2x16x3x5, eval and train mode

Keys
  cases                                   the names above
  <case>/x, <case>/g_out                  float16: multiples of 1/16 (x) and 1/64 (g_out), exact in float16; use .astype(float32)
  <case>/g_loss                           float32 0-d, <case>/cc
  <case>/sd/<name>                        the reference module's state_dict() before the forward (first_pass = 0)
  <case>/idx                              int16, the indices of the fp32 run (= those of the fp64 run)
  <case>/n_grads                          x first, then module.parameters(): proj_in.weight, .bias, proj_out.weight, .bias
  <case>/<mode>/g32_<i>                   float32 gradient i of the fp32 run, mode in (eval, train)
  <case>/<mode>/g64_<i>                   float64 gradient i of the fp64 run, i >= 1
  <case>/<mode>/g64lo_0                   float32(g64_0 - g32_0): the input gradient of the fp64 run is g32_0 + g64lo_0 in
                                          float64 (48 bits, < 1e-14 relative: the file stays under 1 MB)
  <case>/train_equals_eval                1: the train-mode gradients equal the eval-mode ones bit for bit in both dtypes
                                          (the lookup precedes the EMA update, vq.py:130-133) and only `eval` is stored
  loop/...                                the closed loop: Conv2d(3, 16, 1) -> projected VQ (C = 16, P = 8, K = 64, train mode,
                                          decay 0.99, cc = 0.25) -> Conv2d(16, 3, 1), loss = mse(out, target) + vq loss, plain
                                          SGD (lr 0.05), 3 steps on 3 batches [2, 3, 8, 8]:
      loop/x, loop/target [3, 2, 3, 8, 8] float16 grids; loop/lr; loop/sd0/<name> the initial state dict of
      nn.Sequential-free module names enc / vq / dec; loop/idx [3, 2, 8, 8] int16 (equal in both dtypes at every step)
      loop/loss32, loop/loss64 [3]; loop/final32/<name>, loop/final64/<name> parameters AND buffers after step 3

    python tests/golden/make_vq_backward_golden.py
"""
import copy
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shims  # noqa: E402

CC, DECAY, ALPHA = 0.25, 0.99, 1e-5
PLAIN = {"plain_2x6x11": (2, 6, 11), "plain_2x12x3x5": (2, 12, 3, 5), "plain_1x5x2x3x4": (1, 5, 2, 3, 4)}
PROJ = {"proj_2x12x3x5": (2, 12, 3, 5), "proj_3x128x8x8": (3, 128, 8, 8), "proj_1x64x33x17": (1, 64, 33, 17),
        "proj_1x256x4x4": (1, 256, 4, 4)}
PROJ4 = {"proj4_2x12x3x5": (2, 12, 3, 5)}
PROJ16 = {"proj16_2x16x3x5": (2, 16, 3, 5)}


def grid(shape, gen, step):
    """randn rounded to multiples of `step` (a power of two), clipped to +-4: exact in float16."""
    t = (torch.round(torch.randn(shape, generator=gen) / step) * step).clamp(-4, 4)
    assert torch.equal(t.half().float(), t)
    return t


def run(module, dtype, train, x32, g_out32, g_loss32):
    m = copy.deepcopy(module).to(dtype).train(train)
    x = x32.to(dtype).requires_grad_()
    out, idx, loss = m(x)
    grads = torch.autograd.grad([out, loss], [x] + list(m.parameters()), [g_out32.to(dtype), g_loss32.to(dtype)])
    assert all(g.dtype == dtype for g in grads)
    return idx, [g.detach().clone() for g in grads]


def rel(a, b):
    return float((a.double() - b).norm() / b.norm())


def record_case(out, name, module, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    x = grid(shape, gen, 1 / 16)
    g_out = grid(shape, gen, 1 / 64)
    g_loss = torch.tensor(0.75 + 0.125 * (seed % 3))
    module.first_pass.mul_(0)
    out[f"{name}/x"], out[f"{name}/g_out"] = x.half().numpy(), g_out.half().numpy()
    out[f"{name}/g_loss"], out[f"{name}/cc"] = g_loss.numpy(), np.asarray(CC)
    for k, v in module.state_dict().items():
        out[f"{name}/sd/{k}"] = v.numpy().copy()
    res = {}
    for mode, train in (("eval", False), ("train", True)):
        i32, g32 = run(module, torch.float32, train, x, g_out, g_loss)
        i64, g64 = run(module, torch.float64, train, x, g_out, g_loss)
        assert torch.equal(i32, i64), f"{name} {mode}: fp32 and fp64 chose different indices"
        res[mode] = (i32, g32, g64)
    assert torch.equal(res["eval"][0], res["train"][0])
    same = all(torch.equal(a, b) for a, b in zip(res["eval"][1] + res["eval"][2], res["train"][1] + res["train"][2]))
    out[f"{name}/train_equals_eval"] = np.asarray(int(same))
    out[f"{name}/idx"] = res["eval"][0].numpy().astype(np.int16)
    out[f"{name}/n_grads"] = np.asarray(len(res["eval"][1]))
    for mode in (("eval",) if same else ("eval", "train")):
        _, g32, g64 = res[mode]
        for i, (a, b) in enumerate(zip(g32, g64)):
            out[f"{name}/{mode}/g32_{i}"] = a.numpy()
            if i == 0:
                lo = (b - a.double()).float()
                assert rel(a.double() + lo.double(), b) < 1e-14
                out[f"{name}/{mode}/g64lo_0"] = lo.numpy()
            else:
                out[f"{name}/{mode}/g64_{i}"] = b.numpy()
    _, g32, g64 = res["eval"]
    print(f"{name}: train == eval {same}; e_ref = " + " ".join(f"{rel(a, b):.1e}" for a, b in zip(g32, g64)))


class Loop(nn.Module):
    def __init__(self, vq):
        super().__init__()
        self.enc, self.vq, self.dec = nn.Conv2d(3, 16, 1), vq, nn.Conv2d(16, 3, 1)

    def forward(self, x):
        q, idx, vq_loss = self.vq(self.enc(x))
        return self.dec(q), idx, vq_loss


def record_loop(out, vq_cls):
    torch.manual_seed(500)
    model = Loop(vq_cls(num_embeddings=64, embedding_dim=16, commitment_cost=CC, decay=DECAY, laplace_alpha=ALPHA, projection_dim=8))
    model.vq.first_pass.mul_(0)
    with torch.no_grad():
        model.vq.embed.mul_(0.5)
        model.vq.embed_avg.copy_(model.vq.embed)
        model.vq.cluster_size.fill_(2.0)
    gen = torch.Generator().manual_seed(501)
    x, target = grid((3, 2, 3, 8, 8), gen, 1 / 16), grid((3, 2, 3, 8, 8), gen, 1 / 16)
    lr = 0.05
    out["loop/x"], out["loop/target"], out["loop/lr"] = x.half().numpy(), target.half().numpy(), np.asarray(lr)
    for k, v in model.state_dict().items():
        out[f"loop/sd0/{k}"] = v.numpy().copy()
    runs = {}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        m = copy.deepcopy(model).to(dt).train()
        opt = torch.optim.SGD(m.parameters(), lr=lr)
        losses, idxs = [], []
        for step in range(3):
            rec, idx, vq_loss = m(x[step].to(dt))
            loss = torch.nn.functional.mse_loss(rec, target[step].to(dt)) + vq_loss
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss))
            idxs.append(idx.clone())
        runs[tag] = (losses, idxs, {k: v.detach().clone() for k, v in m.state_dict().items()})
    for step in range(3):
        assert torch.equal(runs["32"][1][step], runs["64"][1][step]), f"loop step {step}: fp32 and fp64 chose different indices"
    out["loop/idx"] = torch.stack(runs["32"][1]).numpy().astype(np.int16)
    out["loop/loss32"], out["loop/loss64"] = np.asarray(runs["32"][0], np.float32), np.asarray(runs["64"][0], np.float64)
    for tag in ("32", "64"):
        for k, v in runs[tag][2].items():
            out[f"loop/final{tag}/{k}"] = v.numpy()
    print("loop: losses", runs["64"][0], "e_ref(loss) =", [abs(a - b) / abs(b) for a, b in zip(runs["32"][0], runs["64"][0])])
    print("loop: e_ref(final) = " + " ".join(f"{k}:{rel(runs['32'][2][k], runs['64'][2][k]):.1e}" for k in runs["32"][2]
                                             if runs["64"][2][k].dim() > 0))
    print("loop: distinct codes per step", [int(i.unique().numel()) for i in runs["32"][1]])


def main():
    _ref_shims.install()
    from vq_ae.layers.vq import EMAVectorQuantizer, ProjectedEMAVectorQuantizer2d   # noqa: the reference, unmodified

    out = {"cases": np.array(list(PLAIN) + list(PROJ) + list(PROJ4) + list(PROJ16))}
    seed = 0
    for name, shape in PLAIN.items():
        seed += 1
        torch.manual_seed(100 + seed)
        m = EMAVectorQuantizer(num_embeddings=64, embedding_dim=shape[1], commitment_cost=CC, decay=DECAY, laplace_alpha=ALPHA)
        record_case(out, name, m, shape, seed)
    for cases, P, K in ((PROJ, 8, 256), (PROJ4, 4, 64), (PROJ16, 16, 64)):
        for name, shape in cases.items():
            seed += 1
            torch.manual_seed(100 + seed)
            m = ProjectedEMAVectorQuantizer2d(num_embeddings=K, embedding_dim=shape[1], commitment_cost=CC, decay=DECAY,
                                              laplace_alpha=ALPHA, projection_dim=P)
            with torch.no_grad():
                m.embed.mul_(0.6)                      # the scale of z = proj_in(x) under the default init: all codes in use
                m.embed_avg.copy_(m.embed)
                m.cluster_size.fill_(1.0)
            record_case(out, name, m, shape, seed)
    record_loop(out, ProjectedEMAVectorQuantizer2d)
    path = os.path.join(HERE, "vq_backward.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
