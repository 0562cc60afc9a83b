#!/usr/bin/env python3
"""Generate tests/golden/fixup_train.npz: outputs and gradients of the reference's PreActFixupResBlock and of its VQAE.step,
from the reference's own autograd, once in fp32 and once in fp64 on the CPU.

Build container only: imports the unmodified reference (vq_ae/layers/conv_block.py, vq_ae/model.py) through _ref_shims.

(a) Block cases: one block each, batch 2.  The one-element parameters are drawn non-zero (scale != 1) and branch_conv3 is
    re-drawn non-zero (its zero init hides every gradient behind it).
        same_8_4x6, same_8_1x1, same_8_2x2, sameskip_8_16_3x5, down_8_16_4x6, up_16_8_3x5, up_16_8_1x2, outskip_8_3_4x4
    block/<case>/mode, cin, cout          the constructor arguments
    block/<case>/x, g                     input [2, cin, H, W] and upstream gradient (shape of the output), float32
    block/<case>/names, sizes, sd         the state dict: parameter names (one bytes string, newline-separated), their element
                                          counts, and the tensors flat and concatenated in that order
    block/<case>/out32, out64lo           the output of the fp32 run, and float32(fp64 run - fp32 run): the fp64 result is
                                          out32 + out64lo in float64 (put64 below)
    block/<case>/gin32, gin64lo           the input gradient, stored the same way
    block/<case>/gp32, gp64lo             the parameter gradients, flat and concatenated in the order of `names`

(b) Closed loop: spec `tiny`, three steps of VQAE.step (Huber) + torch.optim.AdamW(lr 1e-3) in train mode (the quantiser's
    EMA runs, first_pass = 0) on three batches of 2 x 3 x 32 x 32.  The initial state is oracle.make_params(tiny, SEED) with
    the codebook calibrated on oracle.make_patches(2, 32, 99), embed_avg = embed, cluster_size = 1 -- generated, not stored.
    The generator ASSERTS that the fp32 and the fp64 run choose identical codes at every step and that every row's
    best-to-second distance margin is >= 1e-3 relative in both runs; SEED (the first that passes, searched on the CPU) is
    recorded.
    loop/seed, lr, batch_nos              SEED, the learning rate, the make_patches batch numbers of the three steps
    loop/idx [3, 2, 8, 8] int16           the codes of every step (equal in both runs)
    loop/min_margin [3]                   the smallest relative margin of each step (the smaller of the two runs)
    loop/recon32, recon64, vq32, vq64 [3] the two losses of every step
    loop/step0/out32, out64lo             the output of the first forward
    loop/step0/names, sizes, g32, g64lo   (names: one bytes string, newline-separated) the first backward of recon + vq loss, the tensors flat and concatenated in the
                                          order of `names`: input, then every parameter of at most 64 elements (every Fixup
                                          scalar, the stems' biases)
    loop/final/names, sizes               parameters and the quantiser's buffers after step 3; of a tensor above 256
                                          elements every eighth element (flat order) is stored: sample() below
    loop/final/d64                        float32(final - initial) of the fp64 run, concatenated (the update is ~1e-2 of the
                                          value, so its fp32 rounding is ~1e-9 of the value)
    loop/final/e32                        |final32 - final64| / |final64| per tensor: the fp32 run's own distance
    loop/final/e32_params, e32_buffers    the same for ALL parameters as one vector, and for the quantiser's buffers as one.
                                          AdamW divides by sqrt(v) + eps: an element whose gradient nearly cancels moves by up
                                          to lr whatever its size, and WHICH elements those are differs between any two fp32
                                          summation orders -- a single tensor's distance is chance (the per-tensor e32 spans
                                          7e-8 .. 2.6e-6), the whole vector's is not.  Tests compare the whole vectors.

    python tests/golden/make_fixup_train_golden.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import _ref_shims  # noqa: E402

CASES = {                                  # name: (mode, cin, cout, H, W)
    "same_8_4x6": ("same", 8, 8, 4, 6),
    "same_8_1x1": ("same", 8, 8, 1, 1),
    "same_8_2x2": ("same", 8, 8, 2, 2),
    "sameskip_8_16_3x5": ("same", 8, 16, 3, 5),
    "down_8_16_4x6": ("down", 8, 16, 4, 6),
    "up_16_8_3x5": ("up", 16, 8, 3, 5),
    "up_16_8_1x2": ("up", 16, 8, 1, 2),
    "outskip_8_3_4x4": ("out", 8, 3, 4, 4),
}
LR, MARGIN = 1e-3, 1e-3


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def put64(out, key, a32, a64, suffix=""):
    """<key>32<suffix> = the fp32 result, <key>64lo<suffix> = float32(fp64 result - fp32 result): the fp64 result is their sum
    in float64 (48 bits, asserted < 1e-12 relative: 2^-24 of the fp32 run's own distance) at two thirds of the bytes."""
    lo = (a64 - a32.double()).float()
    assert rel(a32.double() + lo.double(), a64) < 1e-12, key
    out[key + "32" + suffix], out[key + "64lo" + suffix] = a32.numpy(), lo.numpy()


def sample(v):
    """What is stored of a final tensor: all of it up to 256 elements, every eighth element (flat order) above."""
    v = v.reshape(-1)
    return v if v.numel() <= 256 else v[::8]


def record_block(out, name, seed):
    mode, cin, cout, H, W = CASES[name]
    torch.manual_seed(seed)
    block = _ref_shims.instantiate(_ref_shims.fixup_conf(8), in_channels=cin, out_channels=cout, mode=mode)
    gen = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for k, p in block.named_parameters():
            if p.numel() == 1:
                sign = 1.0 if torch.rand((), generator=gen) < 0.5 else -1.0
                p.fill_(sign * float(0.05 + 0.25 * torch.rand((), generator=gen)))
        block.scale.fill_(float(0.7 + 0.2 * torch.rand((), generator=gen)))
        w3 = block.branch_conv3.weight
        w3.copy_(torch.randn(w3.shape, generator=gen) * (0.5 / w3.shape[1] ** 0.5))
    x = torch.randn((2, cin, H, W), generator=gen)
    pre = f"block/{name}/"
    out[pre + "mode"], out[pre + "cin"], out[pre + "cout"] = np.array(mode), np.asarray(cin), np.asarray(cout)
    pnames = [k for k, _ in block.named_parameters()]
    assert pnames == list(block.state_dict())
    out[pre + "names"] = np.array("\n".join(pnames).encode())
    out[pre + "sizes"] = np.asarray([p.numel() for p in block.parameters()])
    out[pre + "sd"] = torch.cat([p.detach().reshape(-1) for p in block.parameters()]).numpy()
    res = {}
    g = None
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        m = copy.deepcopy(block).to(dt)
        xi = x.clone().to(dt).requires_grad_()
        y = m(xi)
        if g is None:
            g = torch.randn(y.shape, generator=gen)
        names = ["input"] + [k for k, _ in m.named_parameters()]
        grads = torch.autograd.grad(y, [xi] + [p for _, p in m.named_parameters()], g.to(dt))
        res[tag] = (y.detach(), dict(zip(names, grads)))
    put64(out, pre + "out", res["32"][0], res["64"][0])
    put64(out, pre + "gin", res["32"][1]["input"], res["64"][1]["input"])
    put64(out, pre + "gp", torch.cat([res["32"][1][k].reshape(-1) for k in pnames]),
          torch.cat([res["64"][1][k].reshape(-1) for k in pnames]))
    out[pre + "x"], out[pre + "g"] = x.numpy(), g.numpy()
    assert all(float(v.abs().max()) > 0 for v in res["64"][1].values()), name
    print(f"{name}: e_ref out {rel(res['32'][0], res['64'][0]):.1e} | " +
          " ".join(f"{k}:{rel(res['32'][1][k], res['64'][1][k]):.1e}" for k in res["32"][1]))


def margins(flat, embed):
    d = torch.cdist(flat.double(), embed.double(), 4, compute_mode="donot_use_mm_for_euclid_dist")
    two = torch.topk(d, 2, dim=1, largest=False).values
    return (two[:, 1] - two[:, 0]) / two[:, 0]


def run_loop(O, spec, seed, batch_nos, dt):
    p = O.calibrate_codebook(O.make_patches(2, 32, 99), O.make_params(spec, seed), spec)
    model = _ref_shims.build_reference_model(spec, p).to(dt).train()
    vq = model.encoder.vq_layers[0]
    with torch.no_grad():                                  # a codebook in use: m_i = e_i, N_i = 1 (first_pass = 0)
        vq.embed_avg.copy_(vq.embed)
        vq.cluster_size.fill_(1.0)
    rec = dict(idx=[], recon=[], vq=[], margin=[])
    vq.register_forward_pre_hook(lambda m, inp: rec["margin"].append(float(margins(
        inp[0].detach().permute(0, 2, 3, 1).reshape(-1, m.embedding_dim), m.embed).min())))
    vq.register_forward_hook(lambda m, inp, res: rec["idx"].append(res[1].clone()))
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = torch.optim.AdamW(model.parameters(), lr=LR)
    for step, bn in enumerate(batch_nos):
        x = O.make_patches(2, 32, bn).to(dt)
        if step == 0:
            x.requires_grad_()                             # the input gradient of VQAE.step: through `input` and `target`
        y, recon, enc_loss = model.step(x)
        opt.zero_grad()
        (recon + sum(enc_loss)).backward()
        if step == 0:
            rec["out0"] = y.detach().clone()
            rec["g0"] = {"input": x.grad.detach().clone()}
            rec["g0"].update({k: q.grad.detach().clone() for k, q in model.named_parameters() if q.numel() <= 64})
        opt.step()
        rec["recon"].append(float(recon))
        rec["vq"].append(float(enc_loss[0]))
    rec["sd0"], rec["final"] = sd0, {k: v.detach().clone() for k, v in model.state_dict().items()}
    return rec


def record_loop(out):
    from oracle import vqae_oracle as O
    spec = O.SPECS["tiny"]
    for seed in range(39, 64):                    # 0 .. 38 were searched and fail the margin
        batch_nos = [200 + 3 * seed + i for i in range(3)]
        r32 = run_loop(O, spec, seed, batch_nos, torch.float32)
        r64 = run_loop(O, spec, seed, batch_nos, torch.float64)
        same = all(torch.equal(a, b) for a, b in zip(r32["idx"], r64["idx"]))
        mm = [min(a, b) for a, b in zip(r32["margin"], r64["margin"])]
        print(f"seed {seed}: same codes {same}, min margins {['%.1e' % m for m in mm]}")
        if same and min(mm) >= MARGIN:
            break
    else:
        raise SystemExit("no seed with identical codes and margins >= 1e-3")
    assert same and min(mm) >= MARGIN
    out["loop/seed"], out["loop/lr"], out["loop/batch_nos"] = np.asarray(seed), np.asarray(LR), np.asarray(batch_nos)
    out["loop/idx"] = torch.stack(r32["idx"]).numpy().astype(np.int16)
    out["loop/min_margin"] = np.asarray(mm)
    for tag, r in (("32", r32), ("64", r64)):
        out["loop/recon" + tag], out["loop/vq" + tag] = np.asarray(r["recon"]), np.asarray(r["vq"])
    put64(out, "loop/step0/out", r32["out0"], r64["out0"])
    gnames = list(r32["g0"])
    out["loop/step0/names"] = np.array("\n".join(gnames).encode())
    out["loop/step0/sizes"] = np.asarray([r32["g0"][k].numel() for k in gnames])
    put64(out, "loop/step0/g", torch.cat([r32["g0"][k].reshape(-1) for k in gnames]),
          torch.cat([r64["g0"][k].reshape(-1) for k in gnames]))
    fnames = [k for k, v in r64["final"].items() if v.dim() > 0]            # all but first_pass
    out["loop/final/names"] = np.array("\n".join(fnames).encode())
    out["loop/final/sizes"] = np.asarray([sample(r64["final"][k]).numel() for k in fnames])
    out["loop/final/d64"] = torch.cat([sample(r64["final"][k] - r64["sd0"][k]).float() for k in fnames]).numpy()
    out["loop/final/e32"] = np.asarray([rel(sample(r32["final"][k]), sample(r64["final"][k])) for k in fnames])
    pnames = {k for k, _ in _ref_shims.build_reference_model(spec, O.make_params(spec, seed)).named_parameters()}
    for tag, keep in (("params", lambda k: k in pnames), ("buffers", lambda k: k not in pnames)):
        ks = [k for k in fnames if keep(k)]
        out["loop/final/e32_" + tag] = np.asarray(rel(torch.cat([sample(r32["final"][k]) for k in ks]),
                                                      torch.cat([sample(r64["final"][k]) for k in ks])))
        print("loop: e32", tag, float(out["loop/final/e32_" + tag]))
    print("loop: recon", r64["recon"], "vq", r64["vq"], "codes used", [int(i.unique().numel()) for i in r32["idx"]])
    print("loop: e32 max", float(out["loop/final/e32"].max()), "median", float(np.median(out["loop/final/e32"])))


def main():
    _ref_shims.install()
    out = {"cases": np.array(list(CASES))}
    for i, name in enumerate(CASES):
        record_block(out, name, 700 + i)
    record_loop(out)
    path = os.path.join(HERE, "fixup_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 350000


if __name__ == "__main__":
    main()
