#!/usr/bin/env python3
"""Generate tests/golden/mbconv_train.npz: outputs, gradients and BatchNorm buffers of the reference's MBConv in train mode and of
its VQAE.step on the MBConv spec `tinyM`, from the reference's own autograd, once in fp32 and once in fp64 on the CPU.

Build container only: imports the unmodified reference (vq_ae/layers/conv_block.py, vq_ae/layers/misc.py, vq_ae/model.py)
through _ref_shims (mbconv_conf(SPECS["tinyM"])).  Layout and put64 storage are those of fixup_train.npz
(make_fixup_train_golden.py).

(a) Block cases: one block each in TRAIN mode (batch statistics, running-statistics update).  Every BatchNorm weight and bias
    is drawn non-zero -- the last BatchNorm's gamma included, whose zero init (conv_block.py:312-314) hides every gradient behind
    it -- and the running statistics are drawn non-trivial.
        same_8_4x6 (batch 2), same_8_1x2 (batch 4: H = 1, all three rows of the circular 3x3 wrap onto one), sameskip_8_16_3x5,
        down_8_16_4x6, up_16_8_3x5, up_16_8_1x2 (batch 4), outskip_8_3_4x4 (the 3-channel last BatchNorm)
    block/<case>/mode, cin, cout          the constructor arguments
    block/<case>/x, g                     input [B, cin, H, W] and upstream gradient (shape of the output), float32
    block/<case>/names, sizes, sd         the state dict BEFORE the forward: names (one bytes string, newline-separated), element
                                          counts, and the tensors flat and concatenated in that order, float32
                                          (num_batches_tracked as a float)
    block/<case>/pnames                   the parameters among `names`, in order
    block/<case>/out32, out64lo           the output of the fp32 run, and float32(fp64 run - fp32 run) (put64)
    block/<case>/gin32, gin64lo           the input gradient
    block/<case>/gp32, gp64lo             the parameter gradients, flat and concatenated in the order of `pnames`
    block/<case>/bnames, buf32, buf64lo   the six running-statistic buffers AFTER the forward, concatenated in the order of `bnames`
    The generator ASSERTS that every BatchNorm sees M >= 8 rows and that the reference's own fp32-to-fp64 distance of every
    stored group (mbconv_train_cases.grouped) is <= 1e-5: at M = 2 the normalised values are +-1 and the reference's own fp32
    weight gradient is 4.6e-5 from fp64, no yardstick for anything.

(b) Closed loop: spec `tinyM`, three steps of VQAE.step (Huber) + torch.optim.AdamW(lr 1e-3) in train mode on three batches of
    2 x 3 x 32 x 32, recorded exactly as fixup_train's loop: seed search, identical codes in the fp32 and the fp64 run, every
    row's best-to-second margin >= 1e-3.  The BatchNorm buffers join the quantiser's in the `buffers` vector.
    loop/seed, lr, batch_nos, idx, min_margin, recon32/64, vq32/64, step0/*, final/*    as in fixup_train.npz; step0's gradients
    are the input's and those of every parameter of at most 64 elements.

    python tests/golden/make_mbconv_train_golden.py
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ref_shims  # noqa: E402
from make_fixup_train_golden import margins, put64, rel, sample  # noqa: E402

CASES = {                                  # name: (mode, cin, cout, H, W, batch)
    "same_8_4x6": ("same", 8, 8, 4, 6, 2),
    "same_8_1x2": ("same", 8, 8, 1, 2, 4),
    "sameskip_8_16_3x5": ("same", 8, 16, 3, 5, 2),
    "down_8_16_4x6": ("down", 8, 16, 4, 6, 2),
    "up_16_8_3x5": ("up", 16, 8, 3, 5, 2),
    "up_16_8_1x2": ("up", 16, 8, 1, 2, 4),
    "outskip_8_3_4x4": ("out", 8, 3, 4, 4, 2),
}
LR, MARGIN, E_REF_MAX, MIN_ROWS = 1e-3, 1e-3, 1e-5, 8


def record_block(out, name, seed, spec):
    mode, cin, cout, H, W, B = CASES[name]
    torch.manual_seed(seed)
    block = _ref_shims.instantiate(_ref_shims.mbconv_conf(spec), in_channels=cin, out_channels=cout, mode=mode).train()
    gen = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in block.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
                m.weight.copy_(sign * (0.5 + torch.rand(n, generator=gen)))
                m.bias.copy_(0.4 * torch.rand(n, generator=gen) - 0.2)
                m.running_mean.copy_(0.3 * torch.randn(n, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(n, generator=gen))
                m.register_forward_pre_hook(lambda mod, inp: rows.append(inp[0].numel() // inp[0].shape[1]))
    rows = []
    x = torch.randn((B, cin, H, W), generator=gen)
    pre = f"block/{name}/"
    out[pre + "mode"], out[pre + "cin"], out[pre + "cout"] = np.array(mode), np.asarray(cin), np.asarray(cout)
    sd = block.state_dict()
    pnames = [k for k, _ in block.named_parameters()]
    bnames = [k for k in sd if k.endswith(("running_mean", "running_var"))]
    assert len(bnames) == 6
    out[pre + "names"] = np.array("\n".join(sd).encode())
    out[pre + "pnames"] = np.array("\n".join(pnames).encode())
    out[pre + "bnames"] = np.array("\n".join(bnames).encode())
    out[pre + "sizes"] = np.asarray([v.numel() for v in sd.values()])
    out[pre + "sd"] = torch.cat([v.detach().reshape(-1).float() for v in sd.values()]).numpy()
    res = {}
    g = None
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        m = copy.deepcopy(block).to(dt).train()
        xi = x.clone().to(dt).requires_grad_()
        y = m(xi)
        if g is None:
            g = torch.randn(y.shape, generator=gen)
        params = dict(m.named_parameters())
        grads = torch.autograd.grad(y, [xi] + [params[k] for k in pnames], g.to(dt))
        bufs = m.state_dict()
        res[tag] = dict(out=y.detach(), input=grads[0], **dict(zip(pnames, grads[1:])), **{k: bufs[k].clone() for k in bnames})
    assert len(rows) == 6 and min(rows) >= MIN_ROWS, (name, rows)
    put64(out, pre + "out", res["32"]["out"], res["64"]["out"])
    put64(out, pre + "gin", res["32"]["input"], res["64"]["input"])
    put64(out, pre + "gp", torch.cat([res["32"][k].reshape(-1) for k in pnames]),
          torch.cat([res["64"][k].reshape(-1) for k in pnames]))
    put64(out, pre + "buf", torch.cat([res["32"][k].reshape(-1) for k in bnames]),
          torch.cat([res["64"][k].reshape(-1) for k in bnames]))
    out[pre + "x"], out[pre + "g"] = x.numpy(), g.numpy()
    assert all(float(res["64"][k].abs().max()) > 0 for k in pnames), name
    from mbconv_train_cases import result_groups
    g32, g64 = (result_groups(res[t], pnames, bnames) for t in ("32", "64"))
    e = {k: rel(g32[k], g64[k]) for k in g64}
    print(f"{name}: rows {min(rows)} e_ref max {max(e.values()):.1e} min {min(e.values()):.1e}")
    assert max(e.values()) <= E_REF_MAX, (name, e)


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
            x.requires_grad_()
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


def record_loop(out, spec_name="tinyM"):
    from oracle import vqae_oracle as O
    spec = O.SPECS[spec_name]
    for seed in range(63, 128):                   # 0 .. 62 were searched and fail the margin
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
    fnames = [k for k, v in r64["final"].items() if v.dim() > 0]            # all but first_pass and num_batches_tracked
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


def main():
    _ref_shims.install()
    from oracle import vqae_oracle as O
    out = {"cases": np.array(list(CASES))}
    for i, name in enumerate(CASES):
        record_block(out, name, 900 + i, O.SPECS["tinyM"])
    record_loop(out)
    path = os.path.join(HERE, "mbconv_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 700000            # tinyM has four times tiny's block parameters (expand_ratio 4)


if __name__ == "__main__":
    main()
