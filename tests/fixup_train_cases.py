"""Shared by tests/test_fixup_train_cpu.py and tests/test_fixup_train_gpu.py: reads tests/golden/fixup_train.npz (see
tests/golden/make_fixup_train_golden.py for its layout) and rebuilds the mirrors the fixture's cases describe.

Distances are norm-wise, ||a - b64|| / ||b64|| in float64.  They are taken per tensor, except that the one-element tensors
of a case (bias1a .. bias4, scale, bias1c / bias1d) form ONE vector, "scalars", in state-dict order: the distance of a single
fp32 number to its fp64 value is anywhere between 0 and half an ulp by chance, so the fixture's own fp32 distance of a
one-element tensor is no yardstick (same_8_1x1's bias1b: 3.6e-10), while that of the vector of all of them is.
"""
import functools

import numpy as np
import torch

from conftest import load_golden


@functools.lru_cache(maxsize=1)
def fixture():
    z = load_golden("fixup_train")
    return {k: z[k] for k in z.files}


def names_of(z, key):
    return z[key].item().decode().split("\n")


def dist(a, b64):
    a, b64 = torch.as_tensor(a).double().cpu(), torch.as_tensor(b64).double().cpu()
    return float((a - b64).norm() / b64.norm())


def split(names, sizes, flat):
    """flat concatenation -> {name: flat tensor}."""
    out, o = {}, 0
    flat = torch.as_tensor(flat)
    for k, n in zip(names, sizes):
        out[k] = flat[o:o + int(n)]
        o += int(n)
    assert o == flat.numel()
    return out


def grouped(by_name):
    """{name: tensor} -> the comparison groups: multi-element tensors by name, the one-element ones as 'scalars'."""
    out = {k: v.reshape(-1) for k, v in by_name.items() if v.numel() > 1}
    ones = [v.reshape(-1) for v in by_name.values() if v.numel() == 1]
    if ones:
        out["scalars"] = torch.cat(ones)
    return out


def block_cases():
    return [str(c) for c in fixture()["cases"]]


def block_case(case, cls, device="cpu", dtype=torch.float32):
    """-> (block, x, g, ref): the mirror `cls` with the case's state dict, input and upstream gradient (NCHW, on device), and
    ref = {'out' | 'input' | <param group>: (fp64 value, e_ref)}, e_ref the fixture's own fp32-to-fp64 distance."""
    z, pre = fixture(), f"block/{case}/"
    block = cls(int(z[pre + "cin"]), int(z[pre + "cout"]), str(z[pre + "mode"]))
    names, sizes = names_of(z, pre + "names"), z[pre + "sizes"]
    sd = split(names, sizes, z[pre + "sd"])
    shapes = {k: v.shape for k, v in block.state_dict().items()}
    assert list(shapes) == names, (list(shapes), names)
    block.load_state_dict({k: v.reshape(shapes[k]) for k, v in sd.items()})
    block = block.to(device=device, dtype=dtype)
    x = torch.from_numpy(z[pre + "x"]).to(device=device, dtype=dtype)
    g = torch.from_numpy(z[pre + "g"]).to(device=device, dtype=dtype)

    def pair(key):
        a32 = torch.from_numpy(z[pre + key + "32"])
        return a32, a32.double() + torch.from_numpy(z[pre + key + "64lo"]).double()

    ref = {}
    for name, key in (("out", "out"), ("input", "gin")):
        a32, a64 = pair(key)
        ref[name] = (a64, dist(a32, a64))
    p32, p64 = pair("gp")
    g32, g64 = grouped(split(names, sizes, p32)), grouped(split(names, sizes, p64))
    for k in g64:
        ref[k] = (g64[k], dist(g32[k], g64[k]))
    return block, x, g, ref


def block_results(block, x, g, forward):
    """forward(block, x) and its gradients for upstream g -> {'out' | 'input' | <param group>: tensor} (the groups of `grouped`)."""
    x = x.detach().clone().requires_grad_()
    params = dict(block.named_parameters())
    y = forward(block, x)
    grads = torch.autograd.grad(y, [x] + list(params.values()), g)
    res = {"out": y.detach(), "input": grads[0]}
    res.update(grouped(dict(zip(params, grads[1:]))))
    return res


def loop_model(device="cpu", dtype=torch.float32):
    """The closed loop's initial model (a vqae_amd.model.VQAE mirror in train mode) and its three batches."""
    import vqae_amd
    from oracle import vqae_oracle as O
    from vqae_amd.model import VQAE
    z = fixture()
    spec = O.SPECS["tiny"]
    p = O.calibrate_codebook(O.make_patches(2, 32, 99), O.make_params(spec, int(z["loop/seed"])), spec)
    model = VQAE.from_spec(vqae_amd.SPECS["tiny"])
    vq = "encoder.vq_layers.0."
    full = dict(p)
    full[vq + "embed_avg"] = p[vq + "embed"].clone()
    full[vq + "cluster_size"] = torch.ones(spec.num_embeddings)
    full[vq + "first_pass"] = torch.as_tensor(0)
    model.load_state_dict(full)
    model = model.to(device=device, dtype=dtype).train()
    batches = [O.make_patches(2, 32, int(b)).to(device=device, dtype=dtype) for b in z["loop/batch_nos"]]
    return model, batches


def loss_distances(losses):
    """[recon_0, vq_0, recon_1, vq_1, recon_2, vq_2] of a run of the loop -> (its distance to the fp64 record, the fp32
    record's own): the six numbers as one vector, for the reason the one-element tensors are one."""
    z = fixture()
    r32 = torch.tensor([v for i in range(3) for v in (z["loop/recon32"][i], z["loop/vq32"][i])], dtype=torch.float64)
    r64 = torch.tensor([v for i in range(3) for v in (z["loop/recon64"][i], z["loop/vq64"][i])], dtype=torch.float64)
    return dist(torch.tensor(losses, dtype=torch.float64), r64), dist(r32, r64)


def sample(v):
    """make_fixup_train_golden.sample: what the fixture stores of a final tensor."""
    v = v.reshape(-1)
    return v if v.numel() <= 256 else v[::8]


def loop_final_groups(model, sd0):
    """The loop's end state against the fixture -> {'params' | 'buffers': (this run's vector, the fp64 run's, e32)}: ALL
    parameters as one vector and the quantiser's buffers as one (make_fixup_train_golden.py says why: AdamW makes a single
    tensor's distance a matter of chance).  The fp64 vector is initial + the stored fp64 update, so the fp32 rounding of the
    stored update (~1e-9 of the value) is all the storage adds."""
    z = fixture()
    names, sizes = names_of(z, "loop/final/names"), z["loop/final/sizes"]
    d64 = split(names, sizes, z["loop/final/d64"])
    now = model.state_dict()
    pnames = {k for k, _ in model.named_parameters()}
    out = {}
    for tag, keep in (("params", lambda k: k in pnames), ("buffers", lambda k: k not in pnames)):
        ks = [k for k in names if keep(k)]
        got = torch.cat([sample(now[k].detach().double().cpu()) for k in ks])
        want = torch.cat([sample(sd0[k].double().cpu()) + d64[k].double() for k in ks])
        out[tag] = (got, want, float(z["loop/final/e32_" + tag]))
    return out
