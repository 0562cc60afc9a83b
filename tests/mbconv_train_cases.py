"""Shared by tests/test_mbconv_train_cpu.py and tests/test_mbconv_train_gpu.py (and by the fixture's generator): reads
tests/golden/mbconv_train.npz (see tests/golden/make_mbconv_train_golden.py for its layout) and rebuilds the mirrors the
fixture's cases describe.

Distances are norm-wise, ||a - b64|| / ||b64|| in float64 (fixup_train_cases.dist), per tensor -- except that the tensors of
fewer than 8 elements of a case (the 3-channel BatchNorm of the 'out' block) form ONE vector, "small" for the parameter
gradients and "small_buffers" for the running statistics: the distance of a few fp32 numbers to their fp64 values is anywhere
between 0 and half an ulp by chance, so the fixture's own fp32 distance of such a tensor is no yardstick
(fixup_train_cases.py says the same of the one-element tensors).
"""
import functools

import torch

from conftest import load_golden
from fixup_train_cases import dist, names_of, sample, split  # noqa: F401  (re-exported)

SMALL = 8


@functools.lru_cache(maxsize=1)
def fixture():
    z = load_golden("mbconv_train")
    return {k: z[k] for k in z.files}


def grouped(by_name, small="small"):
    """{name: tensor} -> the comparison groups: tensors of at least SMALL elements by name, the others as one vector."""
    out = {k: v.reshape(-1) for k, v in by_name.items() if v.numel() >= SMALL}
    few = [v.reshape(-1) for v in by_name.values() if v.numel() < SMALL]
    if few:
        out[small] = torch.cat(few)
    return out


def result_groups(res, pnames, bnames):
    """{'out', 'input', <parameter>: its gradient, <buffer>: its value after the forward} -> the comparison groups."""
    out = {"out": res["out"].reshape(-1), "input": res["input"].reshape(-1)}
    out.update(grouped({k: res[k] for k in pnames}))
    out.update(grouped({k: res[k] for k in bnames}, "small_buffers"))
    return out


def block_kwargs():
    """The constructor keywords of an MBConv mirror besides (in_channels, out_channels, mode): mbconv.yaml as `tinyM` has it."""
    import vqae_amd
    from vqae_amd.model import default_confs
    conf = default_confs(vqae_amd.SPECS["tinyM"])["encoder_conf"]["conv_block_conf"]
    return {k: v for k, v in conf.items() if not k.startswith("_")}


def block_cases():
    return [str(c) for c in fixture()["cases"]]


def block_case(case, cls, device="cpu", dtype=torch.float32):
    """-> (block, x, g, ref): the mirror `cls` in train mode with the case's state dict, input and upstream gradient (NCHW, on
    device), and ref = {group: (fp64 value, e_ref)} over result_groups, e_ref the fixture's own fp32-to-fp64 distance."""
    z, pre = fixture(), f"block/{case}/"
    block = cls(int(z[pre + "cin"]), int(z[pre + "cout"]), str(z[pre + "mode"]), **block_kwargs())
    names, sizes = names_of(z, pre + "names"), z[pre + "sizes"]
    sd = split(names, sizes, z[pre + "sd"])
    shapes = {k: (v.shape, v.dtype) for k, v in block.state_dict().items()}
    assert list(shapes) == names, (list(shapes), names)
    block.load_state_dict({k: v.reshape(shapes[k][0]).to(shapes[k][1]) for k, v in sd.items()})
    block = block.to(device=device, dtype=dtype).train()
    x = torch.from_numpy(z[pre + "x"]).to(device=device, dtype=dtype)
    g = torch.from_numpy(z[pre + "g"]).to(device=device, dtype=dtype)
    pnames, bnames = names_of(z, pre + "pnames"), names_of(z, pre + "bnames")
    psizes = [int(n) for k, n in zip(names, sizes) if k in set(pnames)]
    bsizes = [int(n) for k, n in zip(names, sizes) if k in set(bnames)]

    def pair(key):
        a32 = torch.from_numpy(z[pre + key + "32"])
        return a32, a32.double() + torch.from_numpy(z[pre + key + "64lo"]).double()

    r32, r64 = {}, {}
    for name, key in (("out", "out"), ("input", "gin")):
        r32[name], r64[name] = pair(key)
    for key, ks, ns in (("gp", pnames, psizes), ("buf", bnames, bsizes)):
        a32, a64 = pair(key)
        r32.update(split(ks, ns, a32))
        r64.update(split(ks, ns, a64))
    g32, g64 = result_groups(r32, pnames, bnames), result_groups(r64, pnames, bnames)
    return block, x, g, {k: (g64[k], dist(g32[k], g64[k])) for k in g64}


def block_results(block, x, g, forward):
    """forward(block, x) and its gradients for upstream g, and the running statistics it leaves -> result_groups."""
    x = x.detach().clone().requires_grad_()
    params = dict(block.named_parameters())
    y = forward(block, x)
    grads = torch.autograd.grad(y, [x] + list(params.values()), g)
    res = {"out": y.detach(), "input": grads[0]}
    res.update(dict(zip(params, grads[1:])))
    bnames = [k for k in block.state_dict() if k.endswith(("running_mean", "running_var"))]
    res.update({k: block.state_dict()[k].detach().clone() for k in bnames})
    return result_groups(res, list(params), bnames)


def loop_model(device="cpu", dtype=torch.float32):
    """The closed loop's initial model (a vqae_amd.model.VQAE mirror of `tinyM` in train mode) and its three batches."""
    import vqae_amd
    from oracle import vqae_oracle as O
    from vqae_amd.model import VQAE
    z = fixture()
    spec = O.SPECS["tinyM"]
    p = O.calibrate_codebook(O.make_patches(2, 32, 99), O.make_params(spec, int(z["loop/seed"])), spec)
    model = VQAE.from_spec(vqae_amd.SPECS["tinyM"])
    vq = "encoder.vq_layers.0."
    full = dict(p)
    full[vq + "embed_avg"] = p[vq + "embed"].clone()
    full[vq + "cluster_size"] = torch.ones(spec.num_embeddings)
    full[vq + "first_pass"] = torch.as_tensor(0)
    for k in model.state_dict():
        if k.endswith("num_batches_tracked"):
            full[k] = torch.as_tensor(1)
    model.load_state_dict(full)
    model = model.to(device=device, dtype=dtype).train()
    batches = [O.make_patches(2, 32, int(b)).to(device=device, dtype=dtype) for b in z["loop/batch_nos"]]
    return model, batches


def loss_distances(losses):
    """[recon_0, vq_0, ..., recon_2, vq_2] of a run of the loop -> (its distance to the fp64 record, the fp32 record's own)."""
    z = fixture()
    r32 = torch.tensor([v for i in range(3) for v in (z["loop/recon32"][i], z["loop/vq32"][i])], dtype=torch.float64)
    r64 = torch.tensor([v for i in range(3) for v in (z["loop/recon64"][i], z["loop/vq64"][i])], dtype=torch.float64)
    return dist(torch.tensor(losses, dtype=torch.float64), r64), dist(r32, r64)


def loop_final_groups(model, sd0):
    """The loop's end state against the fixture -> {'params' | 'buffers': (this run's vector, the fp64 run's, e32)}: ALL
    parameters as one vector, the quantiser's and the BatchNorms' buffers as one (fixup_train_cases.loop_final_groups)."""
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


def closed_loop(amd, device="cpu"):
    """Run the fixture's three steps of train_mbconv.forward_train + Huber + torch.optim.AdamW on `device` -> (codes equal the
    fixture's at every step, the six losses, loop_final_groups)."""
    import torch.nn.functional as F
    z = fixture()
    model, batches = loop_model(device)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = torch.optim.AdamW(model.parameters(), lr=float(z["loop/lr"]))
    losses, same = [], []
    for i, x in enumerate(batches):
        x = x.contiguous(memory_format=torch.channels_last)
        out, vq_losses, (idx,) = amd.train_mbconv.forward_train(model, x, return_indices=True)
        recon = F.huber_loss(input=out, target=x)
        opt.zero_grad()
        (recon + sum(vq_losses)).backward()
        opt.step()
        same.append(bool(torch.equal(idx.cpu().to(torch.int16), torch.from_numpy(z["loop/idx"][i]))))
        losses += [float(recon.detach()), float(vq_losses[0].detach())]
    return same, losses, loop_final_groups(model, sd0)
