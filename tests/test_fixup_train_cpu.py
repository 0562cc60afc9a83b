"""CPU: the training path of the Fixup mirrors (vqae_amd.train) through its plain-torch restatements -- the same forward and
the same hand-derived backward the HIP kernels implement (tests/test_fixup_train_gpu.py runs those).

  * torch.autograd.gradcheck of each Function's restatement in fp64: the activation, the gather-fold of its circular halo, the plain mode, the output op, the bicubic adjoint with and without pre_bias;
  * block_forward / forward_train on CPU tensors against the reference's own fp32 and fp64 autograd
    (tests/golden/fixup_train.npz): distance to fp64 <= 4 x the fixture's own fp32-to-fp64 distance (the project's bar for
    code that sums the same products in another order), per tensor, the one-element tensors as one vector
    (tests/fixup_train_cases.py says why);
  * the closed loop of step() + torch.optim.AdamW reproduces the recorded codes exactly and the final state within the bar.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fixup_train_cases as C

BAR = 4.0


def _p(v):
    return torch.tensor([v], dtype=torch.float64, requires_grad=True)


SHAPES = [(1, 1, 1, 3), (2, 1, 2, 1), (1, 2, 1, 2), (2, 2, 3, 4), (1, 3, 3, 2)]


@pytest.mark.parametrize("shape", SHAPES)
def test_gradcheck_functions(amd, shape):
    T = amd.train
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, dtype=torch.float64, generator=gen, requires_grad=True)
    s = torch.randn(shape, dtype=torch.float64, generator=gen, requires_grad=True)
    for halo in (0, 1):
        assert torch.autograd.gradcheck(lambda x, a, b: T.fixup_act(x, a, b, halo), (x, _p(0.3), _p(-0.2)))
    assert torch.autograd.gradcheck(T.fixup_add, (x, _p(0.3)))
    assert torch.autograd.gradcheck(T.fixup_out, (x, s, _p(1.3), _p(0.1), _p(-0.4)))
    assert torch.autograd.gradcheck(T.fixup_out, (x, s, _p(0.7), _p(0.1)))
    assert torch.autograd.gradcheck(T.bicubic_up2, (x, _p(0.25)))
    assert torch.autograd.gradcheck(T.bicubic_up2, (x,))


@pytest.mark.parametrize("shape", SHAPES)
def test_restatements_are_the_torch_ops(amd, shape):
    """The halo is F.pad(circular) of the interior bit for bit; the bicubic restatement is F.interpolate to fp64 rounding."""
    T = amd.train
    x = torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    a, b = _p(0.3), _p(-0.2)
    y = T.fixup_act(x, a, b, 1)
    inner = T.fixup_act(x, a, b)
    assert torch.equal(inner, F.elu(x + a) + b)
    assert torch.equal(y, F.pad(inner.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="circular").permute(0, 2, 3, 1))
    up = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bicubic", align_corners=False).permute(0, 2, 3, 1)
    assert float((T.bicubic_up2(x) - up).abs().max()) <= 8 * 2.0 ** -52 * float(x.abs().max()) * 2.5
    assert float((T.bicubic_up2(x, _p(0.25)) - (T.bicubic_up2(x) + 0.25)).abs().max()) <= 1e-14


@pytest.mark.parametrize("n", range(1, 10))
def test_bicubic_window(amd, n):
    """Every output whose clamped taps reach input i lies in 2i-3 .. 2i+4 -- the window the gather kernel walks -- and no
    weight of an output that does reach i cancels to zero (the kernel skips zero weights); every row sums to 1."""
    a = amd.train.up2_matrix(n)
    for o in range(2 * n):
        odd = o & 1
        base = (o >> 1) - (1 if odd else 2)
        reached = {min(max(base + k, 0), n - 1) for k in range(4)}
        for i in range(n):
            assert (a[o, i] != 0) == (i in reached)
            if i in reached:
                assert 2 * i - 3 <= o <= 2 * i + 4
        assert float(a[o].sum()) == 1.0


@pytest.mark.parametrize("case", C.block_cases())
def test_block_forward_matches_reference(amd, case):
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    block, x, g, ref = C.block_case(case, PreActFixupResBlock)
    x = x.contiguous(memory_format=torch.channels_last)
    got = C.block_results(block, x, g, amd.train.block_forward)
    assert set(got) == set(ref)
    for k, (v64, e_ref) in ref.items():
        e = C.dist(got[k], v64.reshape(got[k].shape))
        print(f"{case} {k}: e {e:.2e} e_ref {e_ref:.2e}")
        assert e <= BAR * e_ref, (case, k, e, e_ref)
    # the stock-torch form of the same block (the GPU test's second yardstick) is the reference's arithmetic
    stock = C.block_results(block, x, g, amd.train.block_forward_torch)
    for k, (v64, e_ref) in ref.items():
        assert C.dist(stock[k], v64.reshape(stock[k].shape)) <= BAR * e_ref, (case, k)


def test_block_forward_fp64_and_module(amd):
    """In fp64 the CPU path is the reference to fp64 rounding (so the restated backward is the reference's, not merely close
    in fp32); the `_target_` subclass keeps the mirror's constructor and state dict and its forward is block_forward."""
    from vqae_amd.layers.conv_block import PreActFixupResBlock as Mirror
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    for case in C.block_cases():
        block, x, g, ref = C.block_case(case, PreActFixupResBlock, dtype=torch.float64)
        got = C.block_results(block, x, g, lambda b, t: b(t))
        for k, (v64, _) in ref.items():
            assert C.dist(got[k], v64.reshape(got[k].shape)) <= 1e-13, (case, k)
    m = Mirror(8, 16, "down")
    t = PreActFixupResBlock(8, 16, "down")
    assert list(m.state_dict()) == list(t.state_dict())
    t.load_state_dict(m.state_dict())
    x = torch.randn(1, 8, 4, 4, requires_grad=True)
    y = t(x)
    assert y.requires_grad and y.shape == (1, 16, 2, 2)
    assert torch.equal(y, amd.train.block_forward(m, x))


def test_model_mirrors_still_inference_only(amd):
    from vqae_amd.model import VQAE
    m = VQAE.from_spec(amd.SPECS["tiny"])
    x = torch.zeros(1, 3, 32, 32, requires_grad=True)
    with pytest.raises(NotImplementedError):
        m(x)
    with pytest.raises(NotImplementedError):
        m.decoder([torch.zeros(1, 32, 8, 8, requires_grad=True)])
    mb = VQAE.from_spec(amd.SPECS["tinyM"])
    with pytest.raises(NotImplementedError):
        amd.train.forward_train(mb, torch.zeros(1, 3, 32, 32))


def test_fixture_loop_records_agree():
    z = C.fixture()
    assert z["loop/idx"].shape == (3, 2, 8, 8) and z["loop/min_margin"].shape == (3,)
    assert float(z["loop/min_margin"].min()) >= 1e-3
    for k in ("recon", "vq"):
        assert np.all(np.abs(z[f"loop/{k}32"] - z[f"loop/{k}64"]) <= 1e-5 * np.abs(z[f"loop/{k}64"]))
    assert float(z["loop/final/e32_params"]) < 1e-6 and float(z["loop/final/e32_buffers"]) < 1e-6


def test_forward_train_first_step_matches_reference(amd):
    z = C.fixture()
    model, batches = C.loop_model()
    x = batches[0].contiguous(memory_format=torch.channels_last).requires_grad_()
    out, recon, (vq_loss,) = amd.train.step(model, x)
    (recon + vq_loss).backward()
    o32 = torch.from_numpy(z["loop/step0/out32"])
    o64 = o32.double() + torch.from_numpy(z["loop/step0/out64lo"]).double()
    assert C.dist(out.detach(), o64) <= BAR * C.dist(o32, o64)
    assert abs(float(recon) - z["loop/recon64"][0]) <= BAR * abs(z["loop/recon32"][0] - z["loop/recon64"][0]) + 1e-7 * z["loop/recon64"][0]
    names, sizes = C.names_of(z, "loop/step0/names"), z["loop/step0/sizes"]
    g32 = torch.from_numpy(z["loop/step0/g32"])
    g64 = g32.double() + torch.from_numpy(z["loop/step0/g64lo"]).double()
    params = dict(model.named_parameters())
    mine = {k: (x.grad if k == "input" else params[k].grad).reshape(-1) for k in names}
    got, r32, r64 = C.grouped(mine), C.grouped(C.split(names, sizes, g32)), C.grouped(C.split(names, sizes, g64))
    for k in r64:
        e, e_ref = C.dist(got[k], r64[k]), C.dist(r32[k], r64[k])
        print(f"step0 {k}: e {e:.2e} e_ref {e_ref:.2e}")
        assert e <= BAR * e_ref, (k, e, e_ref)


def test_closed_loop_reproduces_fixture(amd):
    """step() + torch.optim.AdamW for the fixture's three steps on the CPU: the recorded codes exactly, the six losses (one vector) and the final
    parameters (one vector) and quantiser buffers (one vector) within 4 x the fp32 reference run's own distance to the fp64 run."""
    z = C.fixture()
    model, batches = C.loop_model()
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = torch.optim.AdamW(model.parameters(), lr=float(z["loop/lr"]))
    losses = []
    for i, x in enumerate(batches):
        x = x.contiguous(memory_format=torch.channels_last)
        out, vq_losses, (idx,) = amd.train.forward_train(model, x, return_indices=True)
        recon = F.huber_loss(input=out, target=x)
        opt.zero_grad()
        (recon + sum(vq_losses)).backward()
        opt.step()
        assert torch.equal(idx.to(torch.int16), torch.from_numpy(z["loop/idx"][i])), f"step {i}: codes differ"
        losses += [float(recon), float(vq_losses[0])]
    e, e_ref = C.loss_distances(losses)
    print(f"loop losses: e {e:.2e} e_ref {e_ref:.2e}")
    assert e <= BAR * e_ref, (e, e_ref)
    for tag, (got, want, e32) in C.loop_final_groups(model, sd0).items():
        e = C.dist(got, want)
        print(f"loop final {tag}: e {e:.2e} e32 {e32:.2e}")
        assert e <= BAR * e32, (tag, e, e32)


def test_new_symbols_validate_before_any_launch(amd):
    """The error convention of the C ABI for the training entry points, without a GPU (validation precedes every HIP call)."""
    import ctypes
    L = amd._lib
    lib = L.lib()
    one = ctypes.c_void_p(16)
    assert lib.vqae_fixup_train_workspace_bytes(1) >= 16 + 256
    assert lib.vqae_fixup_train_workspace_bytes(1 << 30) == lib.vqae_fixup_train_workspace_bytes(1 << 20)
    with pytest.raises(AssertionError):
        L.check(lib.vqae_fixup_act_f32(None, one, one, 1, 0, 1, 2, 2, 4, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_fixup_act_f32(one, one, one, 1, 0, 1, 0, 2, 4, one, None))
    with pytest.raises(NotImplementedError):          # the plain mode has no halo form
        L.check(lib.vqae_fixup_act_f32(one, None, one, 0, 1, 1, 2, 2, 4, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_fixup_act_backward_f32(one, None, one, 1, 1, 1, 2, 2, 4, one, one, one, one, None))   # no x
    with pytest.raises(AssertionError):
        L.check(lib.vqae_fixup_out_f32(one, None, one, one, None, 16, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_fixup_out_backward_f32(one, one, one, 0, one, one, one, None, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_bicubic_up2_bias_f32(one, 1, 2, 2, 4, None, None, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_bicubic_up2_backward_f32(one, 1, 2, 2, 4, one, None, None, None))
    with pytest.raises(amd._lib.VqaeHipError):
        amd.ops.fixup_act(torch.zeros(1, 2, 2, 4), torch.zeros(1), torch.zeros(1))
