"""CPU: the training path of the MBConv mirrors (vqae_amd.train_mbconv) through its plain-torch restatements -- the same forward
and the same hand-derived backward the HIP kernels implement (tests/test_mbconv_train_gpu.py runs those).

  * torch.autograd.gradcheck of each Function's restatement in fp64: bn_act in train and eval mode, with and without SiLU and
    the pooled output; dwconv in its three modes (H = 1, W = 1 included); se_scale;
  * block_forward / forward_train on CPU tensors against the reference's own fp32 and fp64 autograd in train mode
    (tests/golden/mbconv_train.npz): distance to fp64 <= 4 x the fixture's own fp32-to-fp64 distance, per tensor group
    (tests/mbconv_train_cases.py), the running statistics after the forward included;
  * the closed loop of forward_train + torch.optim.AdamW reproduces the recorded codes exactly and the final state within the bar;
  * the C ABI of csrc/mbconv_train.hip validates its arguments before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mbconv_train_cases as C

BAR = 4.0


def _bn(c, train, seed=0):
    gen = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(c).double()
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(c, generator=gen, dtype=torch.float64))
        bn.bias.copy_(torch.randn(c, generator=gen, dtype=torch.float64) * 0.3)
        bn.running_mean.copy_(torch.randn(c, generator=gen, dtype=torch.float64) * 0.3)
        bn.running_var.copy_(0.5 + torch.rand(c, generator=gen, dtype=torch.float64))
    return bn.train(train)


@pytest.mark.parametrize("shape", [(2, 1, 2, 3), (2, 2, 3, 4), (3, 3, 1, 2)])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("silu", [False, True])
def test_gradcheck_bn_act(amd, shape, train, silu):
    T = amd.train_mbconv
    bn = _bn(shape[-1], train)
    x = torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(sum(shape)), requires_grad=True)
    mix = torch.randn(shape[0], shape[-1], dtype=torch.float64, generator=torch.Generator().manual_seed(7))

    def plain(x, w, b):
        return T._BnActFn.apply(x, w, b, bn.running_mean, bn.running_var, train, bn.momentum, bn.eps, silu, False)[0]

    def pooled(x, w, b):
        y, pool = T._BnActFn.apply(x, w, b, bn.running_mean, bn.running_var, train, bn.momentum, bn.eps, silu, True)
        return y, pool * mix

    w, b = bn.weight.detach().clone().requires_grad_(), bn.bias.detach().clone().requires_grad_()
    assert torch.autograd.gradcheck(plain, (x, w, b))
    assert torch.autograd.gradcheck(pooled, (x, w, b))


def test_bn_act_is_torch_batch_norm(amd):
    """The restatement is F.batch_norm (+ F.silu) to fp64 rounding, buffers and num_batches_tracked included; eval mode writes
    nothing; one row in training mode and momentum=None raise as specified."""
    T = amd.train_mbconv
    for train in (True, False):
        a, b = _bn(6, train, 3), _bn(6, train, 3)
        x = torch.randn(3, 2, 5, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        before = {k: v.clone() for k, v in a.state_dict().items()}
        y, pool = T.bn_act(x, a, silu=True, want_pool=True)
        want = F.silu(b(x.permute(0, 3, 1, 2))).permute(0, 2, 3, 1)
        assert float((y - want).detach().abs().max()) <= 1e-14
        assert float((pool - want.sum((1, 2))).detach().abs().max()) <= 1e-13
        for k, v in a.state_dict().items():
            assert float((v.double() - b.state_dict()[k].double()).abs().max()) <= 1e-15, k
            assert train or torch.equal(v, before[k]), k
        assert int(a.num_batches_tracked) == (1 if train else 0)
    with pytest.raises(ValueError):
        T.bn_act(torch.zeros(1, 1, 1, 4, dtype=torch.float64), _bn(4, True))
    T.bn_act(torch.zeros(1, 1, 1, 4, dtype=torch.float64), _bn(4, False))          # eval mode takes one row
    cumulative = torch.nn.BatchNorm2d(4, momentum=None).double()
    with pytest.raises(NotImplementedError):
        T.bn_act(torch.zeros(2, 1, 1, 4, dtype=torch.float64), cumulative)


DW_SHAPES = {"same": [(2, 1, 1, 2), (1, 1, 3, 2), (2, 3, 1, 1), (1, 2, 2, 3), (1, 3, 4, 2)],
             "down": [(2, 2, 2, 2), (1, 4, 2, 3), (1, 2, 6, 1)],
             "up": [(2, 1, 1, 2), (1, 2, 3, 2), (1, 3, 1, 1)]}


@pytest.mark.parametrize("mode", ["same", "down", "up"])
def test_gradcheck_dwconv(amd, mode):
    T = amd.train_mbconv
    k = 3 if mode == "same" else 2
    for shape in DW_SHAPES[mode]:
        gen = torch.Generator().manual_seed(sum(shape))
        x = torch.randn(shape, dtype=torch.float64, generator=gen, requires_grad=True)
        w = torch.randn(shape[-1], 1, k, k, dtype=torch.float64, generator=gen, requires_grad=True)
        assert torch.autograd.gradcheck(lambda x, w: T.dwconv(x, w, mode), (x, w))
        # and the restatement is the torch op
        xc = x.detach().permute(0, 3, 1, 2)
        if mode == "same":
            want = F.conv2d(F.pad(xc, (1, 1, 1, 1), mode="circular"), w.detach(), groups=shape[-1])
        elif mode == "down":
            want = F.conv2d(xc, w.detach(), stride=2, groups=shape[-1])
        else:
            want = F.conv_transpose2d(xc, w.detach(), stride=2, groups=shape[-1])
        assert float((T.dwconv(x.detach(), w.detach(), mode) - want.permute(0, 2, 3, 1)).abs().max()) <= 1e-14


def test_dwconv_odd_extent_takes_the_torch_route(amd):
    """A stride-2 conv on an odd extent is outside the fused node's rule: F.conv2d (floor), with autograd's backward."""
    T = amd.train_mbconv
    x = torch.randn(1, 3, 5, 2, dtype=torch.float64, requires_grad=True)
    w = torch.randn(2, 1, 2, 2, dtype=torch.float64, requires_grad=True)
    y = T.dwconv(x, w, "down")
    assert y.shape == (1, 1, 2, 2)
    assert torch.autograd.gradcheck(lambda x, w: T.dwconv(x, w, "down"), (x, w))


@pytest.mark.parametrize("shape", [(1, 1, 1, 3), (2, 2, 3, 4), (3, 1, 2, 2)])
def test_gradcheck_se_scale(amd, shape):
    T = amd.train_mbconv
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, dtype=torch.float64, generator=gen, requires_grad=True)
    gate = torch.rand(shape[0], shape[-1], dtype=torch.float64, generator=gen, requires_grad=True)
    assert torch.autograd.gradcheck(T.se_scale, (x, gate))
    assert torch.equal(T.se_scale(x, gate), x * gate.reshape(shape[0], 1, 1, -1))


@pytest.mark.parametrize("case", C.block_cases())
def test_block_forward_matches_reference(amd, case):
    from vqae_amd.layers.mbconv_train import MBConv
    block, x, g, ref = C.block_case(case, MBConv)
    x = x.contiguous(memory_format=torch.channels_last)
    got = C.block_results(block, x, g, amd.train_mbconv.block_forward)
    assert set(got) == set(ref)
    for k, (v64, e_ref) in ref.items():
        assert e_ref <= 1e-5, (case, k, e_ref)                 # the generator's condition
        e = C.dist(got[k], v64)
        print(f"{case} {k}: e {e:.2e} e_ref {e_ref:.2e}")
        assert e <= BAR * e_ref, (case, k, e, e_ref)
    # the stock-torch form of the same block (the GPU test's second yardstick) is the reference's arithmetic
    block2, _, _, _ = C.block_case(case, MBConv)
    stock = C.block_results(block2, x, g, amd.train_mbconv.block_forward_torch)
    for k, (v64, e_ref) in ref.items():
        assert C.dist(stock[k], v64) <= BAR * e_ref, (case, k)


def test_block_forward_fp64_and_module(amd):
    """In fp64 the CPU path is the reference to fp64 rounding; the `_target_` subclass keeps the mirror's constructor and state
    dict, trains in train mode, and counts num_batches_tracked."""
    from vqae_amd.layers.conv_block import MBConv as Mirror
    from vqae_amd.layers.mbconv_train import MBConv
    for case in C.block_cases():
        block, x, g, ref = C.block_case(case, MBConv, dtype=torch.float64)
        got = C.block_results(block, x, g, lambda b, t: b(t))
        for k, (v64, _) in ref.items():
            assert C.dist(got[k], v64) <= 1e-12, (case, k)
        assert all(int(m.num_batches_tracked) == 1 for m in block.modules() if isinstance(m, torch.nn.BatchNorm2d))
    kw = C.block_kwargs()
    m, t = Mirror(8, 16, "down", **kw), MBConv(8, 16, "down", **kw)
    assert list(m.state_dict()) == list(t.state_dict())
    t.load_state_dict(m.state_dict())
    y = t.train()(torch.randn(2, 8, 4, 4))
    assert y.requires_grad and y.shape == (2, 16, 2, 2)
    y = t.eval()(torch.randn(2, 8, 4, 4, requires_grad=True))           # eval mode with a graph: the running statistics
    assert y.requires_grad
    with pytest.raises(NotImplementedError):                            # the inference mirror still refuses train mode
        m.train().forward_nhwc(torch.zeros(1, 4, 4, 8))


def test_refuses_fixup(amd):
    from vqae_amd.layers.conv_block import PreActFixupResBlock
    from vqae_amd.model import VQAE
    T = amd.train_mbconv
    with pytest.raises(NotImplementedError):
        T.block_forward(PreActFixupResBlock(8, 8, "same"), torch.zeros(1, 8, 4, 4))
    with pytest.raises(NotImplementedError):
        T.forward_train(VQAE.from_spec(amd.SPECS["tiny"]), torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError):                            # and train.py still refuses the MBConv model
        amd.train.forward_train(VQAE.from_spec(amd.SPECS["tinyM"]), torch.zeros(1, 3, 32, 32))


def test_fixture_loop_records_agree():
    z = C.fixture()
    assert z["loop/idx"].shape == (3, 2, 8, 8) and z["loop/min_margin"].shape == (3,)
    assert float(z["loop/min_margin"].min()) >= 1e-3
    for k in ("recon", "vq"):
        assert np.all(np.abs(z[f"loop/{k}32"] - z[f"loop/{k}64"]) <= 1e-5 * np.abs(z[f"loop/{k}64"]))
    assert float(z["loop/final/e32_params"]) < 2e-6 and float(z["loop/final/e32_buffers"]) < 1e-6
    names = C.names_of(z, "loop/final/names")
    assert any(k.endswith("running_var") for k in names) and any(k.endswith("cluster_size") for k in names)


def test_forward_train_first_step_matches_reference(amd):
    z = C.fixture()
    model, batches = C.loop_model()
    x = batches[0].contiguous(memory_format=torch.channels_last).requires_grad_()
    out, recon, (vq_loss,) = amd.train_mbconv.step(model, x)
    (recon + vq_loss).backward()
    o32 = torch.from_numpy(z["loop/step0/out32"])
    o64 = o32.double() + torch.from_numpy(z["loop/step0/out64lo"]).double()
    assert C.dist(out.detach(), o64) <= BAR * C.dist(o32, o64)
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
    """forward_train + Huber + torch.optim.AdamW for the fixture's three steps on the CPU: the recorded codes exactly, the six
    losses (one vector), the final parameters (one vector) and the quantiser's and BatchNorms' buffers (one vector) within 4 x
    the fp32 reference run's own distance to the fp64 run."""
    same, losses, groups = C.closed_loop(amd)
    assert all(same), same
    e, e_ref = C.loss_distances(losses)
    print(f"loop losses: e {e:.2e} e_ref {e_ref:.2e}")
    assert e <= BAR * e_ref, (e, e_ref)
    for tag, (got, want, e32) in groups.items():
        e = C.dist(got, want)
        print(f"loop final {tag}: e {e:.2e} e32 {e32:.2e}")
        assert e <= BAR * e32, (tag, e, e32)


def test_new_symbols_validate_before_any_launch(amd):
    """The error convention of the C ABI of csrc/mbconv_train.hip, without a GPU (validation precedes every HIP call)."""
    L = amd._lib
    lib = L.lib()
    one = ctypes.c_void_p(16)
    assert [lib.vqae_bn_act_train_supported(c) for c in (0, 3, 4, 6, 8, 260, 1024, 1028)] == [0, 0, 1, 0, 1, 1, 1, 0]
    assert lib.vqae_dwconv_train_supported(8, 4, 6, L.DW_DOWN) == 1 and lib.vqae_dwconv_train_supported(8, 3, 6, L.DW_DOWN) == 0
    assert lib.vqae_dwconv_train_supported(8, 3, 5, L.DW_SAME) == 1 and lib.vqae_dwconv_train_supported(6, 3, 5, L.DW_UP) == 0
    R = L.MBT_ROWS
    assert lib.vqae_bn_act_train_workspace_bytes(2, R + 1, 8) >= 2 * 2 * 2 * 8 * 8
    assert lib.vqae_bn_act_train_workspace_bytes(0, 4, 8) == 0 and lib.vqae_se_scale_workspace_bytes(2, 0, 8) == 0
    assert lib.vqae_dwconv_train_workspace_bytes(2, 4, 6, 8, L.DW_SAME) >= 2 * 9 * 8 * 8
    assert lib.vqae_dwconv_train_workspace_bytes(2, 3, 6, 8, L.DW_DOWN) == 0
    fwd = lambda x, batch, hw, c, training=1: lib.vqae_bn_act_train_forward_f32(
        x, one, one, one, one, training, 0.1, 1e-5, 1, batch, hw, c, one, one, one, None, one, None)
    with pytest.raises(AssertionError):
        L.check(fwd(None, 2, 4, 8))                                     # null pointer
    with pytest.raises(AssertionError):
        L.check(fwd(one, 2, 0, 8))                                      # zero extent
    with pytest.raises(AssertionError):
        L.check(fwd(one, 0, 4, 8))
    with pytest.raises(NotImplementedError):
        L.check(fwd(one, 2, 4, 6))                                      # C % 4 != 0 -> VQAE_ERR_UNSUPPORTED
    assert b"multiple of 4" in lib.vqae_last_error()
    with pytest.raises(ValueError):
        L.check(fwd(one, 1, 1, 8))                                      # one row in training mode
    with pytest.raises(AssertionError):
        L.check(fwd(ctypes.c_void_p(20), 2, 4, 8))                      # misaligned
    bwd = lambda g, c: lib.vqae_bn_act_train_backward_f32(g, one, one, one, one, one, None, 1, 1, 2, 4, c, one, one, one, None)
    with pytest.raises(AssertionError):
        L.check(bwd(None, 8))
    with pytest.raises(NotImplementedError):
        L.check(bwd(one, 3))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_dwconv_train_forward_f32(one, None, L.DW_SAME, 1, 2, 2, 8, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_dwconv_train_forward_f32(one, one, L.DW_SAME, 1, 0, 2, 8, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_dwconv_train_forward_f32(one, one, 3, 1, 2, 2, 8, one, None))            # no such mode
    with pytest.raises(NotImplementedError):
        L.check(lib.vqae_dwconv_train_forward_f32(one, one, L.DW_DOWN, 1, 3, 2, 8, one, None))    # odd extent, stride 2
    with pytest.raises(NotImplementedError):
        L.check(lib.vqae_dwconv_train_backward_f32(one, one, one, L.DW_UP, 1, 2, 2, 6, one, one, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_dwconv_train_backward_f32(one, None, one, L.DW_UP, 1, 2, 2, 8, one, one, one, None))   # g_w without x
    with pytest.raises(AssertionError):
        L.check(lib.vqae_se_scale_forward_f32(one, None, 1, 4, 8, one, None))
    with pytest.raises(NotImplementedError):
        L.check(lib.vqae_se_scale_forward_f32(one, one, 1, 4, 5, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_se_scale_backward_f32(one, one, one, 1, 4, 8, one, one, None, None))     # no workspace
    with pytest.raises(amd._lib.VqaeHipError):
        amd.ops.se_scale_forward(torch.zeros(1, 2, 2, 4), torch.zeros(1, 4))
