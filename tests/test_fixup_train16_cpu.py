"""CPU: the Fixup training path under 16-bit autocast (vqae_amd.train with the 16-bit-I/O nodes of csrc/fixup_train_io.hip),
through its plain-torch restatements, which follow the same dtype rules (tests/test_fixup_train16_gpu.py runs the kernels).

  * the four _io entry points are declared, exported and bound;
  * under torch.autocast("cpu", dtype=torch.bfloat16) train.block_forward gives the output BITS of train.block_forward_torch
    on every fixture block: the conv's own cast of an fp32 activation and the node's 16-bit store round the same fp32 value;
  * the dtypes: a node that feeds a conv writes the autocast dtype, any other fp32; the block output is fp32; g_x has x's
    dtype; the gradients of the one-element parameters are fp32;
  * gradient distance to the fixture's fp64 gradients <= 4 x that of block_forward_torch under the same autocast, per tensor
    (the one-element tensors as one vector).  Measured ratios e_dev / e_ref over all tensors of all eight cases:
    0.99999 .. 1.000003 (the weight gradients are bit-equal; the input gradient and the scalars differ in the order of fp32
    sums);
  * the fp32 wrappers of ops.py refuse a 16-bit tensor before any device call.
"""
import pytest
import torch

import fixup_train_cases as C

BAR = 4.0
BF16 = torch.bfloat16
IO_SYMBOLS = ("vqae_fixup_act_io", "vqae_fixup_act_backward_io", "vqae_fixup_out_io", "vqae_fixup_out_backward_io")


def P(v):
    return torch.tensor([v], dtype=torch.float32, requires_grad=True)


def test_io_symbols_declared_exported_bound(amd):
    import test_abi
    declared, lib = test_abi.declared_symbols(), amd._lib.lib()
    for name in IO_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/vqae_hip.h"
        assert name in amd._lib.SYMBOLS, f"{name} is not bound in _lib.py"
        fn = getattr(lib, name)
        assert fn.argtypes == amd._lib.SYMBOLS[name][1]


def test_io_entry_points_refuse_bad_dtypes(amd):
    """Validation runs before any HIP call: two different 16-bit types and a 16-bit y of `out` are unsupported, an unknown
    code is invalid; each leaves a message."""
    import ctypes
    L = amd._lib
    lib, one = L.lib(), ctypes.c_void_p(16)              # never dereferenced
    with pytest.raises(NotImplementedError):
        L.check(lib.vqae_fixup_act_io(one, L.DT_BF16, one, one, 1, 0, 1, 1, 1, 4, one, L.DT_F16, None))
    assert b"16-bit" in lib.vqae_last_error()
    with pytest.raises(NotImplementedError):
        L.check(lib.vqae_fixup_act_backward_io(one, L.DT_F16, one, L.DT_BF16, one, 1, 0, 1, 1, 1, 4, one, one, one, one, None))
    with pytest.raises(NotImplementedError):
        L.check(lib.vqae_fixup_out_io(one, L.DT_BF16, one, L.DT_F16, one, one, None, 4, one, L.DT_F32, None))
    with pytest.raises(NotImplementedError):
        L.check(lib.vqae_fixup_out_io(one, L.DT_BF16, one, L.DT_BF16, one, one, None, 4, one, L.DT_BF16, None))
    assert b"fp32" in lib.vqae_last_error()
    with pytest.raises(NotImplementedError):
        L.check(lib.vqae_fixup_out_backward_io(one, one, L.DT_BF16, one, 4, one, one, L.DT_F16, one, one, None, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_fixup_act_io(one, 7, one, one, 1, 0, 1, 1, 1, 4, one, L.DT_F32, None))
    with pytest.raises(AssertionError):                  # a 16-bit skip needs its gradient tensor
        L.check(lib.vqae_fixup_out_backward_io(one, one, L.DT_BF16, one, 4, one, None, L.DT_BF16, one, one, None, one, None))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fp32_wrappers_refuse_16bit_tensors(amd, dtype):
    """CPU tensors: the dtype assertion comes before the check for device memory, so before any device call."""
    ops = amd.ops
    g32, x32 = torch.zeros(1, 2, 2, 4), torch.zeros(1, 2, 2, 4)
    g16, x16 = g32.to(dtype), x32.to(dtype)
    a = torch.zeros(1)
    for g, x in ((g32, x16), (g16, x32), (g16, x16)):
        with pytest.raises(AssertionError, match="fixup_act_backward"):
            ops.fixup_act_backward(g, x, a)
        with pytest.raises(AssertionError, match="fixup_out_backward"):
            ops.fixup_out_backward(g, x, a)
    with pytest.raises(AssertionError, match="fixup_act_backward"):
        ops.fixup_act_backward(g16, None, None, act=False)
    with pytest.raises(amd._lib.VqaeHipError):           # fp32 CPU tensors pass the assertion and stop at the device check
        ops.fixup_act_backward(g32, x32, a)


def test_node_dtypes_under_autocast(amd):
    T = amd.train
    gen = torch.Generator().manual_seed(3)
    x32 = torch.randn(2, 3, 5, 4, generator=gen).requires_grad_()
    x16 = torch.randn(2, 3, 5, 4, generator=gen).to(BF16).requires_grad_()
    s16 = torch.randn(2, 3, 5, 4, generator=gen).to(BF16).requires_grad_()
    a, b, c = P(0.3), P(-0.2), P(0.1)
    assert T.fixup_act(x32, a, b, feeds_conv=True).dtype == torch.float32          # no autocast: nothing changes
    with torch.autocast("cpu", dtype=BF16):
        for x in (x32, x16):
            for halo in (0, 1):
                y = T.fixup_act(x, a, b, halo, feeds_conv=True)
                want = torch.nn.functional.elu(x + a) + b
                assert want.dtype == torch.float32                                  # the reference's promotion
                if halo:
                    want = T.pad_circular_nhwc(want)
                assert y.dtype == BF16 and torch.equal(y, want.to(BF16))
                assert T.fixup_act(x, a, b, halo).dtype == torch.float32            # e.g. in front of bicubic_up2
                gx, ga, gb = torch.autograd.grad(y, [x, a, b], torch.ones_like(y))
                assert gx.dtype == x.dtype and ga.dtype == gb.dtype == torch.float32
            y = T.fixup_add(x, c, feeds_conv=True)
            assert y.dtype == BF16 and torch.equal(y, (x + c).to(BF16))
            g = torch.randn(y.shape, generator=gen).to(BF16)
            gx, gc = torch.autograd.grad(y, [x, c], g)
            assert gx.dtype == x.dtype and torch.equal(gx, g.to(x.dtype)) and gc.dtype == torch.float32
            assert float(gc) == float(g.float().sum())
            assert T.fixup_add(x, c).dtype == torch.float32
        for t, skip in ((x16, x32), (x32, s16), (x16, s16)):
            y = T.fixup_out(t, skip, a, b, c)
            assert y.dtype == torch.float32 and torch.equal(y, (t * a + b) + (skip + c))
            g = torch.randn(y.shape, generator=gen)
            gt, gs, gscale, gb4, gb1 = torch.autograd.grad(y, [t, skip, a, b, c], g)
            assert gt.dtype == t.dtype and gs.dtype == skip.dtype
            assert torch.equal(gt, (g * a).to(t.dtype)) and torch.equal(gs, g.to(skip.dtype))
            assert gscale.dtype == gb4.dtype == gb1.dtype == torch.float32


@pytest.mark.parametrize("case", C.block_cases())
def test_block_under_bf16_autocast(amd, case):
    from conftest import record_parity
    from vqae_amd.layers.fixup_train import PreActFixupResBlock
    T = amd.train
    block, x, g, ref = C.block_case(case, PreActFixupResBlock)
    x = x.contiguous(memory_format=torch.channels_last)

    def under(forward):
        def run(blk, t):
            with torch.autocast("cpu", dtype=BF16):
                return forward(blk, t)
        return run

    before = dict(T.stats)
    got = C.block_results(block, x, g, under(T.block_forward))
    stock = C.block_results(block, x, g, under(T.block_forward_torch))
    assert T.stats["io16_hip"] == before["io16_hip"]                               # CPU tensors run no kernel
    n_resize = T.stats["io16_fallbacks"] - before["io16_fallbacks"]
    assert n_resize == (2 if block.mode == "up" else 0)                            # bicubic_up2 of the branch and of the skip
    assert got["out"].dtype == torch.float32 and got["input"].dtype == torch.float32
    assert all(v.dtype == torch.float32 for v in got.values())
    assert torch.equal(got["out"], stock["out"]), case
    fails = []
    for k, (v64, _) in ref.items():
        e_dev, e_ref = C.dist(got[k], v64.reshape(got[k].shape)), C.dist(stock[k], v64.reshape(stock[k].shape))
        print(f"fixup_train16_cpu {case} {k}: e_dev {e_dev:.3e} e_ref {e_ref:.3e} ratio {e_dev / e_ref:.3f}")
        record_parity("fixup_train16_cpu_block", case=case, tensor=k, e_dev=e_dev, e_ref_stock_autocast=e_ref,
                      ratio=e_dev / e_ref)
        assert bool(torch.isfinite(got[k]).all())
        if not e_dev <= BAR * e_ref:
            fails.append((k, e_dev, e_ref))
    assert not fails, fails
