"""The wide split F(4x4, 3x3) trunk kernel's transform fetches four of a tile column's six input columns and takes the other
two, row-combined, from the neighbouring tile column's lanes (csrc/conv_wino43.hip).  The values are the ones
the thread used to load itself, so no bit may change:
  1. rolling the input by whole tile columns (4, 12, 28 columns: across the wrap) rolls the output and changes no bit -- a wrong
     neighbour lane, a wrong wrap or a V slot permutation whose inverse is wrong in the tails would show here;
  2. an input that is zero except in one column (0, 1, 2, 3, 30, 31: both sides of the wrap and every position inside a tile) gives,
     in every band of its period-8 tiling, exactly what the 8-row kernel (whose transform loads all six columns) gives for one period.
All through NativeVQAE.run_blocks on cfg B at the first C = 128 'same' pair; H = 8 runs the 8-row kernel, H = 16 / 32 / 48 the wide one."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(amd, oracle):
    g = load_golden("model_B")
    spec = oracle.SPECS["B"]
    p = oracle.make_params(spec, 0)
    p["encoder.vq_layers.0.embed"] = torch.from_numpy(g["embed"])
    nat = amd.NativeVQAE(amd.SPECS["B"], p)
    blocks = oracle.encoder_blocks(spec)
    first = next(i for i in range(len(blocks) - 1)
                 if blocks[i][1:] == ("same", 128, 128) and blocks[i + 1][1:] == ("same", 128, 128))
    return nat, first


@pytest.mark.parametrize("B,H", [(1, 16), (2, 32), (1, 48)])
def test_column_shift_moves_the_output_and_changes_no_bit(ctx, B, H):
    nat, i = ctx
    gen = torch.Generator().manual_seed(300 + H)
    x = torch.randn(B, H, 32, 128, generator=gen).cuda()
    for count in (1, 2):                              # a single block; a chained pair (the fused next conv1)
        y = nat.run_blocks("encoder", i, count, x)
        assert y.shape == x.shape
        for shift in (4, 12, 28):
            yr = nat.run_blocks("encoder", i, count, torch.roll(x, shift, dims=2).contiguous())
            assert torch.equal(torch.roll(yr, -shift, dims=2), y), (count, B, H, shift)


@pytest.mark.parametrize("c", [0, 1, 2, 3, 30, 31])
def test_single_column_impulse_equals_the_8_row_kernel(ctx, c):
    nat, i = ctx
    gen = torch.Generator().manual_seed(500 + c)
    x8 = torch.zeros(1, 8, 32, 128)
    x8[:, :, c] = torch.randn(1, 8, 128, generator=gen)
    x8 = x8.cuda()
    for count in (1, 2):
        y8 = nat.run_blocks("encoder", i, count, x8)                                   # H = 8: the 8-row kernel
        y = nat.run_blocks("encoder", i, count, x8.repeat(1, 2, 1, 1).contiguous())    # H = 16: the wide kernel
        assert y.shape == (1, 16, 32, 128)
        for b in range(2):
            assert torch.equal(y[:, 8 * b:8 * b + 8], y8), (count, c, b)
