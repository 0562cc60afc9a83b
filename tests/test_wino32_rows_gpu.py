"""The exact-width C = 32 F(2x2, 3x3) kernel (128-wide grid) stages every input row once in an LDS ring of four raw rows and
forms its MFMA operands from the ring on the fly; the column-blocked instantiation (grids k x 128 wide) keeps the transform
that fetches the rows per pass and stores V (csrc/conv_wino.hip).  Both compute the same expressions
in the same order, so no bit may differ:
  1. a 256-wide image of period 128 runs the column-blocked kernel; both halves of its output equal the 128-wide run.
     At H = 4 the halo rows r0 - 1 and r0 + 4 wrap onto rows of the tile itself, at H = 12 the second workgroup of an image
     wraps at neither end;
  2. an input that is zero except in one image row (each of the 8 rows at H = 8) gives what the periodic run gives -- a stale
     or wrongly replaced ring slot shows at the row it concerns;
  3. rolling the input by 2, 4, 6 rows (the 2 x 2 tile phase is kept; rows move between tile rows, workgroups and the wrap)
     or by 2, 62, 64, 126 columns (across the wave boundary at pixel 64 and across the wrap) rolls the output and changes
     no bit.
All through NativeVQAE.run_blocks on cfg B at the first C = 32 'same' pair; count = 1 / 2 run both tails."""
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
                 if blocks[i][1:] == ("same", 32, 32) and blocks[i + 1][1:] == ("same", 32, 32))
    return nat, first


def periodic(nat, i, count, x):
    """The 256-wide image of period 128: the column-blocked kernel.  Returns its two halves."""
    y = nat.run_blocks("encoder", i, count, x.repeat(1, 1, 2, 1).contiguous())
    assert y.shape == (x.shape[0], x.shape[1], 256, 32)
    return y[:, :, :128], y[:, :, 128:]


@pytest.mark.parametrize("B,H", [(1, 4), (2, 8), (1, 12)])
def test_equals_the_column_blocked_kernel(ctx, B, H):
    nat, i = ctx
    gen = torch.Generator().manual_seed(700 + H)
    x = torch.randn(B, H, 128, 32, generator=gen).cuda()
    for count in (1, 2):                              # a single block; a chained pair (the fused next conv1)
        y = nat.run_blocks("encoder", i, count, x)
        assert y.shape == x.shape
        lo, hi = periodic(nat, i, count, x)
        assert torch.equal(lo, y), (count, B, H, "left half")
        assert torch.equal(hi, y), (count, B, H, "right half")


@pytest.mark.parametrize("r", range(8))
def test_single_row_impulse_equals_the_column_blocked_kernel(ctx, r):
    nat, i = ctx
    gen = torch.Generator().manual_seed(800 + r)
    x = torch.zeros(1, 8, 128, 32)
    x[:, r] = torch.randn(1, 128, 32, generator=gen)
    x = x.cuda()
    for count in (1, 2):
        y = nat.run_blocks("encoder", i, count, x)
        lo, hi = periodic(nat, i, count, x)
        assert torch.equal(lo, y), (count, r, "left half")
        assert torch.equal(hi, y), (count, r, "right half")


def test_shifts_move_the_output_and_change_no_bit(ctx):
    nat, i = ctx
    gen = torch.Generator().manual_seed(900)
    x = torch.randn(2, 8, 128, 32, generator=gen).cuda()
    for count in (1, 2):
        y = nat.run_blocks("encoder", i, count, x)
        for dim, shifts in ((1, (2, 4, 6)), (2, (2, 62, 64, 126))):
            for shift in shifts:
                yr = nat.run_blocks("encoder", i, count, torch.roll(x, shift, dims=dim).contiguous())
                assert torch.equal(torch.roll(yr, -shift, dims=dim), y), (count, dim, shift)
