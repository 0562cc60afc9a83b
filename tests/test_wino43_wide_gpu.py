"""The wide instantiation of the split F(4x4, 3x3) trunk kernel (csrc/conv_wino43.hip): at C = 128 and
H % 16 == 0 one 512-thread workgroup owns two 8-row bands and feeds both from every weight fragment it loads.  Each accumulator
sees the MFMAs of the 8-row kernel in their order, so the results must be the 8-row kernel's bit for bit:
  1. a vertically tiled period-8 image gives, in every band, exactly what the 8-row kernel gives for one period;
  2. rolling the input by one band rolls the output and changes no bit (halo rows across bands and workgroups);
  3. the distance to the fp64 block stays within 1.25x of the fp32-MFMA form's (the bar of test_wino43_split_gpu.py) on
     grids of one workgroup wrapping onto itself (H = 16) and of three (H = 48).
All through NativeVQAE.run_blocks on cfg B; H = 8 runs the 8-row kernel, H = 16 / 32 / 48 the wide one."""
import os

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
    split = amd.NativeVQAE(amd.SPECS["B"], p)
    old = os.environ.get("VQAE_W43_SPLIT")
    os.environ["VQAE_W43_SPLIT"] = "0"                # read once per handle
    try:
        plain = amd.NativeVQAE(amd.SPECS["B"], p)
    finally:
        if old is None:
            del os.environ["VQAE_W43_SPLIT"]
        else:
            os.environ["VQAE_W43_SPLIT"] = old
    p64 = {k: v.double() for k, v in p.items() if torch.is_tensor(v) and v.is_floating_point()}
    return spec, p64, split, plain


def _pairs(blocks):
    """indices of the first and the last C = 128 'same' block whose successor is one too"""
    ok = [i for i in range(len(blocks) - 1)
          if blocks[i][1:] == ("same", 128, 128) and blocks[i + 1][1:] == ("same", 128, 128)]
    return [ok[0], ok[-1]]


@pytest.mark.parametrize("B", [1, 3])
def test_bands_of_a_period_8_image_equal_the_8_row_kernel(ctx, oracle, B):
    spec, _, split, _ = ctx
    i = _pairs(oracle.encoder_blocks(spec))[0]
    gen = torch.Generator().manual_seed(11 + B)
    x8 = torch.randn(B, 8, 32, 128, generator=gen).cuda()
    for count in (1, 2):                              # a single block; a chained pair (the fused next conv1)
        y8 = split.run_blocks("encoder", i, count, x8)
        for reps in (2, 4):
            y = split.run_blocks("encoder", i, count, x8.repeat(1, reps, 1, 1).contiguous())
            assert y.shape == (B, 8 * reps, 32, 128)
            for b in range(reps):
                assert torch.equal(y[:, 8 * b:8 * b + 8], y8), (count, reps, b)


@pytest.mark.parametrize("B,H", [(2, 32), (1, 48)])
def test_band_shift_moves_the_output_and_changes_no_bit(ctx, oracle, B, H):
    spec, _, split, _ = ctx
    i = _pairs(oracle.encoder_blocks(spec))[0]
    gen = torch.Generator().manual_seed(100 + H)
    x = torch.randn(B, H, 32, 128, generator=gen).cuda()
    xr = torch.roll(x, 8, dims=1).contiguous()
    for count in (1, 2):
        y = split.run_blocks("encoder", i, count, x)
        yr = split.run_blocks("encoder", i, count, xr)
        assert torch.equal(torch.roll(yr, -8, dims=1), y), (count, B, H)


@pytest.mark.parametrize("side", ["encoder", "decoder"])
def test_wide_trunk_blocks_as_close_to_fp64_as_fp32_mfma(ctx, oracle, side):
    spec, p64, split, plain = ctx
    blocks = oracle.encoder_blocks(spec) if side == "encoder" else oracle.decoder_blocks(spec)
    gen = torch.Generator().manual_seed(7)
    worst = (0.0, 0.0)
    for i in _pairs(blocks):
        for (B, H) in ((1, 16), (3, 16), (1, 48)):
            x = torch.randn(B, 128, H, 32, generator=gen, dtype=torch.float64)
            ex1 = oracle.conv_block(x, p64, blocks[i][0], "same", spec)
            ex2 = oracle.conv_block(ex1, p64, blocks[i + 1][0], "same", spec)
            xin = x.float().permute(0, 2, 3, 1).contiguous().cuda()
            for count, ex in ((1, ex1), (2, ex2)):
                d = []
                for nat in (split, plain):
                    y = nat.run_blocks(side, i, count, xin).permute(0, 3, 1, 2).cpu().double()
                    e = (y - ex).abs()
                    d.append((float((e ** 2).mean().sqrt()), float(e.max())))
                (rs, ms), (rp, mp) = d
                print(f"{blocks[i][0]} x{count} {B}x{H}x32: wide split rms {rs:.3e} max {ms:.3e} | fp32 MFMA rms {rp:.3e} max {mp:.3e}")
                assert rs <= 1.25 * rp and ms <= 1.25 * mp, (blocks[i][0], count, B, H, rs, rp, ms, mp)
                worst = max(worst, (rs / rp, ms / mp))
    print(f"worst wide split / fp32-MFMA distance ratio (rms, max): {worst[0]:.3f}, {worst[1]:.3f}")
