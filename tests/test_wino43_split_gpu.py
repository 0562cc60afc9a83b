"""The split form of the F(4x4, 3x3) trunk (csrc/conv_wino43.hip): at C = 128 on the 32-wide code grid the
GEMMs run on v_mfma_*_bf16 with every fp32 operand split into three bf16 pieces (six of the nine piece products kept, fp32
accumulation).  It must be at least as close to the exact block as the fp32-MFMA form it replaces (VQAE_W43_SPLIT=0): within
1.25x of that form's distance to the fp64 block, RMS and max, per block and per chained pair, on grids of 8 / 16 / 32 rows and
odd batches; and the codes must agree with that form and, on the reference fixture, bit for bit.  C = 64 / 256 keep the fp32
form, so there is nothing to cover there."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _params(oracle):
    g = load_golden("model_B")
    spec = oracle.SPECS["B"]
    p = oracle.make_params(spec, 0)
    p["encoder.vq_layers.0.embed"] = torch.from_numpy(g["embed"])
    return g, spec, p


def _pairs(blocks):
    """(index, prefix) of C = 128 'same' blocks whose successor is one too: first, middle and last of the run."""
    ok = [i for i in range(len(blocks) - 1)
          if blocks[i][1:] == ("same", 128, 128) and blocks[i + 1][1:] == ("same", 128, 128)]
    return [ok[0], ok[len(ok) // 2], ok[-1]]


def test_split_trunk_blocks_as_close_to_fp64_as_fp32_mfma(amd, oracle, monkeypatch):
    g, spec, p = _params(oracle)
    split = amd.NativeVQAE(amd.SPECS["B"], p)
    monkeypatch.setenv("VQAE_W43_SPLIT", "0")
    plain = amd.NativeVQAE(amd.SPECS["B"], p)
    p64 = {k: v.double() for k, v in p.items() if torch.is_tensor(v) and v.is_floating_point()}
    gen = torch.Generator().manual_seed(7)
    worst = (0.0, 0.0)
    checked = 0
    for side, blocks in (("encoder", oracle.encoder_blocks(spec)), ("decoder", oracle.decoder_blocks(spec))):
        for i in _pairs(blocks):
            for (B, H) in ((3, 8), (1, 16), (5, 32)):
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
                    print(f"{blocks[i][0]} x{count} {B}x{H}x32: split rms {rs:.3e} max {ms:.3e} | fp32 MFMA rms {rp:.3e} max {mp:.3e}")
                    assert rs <= 1.25 * rp and ms <= 1.25 * mp, (blocks[i][0], count, B, H, rs, rp, ms, mp)
                    worst = max(worst, (rs / rp, ms / mp))
                    checked += 1
    print(f"{checked} cases, worst split / fp32-MFMA distance ratio (rms, max): {worst[0]:.3f}, {worst[1]:.3f}")


def test_split_trunk_codes_match_fp32_mfma_and_fixture(amd, oracle, monkeypatch):
    g, spec, p = _params(oracle)
    split = amd.NativeVQAE(amd.SPECS["B"], p)
    monkeypatch.setenv("VQAE_W43_SPLIT", "0")
    plain = amd.NativeVQAE(amd.SPECS["B"], p)
    x = oracle.make_patches(3, 256, 23).cuda()
    _, idx_s, loss_s = split.forward(x)
    _, idx_p, loss_p = plain.forward(x)
    agree = float((idx_s == idx_p).float().mean())
    print(f"split vs fp32 MFMA: index agreement {agree:.5f}, loss {float(loss_s):.7f} vs {float(loss_p):.7f}")
    assert agree >= 0.999
    assert abs(float(loss_s) - float(loss_p)) <= 1e-5 * float(loss_p)
    xg = oracle.make_patches(int(g["batch"]), 256, 0).cuda()
    _, idx, _ = split.forward(xg)
    assert np.array_equal(idx.cpu().numpy().reshape(-1), g["idx"].astype(np.int64).reshape(-1))
