"""The fixtures behind tests/test_edges32_gpu.py, on the CPU (no GPU): for every case of tests/edges32_cases.py the reference's
fp32 block on the case's input (block_cases.edge_input on the f32 taps) is within a quarter of the fp32 block bar of the block in
fp64 -- so bar a of the GPU file, max |err| <= 2e-5 * max(1, max |ref|), is not consumed by the yardstick -- and the yardstick
of the F(4x4, 3x3) routes (block_cases.f44_block: conv2 through oracle/winograd_sim.py in fp32) is finite, non-zero, and itself
within that bar, and not the reference's own block (the helper really replaced conv2)."""
import pytest
import torch

from block_cases import edge_input, exact_block, f44_block, find_block, oracle_taps
from edges32_cases import CHAINS, GROUPS, cases, yardstick

BAR = 2e-5


def test_case_table_is_consistent():
    for gid, (name, mode, cin, route, ins, outs) in GROUPS.items():
        assert ins and not set(ins) & set(outs), gid
        assert route not in outs.values(), gid
        assert len(cases(gid)) == len(set(s for _, s, _ in cases(gid))), gid
        for _, (B, H, W), r in cases(gid):
            assert yardstick(r) == "ref32" or (mode == "same" and H % 4 == 0 and W % 4 == 0), (gid, B, H, W)
    for (route, C), (name, shapes) in CHAINS.items():
        assert any(g[:4] == (name, "same", C, route) for g in GROUPS.values()) and all(B > 1 for B, _, _ in shapes), (route, C)


@pytest.mark.parametrize("gid", list(GROUPS))
def test_reference_and_yardstick_against_fp64(oracle, gid):
    name, mode, cin = GROUPS[gid][:3]
    spec, p, _, taps = oracle_taps(oracle, name, "f32")
    side, i, blocks, tap_name = find_block(oracle, spec, mode, cin)
    prefix = blocks[i][0]
    bad = []
    for kind, (B, H, W), route in cases(gid):
        x = edge_input(taps[tap_name], B, H, W)
        assert x.shape == (B, cin, H, W) and x.dtype == torch.float32
        exact = exact_block(oracle, p, name, x, prefix, mode, spec)
        scale = max(1.0, float(exact.abs().max()))
        assert bool(torch.isfinite(exact).all()) and float(exact.abs().max()) > 0
        ref = oracle.conv_block(x, p, prefix, mode, spec)
        err_ref = float((ref.double() - exact).abs().max())
        print(f"{gid} {kind} {(B, H, W)} -> {route}: |ref32 - fp64| = {err_ref / scale:.3e} * scale")
        if not err_ref <= 0.25 * BAR * scale:
            bad.append((kind, B, H, W, "ref32", err_ref / scale))
        if yardstick(route) == "f44":
            y44 = f44_block(oracle, p, x, prefix)
            err44 = float((y44.double() - exact).abs().max())
            print(f"    F(4x4) yardstick: |. - fp64| = {err44 / scale:.3e} * scale, {err44 / err_ref:.2f} x the reference's")
            if not (y44.dtype == torch.float32 and bool(torch.isfinite(y44).all()) and float(y44.abs().max()) > 0
                    and not torch.equal(y44, ref) and err44 <= BAR * scale):
                bad.append((kind, B, H, W, "f44", err44 / scale))
            assert oracle.conv_block(x, p, prefix, mode, spec).equal(ref)          # the helper put the direct conv2 back
    assert not bad, bad
