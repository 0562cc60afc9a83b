"""The 16-bit whole-block kernels (same8_16.hip, trunk16.hip, down16.hip, up16.hip) at the edges of their tile geometry,
against the oracle's block under CPU autocast and against the block in fp64, on identical inputs.

tests/test_blocks_gpu.py meets each of these kernels at one geometry per (C, W): the square 128 x 128 / 256 x 256 fixture
taps, where every image has many tile rows.  Here each kernel runs where its index arithmetic is at its limits -- one tile
row per image (both circular halo rows are the tile's own), one-row images, a tile as wide as the image (the wrap column
is the tile's own far column), an 'up' window wider than the image (every column clamped), an image boundary at every
tile of a batch -- and one smallest step OUTSIDE its `*_supported` predicate, where the dispatch must take another route
and still answer.  `NativeVQAE.block_route` (vqae_block_route) says which route a case ran, so a case cannot pass on a
kernel it was not written for.  It is the only place where the C = 16 / 32 instances of trunk16.hip run: select_route
asks same16_16_supported (H % 8 == 0) first, so they serve the heights that are no multiple of 8.

Inputs: the oracle's own activation in front of the block (block_cases.oracle_taps, the same autocast dtype), cropped from
the top-left corner, continued by its mirror image where the case is wider or taller than the tap; the tap's first B
images, further ones the tap's images rolled by (1, 3) pixels -- activations of the magnitudes the 16-bit bars were
measured at.

Per case:
 a. against `oracle.conv_block` under CPU autocast on the identical input: block_cases.compare, one block -- at most
    8 % of the elements further than 1e-5 * scale, none further than 3 ulp16 * scale;
 b. against the block in fp64 (exact_block): the HIP block no further than 1.25 x the reference's own 16-bit distance,
    RMS and max -- asserted on the errors pooled over all cases of one (group, C, dtype), because a case has as few as
    2 048 elements and the reference's own max varies by 1.6 x between such crops; the per-case ratios are recorded;
 c. every image of a batch equals, bit for bit, the same image run alone.  Where the image alone would leave the case's
    route (head16 wants a multiple of 32 pixels: the c = 128 'up' case (2, 1, 16)), "alone" is the image followed by an
    all-zero image, the smallest batch that stays on the kernel under test;
 d. translation ('same' and 'down' groups; a bicubic resize with clamped borders does not commute with a roll):
    run(roll(x)) == roll(run(x)) bit for bit -- the convs are circular, and every kernel here sums an output over
    taps x channels in an order that does not depend on the pixel's position.
"""
import pytest
import torch

from block_cases import (autocast_ctx, compare, distance_to_exact, edge_input, exact_block, find_block, native_handle, nhwc, oracle_taps,
                         roll_nhwc)
from conftest import record_parity

pytestmark = pytest.mark.gpu

SAME_IN = ((1, 8, 64), (3, 8, 64), (2, 8, 128), (1, 16, 192), (2, 24, 64))


def _t16_small(W):
    return tuple((b, h, W) for b, h in ((1, 1), (2, 1), (3, 2), (1, 3), (2, 4), (1, 12)))


def _t16_wide(W):
    return tuple((b, h, W) for b, h in ((1, 4), (3, 4), (1, 8), (2, 12)))


def _down(r):
    ins = ((1, 2 * r, 64), (3, 2 * r, 64), (1, 2 * r, 128), (2, 6 * r, 64))
    outs = ((1, 2 * r, 32),) + (((1, 2 * r - 2, 64),) if r > 1 else ())
    return ins, outs


UP_IN = ((1, 2, 16), (2, 2, 16), (1, 4, 32), (3, 2, 48), (1, 6, 16))
UP_ODD = ((2, 1, 16), (1, 3, 32))          # odd low-resolution heights: 4-row tiles (c <= 64) cannot cover 2 H rows, 2-row tiles can

# id -> (group, model, mode, cin of the block, route of the "in" cases, "in" shapes, "out" shapes, route an "out" case must
# report or None for "any other").  Shapes are (B, H, W) of the block's input.  The block is the first one of that mode and
# width in the model's encoder ('same', 'down') or decoder ('up') list: enc block 0 for C = 8 / 16 / 32.
GROUPS = {
    "same8_16-c8": ("same8_16", "midA", "same", 8, "same8_16", SAME_IN, ((1, 4, 64), (1, 8, 32)), None),
    "same16_16-c16": ("same16_16", "mid16", "same", 16, "same16_16", SAME_IN, ((1, 4, 128),), "trunk16"),
    "same16_16-c32": ("same16_16", "mid", "same", 32, "same16_16", SAME_IN, ((1, 4, 128),), "trunk16"),
    "trunk16-c16": ("trunk16", "mid16", "same", 16, "trunk16", _t16_small(128) + _t16_small(256), ((1, 4, 64),), None),
    "trunk16-c32": ("trunk16", "mid", "same", 32, "trunk16", _t16_small(128) + _t16_small(256), ((1, 4, 64),), None),
    "trunk16-c64w64": ("trunk16", "mid", "same", 64, "trunk16", _t16_wide(64), ((1, 2, 64), (1, 6, 64)), None),
    "trunk16-c128w32": ("trunk16", "mid", "same", 128, "trunk16", _t16_wide(32), ((1, 2, 32), (1, 6, 32)), None),
    "trunk16-c64w128": ("trunk16", "midC", "same", 64, "trunk16", _t16_wide(128), ((1, 2, 128), (1, 6, 128)), None),
    "trunk16-c128w64": ("trunk16", "midC", "same", 128, "trunk16", _t16_wide(64), ((1, 2, 64), (1, 6, 64)), None),
    "trunk16-c256w32": ("trunk16", "midC", "same", 256, "trunk16", _t16_wide(32), ((1, 2, 32), (1, 6, 32)), None),
    "down16-c8": ("down16", "midA", "down", 8, "down16") + _down(4) + (None,),          # r = d16_tile_rows(cin) = 4, 4, 2, 1
    "down16-c16": ("down16", "mid16", "down", 16, "down16") + _down(4) + (None,),
    "down16-c32": ("down16", "mid", "down", 32, "down16") + _down(2) + (None,),
    "down16-c64": ("down16", "midC", "down", 64, "down16") + _down(1) + (None,),
    "up16-c64": ("up16", "midA", "up", 64, "up16", UP_IN, ((2, 2, 8),) + UP_ODD, "up"),
    "up16-c32": ("up16", "midA", "up", 32, "up16", UP_IN, ((2, 2, 8),) + UP_ODD, "up"),
    "up16-c16": ("up16", "midA", "up", 16, "up16", UP_IN, ((2, 2, 8),) + UP_ODD, "up"),
    "up16-c128": ("up16", "mid", "up", 128, "up16", UP_IN + UP_ODD, ((2, 2, 8),), "up"),
}
ROLLS = {"same": (((1, 0), (1, 0)), ((0, 1), (0, 1)), ((0, 31), (0, 31)), ((1, 33), (1, 33))),      # (input roll, output roll)
         "down": (((2, 0), (1, 0)), ((0, 2), (0, 1)), ((0, 66), (0, 33)))}


def run1(nat, side, i, x_nchw, count=1):
    return nat.run_blocks(side, i, count, nhwc(x_nchw).cuda())


@pytest.mark.parametrize("tag", ["bf16", "f16"])
@pytest.mark.parametrize("gid", list(GROUPS))
def test_16bit_block_kernel_at_its_geometry_edges(amd, oracle, gid, tag):
    """One (group, C, dtype): every "in" case on the named route and every "out" case on another, assertions a to d of
    the module docstring.  All cases run before anything is asserted, so a failure lists every case that missed."""
    group, name, mode, cin, route, ins, outs, out_route = GROUPS[gid]
    spec, p, _, taps = oracle_taps(oracle, name, tag)
    nat = native_handle(amd, oracle, name, tag)
    side, i, blocks, tap_name = find_block(oracle, spec, mode, cin)
    prefix = blocks[i][0]
    wrong_route, bad_ref, bad_batch, bad_roll = [], [], [], []
    se_h = se_r = n_el = 0.0
    mx_h = mx_r = 0.0
    for kind, shapes in (("in", ins), ("out", outs)):
        for (B, H, W) in shapes:
            case = (kind, B, H, W)
            got_route = nat.block_route(side, i, B, H, W)
            if (got_route == route) != (kind == "in") or (kind == "out" and out_route and got_route != out_route):
                wrong_route.append(case + (got_route,))
            x = edge_input(taps[tap_name], B, H, W)
            y = run1(nat, side, i, x)                                    # an error here (no result) fails the test
            with autocast_ctx(tag):
                ref = oracle.conv_block(x, p, prefix, mode, spec).float()
            ok, rel, frac = compare(y, ref, tag, 1)                      # a
            if not ok:
                bad_ref.append(case + (rel, frac))
            rh, rr, mh, mr = distance_to_exact(y, ref, exact_block(oracle, p, name, x, prefix, mode, spec))   # b, pooled below
            n = float(ref.numel())
            se_h += rh * rh * n; se_r += rr * rr * n; n_el += n
            mx_h, mx_r = max(mx_h, mh), max(mx_r, mr)
            record_parity("edges16", group=group, model=name, block=prefix, cin=cin, dtype=tag, case=kind, B=B, H=H, W=W,
                          route=got_route, rel_err=rel, frac_off=frac, rms_ratio_vs_ref16=rh / rr, max_ratio_vs_ref16=mh / mr)
            if B > 1:                                                    # c
                same_route = nat.block_route(side, i, 1, H, W) == got_route
                for b in range(B):
                    xb = x[b:b + 1] if same_route else torch.cat([x[b:b + 1], torch.zeros_like(x[b:b + 1])])
                    if not torch.equal(run1(nat, side, i, xb)[0], y[b]):
                        bad_batch.append(case + (b,))
            for (iy, ix), (oy, ox) in ROLLS.get(mode, ()):               # d
                yr = run1(nat, side, i, torch.roll(x, shifts=(iy % H, ix % W), dims=(2, 3)))
                if not torch.equal(yr, roll_nhwc(y, oy, ox)):
                    bad_roll.append(case + (iy, ix, float((yr - roll_nhwc(y, oy, ox)).abs().max())))
    rms_h, rms_r = (se_h / n_el) ** 0.5, (se_r / n_el) ** 0.5
    record_parity("edges16_pooled", group=group, model=name, cin=cin, dtype=tag, cases=len(ins) + len(outs), elements=int(n_el),
                  rms_ratio_vs_ref16=rms_h / rms_r, max_ratio_vs_ref16=mx_h / mx_r, wrong_route=len(wrong_route),
                  failed_ref=len(bad_ref), failed_batch=len(bad_batch), failed_roll=len(bad_roll))
    assert not wrong_route, wrong_route
    assert not bad_ref, bad_ref
    assert rms_h <= 1.25 * rms_r and mx_h <= 1.25 * mx_r, (rms_h, rms_r, mx_h, mx_r)
    assert not bad_batch, bad_batch
    assert not bad_roll, bad_roll


# (C, W) -> model; R = rows of the pair's tile: 4 at C >= 64; C = 16 / 32 run H = 4 (one tile row of the 16-m-tile form) and
# H = 1 (the 4-m-tile fall-back, whose tile is one row)
T16_PAIRS = {(16, 128): "mid16", (16, 256): "mid16", (32, 128): "mid", (32, 256): "mid", (64, 64): "mid", (128, 32): "mid",
             (64, 128): "midC", (128, 64): "midC", (256, 32): "midC"}


@pytest.mark.parametrize("tag", ["bf16", "f16"])
@pytest.mark.parametrize("C,W", list(T16_PAIRS))
def test_trunk16_chained_pair_at_one_tile_row(amd, oracle, C, W, tag):
    """The NEXT form of every trunk16 instance (conv2 + conv3 + the next block's conv1 in one launch; at C = 256 behind the
    generic conv1 + trunk16_round_pack head) on three images of one tile row each: blocks [i, i + 1] in one run against the
    oracle's block i + 1 on the GPU's own output of block i alone (as test_fused_next_conv1_on_identical_inputs): bar a."""
    name = T16_PAIRS[(C, W)]
    spec, p, _, taps = oracle_taps(oracle, name, tag)
    nat = native_handle(amd, oracle, name, tag)
    side, i, blocks, tap_name = find_block(oracle, spec, "same", C, pair=True)
    bad = []
    for H in ((4, 1) if C <= 32 else (4,)):
        assert nat.block_route(side, i, 3, H, W, chained=True) == "trunk16" and nat.block_route(side, i + 1, 3, H, W) == "trunk16"
        x = edge_input(taps[tap_name], 3, H, W)
        y1, y2 = run1(nat, side, i, x), run1(nat, side, i, x, count=2)
        with autocast_ctx(tag):
            ref2 = oracle.conv_block(y1.permute(0, 3, 1, 2).cpu(), p, blocks[i + 1][0], "same", spec).float()
        ok, rel, frac = compare(y2, ref2, tag, 1)
        record_parity("edges16_chain", model=name, block=blocks[i + 1][0], cin=C, dtype=tag, B=3, H=H, W=W, rel_err=rel, frac_off=frac)
        if not ok:
            bad.append((H, rel, frac))
    assert not bad, bad


def test_block_route_refuses_bad_arguments(amd, oracle):
    nat = native_handle(amd, oracle, "mid16", "bf16")
    assert nat.block_route("encoder", 0, 1, 8, 128) == "same16_16"
    for args in ((99, 1, 8, 128), (-1, 1, 8, 128), (0, 0, 8, 128), (0, 1, 0, 128), (0, 1, 8, 0)):
        with pytest.raises(AssertionError, match="vqae_block_route"):
            nat.block_route("encoder", *args)
