"""The fp32 block routes at the edges of their tile geometry, against the oracle's fp32 block and against the block in fp64 on
identical inputs: the fp32 counterpart of tests/test_edges16_gpu.py.  fixup_fused.hip (C = 8, the C = 16 register Winograd,
launch_fused<32, 4>), down_fused.hip (cin 16 / 32 / 64), wino_trunk_kernel<64 | 128 | 256> in its exact-width and WIDE forms, the
F(4x4, 3x3) kernels (plain at C = 64 / 256, split at C = 128 in its 8-row and 16-row forms), the direct trunk tail, the generic
'same' / 'down' launches, and the two fp32 'up' forms that cfg B does not reach (the (16, 8) up_tail instance of cfg A; C = 256:
three generic 1x1 launches and two bicubic launches).

tests/test_blocks_gpu.py meets each of these at one square geometry with many tile rows per image and a batch of 2.  Here
(tests/edges32_cases.py): one tile row per image, so both circular halo rows are the tile's own; a tile as wide as the image
against the WIDE form at two and three spans; three images of one tile each; H = 1; 8 / 72 / 400 pixels against 128-pixel tiles;
bicubic windows that are clamped on every side -- and one smallest step OUTSIDE each predicate, where the dispatch must take the
route the table names and still answer.  `NativeVQAE.block_route` says which route a case ran.  One handle per model, made
under the default environment; every case reaches its kernel by geometry alone.

Inputs: block_cases.edge_input on the f32 taps.  Per case (all cases of a group run before anything is asserted):
 a. against `oracle.conv_block` in fp32 and against the block in fp64 (exact_block): max |err| <= 2e-5 * max(1, max |ref|), the
    fp32 block bar.  The reference itself is within 6.8e-7 * scale of fp64 on every case (tests/test_edges32_cases_cpu.py);
 b. distance to the fp64 block relative to a CPU fp32 yardstick, RMS and max <= 4 x the yardstick's (the bar of DESIGN
    sections 11 and 21 for fp32 against a reference's own fp32 distance), on the errors pooled over the cases of a group that
    share a yardstick; per-case ratios are recorded.  Yardstick: the reference's fp32 block -- except on `wino43` /
    `wino43_split`, where it is the block with conv2 as F(4x4, 3x3) in fp32 on the CPU (block_cases.f44_block): those
    transforms alone put an fp32 evaluation 3.9 - 5.5 x (RMS) / 6.9 - 8.7 x (max, pooled per group) further from fp64 than the
    direct sum (DESIGN sections 2 and 4), so no kernel of that form can meet a bar relative to the direct reference.  Measured
    pooled ratios: 0.76 - 1.97 RMS; max <= 1.44 except `down_fused-c64` 2.80 and `down-c128` 2.18, where one fp32 accumulator
    runs over K = 512 / 1024 against the CPU library's blocks of 256 (DESIGN section 2 has the CPU emulation of that order);
 c. every image of a batch equals, bit for bit, the same image run alone (B = 1: the fp32 predicates depend on H, W only,
    asserted through block_route);
 d. translation ('same' and 'down'): run(roll(x)) == roll(run(x)) bit for bit, the convs being circular.  Direct-sum routes:
    the ROLLS of the 16-bit file; F(2x2, 3x3) routes: whole 2 x 2 tiles; F(4x4, 3x3) routes: whole 4 x 4 tiles
    (edges32_cases.rolls) -- a shift by less than a Winograd tile changes which input pixels a transform combines first, and
    with it the rounding.  No kernel here needs a shift as large as its workgroup span: each sums an output over
    (transform position x) channels in an order that does not depend on where the tile lies in the workgroup.

What catches a halo taken from the wrong row or image, by family, from the kernels' indexing:
 * F(2x2), `wino-c128` (3, 4, 32): wino_trunk_kernel reads rows r = row0 + 2 s - 1 + j of `xim = t1 + img * H * W * C`, wrapped by
   `r < 0 ? r + H : (r >= H ? r - H : r)`; with H = 4, row0 = 0 both wraps are taken by every workgroup.  Without them rows -1
   and 4 are the neighbouring images' rows 3 and 0: rows 0 and 3 of every image differ from the reference by O(scale) against
   2e-5 (a), and image 1 alone, whose row -1 is then no image's, differs from image 1 of the batch (c).  A column wrapped by the
   span instead of `Wimg` (the WIDE form, (1, 4, 64) and (1, 4, 96)) shows in a, and in d once the roll moves the seam.
 * F(4x4), `wino43-c64` (3, 8, 64) and `wino43_split-c128` (2, 16, 32): rows row0 + 8 band + 4 s - 1 + i wrapped by H, with H = 8
   (16 in the wide form) again both in every workgroup: a and c as above; the roll by (4, 0) puts another tile row on the wrap (d).
 * direct, `tail-c64` (2, 5, 40): conv_mfma_kernel's 128-pixel tile 1 holds rows 3, 4 of image 0 and rows 0, 1 of image 1; the
   taps' rows are wrapped per pixel and offset by `imgoff = (b - img0) * H * W * Cin`.  A halo row taken from the tile's first
   image, or clamped, changes rows 0 and 4 of both images (a) and makes image 1 differ from the image alone, where it is the
   tile's first (c); the partial tile 3 (pixels 384 .. 399) re-gathers the last pixel for its missing rows.
 * 'down', `down_fused-c64` (3, 2, 64): no halo, but one tile per image: `b = tile / (tiles_x * tiles_y)`, `oy0 = tyi * ROWS`; an
   image or tile-row index off by one reads another image's 2 x 2 patches: a and c ((2, 6, 64) has three tile rows per image and rolls by one of them: d).
 * 'up', `up-c16` (2, 3, 5): window_load clamps iy, ix into the image; every window of these grids is clamped on some side, so a
   window that ran on into the next image's rows instead shows in a and in c.
"""
import pytest
import torch

from block_cases import compare, distance_to_exact, edge_input, exact_block, f44_block, find_block, native_handle, nhwc, oracle_taps, roll_nhwc
from conftest import record_parity
from edges32_cases import CHAINS, GROUPS, cases, rolls, yardstick

pytestmark = pytest.mark.gpu
BAR = 2e-5


def run1(nat, side, i, x_nchw, count=1):
    return nat.run_blocks(side, i, count, nhwc(x_nchw).cuda())


@pytest.mark.parametrize("gid", list(GROUPS))
def test_fp32_block_route_at_its_geometry_edges(amd, oracle, gid):
    """One group: every case on the route the table names, assertions a to d of the module docstring."""
    name, mode, cin, route, _, _ = GROUPS[gid]
    spec, p, _, taps = oracle_taps(oracle, name, "f32")
    nat = native_handle(amd, oracle, name, "f32")
    side, i, blocks, tap_name = find_block(oracle, spec, mode, cin)
    prefix = blocks[i][0]
    wrong_route, bad_ref, bad_batch, bad_roll = [], [], [], []
    pools = {}                                                          # yardstick -> [se_hip, se_yard, elements, max_hip, max_yard, cases]
    for kind, (B, H, W), want in cases(gid):
        case = (kind, B, H, W)
        got_route = nat.block_route(side, i, B, H, W)
        if got_route != want:
            wrong_route.append(case + (got_route,))
        x = edge_input(taps[tap_name], B, H, W)
        y = run1(nat, side, i, x)                                       # an error here (no result) fails the test
        ref = oracle.conv_block(x, p, prefix, mode, spec)
        exact = exact_block(oracle, p, name, x, prefix, mode, spec)
        ok, rel, _ = compare(y, ref, "f32", 1)                          # a
        err64 = float((y.permute(0, 3, 1, 2).cpu().double() - exact).abs().max())
        rel64 = err64 / max(1.0, float(exact.abs().max()))
        if not ok or not rel64 <= BAR:
            bad_ref.append(case + (rel, rel64))
        kind_y = yardstick(got_route)                                   # b, pooled below
        yard = f44_block(oracle, p, x, prefix) if kind_y == "f44" else ref
        rh, rr, mh, mr = distance_to_exact(y, yard, exact)
        pool = pools.setdefault(kind_y, [0.0, 0.0, 0.0, 0.0, 0.0, 0])
        n = float(ref.numel())
        pool[0] += rh * rh * n; pool[1] += rr * rr * n; pool[2] += n
        pool[3], pool[4], pool[5] = max(pool[3], mh), max(pool[4], mr), pool[5] + 1
        record_parity("edges32", group=gid, model=name, block=prefix, cin=cin, case=kind, B=B, H=H, W=W, route=got_route,
                      rel_err=rel, rel_err_vs_fp64=rel64, yardstick=kind_y, rms_ratio_vs_yardstick=rh / rr, max_ratio_vs_yardstick=mh / mr)
        if B > 1:                                                       # c
            if nat.block_route(side, i, 1, H, W) != got_route:
                wrong_route.append(case + ("alone", nat.block_route(side, i, 1, H, W)))
            for b in range(B):
                if not torch.equal(run1(nat, side, i, x[b:b + 1])[0], y[b]):
                    bad_batch.append(case + (b,))
        for (iy, ix), (oy, ox) in rolls(mode, got_route, cin, H, W):    # d
            yr = run1(nat, side, i, torch.roll(x, shifts=(iy, ix), dims=(2, 3)))
            if not torch.equal(yr, roll_nhwc(y, oy, ox)):
                bad_roll.append(case + (iy, ix, float((yr - roll_nhwc(y, oy, ox)).abs().max())))
    over = []
    for kind_y, (se_h, se_r, n_el, mx_h, mx_r, n_cases) in pools.items():
        rms_ratio, max_ratio = (se_h / se_r) ** 0.5, mx_h / mx_r
        record_parity("edges32_pooled", group=gid, model=name, cin=cin, yardstick=kind_y, cases=n_cases, elements=int(n_el),
                      rms_ratio_vs_yardstick=rms_ratio, max_ratio_vs_yardstick=max_ratio, wrong_route=len(wrong_route),
                      failed_ref=len(bad_ref), failed_batch=len(bad_batch), failed_roll=len(bad_roll))
        if not (rms_ratio <= 4.0 and max_ratio <= 4.0):
            over.append((kind_y, rms_ratio, max_ratio))
    assert not wrong_route, wrong_route
    assert not bad_ref, bad_ref
    assert not over, over
    assert not bad_batch, bad_batch
    assert not bad_roll, bad_roll


@pytest.mark.parametrize("route,C", list(CHAINS))
def test_fp32_trunk_chained_pair_at_one_tile_row(amd, oracle, route, C):
    """The chained form of every fp32 trunk route (conv2 + conv3 + the next block's conv1 in one launch) on images of one tile
    row each -- on `tail`, with a partial last pixel tile writing the next block's t1: blocks [i, i + 1] in one run against
    the oracle's block i + 1 on the GPU's own output of block i alone, bar a (fp32 and fp64)."""
    name, shapes = CHAINS[(route, C)]
    spec, p, _, taps = oracle_taps(oracle, name, "f32")
    nat = native_handle(amd, oracle, name, "f32")
    side, i, blocks, tap_name = find_block(oracle, spec, "same", C, pair=True)
    bad = []
    for (B, H, W) in shapes:
        assert nat.block_route(side, i, B, H, W, chained=True) == route and nat.block_route(side, i + 1, B, H, W) == route
        x = edge_input(taps[tap_name], B, H, W)
        y1, y2 = run1(nat, side, i, x), run1(nat, side, i, x, count=2)
        x2 = y1.permute(0, 3, 1, 2).cpu()
        ref2 = oracle.conv_block(x2, p, blocks[i + 1][0], "same", spec)
        exact2 = exact_block(oracle, p, name, x2, blocks[i + 1][0], "same", spec)
        ok, rel, _ = compare(y2, ref2, "f32", 1)
        rel64 = float((y2.permute(0, 3, 1, 2).cpu().double() - exact2).abs().max()) / max(1.0, float(exact2.abs().max()))
        record_parity("edges32_chain", model=name, block=blocks[i + 1][0], cin=C, route=route, B=B, H=H, W=W, rel_err=rel, rel_err_vs_fp64=rel64)
        if not ok or not rel64 <= BAR:
            bad.append((B, H, W, rel, rel64))
    assert not bad, bad
