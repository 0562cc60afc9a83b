"""The case table of tests/test_edges32_gpu.py (the fp32 block routes at the edges of their tile geometry) and of
tests/test_edges32_cases_cpu.py (the same cases' inputs, references and yardsticks on the CPU).

Shapes are (B, H, W) of the block's input.  The route names are what `select_route` (csrc/handle.hip) must answer under the
default environment; they follow from the predicates in csrc/:
  fixup_fused   vqae_fixup_same_supported: W % 32 = 0, H % 8 = 0 (C = 8 / 16) or H % 4 = 0 (C = 32); C = 32 only where
                wino_trunk_supported refuses (W no multiple of 128)
  wino          wino_trunk_supported: W a multiple of the workgroup span (32 at C >= 128, 64 at C = 64, 128 at C = 32), H % 4 = 0;
                the exact-width instantiation at one span, WIDE at two or three
  wino43[_split] wino43_supported: W = 64 (C = 64) / 32 (C = 128, 256) exactly, H % 8 = 0; split at C = 128, whose launcher takes the
                16-row ("wide") kernel where H % 16 = 0 and the 8-row one elsewhere
  tail          C = 64 / 128 wherever the Winograd forms refuse: the generic MFMA conv with the fused tail, any H, W >= 1
  same / down   the generic launches: everything else
  down_fused    down_block_supported: cin = 16 / 32 / 64, W % 64 = 0, (H / 2) % r = 0 with r = 4 / 2 / 1 output rows per tile
  up_conv_first_tail / up_conv_first   fp32 'up' blocks, by channels only (up_tail_supported)
"""
from test_edges16_gpu import ROLLS as ROLLS_DIRECT
from test_edges16_gpu import _down
from test_up_fused_gpu import SHAPES as UP_SHAPES

FF8 = ((1, 8, 32), (3, 8, 32), (2, 8, 64), (1, 16, 96), (2, 24, 32))          # 8-row tiles of fixup_fused.hip (C = 8 / 16)
FF8_OUT = {(1, 4, 32): "same", (1, 8, 16): "same"}


def _named(route, shapes):
    return {s: route for s in shapes}


# id -> (model, mode, cin of the block, route of the "in" cases, "in" shapes, {"out" shape: route it must report}).  The block is
# the first one of that mode and width in the model's encoder ('same', 'down') or decoder ('up') list (block_cases.find_block).
GROUPS = {
    "fixup_fused-c8": ("midA", "same", 8, "fixup_fused", FF8, FF8_OUT),
    "fixup_fused-c16": ("mid16", "same", 16, "fixup_fused", FF8, FF8_OUT),
    "fixup_fused-c32": ("mid", "same", 32, "fixup_fused", ((1, 4, 32), (3, 4, 32), (2, 4, 64), (1, 8, 96), (2, 12, 32), (1, 4, 160)),
                        {(1, 2, 32): "same", (1, 4, 16): "same", (1, 4, 128): "wino"}),
    "wino-c64": ("mid", "same", 64, "wino", ((1, 4, 64), (3, 4, 64), (1, 12, 64), (1, 4, 128), (2, 8, 128), (1, 4, 192)),
                 {(1, 8, 64): "wino43", (1, 2, 64): "tail", (1, 4, 32): "tail"}),
    "wino43-c64": ("mid", "same", 64, "wino43", ((1, 8, 64), (3, 8, 64), (2, 16, 64), (1, 24, 64)), {(1, 8, 128): "wino"}),
    "wino-c128": ("mid", "same", 128, "wino", ((1, 4, 32), (3, 4, 32), (1, 12, 32), (1, 4, 64), (2, 8, 64), (1, 4, 96)),
                  {(1, 8, 32): "wino43_split", (1, 2, 32): "tail", (1, 4, 16): "tail"}),
    "wino43_split-c128": ("mid", "same", 128, "wino43_split", ((1, 8, 32), (3, 8, 32), (1, 24, 32), (1, 16, 32), (2, 16, 32)),
                          {(1, 8, 64): "wino"}),
    "wino-c256": ("midC", "same", 256, "wino", ((1, 4, 32), (3, 4, 32), (1, 12, 32), (1, 4, 64), (2, 8, 64)),
                  {(1, 8, 32): "wino43", (1, 2, 32): "same", (2, 3, 24): "same"}),
    "wino43-c256": ("midC", "same", 256, "wino43", ((1, 8, 32), (3, 8, 32), (2, 16, 32), (1, 24, 32)), {(1, 8, 64): "wino"}),
    "tail-c64": ("mid", "same", 64, "tail", ((1, 2, 64), (1, 4, 32), (1, 1, 8), (1, 3, 24), (2, 5, 40)), {(1, 4, 64): "wino"}),
    "tail-c128": ("mid", "same", 128, "tail", ((1, 2, 32), (1, 4, 16), (1, 1, 8), (2, 3, 24), (3, 6, 32)), {(1, 4, 32): "wino"}),
    "same-c8": ("midA", "same", 8, "same", ((1, 4, 32), (1, 1, 8), (2, 3, 20)), {}),
    "same-c256": ("midC", "same", 256, "same", ((1, 2, 32), (1, 1, 8), (2, 3, 24)), {}),
    "down_fused-c16": ("mid16", "down", 16, "down_fused", _down(4)[0], _named("down", _down(4)[1])),
    "down_fused-c32": ("mid", "down", 32, "down_fused", _down(2)[0], _named("down", _down(2)[1])),
    "down_fused-c64": ("midC", "down", 64, "down_fused", _down(1)[0], _named("down", _down(1)[1])),
    "down-c8": ("midA", "down", 8, "down", ((1, 2, 2), (2, 6, 10), (1, 8, 64)), {}),
    "down-c128": ("midC", "down", 128, "down", ((1, 2, 64), (3, 4, 6)), {}),
    "up-c16": ("midA", "up", 16, "up_conv_first_tail", UP_SHAPES, {}),
    "up-c256": ("midC", "up", 256, "up_conv_first", ((1, 1, 1), (2, 3, 5), (1, 4, 17), (1, 9, 33)), {}),
}

# chained pairs at one tile row: (route, C) -> (model, shapes (B, H, W))
CHAINS = {
    ("wino", 64): ("mid", ((3, 4, 64),)),
    ("wino", 128): ("mid", ((3, 4, 32),)),
    ("wino", 256): ("midC", ((3, 4, 32),)),
    ("wino43", 64): ("mid", ((3, 8, 64),)),
    ("wino43_split", 128): ("mid", ((3, 8, 32), (3, 16, 32))),
    ("wino43", 256): ("midC", ((3, 8, 32),)),
    ("tail", 64): ("mid", ((2, 5, 40),)),           # M = 400 and 144 pixels against 128-pixel tiles: the next block's t1 is
    ("tail", 128): ("mid", ((2, 3, 24),)),          # written from a partial last pixel tile
}

F44_ROUTES = ("wino43", "wino43_split")


def cases(gid):
    """[(kind, (B, H, W), route the case must report)] of one group, "in" cases first."""
    _, _, _, route, ins, outs = GROUPS[gid]
    return [("in", s, route) for s in ins] + [("out", s, r) for s, r in outs.items()]


def yardstick(route):
    """Which CPU fp32 evaluation a case's distance to the fp64 block is measured against: the reference's own block, or, on the
    F(4x4, 3x3) routes, the block with conv2 as F(4x4, 3x3) (block_cases.f44_block)."""
    return "f44" if route in F44_ROUTES else "ref32"


def rolls(mode, route, cin, H, W):
    """[((input dy, dx), (output dy, dx))] of assertion d for a case that ran `route`: the 16-bit file's ROLLS on the routes that
    sum an output directly, whole 2 x 2 tiles where conv2 is F(2x2, 3x3) (`wino`, and fixup_fused.hip's C = 16 register
    Winograd), whole 4 x 4 tiles where it is F(4x4, 3x3).  Shifts are taken modulo the image; one that reduces to (0, 0) is
    left out, as is a second one that reduces to the same shift."""
    if mode == "up":
        return []
    if mode == "down":
        cand = ROLLS_DIRECT["down"]
    elif route in F44_ROUTES:
        cand = tuple((s, s) for s in ((4, 0), (0, 4), (0, 28), (4, 36)))
    elif route == "wino" or (route == "fixup_fused" and cin == 16):
        cand = tuple((s, s) for s in ((2, 0), (0, 2), (0, 34), (2, 34)))
    else:
        cand = ROLLS_DIRECT["same"]
    out, seen = [], {(0, 0)}
    for (iy, ix), o in cand:
        key = (iy % H, ix % W)
        if key not in seen:
            seen.add(key)
            out.append((key, o))
    return out
