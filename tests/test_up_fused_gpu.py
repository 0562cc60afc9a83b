"""The fp32 'up' blocks of cfg B (decoder blocks 51, 57, 63: 128 -> 64, 64 -> 32, 32 -> 16 channels) alone, through the handle's own
dispatch (`run_blocks`), at the smallest low-resolution grids that put a bicubic window on every border, a tile edge of the fused
tail (csrc/up_fused.hip: 8 x 16 output pixels, i.e. 4 x 8 low-resolution ones) at 15 / 16 / 17 and 32 / 33 columns, and a partial last
tile in both directions and in the pixel run of the 1x1 convs.

1. the default route against the one VQAE_NO_UP_HEAD_FUSION=1 gives: bit-equal (a build that does not know the switch compares a
   route with itself);
2. an image of a batch equals the same image run alone, bit for bit;
3. the resize does not depend on where a window lies in its tile: a rolled input gives the rolled output wherever the 4 x 4
   windows touch neither a border nor the seam, and an input that varies along one axis only gives outputs that are equal along
   the other within each parity class (even and odd outputs take different weights, whose rounded sums differ);
4. distance to the block evaluated in fp64 on the CPU (oracle.conv_block): the fp32 bar of test_blocks_gpu.py,
   max |err| <= 2e-5 * max(1, max |ref|).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
UP_BLOCKS = (51, 57, 63)
SHAPES = ((1, 1, 1), (2, 3, 5), (1, 2, 16), (1, 5, 15), (1, 4, 17), (3, 8, 32), (1, 9, 33))
_state = {}


def setup(amd, oracle, monkeypatch):
    """(decoder block list, fp32 parameters, default handle, handle made under VQAE_NO_UP_HEAD_FUSION=1), made once"""
    if not _state:
        spec = oracle.SPECS["B"]
        p = oracle.make_params(spec, 0)
        names = amd.spec.decoder_block_names(amd.SPECS["B"])
        assert [i for i, n in enumerate(names) if n[1] == "up"] == list(UP_BLOCKS)
        fused = amd.NativeVQAE(amd.SPECS["B"], p)
        monkeypatch.setenv("VQAE_NO_UP_HEAD_FUSION", "1")          # read when the handle is made
        plain = amd.NativeVQAE(amd.SPECS["B"], p)
        monkeypatch.delenv("VQAE_NO_UP_HEAD_FUSION")
        _state.update(spec=spec, p=p, names=names, fused=fused, plain=plain, x={}, y={},
                      p64={k: v.double() for k, v in p.items() if torch.is_tensor(v) and v.is_floating_point()})
    return _state


def block_input(st, blk, shape):
    if (blk, shape) not in st["x"]:
        gen = torch.Generator().manual_seed(1000 * blk + 100 * shape[0] + 10 * shape[1] + shape[2])
        st["x"][blk, shape] = torch.randn(*shape, st["names"][blk][2], generator=gen)
    return st["x"][blk, shape]


def block_output(st, blk, shape):
    """the default handle's output at one of SHAPES, computed once and never written to"""
    if (blk, shape) not in st["y"]:
        st["y"][blk, shape] = st["fused"].run_blocks("decoder", blk, 1, block_input(st, blk, shape).cuda())
    return st["y"][blk, shape]


@pytest.mark.parametrize("blk", UP_BLOCKS)
def test_up_head_fused_equals_three_launches_bitwise(amd, oracle, monkeypatch, blk):
    st = setup(amd, oracle, monkeypatch)
    for shape in SHAPES:
        a = block_output(st, blk, shape)
        b = st["plain"].run_blocks("decoder", blk, 1, block_input(st, blk, shape).cuda())
        assert a.shape == (shape[0], 2 * shape[1], 2 * shape[2], st["names"][blk][3])
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        assert torch.equal(a, b), (blk, shape, float((a - b).abs().max()))


@pytest.mark.parametrize("blk", UP_BLOCKS)
def test_up_block_image_of_a_batch_equals_image_alone(amd, oracle, monkeypatch, blk):
    st = setup(amd, oracle, monkeypatch)
    for shape in SHAPES:
        y = block_output(st, blk, shape)
        x = block_input(st, blk, shape)
        for i in range(shape[0]):
            alone = st["fused"].run_blocks("decoder", blk, 1, x[i:i + 1].cuda())
            assert torch.equal(alone[0], y[i]), (blk, shape, i)


@pytest.mark.parametrize("blk", UP_BLOCKS)
def test_up_tail_does_not_depend_on_window_position(amd, oracle, monkeypatch, blk):
    st = setup(amd, oracle, monkeypatch)
    H, W = 12, 40
    x = block_input(st, blk, (1, H, W))
    run = lambda t: st["fused"].run_blocks("decoder", blk, 1, t.cuda())
    y = run(x)
    for dy, dx in ((1, 0), (0, 1), (0, 7), (0, 16), (1, 7)):
        ys = run(torch.roll(x, (dy, dx), (1, 2)))
        # low-resolution pixel (i, j) of the rolled grid is (i - dy, j - dx) of the original; the 4 x 4 window of an output of
        # low-resolution pixel i lies within i - 2 .. i + 2, and must stay behind the seam (i - 2 >= dy) and off the border
        r0, r1, c0, c1 = 2 * (dy + 2), 2 * (H - 2), 2 * (dx + 2), 2 * (W - 2)
        assert r1 - r0 >= 8 and c1 - c0 >= 32
        assert torch.equal(ys[:, r0:r1, c0:c1], y[:, r0 - 2 * dy:r1 - 2 * dy, c0 - 2 * dx:c1 - 2 * dx]), (blk, dy, dx)
    rows_only = run(x[:, :, :1].expand(1, H, W, -1).contiguous())            # depends on the row only
    cols_only = run(x[:, :1].expand(1, H, W, -1).contiguous())               # depends on the column only
    for par in (0, 1):
        cls = rows_only[:, :, par::2]
        assert torch.equal(cls, cls[:, :, :1].expand_as(cls)), (blk, "rows", par)
        cls = cols_only[:, par::2]
        assert torch.equal(cls, cls[:, :1].expand_as(cls)), (blk, "cols", par)
    assert not torch.equal(rows_only[:, 0], rows_only[:, 5]) and not torch.equal(cols_only[:, :, 0], cols_only[:, :, 5])


@pytest.mark.parametrize("blk", UP_BLOCKS)
def test_up_block_distance_to_fp64_block(amd, oracle, monkeypatch, blk):
    st = setup(amd, oracle, monkeypatch)
    prefix, mode = st["names"][blk][:2]
    for shape in SHAPES:
        x = block_input(st, blk, shape)
        ref = oracle.conv_block(x.permute(0, 3, 1, 2).double(), st["p64"], prefix, mode, st["spec"])
        got = block_output(st, blk, shape).permute(0, 3, 1, 2).cpu().double()
        err, scale = float((got - ref).abs().max()), max(1.0, float(ref.abs().max()))
        print(f"up block {blk} {shape}: max|err| {err:.3e}, max|ref| {float(ref.abs().max()):.3e}")
        assert err <= 2e-5 * scale, (blk, shape, err, scale)
