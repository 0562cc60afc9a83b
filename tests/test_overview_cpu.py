"""CPU: host logic of the overview levels of vqae_amd.reconstruct (canvas shapes per level, what an injected decode_fn is
called with, bands at a level, argument errors) with an injected decode_fn, as tests/test_reconstruct_cpu.py does it for
level 0.  The fake decoder paints every code as an F x F block of pixels and box-reduces the painted tile on the host with the
contract's own arithmetic: reshape to [H/f, f, W/f, f, 3] -> sum as uint32 -> + f*f/2 -> >> 2L."""
import numpy as np
import pytest
import torch

F = 4                                   # the fake model's down-sampling factor: a tile of 8 x 8 codes is 32 x 32 pixels


class _Model:
    factor = F


def _paint(codes):
    c = np.asarray(codes).astype(np.int64)
    px = np.stack([(c * 3 + ch) % 256 for ch in range(3)], -1).astype(np.uint8)
    return px.repeat(F, axis=-3).repeat(F, axis=-2)


def _box(u8, L):
    """the yardstick of the contract on a uint8 picture [H, W, 3]"""
    f = 1 << L
    H, W, _ = u8.shape
    s = u8.reshape(H // f, f, W // f, f, 3).astype(np.uint32).sum(axis=(1, 3), dtype=np.uint32)
    return ((s + np.uint32(f * f // 2)) >> np.uint32(2 * L)).astype(np.uint8)


class _Decode:
    """decode_fn(idx_tiles, rc, canvas[, level]): pastes the painted, box-reduced tiles and keeps what it was called with"""

    def __init__(self):
        self.calls = []

    def __call__(self, idx_tiles, rc, canvas, *level):
        self.calls.append((len(level) + 3, level[0] if level else None, canvas))
        lv = level[0] if level else 0
        pairs = list(zip(lv, canvas)) if isinstance(lv, (tuple, list)) else [(lv, canvas)]
        t = idx_tiles.numpy()
        for L, cv in pairs:
            ph, pw = t.shape[1] * F >> L, t.shape[2] * F >> L
            for k, (r, c) in enumerate(rc.tolist()):
                cv[r * ph:(r + 1) * ph, c * pw:(c + 1) * pw] = torch.from_numpy(_box(_paint(t[k]), L))
        return canvas


def _grid(seed=0, rows=3, cols=5):
    return np.random.RandomState(seed).randint(0, 256, size=(rows * 8, cols * 8)).astype(np.uint8)


@pytest.mark.parametrize("level", [0, 1, 3, 5])
def test_canvas_shape_per_level(amd, level):
    from vqae_amd.reconstruct import reconstruct_region
    grid, dec = _grid(), _Decode()
    out = reconstruct_region(_Model(), grid, 8, batch_size=4, decode_fn=dec, level=level)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.uint8
    assert tuple(out.shape) == (3 * 32 >> level, 5 * 32 >> level, 3)
    # a tile is a multiple of the factor, so reducing the tiles and reducing the picture are the same thing
    assert np.array_equal(out.numpy(), _box(_paint(grid), level))
    part = reconstruct_region(_Model(), grid, 8, r0=1, c0=2, rows=2, cols=3, batch_size=4, decode_fn=_Decode(), level=level)
    assert np.array_equal(part.numpy(), _box(_paint(grid)[32:96, 64:160], level))


def test_tuple_of_levels_gives_a_tuple_from_one_decode_per_batch(amd):
    from vqae_amd.reconstruct import reconstruct_region
    grid, dec = _grid(1), _Decode()
    outs = reconstruct_region(_Model(), grid, 8, batch_size=4, decode_fn=dec, level=(0, 2, 5))
    assert isinstance(outs, tuple) and len(outs) == 3
    for o, L in zip(outs, (0, 2, 5)):
        assert tuple(o.shape) == (3 * 32 >> L, 5 * 32 >> L, 3)
        assert np.array_equal(o.numpy(), _box(_paint(grid), L))
    assert len(dec.calls) == 4                                         # 15 tiles in batches of 4: one call per batch, not per level
    for nargs, level, canvas in dec.calls:
        assert nargs == 4 and level == (0, 2, 5)
        assert isinstance(canvas, tuple) and all(a is b for a, b in zip(canvas, outs))
    one = reconstruct_region(_Model(), grid, 8, decode_fn=_Decode(), level=[3])      # a sequence of one is still a sequence
    assert isinstance(one, tuple) and len(one) == 1 and tuple(one[0].shape) == (12, 20, 3)


def test_decode_fn_gets_three_arguments_at_level_0_and_four_otherwise(amd):
    from vqae_amd.reconstruct import reconstruct_region
    grid = _grid(2)
    for kw, nargs, level in (({}, 3, None), ({"level": 0}, 3, None), ({"level": 2}, 4, 2), ({"level": (0,)}, 4, (0,))):
        dec = _Decode()
        reconstruct_region(_Model(), grid, 8, decode_fn=dec, **kw)
        assert [(c[0], c[1]) for c in dec.calls] == [(nargs, level)], kw


@pytest.mark.parametrize("band_rows", [1, 2])
def test_bands_at_a_level(amd, band_rows):
    from vqae_amd.reconstruct import reconstruct_slide
    grid = _grid(3)
    bands = list(reconstruct_slide(_Model(), grid, 8, band_rows=band_rows, batch_size=4, decode_fn=_Decode(), level=3))
    assert [r0 for r0, _ in bands] == list(range(0, 3, band_rows))
    for r0, band in bands:
        assert isinstance(band, np.ndarray) and band.dtype == np.uint8
        assert band.shape == (min(band_rows, 3 - r0) * 4, 5 * 4, 3)
    assert np.array_equal(np.concatenate([b for _, b in bands]), _box(_paint(grid), 3))
    both = list(reconstruct_slide(_Model(), grid, 8, band_rows=band_rows, decode_fn=_Decode(), level=(1, 4)))
    assert all(isinstance(b, tuple) and len(b) == 2 and all(isinstance(a, np.ndarray) for a in b) for _, b in both)
    for k, L in enumerate((1, 4)):
        assert np.array_equal(np.concatenate([b[k] for _, b in both]), _box(_paint(grid), L))


def test_overview_and_archive_at_a_level(amd, tmp_path):
    from vqae_amd import hdf5
    from vqae_amd.reconstruct import reconstruct_hdf5, reconstruct_overview
    a = _grid(4)
    path = hdf5.write_hdf5(tmp_path / "enc.hdf5", {"images": {"normal_001": a}})
    want = _box(_paint(a), 4)
    dec = _Decode()
    over = reconstruct_overview(_Model(), path, "normal_001", tile=8, level=4, batch_size=4, decode_fn=dec)
    assert isinstance(over, np.ndarray) and over.dtype == np.uint8 and np.array_equal(over, want)
    assert np.array_equal(reconstruct_overview(_Model(), a, tile=8, level=4, decode_fn=_Decode()), want)      # a grid as it is
    np.save(str(tmp_path / "normal_001.npy"), a)
    assert np.array_equal(reconstruct_overview(_Model(), tmp_path / "normal_001.npy", tile=8, level=4, decode_fn=_Decode()), want)
    assert reconstruct_overview(_Model(), a, tile=8, decode_fn=_Decode()).shape == (3, 5, 3)                   # level 5 by default
    bands = list(reconstruct_hdf5(_Model(), path, "normal_001", tile=8, band_rows=2, level=4, decode_fn=_Decode()))
    assert np.array_equal(np.concatenate([b for _, b in bands]), want)


def test_value_errors(amd):
    from vqae_amd.reconstruct import reconstruct_overview, reconstruct_region, reconstruct_slide
    dec, grid = _Decode(), _grid()
    for level in (-1, 7, (1, 7), (-1,), (2, 2), ()):                   # outside 0 .. 6; repeated; none
        with pytest.raises(ValueError):
            reconstruct_region(_Model(), grid, 8, decode_fn=dec, level=level)
    with pytest.raises(ValueError):                                    # 32 x 32-pixel tiles: 64 does not divide them
        reconstruct_region(_Model(), grid, 8, decode_fn=dec, level=6)
    with pytest.raises(ValueError):                                    # 16 x 32-pixel tiles: 32 does not divide the height
        reconstruct_region(_Model(), grid, (4, 8), decode_fn=dec, level=5)
    with pytest.raises(ValueError):
        list(reconstruct_slide(_Model(), grid, 8, decode_fn=dec, level=7))
    with pytest.raises(ValueError):
        reconstruct_overview(_Model(), grid, tile=8, level=6, decode_fn=dec)
    assert dec.calls == []                                             # refused before any tile was decoded


def test_exported_from_the_package(amd):
    assert amd.reconstruct_overview is amd.reconstruct.reconstruct_overview
