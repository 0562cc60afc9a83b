"""CPU: host logic of vqae_amd.reconstruct (tile order, batching, regions, bands, archive reading, argument errors) with an
injected decode_fn, the way tests/test_driver_cpu.py injects encode_fn / stitch_fn.  The fake decoder paints every code as
an F x F block of pixels whose value depends on the code and the channel, so a misplaced, transposed or mis-widened tile
shows in the picture."""
import numpy as np
import pytest
import torch

F = 2                                   # the fake model's down-sampling factor: a code is an F x F block of pixels


class _Model:                           # what reconstruct_region asks of a model when the decode is injected
    factor = F


def _paint(codes):
    """codes [..., h, w] (any integer dtype, numpy) -> uint8 pixels [..., h*F, w*F, 3]"""
    c = np.asarray(codes).astype(np.int64)
    px = np.stack([(c * 3 + ch) % 256 for ch in range(3)], -1).astype(np.uint8)
    return px.repeat(F, axis=-3).repeat(F, axis=-2)


class _Decode:
    """decode_fn(idx_tiles, rc, canvas): pastes the painted tiles and keeps what it was called with"""

    def __init__(self):
        self.calls = []

    def __call__(self, idx_tiles, rc, canvas):
        t = idx_tiles.view(torch.int16).numpy().view(np.uint16) if idx_tiles.dtype == torch.uint16 else idx_tiles.numpy()
        self.calls.append((idx_tiles.dtype, tuple(idx_tiles.shape), rc.numpy().copy()))
        ph, pw = t.shape[1] * F, t.shape[2] * F
        for k, (r, c) in enumerate(rc.tolist()):
            canvas[r * ph:(r + 1) * ph, c * pw:(c + 1) * pw] = torch.from_numpy(_paint(t[k]))
        return canvas


def _grid(dtype, rows=3, cols=5, th=8, tw=8, seed=0):
    hi = 256 if dtype == np.uint8 else 1000                       # uint16: codes that do not fit a byte
    return np.random.RandomState(seed).randint(0, hi, size=(rows * th, cols * tw)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_region_row_major_batches_with_ragged_tail(amd, dtype):
    from vqae_amd.reconstruct import reconstruct_region
    grid, dec = _grid(dtype), _Decode()
    out = reconstruct_region(_Model(), grid, 8, batch_size=4, decode_fn=dec)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3 * 8 * F, 5 * 8 * F, 3)
    assert np.array_equal(out.numpy(), _paint(grid))
    # 15 tiles in batches of 4: 4 + 4 + 4 + 3, row-major, in the grid's own width
    assert [c[1] for c in dec.calls] == [(4, 8, 8)] * 3 + [(3, 8, 8)]
    assert all(c[0] == (torch.uint8 if dtype == np.uint8 else torch.uint16) for c in dec.calls)
    rc = np.concatenate([c[2] for c in dec.calls])
    assert rc.dtype == np.int32 and np.array_equal(rc, [(r, c) for r in range(3) for c in range(5)])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_region_inside_the_grid(amd, dtype):
    from vqae_amd.reconstruct import reconstruct_region
    grid, dec = _grid(dtype, seed=1), _Decode()
    out = reconstruct_region(_Model(), grid, 8, r0=1, c0=2, rows=2, cols=3, batch_size=4, decode_fn=dec)
    P = 8 * F
    assert np.array_equal(out.numpy(), _paint(grid)[1 * P:3 * P, 2 * P:5 * P])
    assert [c[1][0] for c in dec.calls] == [4, 2]
    # positions handed to the decoder are relative to the canvas of the region
    assert np.array_equal(np.concatenate([c[2] for c in dec.calls]), [(r, c) for r in range(2) for c in range(3)])
    # rows / cols default to the rest of the grid; a device-resident (here: host) tensor is taken as it is
    rest = reconstruct_region(_Model(), torch.from_numpy(grid), 8, r0=2, c0=4, decode_fn=_Decode())
    assert np.array_equal(rest.numpy(), _paint(grid)[2 * P:, 4 * P:])


def test_region_rectangular_tiles_and_wide_grids(amd):
    from vqae_amd.reconstruct import reconstruct_region
    grid = np.random.RandomState(2).randint(0, 70000, size=(2 * 4, 3 * 8)).astype(np.int64)
    for g in (grid, grid.astype(np.int32), grid.astype(np.uint32)):
        out = reconstruct_region(_Model(), g, (4, 8), batch_size=64, decode_fn=_Decode())
        assert np.array_equal(out.numpy(), _paint(grid))
    out = reconstruct_region(_Model(), (grid % 2).astype(bool), (4, 8), decode_fn=_Decode())     # cast_to_lowest_dtype's {0, 1} case
    assert np.array_equal(out.numpy(), _paint(grid % 2))


@pytest.mark.parametrize("band_rows", [1, 2])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_slide_bands(amd, band_rows, dtype):
    from vqae_amd.reconstruct import reconstruct_slide
    grid = _grid(dtype, seed=3)
    bands = list(reconstruct_slide(_Model(), grid, 8, band_rows=band_rows, batch_size=4, decode_fn=_Decode()))
    assert [r0 for r0, _ in bands] == list(range(0, 3, band_rows))
    P = 8 * F
    for r0, band in bands:
        assert isinstance(band, np.ndarray) and band.dtype == np.uint8
        assert band.shape == (min(band_rows, 3 - r0) * P, 5 * P, 3)
    assert np.array_equal(np.concatenate([b for _, b in bands]), _paint(grid))
    # keyword arguments reach reconstruct_region: a column window of every band
    cols = list(reconstruct_slide(_Model(), grid, 8, band_rows=band_rows, c0=1, cols=2, decode_fn=_Decode()))
    assert np.array_equal(np.concatenate([b for _, b in cols]), _paint(grid)[:, 1 * P:3 * P])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_archive_read_back_by_name(amd, tmp_path, dtype):
    from vqae_amd import hdf5
    from vqae_amd.reconstruct import reconstruct_hdf5
    a, b = _grid(dtype, seed=4), _grid(dtype, rows=2, cols=2, seed=5)
    path = hdf5.write_hdf5(tmp_path / "enc.hdf5", {"images": {"normal_001": a, "tumor_002": b},
                                                   "masks": {"normal_001_mask": np.zeros_like(a)}})
    for name, g in (("normal_001", a), ("tumor_002", b)):
        bands = list(reconstruct_hdf5(_Model(), path, name, tile=8, band_rows=2, batch_size=4, decode_fn=_Decode()))
        assert np.array_equal(np.concatenate([x for _, x in bands]), _paint(g))
    with pytest.raises(KeyError):
        list(reconstruct_hdf5(_Model(), path, "no_such_slide", tile=8, decode_fn=_Decode()))
    np.save(str(tmp_path / "tumor_002.npy"), b)
    bands = list(reconstruct_hdf5(_Model(), tmp_path / "tumor_002.npy", "tumor_002", tile=8, decode_fn=_Decode()))
    assert [r0 for r0, _ in bands] == [0, 1] and np.array_equal(np.concatenate([x for _, x in bands]), _paint(b))


def test_value_errors(amd):
    from vqae_amd.reconstruct import reconstruct_region, reconstruct_slide
    dec = _Decode()
    for shape in ((3 * 8 + 1, 5 * 8), (3 * 8, 5 * 8 - 3)):             # sides that are not multiples of the tile
        with pytest.raises(ValueError):
            reconstruct_region(_Model(), np.zeros(shape, np.uint8), 8, decode_fn=dec)
    with pytest.raises(ValueError):
        list(reconstruct_slide(_Model(), np.zeros((3 * 8 + 1, 5 * 8), np.uint8), 8, decode_fn=dec))
    grid = _grid(np.uint8)
    for kw in (dict(r0=3), dict(c0=5), dict(r0=-1), dict(r0=2, rows=2), dict(c0=3, cols=3), dict(rows=0), dict(rows=4)):
        with pytest.raises(ValueError):                                # a region outside the 3 x 5-tile grid
            reconstruct_region(_Model(), grid, 8, decode_fn=dec, **kw)
    assert dec.calls == []                                             # refused before any tile was decoded


def test_exported_from_the_package(amd):
    assert amd.reconstruct_region is amd.reconstruct.reconstruct_region
    assert amd.reconstruct_slide is amd.reconstruct.reconstruct_slide
    assert amd.reconstruct_hdf5 is amd.reconstruct.reconstruct_hdf5

