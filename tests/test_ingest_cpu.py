"""CPU: the numpy restatements of the ingest kernels against hand-written loops, and the host logic of vqae_amd.ingest (tile
order, dropped partial tiles, regions, bands, archive layout, argument errors) with an injected encode_fn, the way
tests/test_reconstruct_cpu.py injects decode_fn.  The fake encoder returns, for every tile, a hash of the tile's bytes plus
the position inside the code tile, so a misplaced, transposed or mis-cut tile shows in the grid."""
import zlib

import numpy as np
import pytest
import torch

F = 4                                   # the fake model's down-sampling factor: tile 8 -> patches of 32 pixels
TH = 8
P = TH * F


class _Model:                           # what encode_region asks of a model when the encode is injected
    factor = F


def _hash_tile(tile_u8):
    """uint8 [P, P, 3] -> int64 [TH, TH]"""
    h = zlib.crc32(np.ascontiguousarray(tile_u8).tobytes()) % 50000
    return (h + np.arange(TH * TH, dtype=np.int64).reshape(TH, TH)) % 60000


class _Encode:
    """encode_fn(tiles_u8): hashes every tile and keeps what it was called with"""

    def __init__(self):
        self.calls = []

    def __call__(self, tiles):
        assert isinstance(tiles, torch.Tensor) and tiles.dtype == torch.uint8 and tuple(tiles.shape[1:]) == (P, P, 3)
        t = tiles.numpy()
        self.calls.append(t.copy())
        return torch.from_numpy(np.stack([_hash_tile(x) for x in t]))


def _canvas(h, w, seed=0):
    rs = np.random.RandomState(seed)
    pixels = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    mask = (rs.random_sample((h, w)) < 0.02).astype(np.uint8) * rs.randint(1, 3, size=(h, w)).astype(np.uint8)
    return pixels, mask


def _want_grid(pixels, rows, cols, y0=0, x0=0):
    out = np.zeros((rows * TH, cols * TH), np.int64)
    for r in range(rows):
        for c in range(cols):
            out[r * TH:(r + 1) * TH, c * TH:(c + 1) * TH] = _hash_tile(pixels[y0 + r * P:y0 + (r + 1) * P, x0 + c * P:x0 + (c + 1) * P])
    return out


def _want_labels(mask, rows, cols, y0=0, x0=0, win=F):
    out = np.zeros((rows * TH, cols * TH), np.uint8)
    for Y in range(out.shape[0]):
        for X in range(out.shape[1]):
            out[Y, X] = mask[y0 + Y * win:y0 + (Y + 1) * win, x0 + X * win:x0 + (X + 1) * win].max()
    return out


# ---- 1. the restatements against loops -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_cut_pixels_reference_against_loops(amd, ch, level):
    f = 1 << level
    h, w, y0, x0 = 3, 2, 1, 2
    canvas = np.random.RandomState(level).randint(0, 256, size=(1 + 2 * h * f + 1, 2 + 3 * w * f, ch)).astype(np.uint8)
    rc = np.array([(1, 2), (0, 0), (2, 0), (0, 3), (-1, 0), (1, 1)], np.int32)        # (2, 0), (0, 3), (-1, 0): outside
    out = np.full((len(rc), h, w, ch), 9, np.uint8)
    got = amd.ops.cut_pixels_reference(canvas, rc, h, w, y0=y0, x0=x0, level=level, out=out)
    assert got is out
    want = np.full_like(out, 9)
    for t, (r, c) in enumerate(rc):
        if t in (2, 3, 4):
            continue
        for y in range(h):
            for x in range(w):
                for k in range(ch):
                    s = 0
                    for dy in range(f):
                        for dx in range(f):
                            s += int(canvas[y0 + (r * h + y) * f + dy, x0 + (c * w + x) * f + dx, k])
                    want[t, y, x, k] = (s + f * f // 2) >> (2 * level)
    assert np.array_equal(got, want)


def test_cut_pixels_reference_rounds_half_up(amd):
    canvas = np.zeros((2, 4, 1), np.uint8)
    canvas[0, 0] = canvas[0, 1] = 255                                                  # mean 127.5 -> 128
    canvas[:, 2:] = 255                                                                # mean 255 stays 255
    got = amd.ops.cut_pixels_reference(canvas, np.array([(0, 0)]), 1, 2, level=1)
    assert got.reshape(-1).tolist() == [128, 255]


def test_pool_labels_reference_against_loops(amd):
    mask = np.random.RandomState(0).randint(0, 3, size=(11, 14)).astype(np.uint8)
    got = amd.ops.pool_labels_reference(mask, (2, 3), y0=1, x0=2)
    assert got.shape == (5, 4) and got.dtype == np.uint8
    for Y in range(5):
        for X in range(4):
            assert got[Y, X] == mask[1 + 2 * Y:3 + 2 * Y, 2 + 3 * X:5 + 3 * X].max()
    assert np.array_equal(amd.ops.pool_labels_reference(mask, 1), mask)
    with pytest.raises(AssertionError):
        amd.ops.pool_labels_reference(mask, 4, out_hw=(3, 3))


def test_ops_refuse_cpu_tensors(amd):
    with pytest.raises(amd._lib.VqaeHipError):
        amd.ops.cut_pixels_u8(torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((1, 2), dtype=torch.int32), 4, 4)
    with pytest.raises(amd._lib.VqaeHipError):
        amd.ops.pool_labels_u8(torch.zeros((8, 8), dtype=torch.uint8), 4)


def test_library_argument_errors_without_gpu(amd):
    """the library judges its arguments before it launches anything"""
    import ctypes
    L = amd._lib
    lib = L.lib()
    one = ctypes.c_void_p(16)           # never dereferenced: validation fails first
    with pytest.raises(AssertionError):                                                # two channels
        L.check(lib.vqae_cut_pixels_u8(one, 64, 64, 2, one, 1, 8, 8, 0, 0, 0, one, None))
    with pytest.raises(NotImplementedError):                                           # a level above the maximum
        L.check(lib.vqae_cut_pixels_u8(one, 64, 64, 3, one, 1, 8, 8, 0, 0, L.MAX_PIXEL_LEVEL + 1, one, None))
    with pytest.raises(AssertionError):                                                # a negative level / origin
        L.check(lib.vqae_cut_pixels_u8(one, 64, 64, 3, one, 1, 8, 8, 0, 0, -1, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_cut_pixels_u8(one, 64, 64, 3, one, 1, 8, 8, -1, 0, 0, one, None))
    with pytest.raises(AssertionError):                                                # no tile fits from the origin
        L.check(lib.vqae_cut_pixels_u8(one, 64, 64, 3, one, 1, 8, 8, 60, 0, 0, one, None))
    with pytest.raises(AssertionError):                                                # null pointers
        L.check(lib.vqae_cut_pixels_u8(None, 64, 64, 3, None, 1, 8, 8, 0, 0, 0, None, None))
    assert lib.vqae_cut_pixels_u8(None, 64, 64, 3, None, 0, 8, 8, 0, 0, 0, None, None) == 0     # n_tiles == 0: nothing to do
    with pytest.raises(AssertionError):                                                # a window reaching outside the mask
        L.check(lib.vqae_pool_labels_u8(one, 64, 64, 0, 1, 4, 4, one, 16, 16, None))
    assert b"outside" in lib.vqae_last_error()
    with pytest.raises(AssertionError):
        L.check(lib.vqae_pool_labels_u8(None, 64, 64, 0, 0, 4, 4, None, 16, 16, None))


# ---- 2. host logic of encode_region / encode_slide -------------------------------------------------------------------
def test_region_row_major_and_partial_tiles_dropped(amd):
    pixels, mask = _canvas(70, 101)                                                    # 2 x 3 whole tiles of 32, the rest dropped
    enc = _Encode()
    grid, labels = amd.encode_region(_Model(), pixels, mask, TH, batch_size=4, encode_fn=enc)
    assert tuple(grid.shape) == (2 * TH, 3 * TH) and tuple(labels.shape) == (2 * TH, 3 * TH) and labels.dtype == torch.uint8
    assert np.array_equal(grid.numpy(), _want_grid(pixels, 2, 3))
    assert np.array_equal(labels.numpy(), _want_labels(mask, 2, 3))
    assert labels.numpy().max() >= 1
    # 6 tiles in batches of 4: 4 + 2, row-major
    assert [len(c) for c in enc.calls] == [4, 2]
    tiles = np.concatenate(enc.calls)
    for k, (r, c) in enumerate((r, c) for r in range(2) for c in range(3)):
        assert np.array_equal(tiles[k], pixels[r * P:(r + 1) * P, c * P:(c + 1) * P]), (r, c)
    # no mask: no labels; a host tensor is taken like an array
    g2, l2 = amd.encode_region(_Model(), torch.from_numpy(pixels), None, (TH, TH), encode_fn=_Encode())
    assert l2 is None and torch.equal(g2, grid)


def test_sub_region_equals_the_slice_of_the_full_result(amd):
    pixels, mask = _canvas(3 * P + 6, 4 * P + 5, seed=1)
    full, full_l = amd.encode_region(_Model(), pixels, mask, TH, encode_fn=_Encode())
    part, part_l = amd.encode_region(_Model(), pixels, mask, TH, y0=P, x0=2 * P, rows=2, cols=2, batch_size=3, encode_fn=_Encode())
    assert torch.equal(part, full[TH:3 * TH, 2 * TH:4 * TH]) and torch.equal(part_l, full_l[TH:3 * TH, 2 * TH:4 * TH])
    # an origin that is no multiple of the tile: rows / cols default to what is left
    off, off_l = amd.encode_region(_Model(), pixels, mask, TH, y0=5, x0=3, encode_fn=_Encode())
    assert tuple(off.shape) == (3 * TH, 4 * TH)
    assert np.array_equal(off.numpy(), _want_grid(pixels, 3, 4, 5, 3)) and np.array_equal(off_l.numpy(), _want_labels(mask, 3, 4, 5, 3))


def test_region_level_reads_the_box_filtered_canvas(amd):
    pixels, mask = _canvas(2 * P * 2 + 3, 3 * P * 2 + 1, seed=2)
    grid, labels = amd.encode_region(_Model(), pixels, mask, TH, level=1, encode_fn=_Encode())
    assert tuple(grid.shape) == (2 * TH, 3 * TH)
    box = pixels[:4 * P, :6 * P].astype(np.uint32).reshape(2 * P, 2, 3 * P, 2, 3).sum(axis=(1, 3))
    small = ((box + 2) >> 2).astype(np.uint8)
    assert np.array_equal(grid.numpy(), _want_grid(small, 2, 3))
    assert np.array_equal(labels.numpy(), _want_labels(mask, 2, 3, win=2 * F))


@pytest.mark.parametrize("band_rows", [1, 2, 5])
def test_slide_bands_equal_one_region(amd, band_rows, tmp_path):
    from vqae_amd.extract_embeddings import cast_to_lowest_dtype
    pixels, mask = _canvas(3 * P + 6, 2 * P + 5, seed=3)
    want, want_l = amd.encode_region(_Model(), pixels, mask, TH, encode_fn=_Encode())
    enc = _Encode()
    grid, labels = amd.encode_slide(_Model(), pixels, mask, TH, band_rows=band_rows, batch_size=3, encode_fn=enc)
    assert isinstance(grid, np.ndarray) and isinstance(labels, np.ndarray)
    assert np.array_equal(grid, want.numpy()) and grid.dtype == cast_to_lowest_dtype(want.numpy()).dtype == np.uint16
    assert np.array_equal(labels, want_l.numpy()) and labels.dtype == np.uint8                  # values {0, 1, 2}
    assert sum(len(c) for c in enc.calls) == 6
    # a memmap is walked band by band like an array; a {0, 1} mask comes back as bool
    mm = np.lib.format.open_memmap(tmp_path / "slide.npy", mode="w+", dtype=np.uint8, shape=pixels.shape)
    mm[:] = pixels
    mm.flush()
    g2, l2 = amd.encode_slide(_Model(), np.load(tmp_path / "slide.npy", mmap_mode="r"), np.minimum(mask, 1), TH, band_rows=band_rows,
                              encode_fn=_Encode())
    assert np.array_equal(g2, grid) and l2.dtype == np.bool_ and np.array_equal(l2, want_l.numpy() > 0)
    g3, l3 = amd.encode_slide(_Model(), pixels, None, TH, band_rows=band_rows, y0=P, rows=2, cols=1, encode_fn=_Encode())
    assert l3 is None and np.array_equal(g3, want.numpy()[TH:3 * TH, :TH])


def test_value_errors_before_anything_is_encoded(amd):
    pixels, mask = _canvas(70, 101)
    enc = _Encode()
    bad = [dict(y0=40), dict(x0=80), dict(rows=3), dict(cols=4), dict(y0=-1), dict(rows=0),      # a region outside the canvas
           dict(level=7), dict(level=-1), dict(level=1, rows=2),                                  # a bad level; 2 rows of 64 in 70
           dict(batch_size=0)]
    for fn in (amd.encode_region, amd.encode_slide):
        for kw in bad:
            with pytest.raises(ValueError):
                fn(_Model(), pixels, mask, TH, encode_fn=enc, **kw)
        with pytest.raises(ValueError):                                                # a mask of another shape
            fn(_Model(), pixels, mask[:, :100], TH, encode_fn=enc)
        with pytest.raises(ValueError):                                                # a canvas smaller than one tile
            fn(_Model(), pixels[:31], None, TH, encode_fn=enc)
        with pytest.raises(ValueError):                                                # not [H, W, 3]
            fn(_Model(), pixels[:, :, :1], None, TH, encode_fn=enc)
    with pytest.raises(ValueError):
        amd.encode_slide(_Model(), pixels, mask, TH, band_rows=0, encode_fn=enc)
    assert enc.calls == []


def test_encode_arrays_hdf5_round_trip(amd, tmp_path):
    from vqae_amd import hdf5
    slides = [("slide_000", *_canvas(3 * P, 2 * P, seed=4)), ("tumor_001", _canvas(2 * P + 1, 3 * P, seed=5)[0], None),
              ("slide_002", _canvas(P, P, seed=6)[0], np.minimum(_canvas(P, P, seed=6)[1], 1))]
    path = amd.encode_arrays_hdf5(tmp_path / "slides.hdf5", _Model(), iter(slides), tile=TH, band_rows=2, encode_fn=_Encode())
    got = hdf5.read_hdf5(path)
    assert sorted(got.keys()) == ["images", "masks"]
    assert sorted(got["images"].keys()) == ["slide_000", "slide_002", "tumor_001"]
    assert sorted(got["masks"].keys()) == ["slide_000_mask", "slide_002_mask"]         # the names of save_encodings_hdf5
    for stem, pixels, mask in slides:
        grid, labels = amd.encode_slide(_Model(), pixels, mask, TH, encode_fn=_Encode())
        g = np.asarray(got["images"][stem])
        assert g.dtype == grid.dtype and np.array_equal(g, grid)
        if mask is not None:
            m = np.asarray(got["masks"][stem + "_mask"])
            assert m.dtype == labels.dtype and np.array_equal(m, labels)
    assert np.asarray(got["masks"]["slide_002_mask"]).dtype == np.bool_ and np.asarray(got["masks"]["slide_000_mask"]).dtype == np.uint8
