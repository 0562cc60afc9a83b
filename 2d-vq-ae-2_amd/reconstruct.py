"""The way back: stored code grids -> the uint8 slide pixels they stand for.

`get_encodings` / `save_encodings_hdf5` (extract_embeddings.py) leave one `[th*rows, tw*cols]` code grid per slide under
`images/<stem>`.  The functions here cut such a grid into code tiles on the device (ops.unstitch_tiles, the inverse of the
stitch), decode the tiles (embed_code -> Decoder.forward, vq_ae/model.py:274-291) and paste the de-normalised, rounded and
clamped uint8 pixels of every tile into place (NativeVQAE.decode_indices_u8) -- the tile at patch position (r, c) of the
extraction lands at pixel (r * P, c * P).  The reference model wraps circularly inside a tile, so a faithful
reconstruction has seams between tiles.

Every function takes `level`: the picture at 1/2**level scale (0 .. 6), each pixel the integer mean, rounding half up, of a
2**level-square block of the level-0 pixels, reduced on the device before anything is stored (vqae_pixels_u8_level), so an
overview of a whole slide is one resident canvas and one download (reconstruct_overview).
"""
from pathlib import Path

import numpy as np
import torch

from . import hdf5
from . import ops
from ._lib import MAX_PIXEL_LEVEL


def _tile_hw(tile):
    th, tw = (tile, tile) if isinstance(tile, (int, np.integer)) else tile
    th, tw = int(th), int(tw)
    if th < 1 or tw < 1:
        raise ValueError(f"tile {tile!r}: sides must be positive")
    return th, tw


def _device_grid(grid, decode_fn):
    """The grid as a tensor in its own width, uploaded once (a tensor stays where it is).  Only the injected-decode path
    of the CPU tests may keep it on the host: the product path needs a GPU and says so."""
    if isinstance(grid, torch.Tensor):
        t = grid
    else:
        a = np.asarray(grid)
        if a.dtype == np.bool_:                                    # cast_to_lowest_dtype stores a {0, 1} grid as bool
            a = a.astype(np.uint8)
        elif a.dtype not in (np.uint8, np.uint16, np.int32, np.int64):
            a = a.astype(np.int32 if a.dtype.itemsize <= 2 else np.int64)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2:
        raise ValueError(f"code grid must be 2-D, got shape {tuple(t.shape)}")
    if not t.is_cuda and decode_fn is None:
        t = t.to("cuda")                                           # raises without a GPU: there is no CPU fallback
    return t


def _levels(level, ph, pw):
    """(levels as a list, whether a sequence was given); ValueError for a level outside 0 .. MAX_PIXEL_LEVEL or a factor that
    does not divide the ph x pw pixels of a tile"""
    many = not isinstance(level, (int, np.integer))
    levels = [int(v) for v in level] if many else [int(level)]
    if many and (not levels or len(set(levels)) != len(levels)):
        raise ValueError(f"levels {level!r}: one or more distinct levels")
    for v in levels:
        if not 0 <= v <= MAX_PIXEL_LEVEL:
            raise ValueError(f"level {v} is outside 0 .. {MAX_PIXEL_LEVEL}")
        if ph % (1 << v) or pw % (1 << v):
            raise ValueError(f"level {v}: {1 << v} does not divide the {ph} x {pw} pixels of a tile")
    return levels, many


def _cut(grid, rc, th, tw):
    """code tiles [n, th, tw] at patch positions rc, in the grid's own dtype"""
    if grid.is_cuda:
        return ops.unstitch_tiles(grid, rc, th, tw, dtype=grid.dtype)
    # host logic under test (decode_fn injected, no GPU): plain indexing
    g = grid.view(torch.int16) if grid.dtype == getattr(torch, "uint16", None) else grid
    rcl = rc.long()
    tiles = g.reshape(grid.shape[0] // th, th, grid.shape[1] // tw, tw).permute(0, 2, 1, 3)[rcl[:, 0], rcl[:, 1]]
    return tiles.contiguous().view(grid.dtype)


def _handle(model, autocast_dtype):
    nat = model if hasattr(model, "with_dtype") else model.native()
    return nat if autocast_dtype is None else nat.with_dtype(autocast_dtype)


@torch.no_grad()
def reconstruct_region(model, grid, tile=32, *, r0=0, c0=0, rows=None, cols=None, batch_size=64, autocast_dtype=None,
                       decode_fn=None, level=0):
    """Pixels of the tiles [r0, r0 + rows) x [c0, c0 + cols) of a stored code grid: a uint8 device tensor
    [rows * P_h, cols * P_w, 3] with P = tile * 2**n_down, the pixel size of one tile.

    level: an int L gives the region at 1/f scale, f = 2**L: [rows * P_h / f, cols * P_w / f, 3]; a sequence of distinct
    levels gives a tuple of such canvases, filled by ONE decode per batch.

    grid: numpy array as stored (uint8 / uint16 / wider) or a device tensor; uploaded once, in its own width.
    tile: the latent tile side, or (th, tw); 32 for every shipped configuration (512 / 2**4, 256 / 2**3).
    Tiles are taken row-major in batches of `batch_size` (the last may be short); their positions go up once per call and
    nothing synchronises with the host per batch.
    model: a NativeVQAE or the VQAE mirror, as run_eval takes them.  autocast_dtype=None keeps the handle's own compute
    dtype, a torch dtype selects `with_dtype`.
    decode_fn(idx_tiles, rc, canvas) replaces the HIP decode (CPU tests of the host logic only, like run_eval's encode_fn);
    with a level other than the int 0 it is called as decode_fn(idx_tiles, rc, canvas, level), level as given and canvas a
    tuple when level is a sequence.
    ValueError: grid sides that are not multiples of the tile; a region outside the grid; a level outside 0 .. 6 or one
    whose factor does not divide the tile's pixel size (before anything is allocated)."""
    th, tw = _tile_hw(tile)
    from .extract_embeddings import _factor                        # (the driver module pulls in the loader machinery: on first use)
    f = _factor(model)
    levels, many = _levels(level, th * f, tw * f)                   # refused before the grid goes up
    g = _device_grid(grid, decode_fn)
    gh, gw = int(g.shape[0]), int(g.shape[1])
    if gh % th or gw % tw or gh == 0 or gw == 0:
        raise ValueError(f"code grid {gh} x {gw} is not a whole number of {th} x {tw} tiles")
    R, C = gh // th, gw // tw
    rows = R - r0 if rows is None else rows
    cols = C - c0 if cols is None else cols
    if r0 < 0 or c0 < 0 or rows < 1 or cols < 1 or r0 + rows > R or c0 + cols > C:
        raise ValueError(f"region rows [{r0}, {r0 + rows}) x cols [{c0}, {c0 + cols}) is outside the {R} x {C}-tile grid")
    if batch_size < 1:
        raise ValueError(f"batch_size {batch_size}")
    canvases = tuple(torch.empty((rows * th * f >> v, cols * tw * f >> v, 3), dtype=torch.uint8, device=g.device) for v in levels)
    canvas = canvases if many else canvases[0]
    extra = () if not many and levels[0] == 0 else (level,)
    decode = decode_fn or _handle(model, autocast_dtype).decode_indices_u8
    # row-major positions: [0] in the grid (where to cut), [1] in the canvas (where to paste); one upload
    rr, cc = np.divmod(np.arange(rows * cols, dtype=np.int32), np.int32(cols))
    rc_host = torch.from_numpy(np.stack([np.stack([rr + r0, cc + c0], 1), np.stack([rr, cc], 1)]).astype(np.int32))
    if g.is_cuda:
        rc_host = rc_host.pin_memory()
    rc = rc_host.to(g.device, non_blocking=True)
    for lo in range(0, rows * cols, batch_size):
        hi = min(lo + batch_size, rows * cols)
        decode(_cut(g, rc[0, lo:hi], th, tw), rc[1, lo:hi], canvas, *extra)
    return canvas


def reconstruct_slide(model, grid, tile=32, *, band_rows=1, **kw):
    """Generator of (r0, band): the slide in bands of `band_rows` tile rows, each a host uint8 array
    [band_rows * P_h, cols * P_w, 3] (the last band may be lower) -- for slides whose pixels do not fit in device memory
    (200 x 400 tiles of 512 x 512 pixels are 63 GB).  The grid goes up once; every band is one reconstruct_region (whose
    keyword arguments pass through, `level` among them: the bands are then [band_rows * P_h / f, ...], or tuples of arrays
    for a sequence of levels) and one synchronous download."""
    if band_rows < 1:
        raise ValueError(f"band_rows {band_rows}")
    th, _ = _tile_hw(tile)
    g = _device_grid(grid, kw.get("decode_fn"))
    if g.shape[0] % th or g.shape[0] == 0:
        raise ValueError(f"code grid of {g.shape[0]} rows is not a whole number of {th}-row tiles")
    R = int(g.shape[0]) // th
    for r0 in range(0, R, band_rows):
        band = reconstruct_region(model, g, tile, r0=r0, rows=min(band_rows, R - r0), **kw)
        yield r0, tuple(b.cpu().numpy() for b in band) if isinstance(band, tuple) else band.cpu().numpy()


def _read_grid(path, name):
    if Path(path).suffix == ".npy":
        return np.load(str(path), allow_pickle=False)
    return hdf5.read_hdf5(path)["images"][name]


def reconstruct_hdf5(model, path, name, **kw):
    """reconstruct_slide over the grid `images/<name>` of an archive written by save_encodings_hdf5 / convert_npy_to_hdf5
    (read with this package's own reader), or over a `<name>.npy` file of save_encodings given as `path`."""
    return reconstruct_slide(model, _read_grid(path, name), **kw)


def reconstruct_overview(model, grid_or_path, name=None, *, tile=32, level=5, **kw):
    """The whole slide at one level as a host uint8 array [R * P_h / f, C * P_w / f, 3]: one reconstruct_region whose canvas
    stays on the device (at level 5 a 200 x 400-tile slide of 512 x 512 tiles is 62 MB) and one download.  grid_or_path: a
    code grid (array or device tensor), or the path of an archive / `.npy` file as reconstruct_hdf5 takes it, with `name`.
    Keyword arguments pass through to reconstruct_region."""
    grid = _read_grid(grid_or_path, name) if isinstance(grid_or_path, (str, Path)) else grid_or_path
    out = reconstruct_region(model, grid, tile, level=level, **kw)
    return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()
