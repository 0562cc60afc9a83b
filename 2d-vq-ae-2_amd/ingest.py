"""The way in: uint8 slide pixels that are already an array -> the code grid and the label grid of the extraction.

`run_eval` / `get_encodings` (extract_embeddings.py) read tiles one item at a time from a Dataset with the contract of
CAMELYON16SlicePatchDataSet (datamodules/camelyon16.py:149-211): worker processes, per-tile collation, page-locked batch
slots.  For a slide that is an array -- a `.npy` / np.memmap (the bands reconstruct_hdf5 writes, for one), an HDF5 pixel
dataset, a tensor on the device -- nothing needs doing per tile on the host: a band of tile rows is one contiguous slab,
one copy takes it to the device, and there the tiles are cut (ops.cut_pixels_u8), normalised and encoded
(NativeVQAE.encode_u8), stitched (ops.stitch_tiles) and the mask pooled into labels (ops.pool_labels_u8).  The layout is
get_encodings': the tile at patch position (r, c) is the patch at pixel (r * P, c * P), P = tile * 2**n_down, partial tiles
at the right and bottom edges are dropped (`_sizes = shape // patch_size`), and the label of a code is the maximum of the
mask over the 2**n_down-square block of pixels it stands for (extract_embeddings.py:127-130).

`level` L reads the slide at 1/2**L scale: every model pixel is the integer mean, rounding half up, of a 2**L-square block of
source pixels (the rule of reconstruct's `level`), so one tile covers P * 2**L source pixels and a label a (2**n_down * 2**L)-
square block of the mask.  encode_region is the inverse of reconstruct_region in layout, `level` included.

One process, one GPU: sharding this path over several GPUs is out of scope here (bands of one slide are independent, so a
caller may hand different slides or regions to different processes).
"""
import numpy as np
import torch

from . import hdf5
from . import ops
from ._lib import MAX_PIXEL_LEVEL
from .reconstruct import _tile_hw


class _Plan:
    """The geometry of one call, checked before anything is allocated."""

    def __init__(self, model, shape, mask_shape, tile, y0, x0, rows, cols, level, batch_size):
        from .extract_embeddings import _factor                    # (the driver module pulls in the loader machinery: on first use)
        self.th, self.tw = _tile_hw(tile)
        self.factor = _factor(model)
        if not isinstance(level, (int, np.integer)) or not 0 <= level <= MAX_PIXEL_LEVEL:
            raise ValueError(f"level {level!r} is outside 0 .. {MAX_PIXEL_LEVEL}")
        self.level, self.f = int(level), 1 << int(level)
        if len(shape) != 3 or shape[2] != 3:
            raise ValueError(f"pixels must be [H, W, 3], got shape {tuple(shape)}")
        self.H, self.W = int(shape[0]), int(shape[1])
        if mask_shape is not None and tuple(mask_shape) != (self.H, self.W):
            raise ValueError(f"mask of shape {tuple(mask_shape)} for pixels of {self.H} x {self.W}")
        if batch_size < 1:
            raise ValueError(f"batch_size {batch_size}")
        self.batch_size = int(batch_size)
        self.ph, self.pw = self.th * self.factor, self.tw * self.factor          # a tile in model pixels
        self.sh, self.sw = self.ph * self.f, self.pw * self.f                    # ... in source pixels
        self.win = self.factor * self.f                                          # source pixels per code, each way
        if y0 < 0 or x0 < 0:
            raise ValueError(f"origin ({y0}, {x0}) is outside the {self.H} x {self.W} canvas")
        self.y0, self.x0 = int(y0), int(x0)
        self.rows = (self.H - self.y0) // self.sh if rows is None else int(rows)
        self.cols = (self.W - self.x0) // self.sw if cols is None else int(cols)
        if self.rows < 1 or self.cols < 1 or self.y0 + self.rows * self.sh > self.H or self.x0 + self.cols * self.sw > self.W:
            raise ValueError(f"region of {self.rows} x {self.cols} tiles of {self.sh} x {self.sw} pixels at ({self.y0}, {self.x0}) "
                             f"does not lie inside the {self.H} x {self.W} canvas")


def _encoder(model, autocast_dtype, encode_fn):
    """(encode(tiles_u8) -> idx [n, th, tw], the grid's dtype or None when only the first batch can tell): the model resolved
    as run_eval resolves it, the codes in the compact width run_eval(compact=True) chooses"""
    from .extract_embeddings import _COMPACT, _encode, _num_codes
    n_codes = _num_codes(model) if model is not None else None
    dtype = None if n_codes is None else _COMPACT[1 if n_codes <= 256 else (2 if n_codes <= 65536 else 4)]
    if encode_fn is not None:
        return encode_fn, dtype
    assert dtype is not None, "encode_region: the model has no spec to read the codebook size from"
    if hasattr(model, "with_dtype"):                               # NativeVQAE: codes leave the VQ kernel already compact
        nat = model.with_dtype(autocast_dtype)
        return (lambda x: nat.encode_u8(x, idx_dtype=dtype)[1]), dtype
    return (lambda x: _encode(model, x, autocast_dtype)), dtype


def _positions(rows, cols, device):
    """row-major patch positions [rows * cols, 2] int32 on `device`: one upload, page-locked when it goes to a GPU"""
    rr, cc = np.divmod(np.arange(rows * cols, dtype=np.int32), np.int32(cols))
    rc = torch.from_numpy(np.stack([rr, cc], 1).astype(np.int32))
    if device.type != "cuda":
        return rc
    return rc.pin_memory().to(device, non_blocking=True)


class _Run:
    """Encodes regions of device canvases into a resident code grid (and label grid): what encode_region does once and
    encode_slide once per band.  Tiles are taken row-major in batches of batch_size through one reused tile buffer; nothing
    here synchronises with the host."""

    def __init__(self, plan, enc, grid_dtype, grid_rows, with_labels, device, rc_rows, timer=None):
        self.p, self.enc, self.device, self.timer = plan, enc, device, timer
        self.on_gpu = device.type == "cuda"
        self.shape = (grid_rows * plan.th, plan.cols * plan.tw)
        self.grid = None if grid_dtype is None else self._new_grid(grid_dtype)
        self.labels = torch.empty(self.shape, dtype=torch.uint8, device=device) if with_labels else None
        self.rc = _positions(rc_rows, plan.cols, device)
        self.buf = None
        if self.on_gpu:
            self.buf = torch.empty((min(plan.batch_size, rc_rows * plan.cols), plan.ph, plan.pw, 3), dtype=torch.uint8, device=device)

    def _new_grid(self, dtype):
        return torch.empty(self.shape, dtype=dtype, device=self.device)

    def region(self, canvas, mask, y0, x0, rows, r_off):
        """tile rows [0, rows) x every column of the region at pixel (y0, x0) of `canvas` -> grid rows from tile row r_off on"""
        from .extract_embeddings import _stage
        p, timer = self.p, self.timer
        n = rows * p.cols
        lo_row, hi_row = r_off * p.th, (r_off + rows) * p.th
        for lo in range(0, n, p.batch_size):
            hi = min(lo + p.batch_size, n)
            rc = self.rc[lo:hi]
            with _stage(timer, "gpu", "cut"):
                if self.on_gpu:
                    tiles = ops.cut_pixels_u8(canvas, rc, p.ph, p.pw, y0=y0, x0=x0, level=p.level, out=self.buf[:hi - lo])
                else:                                              # host logic under test (encode_fn injected, no GPU)
                    tiles = torch.from_numpy(ops.cut_pixels_reference(canvas.numpy(), rc.numpy(), p.ph, p.pw, y0=y0, x0=x0, level=p.level))
            with _stage(timer, "gpu", "encode"):
                idx = self.enc(tiles)
            if self.grid is None:
                self.grid = self._new_grid(idx.dtype)
            with _stage(timer, "gpu", "stitch"):
                self._stitch(idx, rc, self.grid[lo_row:hi_row])
        if self.labels is not None:
            out_hw = (rows * p.th, p.cols * p.tw)
            with _stage(timer, "gpu", "label_pool"):
                if self.on_gpu:
                    self.labels[lo_row:hi_row] = ops.pool_labels_u8(mask, p.win, y0=y0, x0=x0, out_hw=out_hw)
                else:
                    self.labels[lo_row:hi_row] = torch.from_numpy(ops.pool_labels_reference(mask.numpy(), p.win, y0=y0, x0=x0, out_hw=out_hw))

    def _stitch(self, idx, rc, grid):
        if self.on_gpu:
            ops.stitch_tiles(idx, rc, grid)
            return
        th, tw = self.p.th, self.p.tw
        for k, (r, c) in enumerate(rc.tolist()):
            grid[r * th:(r + 1) * th, c * tw:(c + 1) * tw] = idx[k].to(grid.dtype)


def _as_u8_tensor(a, what):
    if isinstance(a, torch.Tensor):
        t = a
    else:
        import warnings
        with warnings.catch_warnings():                            # (a read-only memmap: the tensor is only ever read)
            warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
            t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != torch.uint8:
        raise ValueError(f"{what} must be uint8, got {t.dtype}")
    return t.contiguous()


@torch.no_grad()
def encode_region(model, pixels, mask=None, tile=32, *, y0=0, x0=0, rows=None, cols=None, level=0, batch_size=64,
                  autocast_dtype=torch.float16, encode_fn=None, timer=None):
    """The code grid of the rows x cols tiles of `pixels` from pixel (y0, x0) on, and the label grid of `mask`:
    (grid [rows * th, cols * tw] in the compact code width (uint8 up to 256 codes, else uint16), labels uint8 of the same
    shape or None) as device tensors -- what get_encodings stitches for a slide, before cast_to_lowest_dtype.

    pixels: uint8 [H, W, 3]; a numpy array or host tensor is uploaded once (the rows of the region only), a device tensor stays
    where it is.  mask: uint8 [H, W] or None.  tile: the latent tile side, or (th, tw); one tile is P = tile * 2**n_down model
    pixels a side and P * 2**level source pixels.  rows / cols default to every whole tile from the origin on: partial tiles
    at the right and bottom edges are dropped.  level: 0 .. 6, see the module docstring.
    Tiles are taken row-major in batches of `batch_size` (the last may be short); their positions go up once per call and
    nothing synchronises with the host per batch.
    model: a NativeVQAE or the VQAE / Encoder mirror, as run_eval takes them.  autocast_dtype defaults to run_eval's fp16, so
    that the grids equal get_encodings' by default; None keeps the handle's own compute dtype.
    encode_fn(tiles_u8 [n, P, P, 3]) -> idx [n, th, tw] replaces the HIP encode (CPU tests of the host logic only; host
    pixels then stay on the host and the cut, the stitch and the pooling are the numpy restatements of ops).
    ValueError, before anything is allocated: a region outside the canvas; a canvas smaller than one tile; a mask whose shape
    differs from the pixels'; a level outside 0 .. 6; batch_size < 1.
    timer: an extract_embeddings.StageTimer that collects the stage table (cut / encode / stitch / label_pool)."""
    plan = _Plan(model, tuple(pixels.shape), None if mask is None else tuple(mask.shape), tile, y0, x0, rows, cols, level, batch_size)
    enc, grid_dtype = _encoder(model, autocast_dtype, encode_fn)
    y0 = plan.y0
    if not (isinstance(pixels, torch.Tensor) and pixels.is_cuda):                 # the rows of the region: one contiguous slab
        ya, yb = plan.y0, plan.y0 + plan.rows * plan.sh
        pixels, mask, y0 = pixels[ya:yb], (None if mask is None else mask[ya:yb]), 0
    canvas = _as_u8_tensor(pixels, "pixels")
    labels_src = None if mask is None else _as_u8_tensor(mask, "mask")
    if encode_fn is None:                                          # raises without a GPU: there is no CPU fallback
        canvas = canvas.to("cuda", non_blocking=True)
        labels_src = None if labels_src is None else labels_src.to(canvas.device, non_blocking=True)
    run = _Run(plan, enc, grid_dtype, plan.rows, labels_src is not None, canvas.device, plan.rows, timer)
    run.region(canvas, labels_src, y0, plan.x0, plan.rows, 0)
    return run.grid, run.labels


@torch.no_grad()
def encode_slide(model, pixels, mask=None, tile=32, *, band_rows=4, **kw):
    """(grid, labels | None) of a whole slide (or the region the encode_region keywords y0 / x0 / rows / cols select) as host
    arrays through cast_to_lowest_dtype: exactly what get_encodings yields for the slide and its mask.

    For sources that live on the host or do not fit in device memory: np.ndarray, np.memmap, any object with `shape` whose
    row slices `pixels[a:b]` convert with np.asarray (an HDF5 pixel dataset).  The slide is walked in bands of `band_rows` tile
    rows, each one contiguous slab: it is copied into one of two page-locked staging buffers (allocated by torch) and goes up
    on a side stream, ordered by events, so band n + 1 uploads while band n encodes.  The host waits only for a staging buffer
    to be free again and for the final download; the slide's code and label grids stay on the device and come down once.
    timer: an extract_embeddings.StageTimer that collects the stage table, as get_encodings takes one.
    One process, one GPU (module docstring)."""
    from .extract_embeddings import _stage, cast_to_lowest_dtype
    if band_rows < 1:
        raise ValueError(f"band_rows {band_rows}")
    encode_fn = kw.pop("encode_fn", None)
    autocast_dtype = kw.pop("autocast_dtype", torch.float16)
    timer = kw.pop("timer", None)
    plan = _Plan(model, tuple(pixels.shape), None if mask is None else tuple(mask.shape), tile, kw.pop("y0", 0), kw.pop("x0", 0),
                 kw.pop("rows", None), kw.pop("cols", None), kw.pop("level", 0), kw.pop("batch_size", 64))
    if kw:
        raise TypeError(f"encode_slide: unexpected arguments {sorted(kw)}")
    enc, grid_dtype = _encoder(model, autocast_dtype, encode_fn)
    band_rows = min(int(band_rows), plan.rows)
    bands = [(r, min(band_rows, plan.rows - r)) for r in range(0, plan.rows, band_rows)]
    slab = lambda src, r, n: np.asarray(src[plan.y0 + r * plan.sh: plan.y0 + (r + n) * plan.sh])
    if encode_fn is not None:                                      # host logic under test: no staging, no streams
        run = _Run(plan, enc, grid_dtype, plan.rows, mask is not None, torch.device("cpu"), band_rows, timer)
        for r, n in bands:
            run.region(_as_u8_tensor(slab(pixels, r, n), "pixels"), None if mask is None else _as_u8_tensor(slab(mask, r, n), "mask"),
                       0, plan.x0, n, r)
    else:
        device = torch.device("cuda", torch.cuda.current_device())  # raises without a GPU: there is no CPU fallback
        run = _Run(plan, enc, grid_dtype, plan.rows, mask is not None, device, band_rows, timer)
        hb = band_rows * plan.sh
        with _stage(timer, "host", "staging_alloc"):
            stage = [torch.empty((hb, plan.W, 3), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            dev = [torch.empty((hb, plan.W, 3), dtype=torch.uint8, device=device) for _ in range(2)]
            mstage = mdev = [None, None]
            if mask is not None:
                mstage = [torch.empty((hb, plan.W), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
                mdev = [torch.empty((hb, plan.W), dtype=torch.uint8, device=device) for _ in range(2)]
        main, side = torch.cuda.current_stream(device), torch.cuda.Stream(device, priority=-1)
        side.wait_stream(main)                                     # (the device bands may reuse memory main-stream work still reads)
        copied, encoded = [None, None], [None, None]
        for k, (r, n) in enumerate(bands):
            s, h = k % 2, n * plan.sh
            if copied[s] is not None:                              # the staging buffer is free once its copy has run
                with _stage(timer, "host", "staging_wait"):
                    copied[s].synchronize()
            with _stage(timer, "host", "staging_fill"):
                np.copyto(stage[s][:h].numpy(), slab(pixels, r, n), casting="no")
                if mask is not None:
                    np.copyto(mstage[s][:h].numpy(), slab(mask, r, n), casting="no")
            with torch.cuda.stream(side):
                if encoded[s] is not None:                         # the device band is free once band k - 2 has been encoded
                    side.wait_event(encoded[s])
                with _stage(timer, "gpu", "h2d"):
                    dev[s][:h].copy_(stage[s][:h], non_blocking=True)
                    if mask is not None:
                        mdev[s][:h].copy_(mstage[s][:h], non_blocking=True)
                copied[s] = torch.cuda.Event()
                copied[s].record(side)
            main.wait_event(copied[s])
            run.region(dev[s], mdev[s], 0, plan.x0, n, r)
            encoded[s] = torch.cuda.Event()
            encoded[s].record(main)
    with _stage(timer, "host", "d2h"):
        grid = run.grid.cpu().numpy()
        labels = None if run.labels is None else run.labels.cpu().numpy()
    with _stage(timer, "host", "cast_lowest"):
        grid = cast_to_lowest_dtype(grid)
        labels = None if labels is None else cast_to_lowest_dtype(labels)
    return grid, labels


def encode_arrays_hdf5(out_path, model, slides, **kw):
    """One archive in the layout of save_encodings_hdf5 from an iterable of (stem, pixels, mask | None): `images/<stem>` and
    `masks/<stem>_mask`, each slide through encode_slide (whose keyword arguments pass through) and appended as soon as it is
    done -- the archive CAMELYON16EmbeddingsDataset opens (datamodules/camelyon16.py:226-235) and reconstruct_hdf5,
    classify_hdf5, histogram_hdf5 and train_hdf5 read.  One process, one GPU."""
    with hdf5.H5Writer(out_path) as writer:
        for stem, pixels, mask in slides:
            grid, labels = encode_slide(model, pixels, mask, **kw)
            writer.create_dataset("images", str(stem), grid)
            if labels is not None:
                writer.create_dataset("masks", f"{stem}_mask", labels)
    return str(out_path)
