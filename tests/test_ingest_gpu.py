"""GPU: the way in from uint8 slide pixels to code grids -- vqae_cut_pixels_u8, vqae_pool_labels_u8 and vqae_amd.ingest --
against the numpy restatements (tests/test_ingest_cpu.py pins those to hand-written loops), the extraction driver and the
way back.  Every comparison is exact: nothing here rounds in floating point.

Models are built as tests/test_reconstruct_gpu.py builds them: oracle.make_params(SPECS[name], 0) + the fixture codebook;
`tiny` has patches of 32 pixels, code tiles of 8 and a factor of 4."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

_cache = {}
POISON = 7


def _params(oracle):
    if "p" not in _cache:
        p = oracle.make_params(oracle.SPECS["tiny"], 0)
        p["encoder.vq_layers.0.embed"] = torch.from_numpy(load_golden("model_tiny")["embed"])
        _cache["p"] = p
    return _cache["p"]


def _nat(amd, oracle):
    if "nat" not in _cache:
        _cache["nat"] = amd.NativeVQAE(amd.SPECS["tiny"], _params(oracle))
    return _cache["nat"]


def _cut(amd, canvas, rc, h, w, **kw):
    """(device result, numpy restatement), both started from poisoned tiles"""
    out = torch.full((len(rc), h, w, canvas.shape[2]), POISON, dtype=torch.uint8, device="cuda")
    got = amd.ops.cut_pixels_u8(torch.from_numpy(canvas).cuda(), torch.from_numpy(rc).cuda(), h, w, out=out, **kw)
    assert got is out
    want = amd.ops.cut_pixels_reference(canvas, rc, h, w, out=np.full(tuple(out.shape), POISON, np.uint8), **kw)
    return got.cpu().numpy(), want


# ---- 1. the cut, level 0 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y0,x0", [(0, 0), (3, 5)])
@pytest.mark.parametrize("w,canvas_w", [(32, 100), (32, 97), (6, 19), (32, 128), (10, 64)])     # 16-byte rows, byte rows, tails
@pytest.mark.parametrize("ch", [1, 3])
def test_cut_level0_equals_the_restatement(amd, ch, w, canvas_w, y0, x0):
    h = 5
    canvas = np.random.RandomState(w + canvas_w + ch).randint(0, 256, size=(3 * h + 4, canvas_w, ch)).astype(np.uint8)
    # a permuted subset of a 3 x 3 layout, then tiles that poke outside the canvas below, to the right and above
    rc = np.array([(2, 1), (0, 0), (1, 2), (0, 2), (3, 0), (0, canvas_w // w), (-1, 1), (1, 1)], np.int32)
    got, want = _cut(amd, canvas, rc, h, w, y0=y0, x0=x0)
    assert np.array_equal(got, want)
    assert (want[4:7] == POISON).all() and (got[4:7] == POISON).all()                  # left untouched
    assert np.array_equal(got[1], canvas[y0:y0 + h, x0:x0 + w]) and np.array_equal(got[7], canvas[y0 + h:y0 + 2 * h, x0 + w:x0 + 2 * w])
    if x0 + 3 * w > canvas_w:                                                          # the shifted origin pushes column 2 out
        assert (got[2] == POISON).all() and (got[3] == POISON).all()


def test_cut_no_tiles_and_argument_errors(amd):
    canvas = torch.zeros((16, 16, 3), dtype=torch.uint8, device="cuda")
    none = amd.ops.cut_pixels_u8(canvas, torch.zeros((0, 2), dtype=torch.int32, device="cuda"), 4, 4)
    assert tuple(none.shape) == (0, 4, 4, 3)
    rc = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    with pytest.raises(AssertionError):                                                # a canvas smaller than one tile
        amd.ops.cut_pixels_u8(canvas, rc, 17, 4)
    with pytest.raises(AssertionError):                                                # ... at that level
        amd.ops.cut_pixels_u8(canvas, rc, 4, 4, level=3)
    with pytest.raises(AssertionError):
        amd.ops.cut_pixels_u8(canvas, rc, 4, 4, y0=-1)
    with pytest.raises(NotImplementedError):
        amd.ops.cut_pixels_u8(canvas, rc, 4, 4, level=7)
    with pytest.raises(AssertionError):                                                # two channels
        amd.ops.cut_pixels_u8(torch.zeros((16, 16, 2), dtype=torch.uint8, device="cuda"), rc, 4, 4)


# ---- 2. the cut, levels ----------------------------------------------------------------------------------------------
def _level_canvas(kind, shape, seed):
    if kind == "random":
        return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)
    if kind == "white":
        return np.full(shape, 255, np.uint8)
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    return np.broadcast_to((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], shape).copy()     # 2 x 2 mean 127.5


@pytest.mark.parametrize("kind", ["random", "white", "checkerboard"])
@pytest.mark.parametrize("pad,x0", [(0, 0), (16, 16), (5, 3)])                         # the 16-pixel path twice, the pixel path
@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("ch", [1, 3])
def test_cut_levels_equal_the_integer_box_filter(amd, ch, level, pad, x0, kind):
    f, h, w = 1 << level, 5, 8
    canvas = _level_canvas(kind, (2 + 2 * h * f, 3 * w * f + pad, ch), level)
    rc = np.array([(1, 2), (0, 0), (0, 3), (1, 0), (2, 1), (0, 1)], np.int32)          # (0, 3) and (2, 1) lie outside
    got, want = _cut(amd, canvas, rc, h, w, y0=2, x0=x0, level=level)
    assert np.array_equal(got, want)
    assert (got[2] == POISON).all() and (got[4] == POISON).all()
    if kind == "white":
        assert (got[[0, 1, 3, 5]] == 255).all()
    if kind == "checkerboard" and level:
        assert (got[[0, 1, 3, 5]] == 128).all()                                        # 127.5 rounds half up
    if level == 0:                                                                     # level 0 through the level argument: the copy
        assert np.array_equal(got[1], canvas[2:2 + h, x0:x0 + w])


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("x0", [0, 1])
def test_cut_level6_from_a_512_pixel_source(amd, ch, x0):
    canvas = _level_canvas("random", (512, 512 + x0, ch), 6)
    got, want = _cut(amd, canvas, np.array([(0, 0), (0, 1)], np.int32), 8, 8, x0=x0, level=6)
    assert np.array_equal(got, want) and (got[1] == POISON).all()
    assert np.array_equal(got[0, 0, 0], (canvas[:64, x0:x0 + 64].astype(np.uint32).sum(axis=(0, 1)) + 2048) >> 12)
    for kind, value in (("white", 255), ("checkerboard", 128)):
        got, _ = _cut(amd, _level_canvas(kind, (512, 512 + x0, ch), 0), np.array([(0, 0)], np.int32), 8, 8, x0=x0, level=6)
        assert (got == value).all()


def test_cut_and_pool_index_past_2_31_bytes(amd):
    """row offsets are 64-bit: a tile and a window whose bytes lie beyond 2**31 of their canvas"""
    H, W = 24000, 32768                                                                # 2.36e9 bytes of pixels
    canvas = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    patch = np.random.RandomState(0).randint(0, 256, size=(32, 64, 3)).astype(np.uint8)
    canvas[H - 32:, W - 64:] = torch.from_numpy(patch).cuda()
    rc = torch.tensor([(0, 1), (0, 0)], dtype=torch.int32, device="cuda")
    got = amd.ops.cut_pixels_u8(canvas, rc, 32, 32, y0=H - 32, x0=W - 64)
    assert np.array_equal(got.cpu().numpy(), np.stack([patch[:, 32:], patch[:, :32]]))
    got1 = amd.ops.cut_pixels_u8(canvas, rc, 16, 16, y0=H - 32, x0=W - 64, level=1)
    assert np.array_equal(got1.cpu().numpy(), amd.ops.cut_pixels_reference(patch, rc.cpu().numpy(), 16, 16, level=1))
    del canvas, got, got1
    mask = torch.empty((3 * H, W), dtype=torch.uint8, device="cuda")                   # 2.36e9 bytes of mask
    m = np.random.RandomState(1).randint(0, 3, size=(32, 64)).astype(np.uint8)
    mask[3 * H - 32:, W - 64:] = torch.from_numpy(m).cuda()
    for x0 in (W - 64, W - 63):                                                        # the 16-byte path, the byte path
        got = amd.ops.pool_labels_u8(mask, 4, y0=3 * H - 32, x0=x0)
        assert np.array_equal(got.cpu().numpy(), amd.ops.pool_labels_reference(m, 4, x0=x0 - (W - 64)))


# ---- 3. label pooling ------------------------------------------------------------------------------------------------
def _sparse_mask(h, w, seed):
    """values {0, 1, 2}, about 0.5 % nonzero: nothing in the left third, only 1 in the middle third"""
    rs = np.random.RandomState(seed)
    m = (rs.random_sample((h, w)) < 0.0075).astype(np.uint8) * rs.randint(1, 3, size=(h, w)).astype(np.uint8)
    m[:, :w // 3] = 0
    m[:, w // 3:2 * w // 3] = np.minimum(m[:, w // 3:2 * w // 3], 1)
    return m


@pytest.mark.parametrize("y0,x0,pad", [(0, 0, 0), (3, 16, 16), (2, 5, 7)])              # 16-byte columns twice; unaligned x0, odd width
@pytest.mark.parametrize("win", [1, 4, 16, 64])
def test_pool_labels_equals_the_restatement(amd, win, y0, x0, pad):
    out_h, out_w = {1: (40, 149), 4: (12, 37), 16: (5, 6), 64: (5, 6)}[win]          # (rows that end off a 16-byte column at 1 and 4)
    mask = _sparse_mask(y0 + out_h * win + 1, x0 + out_w * win + pad, win)
    assert 0.002 < (mask != 0).mean() < 0.008
    got = amd.ops.pool_labels_u8(torch.from_numpy(mask).cuda(), win, y0=y0, x0=x0, out_hw=(out_h, out_w))
    want = amd.ops.pool_labels_reference(mask, win, y0=y0, x0=x0, out_hw=(out_h, out_w))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (out_h, out_w)
    assert np.array_equal(got.cpu().numpy(), want)
    assert set(np.unique(want).tolist()) == {0, 1, 2}
    # out_hw defaults to every whole window from the origin on; rectangular windows
    assert np.array_equal(amd.ops.pool_labels_u8(torch.from_numpy(mask).cuda(), win, y0=y0, x0=x0).cpu().numpy(),
                          amd.ops.pool_labels_reference(mask, win, y0=y0, x0=x0))
    if win > 1:
        rect = (3, win)
        assert np.array_equal(amd.ops.pool_labels_u8(torch.from_numpy(mask).cuda(), rect, y0=y0, x0=x0).cpu().numpy(),
                              amd.ops.pool_labels_reference(mask, rect, y0=y0, x0=x0))


def test_pool_labels_all_byte_values_and_other_windows(amd):
    mask = np.random.RandomState(3).randint(0, 256, size=(50, 96)).astype(np.uint8)   # the packed maximum on full bytes
    dev = torch.from_numpy(mask).cuda()
    for win in (2, 8, 32, (5, 3), (1, 16), (7, 2)):
        assert np.array_equal(amd.ops.pool_labels_u8(dev, win).cpu().numpy(), amd.ops.pool_labels_reference(mask, win)), win


def test_pool_labels_window_outside_the_mask_raises(amd):
    mask = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    with pytest.raises(AssertionError):
        amd.ops.pool_labels_u8(mask, 16, out_hw=(4, 5))
    with pytest.raises(AssertionError):
        amd.ops.pool_labels_u8(mask, 16, y0=1, out_hw=(4, 4))
    with pytest.raises(AssertionError):
        amd.ops.pool_labels_u8(mask, 16, x0=-16, out_hw=(1, 1))
    assert tuple(amd.ops.pool_labels_u8(mask, 16, y0=60).shape) == (0, 4)


# ---- 4. encode_region equals the extraction --------------------------------------------------------------------------------
SIZES = [(3, 2), (2, 3)]


def _slides(amd, oracle):
    """(nat, ds, host canvases, host masks, get_encodings results in fp32 and under the default fp16 autocast)"""
    if "slides" not in _cache:
        from vqae_amd.extract_embeddings import SyntheticSlideDataset, get_encodings
        nat = _nat(amd, oracle)
        ds = SyntheticSlideDataset(SIZES, patch_size=32, raw=True)
        canvases = [np.zeros((r * 32, c * 32, 3), np.uint8) for r, c in SIZES]
        masks = [np.zeros((r * 32, c * 32), np.uint8) for r, c in SIZES]
        for i in range(len(ds)):
            s, r, c = ds.locate(i)
            img, lab, _ = ds[i]
            canvases[s][r * 32:(r + 1) * 32, c * 32:(c + 1) * 32] = img.numpy()
            masks[s][r * 32:(r + 1) * 32, c * 32:(c + 1) * 32] = lab.numpy()[0]
        f32 = dict(get_encodings(nat, ds, batch_size=5, autocast_dtype=None, num_workers=0))
        f16 = dict(get_encodings(nat, ds, batch_size=5, num_workers=0))
        _cache["slides"] = (nat, ds, canvases, masks, f32, f16)
    return _cache["slides"]


def _lowest(t):
    from vqae_amd.extract_embeddings import cast_to_lowest_dtype
    return cast_to_lowest_dtype(t.cpu().numpy())


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def test_encode_region_equals_get_encodings(amd, oracle):
    """rests on the encoder's bit-exact batch invariance (tests/test_configs_gpu.py)"""
    nat, ds, canvases, masks, f32, f16 = _slides(amd, oracle)
    for s in range(2):
        grid, labels = amd.encode_region(nat, canvases[s], masks[s], tile=8, autocast_dtype=None)
        assert grid.is_cuda and grid.dtype == torch.uint8 and labels.is_cuda and labels.dtype == torch.uint8
        assert _same(_lowest(grid), f32[f"images/slide_{s:03d}"]) and _same(_lowest(labels), f32[f"masks/slide_{s:03d}_mask"])
        assert f32[f"masks/slide_{s:03d}_mask"].dtype == np.bool_ and f32[f"masks/slide_{s:03d}_mask"].any()
        grid16, labels16 = amd.encode_region(nat, canvases[s], masks[s], tile=8, batch_size=4)        # run_eval's fp16 autocast
        assert _same(_lowest(grid16), f16[f"images/slide_{s:03d}"]) and _same(_lowest(labels16), f16[f"masks/slide_{s:03d}_mask"])
        # a device tensor stays where it is
        dev, _ = amd.encode_region(nat, torch.from_numpy(canvases[s]).cuda(), None, tile=8, autocast_dtype=None, batch_size=1)
        assert torch.equal(dev, grid)


def test_encode_region_through_the_mirror(amd, oracle):
    nat, ds, canvases, masks, f32, f16 = _slides(amd, oracle)
    from vqae_amd.model import VQAE
    model = VQAE.from_spec(amd.SPECS["tiny"])
    model.load_state_dict(_params(oracle), strict=False)
    model = model.cuda().eval()
    grid, labels = amd.encode_region(model, canvases[0], masks[0], tile=8, autocast_dtype=None)
    assert grid.dtype == torch.uint8
    assert _same(_lowest(grid), f32["images/slide_000"]) and _same(_lowest(labels), f32["masks/slide_000_mask"])
    grid16, _ = amd.encode_region(model, canvases[0], None, tile=8)
    assert _same(_lowest(grid16), f16["images/slide_000"])


def test_encode_region_drops_partial_tiles_and_takes_sub_regions(amd, oracle):
    nat, ds, canvases, masks, f32, f16 = _slides(amd, oracle)
    H, W = canvases[1].shape[:2]
    rs = np.random.RandomState(0)
    padded = rs.randint(0, 256, size=(H + 7, W + 13, 3)).astype(np.uint8)
    padded_mask = rs.randint(0, 3, size=(H + 7, W + 13)).astype(np.uint8)
    padded[:H, :W], padded_mask[:H, :W] = canvases[1], masks[1]
    grid, labels = amd.encode_region(nat, padded, padded_mask, tile=8, autocast_dtype=None)
    assert _same(_lowest(grid), f32["images/slide_001"]) and _same(_lowest(labels), f32["masks/slide_001_mask"])
    for src, msk in ((canvases[0], masks[0]), (torch.from_numpy(canvases[0]).cuda(), torch.from_numpy(masks[0]).cuda())):
        part, part_l = amd.encode_region(nat, src, msk, tile=8, y0=32, x0=32, autocast_dtype=None)      # tile (1, 1) on
        assert tuple(part.shape) == (16, 8)
        assert np.array_equal(part.cpu().numpy(), f32["images/slide_000"][8:, 8:])
        assert np.array_equal(part_l.cpu().numpy(), f32["masks/slide_000_mask"][8:, 8:])
    one, _ = amd.encode_region(nat, canvases[0], None, tile=8, y0=32, x0=32, rows=1, cols=1, autocast_dtype=None)
    assert np.array_equal(one.cpu().numpy(), f32["images/slide_000"][8:16, 8:16])


def test_encode_region_level1_reads_the_box_filtered_canvas(amd, oracle):
    nat = _nat(amd, oracle)
    rs = np.random.RandomState(1)
    big = rs.randint(0, 256, size=(2 * 64 + 3, 3 * 64 + 16, 3)).astype(np.uint8)
    big_mask = _sparse_mask(big.shape[0], big.shape[1], 9)
    box = big[:128, :192].astype(np.uint32).reshape(64, 2, 96, 2, 3).sum(axis=(1, 3))
    small = ((box + 2) >> 2).astype(np.uint8)
    want, _ = amd.encode_region(nat, small, None, tile=8, autocast_dtype=None)
    grid, labels = amd.encode_region(nat, big, big_mask, tile=8, level=1, autocast_dtype=None)
    assert tuple(grid.shape) == (16, 24) and torch.equal(grid, want)
    assert np.array_equal(labels.cpu().numpy(), amd.ops.pool_labels_reference(big_mask, 8, out_hw=(16, 24)))


# ---- 5. encode_slide, the archive, the round trip --------------------------------------------------------------------------
@pytest.mark.parametrize("band_rows", [1, 2])
@pytest.mark.parametrize("source", ["array", "memmap"])
def test_encode_slide_equals_get_encodings(amd, oracle, tmp_path, source, band_rows):
    nat, ds, canvases, masks, f32, f16 = _slides(amd, oracle)
    for s in range(2):
        pixels, mask = canvases[s], masks[s]
        if source == "memmap":
            np.save(tmp_path / f"p{s}.npy", pixels)
            np.save(tmp_path / f"m{s}.npy", mask)
            pixels, mask = np.load(tmp_path / f"p{s}.npy", mmap_mode="r"), np.load(tmp_path / f"m{s}.npy", mmap_mode="r")
        grid, labels = amd.encode_slide(nat, pixels, mask, tile=8, band_rows=band_rows, batch_size=4, autocast_dtype=None)
        assert isinstance(grid, np.ndarray) and isinstance(labels, np.ndarray) and labels.dtype == np.bool_
        assert _same(grid, f32[f"images/slide_{s:03d}"]) and _same(labels, f32[f"masks/slide_{s:03d}_mask"])
    grid16, _ = amd.encode_slide(nat, canvases[0], None, tile=8, band_rows=band_rows)
    assert _same(grid16, f16["images/slide_000"])


def test_encode_arrays_hdf5_equals_save_encodings_hdf5(amd, oracle, tmp_path):
    from vqae_amd import hdf5
    from vqae_amd.extract_embeddings import save_encodings_hdf5
    nat, ds, canvases, masks, f32, f16 = _slides(amd, oracle)
    want_path = save_encodings_hdf5(tmp_path / "want.hdf5", nat, ds, batch_size=5, autocast_dtype=None, num_workers=0)
    path = amd.encode_arrays_hdf5(tmp_path / "got.hdf5", nat, ((f"slide_{s:03d}", canvases[s], masks[s]) for s in range(2)),
                                  tile=8, band_rows=2, autocast_dtype=None)
    want, got = hdf5.read_hdf5(want_path), hdf5.read_hdf5(path)
    assert sorted(got.keys()) == sorted(want.keys()) == ["images", "masks"]
    for group in ("images", "masks"):
        assert sorted(got[group].keys()) == sorted(want[group].keys())
        for name in want[group].keys():
            assert _same(np.asarray(got[group][name]), np.asarray(want[group][name])), (group, name)
    # the way back reads it
    for s in range(2):
        bands = list(amd.reconstruct_hdf5(nat, path, f"slide_{s:03d}", tile=8, band_rows=2))
        rec = amd.reconstruct_region(nat, f32[f"images/slide_{s:03d}"], 8).cpu().numpy()
        assert np.array_equal(np.concatenate([b for _, b in bands]), rec)


def test_round_trip_of_one_tile(amd, oracle):
    nat, ds, canvases, masks, f32, f16 = _slides(amd, oracle)
    tile = np.ascontiguousarray(canvases[0][32:64, 32:64])
    grid, _ = amd.encode_region(nat, tile, None, tile=8, autocast_dtype=None)
    back = amd.reconstruct_region(nat, grid, 8)
    want = nat.decode_indices_u8(nat.encode_u8(torch.from_numpy(tile)[None].cuda())[1])[0]
    assert tuple(back.shape) == (32, 32, 3) and torch.equal(back, want)
