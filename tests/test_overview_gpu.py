"""GPU: overview levels -- vqae_pixels_u8_level, vqae_decode_indices_u8_levels and the `level` argument of
vqae_amd.reconstruct -- bit for bit against a host restatement of the contract applied to level-0 uint8 pixels:

    out[Y][X][c] = (sum of the f x f block of level-0 pixels + f*f/2) >> 2L,   f = 2**L

i.e. reshape to [H/f, f, W/f, f, 3] -> sum as uint32 -> + f*f/2 -> >> 2L.  The sums are integers, so every comparison here
is exact.  Level 0 itself is the subject of tests/test_reconstruct_gpu.py; models and codes are those of its
test_decode_indices_u8_matches_own_fp32_output.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURE = {"tiny": "model_tiny", "tinyP": "model_tinyP", "mid16": "taps_mid16_f32"}
_cache = {}


def _box(u8, L):
    """the yardstick on uint8 pictures [..., H, W, 3]"""
    f = 1 << L
    *lead, H, W, C = u8.shape
    s = u8.reshape(*lead, H // f, f, W // f, f, C).astype(np.uint32).sum(axis=(-4, -2), dtype=np.uint32)
    return ((s + np.uint32(f * f // 2)) >> np.uint32(2 * L)).astype(np.uint8)


def _params(oracle, name):
    if ("p", name) not in _cache:
        p = oracle.make_params(oracle.SPECS[name], 0)
        p["encoder.vq_layers.0.embed"] = torch.from_numpy(load_golden(FIXTURE[name])["embed"])
        _cache[("p", name)] = p
    return _cache[("p", name)]


def _nat(amd, oracle, name, dtype=None):
    if (name, dtype) not in _cache:
        _cache[(name, dtype)] = amd.NativeVQAE(amd.SPECS[name], _params(oracle, name), compute_dtype=dtype)
    return _cache[(name, dtype)]


def _codes(oracle, name):
    K = oracle.SPECS[name].num_embeddings
    if name == "mid16":                                                # 128 x 128 pixels at batch 2: 32 x 32 codes, 4 x 4 blocks
        return np.random.RandomState(0).randint(0, K, size=(2, 8, 8)).astype(np.int64).repeat(4, 1).repeat(4, 2)
    return np.random.RandomState(0).randint(0, K, size=(15, 8, 8)).astype(np.int64)


# ---- 1. arithmetic ---------------------------------------------------------------------------------------------------
CRAFTED = [0.5, 1.5, 2.5, 254.5, -3.0, 255.49, 300.0, float("inf"), float("-inf"), float("nan")]
UNIT = dict(mean=(0, 0, 0), std=(1 / 255,) * 3)                       # fp32(1/255) * fp32(255) == 1: v = x


def _crafted_nhwc(B, H, W, seed):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-20, 275, size=(B, H, W, 3)).astype(np.float32)
    x.reshape(-1)[rs.permutation(x.size)[:x.size // 4]] += np.float32(0.5)          # more near-ties
    half = rs.randint(-4, 260, size=x.size // 8).astype(np.float32) + np.float32(0.5)
    x.reshape(-1)[rs.permutation(x.size)[:half.size]] = half                         # exact ties, both parities
    x.reshape(-1)[:len(CRAFTED)] = CRAFTED                                           # clamps, +-inf, NaN
    return x


def _host_u8(x):
    """level 0 with v = x: rint half-to-even, clamp, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), 0, np.clip(np.rint(x), 0, 255)).astype(np.uint8)


def _dev(x_nhwc, layout):
    return torch.from_numpy(x_nhwc if layout == "NHWC" else np.ascontiguousarray(x_nhwc.transpose(0, 3, 1, 2))).cuda()


@pytest.mark.parametrize("layout", ["NHWC", "NCHW"])
@pytest.mark.parametrize("H,W,levels", [(2, 6, (1,)), (6, 10, (1,)), (8, 12, (1, 2)), (64, 64, (1, 2, 3, 4, 5, 6))])
def test_level_arithmetic_exact(amd, layout, H, W, levels):
    assert np.float32(1 / 255) * np.float32(255) == np.float32(1)
    B = 3
    x = _crafted_nhwc(B, H, W, 7 * H + W)
    dev, u0 = _dev(x, layout), _host_u8(x)
    # level 0 through `level` is the call without it
    assert torch.equal(amd.ops.pixels_u8(dev, layout, level=0, **UNIT), amd.ops.pixels_u8(dev, layout, **UNIT))
    assert np.array_equal(amd.ops.pixels_u8(dev, layout, level=0, **UNIT).cpu().numpy(), u0)
    for L in levels:
        got = amd.ops.pixels_u8(dev, layout, level=L, **UNIT).cpu().numpy()
        assert got.shape == (B, H >> L, W >> L, 3) and got.dtype == np.uint8
        assert np.array_equal(got, _box(u0, L)), (layout, H, W, L)


@pytest.mark.parametrize("layout", ["NHWC", "NCHW"])
def test_level_rounding_width_and_nan_blocks(amd, layout):
    def one(block_nhwc, L):
        return amd.ops.pixels_u8(_dev(np.ascontiguousarray(block_nhwc, np.float32), layout), layout, level=L, **UNIT).cpu().numpy()

    # tiles of 2 x 4 pixels at level 1: two output pixels each, from the blocks {0,0,1,1} / {1,1,2,2} (sums 2 and 6)
    t = np.zeros((1, 2, 4, 3), np.float32)
    t[0, :, 0:2] = np.array([[0, 0], [1, 1]], np.float32)[:, :, None]
    t[0, :, 2:4] = np.array([[1, 1], [2, 2]], np.float32)[:, :, None]
    got = one(t, 1)
    assert got.shape == (1, 1, 2, 3)
    assert (got[0, 0, 0] == 1).all()                                   # (2 + 2) >> 2: half goes up; round-half-even would give 0
    assert (got[0, 0, 1] == 2).all()                                   # (6 + 2) >> 2
    # the same two blocks through the one-pixel path (width 2)
    assert (one(t[:, :, 0:2], 1) == 1).all() and (one(t[:, :, 2:4], 1) == 2).all()
    # all 255 over 64 x 64 at level 6: 255 * 4096 + 2048 needs more than 16 bits
    assert (one(np.full((2, 64, 64, 3), 255.0), 6) == 255).all()
    assert (one(np.full((2, 64, 64, 3), 300.0), 6) == 255).all()
    # an all-NaN block
    assert (one(np.full((1, 8, 8, 3), np.nan), 3) == 0).all()
    assert (one(np.full((1, 2, 2, 3), np.nan), 1) == 0).all()


@pytest.mark.parametrize("layout", ["NHWC", "NCHW"])
def test_level_unaligned_input_takes_the_generic_path(amd, layout):
    """a device pointer offset by one float, at a width (12) the 4-pixel path would take"""
    B, H, W = 3, 8, 12
    x = _crafted_nhwc(B, H, W, 5)
    src = x if layout == "NHWC" else np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    buf = torch.zeros(src.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(src.reshape(-1)).cuda()
    dev = buf[1:].view(src.shape)
    assert dev.data_ptr() % 16 == 4 and dev.is_contiguous()
    for L in (1, 2):
        assert np.array_equal(amd.ops.pixels_u8(dev, layout, level=L, **UNIT).cpu().numpy(), _box(_host_u8(x), L))


# ---- 2. paste --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["NHWC", "NCHW"])
@pytest.mark.parametrize("H,W,L,canvas_w", [(8, 12, 1, 20), (8, 12, 1, 19), (8, 12, 2, 12), (8, 12, 2, 11), (4, 6, 1, 13),
                                            (64, 64, 4, 12), (64, 64, 4, 13)])
def test_level_paste_into_canvas(amd, layout, H, W, L, canvas_w):
    """canvas widths: once a multiple of 4 and once not, for the 4-pixel path (8 x 12, 64 x 64) and the byte path (4 x 6)"""
    B = 6
    oh, ow = H >> L, W >> L
    assert canvas_w >= 3 * ow
    x = _crafted_nhwc(B, H, W, 100 + W + L)
    # a permuted subset of a 3 x 3 layout, a tile at a negative position, a tile that sticks out of the canvas
    sticks_out = (0, canvas_w // ow)                                   # its last columns (or all of them) lie past the right edge
    rc = np.array([(2, 1), (0, 0), (1, 2), (0, 2), (-1, 1), sticks_out], np.int32)
    canvas = torch.full((3 * oh + 2, canvas_w, 3), 7, dtype=torch.uint8, device="cuda")
    out = amd.ops.pixels_u8(_dev(x, layout), layout, rc=torch.from_numpy(rc).cuda(), canvas=canvas, level=L, **UNIT)
    assert out is canvas
    want = np.full((3 * oh + 2, canvas_w, 3), 7, np.uint8)
    tiles = _box(_host_u8(x), L)
    for t, (r, c) in enumerate(rc[:4]):
        want[r * oh:(r + 1) * oh, c * ow:(c + 1) * ow] = tiles[t]
    assert np.array_equal(canvas.cpu().numpy(), want)                  # bytes outside the pasted blocks stay 7


# ---- 3. through the handle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,levels", [("tiny", None, (1, 3, 5)), ("tiny", "f16", (1, 3, 5)), ("tiny", "bf16", (1, 3, 5)),
                                               ("tinyP", None, (1, 3, 5)), ("mid16", None, (2, 6)), ("mid16", "f16", (2, 6))])
def test_decode_indices_u8_level_equals_reduced_level_0(amd, oracle, name, dtype, levels):
    nat = _nat(amd, oracle, name, dtype)
    idx = torch.from_numpy(_codes(oracle, name)).cuda()
    u0 = nat.decode_indices_u8(idx)
    B, H, W, _ = u0.shape
    u0 = u0.cpu().numpy()
    assert u0.min() == 0 and u0.max() == 255                           # a picture with both clamps hit, not a constant
    narrow = torch.uint8 if nat.spec.num_embeddings <= 256 else torch.uint16
    for L in levels:
        got = nat.decode_indices_u8(idx, level=L)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (B, H >> L, W >> L, 3)
        assert np.array_equal(got.cpu().numpy(), _box(u0, L)), (name, dtype, L)
        assert torch.equal(nat.decode_indices_u8(idx.to(narrow), level=L), got)                # compact code widths
        assert tuple(nat.decode_indices_u8(idx[:0], level=L).shape) == (0, H >> L, W >> L, 3)  # B == 0


def test_decode_indices_u8_several_levels_from_one_decode(amd, oracle):
    nat = _nat(amd, oracle, "tiny")
    idx = torch.from_numpy(_codes(oracle, "tiny")[:9]).cuda()
    levels = (0, 2, 5)
    single = [nat.decode_indices_u8(idx, level=L) for L in levels]
    outs = nat.decode_indices_u8(idx, level=levels)
    assert isinstance(outs, tuple) and len(outs) == 3
    for a, b in zip(outs, single):
        assert torch.equal(a, b)
    assert all(tuple(o.shape) == (0, 32 >> L, 32 >> L, 3) for o, L in zip(nat.decode_indices_u8(idx[:0], level=levels), levels))
    # with canvases: a 3 x 3 layout, pre-filled
    rc = torch.tensor([(r, c) for r in range(3) for c in range(3)], dtype=torch.int32)[torch.randperm(9, generator=torch.Generator().manual_seed(0))].cuda()
    canvases = [torch.full((3 * (32 >> L) + 1, 3 * (32 >> L) + 2, 3), 7, dtype=torch.uint8, device="cuda") for L in levels]
    got = nat.decode_indices_u8(idx, rc, canvases, level=levels)
    assert isinstance(got, tuple) and all(a is b for a, b in zip(got, canvases))
    for L, cv, dense in zip(levels, canvases, single):
        one = nat.decode_indices_u8(idx, rc, torch.full_like(cv, 7), level=L)
        assert torch.equal(cv, one)
        s = 32 >> L
        want = np.full(tuple(cv.shape), 7, np.uint8)
        for t, (r, c) in enumerate(rc.cpu().tolist()):
            want[r * s:(r + 1) * s, c * s:(c + 1) * s] = dense[t].cpu().numpy()
        assert np.array_equal(cv.cpu().numpy(), want)


# ---- 4. regions ------------------------------------------------------------------------------------------------------
def _region_fixture(amd, oracle):
    if "region" not in _cache:
        nat = _nat(amd, oracle, "tiny")
        grid = np.random.RandomState(5).randint(0, 16, size=(3 * 8, 5 * 8)).astype(np.uint8)
        _cache["region"] = (nat, grid, amd.reconstruct_region(nat, grid, 8, batch_size=4).cpu().numpy())
    return _cache["region"]


@pytest.mark.parametrize("L", [1, 3, 5])
def test_region_at_a_level(amd, oracle, L):
    nat, grid, full0 = _region_fixture(amd, oracle)
    assert full0.shape == (3 * 32, 5 * 32, 3)
    full = amd.reconstruct_region(nat, grid, 8, batch_size=4, level=L)
    assert full.is_cuda and full.dtype == torch.uint8 and tuple(full.shape) == (96 >> L, 160 >> L, 3)
    assert np.array_equal(full.cpu().numpy(), _box(full0, L))
    part = amd.reconstruct_region(nat, grid, 8, r0=1, c0=2, rows=2, cols=3, batch_size=4, level=L)
    assert np.array_equal(part.cpu().numpy(), _box(full0[32:96, 64:160], L))


def test_region_slide_archive_and_overview(amd, oracle, tmp_path):
    nat, grid, full0 = _region_fixture(amd, oracle)
    outs = amd.reconstruct_region(nat, grid, 8, batch_size=4, level=(1, 3, 5))
    assert isinstance(outs, tuple) and len(outs) == 3
    for o, L in zip(outs, (1, 3, 5)):
        assert torch.equal(o, amd.reconstruct_region(nat, grid, 8, batch_size=4, level=L))
    want3 = _box(full0, 3)
    bands = list(amd.reconstruct_slide(nat, grid, 8, level=3, band_rows=2))
    assert [r0 for r0, _ in bands] == [0, 2] and all(isinstance(b, np.ndarray) and b.dtype == np.uint8 for _, b in bands)
    assert np.array_equal(np.concatenate([b for _, b in bands]), want3)
    # an archive written by save_encodings_hdf5
    from vqae_amd.extract_embeddings import SyntheticSlideDataset, save_encodings_hdf5
    ds = SyntheticSlideDataset([(3, 2), (2, 3)], patch_size=32, raw=True)
    path = save_encodings_hdf5(tmp_path / "slides.hdf5", nat, ds, batch_size=5, autocast_dtype=None, num_workers=0)
    for s, (rows, cols) in enumerate([(3, 2), (2, 3)]):
        name = f"slide_{s:03d}"
        level0 = np.concatenate([b for _, b in amd.reconstruct_hdf5(nat, path, name, tile=8, band_rows=2)])
        assert level0.shape == (rows * 32, cols * 32, 3)
        for L in (2, 5):
            want = _box(level0, L)
            got = np.concatenate([b for _, b in amd.reconstruct_hdf5(nat, path, name, tile=8, band_rows=2, level=L)])
            over = amd.reconstruct_overview(nat, path, name, tile=8, level=L)
            assert isinstance(over, np.ndarray) and over.dtype == np.uint8
            assert np.array_equal(got, want) and np.array_equal(over, want)
        assert amd.reconstruct_overview(nat, path, name, tile=8).shape == (rows, cols, 3)          # level 5 by default


# ---- 5. errors: nothing is written ------------------------------------------------------------------------------------------
def test_pixel_level_argument_errors(amd):
    x64 = torch.zeros((1, 64, 64, 3), device="cuda")
    x8 = torch.zeros((1, 8, 12, 3), device="cuda")
    rc = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    canvas = torch.full((70, 70, 3), 7, dtype=torch.uint8, device="cuda")
    with pytest.raises(AssertionError):
        amd.ops.pixels_u8(x64, "NHWC", level=-1)
    with pytest.raises(AssertionError):
        amd.ops.pixels_u8(x64, "NHWC", rc=rc, canvas=canvas, level=-1)
    with pytest.raises(NotImplementedError):
        amd.ops.pixels_u8(x64, "NHWC", level=7)
    with pytest.raises(NotImplementedError):
        amd.ops.pixels_u8(x64, "NHWC", rc=rc, canvas=canvas, level=7)
    with pytest.raises(AssertionError):                                # 16 divides neither 8 nor 12
        amd.ops.pixels_u8(x8, "NHWC", level=4)
    with pytest.raises(AssertionError):                                # 8 divides 8 but not 12
        amd.ops.pixels_u8(x8, "NHWC", rc=rc, canvas=canvas, level=3)
    small = torch.full((3, 6, 3), 7, dtype=torch.uint8, device="cuda")
    with pytest.raises(AssertionError):                                # a canvas smaller than one reduced 4 x 6 tile
        amd.ops.pixels_u8(x8, "NHWC", rc=rc, canvas=small, level=1)
    L, p_ = amd._lib, amd.ops._p
    with pytest.raises(AssertionError):                                # canvas sizes with a dense destination
        L.check(L.lib().vqae_pixels_u8_level(p_(x8), L.LAYOUT_NHWC, 1, 8, 12, 1, None, None, None, p_(canvas), 70, 70, None))
    torch.cuda.synchronize()
    assert (canvas == 7).all() and (small == 7).all()


def test_decode_levels_argument_errors(amd, oracle):
    import ctypes
    nat = _nat(amd, oracle, "tiny")
    idx = torch.zeros((1, 8, 8), dtype=torch.int64, device="cuda")     # 32 x 32-pixel tiles
    rc = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    cv = [torch.full((40, 40, 3), 7, dtype=torch.uint8, device="cuda") for _ in range(3)]
    with pytest.raises(AssertionError):
        nat.decode_indices_u8(idx, level=-1)
    with pytest.raises(NotImplementedError):
        nat.decode_indices_u8(idx, level=7)
    with pytest.raises(AssertionError):                                # 64 does not divide 32
        nat.decode_indices_u8(idx, level=6)
    # one bad level among good ones: refused before anything is launched, the good levels' canvases stay as they were
    with pytest.raises(NotImplementedError):
        nat.decode_indices_u8(idx, rc, cv, level=(0, 2, 7))
    with pytest.raises(AssertionError):
        nat.decode_indices_u8(idx, rc, cv, level=(0, 2, 6))
    with pytest.raises(AssertionError):                                # duplicate levels
        nat.decode_indices_u8(idx, rc, cv, level=(1, 2, 1))
    small = torch.full((7, 40, 3), 7, dtype=torch.uint8, device="cuda")
    with pytest.raises(AssertionError):                                # a canvas smaller than one reduced 8 x 8 tile
        nat.decode_indices_u8(idx, rc, [cv[0], small], level=(0, 2))
    with pytest.raises(AssertionError):
        nat.decode_indices_u8(idx, rc, small, level=2)
    L, p_ = amd._lib, amd.ops._p

    def raw(rc_p, n, levels, canvases, hs, ws):
        k = max(len(levels), 1)
        return L.lib().vqae_decode_indices_u8_levels(
            nat._h, p_(idx), L.IDX_I64, 1, 8, 8, rc_p, n, (ctypes.c_int * k)(*levels),
            (ctypes.c_void_p * k)(*[c.data_ptr() for c in canvases]), (ctypes.c_int * k)(*hs), (ctypes.c_int * k)(*ws), None)

    with pytest.raises(AssertionError):                                # canvas sizes with a dense destination
        L.check(raw(None, 2, [0, 1], cv[:2], [0, 40], [0, 40]))
    with pytest.raises(AssertionError):                                # n_levels = 0
        L.check(raw(p_(rc), 0, [0], cv[:1], [40], [40]))
    with pytest.raises(AssertionError):                                # more levels than there are
        L.check(raw(p_(rc), 8, [0, 1, 2, 3, 4, 5, 0, 1], [cv[0]] * 8, [40] * 8, [40] * 8))
    torch.cuda.synchronize()
    assert all((c == 7).all() for c in cv) and (small == 7).all()
