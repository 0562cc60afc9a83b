"""GPU: the way back from code grids to uint8 pixels -- vqae_pixels_u8, vqae_unstitch_tiles, vqae_decode_indices_u8 and
vqae_amd.reconstruct -- against host restatements, the handle's own fp32 output, the oracle and the extraction driver.

Models are built as tests/test_driver_gpu.py builds them: oracle.make_params(SPECS[name], 0) + the fixture codebook.

Quantisation yardstick: u = clamp(rint(x * std255 + mean255), 0, 255) evaluated on the host in fp64 from the fp32 operands.
The kernel's fp32 fused multiply-add differs from that by one rounding of a value in [0, 255], < 8e-6, so the two agree
wherever the fp64 value is further than BAND = 1e-4 from a half-integer; inside the band they may differ by 1.  So that the
band cannot hide a failure every comparison also asserts: at most 0.5 % of the pixels in the band, at least 10 % of the
pixels unclamped, both clamps hit.  Measured on the CPU oracle (fp32): tiny, RandomState(0) codes: 0.013 % in the band,
15.9 % unclamped, all 256 values present; tinyP: 0.020 %, 20.6 %.  mid16 with independent codes per position leaves only
7.5 - 8.6 % unclamped for every seed 0 .. 13 (a decoder driven by white-noise codes saturates), so its codes are drawn
per 4 x 4 block of the code grid (seed 0): 0.024 % in the band, 11.5 % unclamped.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, record_parity

pytestmark = pytest.mark.gpu

BAND = 1e-4
MEAN, STD = (0.7279, 0.5955, 0.7762), (0.2419, 0.3083, 0.1741)
MEAN255 = np.array([np.float32(m) * np.float32(255) for m in MEAN], np.float32)     # fp32 products, as in csrc/handle.hip
STD255 = np.array([np.float32(s) * np.float32(255) for s in STD], np.float32)
FIXTURE = {"tiny": "model_tiny", "tinyP": "model_tinyP", "mid16": "taps_mid16_f32"}
_cache = {}


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
    """the random code tiles of the decode tests (module docstring): int64 [B, h, w]"""
    K = oracle.SPECS[name].num_embeddings
    if name == "mid16":                                                # 128 x 128 pixels at batch 2: 32 x 32 codes, 4 x 4 blocks
        return np.random.RandomState(0).randint(0, K, size=(2, 8, 8)).astype(np.int64).repeat(4, 1).repeat(4, 2)
    return np.random.RandomState(0).randint(0, K, size=(15, 8, 8)).astype(np.int64)


def _v64(x_nhwc):
    return x_nhwc.astype(np.float64) * STD255.astype(np.float64) + MEAN255.astype(np.float64)


def _quant(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)               # np.rint: round half to even


def _check_against_fp(got_u8, x_nhwc, what, max_diff_outside=0):
    """got_u8 against the fp64 quantisation of the fp32 tensor x_nhwc, with the conditions of the module docstring"""
    v = _v64(x_nhwc)
    want = _quant(v)
    in_band = np.abs(v - np.floor(v) - 0.5) < BAND
    unclamped = (v >= 0) & (v <= 255)
    diff = np.abs(got_u8.astype(np.int16) - want.astype(np.int16))
    print(f"{what}: in band {100 * in_band.mean():.4f} %, unclamped {100 * unclamped.mean():.2f} %, low clamp {int((v < 0).sum())}, "
          f"high clamp {int((v > 255).sum())}, differing {int((diff > 0).sum())}, max diff {int(diff.max())}")
    assert in_band.mean() <= 0.005, what
    assert unclamped.mean() >= 0.10, what
    assert (v < 0).any() and (v > 255).any(), what
    assert diff[~in_band].max() <= max_diff_outside, what
    assert diff.max() <= max(1, max_diff_outside), what
    return diff


# ---- 1. pixel arithmetic ---------------------------------------------------------------------------------------------
CRAFTED = [0.5, 1.5, 2.5, 254.5, -3.0, 255.49, 300.0, float("inf"), float("-inf"), float("nan")]
CRAFTED_U8 = [0, 2, 2, 254, 0, 255, 255, 255, 0, 0]


def _crafted_nhwc(B, H, W, seed):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-20, 275, size=(B, H, W, 3)).astype(np.float32)
    x.reshape(-1)[rs.permutation(x.size)[:x.size // 4]] += np.float32(0.5)          # more near-ties
    half = rs.randint(-4, 260, size=x.size // 8).astype(np.float32) + np.float32(0.5)
    x.reshape(-1)[rs.permutation(x.size)[:half.size]] = half                         # exact ties, both parities
    x.reshape(-1)[:len(CRAFTED)] = CRAFTED
    return x


def _host_u8(x):
    """v = x exactly (std255 = 1, mean255 = 0): rint half-to-even, clamp, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), 0, np.clip(np.rint(x), 0, 255)).astype(np.uint8)


@pytest.mark.parametrize("layout", ["NHWC", "NCHW"])
@pytest.mark.parametrize("W", [2, 6, 32])
def test_pixel_arithmetic_exact(amd, layout, W):
    assert np.float32(1 / 255) * np.float32(255) == np.float32(1)                     # so that v = x
    B, H = 3, 5
    x = _crafted_nhwc(B, H, W, W)
    dev = torch.from_numpy(x if layout == "NHWC" else np.ascontiguousarray(x.transpose(0, 3, 1, 2))).cuda()
    got = amd.ops.pixels_u8(dev, layout, mean=(0, 0, 0), std=(1 / 255,) * 3).cpu().numpy()
    assert got.shape == (B, H, W, 3) and got.dtype == np.uint8
    assert got.reshape(-1)[:len(CRAFTED)].tolist() == CRAFTED_U8
    assert np.array_equal(got, _host_u8(x))
    assert np.array_equal(amd.ops.pixels_u8(dev, layout, mean=None, std=None).cpu().numpy(), got)     # NULL -> 0 / 1


@pytest.mark.parametrize("layout", ["NHWC", "NCHW"])
@pytest.mark.parametrize("W,canvas_w", [(32, 100), (32, 97), (6, 19)])     # 4-pixel path; the byte path (row pitch, width)
def test_pixel_paste_into_canvas(amd, layout, W, canvas_w):
    B, H = 4, 5
    x = _crafted_nhwc(B, H, W, 100 + W)
    rc = np.array([(2, 1), (0, 0), (1, 2), (0, 2)], np.int32)                       # a permuted subset of a 3 x 3 layout
    canvas = torch.full((3 * H + 2, canvas_w, 3), 7, dtype=torch.uint8, device="cuda")
    dev = torch.from_numpy(x if layout == "NHWC" else np.ascontiguousarray(x.transpose(0, 3, 1, 2))).cuda()
    out = amd.ops.pixels_u8(dev, layout, rc=torch.from_numpy(rc).cuda(), canvas=canvas, mean=(0, 0, 0), std=(1 / 255,) * 3)
    assert out is canvas
    want = np.full((3 * H + 2, canvas_w, 3), 7, np.uint8)
    tiles = _host_u8(x)
    for t, (r, c) in enumerate(rc):
        want[r * H:(r + 1) * H, c * W:(c + 1) * W] = tiles[t]
    assert np.array_equal(canvas.cpu().numpy(), want)                               # bytes outside the pasted tiles stay 7


def test_pixel_argument_errors(amd):
    x = torch.zeros((1, 4, 8, 3), device="cuda")
    small = torch.zeros((3, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(AssertionError):                                              # a canvas smaller than one tile
        amd.ops.pixels_u8(x, "NHWC", rc=torch.zeros((1, 2), dtype=torch.int32, device="cuda"), canvas=small)
    with pytest.raises(amd._lib.VqaeHipError):
        amd.ops.pixels_u8(torch.zeros(1, 3, 4, 4))


# ---- 2. unstitch_tiles -----------------------------------------------------------------------------------------------
_NP = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.int32: np.int32, torch.int64: np.int64}


@pytest.mark.parametrize("tile_dtype", list(_NP), ids=lambda d: str(d).replace("torch.", "t_"))
@pytest.mark.parametrize("grid_dtype", list(_NP), ids=lambda d: str(d).replace("torch.", "g_"))
def test_unstitch_is_the_inverse_of_stitch(amd, grid_dtype, tile_dtype):
    rows, cols, th, tw = 3, 5, 8, 8
    hi = min(np.iinfo(_NP[grid_dtype]).max, np.iinfo(_NP[tile_dtype]).max, 1 << 20) + 1       # values both sides hold
    rs = np.random.RandomState(hi % 1000)
    grid = rs.randint(0, hi, size=(rows * th, cols * tw)).astype(_NP[grid_dtype])
    rc = np.array([(r, c) for r in range(rows) for c in range(cols)], np.int32)[rs.permutation(rows * cols)[:9]]
    g_dev, rc_dev = torch.from_numpy(grid).cuda(), torch.from_numpy(rc).cuda()
    tiles = amd.ops.unstitch_tiles(g_dev, rc_dev, th, tw, dtype=tile_dtype)
    assert tiles.dtype == tile_dtype and tuple(tiles.shape) == (9, th, tw)
    want = np.stack([grid[r * th:(r + 1) * th, c * tw:(c + 1) * tw] for r, c in rc])
    assert np.array_equal(tiles.cpu().numpy().astype(np.int64), want.astype(np.int64))
    # stitching them back gives the grid again on the tiles that were cut
    back = torch.zeros_like(g_dev)
    amd.ops.stitch_tiles(tiles, rc_dev, back)
    mask = np.zeros_like(grid, dtype=bool)
    for r, c in rc:
        mask[r * th:(r + 1) * th, c * tw:(c + 1) * tw] = True
    assert np.array_equal(back.cpu().numpy().astype(np.int64), np.where(mask, grid, 0).astype(np.int64))


def test_unstitch_leaves_tiles_outside_the_grid_untouched(amd):
    th = tw = 8
    grid = torch.arange(2 * th * 3 * tw, dtype=torch.int32, device="cuda").reshape(2 * th, 3 * tw)
    rc = torch.tensor([(1, 2), (2, 0), (0, 3), (-1, 1), (0, 0)], dtype=torch.int32, device="cuda")
    out = torch.full((5, th, tw), -5, dtype=torch.int64, device="cuda")
    amd.ops.unstitch_tiles(grid, rc, th, tw, out=out)
    g = grid.cpu().numpy()
    got = out.cpu().numpy()
    assert np.array_equal(got[0], g[th:, 2 * tw:]) and np.array_equal(got[4], g[:th, :tw])
    assert (got[1:4] == -5).all()


# ---- 3. decode_indices_u8 against the handle's own fp32 output --------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("tiny", None), ("tiny", "f16"), ("tiny", "bf16"), ("tinyP", None), ("mid16", None),
                                        ("mid16", "f16")])
def test_decode_indices_u8_matches_own_fp32_output(amd, oracle, name, dtype):
    """mid16 on 128 x 128 reaches the production out-stems: ostem_rb_kernel<16> in fp32 (cout == 3, cin == 16) and stem16.hip's
    ostem16 in f16 (stem 16, 128 % 8 == 0, 128 % 64 == 0); tiny at 32 x 32 takes conv3x3_direct_kernel in the 16-bit modes."""
    nat = _nat(amd, oracle, name, dtype)
    idx = torch.from_numpy(_codes(oracle, name)).cuda()
    x = nat.decode_indices(idx, "NHWC")
    u = nat.decode_indices_u8(idx)
    assert u.dtype == torch.uint8 and tuple(u.shape) == tuple(x.shape)
    _check_against_fp(u.cpu().numpy(), x.cpu().numpy(), f"{name}/{dtype or 'f32'}")
    # compact code widths decode to the same pixels
    narrow = torch.uint8 if nat.spec.num_embeddings <= 256 else torch.uint16
    assert torch.equal(nat.decode_indices_u8(idx.to(narrow)), u)
    assert tuple(nat.decode_indices_u8(idx[:0]).shape) == (0,) + tuple(u.shape[1:])           # B == 0


# ---- 4. against the oracle -------------------------------------------------------------------------------------------
def test_decode_indices_u8_against_oracle(amd, oracle):
    spec, p = oracle.SPECS["tiny"], _params(oracle, "tiny")
    idx = torch.from_numpy(_codes(oracle, "tiny"))
    q = oracle.embed_code(idx, p["encoder.vq_layers.0.embed"]).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        ref = oracle.decoder_forward((q,), p, spec).permute(0, 2, 3, 1).contiguous().numpy()
    u = _nat(amd, oracle, "tiny").decode_indices_u8(idx.cuda()).cpu().numpy()
    # the decoder sits ~1e-5 from the oracle, < 1e-3 of a code value: a pixel may land on the other side of a rounding boundary, never two
    diff = np.abs(u.astype(np.int16) - _quant(_v64(ref)).astype(np.int16))
    record_parity("decode_indices_u8_vs_oracle", model="tiny", dtype="f32", pixels=int(diff.size),
                  share_differing=float((diff > 0).mean()), max_diff=int(diff.max()))
    assert diff.max() <= 1


# ---- 5. region against tiles ---------------------------------------------------------------------------------------------
def _paste_one_by_one(nat, grid, th, tw, r0, c0, rows, cols):
    P = th * nat.factor
    out = np.zeros((rows * P, cols * P, 3), np.uint8)
    for r in range(rows):
        for c in range(cols):
            tile = np.ascontiguousarray(grid[(r0 + r) * th:(r0 + r + 1) * th, (c0 + c) * tw:(c0 + c + 1) * tw]).astype(np.int64)
            out[r * P:(r + 1) * P, c * P:(c + 1) * P] = nat.decode_indices_u8(torch.from_numpy(tile[None]).cuda())[0].cpu().numpy()
    return out


@pytest.mark.parametrize("grid_dtype", [np.uint8, np.uint16])
def test_region_equals_tiles_decoded_one_at_a_time(amd, oracle, grid_dtype):
    """rests on the decoder's bit-exact batch invariance (tests/test_configs_gpu.py)"""
    nat = _nat(amd, oracle, "tiny")
    grid = np.random.RandomState(5).randint(0, 16, size=(3 * 8, 5 * 8)).astype(grid_dtype)
    key = ("one_by_one", 5)
    if key not in _cache:
        _cache[key] = _paste_one_by_one(nat, grid, 8, 8, 0, 0, 3, 5)
    want = _cache[key]
    full = amd.reconstruct_region(nat, grid, 8, batch_size=4)
    assert full.is_cuda and full.dtype == torch.uint8 and tuple(full.shape) == (3 * 32, 5 * 32, 3)
    assert np.array_equal(full.cpu().numpy(), want)
    part = amd.reconstruct_region(nat, grid, 8, r0=1, c0=2, rows=2, cols=3, batch_size=4)
    assert np.array_equal(part.cpu().numpy(), want[32:96, 64:160])
    assert torch.equal(amd.reconstruct_region(nat, torch.from_numpy(grid).cuda(), (8, 8), batch_size=64), full)


# ---- 6. / 7. round trip with the extraction, archive, errors ---------------------------------------------------------------
def _extraction(amd, oracle):
    if "extraction" not in _cache:
        from vqae_amd.extract_embeddings import SyntheticSlideDataset, get_encodings
        nat = _nat(amd, oracle, "tiny")
        ds = SyntheticSlideDataset([(3, 2), (2, 3)], patch_size=32, raw=True)
        grids = dict(get_encodings(nat, ds, batch_size=5, autocast_dtype=None, num_workers=0))
        recs = {s: amd.reconstruct_region(nat, grids[f"images/slide_{s:03d}"], 8).cpu().numpy() for s in range(2)}
        _cache["extraction"] = (nat, ds, grids, recs)
    return _cache["extraction"]


def test_round_trip_with_the_extraction(amd, oracle):
    """the tile the extraction read at patch position (r, c) comes back at pixel (32 r, 32 c)"""
    nat, ds, grids, recs = _extraction(amd, oracle)
    for s, (rows, cols) in enumerate([(3, 2), (2, 3)]):
        assert recs[s].shape == (rows * 32, cols * 32, 3)
    for i in range(len(ds)):
        s, r, c = ds.locate(i)
        idx = nat.encode_u8(ds[i][0][None].cuda())[1]
        want = nat.decode_indices_u8(idx)[0].cpu().numpy()
        assert np.array_equal(recs[s][r * 32:(r + 1) * 32, c * 32:(c + 1) * 32], want), (s, r, c)


def test_reconstruct_hdf5_from_a_written_archive(amd, oracle, tmp_path):
    from vqae_amd.extract_embeddings import save_encodings_hdf5
    nat, ds, grids, recs = _extraction(amd, oracle)
    path = save_encodings_hdf5(tmp_path / "slides.hdf5", nat, ds, batch_size=5, autocast_dtype=None, num_workers=0)
    for s, band_rows in ((0, 2), (1, 1)):
        bands = list(amd.reconstruct_hdf5(nat, path, f"slide_{s:03d}", tile=8, band_rows=band_rows))
        assert [r0 for r0, _ in bands] == list(range(0, recs[s].shape[0] // 32, band_rows))
        assert all(isinstance(b, np.ndarray) and b.dtype == np.uint8 for _, b in bands)
        assert np.array_equal(np.concatenate([b for _, b in bands]), recs[s])
    # the VQAE mirror is taken like the handle
    from vqae_amd.model import VQAE
    model = VQAE.from_spec(amd.SPECS["tiny"])
    model.load_state_dict(_params(oracle, "tiny"), strict=False)
    model = model.cuda().eval()
    assert np.array_equal(amd.reconstruct_region(model, grids["images/slide_000"], 8).cpu().numpy(), recs[0])
    f16 = amd.reconstruct_region(nat, grids["images/slide_000"], 8, autocast_dtype=torch.float16).cpu().numpy()
    want16 = nat.with_dtype(torch.float16).decode_indices_u8(torch.from_numpy(grids["images/slide_000"][:8, :8].astype(np.int64))[None].cuda())
    assert np.array_equal(f16[:32, :32], want16[0].cpu().numpy())


def test_decode_indices_u8_errors_match_decode_indices(amd, oracle):
    p = _params(oracle, "tiny")
    enc_only = amd.NativeVQAE(amd.SPECS["tiny"], {k: v for k, v in p.items() if not k.startswith("decoder.")})
    idx = torch.zeros((1, 8, 8), dtype=torch.int64, device="cuda")
    for call in (enc_only.decode_indices, enc_only.decode_indices_u8):               # a handle without decoder tensors
        with pytest.raises(AssertionError):
            call(idx)
    nat = _nat(amd, oracle, "tiny")
    for call in (nat.decode_indices, nat.decode_indices_u8):                         # a CPU tensor
        with pytest.raises(amd._lib.VqaeHipError):
            call(idx.cpu())
    L = amd._lib
    canvas = torch.zeros((32, 32, 3), dtype=torch.uint8, device="cuda")
    rc = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    p_ = amd.ops._p
    with pytest.raises(AssertionError):                                              # a dense destination with canvas sizes
        L.check(L.lib().vqae_decode_indices_u8(nat._h, p_(idx), L.IDX_I64, 1, 8, 8, None, p_(canvas), 32, 32, None))
    with pytest.raises(AssertionError):                                              # a canvas smaller than one tile
        L.check(L.lib().vqae_decode_indices_u8(nat._h, p_(idx), L.IDX_I64, 1, 8, 8, p_(rc), p_(canvas), 32, 31, None))
    enc_only.close()
