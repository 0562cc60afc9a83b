"""GPU: vqae_code_histogram (csrc/code_stats.hip) against np.bincount on the host copy of the same arrays.  Every comparison
is exact integer equality: the kernel holds no float, so there is no tolerance to choose."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

NP_DTYPES = {"u8": np.uint8, "u16": np.uint16, "i32": np.int32, "i64": np.int64}


def host_ref(codes, mask, K, L):
    """codes [B, n] (any integer dtype), mask [B, n] uint8 or None -> (hist int64 [B, L, K], bad int64 [B, 2])"""
    B = codes.shape[0]
    hist, bad = np.zeros((B, L, K), np.int64), np.zeros((B, 2), np.int64)
    for b in range(B):
        c = codes[b].astype(np.int64)
        m = mask[b].astype(np.int64) if mask is not None else np.zeros_like(c)
        ok = (c >= 0) & (c < K)
        okl = m < L
        v = ok & okl
        hist[b] = np.bincount(m[v] * K + c[v], minlength=L * K).reshape(L, K)
        bad[b] = ((~ok).sum(), (ok & ~okl).sum())
    return hist, bad


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(amd, codes, mask, K, **kw):
    hist, bad = amd.ops.code_histogram(codes, mask, num_embeddings=K, **kw)
    return hist.cpu().numpy(), bad.cpu().numpy()


def check(amd, codes, mask, K, L=None):
    """one array set: per grid and pooled, against the host"""
    L = L if L is not None else (3 if mask is not None else 1)
    want, wbad = host_ref(codes, mask, K, L)
    assert (want.sum((1, 2)) + wbad.sum(1) == codes.shape[1]).all()
    dc, dm = dev(codes), dev(mask) if mask is not None else None
    hist, bad = run(amd, dc, dm, K, n_labels=L)
    assert hist.dtype == np.int64 and hist.shape == want.shape
    assert np.array_equal(hist, want) and np.array_equal(bad, wbad)
    hist, bad = run(amd, dc, dm, K, n_labels=L, pooled=True)
    assert hist.shape == (1, L, K) and np.array_equal(hist[0], want.sum(0)) and np.array_equal(bad[0], wbad.sum(0))
    return want


# ---- widths and sizes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 256, 1024])
@pytest.mark.parametrize("dt", ["u8", "u16", "i32", "i64"])
def test_widths_and_sizes(amd, dt, K):
    rng = np.random.RandomState(K + len(dt))
    top = min(K, 256) if dt == "u8" else K
    for n in (1, 63, 64, 65, 7 * 13, 33 * 65, 257 * 1031):            # the last spans several workgroups
        for B in (1, 3):
            codes = rng.randint(0, top, (B, n)).astype(NP_DTYPES[dt])
            mask = rng.randint(0, 3, (B, n)).astype(np.uint8)
            check(amd, codes, None, K)
            check(amd, codes, mask, K)


@pytest.mark.parametrize("dt", ["u16", "i32"])
@pytest.mark.parametrize("K,with_mask", [(8192, True), (65536, False), (65536, True)])
def test_large_tables(amd, dt, K, with_mask):
    """K = 8192 x 3 labels (24578 bins) is the largest shipped shape of the LDS route; K = 65536 takes the global route."""
    rng = np.random.RandomState(K)
    codes = rng.randint(0, K, (2, 300000)).astype(NP_DTYPES[dt])
    codes[0, :5000] = 17                                               # and a run, so a bin is hit by whole waves
    mask = rng.randint(0, 3, (2, 300000)).astype(np.uint8) if with_mask else None
    check(amd, codes, mask, K)


# ---- alignment ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [1, 2, 3])
def test_unaligned_uint8_views(amd, off):
    rng = np.random.RandomState(off)
    n, K = 70001, 256
    cbuf, mbuf = rng.randint(0, K, n + 64).astype(np.uint8), rng.randint(0, 3, n + 64).astype(np.uint8)
    dcb, dmb = dev(cbuf), dev(mbuf)
    for moff in (off, 0, 7):                                           # the mask aligned like the codes, and not
        dc, dm = dcb[off:off + n].view(1, n), dmb[moff:moff + n].view(1, n)
        assert dc.data_ptr() % 16 == off and dc.is_contiguous()
        want, wbad = host_ref(cbuf[None, off:off + n], mbuf[None, moff:moff + n], K, 3)
        hist, bad = run(amd, dc, dm, K)
        assert np.array_equal(hist, want) and np.array_equal(bad, wbad)
    # a batch of odd-sized grids: every second grid starts at an odd address
    dc, dm = dcb[off:off + 3 * 23333].view(3, 23333), dmb[off:off + 3 * 23333].view(3, 23333)
    want, _ = host_ref(cbuf[off:off + 3 * 23333].reshape(3, -1), mbuf[off:off + 3 * 23333].reshape(3, -1), K, 3)
    assert np.array_equal(run(amd, dc, dm, K)[0], want)


def test_unaligned_uint16_view(amd):
    rng = np.random.RandomState(16)
    n, K = 50003, 1024
    cbuf, mbuf = rng.randint(0, K, n + 8).astype(np.uint16), rng.randint(0, 3, n + 8).astype(np.uint8)
    dc, dm = dev(cbuf)[1:1 + n].view(1, n), dev(mbuf)[1:1 + n].view(1, n)
    assert dc.data_ptr() % 16 == 2
    want, wbad = host_ref(cbuf[None, 1:1 + n], mbuf[None, 1:1 + n], K, 3)
    hist, bad = run(amd, dc, dm, K)
    assert np.array_equal(hist, want) and np.array_equal(bad, wbad)


# ---- skew -----------------------------------------------------------------------------------------------------------------
def test_one_code_beyond_fp32(amd):
    """17.64 M equal codes: the bin must read exactly 17 640 000, which an fp32 count cannot hold (2^24 = 16 777 216)."""
    n, K = 4200 * 4200, 256
    d = torch.full((1, n), 7, dtype=torch.uint8, device="cuda")
    hist, bad = run(amd, d, None, K)
    assert hist[0, 0, 7] == 17_640_000 and hist.sum() == n and not bad.any()
    dm = torch.ones((1, n), dtype=torch.uint8, device="cuda")
    hist, bad = run(amd, d, dm, K)
    assert hist[0, 1, 7] == 17_640_000 and hist.sum() == n and not bad.any()
    for pos in (0, n - 1, n // 2 + 13):
        d[0, pos] = 9
        hist, bad = run(amd, d, None, K)
        assert hist[0, 0, 7] == n - 1 and hist[0, 0, 9] == 1 and hist.sum() == n and not bad.any(), pos
        d[0, pos] = 7


@pytest.mark.parametrize("run_len", [1, 2, 63, 64, 65, 1000])
def test_stripes(amd, run_len):
    n, K = 200003, 256
    codes = ((np.arange(n) // run_len) % 5 * 50).astype(np.uint8)[None]
    mask = ((np.arange(n) // (3 * run_len + 1)) % 3).astype(np.uint8)[None]
    check(amd, codes, mask, K)
    check(amd, codes.astype(np.uint16), None, K)


def _draw(rng, p, n, runs):
    if not runs:
        return rng.choice(len(p), size=n, p=p)
    lengths = rng.geometric(1.0 / 48, size=n // 8)                     # mean run 48 codes
    return np.repeat(rng.choice(len(p), size=lengths.size, p=p), lengths)[:n]


@pytest.mark.parametrize("runs", [False, True])
def test_reference_marginal(amd, runs):
    """1 M codes from the reference's K = 256 train marginal (one code holds 48 %), labels from its train label counts."""
    z = load_golden("code_marginals")
    pc = z["embedding_idx_histogram_256_train"].astype(np.float64)
    pl = z["histogram_train"].astype(np.float64)
    rng = np.random.RandomState(256 + runs)
    n = 1 << 20
    codes = _draw(rng, pc / pc.sum(), n, runs)
    mask = _draw(rng, pl / pl.sum(), n, runs)
    assert codes.size == n and mask.size == n
    want = check(amd, codes.astype(np.uint8)[None], mask.astype(np.uint8)[None], 256)
    assert want.sum(1).max() > 0.4 * n                                 # the skew is there


# ---- out-of-range codes and labels, guard words ----------------------------------------------------------------------------
def raw_call(amd, codes, mask, K, L, pooled, accumulate, hist, bad, batch=None):
    lib = amd._lib.lib()
    B, n = codes.shape
    B = B if batch is None else batch
    ws = torch.empty(max(8, lib.vqae_code_histogram_workspace_bytes(B, n, K, L)), dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    amd._lib.check(lib.vqae_code_histogram(p(codes), amd.ops.idx_code(codes.dtype), p(mask), B, n, K, L, int(pooled),
                                           int(accumulate), p(hist), p(bad), p(ws),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", ["u8", "u16", "i32", "i64"])
def test_out_of_range_and_guards(amd, dt):
    K = 200 if dt == "u8" else 256
    npdt = NP_DTYPES[dt]
    rng = np.random.RandomState(7)
    n = 40009
    codes = rng.randint(0, K, (2, n)).astype(npdt)
    mask = rng.randint(0, 3, (2, n)).astype(np.uint8)
    bad_codes = [K, K + 1, np.iinfo(npdt).max]
    if dt in ("i32", "i64"):
        bad_codes += [-1, np.iinfo(npdt).min]
    if dt == "i64":
        bad_codes += [(1 << 32) + 5, (1 << 40) + 1]                    # in range only if truncated to 32 bits
    where = [0, 1, 17, 4095, 4096, 20000, n - 1][:len(bad_codes)]
    for g in range(2):
        for w, c in zip(where, bad_codes):
            codes[g, w] = c
    mask[0, [1, 5, 300, n - 2]] = (255, 3, 255, 3)                     # position 1 is already a bad code
    mask[1, [9000]] = 3
    want, wbad = host_ref(codes, mask, K, 3)
    assert wbad.tolist() == [[len(bad_codes), 3], [len(bad_codes), 1]]

    G, LK = 8, 3 * K
    sentinel = -0x0123456789ABCDEF
    for pooled in (False, True):
        rows = 1 if pooled else 2
        buf = torch.full((G + rows * LK + G + rows * 2 + G,), sentinel, dtype=torch.int64, device="cuda")
        hist = buf[G:G + rows * LK].view(rows, 3, K)
        bad = buf[2 * G + rows * LK:2 * G + rows * LK + rows * 2].view(rows, 2)
        raw_call(amd, dev(codes), dev(mask), K, 3, pooled, 0, hist, bad)           # overwrites the garbage, zero bins included
        h, b, whole = hist.cpu().numpy(), bad.cpu().numpy(), buf.cpu().numpy()
        assert np.array_equal(h, want.sum(0, keepdims=True) if pooled else want)
        assert np.array_equal(b, wbad.sum(0, keepdims=True) if pooled else wbad)
        assert (h.sum((1, 2)) + b.sum(1) == (2 * n if pooled else n)).all()
        guards = np.concatenate([whole[:G], whole[G + rows * LK:2 * G + rows * LK], whole[-G:]])
        assert (guards == sentinel).all()
    # without bad_dev the same table
    hist = torch.full((2, 3, K), sentinel, dtype=torch.int64, device="cuda")
    raw_call(amd, dev(codes), dev(mask), K, 3, False, 0, hist, None)
    assert np.array_equal(hist.cpu().numpy(), want)


# ---- accumulate -------------------------------------------------------------------------------------------------------------
def test_accumulate_carries_and_overwrite(amd):
    rng = np.random.RandomState(40)
    K, n = 256, 30011
    c1, c2 = (rng.randint(0, K, (2, n)).astype(np.uint8) for _ in range(2))
    m1, m2 = (rng.randint(0, 3, (2, n)).astype(np.uint8) for _ in range(2))
    c1[0, :2000] = 3
    m1[0, :2000] = 1
    m2[1, 5] = 9                                                       # one bad label
    w1, b1 = host_ref(c1, m1, K, 3)
    w2, b2 = host_ref(c2, m2, K, 3)
    pre = (2 ** 40 + np.arange(2 * 3 * K, dtype=np.int64)).reshape(2, 3, K)
    pre[0, 1, 3] = 2 ** 32 - 1000                                      # the adds carry across bit 32
    preb = np.array([[2 ** 40, 2 ** 40 + 1], [2 ** 32 - 1, 5]], np.int64)
    out, bad = dev(pre), dev(preb)
    o, b = amd.ops.code_histogram(dev(c1), dev(m1), num_embeddings=K, out=out, bad=bad)
    assert o is out and b is bad
    amd.ops.code_histogram(dev(c2), dev(m2), num_embeddings=K, out=out, bad=bad)
    assert np.array_equal(out.cpu().numpy(), pre + w1 + w2) and np.array_equal(bad.cpu().numpy(), preb + b1 + b2)
    # pooled accumulate over two calls = the sum of everything
    pout = torch.zeros((1, 3, K), dtype=torch.int64, device="cuda")
    amd.ops.code_histogram(dev(c1), dev(m1), num_embeddings=K, pooled=True, out=pout)
    amd.ops.code_histogram(dev(c2), dev(m2), num_embeddings=K, pooled=True, out=pout)
    assert np.array_equal(pout.cpu().numpy()[0], (w1 + w2).sum(0))
    # an empty batch: OK; without accumulate the pooled table is zeroed
    garbage = torch.full((1, 3, K), 77, dtype=torch.int64, device="cuda")
    gb = torch.full((1, 2), 77, dtype=torch.int64, device="cuda")
    raw_call(amd, dev(c1), dev(m1), K, 3, True, 1, garbage, gb, batch=0)
    assert (garbage == 77).all() and (gb == 77).all()
    raw_call(amd, dev(c1), dev(m1), K, 3, True, 0, garbage, gb, batch=0)
    assert not garbage.any() and not gb.any()
    h0, b0 = amd.ops.code_histogram(torch.empty((0, n), dtype=torch.uint8, device="cuda"), num_embeddings=K, pooled=True)
    assert tuple(h0.shape) == (1, 1, K) and not h0.any() and not b0.any()


# ---- batch independence -----------------------------------------------------------------------------------------------------
def test_batch_independence_and_repeatability(amd):
    rng = np.random.RandomState(3)
    K, n = 1024, 99991
    grid = rng.randint(0, K, n).astype(np.uint16)
    gm = rng.randint(0, 3, n).astype(np.uint8)
    other, om = rng.randint(0, K, n).astype(np.uint16), rng.randint(0, 3, n).astype(np.uint8)
    alone = amd.ops.code_histogram(dev(grid[None]), dev(gm[None]), num_embeddings=K)
    batch_c, batch_m = dev(np.stack([grid, other, grid])), dev(np.stack([gm, om, gm]))
    first = amd.ops.code_histogram(batch_c, batch_m, num_embeddings=K)
    second = amd.ops.code_histogram(batch_c, batch_m, num_embeddings=K)
    for a, b in zip(first, second):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert torch.equal(first[0][0], alone[0][0]) and torch.equal(first[0][2], alone[0][0])
    assert torch.equal(first[1][0], alone[1][0]) and torch.equal(first[1][2], alone[1][0])


# ---- module level -------------------------------------------------------------------------------------------------------------
def test_module_code_histogram_on_device(amd):
    from vqae_amd import code_stats as S
    rng = np.random.RandomState(11)
    grid = rng.randint(0, 256, (37, 91)).astype(np.uint8)
    mask = rng.randint(0, 3, (37, 91)).astype(np.uint8)
    host = S.code_histogram(grid, mask, num_embeddings=256)
    devr = S.code_histogram(dev(grid), dev(mask), num_embeddings=256)
    for k in ("joint", "codes", "labels"):
        assert devr[k].dtype == np.int64 and np.array_equal(devr[k], host[k])
    assert (devr["n"], devr["dead"], devr["perplexity"]) == (host["n"], host["dead"], host["perplexity"])
    assert np.array_equal(S.code_histogram(dev(grid), num_embeddings=256)["codes"], host["codes"])
    with pytest.raises(IndexError):
        S.code_histogram(dev(grid), dev(mask), num_embeddings=200)
    mask[3, 3] = 3
    with pytest.raises(ValueError, match="0 .background., 1 .tissue. and 2 .cancer."):
        S.code_histogram(dev(grid), dev(mask), num_embeddings=256)


def test_histogram_hdf5_device_equals_host(amd, tmp_path):
    from code_stats_archive import small_archive
    from vqae_amd import code_stats as S
    small_archive(tmp_path / "enc.hdf5")
    path = str(tmp_path / "enc.hdf5")
    for split in (None, "train", "validation", "test"):
        d = S.histogram_hdf5(path, split=split, train_frac=0.5, out_dir=str(tmp_path / "dev"))
        h = S.histogram_hdf5(path, split=split, train_frac=0.5, out_dir=str(tmp_path / "host"), hist_fn=S.host_code_histogram)
        # the default table size comes from the slides of the split: 512 where a uint16 slide (codes up to 299) is among them
        assert d["stems"] == h["stems"] and d["num_embeddings"] == h["num_embeddings"]
        assert d["num_embeddings"] == (512 if split != "train" else 256)
        for a, b in [(d["pooled"], h["pooled"])] + [(d["slides"][s], h["slides"][s]) for s in h["stems"]]:
            for k in ("joint", "codes", "labels"):
                assert np.array_equal(a[k], b[k])
            assert (a["n"], a["dead"], a["perplexity"]) == (b["n"], b["dead"], b["perplexity"])
        assert [os.path.basename(f) for f in d["files"]] == [os.path.basename(f) for f in h["files"]] and len(d["files"]) == 3
        for fd, fh in zip(d["files"], h["files"]):
            assert open(fd, "rb").read() == open(fh, "rb").read()
    assert S.pos_weight_hdf5(path, "validation", 0.5) == S.pos_weight_hdf5(path, "validation", 0.5, hist_fn=S.host_code_histogram)
