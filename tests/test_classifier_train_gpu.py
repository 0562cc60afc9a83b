"""GPU: the fused loss-and-gradients path of the slide classifier (csrc/classifier_train.hip) against the reference's recorded
fp64 gradients and, where nothing is recorded, against the package's CPU restatement in fp64.

The tolerance is not a free parameter: with e(G) = max over the seven tensors of max|G - G64| / max|G64| the device may be
4 x e_ref away from fp64, e_ref being e of the reference's own fp32 gradients over the fixture (the same products summed in
another order; see test_classifier_train_cpu.py).  The loss may differ from fp64 by what the forward's measured logit error
allows: max(1, pos_weight) * e_logit * n_valid + 1e-6 * |loss64|."""
import numpy as np
import pytest
import torch

from conftest import record_parity
from test_classifier_train_cpu import (CASES, POS_WEIGHTS, VARIANTS, as_double, build, case_inputs, e_of, e_ref,  # noqa: F401
                                       grads_of, loss_bound, params, recorded, tfx, tmodels, tmodels64)

pytestmark = pytest.mark.gpu

DTYPES = [torch.uint8, torch.int32, torch.int64] + ([torch.uint16] if hasattr(torch, "uint16") else [])
BORDER_GRIDS = ((1, 1), (1, 9), (9, 1), (3, 3), (31, 33), (33, 31), (64, 96), (131, 257))


def split(m, packed):
    """packed fp64 gradients -> the seven arrays"""
    out, o = [], 0
    for p in params(m):
        out.append(packed[o:o + p.numel()].view(p.shape).cpu().numpy())
        o += p.numel()
    assert o == packed.numel()
    return out


def dev(m, codes, mask, target=None, pos_weight=1.0, reduction="sum"):
    """the library's own fp64 outputs -> (loss float, [7 arrays], stats [B,6] tensor, packed tensor)"""
    loss, packed, stats = m.native().loss_grad(codes.cuda(), mask.cuda(), target=None if target is None else target.cuda(),
                                               pos_weight=pos_weight, reduction=reduction)
    return float(loss), split(m, packed), stats.cpu(), packed.cpu()


def yardstick(m64, codes, mask, **kw):
    """the CPU restatement in fp64 -> (result dict, [7 arrays])"""
    from vqae_amd.classifier_train import loss_and_grads
    res = loss_and_grads(m64, codes.long(), mask, **kw)
    return res, grads_of(m64)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fixture_parity(tfx, tmodels, tmodels64, variant):
    from vqae_amd.classifier_train import loss_and_grads
    m = tmodels[variant]
    ref = e_ref(tfx, variant)
    worst = 0.0
    for grid, case in CASES:
        codes, mask, kw = case_inputs(tfx, grid, case)
        loss, G, stats, _ = dev(m, codes, mask, **kw)
        G64 = recorded(tfx, variant, grid, case, "64")
        e = e_of(G, G64)
        worst = max(worst, e)
        record_parity("classifier_train_grads", variant=variant, grid=grid, case=case, e_dev=e, e_ref=ref)
        assert e <= 4 * ref, (variant, grid, case, e, ref)
        e_logit = float((m(codes.cuda()).cpu().double() - tmodels64[variant](codes)).abs().max())
        n = int((mask != 0).sum())
        loss64 = float(tfx[f"{variant}/{grid}/{case}/loss64"])
        scale = n if case == "mean" else 1
        err, bound = abs(loss - loss64) * scale, loss_bound(kw["pos_weight"], e_logit, n, loss64 * scale)
        record_parity("classifier_train_loss", variant=variant, grid=grid, case=case, err=err, bound=bound, e_logit=e_logit)
        assert err <= bound, (variant, grid, case, err, bound)
        assert float(stats[:, 4].sum()) == n
        # the public function: the same numbers in `.grad`, in the parameters' dtype
        res = loss_and_grads(m, codes.cuda(), mask.cuda(), **{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()})
        assert res["loss"] == loss and res["n_valid"] == n
        for p, g in zip(params(m), G):
            assert p.grad.dtype == torch.float32 and p.grad.device == p.device
            assert torch.equal(p.grad, torch.from_numpy(g).float())
    record_parity("classifier_train_grads_worst", variant=variant, e_dev=worst, e_ref=ref)


@pytest.mark.parametrize("hw", BORDER_GRIDS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_borders_and_tiling(tfx, tmodels, tmodels64, variant, hw):
    m, m64 = tmodels[variant], tmodels64[variant]
    H, W = hw
    tol = 4 * e_ref(tfx, variant)
    rs = np.random.RandomState(H * 1000 + W)
    codes = torch.from_numpy(rs.randint(0, 256, (3, H, W)).astype(np.int64))
    mixed = torch.from_numpy(rs.randint(0, 3, (3, H, W)).astype(np.uint8))
    mixed[1] = 0                                                         # a slide that is all background
    mixed[0, 0, 0] = 2                                                   # (at least one valid code on the smallest grids)
    valid = torch.from_numpy(rs.randint(1, 3, (3, H, W)).astype(np.uint8))
    for mask in (mixed, valid):
        pw = POS_WEIGHTS[1]
        _, G64 = yardstick(m64, codes, mask, pos_weight=pw)
        first = None
        for dt in DTYPES:
            loss, G, stats, packed = dev(m, codes.to(dt), mask, pos_weight=pw)
            if first is None:
                first = (loss, stats, packed)
                e = e_of(G, G64)
                assert e <= tol, (variant, hw, e, tol)
            else:                                                        # the stored width does not change a bit
                assert loss == first[0] and torch.equal(stats, first[1]) and torch.equal(packed, first[2]), (variant, hw, dt)
        loss, _, stats, packed = dev(m, codes.to(DTYPES[0]), mask, pos_weight=pw)             # run to run
        assert loss == first[0] and torch.equal(stats, first[1]) and torch.equal(packed, first[2])
    assert first[1][:, 4].tolist() == [H * W] * 3


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_batch_additivity_and_stats_rows(tfx, tmodels, variant):
    m = tmodels[variant]
    rs = np.random.RandomState(21)
    codes = torch.from_numpy(rs.randint(0, 256, (3, 33, 70)).astype(np.uint8))
    mask = torch.from_numpy(rs.randint(0, 3, (3, 33, 70)).astype(np.uint8))
    pw = POS_WEIGHTS[1]
    loss, G, stats, _ = dev(m, codes, mask, pos_weight=pw)
    alone = [dev(m, codes[b:b + 1], mask[b:b + 1], pos_weight=pw) for b in range(3)]
    total = [sum(a[1][i] for a in alone) for i in range(7)]              # fp64 sums of the slides' gradients
    assert e_of(G, total) <= 4 * e_ref(tfx, variant)
    assert abs(loss - sum(a[0] for a in alone)) <= 1e-12 * abs(loss)
    _, _, fwd = m.native().forward(codes.cuda(), logits=False, mask=mask.cuda(), pos_weight=pw)
    assert torch.equal(stats, fwd.cpu())                                 # vqae_classifier_forward's rows, bit for bit
    for b in range(3):
        assert torch.equal(alone[b][2][0], stats[b])
    # mean: one scale for the whole batch, applied in fp64
    loss_m, G_m, stats_m, _ = dev(m, codes, mask, pos_weight=pw, reduction="mean")
    n = float(stats[:, 4].sum())
    assert torch.equal(stats_m, stats) and loss_m == loss / n
    for a, b in zip(G_m, G):
        assert np.array_equal(a, b * (1.0 / n))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ownership(tfx, tmodels, tmodels64, variant):
    """One valid code: its whole gradient comes through one position.  Counted twice, or dropped, it is off by its full size."""
    m, m64 = tmodels[variant], tmodels64[variant]
    tw = 30 if variant == "E1C16O1" else 62                              # the tile width this variant runs on (tiles are 14 rows high)
    H, W = 40, 130
    tol = 4 * e_ref(tfx, variant)
    codes = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (1, H, W)).astype(np.uint8))
    spots = {"tile corner": (14, tw), "last code of a tile": (13, tw - 1), "inside a tile edge": (20, tw),
             "outside a tile edge": (20, tw - 1), "inside a tile's first row": (14, 5), "outside it": (13, 5),
             "one in from the corner": (15, tw + 1), "grid corner": (0, 0), "far grid corner": (H - 1, W - 1)}
    for j, (name, (y, x)) in enumerate(spots.items()):
        mask = torch.zeros((1, H, W), dtype=torch.uint8)
        mask[0, y, x] = 1 + j % 2
        res, G64 = yardstick(m64, codes, mask, pos_weight=POS_WEIGHTS[1])
        loss, G, stats, _ = dev(m, codes, mask, pos_weight=POS_WEIGHTS[1])
        assert stats[0, 4] == 1
        e = e_of(G, G64)
        assert e <= tol, (variant, name, e, tol)
        assert abs(loss - res["loss"]) <= loss_bound(POS_WEIGHTS[1], 1e-5, 1, res["loss"]), (variant, name)   # (logits are within 1e-5)


def test_codes_outside_the_table(tfx, tmodels64):
    """Through ops there is no check: a code outside 0 .. K-1 is a zero vector and no gradient reaches a table row for it."""
    from vqae_amd.classifier import CNNClassifier
    variant, K = "E1C8O1", 200
    full = tmodels64[variant]
    sd = {k: v.clone() for k, v in full.state_dict().items()}
    sd["layers.0.weight"][K:] = 0                                        # the yardstick: rows K .. 255 are zero vectors
    m64 = CNNClassifier(256, 1, 8, 1)
    m64.load_state_dict(sd)
    m64 = m64.double()
    small = CNNClassifier(K, 1, 8, 1)
    sd32 = {k: v.float() for k, v in sd.items()}
    sd32["layers.0.weight"] = sd32["layers.0.weight"][:K]
    small.load_state_dict(sd32)
    rs = np.random.RandomState(9)
    codes = torch.from_numpy(rs.randint(0, 256, (2, 37, 70)).astype(np.uint8))
    mask = torch.from_numpy(rs.randint(0, 3, (2, 37, 70)).astype(np.uint8))
    assert int((codes >= K).sum()) > 100
    _, G64 = yardstick(m64, codes, mask, pos_weight=2.0)
    assert np.abs(G64[0][K:]).max() > 0                                  # autograd does send a gradient to those rows
    G64[0] = G64[0][:K]                                                  # ... which the device's table does not have
    loss, G, stats, packed = dev(small, codes, mask, pos_weight=2.0)
    assert G[0].shape == (K, 1)
    assert e_of(G, G64) <= 4 * e_ref(tfx, variant)
    wild = codes.to(torch.int32)
    wild[codes >= K] = torch.from_numpy(rs.choice([-1, -70000, K, 65536, 2 ** 31 - 1], int((codes >= K).sum())).astype(np.int32))
    loss2, _, stats2, packed2 = dev(small, wild, mask, pos_weight=2.0)
    assert loss2 == loss and torch.equal(stats2, stats) and torch.equal(packed2, packed)


def test_table_from_global_memory(tfx):
    """K = 4096, E = 4: the table gradient is accumulated in HBM, not in LDS."""
    from vqae_amd.classifier import CNNClassifier
    torch.manual_seed(3)
    m = CNNClassifier(4096, 4, 8, 1)
    with torch.no_grad():
        m.layers.embedding.weight.normal_()
    rs = np.random.RandomState(13)
    codes = torch.from_numpy(rs.randint(0, 4096, (2, 37, 70)).astype(np.int32))
    mask = torch.from_numpy(rs.randint(0, 3, (2, 37, 70)).astype(np.uint8))
    res, G64 = yardstick(as_double(m), codes, mask, pos_weight=POS_WEIGHTS[1])
    loss, G, stats, packed = dev(m, codes, mask, pos_weight=POS_WEIGHTS[1])
    e = e_of(G, G64)
    record_parity("classifier_train_grads_k4096", e_dev=e, e_ref=e_ref(tfx, "E4C8O1"))
    assert e <= 4 * e_ref(tfx, "E4C8O1")
    assert abs(loss - res["loss"]) <= 1e-5 * res["loss"]
    loss2, _, stats2, packed2 = dev(m, codes, mask, pos_weight=POS_WEIGHTS[1])
    assert loss2 == loss and torch.equal(stats2, stats) and torch.equal(packed2, packed)


def test_empty_batch(amd, tmodels):
    """batch == 0 through the C ABI: VQAE_OK, zero gradients, zero loss"""
    import ctypes
    L = amd._lib
    h = tmodels["E1C8O1"].native()._h
    n = L.lib().vqae_classifier_grad_floats(h)
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    grads = torch.ones(n, dtype=torch.float64, device="cuda")
    loss = torch.ones(1, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                          # noqa: E731
    torch.cuda.synchronize()
    rc = L.lib().vqae_classifier_loss_grad(h, p(buf), L.IDX_U8, 0, 4, 4, p(buf), None, 1.0, 0, p(grads), p(buf), p(loss), p(buf), None)
    torch.cuda.synchronize()
    assert rc == 0 and not grads.any() and float(loss) == 0.0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_one_sgd_step(tfx, variant):
    from vqae_amd.classifier_train import loss_and_grads
    lr, grid, case = 1e-2, "2x37x70", "pw1"
    codes, mask, kw = case_inputs(tfx, grid, case)
    on_dev, on_cpu = build(tfx, variant), build(tfx, variant)
    nat = on_dev.native()
    loss_and_grads(on_dev, codes.cuda(), mask.cuda(), **kw)
    loss_and_grads(on_cpu, codes, mask, **kw)
    torch.optim.SGD(on_dev.parameters(), lr=lr).step()
    torch.optim.SGD(on_cpu.parameters(), lr=lr).step()
    ref = e_ref(tfx, variant)
    for p, q, g64 in zip(params(on_dev), params(on_cpu), recorded(tfx, variant, grid, case, "64")):
        assert float((p.detach() - q.detach()).abs().max()) <= lr * 4 * ref * float(np.abs(g64).max()), variant
    # the next call sees the stepped weights, through the same handle
    r_dev = loss_and_grads(on_dev, codes.cuda(), mask.cuda(), **kw)
    assert on_dev.native() is nat
    r_cpu = loss_and_grads(on_cpu, codes, mask, **kw)
    assert abs(r_dev["loss"] - r_cpu["loss"]) <= 1e-3 * abs(r_cpu["loss"])
    assert r_dev["loss"] != float(tfx[f"{variant}/{grid}/{case}/loss64"])


def test_a_short_run(amd, tmp_path):
    """20 steps on a two-slide archive whose labels are a fixed function of the codes: the training loss goes down."""
    from vqae_amd import hdf5
    from vqae_amd.classifier import CNNClassifier
    from vqae_amd.classifier_train import train_hdf5
    rs = np.random.RandomState(17)
    label = np.where(np.arange(256) < 32, 0, np.where(np.arange(256) % 3 == 0, 2, 1)).astype(np.uint8)
    images = {"normal_001": rs.randint(0, 256, (48, 80)).astype(np.uint8), "tumor_001": rs.randint(0, 256, (40, 90)).astype(np.uint8)}
    path = hdf5.write_hdf5(tmp_path / "enc.hdf5", {"images": images, "masks": {k + "_mask": label[v] for k, v in images.items()}})
    torch.manual_seed(0)
    clf = CNNClassifier()
    # train_frac 0.4: with one slide of each kind both train (round(0.4) = 0 -> the first slide trains), none validates
    hist = train_hdf5(clf, path, torch.optim.Adam(clf.parameters(), lr=0.03), epochs=20, batch_size=2, train_frac=0.4,
                      pos_weight=2.0, seed=1, reduction="mean", aligned_crops=True)
    assert len(hist) == 20 and all(len(e["steps"]) == 1 and e["steps"][0]["shape"] == (2, 40, 80) for e in hist)
    assert all(e["steps"][0]["stems"] == ["normal_001", "tumor_001"] for e in hist)
    assert hist[0]["val"]["n_valid"] == 0
    first, last = hist[0]["steps"][0]["loss"], hist[-1]["steps"][0]["loss"]
    print(f"short run: loss {first:.4f} -> {last:.4f}")
    assert np.isfinite(last) and last < first
