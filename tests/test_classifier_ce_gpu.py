"""GPU: the multi-class route of the slide classifier (the cross-entropy epilogue of csrc/classifier.hip, the n_out-plane
backward of csrc/classifier_train.hip, vqae_classifier_optim_create_ce) against the reference's recorded fp64 gradients and,
where nothing is recorded, against the package's CPU restatement in fp64.

Tolerances are test_classifier_ce_cpu's: the device's gradients may be 4 x e_ref from fp64 (e_ref: the reference's own fp32
distance over the fixture), the loss what the forward's measured logit error allows (ce_loss_bound), the 8 recorded optimiser
steps 4 x the distance of the reference's own fp32 record.  Exact where exactness is claimed: class maps, counts, rows across
entry points, code widths, batch positions and runs, and the 'mean' scaling.

Measured on an MI355X (every line goes through record_parity; profiles/classify_ce_parity_report.jsonl, DESIGN.md section 11
"Multi-class"): worst e over the fixture 3.65e-7 (E1C8O3, e_ref 2.89e-6), 3.91e-7 (E1C16O2, 1.05e-6), 3.77e-7 (E4C8O4,
5.43e-6); the loss at most 2.4 % of its bound (e_logit <= 4.9e-6); K 4096: 1.7e-7; 8 steps next to the reference's own fp32
record: AdamW 2.98e-6 / 3.18e-6, LAMB 1.110e-6 / 1.114e-6; one SAM + AdamW step 3.129e-6 next to 3.124e-6 for the fp32 mirror."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import record_parity
from test_classifier_ce_cpu import (CAM, CASES, VARIANTS, build, case_inputs, ce_loss_bound, cfx, cmodels, cmodels64,  # noqa: F401
                                    e_ref, recorded)
from test_classifier_train_cpu import as_double, e_of, grads_of, params
from test_classifier_train_gpu import BORDER_GRIDS, DTYPES, split

pytestmark = pytest.mark.gpu

EPS = 0.001


def weights_of(cfx, variant):
    return cfx[f"weight_{VARIANTS[variant][2]}"].tolist()


def dev(m, codes, labels, class_weight=None, label_smoothing=0.0, reduction="sum"):
    """the library's own fp64 outputs -> (loss float, [7 arrays], stats [B,20] tensor, packed tensor)"""
    loss, packed, stats = m.native().loss_grad_ce(codes.cuda(), labels.cuda(), weight=class_weight, label_smoothing=label_smoothing,
                                                  reduction=reduction)
    return float(loss), split(m, packed), stats.cpu(), packed.cpu()


def yardstick(m64, codes, labels, **kw):
    """the CPU restatement in fp64 -> (result dict, [7 arrays])"""
    from vqae_amd.classifier_train import ce_loss_and_grads
    res = ce_loss_and_grads(m64, codes.long(), labels, **kw)
    return res, grads_of(m64)


def weight_sum(stats):
    n = 0.0
    for b in range(stats.shape[0]):                                       # the order the library adds the rows in
        n += float(stats[b, 16])
    return n


# ---- fixture parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fixture_parity(cfx, cmodels, cmodels64, variant):
    from vqae_amd.classifier_train import ce_loss_and_grads
    m = cmodels[variant]
    ref = e_ref(cfx, variant)
    worst = 0.0
    for grid, case in CASES:
        codes, labels, kw = case_inputs(cfx, variant, grid, case)
        loss, G, stats, _ = dev(m, codes, labels, **kw)
        e = e_of(G, recorded(cfx, variant, grid, case, "64"))
        worst = max(worst, e)
        record_parity("classifier_ce_grads", variant=variant, grid=grid, case=case, e_dev=e, e_ref=ref)
        assert e <= 4 * ref, (variant, grid, case, e, ref)
        e_logit = float((m(codes.cuda()).cpu().double() - cmodels64[variant](codes)).abs().max())
        loss64 = float(cfx[f"{variant}/{grid}/{case}/loss64"])
        scale = weight_sum(stats) if kw["reduction"] == "mean" else 1.0
        err, bound = abs(loss - loss64) * scale, ce_loss_bound(kw.get("class_weight"), e_logit, labels.numel(), loss64 * scale)
        record_parity("classifier_ce_loss", variant=variant, grid=grid, case=case, err=err, bound=bound, e_logit=e_logit)
        assert err <= bound, (variant, grid, case, err, bound)
        assert float(stats[:, :16].sum()) == labels.numel() and float(stats[:, 19].sum()) == 0
        # the public function: the same numbers in `.grad`, in the parameters' dtype
        res = ce_loss_and_grads(m, codes.cuda(), labels.cuda(), **kw)
        assert res["loss"] == loss and int(res["confusion"].sum()) == labels.numel()
        for p, g in zip(params(m), G):
            assert p.grad.dtype == torch.float32 and p.grad.device == p.device
            assert torch.equal(p.grad, torch.from_numpy(g).float())
    record_parity("classifier_ce_grads_worst", variant=variant, e_dev=worst, e_ref=ref)


# ---- borders and tiling ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", BORDER_GRIDS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_borders_and_tiling(cfx, cmodels, cmodels64, variant, hw):
    m, m64 = cmodels[variant], cmodels64[variant]
    no = VARIANTS[variant][2]
    H, W = hw
    tol = 4 * e_ref(cfx, variant)
    rs = np.random.RandomState(H * 1000 + W)
    codes = torch.from_numpy(rs.randint(0, 256, (3, H, W)).astype(np.int64))
    labels = torch.from_numpy(rs.randint(0, no, (3, H, W)).astype(np.uint8))
    labels[1] = 0                                                        # a slide that is all background (weight 0 below)
    labels[0, 0, 0] = no - 1
    for kw in (dict(class_weight=weights_of(cfx, variant), label_smoothing=EPS), dict()):
        _, G64 = yardstick(m64, codes, labels, reduction="sum", **kw)
        first = None
        for dt in DTYPES:
            loss, G, stats, packed = dev(m, codes.to(dt), labels, **kw)
            if first is None:
                first = (loss, stats, packed)
                e = e_of(G, G64)
                record_parity("classifier_ce_borders", variant=variant, grid=list(hw), weighted=bool(kw), e_dev=e, bound=tol)
                assert e <= tol, (variant, hw, e, tol)
            else:                                                        # the stored width does not change a bit
                assert loss == first[0] and torch.equal(stats, first[1]) and torch.equal(packed, first[2]), (variant, hw, dt)
        loss, _, stats, packed = dev(m, codes.to(DTYPES[0]), labels, **kw)                     # run to run
        assert loss == first[0] and torch.equal(stats, first[1]) and torch.equal(packed, first[2])
    assert first[1][:, :16].sum(1).tolist() == [H * W] * 3
    assert torch.equal(first[1][1], dev(m, codes[1:2], labels[1:2])[2][0])                     # ... and at any batch position


# ---- ownership ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ownership(cfx, cmodels, cmodels64, variant):
    """One weighted position: its whole gradient comes through one position.  Counted twice, or dropped, it is off by its full
    size."""
    m, m64 = cmodels[variant], cmodels64[variant]
    no = VARIANTS[variant][2]
    tw = 30 if variant == "E1C16O2" else 62                              # the tile width this variant runs on (tiles are 14 rows high)
    H, W = 40, 130
    tol = 4 * e_ref(cfx, variant)
    w = [0.0] * (no - 1) + [1.0]
    codes = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (1, H, W)).astype(np.uint8))
    spots = {"tile corner": (14, tw), "last code of a tile": (13, tw - 1), "inside a tile edge": (20, tw),
             "outside a tile edge": (20, tw - 1), "inside a tile's first row": (14, 5), "outside it": (13, 5),
             "one in from the corner": (15, tw + 1), "grid corner": (0, 0), "far grid corner": (H - 1, W - 1)}
    for name, (y, x) in spots.items():
        labels = torch.zeros((1, H, W), dtype=torch.uint8)
        labels[0, y, x] = no - 1
        res, G64 = yardstick(m64, codes, labels, class_weight=w, reduction="sum")
        loss, G, stats, _ = dev(m, codes, labels, class_weight=w)
        assert stats[0, 16] == 1.0
        e = e_of(G, G64)
        assert e <= tol, (variant, name, e, tol)
        assert abs(loss - res["loss"]) <= ce_loss_bound(w, 1e-5, 1, res["loss"]), (variant, name)   # (logits are within 1e-5)


# ---- outputs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_class_map_probabilities_and_counts(cfx, cmodels, variant):
    m = cmodels[variant]
    no = VARIANTS[variant][2]
    w = weights_of(cfx, variant)
    rs = np.random.RandomState(21)
    codes = torch.from_numpy(rs.randint(0, 256, (3, 33, 70)).astype(np.uint8))
    labels = torch.from_numpy(rs.randint(0, no, (3, 33, 70)).astype(np.uint8))
    planted = [(0, 0, 0, no), (0, 13, 61, 255), (1, 14, 62, no + 1), (2, 32, 69, 200), (2, 5, 5, no)]
    for b, y, x, v in planted:
        labels[b, y, x] = v
    lg, pr, cl, st = m.native().forward_ce(codes.cuda(), logits=True, prob=True, cls=True, labels=labels.cuda(), weight=w,
                                           label_smoothing=EPS)
    lg, pr, cl, st = lg.cpu(), pr.cpu(), cl.cpu(), st.cpu()
    assert cl.dtype == torch.uint8 and torch.equal(cl.long(), lg.argmax(1))                    # the argmax of its own logits
    ok = labels < no
    for b in range(3):
        conf = torch.bincount(labels[b][ok[b]].long() * 4 + cl[b][ok[b]].long(), minlength=16).double()
        assert torch.equal(st[b, :16], conf), b                                                # counts from that class map
    assert st[:, 19].tolist() == [2.0, 1.0, 2.0]                                               # n_bad, exact
    p255 = 255.0 * torch.softmax(lg.double(), 1)
    assert int((pr.double() - torch.round(p255)).abs().max()) <= 1
    clear = (p255 - torch.floor(p255) - 0.5).abs() > 1e-3
    assert torch.equal(pr[clear].double(), torch.round(p255)[clear]) and float(clear.double().mean()) > 0.99
    # one output at a time gives the same bits
    only = m.native().forward_ce(codes.cuda(), logits=False, prob=False, cls=True)
    assert only[0] is None and only[1] is None and only[3] is None and torch.equal(only[2].cpu(), cl)
    # the rows of forward_ce are the rows of loss_grad_ce, bit for bit
    loss, G, stats, _ = dev(m, codes, labels, class_weight=w, label_smoothing=EPS)
    assert torch.equal(stats, st)
    # the host's fp64 sums from the device logits
    from vqae_amd.classifier import ce_stats_host
    conf, wsum, nll, smooth, n_bad = ce_stats_host(lg, labels, w, no)
    assert n_bad == 5 and conf.tolist() == st[:, :16].sum(0).reshape(4, 4)[:no, :no].long().tolist()
    assert abs(float(st[:, 16].sum()) - wsum) <= 1e-7 * wsum                                  # (the library's weights are fp32: 2^-24)
    assert abs(float(st[:, 17].sum()) - nll) <= 1e-6 * nll and abs(float(st[:, 18].sum()) - smooth) <= 1e-6 * smooth


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_batch_additivity_and_mean(cfx, cmodels, variant):
    m = cmodels[variant]
    no = VARIANTS[variant][2]
    w = weights_of(cfx, variant)
    rs = np.random.RandomState(22)
    codes = torch.from_numpy(rs.randint(0, 256, (3, 33, 70)).astype(np.uint8))
    labels = torch.from_numpy(rs.randint(0, no, (3, 33, 70)).astype(np.uint8))
    kw = dict(class_weight=w, label_smoothing=EPS)
    loss, G, stats, _ = dev(m, codes, labels, **kw)
    alone = [dev(m, codes[b:b + 1], labels[b:b + 1], **kw) for b in range(3)]
    total = [sum(a[1][i] for a in alone) for i in range(7)]              # fp64 sums of the slides' gradients
    e = e_of(G, total)
    record_parity("classifier_ce_batch_additivity", variant=variant, e_dev=e, bound=4 * e_ref(cfx, variant))
    assert e <= 4 * e_ref(cfx, variant)
    assert abs(loss - sum(a[0] for a in alone)) <= 1e-12 * abs(loss)
    for b in range(3):
        assert torch.equal(alone[b][2][0], stats[b])
    # mean: one scale for the whole batch, applied once, in fp64
    loss_m, G_m, stats_m, _ = dev(m, codes, labels, reduction="mean", **kw)
    n = weight_sum(stats)
    assert torch.equal(stats_m, stats) and loss_m == loss / n
    for a, b in zip(G_m, G):
        assert np.array_equal(a, b * (1.0 / n))


def test_large_table_from_global_memory(cfx):
    """K = 4096, E = 4, n_out = 3: the table gradient is accumulated in HBM, not in LDS."""
    from vqae_amd.classifier import CNNClassifier
    torch.manual_seed(3)
    m = CNNClassifier(4096, 4, 8, 3)
    with torch.no_grad():
        m.layers.embedding.weight.normal_()
    rs = np.random.RandomState(13)
    codes = torch.from_numpy(rs.randint(0, 4096, (2, 33, 70)).astype(np.int32))
    labels = torch.from_numpy(rs.randint(0, 3, (2, 33, 70)).astype(np.uint8))
    kw = dict(class_weight=CAM, label_smoothing=EPS)
    res, G64 = yardstick(as_double(m), codes, labels, reduction="sum", **kw)
    loss, G, stats, packed = dev(m, codes, labels, **kw)
    e = e_of(G, G64)
    record_parity("classifier_ce_grads_k4096", e_dev=e, e_ref=e_ref(cfx, "E4C8O4"))
    assert e <= 4 * e_ref(cfx, "E4C8O4")
    e_logit = float((m(codes.cuda()).cpu().double() - as_double(m)(codes)).abs().max())
    assert abs(loss - res["loss"]) <= ce_loss_bound(CAM, e_logit, labels.numel(), res["loss"])
    loss2, _, stats2, packed2 = dev(m, codes, labels, **kw)
    assert loss2 == loss and torch.equal(stats2, stats) and torch.equal(packed2, packed)


def test_empty_batch(amd, cmodels):
    """batch == 0 through the C ABI: VQAE_OK, zero gradients, zero loss"""
    L = amd._lib
    h = cmodels["E1C8O3"].native()._h
    n = L.lib().vqae_classifier_grad_floats(h)
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    grads = torch.ones(n, dtype=torch.float64, device="cuda")
    loss = torch.ones(1, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                          # noqa: E731
    torch.cuda.synchronize()
    rc = L.lib().vqae_classifier_loss_grad_ce(h, p(buf), L.IDX_U8, 0, 4, 4, p(buf), None, 0.0, 1, p(grads), p(buf), p(loss), p(buf), None)
    torch.cuda.synchronize()
    assert rc == 0 and not grads.any() and float(loss) == 0.0


def test_classify_slide_on_the_device(cfx, cmodels):
    from vqae_amd.classifier import classify_slide
    m = cmodels["E1C8O3"]
    rs = np.random.RandomState(23)
    grid = rs.randint(0, 256, (45, 71)).astype(np.uint8)
    lab = rs.randint(0, 3, (45, 71)).astype(np.uint8)
    got = classify_slide(m, grid, lab, loss="ce", class_weight=CAM, label_smoothing=EPS, logits=True, prob=True)
    host = classify_slide(m, grid, lab, loss="ce", class_weight=CAM, label_smoothing=EPS, prob=True,
                          forward_fn=lambda c: torch.from_numpy(got["logits"])[None])
    assert np.array_equal(got["class"], host["class"]) and got["confusion"].tolist() == host["confusion"].tolist()
    assert got["confusion"][0, 1:].sum() == 0 and got["recall"][0] == 1.0
    assert abs(got["loss"] - host["loss"]) <= 1e-6 * host["loss"] and got["weight_sum"] == pytest.approx(host["weight_sum"], rel=1e-7)
    assert got["precision"] == host["precision"] and got["recall"] == host["recall"]
    assert int(np.abs(got["prob"].astype(int) - host["prob"].astype(int)).max()) <= 1


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
OPT = dict(lr=1e-2, betas=(0.9, 0.999), weight_decay=0.01)


def measure(test, truth, start):
    """make_classifier_optim_golden.measure: max over the tensors of ||dp_test - dp_truth|| / ||dp_truth||, in fp64"""
    worst = 0.0
    for a, b, s in zip(test, truth, start):
        a, b, s = (np.asarray(x, np.float64) for x in (a, b, s))
        worst = max(worst, float(np.linalg.norm(((a - s) - (b - s)).ravel()) / np.linalg.norm((b - s).ravel())))
    return worst


def run_trainer(amd, cfx, kind, steps, sam_rho=None):
    from vqae_amd.optim import ClassifierTrainer
    clf = build(cfx, "E1C8O3")
    codes, labels, kw = case_inputs(cfx, "E1C8O3", "2x37x70", "cam_mean")
    tr = ClassifierTrainer(clf, kind, loss="ce", class_weight=kw["class_weight"], label_smoothing=kw["label_smoothing"],
                           sam_rho=sam_rho, **OPT)
    codes, labels = codes.cuda(), labels.cuda()
    outs = [tr.step(codes, labels, reduction="mean") for _ in range(steps)]
    return tr, clf, outs


@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_eight_recorded_steps(amd, cfx, kind):
    start = [p.detach().numpy().copy() for p in params(build(cfx, "E1C8O3"))]
    p32, p64 = ([cfx[f"optim/{kind}/p{tag}_{i}"] for i in range(7)] for tag in ("32", "64"))
    tr, clf, outs = run_trainer(amd, cfx, kind, 8)
    got = [w.numpy() for w in tr.weights()]
    d, yard = measure(got, p64, start), measure(p32, p64, start)
    losses = [float(loss) for loss, _ in outs]
    record_parity("classifier_ce_trainer", kind=kind, device=d, yardstick=yard, loss_first=losses[0], loss_last=losses[-1])
    assert all(loss.is_cuda and stats.is_cuda and tuple(stats.shape) == (2, 20) for loss, stats in outs)
    assert d <= 4 * yard, (kind, d, yard)
    want = cfx[f"optim/{kind}/loss64"]
    assert abs(losses[0] - want[0]) <= 1e-5 * want[0] and abs(losses[-1] - want[-1]) <= 1e-3 * want[-1] and losses[-1] < losses[0]
    # two identical runs give the same bits
    tr2, _, _ = run_trainer(amd, cfx, kind, 8)
    for a, b in zip(got, tr2.weights()):
        assert np.array_equal(a.view(np.uint32), b.numpy().view(np.uint32))
    # the module takes the weights on request, and the forward reads the stepped image
    tr.sync_to_module()
    codes = torch.from_numpy(cfx["codes_2x37x70"]).cuda()
    assert torch.equal(clf(codes), tr.native.forward(codes)[0])
    tr.close()
    tr2.close()


def test_one_sam_step(amd, cfx):
    """SAM(rho 0.05) over AdamW, one step (two passes): against the fp64 restatement stepped with the SAM mirror.  The device,
    another fp32 evaluation of the same two passes and the same update, may be 4 x as far from fp64 as the fp32 restatement
    stepped with the same mirror is -- the rule of the recorded steps, with the yardstick formed here."""
    from vqae_amd.classifier_train import ce_loss_and_grads
    from vqae_amd.optim import SAM
    codes, labels, kw = case_inputs(cfx, "E1C8O3", "2x37x70", "cam_mean")
    ends = {}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        m = build(cfx, "E1C8O3", dt)
        opt = SAM(params(m), torch.optim.AdamW, rho=0.05, **OPT)
        ce_loss_and_grads(m, codes, labels, **kw)
        opt.first_step(zero_grad=True)
        ce_loss_and_grads(m, codes, labels, **kw)
        opt.second_step(zero_grad=True)
        ends[tag] = [p.detach().numpy().copy() for p in params(m)]
    start = [p.detach().numpy().copy() for p in params(build(cfx, "E1C8O3"))]
    tr, _, outs = run_trainer(amd, cfx, "adamw", 1, sam_rho=0.05)
    got = [w.numpy() for w in tr.weights()]
    d, yard = measure(got, ends["64"], start), measure(ends["32"], ends["64"], start)
    record_parity("classifier_ce_trainer_sam", device=d, yardstick=yard)
    assert d <= 4 * yard, (d, yard)
    first = float(cfx["E1C8O3/2x37x70/cam_mean/loss64"])
    assert abs(float(outs[0][0]) - first) <= 1e-5 * first                # the first pass's loss
    tr.close()


def test_state_dict_round_trip(amd, cfx):
    """4 steps -> state_dict and weights -> a new trainer for 4 more: the bits of 8 steps in one go."""
    from vqae_amd.optim import ClassifierTrainer
    straight, _, _ = run_trainer(amd, cfx, "lamb", 8)
    want = [w.numpy() for w in straight.weights()]
    half, clf, _ = run_trainer(amd, cfx, "lamb", 4)
    sd = half.state_dict()
    assert int(sd["state"][0]["step"]) == 4 and tuple(sd["state"][5]["exp_avg"].shape) == (3, 8, 3, 3)
    half.sync_to_module()
    half.close()
    codes, labels, kw = case_inputs(cfx, "E1C8O3", "2x37x70", "cam_mean")
    tr = ClassifierTrainer(clf, "lamb", lr=99.0, loss="ce", class_weight=kw["class_weight"], label_smoothing=kw["label_smoothing"])
    tr.load_state_dict(sd)
    for _ in range(4):
        tr.step(codes.cuda(), labels.cuda(), reduction="mean")
    for a, b in zip(want, tr.weights()):
        assert np.array_equal(a.view(np.uint32), b.numpy().view(np.uint32))
    tr.close()
    straight.close()
