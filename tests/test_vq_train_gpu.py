"""GPU parity of training-mode vector quantisation (vq.py:47-94): vq_code_stats_kernel, vq_ema_update_kernel and the two
module mirrors in .train(), each against an fp64 restatement of the same operation (oracle.code_stats_exact,
oracle.update_ema_exact) at ragged sizes, in every index dtype and on rows placed where the kernel changes path.

Bars: counts exact; dw exact wherever every fp32 partial sum is (small integers, single rows), else inside the a-priori
bound of the kernel's documented summation order; the EMA step inside the a-priori bound of its fp32 operations."""
import copy
import math

import numpy as np
import pytest
import torch

from conftest import record_parity

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                       # fp32 unit roundoff
WAVES = 16                                           # wave slices per code (vq_code_stats_kernel)


def code_stats(amd, z, idx, K):
    counts, dw = amd.ops.vq_code_stats(z.cuda(), idx.cuda(), K)
    torch.cuda.synchronize()
    return counts.cpu(), dw.cpu()


def code_stats_entry(amd, z, idx, K, counts, dw):
    """The C entry on the caller's own output buffers (ops.vq_code_stats allocates fresh ones)."""
    L, ops = amd._lib, amd.ops
    N, D = z.shape
    L.check(L.lib().vqae_vq_code_stats_f32(ops._p(z), ops._p(idx), ops.idx_code(idx.dtype), N, K, D, ops._p(counts), ops._p(dw),
                                           ops._stream()))
    torch.cuda.synchronize()


def int_rows(N, D, seed):
    """Integers in [-64, 64] as fp32: every partial sum of up to 2^17 of them is an integer below 2^24, exact in any order."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 65, (N, D), generator=g).float()


def normal_rows(N, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, D, generator=g) * 1.7 + 0.3


def dw_bound(N, dw_abs):
    """Sequential fp32 adds inside a wave slice of ceil(N / 16) rows, then the 16 partials in order: fewer than
    ceil(N / 16) + 16 rounded adds touch any term, each of relative size <= u."""
    return (math.ceil(N / WAVES) + WAVES) * U * dw_abs


# ---- vq_code_stats ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 63, 64, 65, 130, 512])
def test_code_stats_exact_on_integer_rows(amd, oracle, D):
    """Every channel slot per lane (D up to 512), D off the 64-lane grid, slices that are empty (N < 16), shorter than a
    ballot (N = 17, 64), and not multiples of 64 rows; K = 1, few and many codes: bit for bit the fp64 scatter-add."""
    zfull = int_rows(4097, D, 100 + D)
    for N in (1, 15, 17, 64, 1000, 1025, 4097):
        z = zfull[:N].contiguous()
        for K in (1, 5, 300):
            idx = torch.randint(0, K, (N,), generator=torch.Generator().manual_seed(N * 7 + K))
            rc, rdw, _ = oracle.code_stats_exact(z, idx, K)
            counts, dw = code_stats(amd, z, idx, K)
            assert torch.equal(counts.double(), rc), (N, D, K)
            assert torch.equal(dw.double(), rdw), (N, D, K, int((dw.double() != rdw).sum()))


def index_dtypes(K):
    dts = [torch.int32]
    if K <= 256:
        dts.append(torch.uint8)
    if hasattr(torch, "uint16"):
        dts.append(torch.uint16)
    return dts


@pytest.mark.parametrize("D", [3, 65, 130])
@pytest.mark.parametrize("N", [17, 1025])
def test_code_stats_index_dtypes(amd, oracle, N, D):
    """The uint8 / uint16 / int32 instantiations return the int64 call's bits (which are the fp64 reference's)."""
    z = int_rows(N, D, 200 + D)
    for K in (5, 200, 300):
        idx = torch.randint(0, K, (N,), generator=torch.Generator().manual_seed(N + K))
        rc, rdw, _ = oracle.code_stats_exact(z, idx, K)
        c64, dw64 = code_stats(amd, z, idx, K)
        assert torch.equal(c64.double(), rc) and torch.equal(dw64.double(), rdw)
        for dt in index_dtypes(K):
            c, dw = code_stats(amd, z, idx.to(dt), K)
            assert torch.equal(c, c64) and torch.equal(dw, dw64), (K, dt)


@pytest.mark.parametrize("N,D,K", [(1, 3, 5), (17, 65, 300), (1025, 130, 5), (4097, 64, 300)])
def test_code_stats_index_patterns(amd, oracle, N, D, K):
    """All rows on one code: every other code is exactly 0 in counts and in every channel of dw (no stale or
    uninitialised partial leaks out).  Code K - 1 used by the last row only: its sum is that row, bit for bit."""
    z = normal_rows(N, D, 300 + N)
    zi = int_rows(N, D, 301 + N)
    k0 = K // 2
    idx = torch.full((N,), k0, dtype=torch.int64)
    counts, dw = code_stats(amd, zi, idx, K)
    others = torch.arange(K) != k0
    assert float(counts[k0]) == N and torch.equal(dw[k0].double(), zi.double().sum(0))
    assert not counts[others].any() and not dw[others].any()
    counts, dw = code_stats(amd, z, idx, K)           # the same on normal rows: zeros are zeros whatever the data
    assert not counts[others].any() and not dw[others].any()
    idx = torch.randint(0, K - 1, (N,), generator=torch.Generator().manual_seed(N))
    idx[-1] = K - 1
    counts, dw = code_stats(amd, z, idx, K)
    assert float(counts[K - 1]) == 1.0 and torch.equal(dw[K - 1], z[-1])
    rc, _, _ = oracle.code_stats_exact(z, idx, K)
    assert torch.equal(counts.double(), rc)


@pytest.mark.parametrize("N", [1025, 4097])
def test_code_stats_sentinel_rows(amd, N):
    """One row with a code of its own at each place where the row loop changes: the first and last row, each wave-slice
    boundary w * ceil(N / 16) with its neighbours, and rows 63 / 64 / 65 of every slice (the ballot's last lane, the
    next ballot's first two).  Each must come back alone and unchanged; all other rows sit on code 0."""
    D = 130
    per = math.ceil(N / WAVES)
    rows = {0, N - 1}
    for w in range(WAVES):
        rows |= {w * per - 1, w * per, w * per + 1}
        rows |= {w * per + r for r in (63, 64, 65) if r < per}
    rows = sorted(r for r in rows if 0 <= r < N)
    K = max(64, len(rows) + 1)
    z = normal_rows(N, D, 400 + N)
    idx = torch.zeros(N, dtype=torch.int64)
    idx[rows] = torch.arange(1, len(rows) + 1)
    counts, dw = code_stats(amd, z, idx, K)
    assert float(counts[0]) == N - len(rows)
    assert torch.equal(counts[1:len(rows) + 1], torch.ones(len(rows)))
    assert torch.equal(dw[1:len(rows) + 1], z[rows])
    assert not counts[len(rows) + 1:].any() and not dw[len(rows) + 1:].any()


@pytest.mark.parametrize("N,D,K", [(4097, 130, 5), (1000, 8, 300), (20000, 256, 32)])
def test_code_stats_normal_rows_within_order_bound(amd, oracle, N, D, K):
    """z = randn * 1.7 + 0.3: |dw - fp64| <= (ceil(N / 16) + 16) u sum|z| over the code's rows in that channel (dw_bound:
    the kernel's documented order, nothing measured); counts exact."""
    z = normal_rows(N, D, 500 + N)
    idx = torch.randint(0, K, (N,), generator=torch.Generator().manual_seed(N + D))
    rc, rdw, rabs = oracle.code_stats_exact(z, idx, K)
    counts, dw = code_stats(amd, z, idx, K)
    assert torch.equal(counts.double(), rc)
    err, bound = (dw.double() - rdw).abs(), dw_bound(N, rabs)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    record_parity("vq_code_stats_normal_rows", N=N, D=D, K=K, worst_err_over_bound=ratio, max_abs_err=float(err.max()))
    assert bool((err <= bound).all()), ratio


def test_code_stats_properties(amd):
    """Run-to-run identical; a code's outputs depend on its own rows only; the outputs do not depend on what the output
    buffers held (the entry overwrites, it does not accumulate)."""
    N, D, K = 4097, 130, 37
    z = normal_rows(N, D, 600).cuda()
    idx = torch.randint(0, K, (N,), generator=torch.Generator().manual_seed(6)).cuda()
    c1, d1 = amd.ops.vq_code_stats(z, idx, K)
    c2, d2 = amd.ops.vq_code_stats(z, idx, K)
    assert torch.equal(c1, c2) and torch.equal(d1, d2)
    k = 2
    z2 = torch.where((idx == k).unsqueeze(-1), z, normal_rows(N, D, 601).cuda() * 50.0)
    c3, d3 = amd.ops.vq_code_stats(z2, idx, K)
    assert torch.equal(c3, c1) and torch.equal(d3[k], d1[k]) and not torch.equal(d3, d1)
    for fill in (float("nan"), 1e30):
        counts = torch.full((K,), fill, device="cuda")
        dw = torch.full((K, D), fill, device="cuda")
        code_stats_entry(amd, z, idx, K, counts, dw)
        assert torch.equal(counts, c1) and torch.equal(dw, d1), fill


def test_code_stats_edges(amd):
    """embedding_dim above the kernel's 8 channel slots per lane is refused, not truncated; an empty shard (N = 0, what a
    rank without rows hands the all-reduce) gives all-zero counts and dw, through the wrapper and on pre-filled buffers."""
    with pytest.raises(NotImplementedError):
        amd.ops.vq_code_stats(torch.zeros(4, 513).cuda(), torch.zeros(4, dtype=torch.int64).cuda(), 3)
    for D, K in ((8, 5), (130, 300)):
        z, idx = torch.zeros(0, D).cuda(), torch.zeros(0, dtype=torch.int64).cuda()
        counts, dw = amd.ops.vq_code_stats(z, idx, K)
        torch.cuda.synchronize()
        assert counts.shape == (K,) and dw.shape == (K, D) and not counts.any() and not dw.any()
        counts = torch.full((K,), float("nan"), device="cuda")
        dw = torch.full((K, D), float("nan"), device="cuda")
        code_stats_entry(amd, z, idx, K, counts, dw)
        assert not counts.any() and not dw.any()


# ---- vq_ema_update --------------------------------------------------------------------------------------------------------------
def ema_inputs(K, D, seed, zero_start):
    """counts with zeros (code K - 1 always unused once K > 1, code 0 always used so that sum(cluster_size) > 0), dw zero on
    the unused codes, a normal embed_avg, cluster_size at zero or positive."""
    g = torch.Generator().manual_seed(seed)
    counts = torch.randint(0, 50, (K,), generator=g).float() * (torch.rand(K, generator=g) > 0.3)
    counts[0] = 3.0
    if K > 1:
        counts[K - 1] = 0.0
    dw = (torch.randn(K, D, generator=g) * 1.7 + 0.3) * counts.unsqueeze(-1)
    ea = torch.randn(K, D, generator=g)
    cs = torch.zeros(K) if zero_start else torch.rand(K, generator=g) * 20 + 0.5
    return counts, dw, ea, cs


def run_ema_update(ops, counts, dw, ea, cs, decay, alpha):
    e_d, ea_d, cs_d = torch.full_like(ea, float("nan")).cuda(), ea.clone().cuda(), cs.clone().cuda()
    ops.vq_ema_update(e_d, ea_d, cs_d, counts.cuda(), dw.cuda(), decay, alpha)
    torch.cuda.synchronize()
    return e_d.cpu(), ea_d.cpu(), cs_d.cpu()


def ema_ratios(got, ref, bounds):
    """(worst |got - ref| / bound of (cluster_size, embed_avg, embed), whether every element of every output is finite and
    within its bound).  The verdict is taken element by element, so a NaN or an unwritten output fails it; where a bound
    is 0 the result must equal ref."""
    out, ok = [], True
    for x, r, b in ((got[2], ref[2], bounds[0]), (got[1], ref[1], bounds[1]), (got[0], ref[0], bounds[2])):
        err = (x.double() - r).abs()
        ok = ok and bool(torch.isfinite(x).all()) and bool((err <= b).all())
        out.append(float((err[b > 0] / b[b > 0]).max()) if bool((b > 0).any()) else 0.0)
    return out, ok


EMA_SHAPES = [(1, 1), (1, 130), (5, 8), (32, 256), (1000, 8), (1024, 130), (1025, 1), (1025, 8), (3000, 130), (3000, 256)]


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.99, 0.999])
@pytest.mark.parametrize("K,D", EMA_SHAPES)
def test_ema_update_within_fp32_bounds(amd, oracle, K, D, decay):
    """vq_ema_update_kernel against oracle.update_ema_exact (fp64, on float32(decay), float32(1 - decay), float32(alpha),
    float32(K alpha), each formed in double first -- the scalars torch's fp32 tensors see), u = 2^-24:

      |cluster_size - ref| <= 4u M_cs,  M_cs = |cs| d + counts (1 - d)   (two products and one add are 3u; 4u leaves the
      |embed_avg    - ref| <= 4u M_ea,  M_ea = |ea| d + |dw| (1 - d)      second-order terms room)
      |embed        - ref| <= (4u M_ea + c u |ea_ref|) / sm,   c = 2 (13 + ceil(K / 1024)) + 9.

    c counts the relative error of sm = n ((cs + a) / (n + K a)), which divides embed_avg.  n = sum(cluster_size) is a sum
    of non-negative terms, so relative errors add at most: 4u carried in from each term (the first bound; M_cs = cs for
    cs >= 0), ceil(K / 1024) - 1 rounded serial adds per thread, 10 levels of the 1024-wide tree: 13 + ceil(K / 1024).  n
    enters sm twice (the factor and the denominator): 2 (13 + ceil(K / 1024)).  Then 4u carried in by cs in (cs + a) and five
    rounded elementwise operations -- cs + a, n + K a, the division, the product with n, embed_avg / sm: 9.  All of it
    follows from the arithmetic; nothing here is a measured figure.  K > 1024 runs the serial part of the reduction."""
    worst, ok = {}, {}
    for zero_start in (True, False):
        counts, dw, ea, cs = ema_inputs(K, D, 31 * K + D, zero_start)
        ref = oracle.update_ema_exact(None, None, ea, cs, decay, 1e-5, stats=(counts, dw))
        assert float(ref[2].sum()) > 0 and bool((ref[5] > 0).all())
        got = run_ema_update(amd.ops, counts, dw, ea, cs, decay, 1e-5)
        tag = "zero" if zero_start else "positive"
        worst[tag], ok[tag] = ema_ratios(got, ref, oracle.update_ema_bounds(ref))
    record_parity("vq_ema_update", K=K, D=D, decay=decay, err_over_bound_cs_ea_embed_zero_start=worst["zero"],
                  err_over_bound_cs_ea_embed_positive_start=worst["positive"])
    assert ok["zero"] and ok["positive"], worst


# ---- the modules in training mode ---------------------------------------------------------------------------------------------
def check_init_ema(oracle, m, flat, before):
    """_init_ema on a copy of the module against oracle.init_ema in fp64, at the project's bar for this path (rtol 2e-6,
    atol 1e-6: test_ema_bookkeeping_matches_golden); returns the copy's buffers: the state the module's own first training step continues from."""
    m0 = copy.deepcopy(m)
    m0._init_ema(flat.cuda())
    torch.cuda.synchronize()
    e, ea, cs = oracle.init_ema(flat.double(), before[0].double(), before[1].double(), before[2].double())
    got = (m0.embed.cpu(), m0.embed_avg.cpu(), m0.cluster_size.cpu())
    for x, r in zip(got, (e, ea, cs)):
        assert bool(((x.double() - r).abs() <= 2e-6 * r.abs() + 1e-6).all())
    assert torch.equal(got[0], got[1]) and int(m0.first_pass) == 0
    return got


def check_train_step(oracle, m, x, flat, decay, tag, step):
    """One training step of module `m` on input x whose quantiser rows are `flat`, from the module's own buffers (copied
    before the step, so no drift accumulates): indices = the oracle's argmin on the module's embed, q = the straight-through
    lookup in that embed, buffers within the code_stats and EMA bounds combined ((1 - d) dw_bound added on embed_avg)."""
    K, N = m.num_embeddings, flat.shape[0]
    before = (m.embed.cpu(), m.embed_avg.cpu(), m.cluster_size.cpu())
    if int(m.first_pass):
        before = check_init_ema(oracle, m, flat, before)
    out, idx, loss = m(x.cuda())
    torch.cuda.synchronize()
    assert int(m.first_pass) == 0
    oidx, _, _ = oracle.vq_argmin_p4(flat, before[0])
    assert torch.equal(idx.reshape(-1).cpu(), oidx), f"{tag} step {step}: {int((idx.reshape(-1).cpu() != oidx).sum())} index mismatches"
    ref = oracle.update_ema_exact(flat, oidx, before[1], before[2], decay, 1e-5)
    _, _, dw_abs = oracle.code_stats_exact(flat, oidx, K)
    bounds = oracle.update_ema_bounds(ref, float(np.float32(1 - decay)) * dw_bound(N, dw_abs))
    ratios, ok = ema_ratios((m.embed.cpu(), m.embed_avg.cpu(), m.cluster_size.cpu()), ref, bounds)
    record_parity("vq_train_step", module=tag, decay=decay, step=step, err_over_bound_cs_ea_embed=ratios)
    assert ok, (tag, step, ratios)
    q = flat + (before[0][oidx] - flat)
    ref_loss = float(((flat - before[0][oidx]).double() ** 2).mean())
    assert abs(float(loss) - ref_loss) <= 2e-6 * ref_loss
    return out.cpu(), q


@pytest.mark.parametrize("decay", [0.999, 0.9])
def test_ema_quantizer_training_steps(amd, oracle, decay):
    """EMAVectorQuantizer.train() at D = 130 (three channel slots per lane, D % 4 != 0), K = 300 (unused codes: 126 rows),
    three steps on fresh inputs; step 0 initialises the codebook from the batch statistics (first_pass)."""
    from vqae_amd.layers.vq import EMAVectorQuantizer
    D, K = 130, 300
    torch.manual_seed(17)
    m = EMAVectorQuantizer(K, D, 1.0, decay, 1e-5).cuda().train()
    assert int(m.first_pass) == 1
    for step in range(3):
        x = normal_rows(2 * 9 * 7, D, 700 + step).reshape(2, 9, 7, D).permute(0, 3, 1, 2).contiguous()
        flat = x.permute(0, 2, 3, 1).reshape(-1, D).contiguous()
        out, q = check_train_step(oracle, m, x, flat, decay, "EMAVectorQuantizer", step)
        assert torch.equal(out.permute(0, 2, 3, 1).reshape(-1, D), q)


def test_projected_quantizer_training_steps(amd, oracle):
    """ProjectedEMAVectorQuantizer2d(projection_dim = 8).train(): the unfused route, conv2d to 8 channels -> init / update ->
    conv2d back.  proj_in is the channel selection of test_vq_projected_index_exact_on_identical_z, so the quantiser's rows
    are known exactly; out = proj_out(q) in fp64, element by element, to 2e-6 of that element's magnitude sum
    sum_j |w_j q_j| + |b| (the relative bar of an 8-term fp32 dot product, which may cancel)."""
    from vqae_amd.layers.vq import ProjectedEMAVectorQuantizer2d
    C, K, decay = 128, 64, 0.99
    sel = [3, 17, 29, 45, 64, 90, 101, 127]
    torch.manual_seed(18)
    m = ProjectedEMAVectorQuantizer2d(K, C, 1.0, decay, 1e-5, projection_dim=8)
    with torch.no_grad():
        m.proj_in.weight.zero_()
        m.proj_in.bias.zero_()
        for j, c in enumerate(sel):
            m.proj_in.weight[j, c, 0, 0] = 1.0
    m = m.cuda().train()
    w_out, b_out = m.proj_out.weight.detach().cpu(), m.proj_out.bias.detach().cpu()
    for step in range(2):
        z = normal_rows(2 * 9 * 7, 8, 800 + step)
        x = torch.zeros(2, 9, 7, C)
        x[..., sel] = z.reshape(2, 9, 7, 8)
        x = x.permute(0, 3, 1, 2).contiguous()
        zz = amd.ops.conv2d(amd.ops.nchw_to_nhwc(x.cuda()), m._weights()[0], 8, 1, bias_vec=m.proj_in.bias.detach())
        assert torch.equal(zz.reshape(-1, 8).cpu(), z), "conv2d to 8 channels does not reproduce the selected channels"
        out, q = check_train_step(oracle, m, x, z, decay, "ProjectedEMAVectorQuantizer2d", step)
        qn = q.reshape(2, 9, 7, 8).permute(0, 3, 1, 2).double()
        want = torch.nn.functional.conv2d(qn, w_out.double(), b_out.double())
        mag = torch.nn.functional.conv2d(qn.abs(), w_out.double().abs(), b_out.double().abs())
        assert out.shape == want.shape and bool(torch.isfinite(out).all())
        err = (out.double() - want).abs()
        record_parity("vq_projected_train_out", step=step, worst_err_over_magnitude=float((err / mag).max()),
                      worst_err_over_max_abs=float(err.max() / want.abs().max()))
        assert bool((err <= 2e-6 * mag).all())
