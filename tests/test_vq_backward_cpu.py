"""CPU: the closed-form backward of both quantisers (vqae_amd.layers.vq.backward_reference / projected_backward_reference,
pure torch) in fp64 against the gradients the reference's own autograd gave in fp64 (tests/golden/vq_backward.npz, recorded by
tests/golden/make_vq_backward_golden.py from the unmodified vq_ae/layers/vq.py): 1e-12 relative per tensor.  These two
functions are the yardstick of the HIP kernels in test_vq_backward_gpu.py, which also imports the fixture helpers below."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

PLAIN = ("plain_2x6x11", "plain_2x12x3x5", "plain_1x5x2x3x4")
PROJ8 = ("proj_2x12x3x5", "proj_3x128x8x8", "proj_1x64x33x17", "proj_1x256x4x4")
PROJ4 = ("proj4_2x12x3x5",)
PROJ16 = ("proj16_2x16x3x5",)
GRAD_NAMES = ("x", "proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias")


@pytest.fixture(scope="module")
def bfx():
    return load_golden("vq_backward")


def rel(a, b):
    """||a - b|| / ||b|| in fp64; 0 when both are zero."""
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    n = float(b.norm())
    d = float((a - b).norm())
    return d / n if n > 0 else d


def load_case(fx, name):
    """-> dict: x, g_out [B, C, ...] fp32, g_loss 0-d fp32, cc, sd {name: tensor}, idx, and grads(mode) -> (g32, g64) lists
    (x first, then proj_in.weight, .bias, proj_out.weight, .bias); train mode reads the eval arrays where the generator
    found the two bit-equal."""
    t = lambda k: torch.from_numpy(np.asarray(fx[f"{name}/{k}"]))
    sd = {k[len(name) + 4:]: torch.from_numpy(np.asarray(fx[k])) for k in fx.files if k.startswith(f"{name}/sd/")}
    n = int(fx[f"{name}/n_grads"])
    same = bool(int(fx[f"{name}/train_equals_eval"]))

    def grads(mode):
        m = "eval" if same else mode
        g32 = [t(f"{m}/g32_{i}") for i in range(n)]
        g64 = [g32[0].double() + t(f"{m}/g64lo_0").double()] + [t(f"{m}/g64_{i}") for i in range(1, n)]
        return g32, g64

    return {"x": t("x").float(), "g_out": t("g_out").float(), "g_loss": t("g_loss"), "cc": float(fx[f"{name}/cc"]), "sd": sd,
            "idx": t("idx").long(), "grads": grads, "train_equals_eval": same}


def rows(t):
    """[B, C, ...] -> channel-last rows [N, C] (vq.py:107-116)."""
    return t.permute(0, *range(2, t.dim()), 1).reshape(-1, t.shape[1])


def unrows(r, shape):
    """[N, C] -> [B, C, ...]"""
    return r.reshape(shape[0], *shape[2:], shape[1]).permute(0, -1, *range(1, len(shape) - 1))


def projected_inputs(case, dtype):
    """(g_out rows, x rows, z, q, g_loss, w_in [P, C], w_out [C, P]) of a projected case in `dtype`, q = embed[idx]."""
    sd = case["sd"]
    w_in = sd["proj_in.weight"].to(dtype).flatten(1)
    w_out = sd["proj_out.weight"].to(dtype).flatten(1)
    x = rows(case["x"]).to(dtype)
    z = x @ w_in.t() + sd["proj_in.bias"].to(dtype)
    q = sd["embed"].to(dtype)[case["idx"].reshape(-1)]
    return rows(case["g_out"]).to(dtype), x, z, q, case["g_loss"].to(dtype), w_in, w_out


@pytest.mark.parametrize("name", PROJ8 + PROJ4 + PROJ16)
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_projected_reference_reproduces_autograd_fp64(bfx, name, mode):
    from vqae_amd.layers.vq import projected_backward_reference
    case = load_case(bfx, name)
    g_out, x, z, q, g_loss, w_in, w_out = projected_inputs(case, torch.float64)
    got = projected_backward_reference(g_out, x, z, q, g_loss, case["cc"], w_in, w_out)
    _, g64 = case["grads"](mode)
    assert len(g64) == 5
    for nm, g, ref in zip(GRAD_NAMES, got, g64):
        g = unrows(g, case["x"].shape) if nm == "x" else g.reshape(ref.shape)
        assert g.dtype == torch.float64
        assert rel(g, ref) <= 1e-12, (name, mode, nm, rel(g, ref))


@pytest.mark.parametrize("name", PLAIN)
def test_plain_formula_reproduces_autograd_fp64(bfx, name):
    from vqae_amd.layers.vq import backward_reference
    case = load_case(bfx, name)
    x = rows(case["x"]).double()
    q = case["sd"]["embed"].double()[case["idx"].reshape(-1)]
    got = backward_reference(rows(case["g_out"]).double(), x, q, case["g_loss"].double(), case["cc"])
    for mode in ("eval", "train"):
        _, g64 = case["grads"](mode)
        assert len(g64) == 1
        assert rel(unrows(got, case["x"].shape), g64[0]) <= 1e-12, (name, mode)


def test_reference_is_linear_in_the_upstream_gradients(bfx):
    """None stands for a zero upstream gradient: f(g_out, g_loss) = f(g_out, None) + f(None, g_loss), and f(None, None) = 0."""
    from vqae_amd.layers.vq import backward_reference, projected_backward_reference
    case = load_case(bfx, "proj_2x12x3x5")
    g_out, x, z, q, g_loss, w_in, w_out = projected_inputs(case, torch.float64)
    both = projected_backward_reference(g_out, x, z, q, g_loss, case["cc"], w_in, w_out)
    a = projected_backward_reference(g_out, x, z, q, None, case["cc"], w_in, w_out)
    b = projected_backward_reference(None, x, z, q, g_loss, case["cc"], w_in, w_out)
    none = projected_backward_reference(None, x, z, q, None, case["cc"], w_in, w_out)
    for t, u, v, w in zip(both, a, b, none):
        assert rel(u + v, t) <= 1e-14 and not w.any()
    assert not b[3].any() and not b[4].any()                    # the loss reaches proj_out through nothing
    assert torch.equal(backward_reference(None, x, x - 1.0, None, 0.25), torch.zeros_like(x))
    assert torch.equal(backward_reference(g_out, x, x - 1.0, None, 0.25), g_out)


def test_fixture_records_what_the_tests_assume(bfx):
    """Every case has the indices of both dtypes' runs (the generator asserts they agree), train-mode gradients (stored or
    declared bit-equal to eval), and the reference's own fp32 error is the size the bars are built from (1e-8 .. 1e-6)."""
    assert tuple(bfx["cases"]) == PLAIN + PROJ8 + PROJ4 + PROJ16
    for name in PLAIN + PROJ8 + PROJ4 + PROJ16:
        case = load_case(bfx, name)
        assert int(case["sd"]["first_pass"]) == 0
        assert case["idx"].shape == case["x"].shape[:1] + case["x"].shape[2:]
        for mode in ("eval", "train"):
            g32, g64 = case["grads"](mode)
            assert g32[0].shape == case["x"].shape
            for a, b in zip(g32[:4], g64[:4]):
                assert 1e-9 < rel(a, b) < 1e-6, (name, mode, rel(a, b))
    assert bfx["loop/loss32"].shape == (3,) and bfx["loop/idx"].shape == (3, 2, 8, 8)


def test_entry_points_validate_before_any_launch(amd):
    """projection_dim != 8, channels % 4 != 0 and channels above the kernel's two slabs are refused as vqae_vq_projected_f32
    refuses them (NotImplementedError), before any HIP call; the workspace size is a function of the shapes alone."""
    L = amd._lib
    lib = L.lib()
    one = ctypes.c_void_p(16)           # never dereferenced: validation fails first
    for C, D in ((128, 4), (128, 16), (6, 8), (2, 8), (260, 8), (512, 8)):
        with pytest.raises(NotImplementedError):
            L.check(lib.vqae_vq_projected_backward_f32(one, one, one, one, one, one, one, 64, C, D, 0.25, one, one, one, one, one,
                                                       one, None))
    with pytest.raises(AssertionError):         # rows without x / z / q
        L.check(lib.vqae_vq_projected_backward_f32(None, None, None, None, None, None, None, 64, 128, 8, 0.25, None, None, None,
                                                   None, None, None, None))
    with pytest.raises(NotImplementedError):
        L.check(lib.vqae_vq_backward_f32(one, one, one, one, 0.25, 64, 5000, one, None))
    with pytest.raises(AssertionError):
        L.check(lib.vqae_vq_backward_f32(None, None, None, one, 0.25, 64, 8, one, None))
    ws = lib.vqae_vq_projected_backward_workspace_bytes
    assert ws(262144, 128) == ws(262144, 128) and ws(262144, 128) >= 512 * (17 * 128 + 8) * 8
    assert ws(1, 4) >= (17 * 4 + 8) * 8 and ws(0, 128) > 0
    assert ws(262144, 256) > ws(262144, 128) > ws(1000, 128)
