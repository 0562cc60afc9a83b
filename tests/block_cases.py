"""Shared by tests/test_blocks_gpu.py, tests/test_edges16_gpu.py and tests/test_edges32_*.py: the oracle's per-block activations
of the mid-size models, the handles that run them, the block-parity bars, and the inputs of the edge cases.

Oracle link: tests/golden/taps_<model>_<dtype>.npz hold, for every block of the mid-size models, a strided sample and the
fp64 checksums of the REFERENCE's output (fp32 and under torch.autocast bf16 / f16); `oracle_taps` recomputes the full
tensors on this machine's CPU and re-checks them against those samples.  Taps and handles are made once per
(model, dtype) and process; nothing here changes them afterwards, and no caller may.

Bars (`compare`): fp32 -- max |err| <= 2e-5 * max(1, max|ref|) per block (summation order differs from oneDNN's);
16-bit -- conv operands / outputs are rounded to the 16-bit type on both sides, so outputs are equal except where an
fp32 accumulation lands within summation-order noise of a 16-bit rounding boundary: <= 8 % of the elements may differ by
more than 1e-5 * scale, and NONE by more than 3 ulp16 * scale (tests/test_blocks_gpu.py has the measurements behind them).
`exact_block` / `distance_to_exact`: the block in fp64 without rounding points, the value both 16-bit evaluations
approximate; the HIP block may be no further from it than 1.25x the reference's own 16-bit evaluation.
"""
import contextlib

import numpy as np
import torch

from conftest import load_golden, tap_sample

TDT = {"f32": None, "bf16": torch.bfloat16, "f16": torch.float16}
ULP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
_cache = {}
_handles = {}
_p64 = {}


def autocast_ctx(tag):
    return torch.autocast("cpu", dtype=TDT[tag]) if TDT[tag] is not None else contextlib.nullcontext()


def oracle_taps(oracle, name, tag):
    """Full per-block tensors of the oracle on this machine's CPU, verified against the reference's fixture."""
    key = (name, tag)
    if key in _cache:
        return _cache[key]
    g = load_golden(f"taps_{name}_{tag}")
    spec = oracle.SPECS[name]
    p = oracle.make_params(spec, 0)
    p["encoder.vq_layers.0.embed"] = torch.from_numpy(g["embed"])
    x = oracle.make_patches(int(g["batch"]), int(g["size"]), 0)
    # encoder taps from x; decoder taps from the REFERENCE's indices (q = codebook lookup [+ proj_out]): on another CPU
    # the 16-bit encoder flips a few near-tie indices, which would change q wholesale and make the decoder taps
    # incomparable with the fixture.  (embed[idx] differs from the reference's x + (q - x) by <= 1 fp32 ulp.)
    taps = {}
    with autocast_ctx(tag):
        oracle.encoder_forward(x, p, spec, taps)
        vq = "encoder.vq_layers.0."
        q = p[vq + "embed"][torch.from_numpy(g["idx"].astype(np.int64))].permute(0, 3, 1, 2).contiguous()
        if spec.projection_dim > 0:
            q = torch.nn.functional.conv2d(q, p[vq + "proj_out.weight"], p[vq + "proj_out.bias"])
        taps["q"] = q
        taps["out"] = oracle.decoder_forward((q,), p, spec, taps)
    # the GPU box's CPU may take other oneDNN kernels than the container the fixture was recorded in: allow
    # summation-order noise (fp32) / isolated 16-bit rounding flips here; bit-exactness is the CPU suite's job
    for k in g.files:
        if not k.startswith("tap:"):
            continue
        got, ref = tap_sample(taps[k[4:]].float()).numpy(), g[k]
        scale = max(1.0, float(np.abs(ref).max()))
        err = np.abs(got - ref)
        if tag == "f32":
            assert err.max() <= 1e-5 * scale, (k, err.max())
        else:                # the taps are cumulative (each block runs on the chain's own previous output): flips add up
            rms = float(np.sqrt((err.astype(np.float64) ** 2).mean() / (ref.astype(np.float64) ** 2).mean()))
            assert rms <= 4 * ULP[tag], (k, rms)
    _cache[key] = (spec, p, x, {k: v.float() for k, v in taps.items() if torch.is_tensor(v)})
    return _cache[key]


def native_handle(amd, oracle, name, tag):
    """The handle of model `name` with the taps' parameters in compute dtype `tag`, built under the process's own
    environment (tests that build a handle under a VQAE_* switch make their own)."""
    key = (name, tag)
    if key not in _handles:
        p = oracle_taps(oracle, name, tag)[1]
        _handles[key] = amd.NativeVQAE(amd.SPECS[name], p, compute_dtype=None if tag == "f32" else tag)
    return _handles[key]


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def compare(got_nhwc, ref_nchw, tag, n_blocks):
    got = got_nhwc.permute(0, 3, 1, 2).cpu()
    err = (got - ref_nchw).abs()
    scale = max(1.0, float(ref_nchw.abs().max()))
    mx = float(err.max())
    frac = float((err > 1e-5 * scale).float().mean())
    if tag == "f32":
        ok = mx <= 2e-5 * scale * n_blocks
    else:
        ok = frac <= 0.08 * n_blocks and mx <= 3 * ULP[tag] * scale * n_blocks
    return ok, mx / scale, frac


def exact_block(oracle, p, name, x_nchw, prefix, mode, spec):
    """The block in fp64 with no rounding points: what the 16-bit evaluations (reference autocast and HIP) approximate."""
    if name not in _p64:
        _p64.clear()                                   # one model's fp64 weights at a time
        _p64[name] = {k: v.double() for k, v in p.items() if torch.is_tensor(v) and v.is_floating_point()}
    return oracle.conv_block(x_nchw.double(), _p64[name], prefix, mode, spec)


def distance_to_exact(got_nhwc, ref_nchw, exact_nchw):
    """(rms_hip, rms_ref, max_hip, max_ref) of |. - exact| in fp64."""
    got = got_nhwc.permute(0, 3, 1, 2).cpu().double()
    eh, er = (got - exact_nchw).abs(), (ref_nchw.double() - exact_nchw).abs()
    return float((eh ** 2).mean().sqrt()), float((er ** 2).mean().sqrt()), float(eh.max()), float(er.max())


def block_lists(oracle, spec):
    """(side, [(prefix, mode, cin, cout)], name of the tap in front of the side's first block)."""
    return (("encoder", oracle.encoder_blocks(spec), "stem"), ("decoder", oracle.decoder_blocks(spec), "q"))


def find_block(oracle, spec, mode, cin, pair=False):
    """(side, index, blocks, name of the tap in front of it) of the first block of that mode and input width -- with
    pair, the first that is followed by another 'same' block of its width."""
    for side, blocks, first_in in block_lists(oracle, spec):
        if (side == "decoder") != (mode == "up") and not pair:
            continue
        for i, (prefix, m, ci, co) in enumerate(blocks):
            if m != mode or ci != cin or (pair and not (i + 1 < len(blocks) and blocks[i + 1][1:] == ("same", cin, cin))):
                continue
            return side, i, blocks, (first_in if i == 0 else blocks[i - 1][0])
    raise AssertionError((mode, cin, pair))


def mirror_index(n, size):
    """0 .. n - 1 of a signal of `size` samples continued by its mirror image: 0 1 .. size-1 size-1 .. 1 0 0 1 .."""
    i = torch.arange(n) % (2 * size)
    return torch.where(i < size, i, 2 * size - 1 - i)


def edge_input(tap_nchw, B, H, W):
    """The case's input [B, C, H, W] from the activation tap in front of the block cropped from the top-left
    corner, continued by its mirror image where the case is wider or taller than the tap; the tap's first B images, further ones
    the tap's images rolled by (1, 3) pixels."""
    nb = tap_nchw.shape[0]
    imgs = [torch.roll(tap_nchw[j % nb], shifts=(j // nb, 3 * (j // nb)), dims=(1, 2)) for j in range(B)]
    x = torch.stack(imgs)
    return x[:, :, mirror_index(H, x.shape[2])][:, :, :, mirror_index(W, x.shape[3])].contiguous()


def roll_nhwc(t, dy, dx):
    return torch.roll(t, shifts=(dy % t.shape[1], dx % t.shape[2]), dims=(1, 2))


def f44_block(oracle, p, x_nchw, prefix):
    """The 'same' block in x's dtype with conv2 evaluated as Winograd F(4x4, 3x3) (oracle/winograd_sim.py, test infrastructure
    the product never imports): the CPU yardstick of the routes whose conv2 is F(4x4, 3x3), whose transforms cost accuracy
    that no kernel of that form can avoid.  H and W multiples of 4."""
    import importlib
    sim = importlib.import_module("oracle.winograd_sim")
    direct = oracle.conv_circular3x3
    oracle.conv_circular3x3 = lambda t, w: sim.winograd_conv3x3_circular(t, w, 4)
    try:
        return oracle.fixup_block(x_nchw, p, prefix, "same")
    finally:
        oracle.conv_circular3x3 = direct
