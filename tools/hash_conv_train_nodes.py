#!/usr/bin/env python3
"""sha256 of every output (y, g_x, g_w, g_a, g_b) of the conv1x1, conv_down and conv3x3 nodes of csrc/conv_train.hip on seeded
inputs, at the op shapes of profiles/conv_train_refactor.json and profiles/conv3x3_train.json and at three edge shapes of each
node's GPU test (M = 33, 129 and the shape of two accumulation runs, Ci, Co = 24, 40): the order of every sum in those nodes is
part of their recorded results, so a change to the shared kernels or to the host code in front of them must leave these digests
as they were.  Where the library has it, the conv3x3z node of csrc/conv_train_thin.hip follows (y, g_x, g_w, g_b = g_c, g_bias at
the op shapes of profiles/conv3x3z_train.json and the same edge shapes, Ci, Co = 3, 16 and 16, 3); a build without the node
gives the first three nodes' list alone.  Raw ctypes on the library file given, so the same script runs on another build of it:

    python tools/hash_conv_train_nodes.py LIBVQAE_HIP.so OUT.json
"""
import ctypes, hashlib, json, sys
from ctypes import c_int, c_int64, c_void_p as V, c_size_t
import torch

lib = ctypes.CDLL(sys.argv[1])
# node -> (kernel size, stride, image: called with (batch, h, w), a weight layout and a forward workspace)
NODES = {"conv1x1": (1, 1, False), "conv_down": (2, 2, True), "conv3x3": (3, 1, True)}
for node, (_, _, image) in NODES.items():
    geo, lay = ([c_int64, c_int, c_int], [c_int]) if image else ([c_int64], [])
    getattr(lib, f"vqae_{node}_train_workspace_bytes").restype = c_size_t
    getattr(lib, f"vqae_{node}_train_workspace_bytes").argtypes = geo + [c_int, c_int]
    getattr(lib, f"vqae_{node}_train_forward_f32").argtypes = [V, V, V, c_int, V] + lay + geo + [c_int, c_int, V] + [V] * (1 + image)
    getattr(lib, f"vqae_{node}_train_backward_f32").argtypes = [V, V, V, V, c_int, V] + lay + geo + [c_int, c_int] + [V] * 6
p = lambda t: V(t.data_ptr())
sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
out = []
a, b = torch.tensor([0.03]).cuda(), torch.tensor([-0.02]).cuda()


def run(node, tag, B, OH, OW, ci, co, pre, layout):
    """one forward and backward of a node with output rows [B, OH, OW] (conv1x1: M = B OH OW rows)"""
    k, stride, image = NODES[node]
    H, W = OH * stride, OW * stride
    gen = torch.Generator().manual_seed(ci + co)
    x, g = torch.randn(B, H, W, ci, generator=gen).cuda(), torch.randn(B, OH, OW, co, generator=gen).cuda()
    w = (torch.randn(co, ci, k, k, generator=gen) / (k * k * ci) ** 0.5).cuda()
    if layout:
        w = w.contiguous(memory_format=torch.channels_last)
    geo = [layout, B, H, W] if image else [B * H * W]
    y, gx, gw = torch.empty_like(g), torch.empty_like(x), torch.empty_like(w)
    ga, gb = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    ws = torch.empty(getattr(lib, f"vqae_{node}_train_workspace_bytes")(*geo[int(image):], ci, co), dtype=torch.uint8, device="cuda")
    fwd, bwd = getattr(lib, f"vqae_{node}_train_forward_f32"), getattr(lib, f"vqae_{node}_train_backward_f32")
    assert fwd(p(x), p(a), p(b), pre, p(w), *geo, ci, co, p(y), *([p(ws)] if image else []), None) == 0
    assert bwd(p(g), p(x), p(a), p(b), pre, p(w), *geo, ci, co, p(gx), p(gw), p(ga), p(gb), p(ws), None) == 0
    torch.cuda.synchronize()
    out.append({"node": node, "shape": tag, "BOHOW": [B, OH, OW], "Ci": ci, "Co": co, "pre": pre, "w_layout": layout, "y": sha(y),
                "g_x": sha(gx), "g_w": sha(gw.as_strided((gw.numel(),), (1,))), "g_a": sha(ga), "g_b": sha(gb)})


R = lib.vqae_conv1x1_train_wgrad_run()
EDGES = [("M33", 1, 3, 11), ("M129", 1, 3, 43), ("two_runs", 3, 7, 49) if R == 512 else ("two_runs", 1, 1, 2 * R + 5)]
for (M, ci, co) in [(1048576, 16, 16), (262144, 64, 64), (65536, 128, 128)]:
    for pre in (0, 1, 2):
        run("conv1x1", "op", M // 1024, 32, 32, ci, co, pre, 0)
for (name, B, H, ci, co, pre) in [("B_down0_branch", 16, 256, 32, 32, 2), ("B_down0_skip", 16, 256, 16, 32, 1), ("B_down1_branch", 16, 128, 64, 64, 2),
                                  ("B_down1_skip", 16, 128, 32, 64, 1), ("B_down2_branch", 16, 64, 128, 128, 2), ("B_down2_skip", 16, 64, 64, 128, 1),
                                  ("C_down2_branch", 16, 64, 256, 256, 2)]:
    for layout in (0, 1):
        run("conv_down", name, B, H // 2, H // 2, ci, co, pre, layout)
for (name, B, H, ci, co) in [("B_trunk_128", 64, 32, 128, 128), ("hires_same_16", 16, 256, 16, 16), ("C_trunk_256", 64, 32, 256, 256)]:
    for layout in (0, 1):
        run("conv3x3", name, B, H, H, ci, co, 2, layout)
for layout in (0, 1):
    for pre in (0, 1, 2):
        run("conv3x3", "pre", 4, 32, 32, 64, 64, pre, layout)
for node, (_, _, image) in NODES.items():
    for (tag, B, OH, OW) in EDGES:
        for layout in ((0, 1) if image else (0,)):
            run(node, tag, B, OH, OW, 24, 40, 2, layout)


def run_z(tag, B, H, W, ci, co, pre, layout):
    """one forward and backward of the zero-padded 3x3 node with a 3-channel side (bias behind w, g_bias behind g_b)"""
    gen = torch.Generator().manual_seed(ci + co)
    x, g = torch.randn(B, H, W, ci, generator=gen).cuda(), torch.randn(B, H, W, co, generator=gen).cuda()
    w, bias = (torch.randn(co, ci, 3, 3, generator=gen) / (9 * ci) ** 0.5).cuda(), torch.randn(co, generator=gen).cuda()
    if layout:
        w = w.contiguous(memory_format=torch.channels_last)
    y, gx, gw, gbias = torch.empty_like(g), torch.empty_like(x), torch.empty_like(w), torch.empty_like(bias)
    gb = torch.zeros(1, device="cuda")
    ws = torch.empty(lib.vqae_conv3x3z_train_workspace_bytes(B, H, W, ci, co), dtype=torch.uint8, device="cuda")
    assert lib.vqae_conv3x3z_train_forward_f32(p(x), None, p(b), pre, p(w), p(bias), layout, B, H, W, ci, co, p(y), None, None) == 0
    assert lib.vqae_conv3x3z_train_backward_f32(p(g), p(x), None, p(b), pre, p(w), layout, B, H, W, ci, co, p(gx), p(gw), None, p(gb),
                                                p(gbias), p(ws), None) == 0
    torch.cuda.synchronize()
    out.append({"node": "conv3x3z", "shape": tag, "BOHOW": [B, H, W], "Ci": ci, "Co": co, "pre": pre, "w_layout": layout, "y": sha(y),
                "g_x": sha(gx), "g_w": sha(gw.as_strided((gw.numel(),), (1,))), "g_b": sha(gb), "g_bias": sha(gbias)})


if hasattr(lib, "vqae_conv3x3z_train_forward_f32"):
    geo = [c_int64, c_int, c_int]
    lib.vqae_conv3x3z_train_workspace_bytes.restype = c_size_t
    lib.vqae_conv3x3z_train_workspace_bytes.argtypes = geo + [c_int, c_int]
    lib.vqae_conv3x3z_train_forward_f32.argtypes = [V, V, V, c_int, V, V, c_int] + geo + [c_int, c_int, V, V, V]
    lib.vqae_conv3x3z_train_backward_f32.argtypes = [V, V, V, V, c_int, V, c_int] + geo + [c_int, c_int] + [V] * 7
    for (name, B, H, ci, co, pre) in [("in_stem_16", 16, 256, 3, 16, 0), ("out_stem_16", 16, 256, 16, 3, 0), ("in_stem_8", 8, 512, 3, 8, 0),
                                      ("out_stem_8", 8, 512, 8, 3, 0)]:
        for layout in (0, 1):
            run_z(name, B, H, H, ci, co, pre, layout)
    for (tag, B, H, W) in EDGES:
        for layout in (0, 1):
            for ci, co in ((3, 16), (16, 3)):
                run_z(tag, B, H, W, ci, co, 1, layout)
json.dump(out, open(sys.argv[2], "w"), indent=1)
print("hashed", len(out), "cases with", sys.argv[1])
