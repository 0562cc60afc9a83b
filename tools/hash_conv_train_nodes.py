#!/usr/bin/env python3
"""sha256 of every output (y, g_x, g_w, g_a, g_b) of the conv1x1, conv_down and conv3x3 nodes of csrc/conv_train.hip on seeded
inputs, at the op shapes of profiles/conv_train_refactor.json and profiles/conv3x3_train.json and at three edge shapes of each
node's GPU test (M = 33, 129 and the shape of two accumulation runs, Ci, Co = 24, 40): the order of every sum in those nodes is
part of their recorded results, so a change to the shared kernels or to the host code in front of them must leave these digests
as they were.  Raw ctypes on the library file given, so the same script runs on another build of it:

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
json.dump(out, open(sys.argv[2], "w"), indent=1)
print("hashed", len(out), "cases with", sys.argv[1])
