#!/usr/bin/env python3
"""sha256 of every output (y, g_x, g_w, g_a, g_b) of the conv1x1 and conv_down nodes of csrc/conv_train.hip on seeded inputs, at the
op shapes of profiles/conv_train_refactor.json: the order of every sum in those nodes is part of their recorded results, so a
change to the shared kernels must leave these digests as they were.  Raw ctypes on the library file given, so the same script
runs on another build of it (one that lacks newer symbols included):

    python tools/hash_conv_train_nodes.py LIBVQAE_HIP.so OUT.json

tools/bench_conv3x3_train.py --existing-nodes PARENT.json NEW.json stores two such lists next to its timings.
"""
import ctypes, hashlib, json, sys
from ctypes import c_int, c_int64, c_void_p, c_size_t
import torch

lib = ctypes.CDLL(sys.argv[1])
V = c_void_p
lib.vqae_conv1x1_train_workspace_bytes.restype = c_size_t
lib.vqae_conv1x1_train_workspace_bytes.argtypes = [c_int64, c_int, c_int]
lib.vqae_conv1x1_train_forward_f32.argtypes = [V, V, V, c_int, V, c_int64, c_int, c_int, V, V]
lib.vqae_conv1x1_train_backward_f32.argtypes = [V, V, V, V, c_int, V, c_int64, c_int, c_int, V, V, V, V, V, V]
lib.vqae_conv_down_train_workspace_bytes.restype = c_size_t
lib.vqae_conv_down_train_workspace_bytes.argtypes = [c_int64, c_int, c_int, c_int, c_int]
lib.vqae_conv_down_train_forward_f32.argtypes = [V, V, V, c_int, V, c_int, c_int64, c_int, c_int, c_int, c_int, V, V, V]
lib.vqae_conv_down_train_backward_f32.argtypes = [V, V, V, V, c_int, V, c_int, c_int64, c_int, c_int, c_int, c_int, V, V, V, V, V, V]
p = lambda t: V(t.data_ptr())
sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
out = []
a, b = torch.tensor([0.03]).cuda(), torch.tensor([-0.02]).cuda()
for (M, ci, co) in [(1048576, 16, 16), (262144, 64, 64), (65536, 128, 128)]:
    gen = torch.Generator().manual_seed(ci + co)
    x, g = torch.randn(M, ci, generator=gen).cuda(), torch.randn(M, co, generator=gen).cuda()
    w = (torch.randn(co, ci, generator=gen) / ci ** 0.5).cuda()
    for pre in (0, 1, 2):
        y, gx, gw = torch.empty(M, co, device="cuda"), torch.empty(M, ci, device="cuda"), torch.empty(co, ci, device="cuda")
        ga, gb = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
        ws = torch.empty(lib.vqae_conv1x1_train_workspace_bytes(M, ci, co), dtype=torch.uint8, device="cuda")
        assert lib.vqae_conv1x1_train_forward_f32(p(x), p(a), p(b), pre, p(w), M, ci, co, p(y), None) == 0
        assert lib.vqae_conv1x1_train_backward_f32(p(g), p(x), p(a), p(b), pre, p(w), M, ci, co, p(gx), p(gw), p(ga), p(gb), p(ws), None) == 0
        torch.cuda.synchronize()
        out.append({"node": "conv1x1", "M": M, "Ci": ci, "Co": co, "pre": pre, "y": sha(y), "g_x": sha(gx), "g_w": sha(gw), "g_a": sha(ga), "g_b": sha(gb)})
for (name, B, H, ci, co, pre) in [("B_down0_branch", 16, 256, 32, 32, 2), ("B_down0_skip", 16, 256, 16, 32, 1), ("B_down1_branch", 16, 128, 64, 64, 2),
                                  ("B_down1_skip", 16, 128, 32, 64, 1), ("B_down2_branch", 16, 64, 128, 128, 2), ("B_down2_skip", 16, 64, 64, 128, 1),
                                  ("C_down2_branch", 16, 64, 256, 256, 2)]:
    gen = torch.Generator().manual_seed(ci + co)
    x, g = torch.randn(B, H, H, ci, generator=gen).cuda(), torch.randn(B, H // 2, H // 2, co, generator=gen).cuda()
    w0 = (torch.randn(co, ci, 2, 2, generator=gen) / (4 * ci) ** 0.5).cuda()
    for layout in (0, 1):
        w = w0.contiguous(memory_format=torch.channels_last) if layout else w0
        y, gx, gw = torch.empty_like(g), torch.empty_like(x), torch.empty_like(w)
        ga, gb = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
        ws = torch.empty(lib.vqae_conv_down_train_workspace_bytes(B, H, H, ci, co), dtype=torch.uint8, device="cuda")
        assert lib.vqae_conv_down_train_forward_f32(p(x), p(a), p(b), pre, p(w), layout, B, H, H, ci, co, p(y), p(ws), None) == 0
        assert lib.vqae_conv_down_train_backward_f32(p(g), p(x), p(a), p(b), pre, p(w), layout, B, H, H, ci, co, p(gx), p(gw), p(ga), p(gb), p(ws), None) == 0
        torch.cuda.synchronize()
        gwb = gw.as_strided((gw.numel(),), (1,))
        out.append({"node": "conv_down", "shape": name, "w_layout": layout, "pre": pre, "y": sha(y), "g_x": sha(gx), "g_w": sha(gwb), "g_a": sha(ga), "g_b": sha(gb)})
json.dump(out, open(sys.argv[2], "w"), indent=1)
print("hashed", len(out), "cases with", sys.argv[1])
