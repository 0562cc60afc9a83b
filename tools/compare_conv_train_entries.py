#!/usr/bin/env python3
"""The host entries of csrc/conv_train.hip of two builds, argument for argument, WITHOUT a GPU: every *_forward_f32 / *_backward_f32
call below carries at least one fault, so it returns from its checks before any HIP call.  Compared: return code and
vqae_last_error() text of each call, the value of every *_workspace_bytes / *_supported / *_wgrad_run call.  Raw ctypes on two
library files, pointers are made-up addresses that are never read:

    python tools/compare_conv_train_entries.py PARENT/libvqae_hip.so NEW/libvqae_hip.so OUT.json
"""
import ctypes, hashlib, itertools, json, sys
from ctypes import c_char_p, c_int, c_int64, c_size_t, c_void_p as V

# name -> (stem, takes an image (batch, h, w), a weight layout and a forward workspace)
NODES = {"conv1x1": ("vqae_conv1x1_train", False), "conv_down": ("vqae_conv_down_train", True), "conv3x3": ("vqae_conv3x3_train", True)}
OK_PTR, ODD_PTR, WS8_PTR = 0x10000, 0x10004, 0x10008            # 16-byte aligned; 4 mod 16; 8 mod 16 (fine for a workspace only)
FWD_PTRS, BWD_PTRS = ("x", "a", "b", "w", "y", "ws"), ("g", "x", "a", "b", "w", "g_x", "g_w", "g_a", "g_b", "ws")
GOOD = dict(pre=2, w_layout=1, batch=2, h=4, w=6, cin=16, cout=24)


def load(path):
    lib = ctypes.CDLL(path)
    lib.vqae_last_error.restype = c_char_p
    for stem, image in NODES.values():
        geo = [c_int64, c_int, c_int] if image else [c_int64]
        lay = [c_int] if image else []
        getattr(lib, stem + "_workspace_bytes").restype = c_size_t
        getattr(lib, stem + "_workspace_bytes").argtypes = geo + [c_int, c_int]
        getattr(lib, stem + "_forward_f32").argtypes = [V, V, V, c_int, V] + lay + geo + [c_int, c_int, V] + ([V] if image else []) + [V]
        getattr(lib, stem + "_backward_f32").argtypes = [V, V, V, V, c_int, V] + lay + geo + [c_int, c_int] + [V] * 6
    return lib


def call(lib, node, op, k):
    """one faulty call -> (code, message)"""
    stem, image = NODES[node]
    geo = [k["batch"], k["h"], k["w"]] if image else [k["batch"]]
    lay = [k["w_layout"]] if image else []
    if op == "forward":
        args = [k["x"], k["a"], k["b"], k["pre"], k["w_ptr"]] + lay + geo + [k["cin"], k["cout"], k["y"]] + ([k["ws"]] if image else [])
    else:
        args = [k["g"], k["x"], k["a"], k["b"], k["pre"], k["w_ptr"]] + lay + geo + [k["cin"], k["cout"], k["g_x"], k["g_w"], k["g_a"],
                                                                                  k["g_b"], k["ws"]]
    code = getattr(lib, f"{stem}_{op}_f32")(*args, None)
    assert code != 0, (node, op, k)                                  # a call without a fault would reach the GPU
    return code, lib.vqae_last_error().decode()


def faults(node, op):
    """(name, changes to the good arguments); each one alone makes the call fail on every node it is listed for"""
    image = NODES[node][1]
    ptrs = [n for n in (FWD_PTRS if op == "forward" else BWD_PTRS) if image or op == "backward" or n != "ws"]
    out = []
    for n in ptrs:
        key = "w_ptr" if n == "w" else n
        if n not in ("g_x", "g_w", "g_a", "g_b"):                    # optional outputs may be null
            out.append((f"{n}=null", {key: None, **({"w_layout": 0} if (n, op) == ("ws", "forward") else {})}))
        if n not in ("a", "b", "g_a", "g_b"):                        # scalars have no alignment rule
            out.append((f"{n}=misaligned", {key: ODD_PTR}))
    out += [(f"pre={v}", {"pre": v}) for v in (-1, 3)]
    if image:
        out += [(f"w_layout={v}", {"w_layout": v}) for v in (-1, 2)]
        out += [(f"h={v}", {"h": v}) for v in (0, -2)] + [(f"w={v}", {"w": v}) for v in (0, -3)]
        if node == "conv_down":
            out += [("h odd", {"h": 5}), ("w odd", {"w": 7}), ("h w odd", {"h": 1, "w": 1})]
        per = 4 if node == "conv_down" else 1
        out += [("rows=2^40", {"batch": 1 << 20, "h": 1 << 10, "w": per << 10}), ("rows>2^40", {"batch": (1 << 20) + 1, "h": 1 << 10, "w": per << 10}),
                ("rows huge", {"batch": 1 << 62, "h": 1 << 30, "w": 1 << 30}), ("per>=2^40", {"batch": 1, "h": 1 << 22, "w": 1 << 22})]
    else:
        out += [("rows=2^40", {"batch": 1 << 40}), ("rows>2^40", {"batch": (1 << 40) + 1}), ("rows huge", {"batch": (1 << 63) - 1})]
    out += [(f"batch={v}", {"batch": v}) for v in (0, -1)]
    out += [(f"c={ci},{co}", {"cin": ci, "cout": co}) for ci, co in ((0, 8), (8, 0), (4, 8), (8, 12), (264, 8), (8, 264), (-8, 8), (20, 20))]
    return out


def entry_cases():
    """every single fault, every pair of them, the non-faults that must not hide one (pre with a null a / b, a workspace at 8 mod 16)"""
    for node, op in itertools.product(NODES, ("forward", "backward")):
        good = dict(GOOD, w_ptr=OK_PTR, **{n: OK_PTR for n in set(FWD_PTRS + BWD_PTRS) - {"w"}})
        fs = faults(node, op)
        for name, ch in fs:
            yield node, op, name, {**good, **ch}
            yield node, op, name + " ws 8 mod 16", {**good, "ws": WS8_PTR, **ch}
        for (n1, c1), (n2, c2) in itertools.combinations(fs, 2):
            yield node, op, n1 + " + " + n2, {**good, **c1, **c2}
        for pre, a, b in itertools.product((0, 1, 2), (None, OK_PTR), (None, OK_PTR)):
            yield node, op, f"pre={pre} a={a} b={b} + x=null", {**good, "pre": pre, "a": a, "b": b, "x": None}
            if (pre >= 1 and b is None) or (pre == 2 and a is None):
                yield node, op, f"pre={pre} a={a} b={b}", {**good, "pre": pre, "a": a, "b": b}


def value_cases():
    chans = (0, 4, 8, 12, 16, 24, 32, 40, 64, 96, 128, 136, 200, 248, 256, 264)
    for node, (stem, image) in NODES.items():
        for ci, co in itertools.product(chans, chans):
            yield node, "supported", (ci, co)
        yield node, "wgrad_run", ()
        cc = ((8, 8), (16, 24), (32, 32), (64, 128), (256, 256), (8, 256), (256, 8), (12, 8), (8, 264))
        if image:
            geos = [(b, h, w) for b in (0, 1, 3, 16) for h in (-2, 0, 1, 2, 3, 4, 14, 64, 129) for w in (0, 1, 2, 5, 6, 32, 130)]
            geos += [(1 << 20, 1 << 10, 1 << 10), ((1 << 20) - 1, 1 << 10, 1 << 10), (1 << 18, 1 << 11, 1 << 11), ((1 << 18) + 1, 1 << 11, 1 << 11),
                     (1 << 62, 1 << 30, 1 << 30), (1, 1 << 22, 1 << 22), (-1, 4, 4), (1 << 40, 2, 2), ((1 << 40) - 1, 2, 2)]
        else:
            geos = [(m,) for m in (-1, 0, 1, 2, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1000, 4096, 65536, 65537, 262144, 1048576,
                                   (1 << 31) - 1, 1 << 31, (1 << 40) - 1, 1 << 40, (1 << 40) + 1, (1 << 63) - 1)]
            geos += [(m,) for m in range(3, 40000, 97)]
        for g, (ci, co) in itertools.product(geos, cc):
            yield node, "workspace_bytes", g + (ci, co)


def record(lib):
    rows = [[node, op, name, *call(lib, node, op, k)] for node, op, name, k in entry_cases()]
    rows += [[node, fn, list(args), getattr(lib, f"{NODES[node][0]}_{fn}")(*args)] for node, fn, args in value_cases()]
    return rows


if __name__ == "__main__":
    old, new = record(load(sys.argv[1])), record(load(sys.argv[2]))
    assert len(old) == len(new)
    diff = [(o, n) for o, n in zip(old, new) if o != n]
    res = {"values": len(new), "entry_calls": sum(r[1] in ("forward", "backward") for r in new),
           "nonzero_workspaces": sum(r[1] == "workspace_bytes" and r[3] > 0 for r in new),
           "return_codes": {str(c): sum(r[1] in ("forward", "backward") and r[3] == c for r in new) for c in (-1, -2)},
           "distinct_messages": len({r[4] for r in new if r[1] in ("forward", "backward")}),
           "differences": len(diff), "first_differences": diff[:10],
           "sha256": hashlib.sha256(json.dumps(new).encode()).hexdigest()}
    json.dump(res, open(sys.argv[3], "w"), indent=1)
    print(json.dumps(res, indent=1))
    sys.exit(1 if diff else 0)
