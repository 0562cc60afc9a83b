#!/usr/bin/env python3
"""sha256 of the outputs of cfg B's three fp32 'up' blocks (decoder blocks 51, 57, 63: 128 -> 64, 64 -> 32, 32 -> 16 channels) on
seeded inputs, each block run alone through the handle's own dispatch at two low-resolution grids with partial tiles and every
border: the order of every sum in those blocks is part of their recorded results, so a change to their kernels or routes must
leave these digests as they were.  Only `run_blocks` is used, so the same file runs on another checkout or, with VQAE_HIP_LIB, on
another build of the library:

    python tools/hash_up_blocks.py OUT.json
"""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import vqae_amd
from vqae_amd.spec import decoder_block_names
from oracle import vqae_oracle as O

nat = vqae_amd.NativeVQAE(vqae_amd.SPECS["B"], O.make_params(O.SPECS["B"], 0))
names = decoder_block_names(vqae_amd.SPECS["B"])
out = []
for blk in [i for i, n in enumerate(names) if n[1] == "up"]:
    for shape in ((3, 8, 32), (1, 9, 33)):
        x = torch.randn(*shape, names[blk][2], generator=torch.Generator().manual_seed(blk)).cuda()
        y = nat.run_blocks("decoder", blk, 1, x)
        torch.cuda.synchronize()
        out.append({"block": blk, "name": names[blk][0], "cin": names[blk][2], "cout": names[blk][3], "BHW": list(shape),
                    "y": hashlib.sha256(y.cpu().contiguous().numpy().tobytes()).hexdigest()})
json.dump(out, open(sys.argv[1], "w"), indent=1)
print("hashed", len(out), "cases with", vqae_amd._lib.LIB_PATH)
