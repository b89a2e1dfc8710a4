"""Outputs of the fused inference feed-forward kernel (ops.ffn_k256, csrc/ffn.hip) on seeded inputs, as .npy files under a
directory, so that two library builds can be compared bit for bit:
    RDETR_LIB_PATH=a.so python tools/dump_ffn_outputs.py OUT_A ; RDETR_LIB_PATH=b.so python tools/dump_ffn_outputs.py OUT_B
    python tools/dump_ffn_outputs.py --compare OUT_A OUT_B
Inputs are generated on the CPU, so they do not depend on the library."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.dump_chain_kernels import compare  # noqa: E402

SHAPES = ((44646, 2048), (16384, 2048), (273, 128))          # rows, d_ffn


def dump(out_dir):
    from relation_detr_amd import _lib, ops
    os.makedirs(out_dir, exist_ok=True)
    print("library:", _lib.LIB_PATH)
    g = torch.Generator().manual_seed(22)
    for rows, F in SHAPES:
        x = torch.randn(rows, 256, generator=g).bfloat16().cuda()
        w1 = (torch.randn(F, 256, generator=g) / 16).bfloat16().cuda()
        b1 = torch.randn(F, generator=g).bfloat16().cuda()
        w2 = (torch.randn(256, F, generator=g) / 45).bfloat16().cuda()
        b2 = (torch.randn(256, generator=g) * 0.1).bfloat16().cuda()
        out = ops.ffn_k256(x, w1, b1, w2, b2)
        torch.cuda.synchronize()
        np.save(os.path.join(out_dir, f"ffn_k256_{rows}x{F}.npy"), out.cpu().view(torch.int16).numpy())
    print("wrote", len(SHAPES), "arrays to", out_dir)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
