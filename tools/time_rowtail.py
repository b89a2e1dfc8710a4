"""rdetr_linear_ln_rows_bf16 (csrc/rowtail.hip) against the sequences it replaces on a decoder layer's chain, each replayed as a HIP
graph of 20 back-to-back calls, us per call, alternating old / new, five runs each, at 600, 1,800 and 3,600 rows:
    norm2   library GEMM out_proj + add_layer_norm with pos       -> one launch
    norm1   library GEMM output_proj + add_layer_norm             -> one launch
(the third use, linear2 + norm3 + the decoder's norm at K = 2048, lost this comparison and is gone: profiles/r19/README.md).
Then the row sweep of the short-row kernel against the 256-row-tile kernel of csrc/linear.hip (both behind
ops.linear_ln_k256; rowtail.MAX_ROWS moved out of the way for each side): the crossover is what rowtail.MAX_ROWS is set from.
RDETR_LIB_PATH selects the library build."""
import os
import sys

import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd import _lib, ops, rowtail  # noqa: E402
from tools.time_qpos import timed  # noqa: E402

dev = "cuda:0"
BF = torch.bfloat16


def make(rows, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(BF).to(dev)                # noqa: E731
    return dict(x=t(2, rows // 2, K), res=t(2, rows // 2, 256), pos=t(2, rows // 2, 256), w=t(256, K, scale=K ** -0.5), b=t(256, scale=0.1),
                g1=t(256) * 0.2 + 1, b1=t(256, scale=0.2))


def old_sequence(d, use):
    y = F.linear(d["x"], d["w"], d["b"])
    if use == "norm2":
        return ops.add_layer_norm(y, d["res"], d["g1"], d["b1"], 1e-5, pos=d["pos"])
    return ops.add_layer_norm(d["res"], y, d["g1"], d["b1"], 1e-5)


def new_kernel(d, use):
    extra = {"pos": d["pos"]} if use == "norm2" else None
    return ops.linear_ln_k256(d["x"], d["w"], d["b"], d["res"], d["g1"], d["b1"], 1e-5, extra=extra)


if __name__ == "__main__":
    print("library:", _lib.LIB_PATH, "| rowtail.MAX_ROWS", rowtail.MAX_ROWS)
    default_max = rowtail.MAX_ROWS
    rowtail.MAX_ROWS = 1 << 40
    for use, K in (("norm2", 256), ("norm1", 256)):
        for rows in (600, 1800, 3600):
            d = make(rows, K)
            runs = [(timed(lambda: old_sequence(d, use)), timed(lambda: new_kernel(d, use))) for _ in range(5)]
            print(f"{use:5s} rows {rows:5d}: library GEMM + add_layer_norm " + " ".join(f"{a:.1f}" for a, _ in runs) + " us | one launch " + " ".join(f"{c:.1f}" for _, c in runs)
                  + f" us | new wins every run: {all(c < a for a, c in runs)}")
    print("row sweep, short-row kernel (32 rows per workgroup) against the 256-row-tile kernel:")
    for rows in (1800, 3600, 7200, 14400, 28800, 44646):
        d = make(rows, 256)
        runs = []
        for _ in range(5):
            rowtail.MAX_ROWS = 0
            tall = timed(lambda: new_kernel(d, "norm1"))
            rowtail.MAX_ROWS = 1 << 40
            runs.append((tall, timed(lambda: new_kernel(d, "norm1"))))
        print(f"rows {rows:6d}: tall " + " ".join(f"{a:.1f}" for a, _ in runs) + " us | short " + " ".join(f"{c:.1f}" for _, c in runs)
              + f" us | short wins every run: {all(c < a for a, c in runs)}")
    rowtail.MAX_ROWS = default_max
