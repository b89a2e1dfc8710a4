"""ops.tokens_from_levels (csrc/glue.hip) on the pyramids bench.py runs: us per call, 20 back-to-back calls replayed as a HIP graph
and timed with device events.  The features go with the level embeddings, as the stack calls it.  Works against the tree it is
run from; RDETR_LIB_PATH selects the library build."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd import _lib, ops  # noqa: E402
from tools.time_topk import timed  # noqa: E402

PYRAMIDS = {
    "r50": ([(100, 168), (50, 84), (25, 42), (13, 21)], (2, 4)),
    "focalnet": ([(304, 504), (152, 252), (76, 126), (38, 63), (19, 32)], (1, 2)),
}

if __name__ == "__main__":
    print("library:", _lib.LIB_PATH)
    for name, (shapes, batches) in PYRAMIDS.items():
        for B in batches:
            lv = [torch.randn(B, 256, h, w, device="cuda").bfloat16() for h, w in shapes]
            em = list(torch.randn(len(shapes), 256, device="cuda").bfloat16())
            t = timed(lambda: ops.tokens_from_levels(lv, add_vecs=em))            # us
            nbytes = 2 * sum(x.numel() for x in lv) * 2
            print(f"{name} B={B}: tokens_from_levels {t:6.1f} us  ({nbytes/t/1e6:.2f} TB/s)", flush=True)
