"""ops.topk (csrc/topk.hip) on the selections bench.py's three configurations run: us per call, 20 back-to-back calls replayed as a
HIP graph and timed with device events.  Scores are shaped like the stack's: bf16 class-logit maxima around the class prior for the
two-stage proposals, fp32 sigmoid probabilities for PostProcess.  Works against the tree it is run from; RDETR_LIB_PATH selects the
library build."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd import _lib, ops  # noqa: E402


def timed(fn, reps=20, rounds=30):
    """us per call: `reps` calls captured into one graph, `rounds` replays between two device events."""
    with torch.no_grad():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
        for _ in range(5):
            g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * rounds) * 1e3


SHAPES = [(2, 22323, 900, torch.bfloat16), (2, 81900, 300, torch.float32), (2, 27300, 300, torch.float32),
          (1, 204098, 900, torch.bfloat16), (1, 81900, 300, torch.float32)]

if __name__ == "__main__":
    print("library:", _lib.LIB_PATH)
    torch.manual_seed(0)
    for rows, n, k, dtype in SHAPES:
        logits = torch.randn(rows, n, device="cuda") - 4.6
        x = logits.to(torch.bfloat16) if dtype == torch.bfloat16 else torch.sigmoid(logits)
        t = timed(lambda: ops.topk(x, k))
        line = f"[{rows}, {n}] {str(dtype).split('.')[-1]} k={k}: topk {t:6.1f} us"
        if dtype == torch.bfloat16:      # scores within 0.2 of the class prior: two level-1 bins hold the whole row
            x = (torch.randn(rows, n, device="cuda") * 0.05 - 4.0).to(torch.bfloat16)
            line += f"   concentrated scores {timed(lambda: ops.topk(x, k)):6.1f} us"
        print(line, flush=True)
