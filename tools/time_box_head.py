"""rdetr_box_head_k256_bf16 (csrc/mlp.hip) against the unfused sequence it replaces (3 library GEMMs + box_refine per input), each
replayed as a HIP graph of 20 back-to-back calls: us per call for the two-stage call (1,800 rows, one input, logit reference) and
for a decoder layer's two inputs at 600, 1,800 and 3,600 rows each.  Then the kernel with the class head absorbed
(rdetr_box_head_cls_k256_bf16) against the kernel followed by the library GEMM it absorbs (Linear(256, 91) on input A), alternating,
five runs each.  RDETR_LIB_PATH selects the library build."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd import _lib, ops  # noqa: E402
from relation_detr_amd.transformer import MLP  # noqa: E402
from tools.time_qpos import timed  # noqa: E402

dev = "cuda:0"


def unfused(head, x, ref, logit=False):
    delta = head(x)
    return (delta.float() + ref).sigmoid() if logit else ops.box_refine(delta, ref)


if __name__ == "__main__":
    print("library:", _lib.LIB_PATH)
    torch.manual_seed(0)
    head = MLP(256, 256, 4, 3).to(dev).to(torch.bfloat16)
    rows = 1800
    xa = torch.randn(2, rows // 2, 256, device=dev).to(torch.bfloat16)
    logit = torch.randn(2, rows // 2, 4, device=dev)
    fused = timed(lambda: ops.box_head_k256(xa, None, head.layers, logit, reference_is_logit=True))
    plain = timed(lambda: unfused(head, xa, logit, True))
    print(f"rows 1 x {rows} (two-stage call, logit reference): fused {fused:.1f} us | unfused 3 GEMMs + refine {plain:.1f} us")
    for rows in (600, 1800, 3600):
        xa = torch.randn(2, rows // 2, 256, device=dev).to(torch.bfloat16)
        xb = torch.randn(2, rows // 2, 256, device=dev).to(torch.bfloat16)
        ref = torch.rand(2, rows // 2, 4, device=dev)
        fused = timed(lambda: ops.box_head_k256(xa, xb, head.layers, ref))
        plain = timed(lambda: (unfused(head, xa, ref), unfused(head, xb, ref)))
        print(f"rows 2 x {rows} (decoder layer): fused {fused:.1f} us | unfused 6 GEMMs + 2 refines {plain:.1f} us")
    cls = torch.nn.Linear(256, 91).to(dev).to(torch.bfloat16)
    for rows in (600, 1800, 3600):
        xa = torch.randn(2, rows // 2, 256, device=dev).to(torch.bfloat16)
        xb = torch.randn(2, rows // 2, 256, device=dev).to(torch.bfloat16)
        ref = torch.rand(2, rows // 2, 4, device=dev)
        for name, second in (("two inputs", xb), ("last layer, one input", None)):
            runs = []
            for _ in range(5):                                                # alternating: sequence, absorbed, sequence, ...
                runs.append((timed(lambda: (ops.box_head_k256(xa, second, head.layers, ref), cls(xa))),
                             timed(lambda: ops.box_head_k256(xa, second, head.layers, ref, class_head={"linear": cls}))))
            print(f"rows {rows} ({name}): kernel + class GEMM " + " ".join(f"{a:.1f}" for a, _ in runs) + " us | class head absorbed "
                  + " ".join(f"{c:.1f}" for _, c in runs) + f" us | absorbed wins every run: {all(c < a for a, c in runs)}")
