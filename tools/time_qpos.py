"""rdetr_query_pos_k256_bf16 (csrc/qpos.hip) against the unfused sequence it replaces (4 library GEMMs + scaled_pos), each
replayed as a HIP graph of 20 back-to-back calls: us per call at 600, 1,800 and 3,600 rows.  Then the kernel with the layer's
self-attention in-projection absorbed (rdetr_query_pos_inproj_k256_bf16) against the kernel followed by the two library GEMMs it
absorbs (qk = qpp W[:512]^T, v = query W[512:]^T), alternating, five runs each.  RDETR_LIB_PATH selects the library build."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from relation_detr_amd import _lib, ops  # noqa: E402
from relation_detr_amd.transformer import MLP  # noqa: E402

dev = "cuda:0"
torch.manual_seed(0)
head = MLP(512, 256, 256, 2).to(dev).to(torch.bfloat16)
scale = MLP(256, 256, 256, 2).to(dev).to(torch.bfloat16)


def timed(fn, reps=20, rounds=30):
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


if __name__ == "__main__":
  print("library:", _lib.LIB_PATH)
  for rows in (600, 1800, 3600):
      emb = torch.randn(2, rows // 2, 512, device=dev).to(torch.bfloat16)
      q = torch.randn(2, rows // 2, 256, device=dev).to(torch.bfloat16)
      fused = timed(lambda: ops.query_pos_k256(emb, q, head.layers, scale.layers))
      fused0 = timed(lambda: ops.query_pos_k256(emb, q, head.layers, None))
      unfused = timed(lambda: ops.scaled_pos(head(emb), scale(q), q))
      unfused0 = timed(lambda: head(emb))
      print(f"rows {rows}: fused {fused:.1f} us (layer 0: {fused0:.1f}) | unfused 4 GEMMs + scaled_pos {unfused:.1f} us (layer 0, 2 GEMMs: {unfused0:.1f})")

  w = (torch.randn(768, 256, device=dev) * 0.05).to(torch.bfloat16)
  b = (torch.randn(768, device=dev) * 0.1).to(torch.bfloat16)

  def sequence(emb, q, sc):
      _, qpp = ops.query_pos_k256(emb, q, head.layers, sc)
      return F.linear(qpp, w[:512], b[:512]), F.linear(q, w[512:], b[512:])

  for rows in (600, 1800, 3600):
      emb = torch.randn(2, rows // 2, 512, device=dev).to(torch.bfloat16)
      q = torch.randn(2, rows // 2, 256, device=dev).to(torch.bfloat16)
      for name, sc in (("layers >= 1", scale.layers), ("layer 0", None)):
          runs = []
          for _ in range(5):                                                  # alternating: sequence, absorbed, sequence, ...
              runs.append((timed(lambda: sequence(emb, q, sc)), timed(lambda: ops.query_pos_k256(emb, q, head.layers, sc, in_proj={"weight": w, "bias": b}))))
          print(f"rows {rows} ({name}): kernel + 2 GEMMs " + " ".join(f"{a:.1f}" for a, _ in runs) + " us | in-projection absorbed "
                + " ".join(f"{c:.1f}" for _, c in runs) + f" us | absorbed wins every run: {all(c < a for a, c in runs)}")
