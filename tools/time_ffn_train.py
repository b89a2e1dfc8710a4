#!/usr/bin/env python3
"""Time forward + backward of one encoder feed-forward block linear2(relu(linear1(x))) in bf16 training, every gradient included
(x, both weights, both biases), old route against new (the same inputs and modules, alternating per rep):

  old  transformer.feed_forward with ffn_train_fused off: two library GEMMs and a ReLU pass forward; dY W2 GEMM, ReLU backward pass
       over [rows, d_ffn], dx GEMM, two weight-gradient GEMMs and two column sums backward
  new  ffn_train_fused on (ffn_train.FeedForwardFunction): the two weight packs + rdetr_ffn_k256_train_bf16 forward; two weight
       transposes + pack + rdetr_ffn_k256_backward_bf16, the same two weight-gradient GEMMs and column sums backward

Shapes: 20,274 / 44,646 / 89,292 rows, d_ffn 2048.  hipEvents around each rep after warm-up, median [min-max]; peak allocated
memory of one step of each route above the inputs; normwise relative difference of the two routes' gradients.

    python tools/time_ffn_train.py [--reps 15] [--warmup 3] [--label TEXT] [--route old|new] [--rows N ...]
"""
import argparse
import dataclasses
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from relation_detr_amd import options  # noqa: E402
from relation_detr_amd.transformer import feed_forward  # noqa: E402

D_FFN = 2048


def nrel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def time_rows(rows, reps, warmup, dev, only=None):
    torch.manual_seed(0)
    lin1 = torch.nn.Linear(256, D_FFN).to(dev).to(torch.bfloat16)
    lin2 = torch.nn.Linear(D_FFN, 256).to(dev).to(torch.bfloat16)
    x = torch.randn(rows, 256, device=dev).to(torch.bfloat16).requires_grad_(True)
    go = torch.randn(rows, 256, device=dev).to(torch.bfloat16)
    leaves = [x, lin1.weight, lin1.bias, lin2.weight, lin2.bias]
    opts = {"old": dataclasses.replace(options.get(), ffn_train_fused=False), "new": dataclasses.replace(options.get(), ffn_train_fused=True)}
    routes = [k for k in ("old", "new") if only in (None, k)]
    times = {k: [] for k in routes}
    peak, grads = {}, {}
    for i in range(warmup + reps):
        for key in routes:
            for t in leaves:
                t.grad = None
            torch.cuda.synchronize()
            if i == 0:
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            feed_forward(lin1, lin2, x, opts[key]).backward(go)
            e1.record()
            torch.cuda.synchronize()
            if i == 0:
                peak[key] = torch.cuda.max_memory_allocated() - base
            if i >= warmup:
                times[key].append(e0.elapsed_time(e1))
            if only is None and i == warmup + reps - 1:
                grads[key] = [t.grad.float() for t in leaves]
    if only:                                    # one route (a profiler run): its kernels only
        print(f"rows {rows:6d} {only} {statistics.median(times[only]):.3f} ms")
        return
    med = {k: statistics.median(t) for k, t in times.items()}
    lo = {k: min(t) for k, t in times.items()}
    hi = {k: max(t) for k, t in times.items()}
    diff = "  ".join(f"{n} {nrel(a, b):.1e}" for n, a, b in zip(("dx", "dW1", "db1", "dW2", "db2"), grads["new"], grads["old"]))
    verdict = "ranges disjoint, new below old" if hi["new"] < lo["old"] else ("ranges overlap" if lo["new"] <= hi["old"] else "new ABOVE old")
    print(f"rows {rows:6d} d_ffn {D_FFN}  old {med['old']:7.3f} ms [{lo['old']:.3f}-{hi['old']:.3f}]  "
          f"new {med['new']:7.3f} ms [{lo['new']:.3f}-{hi['new']:.3f}]  old/new {med['old'] / med['new']:5.2f}x  ({verdict})  "
          f"peak MiB old {peak['old'] / 2 ** 20:.1f} new {peak['new'] / 2 ** 20:.1f}  |new-old|/|old| {diff}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--route", choices=("old", "new"), help="run one route only (a profiler run)")
    ap.add_argument("--rows", type=int, nargs="*", default=[20274, 44646, 89292])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ffn_train.py needs a GPU")
    dev = torch.device("cuda", 0)
    print(f"encoder feed-forward block forward + backward, bf16 training, all five gradients: old route (library GEMMs + ReLU passes "
          f"under autograd) vs new (FeedForwardFunction).  {a.label}")
    print(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, median of {a.reps} reps after {a.warmup} warm-up "
          f"[min-max], hipEvents around forward + backward of each route, routes alternating")
    for rows in a.rows:
        time_rows(rows, a.reps, a.warmup, dev, a.route)


if __name__ == "__main__":
    main()
