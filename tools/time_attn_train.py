#!/usr/bin/env python3
"""Time the decoder self-attention core forward + backward in bf16 training, old route against new (the same inputs,
alternating per rep):

  old  QK^T GEMM -> fp32 copy -> rdetr_bias_softmax_f32 (_BiasSoftmaxFunction) -> bf16 copy -> PV GEMM, and their autograd
       backward: torch elementwise / reduction passes over fp32 [B*H, N, M] and two GEMMs   (RelationSelfAttention.forward with
       attn_train_fused off, from the q / k / v projections to the context)
  new  RelationAttentionFunction: the flash-style forward with the row log-sum-exp + csrc/attn_bwd.hip   (attn_train_fused on)

Shapes (8 heads of 32): (B, N) = (2, 1100) with a float bias holding -inf in a denoising-style block mask (the main decoder with
its denoising queries), (2, 1500) without bias (hybrid branch), (4, 900) with a bias, (2, 300) with a bias.  q / k are column
slices of one packed projection as in the decoder; every gradient (q / k, v, bias) is requested.  hipEvents around each rep
after warm-up, median [min-max]; peak allocated memory of one step of each route (torch.cuda.max_memory_allocated above the
inputs); normwise relative difference of the two routes' gradients.

    python tools/time_attn_train.py [--reps 15] [--warmup 3] [--label TEXT] [--route old|new]
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from relation_detr_amd import ops  # noqa: E402
from relation_detr_amd.self_attn import _BiasSoftmaxFunction  # noqa: E402

H, C = 8, 256


def inputs(B, N, with_bias, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    qk = torch.randn(B, N, 2 * C, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    v = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    bias = None
    if with_bias:
        bias = (torch.rand(B * H, N, N, generator=g) * 3.0).to(dev)
        if with_bias == "dn":                       # denoising-style visibility: the first 200 queries and the rest apart
            i = torch.arange(N, device=dev)
            bias.masked_fill_((i[:, None] < 200) != (i[None, :] < 200), float("-inf"))
        bias.requires_grad_(True)
    go = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(dev)
    return qk, v, bias, go


def old_route(qk, v, bias, go):
    B, N, _ = qk.shape
    d = C // H
    q, k = qk[..., :C], qk[..., C:]
    qh = (q * (1.0 / math.sqrt(d))).view(B, N, H, d).transpose(1, 2).contiguous()
    kh = k.view(B, N, H, d).transpose(1, 2).contiguous()
    vh = v.view(B, N, H, d).transpose(1, 2).contiguous()
    scores = torch.matmul(qh, kh.transpose(-1, -2)).float().reshape(B * H, N, N).contiguous()
    probs = _BiasSoftmaxFunction.apply(scores, bias, None)
    ctx = torch.matmul(probs.view(B, H, N, N).to(vh.dtype), vh).transpose(1, 2).reshape(B, N, C)
    ctx.backward(go)


def new_route(qk, v, bias, go):
    ctx = ops.RelationAttentionFunction.apply(qk, None, v, bias, None, H, 1.0 / math.sqrt(C // H))
    ctx.backward(go)


def nrel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def time_config(name, B, N, with_bias, reps, warmup, dev, only=None):
    qk, v, bias, go = inputs(B, N, with_bias, dev)
    leaves = [t for t in (qk, v, bias) if t is not None]
    routes = {k: f for k, f in (("old", old_route), ("new", new_route)) if only in (None, k)}
    times = {k: [] for k in routes}
    peak = {}
    grads = {}
    for i in range(warmup + reps):
        for key, fn in routes.items():
            for t in leaves:
                t.grad = None
            torch.cuda.synchronize()
            if i == 0:
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(qk, v, bias, go)
            e1.record()
            torch.cuda.synchronize()
            if i == 0:
                peak[key] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            if i >= warmup:
                times[key].append(e0.elapsed_time(e1))
            if only is None and i == warmup + reps - 1:
                grads[key] = [t.grad.float() for t in leaves]
    if only:                                    # one route (a profiler run): its kernels only
        print(f"{name:22s} B={B} N={N} {only} {statistics.median(times[only]):.3f} ms")
        return
    med = {k: statistics.median(t) for k, t in times.items()}
    spread = {k: (min(t), max(t)) for k, t in times.items()}
    names = ["qk", "v", "bias"][:len(leaves)]
    diff = "  ".join(f"{n} {nrel(a, b):.1e}" for n, a, b in zip(names, grads["new"], grads["old"]))
    print(f"{name:22s} B={B} N={N:5d}  old {med['old']:7.3f} ms [{spread['old'][0]:.3f}-{spread['old'][1]:.3f}]  "
          f"new {med['new']:7.3f} ms [{spread['new'][0]:.3f}-{spread['new'][1]:.3f}]  old/new {med['old'] / med['new']:5.2f}x  "
          f"peak MiB old {peak['old']:7.1f} new {peak['new']:7.1f}  |new-old|/|old| {diff}", flush=True)
    del leaves, grads, qk, v, bias, go
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--route", choices=("old", "new"), help="run one route only (a profiler run)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_attn_train.py needs a GPU")
    dev = torch.device("cuda", 0)
    print(f"decoder self-attention core forward + backward, bf16 training: old route (GEMM + bias-softmax chain) vs new "
          f"(RelationAttentionFunction).  {a.label}")
    print(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, median of {a.reps} reps after {a.warmup} warm-up "
          f"[min-max], hipEvents around forward + backward of each route, routes alternating")
    for name, B, N, with_bias in (("main+dn, bias, -inf", 2, 1100, "dn"), ("hybrid, no bias", 2, 1500, None),
                                  ("bias", 4, 900, "plain"), ("bias", 2, 300, "plain")):
        time_config(name, B, N, with_bias, a.reps, a.warmup, dev, a.route)


if __name__ == "__main__":
    main()
