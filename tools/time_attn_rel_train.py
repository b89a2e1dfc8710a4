#!/usr/bin/env python3
"""Time one decoder self-attention core forward + backward in bf16 training INCLUDING the production of the relation bias and
the gradient of pos_proj, old route against new (the same inputs, alternating per rep):

  old  rdetr_relation_bias_ws_f32 -> (out > 0) -> masked_fill_ of the denoising mask (_RelationBiasFunction, as
       DeferredRelationBias.materialize does) -> RelationAttentionFunction (attn_train_fused: csrc/attn.hip + csrc/attn_bwd.hip with a
       dbias output) -> rdetr_relation_bias_backward_f32: three [B*H, N, N]-sized tensors (fp32 bias, u8 ReLU mask, fp32 dbias)
  new  RelationAttentionBoxesFunction (rel_train_fused: csrc/attn_rel.hip with the row log-sum-exp + csrc/attn_rel_bwd.hip): none

Shapes (8 heads of 32, 16 sine features): (B, N) = (2, 1100) with a denoising-style block mask (the main decoder with its
denoising queries), (4, 900) without mask, (2, 300) without.  q / k are column slices of one packed projection as in the decoder;
every gradient (q / k, v, pos_proj weight and bias) is requested.  hipEvents around each rep after warm-up, median [min-max];
peak allocated memory of one step of each route (torch.cuda.max_memory_allocated above the inputs); normwise relative
difference of the two routes' gradients.

    python tools/time_attn_rel_train.py [--reps 15] [--warmup 3] [--label TEXT] [--route old|new]
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
from relation_detr_amd.attn_rel_train import RelationAttentionBoxesFunction  # noqa: E402
from relation_detr_amd.relation import _RelationBiasFunction  # noqa: E402

H, C, F = 8, 256, 16
SCALE = 1.0 / math.sqrt(C // H)


def inputs(B, N, masked, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    qk = torch.randn(B, N, 2 * C, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    v = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    boxes = [torch.cat([torch.rand(B, N, 2, generator=g), torch.rand(B, N, 2, generator=g) * 0.4 + 0.02], -1).to(dev) for _ in range(2)]
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(4 * F, H, 1).to(dev)
    mask = None
    if masked:                                      # denoising-style visibility: the first 200 queries and the rest apart
        i = torch.arange(N, device=dev)
        mask = (i[:, None] < 200) != (i[None, :] < 200)
    go = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(dev)
    return qk, v, boxes[0], boxes[1], conv.weight, conv.bias, mask, go


def old_route(qk, v, src, tgt, w, b, mask, go):
    bias = _RelationBiasFunction.apply(src, tgt, w, b, F, 10000.0, 100.0).flatten(0, 1)
    if mask is not None:
        bias.masked_fill_(mask, float("-inf"))
    ctx = ops.RelationAttentionFunction.apply(qk, None, v, bias, None, H, SCALE)
    ctx.backward(go)


def new_route(qk, v, src, tgt, w, b, mask, go):
    ctx = RelationAttentionBoxesFunction.apply(qk, None, v, src, tgt, w, b, mask, H, SCALE, F, 10000.0, 100.0)
    ctx.backward(go)


def nrel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def time_config(name, B, N, masked, reps, warmup, dev, only=None):
    args = inputs(B, N, masked, dev)
    leaves = [args[0], args[1], args[4], args[5]]
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
            fn(*args)
            e1.record()
            torch.cuda.synchronize()
            if i == 0:
                peak[key] = torch.cuda.max_memory_allocated() - base
            if i >= warmup:
                times[key].append(e0.elapsed_time(e1))
            if only is None and i == warmup + reps - 1:
                grads[key] = [t.grad.float() for t in leaves]
    if only:                                    # one route (a profiler run): its kernels only
        print(f"{name:14s} B={B} N={N} {only} {statistics.median(times[only]):.3f} ms")
        return
    med = {k: statistics.median(t) for k, t in times.items()}
    spread = {k: (min(t), max(t)) for k, t in times.items()}
    diff = "  ".join(f"{n} {nrel(a, b):.1e}" for n, a, b in zip(("qk", "v", "w", "b"), grads["new"], grads["old"]))
    one = 4 * B * H * N * N
    print(f"{name:14s} B={B} N={N:5d}  old {med['old']:7.3f} ms [{spread['old'][0]:.3f}-{spread['old'][1]:.3f}]  "
          f"new {med['new']:7.3f} ms [{spread['new'][0]:.3f}-{spread['new'][1]:.3f}]  old/new {med['old'] / med['new']:5.2f}x  "
          f"peak bytes old {peak['old']} new {peak['new']} saved {peak['old'] - peak['new']} (one fp32 bias = {one})  "
          f"|new-old|/|old| {diff}", flush=True)
    del leaves, grads, args
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--route", choices=("old", "new"), help="run one route only (a profiler run)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_attn_rel_train.py needs a GPU")
    dev = torch.device("cuda", 0)
    print(f"decoder self-attention core forward + backward with the relation bias and pos_proj's gradient, bf16 training: old route "
          f"(materialised bias + RelationAttentionFunction) vs new (RelationAttentionBoxesFunction).  {a.label}")
    print(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, median of {a.reps} reps after {a.warmup} warm-up "
          f"[min-max], hipEvents around forward + backward of each route, routes alternating")
    for name, B, N, masked in (("main+dn, mask", 2, 1100, True), ("no mask", 4, 900, False), ("no mask", 2, 300, False)):
        time_config(name, B, N, masked, a.reps, a.warmup, dev, a.route)


if __name__ == "__main__":
    main()
