#!/usr/bin/env python3
"""Time one MSDA core forward + backward in training mode, old route against new (the same inputs, alternating per rep):

  old  torch producer (softmax over the logits, sampling_locations() as torch elementwise ops) -> fp32 locations / weights ->
       MultiScaleDeformableAttnFunction (fp32 value copy + rdetr_msda_backward_*_f32 in its backward) -> autograd back through
       the producer                                               (MultiScaleDeformableAttention.forward without msda_train_fused)
  new  MultiScaleDeformableAttnFusedFunction: fused-producer gather forward + rdetr_msda_backward_fused_* (msda_train_fused)

Shapes: the R50 encoder shape (bench.R50_SHAPES, S = Nq = 22,323, 2-d reference points) at B = 1 and 2, the decoder shape
(Nq = 900, 4-d reference points) at B = 2; fp32 and bf16; atomic and deterministic grad_value.  hipEvents around each rep after
warm-up, median over the reps.  Every gradient the step produces (value, offsets, logits, reference points) is requested.

    python tools/time_msda_train.py [--reps 15] [--warmup 3] [--label TEXT] [--quick] [--route old|new]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from relation_detr_amd import ops  # noqa: E402
from relation_detr_amd.ms_deform_attn import sampling_locations  # noqa: E402


def inputs(B, Nq, ref_dim, dtype, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    shp = torch.tensor(bench.R50_SHAPES, dtype=torch.int64)
    areas = shp[:, 0] * shp[:, 1]
    start = torch.cat([areas.new_zeros(1), areas.cumsum(0)[:-1]])
    S, L = int(areas.sum()), shp.shape[0]
    if Nq is None:
        Nq = S
    value = torch.randn(B, S, 8, 32, generator=g)
    offsets = torch.randn(B, Nq, 8, L, 4, 2, generator=g) * (1.0 if ref_dim == 2 else 2.0)
    logits = torch.randn(B, Nq, 8, L * 4, generator=g)
    if ref_dim == 2:
        ref = torch.rand(B, Nq, L, 2, generator=g)
    else:
        ref = torch.cat([torch.rand(B, Nq, L, 2, generator=g), torch.rand(B, Nq, L, 2, generator=g) * 0.4 + 0.05], -1)
    go = torch.randn(B, Nq, 256, generator=g)
    value, offsets, logits, go = (t.to(dtype).to(dev) for t in (value, offsets, logits, go))
    leaves = [t.requires_grad_(True) for t in (value, offsets, logits, ref.to(dev))]
    return leaves, shp.to(dev), start.to(dev), go


def old_route(v, shp, start, o, lg, r, go):
    B, Nq, H, L, P, _ = o.shape
    w = lg.softmax(-1).view(B, Nq, H, L, P)
    loc = sampling_locations(r, o, shp, P)
    out = ops.MultiScaleDeformableAttnFunction.apply(v.contiguous(), shp, start, loc.float().contiguous(), w.float().contiguous(), 64)
    out.backward(go)


def new_route(v, shp, start, o, lg, r, go):
    out = ops.MultiScaleDeformableAttnFusedFunction.apply(v, shp, start, o, lg, r)
    out.backward(go)


def time_config(name, B, Nq, ref_dim, dtype, det, reps, warmup, dev, only=None):
    leaves, shp, start, go = inputs(B, Nq, ref_dim, dtype, dev)
    ops.host_levels(shp, start)
    routes = {k: f for k, f in (("old", old_route), ("new", new_route)) if only in (None, k)}
    grads = {}
    times = {k: [] for k in routes}
    torch.use_deterministic_algorithms(det, warn_only=True)
    try:
        for i in range(warmup + reps):
            for key, fn in routes.items():
                for t in leaves:
                    t.grad = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(leaves[0], shp, start, leaves[1], leaves[2], leaves[3], go)
                e1.record()
                torch.cuda.synchronize()
                if i >= warmup:
                    times[key].append(e0.elapsed_time(e1))
                if only is None:
                    grads[key] = [t.grad.float() for t in leaves]
    finally:
        torch.use_deterministic_algorithms(False)
    if only:                                    # one route (a profiler run): its kernels only
        print(f"{name:8s} B={B} {str(dtype).split('.')[-1]:8s} {'det' if det else 'atomic'} {only} {statistics.median(times[only]):.3f} ms")
        return
    # the two routes' gradients (same inputs): largest difference relative to the largest magnitude, per tensor
    rel = [float((a - b).abs().max()) / max(1e-30, float(b.abs().max())) for a, b in zip(grads["new"], grads["old"])]
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (min(v), max(v)) for k, v in times.items()}
    line = (f"{name:8s} B={B} Nq={Nq if Nq else 'S':>5} ref={ref_dim} {str(dtype).split('.')[-1]:8s} "
            f"{'det   ' if det else 'atomic'}  old {med['old']:8.3f} ms [{spread['old'][0]:.3f}-{spread['old'][1]:.3f}]  "
            f"new {med['new']:8.3f} ms [{spread['new'][0]:.3f}-{spread['new'][1]:.3f}]  new/old {med['new'] / med['old']:.3f}  "
            f"max|new-old|/max|old| value {rel[0]:.1e} offsets {rel[1]:.1e} logits {rel[2]:.1e} ref {rel[3]:.1e}")
    print(line, flush=True)
    del leaves, grads
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--quick", action="store_true", help="encoder B=1 and decoder only, for a profiler run")
    ap.add_argument("--route", choices=("old", "new"), help="run one route only (a profiler run)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_msda_train.py needs a GPU")
    dev = torch.device("cuda", 0)
    print(f"MSDA core forward + backward, training mode: old route (torch producer + MultiScaleDeformableAttnFunction) vs new "
          f"(MultiScaleDeformableAttnFusedFunction).  {a.label}")
    print(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, median of {a.reps} reps after {a.warmup} warm-up "
          f"[min-max], hipEvents around forward + backward of each route, routes alternating")
    configs = [("encoder", 1, None, 2), ("encoder", 2, None, 2), ("decoder", 2, 900, 4)]
    if a.quick:
        configs = [configs[0], configs[2]]
    for dtype in (torch.float32, torch.bfloat16):
        for det in (False, True):
            for name, B, Nq, ref_dim in configs:
                time_config(name, B, Nq, ref_dim, dtype, det, a.reps, a.warmup, dev, a.route)


if __name__ == "__main__":
    main()
