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

``--hm``: the head-major training route instead (msda_train_head_major, relation_detr_amd/msda_train_hm.py) against the parent's best
(msda_train_fused), bf16, the R50 encoder shape at B = 1, 2 and 4 with a padding mask on the tail of the last image, atomic and
deterministic grad_value:

  core    masked_fill + MultiScaleDeformableAttnFusedFunction on the [B,S,8,32] value (what the module runs; "nofill": the Function
          alone) against MultiScaleDeformableAttnHeadMajorFunction on the projected value + mask; gradients for value, offsets,
          logits and reference points
  module  MultiScaleDeformableAttention.forward + backward (query = value shape; every input and parameter gradient), the same
          weights in both modules

The routes of a rep run in alternating order (forward order on even reps, reversed on odd ones).

    python tools/time_msda_train.py --hm [--reps 15] [--warmup 3] [--batches 1 2 4] [--label TEXT]
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


def _timed_routes(routes, reset, reps, warmup):
    """{name: callable} -> {name: [ms per rep]}; every rep runs all routes, in forward order on even reps and reversed on odd ones."""
    times = {k: [] for k in routes}
    names = list(routes)
    for i in range(warmup + reps):
        for key in (names if i % 2 == 0 else names[::-1]):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            routes[key]()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[key].append(e0.elapsed_time(e1))
    return times


def _fmt(times, key):
    v = times[key]
    return f"{key} {statistics.median(v):8.3f} ms [{min(v):.3f}-{max(v):.3f}]"


def time_head_major(B, det, reps, warmup, dev):
    from relation_detr_amd import MultiScaleDeformableAttention, msda_train_hm, options
    leaves, shp, start, go = inputs(B, None, 2, torch.bfloat16, dev)
    ops.host_levels(shp, start)
    S = leaves[0].shape[1]
    v = leaves[0].detach().view(B, S, 256).clone().requires_grad_(True)        # the projected value, before the padding fill
    off, lg, ref = leaves[1:]
    mask = torch.zeros(B, S, dtype=torch.bool, device=dev)
    mask[B - 1, -S // 10:] = True
    tensors = [v, off, lg, ref]

    def reset():
        for t in tensors:
            t.grad = None

    def fused(fill=True):
        vv = v.masked_fill(mask[..., None], 0.0) if fill else v
        ops.MultiScaleDeformableAttnFusedFunction.apply(vv.view(B, S, 8, 32), shp, start, off, lg, ref).backward(go)

    def head_major():
        msda_train_hm.MultiScaleDeformableAttnHeadMajorFunction.apply(v, mask, shp, start, off, lg, ref).backward(go)

    tag = f"B={B} {'det   ' if det else 'atomic'}"
    torch.use_deterministic_algorithms(det, warn_only=True)
    try:
        t = _timed_routes({"fused": fused, "nofill": lambda: fused(False), "hm": head_major}, reset, reps, warmup)
        ratio = statistics.median(t["hm"]) / statistics.median(t["fused"])
        print(f"core   {tag}  {_fmt(t, 'fused')}  {_fmt(t, 'nofill')}  {_fmt(t, 'hm')}  hm/fused {ratio:.3f}", flush=True)
        # the module: same weights, the two switches
        mods = {}
        torch.manual_seed(0)
        for key, on in (("fused", False), ("hm", True)):
            with options.override(msda_train_fused=True, msda_train_head_major=on):
                m = MultiScaleDeformableAttention(256, 4, 8, 4)
            if mods:
                m.load_state_dict(mods["fused"].state_dict())
            else:
                with torch.no_grad():
                    for p in m.parameters():
                        p.add_(torch.randn_like(p) * 0.02)
            mods[key] = m.to(dev).to(torch.bfloat16).train()
        g = torch.Generator().manual_seed(1)
        q, x = (torch.randn(B, S, 256, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True) for _ in range(2))
        r = ref.detach().clone().requires_grad_(True)
        tensors = [q, x, r] + [p for m in mods.values() for p in m.parameters()]
        run = lambda m: m(q, r, x, shp, start, mask).backward(go)
        t = _timed_routes({k: (lambda m=m: run(m)) for k, m in mods.items()}, reset, reps, warmup)
        ratio = statistics.median(t["hm"]) / statistics.median(t["fused"])
        print(f"module {tag}  {_fmt(t, 'fused')}  {_fmt(t, 'hm')}  hm/fused {ratio:.3f}", flush=True)
    finally:
        torch.use_deterministic_algorithms(False)
    del leaves, tensors, mods
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--quick", action="store_true", help="encoder B=1 and decoder only, for a profiler run")
    ap.add_argument("--route", choices=("old", "new"), help="run one route only (a profiler run)")
    ap.add_argument("--hm", action="store_true", help="time the head-major training route against msda_train_fused")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4], help="batch sizes of --hm")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_msda_train.py needs a GPU")
    dev = torch.device("cuda", 0)
    if a.hm:
        print(f"MSDA training, bf16, R50 encoder shape (S = Nq = 22,323, 2-d reference points): msda_train_fused (fused) vs "
              f"msda_train_head_major (hm).  {a.label}")
        print(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, median of {a.reps} reps after {a.warmup} warm-up "
              f"[min-max], hipEvents around forward + backward of each route, route order alternating per rep")
        for det in (False, True):
            for B in a.batches:
                time_head_major(B, det, a.reps, a.warmup, dev)
        return
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
