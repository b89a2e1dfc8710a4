#!/usr/bin/env python3
"""Time forward + backward of one residual add + LayerNorm, norm(x + r), in training, every gradient included (x, r, gamma, beta),
old route against new (the same inputs and module, alternating per rep, in one process):

  old  transformer.add_norm with ln_train_fused off: an add pass (the sum rounded to the storage type), the library LayerNorm, its
       backward and the parameter-gradient pass under autograd
  new  ln_train_fused on (ln_train.AddLayerNormFunction): rdetr_add_layernorm_train_* forward, rdetr_add_layernorm_backward_* (one row
       kernel + the fixed-order sum of its partials) backward

Two clocks per route, both hipEvents around one forward + backward after warm-up, median [min-max]:
  idle    the device is idle when the rep starts, so the host's launch path is inside the interval (what a launch-bound step sees)
  queued  a long GEMM is enqueued first and the first event after it, so the whole rep is queued before the device reaches it and
          the interval is device time (what a step sees whose host runs ahead of the device, as at encoder height)

Shapes: bf16 at 44,646 / 89,292 / 178,584 rows (B = 1, 2, 4 of the R50 encoder) and at 1,800 / 4,000 rows (decoder), fp32 at 44,646.
Bytes/s of the new route (queued clock) against its 7 traversals of [rows, 256] (forward: x, r in, y out; backward: dy, x, r in,
dx out); normwise relative difference of the two routes' gradients.

    python tools/time_ln_train.py [--reps 30] [--warmup 5] [--label TEXT] [--route old|new] [--case DTYPE:ROWS ...]
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
from relation_detr_amd.transformer import add_norm  # noqa: E402

CASES = ["bf16:44646", "bf16:89292", "bf16:178584", "bf16:1800", "bf16:4000", "fp32:44646"]
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def nrel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def time_case(name, rows, reps, warmup, dev, only=None):
    dtype = DTYPES[name]
    torch.manual_seed(0)
    norm = torch.nn.LayerNorm(256).to(dev).to(dtype)
    with torch.no_grad():
        norm.weight.add_(0.1 * torch.randn(256, device=dev).to(dtype))
        norm.bias.add_(0.1 * torch.randn(256, device=dev).to(dtype))
    x = torch.randn(rows, 256, device=dev).to(dtype).requires_grad_(True)
    r = torch.randn(rows, 256, device=dev).to(dtype).requires_grad_(True)
    go = torch.randn(rows, 256, device=dev).to(dtype)
    leaves = [x, r, norm.weight, norm.bias]
    opts = {"old": dataclasses.replace(options.get(), ln_train_fused=False), "new": dataclasses.replace(options.get(), ln_train_fused=True)}
    routes = [k for k in ("old", "new") if only in (None, k)]
    times = {(k, c): [] for k in routes for c in ("idle", "queued")}
    grads = {}
    plug = torch.randn(8192, 8192, device=dev).to(torch.bfloat16)
    for i in range(warmup + reps):
        for clock in ("idle", "queued"):
            for key in (routes if i % 2 == 0 else routes[::-1]):
                for t in leaves:
                    t.grad = None
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if clock == "queued":
                    plug @ plug                      # ~1 ms of device work: the rep below is fully queued when it ends
                e0.record()
                add_norm(norm, x, r, opts=opts[key]).backward(go)
                e1.record()
                torch.cuda.synchronize()
                if i >= warmup:
                    times[key, clock].append(e0.elapsed_time(e1) * 1e3)
                if only is None and i == warmup + reps - 1:
                    grads[key] = [t.grad.float() for t in leaves]
    med = {k: statistics.median(t) for k, t in times.items()}
    lo = {k: min(t) for k, t in times.items()}
    hi = {k: max(t) for k, t in times.items()}
    if only:                                    # one route (a profiler run): its kernels only
        print(f"{name} rows {rows:6d} {only} idle {med[only, 'idle']:.1f} us queued {med[only, 'queued']:.1f} us")
        return
    traffic = 7 * rows * 256 * x.element_size()
    diff = "  ".join(f"{n} {nrel(a, b):.1e}" for n, a, b in zip(("dx", "dr", "dgamma", "dbeta"), grads["new"], grads["old"]))
    for clock in ("idle", "queued"):
        o, n = ("old", clock), ("new", clock)
        verdict = "ranges disjoint, new below old" if hi[n] < lo[o] else ("ranges overlap" if lo[n] <= hi[o] else "new ABOVE old")
        tail = f"  new: {traffic / 1e6:.1f} MB in 7 traversals = {traffic / med[n] / 1e6:.2f} TB/s" if clock == "queued" else ""
        print(f"{name} rows {rows:6d} {clock:6s}  old {med[o]:7.1f} us [{lo[o]:.1f}-{hi[o]:.1f}]  new {med[n]:7.1f} us "
              f"[{lo[n]:.1f}-{hi[n]:.1f}]  new/old {med[n] / med[o]:5.2f}  ({verdict}){tail}", flush=True)
    print(f"{name} rows {rows:6d} |new-old|/|old| {diff}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--route", choices=("old", "new"), help="run one route only (a profiler run)")
    ap.add_argument("--case", nargs="*", default=CASES, help="DTYPE:ROWS, e.g. bf16:44646")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ln_train.py needs a GPU")
    dev = torch.device("cuda", 0)
    print(f"add + LayerNorm forward + backward in training, all four gradients: old route (add pass + library LayerNorm under autograd) vs "
          f"new (AddLayerNormFunction).  {a.label}")
    print(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, median of {a.reps} reps after {a.warmup} warm-up "
          f"[min-max], hipEvents around forward + backward of each route, order alternating per rep; idle = device idle at the start "
          f"(host launch path inside the interval), queued = behind a ~1 ms GEMM (device time)")
    for spec in a.case:
        name, rows = spec.split(":")
        time_case(name, int(rows), a.reps, a.warmup, dev, a.route)


if __name__ == "__main__":
    main()
