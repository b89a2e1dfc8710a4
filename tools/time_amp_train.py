#!/usr/bin/env python3
"""Time forward + backward of the dense tail of an encoder layer, and of one residual add + LayerNorm, in training under
``torch.autocast(bfloat16)`` over fp32 parameters, ``ln_train_fused`` + ``ffn_train_fused`` off against on (the same inputs and
modules, alternating per rep, in one process):

  chain   q1 = norm1(query + attn); out = norm2(q1 + linear2(relu(linear1(q1))))  -- query the fp32 residual stream, attn a bf16
          sublayer output (what output_proj returns under autocast), d_ffn 2048, at 44,646 / 89,292 / 178,584 rows (B = 1, 2, 4 of
          the R50 encoder); every gradient included (query, attn, the two norms, the two linears)
  norm    norm(x + r), x fp32, r bf16, at 1,800 / 4,000 rows (decoder height)

  off  plain torch under autocast: fp32 add and LayerNorm passes, a cast of every norm output in front of the next GEMM, two
       library GEMMs + ReLU per direction
  on   amp_train.AddLayerNormMixedFunction / FeedForwardMixedFunction: the mixed-precision kernels of csrc/layernorm.hip and csrc/ffn.hip

Two clocks per route, both hipEvents around one forward + backward after warm-up, median [min-max]:
  idle    the device is idle when the rep starts, so the host's launch path is inside the interval (what a launch-bound step sees)
  queued  a long GEMM is enqueued first and the first event after it, so the whole rep is queued before the device reaches it and
          the interval is device time

    python tools/time_amp_train.py [--reps 20] [--warmup 5] [--label TEXT] [--case chain:ROWS|norm:ROWS ...]
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
from relation_detr_amd.transformer import add_norm, feed_forward  # noqa: E402

CASES = ["chain:44646", "chain:89292", "chain:178584", "norm:1800", "norm:4000"]
BF = torch.bfloat16


def nrel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def time_case(kind, rows, reps, warmup, dev):
    torch.manual_seed(0)
    norm1, norm2 = torch.nn.LayerNorm(256).to(dev), torch.nn.LayerNorm(256).to(dev)
    linear1, linear2 = torch.nn.Linear(256, 2048).to(dev), torch.nn.Linear(2048, 256).to(dev)
    query = torch.randn(rows, 256, device=dev).requires_grad_(True)
    attn = torch.randn(rows, 256, device=dev).to(BF).requires_grad_(True)
    go = torch.randn(rows, 256, device=dev)
    modules = (norm1,) if kind == "norm" else (norm1, norm2, linear1, linear2)
    leaves = [query, attn] + [p for m in modules for p in m.parameters()]
    opts = {"off": dataclasses.replace(options.get(), ln_train_fused=False, ffn_train_fused=False),
            "on": dataclasses.replace(options.get(), ln_train_fused=True, ffn_train_fused=True)}

    def step(o):
        with torch.autocast("cuda", dtype=BF):
            q1 = add_norm(norm1, query, attn, opts=o)
            out = q1 if kind == "norm" else add_norm(norm2, q1, feed_forward(linear1, linear2, q1, o), opts=o)
        out.backward(go)

    routes = ["off", "on"]
    times = {(k, c): [] for k in routes for c in ("idle", "queued")}
    grads = {}
    plug = torch.randn(8192, 8192, device=dev).to(BF)
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
                step(opts[key])
                e1.record()
                torch.cuda.synchronize()
                if i >= warmup:
                    times[key, clock].append(e0.elapsed_time(e1) * 1e3)
                if i == warmup + reps - 1:
                    grads[key] = [t.grad.float() for t in leaves]
    med = {k: statistics.median(t) for k, t in times.items()}
    lo = {k: min(t) for k, t in times.items()}
    hi = {k: max(t) for k, t in times.items()}
    for clock in ("idle", "queued"):
        o, n = ("off", clock), ("on", clock)
        verdict = "ranges disjoint, on below off" if hi[n] < lo[o] else ("ranges overlap" if lo[n] <= hi[o] else "on ABOVE off")
        print(f"{kind:5s} rows {rows:6d} {clock:6s}  off {med[o]:8.1f} us [{lo[o]:.1f}-{hi[o]:.1f}]  on {med[n]:8.1f} us "
              f"[{lo[n]:.1f}-{hi[n]:.1f}]  on/off {med[n] / med[o]:5.2f}  ({verdict})", flush=True)
    worst = max(nrel(a, b) for a, b in zip(grads["on"], grads["off"]))
    print(f"{kind:5s} rows {rows:6d} worst |on-off|/|off| over the {len(leaves)} gradients {worst:.1e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--case", nargs="*", default=CASES, help="chain:ROWS or norm:ROWS, e.g. chain:44646")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_amp_train.py needs a GPU")
    dev = torch.device("cuda", 0)
    print(f"bf16 autocast over fp32 parameters, forward + backward, every gradient: ln_train_fused + ffn_train_fused off (torch) vs on "
          f"(amp_train).  {a.label}")
    print(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, median of {a.reps} reps after {a.warmup} warm-up "
          f"[min-max], hipEvents around forward + backward of each route, order alternating per rep; idle = device idle at the start "
          f"(host launch path inside the interval), queued = behind a ~1 ms GEMM (device time)")
    for spec in a.case:
        kind, rows = spec.split(":")
        time_case(kind, int(rows), a.reps, a.warmup, dev)


if __name__ == "__main__":
    main()
