"""Time the ResNet backbone with and without the fused epilogues (csrc/backbone.hip), and the three kernels alone.

    python tools/time_backbone.py [--sizes 800x1344,1216x2016] [--batches 1,2,4] [--dtypes fp32,bf16] [--layouts nchw,nhwc]
                                  [--modes eval,train] [--windows 5] [--iters 3] [--budget-seconds 900] [--out FILE] [--no-kernels]

Every point is ``resnet50``, ``return_indices=(1, 2, 3)``, ``freeze_indices=(0,)`` (the R50 configuration), ``fused=True`` against
``fused=False`` on the same module and input.  ``eval`` is the forward under ``no_grad``; ``train`` the forward and the backward of
``sum <y_i, g_i>`` in training mode.  A point is timed as device events around windows of ``--iters`` runs behind a warm-up (which
also lets the convolution library choose its algorithms); reported are the median window, per run, and the spread of the windows.
One profiled run per route gives the launch count and the share of device time spent outside the epilogue kernels and torch's
elementwise / pooling kernels, i.e. in the library's convolutions and what they launch around themselves.

The kernels alone run at the layer1 shape of the 800 x 1344 input, [8, 256, 200, 336] (stem: [8, 64, 400, 672]): 550 MB per fp32
tensor, 275 MB per bf16 tensor, so no operand fits the 256 MiB Infinity Cache.  Achieved bytes per second count every operand once
and are set against 8 TB/s.

``--budget-seconds`` stops starting new points once that much time has passed; the points left out are listed, not guessed."""
import argparse
import itertools
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd.backbones import ResNetBackbone, frozen_bn_act, frozen_bn_act_backward, stem_bn_relu_maxpool     # noqa: E402

DEV = "cuda:0"
PEAK = 8.0e12
OURS = ("ew_nchw_kernel", "ew_nhwc_kernel", "stem_pool_kernel")
TORCH_POINTWISE = ("elementwise_kernel", "max_pool", "MaxPool", "reduce_kernel", "CatArrayBatchedCopy", "fill")


def windows_ms(fn, windows, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / iters)
    return statistics.median(times), min(times), max(times)


def profile_once(fn):
    """-> (launches, share of device time outside epilogue / pointwise kernels) of one run."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    launches, total, other = 0, 0.0, 0.0
    for e in prof.events():
        spent = getattr(e, "device_time_total", None)
        spent = getattr(e, "cuda_time_total", 0.0) if spent is None else spent
        if "cuda" in str(getattr(e, "device_type", "")).lower() and spent > 0 and not e.name.startswith(("Memcpy", "Memset")):
            launches += 1
            total += spent
            if not any(k in e.name for k in OURS + TORCH_POINTWISE):
                other += spent
    return launches, (other / total if total else float("nan"))


def network_point(model, size, batch, dtype, layout, mode, args):
    h, w = size
    g = torch.Generator().manual_seed(0)
    x = torch.randn(batch, 3, h, w, generator=g).to(DEV).to(dtype)
    if layout == "nhwc":
        x = x.contiguous(memory_format=torch.channels_last)
    model = model.to(dtype)
    model.train(mode == "train")
    grads = None

    def run():
        nonlocal grads
        if mode == "eval":
            with torch.no_grad():
                return model(x)
        out = model(x)
        if grads is None:
            grads = [torch.randn_like(v) for v in out.values()]
        model.zero_grad(set_to_none=True)
        torch.autograd.backward(list(out.values()), grads)

    row = {}
    for fused in (True, False):
        model.fused = fused
        assert model.takes_fused_route(x) == fused
        med, lo, hi = windows_ms(run, args.windows, args.iters)
        launches, share = profile_once(run)
        row[fused] = (med, lo, hi, launches, share)
    model.fused = True
    return row


def kernel_points(args, emit):
    emit("# kernels alone at the layer1 shape, every operand larger than the Infinity Cache; GB/s = operand bytes / median window")
    for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        for cl in (False, True):
            fmt = torch.channels_last if cl else torch.contiguous_format
            x = torch.randn(8, 256, 200, 336, device=DEV, dtype=dtype).contiguous(memory_format=fmt)
            r, out = torch.randn_like(x), torch.empty_like(x)
            s, h = torch.rand(256, device=DEV) + 0.5, torch.randn(256, device=DEV)
            nbytes = x.numel() * x.element_size()
            cases = [("frozen_bn_act relu", 2, lambda: frozen_bn_act(x, s, h, out=out)),
                     ("frozen_bn_act + residual relu", 3, lambda: frozen_bn_act(x, s, h, residual=r, out=out)),
                     ("frozen_bn_act_backward", 3, lambda: frozen_bn_act_backward(r, x, s, True, False)),
                     ("frozen_bn_act_backward + dres", 4, lambda: frozen_bn_act_backward(r, x, s, True, True))]
            for label, passes, fn in cases:
                with torch.no_grad():
                    med, lo, hi = windows_ms(fn, args.windows, 4)
                emit(f"kernel {label:32s} {name} {'nhwc' if cl else 'nchw'}  {med:8.3f} ms [{lo:.3f} .. {hi:.3f}]  "
                     f"{passes * nbytes / med / 1e6:8.0f} GB/s  {passes * nbytes / med * 1e3 / PEAK:5.2f} of 8 TB/s")
            del x, r, out
            x = torch.randn(8, 64, 400, 672, device=DEV, dtype=dtype).contiguous(memory_format=fmt)
            s, h = torch.rand(64, device=DEV) + 0.5, torch.randn(64, device=DEV)
            nbytes = x.numel() * x.element_size()
            with torch.no_grad():
                med, lo, hi = windows_ms(lambda: stem_bn_relu_maxpool(x, s, h), args.windows, 4)
                ref, rlo, rhi = windows_ms(lambda: torch.nn.functional.max_pool2d(torch.relu_(x * s.view(1, -1, 1, 1).to(dtype)
                                                                                             + h.view(1, -1, 1, 1).to(dtype)), 3, 2, 1),
                                           args.windows, 4)
            emit(f"kernel {'stem_pool':32s} {name} {'nhwc' if cl else 'nchw'}  {med:8.3f} ms [{lo:.3f} .. {hi:.3f}]  "
                 f"{1.25 * nbytes / med / 1e6:8.0f} GB/s  {1.25 * nbytes / med * 1e3 / PEAK:5.2f} of 8 TB/s   torch's operators: {ref:.3f} ms "
                 f"[{rlo:.3f} .. {rhi:.3f}]")
            del x
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="800x1344,1216x2016")
    ap.add_argument("--batches", default="1,2,4")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--layouts", default="nchw,nhwc")
    ap.add_argument("--modes", default="eval,train")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--budget-seconds", type=float, default=900.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    started, sink = time.time(), open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    emit(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; windows {args.windows} x {args.iters} runs, median [min .. max] per run")
    if not args.no_kernels:
        kernel_points(args, emit)
    emit("# resnet50 R50 configuration: ms per run, fused=True | fused=False; launches; share of device time in the library's convolutions")
    model = ResNetBackbone("resnet50", return_indices=(1, 2, 3), freeze_indices=(0,)).to(DEV)
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    dtypes = {"fp32": torch.float32, "bf16": torch.bfloat16}
    skipped, lost = [], []
    for size, mode, dname, layout, batch in itertools.product(sizes, args.modes.split(","), args.dtypes.split(","), args.layouts.split(","),
                                                              [int(b) for b in args.batches.split(",")]):
        label = f"{size[0]}x{size[1]} B={batch} {dname} {layout} {mode}"
        if time.time() - started > args.budget_seconds:
            skipped.append(label)
            continue
        row = network_point(model, size, batch, dtypes[dname], layout, mode, args)
        (fm, flo, fhi, fl, fs), (pm, plo, phi, pl, ps) = row[True], row[False]
        if fm > pm:
            lost.append(label)
        emit(f"{label:36s} fused {fm:8.3f} [{flo:.3f} .. {fhi:.3f}] | torch {pm:8.3f} [{plo:.3f} .. {phi:.3f}]  ratio {pm / fm:5.2f}  "
             f"launches {fl} | {pl}  conv share {fs:4.2f} | {ps:4.2f}")
        torch.cuda.empty_cache()
    emit(f"# points where fused=True was slower: {lost if lost else 'none'}")
    emit(f"# points not measured (time budget of {args.budget_seconds:.0f} s): {skipped if skipped else 'none'}")


if __name__ == "__main__":
    main()
