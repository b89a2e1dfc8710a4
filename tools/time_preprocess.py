"""A/B of the image front end: the fused route (csrc/images.hip, one launch per 16 images) against ImagePreprocessor(fused=False), the
restatement of the reference's operator sequence, same process, same device images, alternating.

Shapes: uint8 sources of 480 x 640, 427 x 640, 640 x 480 and 375 x 500 (image b of a batch is entry b % 4) resized by the 800 / 1333
rule, B = 1, 2, 4, batch in fp32 and bf16, NCHW and channels-last; and the 1200 / 2000 rule at B = 2.  Per point and route:
  device    device events around a window of --iters calls, per call: median (min - max) of 5 windows per route, alternating; with one
            short kernel per call this is the rate at which the host issues calls, which is what a caller sees
  busy      the summed durations of one call's kernels and device copies (torch.profiler, median of 5 calls, a pass of its own)
  launches  kernels + device copies of one call (same pass)
and for the fused kernel the achieved bytes per second, byte model below over the busy time, as a share of the 8.0 TB/s HBM peak
(MI355X_MICROARCH.md; a float4 copy reaches 6.29 TB/s of it).

Byte model of one call: every source byte read once (3 h w), every batch element written once (B 3 Hp Wp elements of 4 or 2 bytes),
every mask byte written once (B Hp Wp).  Sources re-read across tiles come from the caches and are not counted.

Run on the GPU:  python tools/time_preprocess.py [--iters 100] [--batches 1,2,4] [--out profiles/r25/preprocess_ab.txt]
(--rehearse: tiny shapes on the CPU, torch route only, no timings)
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd import ImagePreprocessor  # noqa: E402

SOURCES = ((480, 640), (427, 640), (640, 480), (375, 500))
HBM_PEAK = 8.0e12


def make_images(B, device, sources=SOURCES):
    g = torch.Generator().manual_seed(B)
    return [torch.randint(0, 256, (3,) + sources[b % len(sources)], dtype=torch.uint8, generator=g).to(device) for b in range(B)]


def model_bytes(images, batch):
    source = sum(im.numel() * im.element_size() for im in images)
    return source + batch.tensors.numel() * batch.tensors.element_size() + batch.mask.numel()


def launches_of(fn):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception:                                                             # noqa: BLE001 -- the profiler is optional here
        return -1


def busy_of(fn, calls=5):
    """Median over ``calls`` of the summed durations of one call's device events, in ms: what the device is busy for, where the window
    figure is bounded by how fast the host can issue."""
    from torch.profiler import ProfilerActivity, profile
    sums = []
    try:
        for _ in range(calls):
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            sums.append(sum(e.time_range.elapsed_us() for e in prof.events() if str(e.device_type).endswith("CUDA")) * 1e-3)
        return statistics.median(sums)
    except Exception:                                                             # noqa: BLE001 -- the profiler is optional here
        return float("nan")


def measure(fns, iters, windows=5):
    """name -> (device ms per call: median, min, max over the windows; launches; busy ms) for the routes in ``fns``, alternating."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    device = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            device[k].append(a.elapsed_time(b) / iters)
    return {k: (statistics.median(device[k]), min(device[k]), max(device[k]), launches_of(fns[k]), busy_of(fns[k])) for k in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batches", default="1,2,4")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.rehearse:
        images = make_images(2, "cpu", ((48, 64), (43, 64)))
        batch, _ = ImagePreprocessor(80, 133, fused=False).eval()(images)
        print("rehearsal on the CPU, not a measurement:", tuple(batch.tensors.shape), batch.image_sizes.tolist(), model_bytes(images, batch), "bytes")
        return
    if not torch.cuda.is_available():
        sys.exit("time_preprocess.py needs the GPU (--rehearse checks the host logic only)")
    dev = "cuda:0"
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; image front end, uint8 sources {SOURCES}, fused route against the torch "
        f"route; device ms per call over windows of {args.iters} calls (median, min - max of 5); share = model bytes / busy time / 8.0 TB/s")
    points = [(800, 1333, B) for B in (int(b) for b in args.batches.split(","))] + [(1200, 2000, 2)]
    lost = []
    for lo, hi, B in points:
        images = make_images(B, dev)
        for dtype in (torch.float32, torch.bfloat16):
            for cl in (False, True):
                routes = {name: ImagePreprocessor(lo, hi, dtype=dtype, channels_last=cl, fused=fused).eval()
                          for name, fused in (("fused", True), ("torch", False))}
                assert routes["fused"].takes_fused_route(images)
                batch = routes["fused"](images)[0]
                res = measure({name: (lambda m=m: m(images)) for name, m in routes.items()}, args.iters)
                layout = "channels-last" if cl else "NCHW"
                say(f"{lo} / {hi}, B = {B}, batch {tuple(batch.tensors.shape)} {str(dtype).split('.')[-1]} {layout}")
                for route, (d, mn, mx, n, busy) in res.items():
                    say(f"  {route:5s} device {d:8.4f} ms ({mn:.4f} - {mx:.4f})   kernels busy {busy:8.4f} ms   launches {n:4d}")
                nbytes = model_bytes(images, batch)
                rate = nbytes / (res["fused"][4] * 1e-3)
                say(f"  torch / fused: {res['torch'][0] / res['fused'][0]:.2f}x per call, {res['torch'][4] / res['fused'][4]:.2f}x busy   fused kernel: "
                    f"{nbytes / 1e6:.2f} MB in the model, {rate / 1e12:.3f} TB/s, {100 * rate / HBM_PEAK:.1f} % of the HBM peak")
                if res["fused"][0] >= res["torch"][0]:
                    lost.append((lo, hi, B, dtype, layout))
    say(f"points where the fused route is not faster: {lost if lost else 'none'}")


if __name__ == "__main__":
    main()
