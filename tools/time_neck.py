"""A/B of the neck and the position encoding: the fused route (csrc/neck.hip) against the fused=False restatement of the reference,
same process, same inputs, alternating.

Shapes: the R50 feature maps 512 x 100 x 168, 1024 x 50 x 84, 2048 x 25 x 42 of an 800 x 1344 batch (valid 800 x 1333 and smaller),
256 output channels, GroupNorm(32), one extra level, PositionEmbeddingSine(128, 10000, True, offset=-0.5); B = 1, 2, 4.
Modes: eval in fp32 and in bf16 (module and inputs cast), forward + backward in fp32 and under bf16 autocast (the backward of the sum
of the four maps against fixed upstream gradients).  Parts, timed separately: the whole PyramidBuilder, the convolutions alone, the
GroupNorms alone (on the convolutions' outputs), masks + position encoding alone.  Per part and route:
  device    device events around a window of --iters calls, per call: median (min - max) of 5 windows per route, alternating
  wall      host clock from an idle device (synchronised before) to the synchronise after one call, median of --runs
  launches  kernels + device copies of one call (torch.profiler, a pass of its own)

Run on the GPU:  python tools/time_neck.py [--iters 200] [--runs 10] [--batches 1,2,4] [--out profiles/r21/neck_ab.txt]
(--rehearse: tiny shapes on the CPU, torch route only, no timings)
"""
import argparse
import os
import statistics
import sys
import time

import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd import ChannelMapper, PositionEmbeddingSine, PyramidBuilder  # noqa: E402
from relation_detr_amd import neck as nk  # noqa: E402

IN_CHANNELS = (512, 1024, 2048)
SIZES = ((100, 168), (50, 84), (25, 42))
IMAGE = (800, 1344)
VALID = ((800, 1333), (750, 1101), (640, 960), (800, 1200))


def make_inputs(B, device, dtype, sizes=SIZES, channels=IN_CHANNELS, image=IMAGE):
    g = torch.Generator().manual_seed(B)
    feats = [torch.randn(B, c, h, w, generator=g).to(device=device, dtype=dtype) for c, (h, w) in zip(channels, sizes)]
    mask = torch.ones(B, *image)
    for b in range(B):
        h, w = VALID[b % len(VALID)]
        mask[b, :min(h, image[0]), :min(w, image[1])] = 0
    return feats, mask.to(device)


def launches_of(fn):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception:                                                             # noqa: BLE001 -- the profiler is optional here
        return -1


def measure(fns, iters, runs, windows=5):
    """name -> (device ms per call: median, min, max over the windows; wall ms median; launches) for the routes in ``fns``, alternating."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    device = {k: [] for k in fns}
    wall = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            device[k].append(a.elapsed_time(b) / iters)
    for _ in range(runs):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(device[k]), min(device[k]), max(device[k]), statistics.median(wall[k]), launches_of(fns[k])) for k in fns}


def parts(builders, feats, mask, train, autocast):
    """part -> {route: callable}."""
    ctx = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if autocast else (lambda: torch.autocast("cuda", enabled=False))
    fused, plain = builders["fused"], builders["torch"]
    with torch.no_grad(), ctx():
        raw = [blk[0](feats[min(i, 2)]) for i, blk in enumerate(fused.neck.convs)]
        ups = [torch.randn_like(r) for r in raw]
    norms = [blk[1] for blk in fused.neck.convs]
    level_hw = [tuple(r.shape[-2:]) for r in raw]
    pe_f, pe_t = fused.position_embedding, plain.position_embedding

    def whole(builder):
        def run():
            with ctx():
                if not train:
                    with torch.no_grad():
                        return builder(feats, mask)
                builder.zero_grad(set_to_none=True)
                for f in feats:
                    f.grad = None
                outs = builder(feats, mask)[0]
                torch.autograd.backward(outs, [u.to(o.dtype) for u, o in zip(ups, outs)])
        return run

    def convs():
        with ctx():
            if not train:
                with torch.no_grad():
                    return [blk[0](feats[min(i, 2)]) for i, blk in enumerate(fused.neck.convs)]
            fused.zero_grad(set_to_none=True)
            for f in feats:
                f.grad = None
            outs = [blk[0](feats[min(i, 2)]) for i, blk in enumerate(fused.neck.convs)]
            torch.autograd.backward(outs, ups)

    def gn(route):
        def run():
            xs = [r.detach().requires_grad_(train) for r in raw]
            with torch.set_grad_enabled(train), ctx():
                if route == "fused":
                    ys = nk.group_norm_levels(xs, [n.weight for n in norms], [n.bias for n in norms], 32, 1e-5)
                else:
                    ys = [n(x) for x, n in zip(xs, norms)]                           # under autocast: torch casts to fp32 and returns fp32
                if train:
                    torch.autograd.backward(ys, [u.to(y.dtype) for u, y in zip(ups, ys)])
        return run

    def pos_fused():
        with torch.no_grad():
            masks, cum = nk._masks_and_counts(mask, level_hw)
            return masks, pe_f.forward_levels(cum, mask.shape[0], level_hw, raw[0].dtype)

    def pos_torch():
        with torch.no_grad():
            masks = [F.interpolate(mask[None], size=hw)[0].to(torch.bool) for hw in level_hw]
            return masks, [pe_t(m).to(raw[0].dtype) for m in masks]

    out = {"whole": {"fused": whole(fused), "torch": whole(plain)}, "convs": {"both": convs},
           "groupnorm": {"fused": gn("fused"), "torch": gn("torch")}}
    if not train:
        out["masks+pos"] = {"fused": pos_fused, "torch": pos_torch}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--batches", default="1,2,4")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.rehearse:
        feats, mask = make_inputs(2, "cpu", torch.float32, ((12, 20), (6, 10), (3, 5)), (16, 24, 40), (96, 160))
        b = PyramidBuilder(ChannelMapper([16, 24, 40], 256, 4, fused=False), PositionEmbeddingSine(128, 10000, True, offset=-0.5, fused=False))
        f, m, p = b(feats, mask)
        print("rehearsal on the CPU, not a measurement:", [tuple(x.shape) for x in f], [tuple(x.shape) for x in m], [tuple(x.shape) for x in p])
        return
    if not torch.cuda.is_available():
        sys.exit("time_neck.py needs the GPU (--rehearse checks the host logic only)")
    dev = "cuda:0"
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; neck + masks + position encoding at the R50 shapes, fused route against "
        f"the torch route; device ms per call over windows of {args.iters} calls (median, min - max of 5), wall ms from an idle device (median of {args.runs})")
    modes = (("eval fp32", torch.float32, False, False), ("eval bf16", torch.bfloat16, False, False),
             ("fwd+bwd fp32", torch.float32, True, False), ("fwd+bwd bf16 autocast", torch.float32, True, True))
    for B in [int(b) for b in args.batches.split(",")]:
        for mode, dtype, train, autocast in modes:
            feats, mask = make_inputs(B, dev, dtype)
            for f in feats:
                f.requires_grad_(train)                                              # training: the backbone wants the data gradients too
            builders = {}
            for name, fused in (("fused", True), ("torch", False)):
                builders[name] = PyramidBuilder(ChannelMapper(list(IN_CHANNELS), 256, 4, fused=fused),
                                                PositionEmbeddingSine(128, 10000, True, offset=-0.5, fused=fused)).to(device=dev, dtype=dtype)
                builders[name].train(train)
            builders["torch"].load_state_dict(builders["fused"].state_dict())
            say(f"B = {B}, {mode}")
            for part, fns in parts(builders, feats, mask, train, autocast).items():
                res = measure(fns, args.iters, args.runs)
                for route, (d, lo, hi, w, n) in res.items():
                    say(f"  {part:10s} {route:5s} device {d:8.3f} ms ({lo:.3f} - {hi:.3f})   wall {w:8.3f} ms   launches {n:4d}")
                if "fused" in res:
                    say(f"  {part:10s} torch / fused: device {res['torch'][0] / res['fused'][0]:.2f}x   wall {res['torch'][3] / res['fused'][3]:.2f}x")


if __name__ == "__main__":
    main()
