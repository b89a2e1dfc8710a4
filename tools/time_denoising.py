"""A/B of the denoising query generator: GenerateCDNQueries(fused=True) against its torch route (fused=False, the reference's
operation sequence), forward + backward, same process, same targets, alternating.

Shapes of the R50 configuration: C = 91, d = 256, 900 matching queries, denoising_nums = 100; B = 2 and 4 images with 7 and 20
boxes each.  The backward is the gradient of label_encoder.weight under a fixed upstream gradient of the label queries.  Per route
and shape:
  wall      host clock from an idle device (synchronised before) to the synchronise after backward, median and spread of the runs
  device    sum of the kernel and copy durations of one step (torch.profiler, a pass of its own)
  launches  kernels + device copies of that step;  syncs: runtime calls that wait for the device (synchronise calls and blocking copies)

Run on the GPU:  python tools/time_denoising.py [--runs 20] [--out profiles/r17/denoising_ab.txt]
(--rehearse: tiny shapes on the CPU, torch route only, no timings)
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd import GenerateCDNQueries  # noqa: E402


def make_targets(B, C, boxes_per_image, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    labels = [torch.randint(0, C, (boxes_per_image,), generator=g).to(device) for _ in range(B)]
    boxes = [torch.cat((torch.rand(boxes_per_image, 2, generator=g), 0.02 + 0.4 * torch.rand(boxes_per_image, 2, generator=g)), -1).to(device)
             for _ in range(B)]
    return labels, boxes


def step(module, labels, boxes, upstream):
    module.label_encoder.weight.grad = None
    label_query, box_query, mask, groups, group_size = module(labels, boxes)
    label_query.backward(upstream[:, :label_query.shape[1]])
    return label_query, box_query, mask, groups, group_size


def profile_step(module, labels, boxes, upstream):
    """(device microseconds, launches, syncs, the waiting calls by name) of one step, or None where the profiler gives no device events."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step(module, labels, boxes, upstream)
        torch.cuda.synchronize()
    device_us, launches, waits = 0.0, 0, {}
    for e in prof.events():
        if str(e.device_type).endswith("CUDA"):
            device_us += e.device_time if hasattr(e, "device_time") else e.cuda_time
            launches += 1
        elif "Synchronize" in e.name or e.name in ("hipMemcpyWithStream", "hipMemcpy"):
            waits[e.name] = waits.get(e.name, 0) + 1
    if "hipDeviceSynchronize" in waits:                                               # the synchronise that closes the window
        waits["hipDeviceSynchronize"] -= 1
    waits = {k: v for k, v in waits.items() if v}
    return (device_us, launches, sum(waits.values()), waits) if launches else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.rehearse:
        labels, boxes = make_targets(2, 7, 3, "cpu")
        module = GenerateCDNQueries(num_queries=12, num_classes=7, label_embed_dim=16, denoising_nums=6, fused=False)
        out = step(module, labels, boxes, torch.ones(2, 12, 16))
        print("rehearsal on the CPU, not a measurement: label queries", tuple(out[0].shape), "groups", out[3], "group size", out[4],
              "gradient norm", float(module.label_encoder.weight.grad.norm()))
        return
    if not torch.cuda.is_available():
        sys.exit("time_denoising.py needs the GPU (--rehearse checks the host logic only)")
    dev = "cuda:0"
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; forward + backward of the denoising generator, {args.runs} alternating "
        "runs per route")
    say("# C = 91, d = 256, 900 matching queries, denoising_nums = 100; wall in ms (median, min - max); device = kernel + copy time of one step")
    for B in (2, 4):
        for G in (7, 20):
            labels, boxes = make_targets(B, 91, G, dev)
            routes = {"fused": GenerateCDNQueries(900, 91, 256, 100, fused=True).to(dev), "torch": GenerateCDNQueries(900, 91, 256, 100, fused=False).to(dev)}
            routes["torch"].load_state_dict(routes["fused"].state_dict())
            upstream = torch.randn(B, 200, 256, generator=torch.Generator().manual_seed(1)).to(dev)
            for module in routes.values():
                for _ in range(3):
                    out = step(module, labels, boxes, upstream)
            wall = {name: [] for name in routes}
            for _ in range(args.runs):
                for name, module in routes.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    step(module, labels, boxes, upstream)
                    torch.cuda.synchronize()
                    wall[name].append((time.perf_counter() - t0) * 1e3)
            say(f"B = {B}, {G} boxes per image: {out[3]} groups of {out[4]}, {out[0].shape[1]} denoising queries per image, mask {tuple(out[2].shape)}")
            for name, module in routes.items():
                w = wall[name]
                line = f"  {name:5s} wall {statistics.median(w):8.3f} ms ({min(w):.3f} - {max(w):.3f})"
                try:
                    prof = profile_step(module, labels, boxes, upstream)
                except Exception as e:                                               # noqa: BLE001 -- the profiler is optional here
                    prof = None
                    line += f"   profiler failed: {type(e).__name__}"
                if prof is None:
                    line += "   device time, launches, syncs: not measured"
                else:
                    line += f"   device {prof[0] / 1e3:7.3f} ms   launches {prof[1]:5d}   syncs {prof[2]:4d}"
                    line += " (" + ", ".join(f"{k} {v}" for k, v in sorted(prof[3].items())) + ")"
                say(line)
            say(f"  wall: torch / fused = {statistics.median(wall['torch']) / statistics.median(wall['fused']):.2f}x")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
