"""A/B of the training criterion: RelationCriterion(fused=True) with scipy's solver on the host ("fused"), the same with the
assignments solved on the device ("device", matcher="device": csrc/assign.hip) and the torch route (fused=False, the reference's
loops), forward + backward, same process, same inputs, alternating.

Shapes of the R50 configuration: 6 decoder layers, 900 matching + 200 denoising queries, 1500 hybrid queries, 91 classes; B = 2 and
4 images with 7 and 20 boxes each.  Per route and shape:
  wall      host clock from an idle device (synchronised before) to the synchronise after backward, median and spread of the runs,
            and the part of it spent inside scipy's linear_sum_assignment, which the fused and the torch route call
  device    sum of the kernel and copy durations of one step (torch.profiler, a pass of its own); for the device matcher also
            the part of it inside assign_match_kernel and that kernel's launches
  launches  kernels + device copies of that step;  syncs: runtime calls that wait for the device (synchronise calls and blocking copies)

Run on the GPU:  python tools/time_criterion.py [--runs 20]      (--rehearse: tiny shapes on the CPU, torch route only, no timings)
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd import RelationCriterion  # noqa: E402


def make_inputs(L, B, C, nq, n_dn, nh, boxes_per_image, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = lambda *s: (2 * torch.randn(*s, C, generator=g)).clamp(-6, 6).to(device).requires_grad_(True)
    boxes = lambda *s: torch.cat((torch.rand(*s, 2, generator=g), 0.02 + 0.4 * torch.rand(*s, 2, generator=g)), -1).to(device)
    outs = [logits(L, B, n_dn + nq), boxes(L, B, n_dn + nq).requires_grad_(True), logits(B, nq), boxes(B, nq).requires_grad_(True),
            logits(L, B, nh), boxes(L, B, nh).requires_grad_(True), logits(B, nh), boxes(B, nh).requires_grad_(True)]
    targets = [{"labels": torch.randint(0, C, (boxes_per_image,), generator=g).to(device), "boxes": boxes(boxes_per_image)} for _ in range(B)]
    return outs, targets


SOLVER = {"seconds": 0.0}
ASSIGN = {"us": 0.0, "launches": 0}                 # the assignment kernel's share of the last profiled step


def time_the_solver():
    """Both routes look scipy's solver up at call time: count the seconds spent inside it."""
    import scipy.optimize
    solve = scipy.optimize.linear_sum_assignment

    def timed(*args, **kwargs):
        t0 = time.perf_counter()
        try:
            return solve(*args, **kwargs)
        finally:
            SOLVER["seconds"] += time.perf_counter() - t0
    scipy.optimize.linear_sum_assignment = timed


def step(criterion, outs, targets, dn_meta):
    for o in outs:
        o.grad = None
    losses = criterion(tuple(outs), targets, dn_meta)
    torch.stack(list(losses.values())).sum().backward()
    return losses


def profile_step(criterion, outs, targets, dn_meta):
    """(device microseconds, launches, syncs, the waiting calls by name) of one step, or None where the profiler gives no device events."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step(criterion, outs, targets, dn_meta)
        torch.cuda.synchronize()
    device_us, launches, waits = 0.0, 0, {}
    ASSIGN["us"], ASSIGN["launches"] = 0.0, 0
    for e in prof.events():
        if str(e.device_type).endswith("CUDA"):
            us = e.device_time if hasattr(e, "device_time") else e.cuda_time
            device_us += us
            launches += 1
            if "assign_match_kernel" in e.name:
                ASSIGN["us"] += us
                ASSIGN["launches"] += 1
        elif "Synchronize" in e.name or e.name in ("hipMemcpyWithStream", "hipMemcpy"):
            waits[e.name] = waits.get(e.name, 0) + 1
    if "hipDeviceSynchronize" in waits:                                               # the synchronise that closes the window
        waits["hipDeviceSynchronize"] -= 1
    waits = {k: v for k, v in waits.items() if v}
    return (device_us, launches, sum(waits.values()), waits) if launches else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    time_the_solver()
    if args.rehearse:
        outs, targets = make_inputs(2, 2, 7, 12, 4, 16, 3, "cpu")
        losses = step(RelationCriterion(7, fused=False), outs, targets, (1, 4))
        print("rehearsal on the CPU, not a measurement:", len(losses), "losses, total", float(sum(v.item() for v in losses.values())))
        return
    if not torch.cuda.is_available():
        sys.exit("time_criterion.py needs the GPU (--rehearse checks the host logic only)")
    dev = "cuda:0"
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; forward + backward of the criterion, {args.runs} alternating runs per route")
    print("# L = 6, 900 matching queries, 1500 hybrid queries, C = 91; wall in ms (median, min - max); device = kernel + copy time of one step")
    for B in (2, 4):
        for G in (7, 20):
            max_gt = 8 if G == 7 else 20                                              # 25 x 8 and 10 x 20 denoising queries: 200
            dn_meta = (200 // max_gt, max_gt)
            outs, targets = make_inputs(6, B, 91, 900, 200, 1500, G, dev)
            routes = {"fused": RelationCriterion(91, fused=True), "device": RelationCriterion(91, fused=True, matcher="device"),
                      "torch": RelationCriterion(91, fused=False)}
            values = {}
            for name, c in routes.items():
                for _ in range(3):
                    values[name] = step(c, outs, targets, dn_meta)
            worst = max(abs(values["fused"][k].item() - values["torch"][k].item()) / max(1.0, abs(values["torch"][k].item()))
                        for k in values["torch"])
            wall = {name: [] for name in routes}
            solver = {name: 0.0 for name in routes}
            for _ in range(args.runs):
                for name, c in routes.items():
                    torch.cuda.synchronize()
                    SOLVER["seconds"] = 0.0
                    t0 = time.perf_counter()
                    step(c, outs, targets, dn_meta)
                    torch.cuda.synchronize()
                    wall[name].append((time.perf_counter() - t0) * 1e3)
                    solver[name] += SOLVER["seconds"] * 1e3 / args.runs
            same = all(torch.equal(values["device"][k], values["fused"][k]) for k in values["fused"])
            print(f"B = {B}, {G} boxes per image, dn_meta = {dn_meta}: {len(values['torch'])} losses, worst |fused - torch| / max(1, |torch|) = {worst:.2e}, "
                  f"device matcher's losses {'equal' if same else 'DIFFER from'} the scipy matcher's bit for bit")
            for name, c in routes.items():
                w = wall[name]
                line = f"  {name:6s} wall {statistics.median(w):8.2f} ms ({min(w):.2f} - {max(w):.2f}), of which scipy's solver {solver[name]:6.2f} ms (mean)"
                try:
                    prof = profile_step(c, outs, targets, dn_meta)
                except Exception as e:                                               # noqa: BLE001 -- the profiler is optional here
                    prof = None
                    line += f"   profiler failed: {type(e).__name__}"
                if prof is None:
                    line += "   device time, launches, syncs: not measured"
                else:
                    line += f"   device {prof[0] / 1e3:7.3f} ms   launches {prof[1]:5d}   syncs {prof[2]:4d}"
                    line += " (" + ", ".join(f"{k} {v}" for k, v in sorted(prof[3].items())) + ")"
                    if name == "device":
                        line += f"   of the device time assign_match_kernel {ASSIGN['us'] / 1e3:.3f} ms in {ASSIGN['launches']} launches"
                print(line, flush=True)
            print(f"  wall: torch / fused = {statistics.median(wall['torch']) / statistics.median(wall['fused']):.2f}x, "
                  f"fused / device = {statistics.median(wall['fused']) / statistics.median(wall['device']):.2f}x", flush=True)


if __name__ == "__main__":
    main()
