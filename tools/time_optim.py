"""A/B of the optimizer step: FusedAdamW(fused=True) (clip + step, csrc/optim.hip) against torch's two multi-tensor routes, same
process, same parameter shapes and gradients, alternating.

The case is the full R50 parameter set of build_relation_transformer() at its defaults (317 tensors, 19,752,960 fp32 elements) with a
gradient of full size on every tensor, max_norm = 0.1, lr = weight_decay = 1e-4 over relation_param_groups.  Routes:
  fused         FusedAdamW(fused=True).clip_grad_norm_ + .step()
  foreach       torch.nn.utils.clip_grad_norm_(foreach=True) + torch.optim.AdamW(foreach=True).step()
  torch-fused   torch.nn.utils.clip_grad_norm_(foreach=True) + torch.optim.AdamW(fused=True).step()
Per route:
  wall      host clock from an idle device (synchronised before) to the synchronise after the step: median and spread of the runs
  stream    device events around `--burst` steps issued back to back, per step: the rate the device sustains when the host runs ahead
  device    sum of the kernel and copy durations of one step (torch.profiler, a pass of its own);  launches: kernels + device copies
  bytes/s   the byte model over the device time: this route moves 8 fp32 streams per element (the norm reads g; the update reads
            g, p, m, v and writes p, m, v), the torch routes 10 (the norm reads g, the scale reads and writes g, the update moves 7)
The torch routes scale their gradients in place, so theirs shrink from run to run until the coefficient is 1; the work stays the same.

--sweep times the fused route's three launches alone (device events around bursts of them) over chunk sizes and grid caps: how
optim.CHUNK and the library's grid cap were chosen.

Run on the GPU:  python tools/time_optim.py [--runs 20] [--sweep]      (--rehearse: a tiny set on the CPU, torch route only, no timings)
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd import FusedAdamW, build_relation_transformer, optim, relation_param_groups  # noqa: E402

MAX_NORM, LR, WD = 0.1, 1e-4, 1e-4
STREAMS = {"fused": 8, "foreach": 10, "torch-fused": 10}


def make_route(name, device, seed=0):
    """(model, step function) of one route; every route gets the same parameters and gradients."""
    torch.manual_seed(seed)
    net = build_relation_transformer().to(device)
    g = torch.Generator(device=device).manual_seed(seed + 1)
    for p in net.parameters():
        p.grad = torch.randn(p.shape, generator=g, device=device) * 1e-3
    groups = relation_param_groups(net, LR)
    if name == "fused":
        opt = FusedAdamW(groups, lr=LR, weight_decay=WD, fused=True)

        def step():
            opt.clip_grad_norm_(MAX_NORM)
            opt.step()
    else:
        kw = {"foreach": True} if name == "foreach" else {"fused": True}
        opt = torch.optim.AdamW(groups, lr=LR, weight_decay=WD, **kw)
        params = [p for group in opt.param_groups for p in group["params"]]

        def step():
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
            opt.step()
    return net, step


def profile_step(step):
    """(device microseconds, launches, the device events by name) of one step, or None where the profiler gives no device events."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    device_us, launches, names = 0.0, 0, {}
    for e in prof.events():
        if str(e.device_type).endswith("CUDA") and not e.name.startswith("Optimizer."):      # the optimizer's profiler annotation
            device_us += e.device_time if hasattr(e, "device_time") else e.cuda_time
            launches += 1
            names[e.name] = names.get(e.name, 0) + 1
    return (device_us, launches, names) if launches else None


def stream_ms(step, burst):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(burst):
        step()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / burst


def kernels_ms(opt, burst):
    """Device events around `burst` rounds of the fused route's three launches alone, per round, on the tables of opt's last step."""
    from relation_detr_amd import _lib
    lib, t = _lib.load(), opt._tables
    ws_bytes = int(lib.rdetr_optim_workspace_bytes(t["n_chunks"]))
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=t["table"].device)
    s = torch.cuda.current_stream().cuda_stream
    table = (t["tensors_ptr"], t["steps_ptr"], t["map_ptr"], t["n_tensors"], t["n_chunks"], optim.CHUNK, optim.GRID_CAP)

    def step():
        _lib.check(lib.rdetr_grad_sqnorm_f32(*table, ws.data_ptr(), ws_bytes, s), "sqnorm")
        _lib.check(lib.rdetr_grad_clip_coef(ws.data_ptr(), ws_bytes, t["n_chunks"], MAX_NORM, s), "coef")
        _lib.check(lib.rdetr_adamw_step_f32(*table, ws.data_ptr() + 4 * t["n_chunks"], s), "adamw")
    return stream_ms(step, burst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.rehearse:
        net = build_relation_transformer(d_ffn=64, enc_layers=1, dec_layers=1, num_queries=20, hybrid_num_proposals=30)
        for p in net.parameters():
            p.grad = torch.randn(p.shape) * 1e-3
        opt = FusedAdamW(relation_param_groups(net, LR), lr=LR, weight_decay=WD, fused=False)
        norm = opt.clip_grad_norm_(MAX_NORM)
        opt.step()
        n = sum(p.numel() for p in net.parameters())
        print(f"rehearsal on the CPU, not a measurement: {len(list(net.parameters()))} tensors, {n} elements, norm {norm.item():.4f}, "
              f"{len(optim.build_chunk_map([p.numel() for p in net.parameters()]))} chunks of {optim.CHUNK}")
        return
    if not torch.cuda.is_available():
        sys.exit("time_optim.py needs the GPU (--rehearse checks the host logic only)")
    dev = "cuda:0"
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; clip_grad_norm_ + AdamW step, {args.runs} alternating runs per route, "
          f"bursts of {args.burst}")
    routes = {}
    for name in STREAMS:
        routes[name] = make_route(name, dev)
    n_tensors = len(list(routes["fused"][0].parameters()))
    n_elem = sum(p.numel() for p in routes["fused"][0].parameters())
    print(f"# {n_tensors} tensors, {n_elem} fp32 elements; CHUNK = {optim.CHUNK}: "
          f"{len(optim.build_chunk_map([p.numel() for p in routes['fused'][0].parameters()]))} chunks; wall, stream and device in ms")
    for _, step in routes.values():
        for _ in range(5):
            step()
    wall = {name: [] for name in routes}
    stream = {name: [] for name in routes}
    for _ in range(args.runs):
        for name, (_, step) in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    for _ in range(5):
        for name, (_, step) in routes.items():
            stream[name].append(stream_ms(step, args.burst))
    for name, (_, step) in routes.items():
        w, s = wall[name], stream[name]
        model = STREAMS[name] * 4 * n_elem
        line = (f"  {name:11s} wall {statistics.median(w):7.3f} ({min(w):.3f} - {max(w):.3f})   stream {statistics.median(s):7.3f} "
                f"({min(s):.3f} - {max(s):.3f}) = {model / statistics.median(s) / 1e9:6.2f} TB/s of {model / 1e6:.0f} MB")
        try:
            prof = profile_step(step)
        except Exception as e:                                                   # noqa: BLE001 -- the profiler is optional here
            prof = None
            line += f"   profiler failed: {type(e).__name__}"
        if prof is None:
            line += "   device time, launches: not measured"
        else:
            line += f"   device {prof[0] / 1e3:7.3f} = {model / prof[0] / 1e6:6.2f} TB/s   launches {prof[1]:5d}"
            if prof[1] <= 8:
                line += " (" + ", ".join(f"{v} x {k.replace('(anonymous namespace)::', '').split('(')[0][:60].strip()}" for k, v in prof[2].items()) + ")"
        print(line, flush=True)
    for other in ("foreach", "torch-fused"):
        print(f"  {other} / fused: wall {statistics.median(wall[other]) / statistics.median(wall['fused']):.2f}x, "
              f"stream {statistics.median(stream[other]) / statistics.median(stream['fused']):.2f}x", flush=True)
    if args.sweep:
        net = routes["fused"][0]
        chunk0, cap0 = optim.CHUNK, optim.GRID_CAP
        print("# fused route, the three launches alone: ms per round (median of 5 bursts) by chunk size and grid cap")
        for chunk in (2048, 4096, 8192, 16384, 32768):
            cells = []
            for cap in (512, 1024, 2048, 4096, 1 << 20):
                optim.CHUNK, optim.GRID_CAP = chunk, cap
                opt = FusedAdamW(relation_param_groups(net, LR), lr=LR, weight_decay=WD, fused=True)

                def step():
                    opt.clip_grad_norm_(MAX_NORM)
                    opt.step()
                for _ in range(2):
                    step()
                cells.append(f"cap {cap:7d}: {statistics.median(kernels_ms(opt, args.burst) for _ in range(5)):.4f}")
            print(f"  chunk {chunk:6d}   " + "   ".join(cells), flush=True)
        optim.CHUNK, optim.GRID_CAP = chunk0, cap0


if __name__ == "__main__":
    main()
