"""A/B of the training augmentation (frontend/augment.py): decoded uint8 images -> the normalised, padded batch and its mask.

Routes, same process, same images and the same recorded choices, alternating:
  fused     DetrAugment(fused=True) on device images: csrc/images.hip, at most two launches per 16 images
  torch     DetrAugment(fused=False) on the same device images: the reference's operator sequence as device kernels
  host      DetrAugment(fused=False) on host images, then the upload of the fp32 batch and the mask: what a user does today with the
            reference's transforms on the CPU (the number to beat).  Its torch threads are whatever the process was given.

Shapes: uint8 sources of 480 x 640, 427 x 640, 640 x 480 and 375 x 500 (image b of a batch is entry b % 4), the real ``detr`` preset;
B = 1, 2, 4, 16; every image on the resize branch, every image on the crop branch, and the branches as drawn.  Per point and route:
  device    device events around a window of calls, per call: median (min - max) of 5 windows per route, alternating.  The host route's
            window is shorter (--host-iters); its time is host time, which the events enclose
  busy      the summed durations of one call's kernels and device copies (torch.profiler, median of 5 calls, a pass of its own)
  launches  kernels + device copies of one call (same pass)
  bytes     a model from the shapes: fused = the sources read once + the uint8 scratch written and read once + batch + mask written once;
            host = the upload (batch + mask)

Run on the GPU:  python tools/time_augment.py [--iters 50] [--host-iters 3] [--batches 1,2,4,16] [--out profiles/r31/augment_ab.txt]
(--rehearse: tiny shapes on the CPU, torch route only, no timings)
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relation_detr_amd import DetrAugment, detr_plan, sample_detr_choices  # noqa: E402
from time_preprocess import SOURCES, busy_of, launches_of, make_images  # noqa: E402


def choices_for(sizes, branch, seed, **preset):
    """One choice per image from a seeded generator, every image on ``branch`` ("resize", "crop") or as drawn ("mix")."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for size in sizes:
        while True:
            c = sample_detr_choices([size], g, **preset)[0]
            if branch == "mix" or c.crop == (branch == "crop"):
                out.append(c)
                break
    return out


def fused_bytes(images, choices, batch, max_size, crop_range):
    total = sum(im.numel() for im in images) + batch.tensors.numel() * batch.tensors.element_size() + batch.mask.numel()
    for im, c in zip(images, choices):
        (_, first, crop), final = detr_plan(im.shape[1], im.shape[2], c, max_size, crop_range)
        if first is not None and tuple(crop[2:]) != tuple(final):
            total += 2 * 3 * crop[2] * ((crop[3] + 15) // 16 * 16)
    return total


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--batches", default="1,2,4,16")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.rehearse:
        small = dict(scales=(48, 56, 64), crop_resize=(40, 50), crop_range=(38, 60))
        images = make_images(3, "cpu", ((70, 100), (95, 130)))
        aug = DetrAugment(max_size=133, fused=False, **small).train()
        for branch in ("resize", "crop", "mix"):
            choices = choices_for([tuple(im.shape[1:]) for im in images], branch, 1, **small)
            batch, _ = aug(images, None, choices)
            print("rehearsal on the CPU, not a measurement:", branch, tuple(batch.tensors.shape), batch.image_sizes.tolist(),
                  fused_bytes(images, choices, batch, 133, (38, 60)), "bytes in the fused model")
        return
    if not torch.cuda.is_available():
        sys.exit("time_augment.py needs the GPU (--rehearse checks the host logic only)")
    dev = "cuda:0"
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {torch.get_num_threads()} host threads; training augmentation, uint8 "
        f"sources {SOURCES}, the detr preset; device ms per call over windows of {args.iters} calls ({args.host_iters} for the host route), "
        f"median (min - max) of 5")
    lost = []
    points = [(B, torch.float32, False) for B in (int(b) for b in args.batches.split(","))] + [(4, torch.bfloat16, True)]
    for B, dtype, cl in points:
        on_device, on_host = make_images(B, dev), make_images(B, "cpu")
        routes = {"fused": (DetrAugment(dtype=dtype, channels_last=cl, fused=True).train(), on_device),
                  "torch": (DetrAugment(dtype=dtype, channels_last=cl, fused=False).train(), on_device),
                  "host": (DetrAugment(dtype=dtype, channels_last=cl, fused=False).train(), on_host)}
        for branch in ("resize", "crop", "mix"):
            choices = choices_for([tuple(im.shape[1:]) for im in on_host], branch, 100 + B)
            assert routes["fused"][0].takes_fused_route(on_device, choices)

            def call(name):
                aug, images = routes[name]
                batch, _ = aug(images, None, choices)
                if name == "host":
                    return batch.tensors.to(dev), batch.mask.to(dev)
                return batch.tensors, batch.mask
            fns = {name: (lambda name=name: call(name)) for name in routes}
            batch = routes["fused"][0](on_device, None, choices)[0]
            for name, fn in fns.items():
                for _ in range(1 if name == "host" else 3):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in fns}
            for _ in range(5):
                for name, fn in fns.items():
                    times[name].append(window(fn, args.host_iters if name == "host" else args.iters))
            layout = "channels-last" if cl else "NCHW"
            crops = sum(c.crop for c in choices)
            say(f"B = {B}, {branch}: {crops} of {B} images on the crop branch, batch {tuple(batch.tensors.shape)} {str(dtype).split('.')[-1]} {layout}")
            upload = batch.tensors.numel() * batch.tensors.element_size() + batch.mask.numel()
            model = {"fused": fused_bytes(on_host, choices, batch, 1333, (384, 600)), "host": upload}
            med = {}
            for name, fn in fns.items():
                med[name] = statistics.median(times[name])
                note = f"   {model[name] / 1e6:8.2f} MB in the model" if name in model else ""
                say(f"  {name:5s} device {med[name]:9.4f} ms ({min(times[name]):.4f} - {max(times[name]):.4f})   kernels busy "
                    f"{busy_of(fn):8.4f} ms   launches {launches_of(fn):4d}{note}")
            say(f"  torch / fused: {med['torch'] / med['fused']:.2f}x   host + upload / fused: {med['host'] / med['fused']:.2f}x per call")
            if med["fused"] >= min(med["torch"], med["host"]):
                lost.append((B, branch, str(dtype), layout))
    say(f"points where the fused route is not the fastest: {lost if lost else 'none'}")


if __name__ == "__main__":
    main()
