#!/usr/bin/env python3
"""Bits of the three MSDA backward operators on a fixed seeded list of small cases: one SHA-256 per output tensor.

Run it once per library build (``RDETR_LIB_PATH`` selects the library of a process) and diff the two outputs: a refactor of
csrc/msda_bwd.hip must leave every line the same.

  mat    ops.ms_deform_attn_backward                      fp32, locations / weights materialised on the host
  fused  ops.ms_deform_attn_backward_fused                fp32 and bf16, value [B,S,H,D]
  hm     msda_train_hm.ms_deform_attn_backward_fused_hm   bf16, head-major value; producers dense and as column slices of one buffer

Cases: L in {1, 3, 4, 5, 8} x ref_dim in {2, 4} x Nq in {5, 11, 37}, B = 2, inputs of tests' ``producer_inputs`` (one NaN offset,
points outside their level), atomic and deterministic mode.  The atomic grad_value is run-dependent: it is not hashed but held
to the tests' bound (close_abs / close_bf16) against the deterministic grad_value of the same library; lines starting with '#'
carry those figures and are left out of a diff.

    python tools/msda_bwd_bits.py > bits.txt
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from relation_detr_amd import _lib, msda_train_hm, ops  # noqa: E402
from relation_detr_amd.ms_deform_attn import sampling_locations  # noqa: E402
from test_gpu_msda_train_fused import SHAPES1, SHAPES4, SHAPES5, SHAPES8, close_abs, close_bf16, producer_inputs  # noqa: E402

SHAPES3 = [(9, 13), (5, 7), (3, 4)]
DEV = "cuda:0"


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def report(tag, names, atomic, det, close):
    for name, a, d in zip(names, atomic, det):
        if name == "grad_value":
            close(a, d, f"{tag} atomic grad_value against deterministic")
            print(f"# {tag} atomic grad_value max |atomic - det| {float((a - d).abs().max()):.3e}")
        else:
            print(f"{tag} atomic {name} {sha(a)}")
        print(f"{tag} det    {name} {sha(d)}")


def main():
    if not torch.cuda.is_available():
        sys.exit("msda_bwd_bits.py needs a GPU")
    print(f"# library {os.path.basename(_lib.LIB_PATH)} abi {_lib.load().rdetr_abi_version()}")
    fused_names = ("grad_value", "grad_offsets", "grad_logits", "grad_ref")
    for shapes in (SHAPES1, SHAPES3, SHAPES4, SHAPES5, SHAPES8):
        for ref_dim in (2, 4):
            for Nq in (5, 11, 37):
                L = len(shapes)
                for dtype in (torch.float32, torch.bfloat16):
                    tag = f"L{L} ref{ref_dim} Nq{Nq} {str(dtype).split('.')[-1]}"
                    close = close_abs if dtype == torch.float32 else close_bf16
                    inp = producer_inputs(2, Nq, shapes, ref_dim, seed=1000 * L + 10 * Nq + ref_dim, dtype=dtype)[:7]
                    value, shp, start, off, lg, ref, go = (t.to(DEV).contiguous() for t in inp)
                    run = lambda det: ops.ms_deform_attn_backward_fused(value, shp, start, off, lg, ref, go, deterministic=det,
                                                                        need_ref_grad=True)
                    report(f"{tag} fused", fused_names, run(False), run(True), close)
                    if dtype == torch.float32:
                        loc = sampling_locations(ref, off, shp, 4).contiguous()
                        w = lg.softmax(-1).view(2, Nq, 8, L, 4).contiguous()
                        run = lambda det: ops.ms_deform_attn_backward(value, shp, start, loc, w, go, deterministic=det)
                        report(f"{tag} mat", ("grad_value", "grad_loc", "grad_attn"), run(False), run(True), close)
                        continue
                    vh = value.permute(0, 2, 1, 3).contiguous()
                    n = 8 * L * 4
                    both = torch.cat([off.view(2, Nq, 2 * n), lg.view(2, Nq, n), torch.zeros(2, Nq, 6, dtype=dtype, device=DEV)], -1)
                    sliced = (both[..., :2 * n].view(off.shape), both[..., 2 * n:3 * n].view(lg.shape))
                    for what, (o, l_) in (("hm dense", (off, lg)), ("hm sliced", sliced)):
                        run = lambda det: msda_train_hm.ms_deform_attn_backward_fused_hm(vh, shp, start, o, l_, ref, go, deterministic=det,
                                                                                       need_ref_grad=True)
                        report(f"{tag} {what}", fused_names, run(False), run(True), close)
    torch.cuda.synchronize()
    print("# done")


if __name__ == "__main__":
    main()
