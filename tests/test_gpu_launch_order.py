"""A kernel's dynamic-LDS attribute must not depend on which of its template instantiations a process launches first.

The host wrappers allow each kernel its dynamic LDS once, through a function-local static.  Where that static was shared between
the instantiations of a kernel template (the resident MSDA kernel's four variants shared one), only the variant a process
launched FIRST ever got the attribute.  Every case below is therefore a fresh process whose first and only launch of the kernel
family is one particular variant, checked against the CPU reference at the bound of that kernel's own parity test:

    resident MSDA (csrc/msda_res.hip), B = 1, pyramids of test_gpu_resident.py; msda_res_forward's `lr` picks the variant:
        L = 4, levels 2 + 3 resident    L = 4, only level 3 fits    L = 5, levels 3 + 4 resident    L = 5, only level 4 fits
    linear_k256 (csrc/linear.hip) with N = 384 first: the NT = 12 instantiation
    encoder_proj (csrc/proj.hip) with q_cols = 480 first

Today's runtime does not enforce the attribute, so this passed before the statics were made per kernel as well: it pins the
property, it does not demonstrate the bug.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RESIDENT = {
    "resident_L4_two_levels": [(12, 20), (6, 10), (3, 5), (2, 3)],
    "resident_L4_one_level": [(160, 160), (80, 80), (48, 48), (20, 20)],
    "resident_L5_two_levels": [(76, 126), (38, 63), (19, 32), (10, 16), (5, 8)],
    "resident_L5_one_level": [(300, 500), (150, 250), (75, 125), (38, 63), (19, 32)],
}
CASES = sorted(RESIDENT) + ["linear_k256_N384", "encoder_proj_q480"]


def _child(case):
    sys.path.insert(0, ROOT)
    import torch
    from relation_detr_amd import _lib, ops
    _lib.load()
    dev = "cuda:0"
    if case in RESIDENT:
        from oracle import c_oracle
        from test_gpu_window import _check, _encoder_inputs, _head_major
        value, shp, start, loc, attn, S, L = _encoder_inputs(RESIDENT[case], 1, 4.0, seed=7)
        out = ops.ms_deform_attn_forward(_head_major(value.to(dev)), shp.to(dev), start.to(dev), loc.to(dev), attn.to(dev),
                                         value_layout="bhsd", algo="resident").float().cpu().numpy()
        _check(out, c_oracle.msda_forward(value.float().numpy(), shp.numpy(), start.numpy(), loc.numpy(), attn.numpy()))
        return
    g = torch.Generator().manual_seed(3)
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)
    if case == "linear_k256_N384":
        x, w, b = rnd(700, 256), rnd(384, 256, scale=0.06), rnd(384)
        got = ops.linear_k256(x.to(dev), w.to(dev), b.to(dev)).float().cpu()
        want = x.float() @ w.float().t() + b.float()
        assert float(((got - want).abs() - want.abs() * 2 ** -8).max()) <= 2e-3
    elif case == "encoder_proj_q480":
        x, xq, wv, bv = rnd(2, 700, 256), rnd(2, 700, 256), rnd(256, 256, scale=0.06), rnd(256, scale=0.1)
        wq, bq = rnd(480, 256, scale=0.06), rnd(480, scale=0.1)
        vh, q = ops.encoder_proj(x.to(dev), xq.to(dev), wv.to(dev), bv.to(dev), wq.to(dev), bq.to(dev), None)
        want_v = (x.float() @ wv.float().t() + bv.float()).view(2, 700, 8, 32).permute(0, 2, 1, 3)
        want_q = xq.float() @ wq.float().t() + bq.float()
        for got, want in ((vh.float().cpu(), want_v), (q.float().cpu(), want_q)):
            assert ((got - want).abs() <= 2.0 ** -8 * want.abs() + 2e-3).all()
    else:
        raise SystemExit(f"unknown case {case}")


@pytest.mark.gpu
def test_each_variant_as_the_first_launch_of_a_process():
    for case in CASES:                                             # in turn; nothing more is started after a child that failed
        p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), case], capture_output=True, text=True)
        assert p.returncode == 0, f"{case}: exit status {p.returncode}\n{p.stderr[-2000:]}"


if __name__ == "__main__":
    _child(sys.argv[1])
