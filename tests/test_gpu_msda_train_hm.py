"""GPU tests of the head-major MSDA training route (relation_detr_amd/msda_train_hm.py): the re-layout kernel of the value
gradient (csrc/glue.hip), the fused-producer backward on a head-major value (csrc/msda_bwd.hip, msda_bwd_fused_kernel<.., HM>),
``MultiScaleDeformableAttnHeadMajorFunction`` and ``MultiScaleDeformableAttention`` under ``msda_train_head_major``.

Oracle: float64 torch autograd on the CPU (test_gpu_msda_train_fused.oracle) on the bf16-rounded inputs; bound
|err| <= 2^-8 * |ref| + 1e-3 * max(1, |ref|max), offsets and reference points away from interpolation kinks.  Everything that can
be compared with the [B,S,H,D] fused backward is compared bit for bit: the layout is an addressing matter only.
"""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import kink_mask, pyramid
from test_gpu_msda_train_fused import (DEV, NAN_AT, SHAPES1, SHAPES4, SHAPES5, SHAPES8, _n, close_bf16, kept_enough, oracle, producer_inputs,
                                       ref_mask)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SHAPES3 = [(9, 13), (5, 7), (3, 4)]
# one block of the backward serves 8 queries: Nq = 5 is below that, Nq = 37 no multiple of it, Nq = 11 one full block and a tail
# whose last wave holds a single valid query
CASES = [(SHAPES4, 37, 2), (SHAPES4, 5, 2), (SHAPES5, 37, 2), (SHAPES5, 5, 4), (SHAPES3, 37, 2),
         (SHAPES8, 11, 2), (SHAPES8, 11, 4), (SHAPES1, 11, 2), (SHAPES1, 11, 4)]
Q_LAST, Q_FIRST = 1, 2                 # queries (image 1) whose corners are pixel S-1 / pixel 0
RESIDENT_SHAPES = [(100, 134), (50, 67), (25, 34), (13, 17)]      # S = 17,821 >= 16,384: "auto" takes the resident kernel
MODULE_SHAPES = [(56, 76), (28, 38), (14, 19), (7, 10)]           # S = 5,656: the smallest such pyramid past the 4,096 gate


@pytest.fixture(scope="module")
def hm():
    from relation_detr_amd import _lib, msda_train_hm
    _lib.load()
    return msda_train_hm


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def head_major(value):
    return value.permute(0, 2, 1, 3).contiguous()


# ------------------------------------------------------------------------------------------------------------ 1. re-layout
def _relayout_inputs():
    g = torch.Generator().manual_seed(1)
    B, S = 2, 291
    grad = torch.randn(B, 8, S, 32, generator=g)
    mask = torch.zeros(B, S, dtype=torch.bool)
    mask[1, 250:] = True
    mask[1, 7] = True
    grad[0, 3, 10, 5] = float("inf")                     # outside every padded row
    grad[1, 2, 11, 31] = float("nan")
    grad[1, 0, 260, 0] = float("inf")                    # inside padded rows: never read, written as zero
    grad[1, 7, 7, 9] = float("nan")
    return grad.to(DEV), mask.to(DEV)


def _relayout_want(grad, mask):
    B, _, S, _ = grad.shape
    want = grad.permute(0, 2, 1, 3).reshape(B, S, 256).to(BF)
    return want if mask is None else want.masked_fill(mask[..., None], 0)


@pytest.mark.parametrize("masked", [True, False])
def test_grad_value_from_head_major_is_the_permuted_cast(hm, masked):
    grad, mask = _relayout_inputs()
    mask = mask if masked else None
    got = hm.grad_value_from_head_major(grad, mask)
    want = _relayout_want(grad, mask)
    assert got.dtype == BF and got.is_contiguous() and same_bits(got, want)
    assert torch.isnan(got[1, 11, 2 * 32 + 31]) and torch.isinf(got[0, 10, 3 * 32 + 5])
    if masked:
        assert not got[1, 250:].any() and not got[1, 7].any()
        assert same_bits(hm.grad_value_from_head_major(grad, mask.to(torch.uint8)), want)


def test_grad_value_from_head_major_into_a_column_slice(hm):
    grad, mask = _relayout_inputs()
    B, S = mask.shape
    wide = torch.full((B, S, 384), 7.0, dtype=BF, device=DEV)
    out = hm.grad_value_from_head_major(grad, mask, out=wide[..., 64:320])
    assert out.data_ptr() == wide[..., 64:320].data_ptr()
    assert same_bits(wide[..., 64:320], _relayout_want(grad, mask))
    assert (wide[..., :64] == 7.0).all() and (wide[..., 320:] == 7.0).all()
    assert hm.grad_value_from_head_major(torch.zeros(0, 8, 5, 32, device=DEV)).shape == (0, 5, 256)


# ------------------------------------------------------------------------------------------------------------ 2-4. backward
@functools.lru_cache(maxsize=None)
def _case(idx):
    """Inputs of CASES[idx] (B = 2, NaN offset, points outside their level, the two corner queries), the fp64 oracle and the four
    runs: head-major and [B,S,H,D], atomic and deterministic.  Computed once, read by every test."""
    from relation_detr_amd import msda_train_hm, ops
    shapes, Nq, ref_dim = CASES[idx]
    B = 2
    value, shp, start, off, lg, ref, go, off_o = producer_inputs(B, Nq, shapes, ref_dim, seed=300 + idx, dtype=BF)
    h_last, w_last = shapes[-1]
    L = len(shapes)
    # bottom-right corner of every head's points on the last level = its pixel (h-1, w-1) = pixel S-1 (x = w - 1.5, y = h - 1.5)
    ref[1, Q_LAST, L - 1, :2] = torch.tensor([(w_last - 1) / w_last, (h_last - 1) / h_last])
    # ... and on level 0 only the bottom-right corner inside, at pixel (0, 0) = pixel 0 (x = y = -0.5)
    ref[1, Q_FIRST, 0, :2] = 0.0
    for t in (off, off_o):
        t[1, Q_LAST, :, L - 1] = 0
        t[1, Q_FIRST, :, 0] = 0
    dev = [t.to(DEV).contiguous() for t in (value, shp, start, off, lg, ref, go)]
    vh = head_major(dev[0])
    res = {"inputs": (value, shp, start, off, lg, ref, go), "dev": dev, "vh": vh, "S": value.shape[1]}
    res["oracle"] = oracle(value.double(), shp, off_o, lg.double(), ref, go.double())
    for det in (False, True):
        res["hm", det] = msda_train_hm.ms_deform_attn_backward_fused_hm(vh, *dev[1:], deterministic=det, need_ref_grad=True)
        res["bshd", det] = ops.ms_deform_attn_backward_fused(*dev, deterministic=det, need_ref_grad=True)
    res["hm2"] = msda_train_hm.ms_deform_attn_backward_fused_hm(vh, *dev[1:], deterministic=True, need_ref_grad=True)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"L{len(s)}-Nq{n}-ref{r}" for s, n, r in CASES])
@pytest.mark.parametrize("deterministic", [False, True])
def test_head_major_backward_matches_oracle(hm, idx, deterministic):
    c = _case(idx)
    _, shp, _, _, _, _, _ = c["inputs"]
    gv, goff, glg, gref = c["hm", deterministic]
    assert gv.dtype == torch.float32 and goff.dtype == BF and glg.dtype == BF and gref.dtype == torch.float32
    assert gv.shape == c["vh"].shape
    _, rv, ro, rl, rr, loc = c["oracle"]
    gv_bshd = gv.permute(0, 2, 1, 3)
    kept_enough(CASES[idx][0], loc, shp)
    close_bf16(gv_bshd, rv, "grad_value")
    close_bf16(glg, rl, "grad_logits")
    close_bf16(goff, ro, "grad_offsets", kink_mask(_n(loc), shp.numpy()))
    close_bf16(gref, rr, "grad_reference_points", np.broadcast_to(ref_mask(loc, shp), rr.shape))
    assert goff[NAN_AT].item() == 0.0                       # the NaN point contributes nothing
    # the rows at the two ends of the plane are reached (and only through in-range corners): non-zero in every head, and right
    for pixel in (c["S"] - 1, 0):
        row, want = gv_bshd[1, pixel], rv[1, pixel]
        assert (row.abs().amax(-1) > 0).all(), pixel
        close_bf16(row, want, f"grad_value row of pixel {pixel}")


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"L{len(s)}-Nq{n}-ref{r}" for s, n, r in CASES])
def test_layout_is_addressing_only(hm, idx):
    c = _case(idx)
    for det in (False, True):                              # fixed shuffle trees: the same bits in both layouts and both modes
        for k, what in ((1, "grad_offsets"), (2, "grad_logits"), (3, "grad_ref")):
            assert same_bits(c["hm", det][k], c["bshd", det][k]), (what, det)
            assert same_bits(c["hm", det][k], c["hm", True][k]), (what, det)
    # deterministic grad_value: the same products summed in the same stable sorted order per row
    assert same_bits(c["hm", True][0].permute(0, 2, 1, 3).contiguous(), c["bshd", True][0])
    assert all(same_bits(a, b) for a, b in zip(c["hm", True], c["hm2"]))
    np.testing.assert_allclose(c["hm", False][0].cpu().numpy(), c["hm", True][0].cpu().numpy(), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("idx,pad", [(0, 8), (2, 0), (4, 2)])
def test_strided_producers_and_merged_gradient_buffer(hm, idx, pad):
    c = _case(idx)
    _, shp, start, off, lg, ref, go = c["dev"]
    B, Nq, H, L, P, _ = off.shape
    n = H * L * P
    W = 3 * n + pad
    both = torch.full((B, Nq, W), 3.0, dtype=BF, device=DEV)
    both[..., :2 * n] = off.view(B, Nq, 2 * n)
    both[..., 2 * n:3 * n] = lg.view(B, Nq, n)
    off_s, lg_s = both[..., :2 * n].view(B, Nq, H, L, P, 2), both[..., 2 * n:3 * n].view(B, Nq, H, L * P)
    assert not off_s.is_contiguous()
    sentinel = -123.0
    for det in (False, True):
        dense = c["hm", det]
        buf = torch.full((B, Nq, W), sentinel, dtype=BF, device=DEV)
        got = hm.ms_deform_attn_backward_fused_hm(c["vh"], shp, start, off_s, lg_s, ref, go, deterministic=det, need_ref_grad=True,
                                                  grad_producer_out=buf)
        assert got[1].data_ptr() == buf.data_ptr() and got[2].data_ptr() == buf[..., 2 * n:].data_ptr()
        assert same_bits(buf[..., :2 * n], dense[1].view(B, Nq, 2 * n)) and same_bits(buf[..., 2 * n:3 * n], dense[2].view(B, Nq, n))
        assert (buf[..., 3 * n:] == sentinel).all()                     # nothing outside the two slices is written
        assert same_bits(got[3], dense[3])
        if det:
            assert same_bits(got[0], dense[0])
    # without a buffer of the caller's: the two gradients are the slices of ONE new [B, Nq, 3n] tensor
    got = hm.ms_deform_attn_backward_fused_hm(c["vh"], shp, start, off_s, lg_s, ref, go, deterministic=True)
    base = got[1]._base
    assert base is not None and base is got[2]._base and tuple(base.shape) == (B, Nq, 3 * n) and base.is_contiguous()
    assert got[2].data_ptr() == base.data_ptr() + 2 * n * 2 and got[3] is None
    assert same_bits(base[..., :2 * n], c["hm", True][1].view(B, Nq, 2 * n)) and same_bits(base[..., 2 * n:], c["hm", True][2].view(B, Nq, n))
    # strided inputs, dense outputs of their own (an offsets slice alone)
    got = hm.ms_deform_attn_backward_fused_hm(c["vh"], shp, start, off_s, lg, ref, go, deterministic=True)
    assert got[1].is_contiguous() and same_bits(got[1], c["hm", True][1]) and same_bits(got[2], c["hm", True][2])


# ------------------------------------------------------------------------------------------------------------ 5. Function
def _function_inputs(shapes, B, Nq, seed, pad_tail):
    g = torch.Generator().manual_seed(seed)
    shp, start, S = pyramid(shapes)
    L = len(shapes)
    Nq = S if Nq is None else Nq
    v = torch.randn(B, S, 256, generator=g).to(BF)
    off = torch.randn(B, Nq, 8, L, 4, 2, generator=g).to(BF)
    lg = (torch.randn(B, Nq, 8, L * 4, generator=g) * 2).to(BF)
    ref = torch.rand(B, Nq, L, 2, generator=g) * 1.2 - 0.1
    go = torch.randn(B, Nq, 256, generator=g).to(BF)
    mask = torch.zeros(B, S, dtype=torch.bool)
    mask[B - 1, S - pad_tail:] = True
    return [t.to(DEV) for t in (v, mask, shp, start, off, lg, ref, go)]


def _check_function(hm, ops, shapes, B, Nq, pad_tail, algo):
    v, mask, shp, start, off, lg, ref, go = _function_inputs(shapes, B, Nq, seed=21, pad_tail=pad_tail)
    vh = ops.value_to_head_major(v, mask)
    want = ops.ms_deform_attn_forward_fused(vh, shp, start, off, lg, ref, None, value_layout="bhsd")
    assert same_bits(want, ops.ms_deform_attn_forward_fused(vh, shp, start, off, lg, ref, None, value_layout="bhsd", algo=algo))
    leaves = [t.clone().requires_grad_(True) for t in (v, off, lg, ref)]
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        out = hm.MultiScaleDeformableAttnHeadMajorFunction.apply(leaves[0], mask, shp, start, leaves[1], leaves[2], leaves[3])
        assert out.dtype == BF and torch.equal(out.detach(), want)                  # the eval path's kernels, its bits
        out.backward(go)
    finally:
        torch.use_deterministic_algorithms(was)
    gv, goff, glg, gref = (t.grad for t in leaves)
    assert gv.dtype == BF and goff.dtype == BF and glg.dtype == BF and gref.dtype == torch.float32
    assert not gv[mask].any() and gv[~mask].any()                                    # exactly zero on the padded rows
    det = hm.ms_deform_attn_backward_fused_hm(vh, shp, start, off, lg, ref, go, deterministic=True, need_ref_grad=True)
    assert same_bits(gv, hm.grad_value_from_head_major(det[0], mask))
    assert same_bits(goff, det[1]) and same_bits(glg, det[2]) and same_bits(gref, det[3])
    # ... and, bit for bit, the [B,S,H,D] fused backward on the same (zero-filled) value
    v_bshd = vh.permute(0, 2, 1, 3).contiguous()
    old = ops.ms_deform_attn_backward_fused(v_bshd, shp, start, off, lg, ref, go, deterministic=True, need_ref_grad=True)
    assert same_bits(det[0].permute(0, 2, 1, 3).contiguous(), old[0])
    assert same_bits(det[1], old[1]) and same_bits(det[2], old[2]) and same_bits(det[3], old[3])
    # only the gradients autograd asks for
    only_v = v.clone().requires_grad_(True)
    hm.MultiScaleDeformableAttnHeadMajorFunction.apply(only_v, mask, shp, start, off, lg, ref).backward(go)
    assert only_v.grad is not None and not only_v.grad[mask].any()


def test_function_forward_is_the_eval_path_direct_kernel(hm):
    from relation_detr_amd import ops
    _check_function(hm, ops, SHAPES4, B=2, Nq=37, pad_tail=20, algo="direct")


def test_function_forward_is_the_eval_path_resident_kernel(hm):
    from relation_detr_amd import ops
    _, _, S = pyramid(RESIDENT_SHAPES)
    assert S == 17821 and ops._resident_pays(1, S, 4, RESIDENT_SHAPES)
    _check_function(hm, ops, RESIDENT_SHAPES, B=1, Nq=None, pad_tail=300, algo="resident")


# ------------------------------------------------------------------------------------------------------------ 6. module
def _module_inputs(shapes, B, Nq=None, ref_dim=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    shp, start, S = pyramid(shapes)
    Nq = S if Nq is None else Nq
    query = torch.randn(B, Nq, 256, generator=g).to(BF)
    value = torch.randn(B, S, 256, generator=g).to(BF)
    ref = torch.rand(B, Nq, 4, 2, generator=g)
    if ref_dim == 4:
        ref = torch.cat([ref, torch.rand(B, Nq, 4, 2, generator=g) * 0.4 + 0.05], -1)
    mask = torch.zeros(B, S, dtype=torch.bool)
    mask[B - 1, -S // 9:] = True
    go = torch.randn(B, Nq, 256, generator=g).to(BF)
    return query, value, ref, mask, go, shp, start


def _run_module(mod, query, value, ref, mask, go, shp, start, dtype):
    q, v = (t.to(DEV).to(dtype).requires_grad_(True) for t in (query, value))
    r = ref.to(DEV).requires_grad_(True)
    out = mod(q, r, v, shp.to(DEV), start.to(DEV), mask.to(DEV))
    out.backward(go.to(DEV).to(dtype))
    res = {"output": out.detach(), "d/d query": q.grad, "d/d value": v.grad, "d/d reference_points": r.grad}
    res.update({n: p.grad for n, p in mod.named_parameters()})
    return res


def test_module_route_is_as_accurate_as_the_bshd_training_route(hm):
    """fp32 on the materialised route (the same weights) is the reference; per tensor the worst |err| / max(1, max|ref|) of the new
    route (b) against that of ``msda_train_fused`` (a): err_b <= 1.5 * err_a + 2^-9 -- both round at the same places."""
    from relation_detr_amd import MultiScaleDeformableAttention, options
    torch.manual_seed(0)
    with options.override(msda_train_fused=False, msda_train_head_major=False):
        base = MultiScaleDeformableAttention(256, 4, 8, 4).train()
    with torch.no_grad():                      # non-trivial offsets / logits projections; weights that bf16 holds exactly
        for p in base.parameters():
            p.add_(torch.randn_like(p) * 0.02)
            p.copy_(p.to(BF).float())
    state = base.state_dict()
    base = base.to(DEV)
    mods = {}
    for key, kw in (("a", dict(msda_train_fused=True, msda_train_head_major=False)), ("b", dict(msda_train_fused=True, msda_train_head_major=True))):
        with options.override(**kw):
            m = MultiScaleDeformableAttention(256, 4, 8, 4)
        m.load_state_dict(state)
        mods[key] = m.to(DEV).to(BF).train()
    inputs = _module_inputs(MODULE_SHAPES, B=2)
    assert inputs[1].shape[1] == 5656
    want = _run_module(base, *inputs, torch.float32)
    got = {k: _run_module(m, *inputs, BF) for k, m in mods.items()}
    lines = [f"{'tensor':32s} {'err_a (msda_train_fused)':>26s} {'err_b (msda_train_head_major)':>30s}"]
    bad = []
    for name, ref in want.items():
        scale = max(1.0, float(ref.abs().max()))
        ea, eb = (float((got[k][name].float() - ref.float()).abs().max()) / scale for k in ("a", "b"))
        lines.append(f"{name:32s} {ea:26.3e} {eb:30.3e}")
        if not eb <= 1.5 * ea + 2.0 ** -9:
            bad.append(name)
    table = "\n".join(lines)
    print("\n" + table)
    if os.environ.get("RDETR_ACCURACY_OUT"):
        with open(os.environ["RDETR_ACCURACY_OUT"], "w") as f:
            f.write("MultiScaleDeformableAttention, bf16, .train(), levels (56,76),(28,38),(14,19),(7,10), B = 2, mask on the tail of image 1;\n"
                    "worst |err| / max(1, max|ref|) against the same weights in fp32 on the materialised route\n" + table + "\n")
    assert not bad, f"new route less accurate than the [B,S,H,D] training route: {bad}\n{table}"
    assert not got["b"]["d/d value"][inputs[3].to(DEV)].any()         # nothing flows into the padded rows


def test_module_takes_the_head_major_route_only_where_it_applies(hm, monkeypatch):
    from relation_detr_amd import MultiScaleDeformableAttention, options
    calls = []
    real = hm.MultiScaleDeformableAttnHeadMajorFunction.apply
    monkeypatch.setattr(hm.MultiScaleDeformableAttnHeadMajorFunction, "apply", lambda *a: calls.append(1) or real(*a))

    def run(on, shapes=MODULE_SHAPES, dtype=BF, Nq=None, ref_dim=2, grad=True):
        with options.override(msda_train_fused=True, msda_train_head_major=on):
            mod = MultiScaleDeformableAttention().to(DEV).to(dtype).train()
        query, value, ref, mask, go, shp, start = _module_inputs(shapes, 1, Nq, ref_dim)
        before = len(calls)
        if not grad:
            with torch.no_grad():
                mod(query.to(DEV).to(dtype), ref.to(DEV), value.to(DEV).to(dtype), shp.to(DEV), start.to(DEV), mask.to(DEV))
            return len(calls) - before
        res = _run_module(mod, query, value, ref, mask, go, shp, start, dtype)
        assert all(t is not None and torch.isfinite(t.float()).all() for t in res.values())
        assert res["d/d value"].abs().max() > 0 and res["value_proj.weight"].abs().max() > 0
        return len(calls) - before

    assert run(False) == 0
    assert run(True) == 1
    assert run(True, grad=False) == 0                              # inference keeps the eval path
    assert run(True, dtype=torch.float32) == 0
    assert run(True, ref_dim=4) == 0
    assert run(True, Nq=900) == 0
    assert run(True, shapes=SHAPES4) == 0                          # S = 307 < 4,096
    assert len(calls) == 1
