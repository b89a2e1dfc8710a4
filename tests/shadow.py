"""Shadow checks of every kernel launch on a forward (or training step) of the stack.

``Shadow(monkeypatch)`` replaces the module-level functions of ``relation_detr_amd.ops`` with wrappers, and those of the four
training modules that call the library themselves (``ffn_train``, ``ln_train``, ``attn_rel_train``, ``msda_train_hm``).  Every call
site in transformer.py, ms_deform_attn.py, self_attn.py and relation.py looks the former up as ``ops.<name>``; the autograd
Functions in ops.py and in the training modules reach their entries through their own module's globals, so a wrapper sees every
launch of the stack, forward or training step, whichever opt-in training route is on.  A wrapper copies the tensor
arguments BEFORE the call (some entries work in place, some write ``out=`` slices of wider buffers), calls the kernel, then
computes a reference from the copies and RECORDS the result (op, call index, worst err / bound ratio, failing elements, where
the worst one is).  ``Shadow.report()`` prints the per-op table; ``Shadow.assert_ok()`` fails on any bad record.

Every function of ``ops`` is classified in ``KERNEL_ENTRIES`` (a checker each) or ``HOST_ONLY``, every function of the training
modules in ``TRAIN_ENTRIES`` (keyed "module.function", the op name of its records) or ``TRAIN_HOST_ONLY``; a call to a function in
neither is recorded as "kernel `<name>` ran without a shadow reference".  At the C boundary every launching ``rdetr_*`` symbol
of the library object is replaced by a counting tripwire that fails unless a checked entry is active (depth > 0), so no launch
can get past the harness through an unclassified helper.

Checkers are plain torch in float64 on the exact operand values the kernel read (bf16 values upcast), plus
``oracle.torch_ref`` for the MSDA core, the sampling locations and the relation bias.  Intermediates are rounded to bf16
exactly where the unfused route stores them.  A checker never calls ``ops`` or ``_lib``.  Every element is compared.

Bounds (err = |kernel - reference|; "exact" = bit equality; each from the unit test named):

  op                              bound                                            unit test
  ms_deform_attn_forward[_fused]  bf16: 2^-8 |ref| + 1e-3;  fp32: 1e-4             test_gpu_parity::test_msda_forward_bf16,
                                                                                   ::test_msda_fused_producer_matches_unfused
  value_to_head_major             exact                                            test_gpu_window::test_value_to_head_major
  value_proj_head_major           2^-8 |ref| + 1e-3                                test_gpu_window::test_value_projection_into_head_major
  encoder_proj                    2^-8 |ref| + 2e-3 (both outputs)                 test_gpu_glue::test_encoder_proj_matches_the_separate_projections
  linear_k256                     2^-8 |ref| + 2e-3                                test_gpu_glue::test_linear_k256_matches_fp32_reference
  ffn_k256                        2^-8 |ref| + 1.5e-2 (hidden rounded to bf16)     test_gpu_glue::test_ffn_k256_matches_unfused_reference
  linear_ln_k256                  2^-8 |ref| + 2^-5 + 1e-3 (projection rounded)    test_gpu_glue::test_linear_ln_k256_is_linear_then_add_layer_norm
                                                                                   (2^-5 to the composition) + add_layer_norm's bound
  ffn_ln_k256                     2^-8 |ref| + 2^-5 + 1e-3; pos output exact       test_gpu_glue::test_ffn_ln_k256_is_ffn_then_add_layer_norm
  add_layer_norm                  fp32: 2e-5;  bf16: 2^-8 |ref| + 1e-3;            test_gpu_glue::test_add_layer_norm_vs_torch,
                                  pos output exact (out + pos)                     ::test_add_layer_norm_second_output_is_the_separate_add
  relation_bias                   1e-4                                             test_gpu_parity::test_relation_bias_vs_oracle
  bias_softmax_                   2e-6                                             test_gpu_parity::test_bias_softmax_vs_torch
  relation_attention[_boxes]      2^-7 |ref| + 4e-3                                test_gpu_glue::test_relation_attention_vs_reference,
                                                                                   test_gpu_attn_rel (_close)
  _relation_attention_train       out as above; lse (natural log) 1e-3            test_gpu_attn_train::test_train_forward_is_the_inference_kernel_and_lse
  box_head_k256                   4e-3                                             test_gpu_glue::test_fused_box_head_matches_the_unfused_sequence
  query_pos_k256                  2^-7 max|ref|; query + pos exact                 test_gpu_glue::test_fused_query_pos_matches_the_unfused_sequence
  box_refine                      2e-6                                             test_gpu_glue::test_box_refine_vs_torch
  sine_pos_embed                  fp32: 5e-6;  bf16: 2^-8                          test_gpu_glue::test_sine_pos_embed_vs_torch
  decoder_reference               reference exact; embedding fp32 1e-5, bf16 2^-8  test_gpu_glue::test_decoder_entry_kernels_match_the_torch_sequences
  pyramid_points                  ratios / keep exact, reference 2e-7,             test_gpu_glue::test_pyramid_points_matches_the_torch_sequences
                                  logits 2e-6 (inf where the torch sequence has inf)
  tokens_from_levels, scaled_pos, exact                                            test_gpu_glue (tokens / decoder entry / zero_masked_rows /
  zero_masked_rows_, row_max,                                                      row_max / topk / detections tests)
  topk (values + tie order), detections_from_topk
  _relation_attention_backward    2^-7 |ref| + 2e-2 max|ref|, the row term         test_gpu_attn_train::_check_grad
                                  rowsum(dout * out) from the `out` it is handed
  relation_bias_backward          weight 1e-4 |ref| + 2e-3 sqrt(pairs) / 30,       test_gpu_parity::test_relation_bias_backward_kernel
                                  bias 1e-5 |ref| + 1e-3
  ms_deform_attn_backward         value / weights 1e-4 max(1, max|ref|);           test_gpu_msda_train_fused (close_abs, close_offsets)
                                  locations 1e-4 |ref| + 5e-4 away from kinks, at the
                                  fp32 pixel coordinates the kernel forms
  ms_deform_attn_backward_fused   fp32: as above;  bf16: 2^-8 |ref| + 1e-3 max(1, max|ref|),   test_gpu_msda_train_fused (close_bf16)
                                  offsets / reference points away from kinks

Training entries outside ops.py ("bf16 form" = 2^-8 |ref| + 1e-3 max(1, max|ref|) against the float64 value: the one rounding
to bf16 the kernel makes, plus its fp32 accumulation; tests/test_shadow_train_host.py holds the checkers themselves on the CPU):

  ffn_train.ffn_k256_train        out as ffn_k256;  hid = relu(x W1^T + b1): bf16 form          test_gpu_ffn_train (within_bf16_form)
  ffn_train.ffn_k256_backward     dH = dy W2 where the handed hid > 0: bf16 form, bit-zero     test_gpu_ffn_train::test_backward_kernel_rounding_points
                                  elsewhere;  dx = dH W1 from the RETURNED dH: bf16 form
  ln_train.add_layer_norm_train   out as add_layer_norm;  mean, rstd of x + residual:           test_gpu_ln_train (stats 1e-5)
                                  1e-5 max(1, |ref|) per row
  ln_train.add_layer_norm_backward  statistics recomputed in float64.  bf16: dx, dgamma, dbeta  test_gpu_ln_train::test_accuracy_against_float64
                                  bf16 form;  fp32: dx 1e-5 max(1, max|ref|), dgamma / dbeta
                                  (1e-6 + 4 2^-24 sqrt(rows)) max(1, max|ref|)
  attn_rel_train._relation_attention_boxes_train   out as relation_attention_boxes, lse as      test_gpu_attn_rel_train, test_gpu_attn_train
                                  _relation_attention_train
  attn_rel_train._relation_attention_boxes_backward   dq, dk, dv as _relation_attention_backward  test_gpu_attn_rel_train (_check_all, TAU)
                                  with the float64 relation bias;  grad_weight, grad_bias through
                                  the float64 ReLU: 2^-7 |ref| + 2e-2 max|ref| + sum |dS_ref| |feature|
                                  over the pairs with |pre-activation bias| < TAU = 8e-3 (the branch
                                  the bf16 sine features may switch); those pairs, over images and
                                  heads, at most 25 % of [N, M] and no complete row, or the call fails
  msda_train_hm.ms_deform_attn_backward_fused_hm   ms_deform_attn_backward_fused's checker and    test_gpu_msda_train_hm
                                  bf16 bounds on the [B,S,H,D] permutation of the value
  msda_train_hm.grad_value_from_head_major   exact (the torch expression of its docstring)       test_gpu_msda_train_hm
No constant was raised for the training step: profiles/r14/ has every entry's worst err / bound ratio there, all below 1.
"""
from __future__ import annotations

import collections
import dataclasses
import inspect
import math
from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle import torch_ref

# rdetr_* symbols that launch nothing (host helpers and sizes): everything else in _lib.SIGNATURES is under the tripwire
NON_LAUNCHING = ("rdetr_abi_version", "rdetr_status_string", "rdetr_msda_fast_path", "rdetr_msda_levels_window_ok")


def launching_symbols(signatures) -> List[str]:
    return sorted(n for n in signatures if n not in NON_LAUNCHING and not n.endswith("_workspace_bytes"))


def ops_functions(ops_module) -> List[str]:
    """Every module-level function defined in ops.py."""
    return sorted(n for n, f in vars(ops_module).items() if inspect.isfunction(f) and f.__module__ == ops_module.__name__)


# ------------------------------------------------------------------------------------------------------------ comparison
BF16 = torch.bfloat16


def _bf(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the bf16 value the unfused route stores -> float64."""
    return x.float().to(BF16).double()


def _d(t):
    return None if t is None else t.detach().double()


def _d64(t):
    return t if t is None or t.dtype == torch.float64 else t.detach().double()


def _sum(a, b, dtype):
    """a + b as torch computes it in ``dtype`` (bf16: fp32 arithmetic, one rounding to bf16; fp32: the rounded exact sum)."""
    if dtype == BF16:
        return (a.float() + b.float()).to(dtype)
    return (a.double() + b.double()).to(dtype)


@dataclasses.dataclass
class Cmp:
    label: str
    got: torch.Tensor
    ref: torch.Tensor
    bound: object = 0.0                      # tensor or scalar; 0 = exact (bit equality of the values)
    keep: Optional[torch.Tensor] = None      # bool: elements compared (others are kink points etc.)
    gate: bool = False                       # a condition of the check, not an error: fails like any Cmp, but while it holds
                                             # its ratio stays out of the record's worst err / bound


@dataclasses.dataclass
class Record:
    op: str
    call: int
    ratio: float
    failing: int
    checked: int
    where: str


def _compare(c: Cmp):
    got = c.got.detach().double()
    ref = c.ref.detach().double().to(got.device)
    if got.shape != ref.shape:
        return math.inf, got.numel(), got.numel(), f"{c.label}: shape {tuple(got.shape)} vs reference {tuple(ref.shape)}"
    both_nan = torch.isnan(got) & torch.isnan(ref)
    same_inf = torch.isinf(ref) & (got == ref)
    err = (got - ref).abs()
    bound = c.bound if torch.is_tensor(c.bound) else torch.full_like(err, float(c.bound))
    bound = bound.double().to(err.device).expand_as(err)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    ratio = torch.where(both_nan | same_inf, torch.zeros_like(ratio), ratio)
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    if c.keep is not None:
        ratio = torch.where(c.keep.to(ratio.device).expand_as(ratio), ratio, torch.zeros_like(ratio))
    checked = int(ratio.numel() if c.keep is None else c.keep.expand_as(ratio).sum().item())
    if ratio.numel() == 0:
        return 0.0, 0, 0, c.label
    flat = int(torch.argmax(ratio).item())
    worst = float(ratio.view(-1)[flat].item())
    failing = int((ratio > 1).sum().item())
    idx = []
    for s in reversed(ratio.shape):
        idx.append(flat % s)
        flat //= s
    idx = tuple(reversed(idx))
    where = f"{c.label}{list(idx)} of {list(ratio.shape)}: got {got[idx].item():.6g} ref {ref[idx].item():.6g}"
    return worst, failing, checked, where


# ------------------------------------------------------------------------------------------------------------- references
def _msda_core_chunked(value, shapes, loc, w, budget=1 << 29):
    """oracle.torch_ref.msda_core in query chunks (it stacks [B*H, D, Nq, L*P] samples)."""
    B, S, H, D = value.shape
    Nq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    step = max(1, budget // max(1, B * H * D * L * P * value.element_size()))
    return torch.cat([torch_ref.msda_core(value, shapes, loc[:, s:s + step], w[:, s:s + step]) for s in range(0, Nq, step)], 1)


def _shapes_cpu(spatial_shapes):
    return spatial_shapes.detach().cpu()


def _gather_bound(out_dtype, ref):
    return 2.0 ** -8 * ref.abs() + 1e-3 if out_dtype == BF16 else 1e-4


def _value_bshd(value, layout):
    v = _d(value)
    return v.permute(0, 2, 1, 3) if layout == "bhsd" else v


def chk_ms_deform_attn_forward(a, res):
    v = _value_bshd(a["value"], a["value_layout"])
    ref = _msda_core_chunked(v, _shapes_cpu(a["spatial_shapes"]), _d(a["sampling_loc"]), _d(a["attn_weight"]))
    return [Cmp("out", res, ref, _gather_bound(res.dtype, ref))]


def _fused_producer(value, shapes, offsets, logits, ref_pts, mask, layout):
    v = _value_bshd(value, layout)
    if mask is not None:
        v = v.masked_fill(mask.bool()[:, :, None, None], 0.0)
    B, Nq, H, L, P, _ = offsets.shape
    w = _d(logits).reshape(B, Nq, H, L * P).softmax(-1).view(B, Nq, H, L, P)
    loc = torch_ref.sampling_locations_from_reference(_d(ref_pts), _d(offsets), shapes.to(v.device).double(), P)
    return v, loc, w


def chk_ms_deform_attn_forward_fused(a, res):
    shapes = _shapes_cpu(a["spatial_shapes"])
    v, loc, w = _fused_producer(a["value"], shapes, a["sampling_offsets"], a["attn_logits"], a["reference_points"],
                                a["key_padding_mask"], a["value_layout"])
    ref = _msda_core_chunked(v, shapes, loc, w)
    return [Cmp("out", res, ref, _gather_bound(res.dtype, ref))]


def _head_major(x, mask):
    B, S, C = x.shape
    y = x.view(B, S, 8, C // 8)
    if mask is not None:
        y = y.masked_fill(mask.bool()[:, :, None, None], 0.0)
    return y.permute(0, 2, 1, 3)


def chk_value_to_head_major(a, res):
    return [Cmp("out", res, _head_major(_d(a["value"]), a["key_padding_mask"]))]


def _linear(x, w, b):
    y = _d(x) @ _d(w).t()
    return y if b is None else y + _d(b)


def chk_value_proj_head_major(a, res):
    ref = _head_major(_linear(a["x"], a["weight"], a["bias"]), a["key_padding_mask"])
    return [Cmp("out", res, ref, 2.0 ** -8 * ref.abs() + 1e-3)]


def chk_encoder_proj(a, res):
    hm = _head_major(_linear(a["x"], a["wv"], a["bv"]), a["key_padding_mask"])
    q = _linear(a["xq"], a["wq"], a["bq"])
    return [Cmp("value_hm", res[0], hm, 2.0 ** -8 * hm.abs() + 2e-3), Cmp("offsets_logits", res[1], q, 2.0 ** -8 * q.abs() + 2e-3)]


def chk_linear_k256(a, res):
    ref = _linear(a["x"], a["weight"], a["bias"])
    if a["relu"]:
        ref = ref.relu()
    return [Cmp("out", res, ref, 2.0 ** -8 * ref.abs() + 2e-3)]


def _ffn(x, w1, b1, w2, b2):
    return _linear(_bf(_linear(x, w1, b1).relu()), w2, b2)


def chk_ffn_k256(a, res):
    ref = _ffn(a["x"], a["w1"], a["b1"], a["w2"], a["b2"])
    return [Cmp("out", res, ref, 2.0 ** -8 * ref.abs() + 1.5e-2)]


def _layer_norm(s, w, b, eps):
    return F.layer_norm(s, (s.shape[-1],), _d(w), _d(b), eps)


def chk_ffn_ln_k256(a, res):
    x = _d(a["x"])
    ref = _layer_norm(x + _bf(_ffn(a["x"], a["w1"], a["b1"], a["w2"], a["b2"])), a["gamma"], a["beta"], a["eps"])
    out = res if a["pos"] is None else res[0]
    cmps = [Cmp("out", out, ref, 2.0 ** -8 * ref.abs() + 2.0 ** -5 + 1e-3)]
    if a["pos"] is not None:
        cmps.append(Cmp("out_plus_pos", res[1], _sum(out, a["pos"], out.dtype)))
    return cmps


def chk_linear_ln_k256(a, res):
    s = _d(a["residual"]) + _bf(_linear(a["x"], a["weight"], a["bias"]))
    ref = _layer_norm(s, a["gamma"], a["beta"], a["eps"])
    return [Cmp("out", res, ref, 2.0 ** -8 * ref.abs() + 2.0 ** -5 + 1e-3)]


def chk_add_layer_norm(a, res):
    x = a["x"]
    s = _d(x) if a["residual"] is None else _d(x) + _d(a["residual"])
    ref = _layer_norm(s, a["weight"].to(x.dtype), a["bias"].to(x.dtype), a["eps"])
    out = res if a["pos"] is None else res[0]
    bound = 2e-5 if x.dtype == torch.float32 else 2.0 ** -8 * ref.abs() + 1e-3
    cmps = [Cmp("out", out, ref, bound)]
    if a["pos"] is not None:
        cmps.append(Cmp("out_plus_pos", res[1], _sum(out, a["pos"], x.dtype)))
    return cmps


def chk_relation_bias(a, res):
    ref = torch_ref.relation_bias(_d(a["src_boxes"]), _d(a["tgt_boxes"]), _d(a["proj_weight"]), _d(a["proj_bias"]),
                                  a["num_pos_feats"], a["temperature"], a["scale"])
    return [Cmp("out", res, ref, 1e-4)]


def chk_bias_softmax_(a, res):
    s = _d(a["scores"])
    if a["bias"] is not None:
        s = s + _d(a["bias"])
    if a["mask"] is not None:
        s = s.masked_fill(a["mask"].bool(), float("-inf"))
    ref = s.softmax(-1)
    return [Cmp("probs", res, ref, 2e-6)]


def _attention(q, k, v, H, bias, mask, scale):
    """float64 softmax(Q K^T scale + bias) V per head -> (out [B,N,C], logits [B,H,N,M]).  float64 inputs are used as they are
    (the backward checker passes autograd leaves); anything else is detached and upcast."""
    q, k, v = _d64(q), _d64(k), _d64(v)
    B, N, C = q.shape
    M, D = k.shape[1], C // H
    s = q.view(B, N, H, D).transpose(1, 2) @ k.view(B, M, H, D).transpose(1, 2).transpose(-1, -2) * (D ** -0.5 if scale is None else scale)
    if bias is not None:
        s = s + _d64(bias).view(B, H, N, M)
    if mask is not None:
        s = s.masked_fill(mask.bool(), float("-inf"))
    out = (s.softmax(-1) @ v.view(B, M, H, D).transpose(1, 2)).transpose(1, 2).reshape(B, N, C)
    return out, s


def _attn_cmp(label, got, ref):
    return Cmp(label, got, ref, 2.0 ** -7 * ref.abs() + 4e-3)


def chk_relation_attention(a, res):
    ref, _ = _attention(a["q"], a["k"], a["v"], a["num_heads"], a["bias"], a["mask"], a["scale"])
    return [_attn_cmp("out", res, ref)]


def chk_relation_attention_boxes(a, res):
    bias = torch_ref.relation_bias(_d(a["src_boxes"]), _d(a["tgt_boxes"]), _d(a["proj_weight"]), _d(a["proj_bias"]),
                                   a["num_pos_feats"], a["temperature"], a["rel_scale"])
    ref, _ = _attention(a["q"], a["k"], a["v"], a["num_heads"], bias, a["mask"], a["scale"])
    return [_attn_cmp("out", res, ref)]


def chk__relation_attention_train(a, res):
    ref, s = _attention(a["q"], a["k"], a["v"], a["num_heads"], a["bias"], a["mask"], a["scale"])
    lse = torch.logsumexp(s, -1).reshape(-1, s.shape[2])
    return [_attn_cmp("out", res[0], ref), Cmp("lse", res[1].double() * math.log(2.0), lse, 1e-3)]


def _attention_backward64(a, bias):
    """The attention backward in float64 from the operands the kernel reads: P = softmax of the logits, dP = dout V^T, and the
    row term D = rowsum(dout * out) from the forward output `out` it is handed (bf16), as the flash-style backward defines it
    -- D from the exact output instead differs by the bf16 rounding of `out` times |dout|, which at full size, where the
    dq / dk of most rows are small against dP, is several times the bound.  -> ({dq, dk, dv}, dS [B,H,N,M])."""
    H, scale = a["num_heads"], a["scale"]
    q, k, v, out = _d(a["q"]), _d(a["k"]), _d(a["v"]), _d(a["out"])
    dout = a["dout"].to(BF16).double()                         # the kernel reads dout in bf16
    B, N, C = q.shape
    M, D = k.shape[1], C // H
    scale = D ** -0.5 if scale is None else scale
    heads = lambda t, n: t.view(B, n, H, D).transpose(1, 2)                                          # noqa: E731
    _, s = _attention(q, k, v, H, bias, a["mask"], scale)
    p = torch.nan_to_num(s.softmax(-1), nan=0.0)                                                      # fully masked rows: 0
    dp = heads(dout, N) @ heads(v, M).transpose(-1, -2)
    dterm = (heads(dout, N) * heads(out, N)).sum(-1, keepdim=True)
    ds = torch.where(p > 0, p * (dp - dterm), torch.zeros_like(p))                                   # a dead row's `out` is NaN
    refs = {"dq": (ds @ heads(k, M) * scale).transpose(1, 2).reshape(B, N, C),
            "dk": (ds.transpose(-1, -2) @ heads(q, N) * scale).transpose(1, 2).reshape(B, M, C),
            "dv": (p.transpose(-1, -2) @ heads(dout, N)).transpose(1, 2).reshape(B, M, C)}
    return refs, ds


def _attn_grad_bound(ref):
    return 2.0 ** -7 * ref.abs() + 2e-2 * ref.abs().max() + 1e-30


def chk__relation_attention_backward(a, res):
    refs, ds = _attention_backward64(a, a["bias"])
    refs["dbias"] = ds.reshape(-1, *ds.shape[2:]) if a["bias"] is not None and a["need_dbias"] else None
    cmps = []
    for name, got in zip(("dq", "dk", "dv", "dbias"), res[:4]):
        ref = refs[name]
        if ref is not None:
            cmps.append(Cmp(name, got, ref.reshape(got.shape), _attn_grad_bound(ref.reshape(got.shape))))
    return cmps


def chk_relation_bias_backward(a, res):
    src, tgt = _d(a["src_boxes"]), _d(a["tgt_boxes"])
    g = _d(a["grad_out"]) * a["active"].bool()
    B, Hh, N1, N2 = g.shape
    gw = torch.zeros(Hh, 4 * a["num_pos_feats"], dtype=torch.float64, device=g.device)
    for b in range(B):
        feat = torch_ref.sine_embed(torch_ref.box_rel_encoding(src[b:b + 1], tgt[b:b + 1]), a["num_pos_feats"], a["temperature"],
                                    a["scale"])[0]
        gw += torch.einsum("hij,ijc->hc", g[b], feat)
    gb = g.sum(dim=(0, 2, 3))
    scale = math.sqrt(B * N1 * N2)
    return [Cmp("grad_weight", res[0], gw, 1e-4 * gw.abs() + 2e-3 * scale / 30), Cmp("grad_bias", res[1], gb, 1e-5 * gb.abs() + 1e-3)]


def _kink_keep(loc, shapes):
    size = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(loc.device, torch.float64)       # (w, h) per level
    pix = loc * size.view(1, 1, 1, -1, 1, 2) - 0.5
    return (pix - pix.round()).abs() > 1e-3


def _msda_backward64(v, shapes, go, make_loc_w, leaves, budget=1 << 28):
    """float64 autograd through msda_core in query chunks; make_loc_w(s, e) -> (loc, w) of queries [s, e)."""
    B, S, H, D = v.shape
    loc_all = []
    Nq = go.shape[1]
    L, P = shapes.shape[0], 4
    step = max(1, budget // max(1, B * H * D * L * P * 8 * 3))
    for s in range(0, Nq, step):
        with torch.enable_grad():                              # checkers run under no_grad, and so does Function.backward
            loc, w = make_loc_w(s, s + step)
            out = torch_ref.msda_core(v, shapes, loc, w)
            out.backward(go[:, s:s + step])
        loc_all.append(loc.detach())
    return torch.cat(loc_all, 1)


def _abs_bound(ref):
    return 1e-4 * max(1.0, float(ref.abs().max())) if ref.numel() else 1e-4


def _kernel_pixel_loc(loc, shapes):
    """The locations the gather kernels actually sample: their pixel coordinate x = loc * w - 0.5 is formed in fp32 (two
    roundings, no FMA, csrc/msda_bwd.hip), mapped back to [0, 1] in float64 so that msda_core samples exactly there.  At the
    R50 level-0 width, fp32 pixel coordinates carry ~1e-5 px, which the location gradient (sampled value differences times
    the level size) turns into ~1e-3 absolute: several times the 5e-4 bound against float64 coordinates."""
    size = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(loc.device, torch.float32).view(1, 1, 1, -1, 1, 2)
    px = loc.float() * size - 0.5
    return (px.double() + 0.5) / size.double()


def chk_ms_deform_attn_backward(a, res):
    shapes = _shapes_cpu(a["spatial_shapes"])
    v = _d(a["value"]).requires_grad_(True)
    loc = _kernel_pixel_loc(a["sampling_loc"], shapes).requires_grad_(True)
    w = _d(a["attn_weight"]).requires_grad_(True)
    _msda_backward64(v, shapes, _d(a["grad_output"]), lambda s, e: (loc[:, s:e], w[:, s:e]), (v, loc, w))
    keep = _kink_keep(loc.detach(), shapes)
    return [Cmp("grad_value", res[0], v.grad, _abs_bound(v.grad)),
            Cmp("grad_loc", res[1], loc.grad, 1e-4 * loc.grad.abs() + 5e-4, keep),
            Cmp("grad_attn", res[2], w.grad, _abs_bound(w.grad))]


def chk_ms_deform_attn_backward_fused(a, res):
    shapes = _shapes_cpu(a["spatial_shapes"])
    v = _d(a["value"]).requires_grad_(True)
    off = _d(a["sampling_offsets"]).requires_grad_(True)
    lg = _d(a["attn_logits"]).requires_grad_(True)
    rp = _d(a["reference_points"]).requires_grad_(True)
    B, Nq, H, L, P, _ = off.shape

    def make(s, e):
        loc = torch_ref.sampling_locations_from_reference(rp[:, s:e], off[:, s:e], shapes.to(v.device).double(), P)
        return loc, lg[:, s:e].softmax(-1).view(B, -1, H, L, P)
    go = _d(a["grad_output"])
    loc = _msda_backward64(v, shapes, go, make, (v, off, lg, rp))
    keep = _kink_keep(loc, shapes)
    if a["value"].dtype == BF16:
        def bnd(ref):
            return 2.0 ** -8 * ref.abs() + 1e-3 * max(1.0, float(ref.abs().max()))
        cmps = [Cmp("grad_value", res[0], v.grad, bnd(v.grad)), Cmp("grad_offsets", res[1], off.grad, bnd(off.grad), keep),
                Cmp("grad_logits", res[2], lg.grad, bnd(lg.grad))]
        if res[3] is not None:
            cmps.append(Cmp("grad_ref", res[3], rp.grad, bnd(rp.grad), keep.all(2).all(-2).all(-1, keepdim=True)))
        return cmps
    cmps = [Cmp("grad_value", res[0], v.grad, _abs_bound(v.grad)),
            Cmp("grad_offsets", res[1], off.grad, 1e-4 * off.grad.abs() + 5e-4, keep),
            Cmp("grad_logits", res[2], lg.grad, _abs_bound(lg.grad))]
    if res[3] is not None:
        cmps.append(Cmp("grad_ref", res[3], rp.grad, 1e-4 * rp.grad.abs() + 5e-4, keep.all(2).all(-2).all(-1, keepdim=True)))
    return cmps


def _inverse_sigmoid(x, eps):
    x = x.clamp(0, 1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def chk_box_refine(a, res):
    ref = (_d(a["delta"]) + _inverse_sigmoid(_d(a["reference"]), a["eps"])).sigmoid()
    return [Cmp("out", res, ref, 2e-6)]


def _sine(pos, F_, temperature, scale):
    """get_sine_pos_embed(exchange_xy=True) in float64."""
    k = torch.arange(F_ // 2, dtype=torch.float64, device=pos.device)
    dim_t = temperature ** (k * 2 / F_)
    ang = pos.unsqueeze(-1) * scale / dim_t
    emb = torch.stack((ang.sin(), ang.cos()), -1).flatten(-2)
    return torch.cat((emb[..., 1:2, :], emb[..., 0:1, :], emb[..., 2:, :]), -2).flatten(-2)


def chk_sine_pos_embed(a, res):
    ref = _sine(_d(a["pos"]), a["num_pos_feats"], a["temperature"], a["scale"])
    return [Cmp("out", res, ref, 5e-6 if a["dtype"] == torch.float32 else 2.0 ** -8)]


def chk_zero_masked_rows_(a, res):
    return [Cmp("out", res, _d(a["x"]).masked_fill(a["mask"].bool().reshape(*a["x"].shape[:-1], 1), 0.0))]


def chk_row_max(a, res):
    return [Cmp("out", res, _d(a["x"]).max(-1)[0])]


def _mlp_bf16(x, layers, last_rounded=True):
    """nn.Linear chain with ReLU between, every output stored in bf16 (the unfused bf16 route)."""
    for i, l in enumerate(layers):
        x = _linear(x, l.weight, l.bias)
        if i + 1 < len(layers):
            x = x.relu()
        if i + 1 < len(layers) or last_rounded:
            x = _bf(x)
    return x


def chk_box_head_k256(a, res):
    ref_pts = _d(a["reference"])
    base = ref_pts if a["reference_is_logit"] else _inverse_sigmoid(ref_pts, a["eps"])
    cmps = []
    outs = (res,) if a["xb"] is None else res
    for label, x, got in zip(("boxes_a", "boxes_b"), (a["xa"], a["xb"]), outs):
        ref = (_mlp_bf16(x, a["layers"]) + base).sigmoid()
        cmps.append(Cmp(label, got, ref, 4e-3))
    return cmps


def chk_query_pos_k256(a, res):
    pos = _mlp_bf16(a["emb"], a["head_layers"])
    if a["scale_layers"] is not None:
        pos = _bf(pos * _mlp_bf16(a["query"], a["scale_layers"]))
    got_pos, qpp = res
    return [Cmp("query_pos", got_pos, pos, 2.0 ** -7 * float(pos.abs().max())),
            Cmp("query_plus_pos", qpp, _sum(a["query"], got_pos, BF16))]


def chk_topk(a, res):
    x = _d(a["x"])
    order = torch.sort(x, dim=1, descending=True, stable=True)
    k = a["k"]
    return [Cmp("values", res[0], order.values[:, :k]), Cmp("indices", res[1], order.indices[:, :k])]


def chk_detections_from_topk(a, res):
    score, idx, boxes, sizes, C = a["score"], a["index"], a["boxes"], a["image_sizes"], a["num_classes"]
    box_idx = torch.div(idx, C, rounding_mode="trunc")
    label = idx % C
    cx, cy, w, h = boxes.gather(1, box_idx.unsqueeze(-1).expand(-1, -1, 4)).unbind(-1)
    xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    img_h, img_w = sizes.to(xyxy.dtype).unbind(1)
    xyxy = xyxy * torch.stack([img_w, img_h, img_w, img_h], 1)[:, None, :]
    ref = torch.cat([xyxy, score.unsqueeze(-1).to(xyxy.dtype), label.unsqueeze(-1).to(xyxy.dtype)], -1)
    return [Cmp("detections", res, ref)]


def chk_scaled_pos(a, res):
    dt = a["a"].dtype
    pos = (a["a"].float() * a["scale"].float()).to(dt) if dt == BF16 else (_d(a["a"]) * _d(a["scale"])).to(dt)
    return [Cmp("pos", res[0], pos), Cmp("query_plus_pos", res[1], _sum(a["query"], pos, dt))]


def chk_decoder_reference(a, res):
    rp, vr = a["reference_points"], a["valid_ratios"]
    ref_in = (_d(rp)[:, :, None] * torch.cat([_d(vr), _d(vr)], -1)[:, None]).float()
    emb = _sine(ref_in[:, :, 0, :].double(), a["num_pos_feats"], a["temperature"], a["scale"])
    return [Cmp("ref_in", res[0], ref_in), Cmp("embedding", res[1], emb, 1e-5 if a["dtype"] == torch.float32 else 2.0 ** -8)]


def chk_pyramid_points(a, res):
    """The torch sequences the kernels replace (transformer.py level_misc / reference_and_proposals / encoder_output), with the
    valid ratio correctly rounded."""
    masks, pad = a["level_masks"], a["pad_mask"]
    ratios = []
    centre, size, index, prop = [], [], [], []
    dev = masks[0].device
    for lvl, m in enumerate(masks):
        _, h, w = m.shape
        # the quotient correctly rounded to fp32 (torch divides by a Python scalar through its reciprocal, 1 ulp off at w = 504)
        ratios.append(torch.stack([(~m[:, 0, :]).sum(1).double() / w, (~m[:, :, 0]).sum(1).double() / h], -1).float())
        ys, xs = torch.meshgrid(torch.arange(0.5, h + 0.5, device=dev), torch.arange(0.5, w + 0.5, device=dev), indexing="ij")
        centre.append(torch.stack((xs.reshape(-1), ys.reshape(-1)), -1))
        size.append(torch.tensor([w, h], dtype=torch.float32, device=dev).expand(h * w, 2))
        index.append(torch.full((h * w,), lvl, dtype=torch.int64, device=dev))
        prop.append(torch.full((h * w, 2), 0.05 * 2.0 ** lvl, dtype=torch.float32, device=dev))
    vr = torch.stack(ratios, 1)
    centre, size, index, prop = torch.cat(centre), torch.cat(size), torch.cat(index), torch.cat(prop)
    full = centre[None] / (vr[:, index] * size[None])
    reference = full[:, :, None] * vr[:, None]
    proposals = torch.cat([full, prop[None].expand(full.shape[0], -1, -1)], -1)
    valid = ((proposals > 0.01) & (proposals < 0.99)).all(-1, keepdim=True)
    logit = torch.log(_d(proposals) / (1 - _d(proposals)))
    pm = pad if pad is not None else torch.zeros(full.shape[:2], dtype=torch.bool, device=dev)
    logit = logit.masked_fill(pm.unsqueeze(-1) | ~valid, float("inf"))
    keep = ((~pm.unsqueeze(-1)) & valid).squeeze(-1).to(a["keep_dtype"])
    return [Cmp("valid_ratios", res[0], vr), Cmp("reference", res[1], reference, 2e-7), Cmp("proposal_logit", res[2], logit, 2e-6),
            Cmp("keep", res[3], keep)]


def chk_tokens_from_levels(a, res):
    parts = []
    for l, x in enumerate(a["levels"]):
        t = x.flatten(2).transpose(1, 2)
        if a["add_vecs"] is not None:
            t = _sum(t, a["add_vecs"][l].to(x.dtype), x.dtype)
        parts.append(t)
    return [Cmp("tokens", res, torch.cat(parts, 1))]


KERNEL_ENTRIES: Dict[str, Callable] = {
    "ms_deform_attn_forward": chk_ms_deform_attn_forward,
    "ms_deform_attn_forward_fused": chk_ms_deform_attn_forward_fused,
    "value_to_head_major": chk_value_to_head_major,
    "value_proj_head_major": chk_value_proj_head_major,
    "encoder_proj": chk_encoder_proj,
    "linear_k256": chk_linear_k256,
    "ffn_k256": chk_ffn_k256,
    "ffn_ln_k256": chk_ffn_ln_k256,
    "linear_ln_k256": chk_linear_ln_k256,
    "add_layer_norm": chk_add_layer_norm,
    "relation_bias": chk_relation_bias,
    "bias_softmax_": chk_bias_softmax_,
    "relation_attention": chk_relation_attention,
    "relation_attention_boxes": chk_relation_attention_boxes,
    "_relation_attention_train": chk__relation_attention_train,
    "_relation_attention_backward": chk__relation_attention_backward,
    "relation_bias_backward": chk_relation_bias_backward,
    "ms_deform_attn_backward": chk_ms_deform_attn_backward,
    "ms_deform_attn_backward_fused": chk_ms_deform_attn_backward_fused,
    "box_refine": chk_box_refine,
    "sine_pos_embed": chk_sine_pos_embed,
    "zero_masked_rows_": chk_zero_masked_rows_,
    "row_max": chk_row_max,
    "box_head_k256": chk_box_head_k256,
    "query_pos_k256": chk_query_pos_k256,
    "topk": chk_topk,
    "detections_from_topk": chk_detections_from_topk,
    "scaled_pos": chk_scaled_pos,
    "decoder_reference": chk_decoder_reference,
    "pyramid_points": chk_pyramid_points,
    "tokens_from_levels": chk_tokens_from_levels,
}

# functions of ops that launch nothing of their own (argument checks, routing predicates, level-table caches), plus the weight
# packers, which launch a re-layout only from inside a checked entry (the tripwire holds them to that; the consumer's check
# covers the packed copy), and the two public attention-training wrappers, whose one launch is the checked private entry
HOST_ONLY = frozenset({
    "_cptr", "_stream_ptr", "_require_device", "_require_contiguous", "host_levels", "check_levels", "levels_window_ok",
    "_host_level_arrays", "_msda_algo", "_resident_pays", "_value_dims", "_producer_row_stride", "msda_fast_path",
    "_mask_u8", "_producer_operand", "_check_fused_operands", "_msda_backward_buffers",
    "relation_bias_backward_supported", "_row_matrix", "_attention_rows", "_attention_operands", "_attention_grad_buffers", "_rows_view",
    "box_head_k256_supported", "query_pos_k256_supported", "encoder_proj_supported", "topk_supported", "linear_k256_supported",
    "ffn_k256_supported", "linear_ln_k256_supported",
    "_packed_k256", "_packed_k_halves", "_packed_query_proj", "ffn_k256_packed_weights",
    "relation_attention_train", "relation_attention_backward",
})


# ------------------------------------------------------------------------------ training entries outside ops.py
TRAIN_MODULES = ("ffn_train", "ln_train", "attn_rel_train", "msda_train_hm")
LN_EPS = 1e-5                    # add_layer_norm_backward takes no eps: every norm of the network keeps nn.LayerNorm's default
TAU = 8e-3                       # |pre-activation relation bias| below which the bf16 sine features may switch the ReLU branch


def train_functions(module) -> List[str]:
    """Every module-level function defined in one of the training modules, as "module.function"."""
    short = module.__name__.rsplit(".", 1)[-1]
    return sorted(f"{short}.{n}" for n, f in vars(module).items() if inspect.isfunction(f) and f.__module__ == module.__name__)


def _bf16_form(ref):
    """2^-8 |ref| (one rounding to bf16 of the float64 value) + 1e-3 max(1, max |ref|): tests/test_gpu_ffn_train.py::within_bf16_form"""
    return 2.0 ** -8 * ref.abs() + 1e-3 * max(1.0, float(ref.abs().max()) if ref.numel() else 1.0)


def chk_ffn_k256_train(a, res):
    out, hid = res
    ref_h = _linear(a["x"], a["w1"], a["b1"]).relu()
    return chk_ffn_k256(a, out) + [Cmp("hid", hid, ref_h, _bf16_form(ref_h))]


def chk_ffn_k256_backward(a, res):
    """dH against bf16(dy W2) where the handed hid > 0 and bit-zero elsewhere; dx = dH W1 from the dH the kernel RETURNED, so
    that a one-ulp difference in dH against the reference's own dH is not summed F times into dx."""
    dx, dh = res
    live = a["hid"] > 0
    ref_dh = a["dy"].to(BF16).double() @ _d(a["w2"])                    # the kernel reads dy in bf16
    ref_dx = _d(dh) @ _d(a["w1"])
    ref_dh = ref_dh * live
    return [Cmp("dH", dh, ref_dh, torch.where(live, _bf16_form(ref_dh), torch.zeros_like(ref_dh))), Cmp("dx", dx, ref_dx, _bf16_form(ref_dx))]


def _ln_stats64(x, residual, eps):
    s = _d(x) if residual is None else _d(x) + _d(residual)
    mean = s.mean(-1, keepdim=True)
    rstd = (s.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    return s, mean, rstd


def chk_add_layer_norm_train(a, res):
    out, stats = res
    _, mean, rstd = _ln_stats64(a["x"], a["residual"], a["eps"])
    mean, rstd = mean.reshape(-1), rstd.reshape(-1)
    return chk_add_layer_norm(dict(a, pos=None), out) + [
        Cmp("mean", stats[:, 0], mean, 1e-5 * mean.abs().clamp_min(1.0)), Cmp("rstd", stats[:, 1], rstd, 1e-5 * rstd.abs().clamp_min(1.0))]


def chk_add_layer_norm_backward(a, res):
    """float64 LayerNorm backward of x + residual with the statistics recomputed in float64 (not the handed fp32 ones)."""
    dx, dgamma, dbeta = res
    x = a["x"]
    s, mean, rstd = _ln_stats64(x, a["residual"], LN_EPS)
    dy = a["dy"].to(x.dtype).double()                                   # the kernel reads dy in x's dtype
    xhat = (s - mean) * rstd
    g = dy * _d(a["weight"]).reshape(-1)
    ref_dx = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    ref_dg, ref_db = (dy * xhat).reshape(-1, 256).sum(0), dy.reshape(-1, 256).sum(0)
    rows = x.numel() // 256
    if x.dtype == BF16:
        bx, bg, bb = _bf16_form(ref_dx), _bf16_form(ref_dg), _bf16_form(ref_db)
    else:
        top = lambda r: max(1.0, float(r.abs().max()))                                               # noqa: E731
        par = 1e-6 + 4 * 2.0 ** -24 * math.sqrt(rows)
        bx, bg, bb = 1e-5 * top(ref_dx), par * top(ref_dg), par * top(ref_db)
    cmps = [Cmp("dx", dx, ref_dx, bx)]
    if a["need_params"]:
        cmps += [Cmp("dgamma", dgamma.reshape(-1), ref_dg, bg), Cmp("dbeta", dbeta.reshape(-1), ref_db, bb)]
    else:
        assert dgamma is None and dbeta is None
    return cmps


def _relation_pre64(a):
    """float64 pre-activation relation bias [B,H,N,M] and the sine features [B,N,M,4F] it is projected from."""
    feat = torch_ref.sine_embed(torch_ref.box_rel_encoding(_d(a["src_boxes"]), _d(a["tgt_boxes"]), a["eps"]), a["num_pos_feats"],
                                a["temperature"], a["rel_scale"])
    H = a["num_heads"]
    pre = torch.einsum("bnmc,hc->bhnm", feat, _d(a["proj_weight"]).reshape(H, -1))
    if a["proj_bias"] is not None:
        pre = pre + _d(a["proj_bias"]).view(1, H, 1, 1)
    return pre, feat


def _boxes_bias64(a):
    return torch_ref.relation_bias(_d(a["src_boxes"]), _d(a["tgt_boxes"]), _d(a["proj_weight"]), _d(a["proj_bias"]),
                                   a["num_pos_feats"], a["temperature"], a["rel_scale"])


def chk__relation_attention_boxes_train(a, res):
    ref, s = _attention(a["q"], a["k"], a["v"], a["num_heads"], _boxes_bias64(a), a["mask"], a["scale"])
    lse = torch.logsumexp(s, -1).reshape(-1, s.shape[2])
    return [_attn_cmp("out", res[0], ref), Cmp("lse", res[1].double() * math.log(2.0), lse, 1e-3)]


def chk__relation_attention_boxes_backward(a, res):
    """dq, dk, dv as chk__relation_attention_backward with the float64 bias; grad_weight / grad_bias through the float64 ReLU.
    The kernels round the sine features to bf16, so a pair whose pre-activation bias lies within TAU of zero may take the other
    ReLU branch (tests/test_gpu_attn_rel_train.py).  The harness cannot mask the kernel's operands, so those pairs are not
    removed: the two parameter-gradient bounds get sum |dS_ref| |feature| over exactly those pairs, which caps what a switched
    branch can change.  The pairs must be at most 25 % of all and no complete row, or the call is recorded as failing."""
    refs, ds = _attention_backward64(a, _boxes_bias64(a))
    pre, feat = _relation_pre64(a)
    H = a["num_heads"]
    active, kink = pre > 0, pre.abs() < TAU
    gw = torch.einsum("bhnm,bnmc->hc", ds * active, feat)
    gb = (ds * active).sum(dim=(0, 2, 3))
    allow_w = torch.einsum("bhnm,bnmc->hc", ds.abs() * kink, feat.abs())
    allow_b = (ds.abs() * kink).sum(dim=(0, 2, 3))
    pairs = kink.any(0).any(0)                                                                        # [N, M]
    share = pairs.double().mean().reshape(1)
    full_rows = pairs.all(1).sum().double().reshape(1)
    cmps = [Cmp(n, got, refs[n].reshape(got.shape), _attn_grad_bound(refs[n].reshape(got.shape))) for n, got in zip(("dq", "dk", "dv"), res[:3])]
    cmps.append(Cmp("grad_weight", res[3].reshape(H, -1), gw, _attn_grad_bound(gw) + allow_w))
    if res[4] is not None:
        cmps.append(Cmp("grad_bias", res[4].reshape(-1), gb, _attn_grad_bound(gb) + allow_b))
    cmps += [Cmp("kink_pair_share", share, torch.zeros_like(share), 0.25, gate=True),
             Cmp("kink_complete_rows", full_rows, torch.zeros_like(full_rows), gate=True)]
    return cmps


def chk_ms_deform_attn_backward_fused_hm(a, res):
    """chk_ms_deform_attn_backward_fused on the [B,S,H,D] permutation of the value, grad_value permuted back: the module documents
    the other gradients as the bits of that entry."""
    b = dict(value=a["value_hm"].permute(0, 2, 1, 3).contiguous(), spatial_shapes=a["spatial_shapes"], sampling_offsets=a["sampling_offsets"],
             attn_logits=a["attn_logits"], reference_points=a["reference_points"], grad_output=a["grad_output"])
    return chk_ms_deform_attn_backward_fused(b, [res[0].permute(0, 2, 1, 3).contiguous(), res[1], res[2], res[3]])


def chk_grad_value_from_head_major(a, res):
    g = a["grad_hm"]
    B, _, S, _ = g.shape
    ref = g.permute(0, 2, 1, 3).reshape(B, S, 256).to(BF16)
    if a["key_padding_mask"] is not None:
        ref = ref.masked_fill(a["key_padding_mask"].bool()[..., None], 0)
    return [Cmp("out", res, ref)]


TRAIN_ENTRIES: Dict[str, Callable] = {
    "ffn_train.ffn_k256_train": chk_ffn_k256_train,
    "ffn_train.ffn_k256_backward": chk_ffn_k256_backward,
    "ln_train.add_layer_norm_train": chk_add_layer_norm_train,
    "ln_train.add_layer_norm_backward": chk_add_layer_norm_backward,
    "attn_rel_train._relation_attention_boxes_train": chk__relation_attention_boxes_train,
    "attn_rel_train._relation_attention_boxes_backward": chk__relation_attention_boxes_backward,
    "msda_train_hm.ms_deform_attn_backward_fused_hm": chk_ms_deform_attn_backward_fused_hm,
    "msda_train_hm.grad_value_from_head_major": chk_grad_value_from_head_major,
}

# the rest of the four modules: routing predicates and argument helpers that launch nothing; ffn_train._pack, which launches a
# re-layout only from inside a checked entry (as the ops packers); and the two public natural-log wrappers of attn_rel_train,
# whose one launch is the checked private entry
TRAIN_HOST_ONLY = frozenset({
    "ffn_train.ffn_train_supported", "ffn_train._pack", "ffn_train._aligned_rows",
    "ln_train._aligned", "ln_train._rows", "ln_train.add_layer_norm_train_supported", "ln_train._param", "ln_train._entry",
    "attn_rel_train._f32", "attn_rel_train.relation_attention_boxes_train", "attn_rel_train.relation_attention_boxes_backward",
    "msda_train_hm._merged_slices", "msda_train_hm.split_merged_projection",
})


# ----------------------------------------------------------------------------------------------------------------- harness
def _copy(x):
    if torch.is_tensor(x):
        return x.detach().clone()
    if isinstance(x, (list, tuple)) and any(torch.is_tensor(t) for t in x):
        return type(x)(_copy(t) for t in x)
    return x


class Shadow:
    """``Shadow(monkeypatch, fault=None, check=True)``; ``fault(name, call, bound_args, result, rerun) -> result`` may replace a
    kernel's result before the check (the harness's own fault-injection test).  ``check=False`` installs only the counting
    tripwires at the C boundary (``launches``): no wrapper, no reference, no error for a launch outside an entry."""

    def __init__(self, monkeypatch, fault: Optional[Callable] = None, check: bool = True):
        import importlib

        from relation_detr_amd import _lib, ops
        self.records: List[Record] = []
        self.calls: collections.Counter = collections.Counter()
        self.checked: collections.Counter = collections.Counter()
        self.errors: List[str] = []
        self.launches: collections.Counter = collections.Counter()
        self.depth = 0
        self.fault = fault
        self.check = check
        targets = [(ops, name, name, KERNEL_ENTRIES, HOST_ONLY) for name in ops_functions(ops)]
        for short in TRAIN_MODULES:
            module = importlib.import_module(f"relation_detr_amd.{short}")
            targets += [(module, key.split(".", 1)[1], key, TRAIN_ENTRIES, TRAIN_HOST_ONLY) for key in train_functions(module)]
        for module, attr, key, entries, host_only in targets if check else ():
            if key in host_only:
                continue
            fn = getattr(module, attr)
            monkeypatch.setattr(module, attr, self._checked(key, fn, entries[key]) if key in entries else self._unclassified(key, fn))
        lib = _lib.load()
        for sym in launching_symbols(_lib.SIGNATURES):
            monkeypatch.setattr(lib, sym, self._tripwire(sym, getattr(lib, sym)))

    def _tripwire(self, sym, fn):
        def wrapper(*args):
            self.launches[sym] += 1
            if self.check and self.depth <= 0:
                self.errors.append(f"{sym} launched outside any checked ops entry")
            return fn(*args)
        return wrapper

    def _unclassified(self, name, fn):
        def wrapper(*args, **kwargs):
            self.errors.append(f"kernel `{name}` ran without a shadow reference")
            return fn(*args, **kwargs)
        return wrapper

    def _checked(self, name, fn, checker):
        sig = inspect.signature(fn)

        def wrapper(*args, **kwargs):
            call = self.calls[name]
            self.calls[name] += 1
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            copies = {k: _copy(v) for k, v in bound.arguments.items()}
            self.depth += 1
            try:
                result = fn(*args, **kwargs)
                if self.fault is not None:
                    result = self.fault(name, call, bound.arguments, result, fn)
            finally:
                self.depth -= 1
            # the references are torch's own float64 operators, some of which have no deterministic variant (grid_sample's
            # backward): a step run under torch.use_deterministic_algorithms(True) is for the kernels, not for them
            strict, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
            torch.use_deterministic_algorithms(False)
            try:
                with torch.no_grad():
                    self._record(name, call, checker(copies, result))
            finally:
                torch.use_deterministic_algorithms(strict, warn_only=warn)
            return result
        return wrapper

    def _record(self, name, call, cmps):
        worst, failing, checked, where = 0.0, 0, 0, ""
        for c in cmps:
            r, f, n, w = _compare(c)
            failing += f
            checked += n
            if r >= worst and (f or not c.gate):
                worst, where = r, w
        self.checked[name] += checked
        self.records.append(Record(name, call, worst, failing, checked, where))

    # ---------------------------------------------------------------------------------------------------------- results
    def called(self) -> set:
        return {r.op for r in self.records}

    def failures(self) -> List[Record]:
        return [r for r in self.records if r.failing or not math.isfinite(r.ratio)]

    def report(self, title: str = "") -> str:
        by = collections.OrderedDict()
        for r in sorted(self.records, key=lambda r: r.op):
            by.setdefault(r.op, []).append(r)
        lines = [f"shadow checks: {title}", f"{'op':34s} {'calls':>6s} {'elements checked':>17s} {'max err/bound':>14s}  worst at"]
        for op, rs in by.items():
            w = max(rs, key=lambda r: r.ratio)
            lines.append(f"{op:34s} {len(rs):6d} {sum(r.checked for r in rs):17d} {w.ratio:14.4f}  call {w.call}: {w.where}")
        for e in sorted(set(self.errors)):
            lines.append("ERROR " + e)
        text = "\n".join(lines)
        print(text)
        return text

    def assert_ok(self, expected_ops=None):
        bad = self.failures()
        msgs = [f"{r.op} call {r.call}: {r.failing} elements over bound, worst ratio {r.ratio:.3g} at {r.where}" for r in bad[:20]]
        assert not self.errors, sorted(set(self.errors))
        assert not bad, "\n".join(msgs)
        assert all(self.checked[op] > 0 for op in self.called()), [op for op in self.called() if not self.checked[op]]
        if expected_ops is not None:
            assert self.called() == set(expected_ops), (sorted(self.called() - set(expected_ops)),
                                                        sorted(set(expected_ops) - self.called()))
