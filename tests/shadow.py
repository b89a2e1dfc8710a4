"""Shadow checks of every kernel launch on a forward (or training step) of the stack.

``Shadow(monkeypatch)`` replaces the module-level functions of ``relation_detr_amd.ops`` with wrappers, and those of the eleven
modules that call the library themselves: the training routes ``ffn_train``, ``ln_train``, ``attn_rel_train``, ``msda_train_hm`` and
``amp_train``, the rest of a detector's training step, ``neck``, ``denoising``, ``criterion`` and ``optim`` (there also the two
launching methods of ``FusedAdamW``, patched on the class), and what runs in front of the neck, in the subpackages:
``backbones.epilogue`` and ``frontend.images`` (TRAIN_MODULES names a module by its dotted path below the package, and that path
starts the op name of its records).  A wrapper is installed in the defining module AND wherever another module of the package holds
the same function object as a global: backbones/resnet.py binds ``stem_bn_relu_maxpool`` by name, and the ``__init__`` files re-export
entries; tests/test_shadow_complete.py holds from the source that every such binding is patched.  Every call
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
  relation_bias                   1e-4 + 4 2^-24 sum |(W_sin, W_cos)| |sine argument| test_gpu_parity::test_relation_bias_vs_oracle
                                  (relation_bias_bound: the fp32 rounding of the arguments)
  bias_softmax_                   2e-6 + 2^-22 max_row |logit| p  (bias_softmax_bound:   test_gpu_parity::test_bias_softmax_vs_torch
                                  the fp32 rounding of the logits)
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
                                  rowsum(dout * out) from the `out` it is handed;
                                  dv + 2^-9 P^T |dO|, dk + 2^-9 scale |dS|^T |Q|
                                  (attention_grad_rounding: P and dS in bf16)
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
  attn_rel_train._relation_attention_boxes_train   out as relation_attention_boxes, lse 1e-3 +  test_gpu_attn_rel_train, test_gpu_attn_train
                                  2^-9 sum_ch |W[h, ch]| (boxes_lse_bound: the bf16 sine features)
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

The detector step (tests/test_gpu_shadow_detector.py; "floor form" = max(4 e32, 2^-20 scale), e32 the error of the module's own
torch route run in fp32 on the same operands against the same route in float64, computed inside the checker, scale = max(1, |ref|)
unless said otherwise; the golden fixtures g10, g11, g12 pin those routes to the reference project):

  amp_train.add_layer_norm_mixed_train     out 2e-5 (add_layer_norm, fp32), mean / rstd 1e-5 max(1, |ref|)   test_gpu_amp_train::test_layernorm_kernels_against_float64
  amp_train.add_layer_norm_mixed_backward  the fp32 bounds of ln_train.add_layer_norm_backward; the bf16 dx    (the fp32 bounds of test_gpu_ln_train)
                                  is the rounding of the fp32 dx, exact
  amp_train.ffn_mixed_train       ffn_train.ffn_k256_train's on the operands rounded to bf16; x's rounding exact  test_gpu_amp_train (bits of the bf16 route),
  amp_train.ffn_mixed_backward    dH as ffn_train.ffn_k256_backward; fp32 dx (1e-6 + 4 2^-24 sqrt(F))            ::test_ffn_backward_keeps_dh_and_leaves_dx_unrounded,
                                  max(1, max|ref|) against float64 dH_returned @ bf16(w1); bf16 dx: bf16 form    ::test_function_gradients_against_fp64
  neck.group_norm_levels_forward  per tensor 4 max(torch's fp32 CPU GroupNorm's own error, 2^-23 max|ref|),      test_gpu_neck::test_group_norm_forward_and_backward_fp32,
  neck.group_norm_levels_backward + 2^-8 |ref| for a bf16 result; mean 4 2^-23 max(1, max|ref|); rstd the same   ::test_group_norm_bf16
                                  yardstick on itself; the backward's statistics recomputed in float64
  neck._masks_and_counts          exact                                                                          test_gpu_neck::test_masks_and_counts_are_exact
  neck._sine_pos_packed           5e-6 (+ 2^-8 |ref| in bf16) against float64 sin / cos of the fp32 argument     test_gpu_neck::test_position_encoding_at_every_pixel
  denoising.cdn_noise, .denoising_mask   exact (the numpy Philox restatement; the torch expression)              test_gpu_denoising
  denoising.cdn_queries_forward   labels and label queries exact; box queries floor form                         test_gpu_denoising (within)
  denoising.cdn_embed_backward    floor form, + 2^-8 |ref| in bf16                                               test_gpu_denoising::test_embedding_gradient
  criterion.match_cost            floor form, scale max(1, sum of the cost's term magnitudes) (match_cost_scale);  test_gpu_criterion::test_match_cost (within)
                                  padded columns exactly 0
  criterion.set_loss_forward      floor form: sums, dlogits per element (+ 2^-8 |ref| in bf16), the box          test_gpu_criterion::test_set_loss (within)
                                  gradients with the tensor's max|ref| as scale
  criterion.assign_match          device route only (the host route is scipy itself and is not recorded): per    test_gpu_assign::check_assignment
                                  row a valid assignment, total cost = scipy's optimum on the copied costs to
                                  1e-9 sum|chosen|, the denoising prefix the fixed pattern, status 0
  optim.FusedAdamW._clip_fused    total norm, coefficient: floor form, scale |ref|                               test_gpu_optim (docstring)
  optim.FusedAdamW._step_fused    floor form, gc = |g coef| with the coefficient that was armed: exp_avg scale   test_gpu_optim (docstring)
                                  max(|m_old|, gc); exp_avg_sq max(v_old, gc^2); param |p_old| + step_size
                                  (|m_old| + gc) / denom; tensors without a gradient keep their bits; step + 1
profiles/r23/ has the two report tables of the detector step (mixed precision with everything on, two steps; fp32 defaults), every
ratio below 1.  Three bounds that the composed step exceeded changed their FORM, in the unit test and here together, each for a scale the
earlier form lacked: relation_bias (relation_bias_bound), bias_softmax_ (bias_softmax_bound) and criterion.match_cost (match_cost_scale).

From the images (cases (d), (e), (f) of tests/test_gpu_shadow_detector.py and T4 of tests/test_gpu_dirty_shapes.py; the operands are the
wrapper's copies, so an in-place ``frozen_bn_act_forward(x, ..., out=x)`` is checked against what x held before the launch):

  backbones.epilogue.frozen_bn_act_forward   fp32: exact, x * s, + shift, + residual, relu as separate fp32 torch operators;     test_gpu_backbone (check_forward, bf16_slack)
                                  bf16: 2^-8 |ref| + 2^-20 (|x s| + |shift| + |res|) against float64
  backbones.epilogue.frozen_bn_act_backward  the mask from the y the call was handed: dres = dy where not (y <= 0), else 0, exact;   test_gpu_backbone::test_frozen_bn_act_backward
                                  dx = dres * s, fp32 exact (torch's fp32 product), bf16 2^-8 |ref|; dres None exactly when not asked for
  backbones.epilogue.stem_bn_relu_maxpool    fp32: exact, max_pool2d(relu(x * s + h), 3, 2, 1); bf16: 2^-8 |ref| + the forward's slack   test_gpu_backbone::test_stem_pool
                                  max-pooled
  frontend.images.batch_images    mask, sizes and padding (+0 to the bit) exact; uint8 sources by the near-tie rule (exact off the ties, one   test_gpu_images (check_batch),
                                  of three neighbouring table values on them, at most NEAR_TIE_SHARE = 2 % of the batch near ties or the call   test_images_host (the float64 filter,
                                  fails); float sources max(4 e32, 2^-20 max(1, |ref|)); copies exact; bf16 the rounding of the fp32 value       the near-tie rule)
profiles/r28/ has the report tables of those cases, every ratio below 1; no bound changed.

Elements a checker excludes (``Cmp.keep``: the kink points of the sampling-location gradients, the dead columns of a cost table) may
be inaccurate, never unwritten: a NaN or an infinity there that the reference lacks fails the record like any other element.
tests/test_gpu_dirty_shapes.py runs the harness at small ragged shapes with every uninitialised allocation filled with 0x00, 0xFF
and 0x42 first (tests/dirty.py); profiles/r26/ has those report tables.  Two bounds that its training step exceeded on clean memory
changed their FORM there, in the unit test and here together, for a scale the earlier form lacked: the dk and dv of the attention
backwards (attention_grad_rounding) and the log-sum-exp of the attention forward that generates its bias (boxes_lse_bound).

Where a call WRITES (``Shadow(monkeypatch, writes=True, guard=None)``; off by default, every test above runs as it did).  Everything
above checks what an entry returns; none of it notices a kernel that also writes memory it does not own.  With ``writes=True``
every checked call adds ONE MORE RECORD under the same op (``Record.kind == "writes"``; it fails the op like any bad record, and
the report gets a "writes" column), from three comparisons:
  operand bits    every tensor argument -- and every tensor inside a list, tuple or dict argument, the parameters of a module
                  argument, the parameters, gradients and state of an optimizer -- that the entry's write set does not name is
                  bit-identical to its copy from before the call.  Compared through an integer view of the element size: a NaN
                  equals itself, -0.0 differs from +0.0, a NaN with another payload differs.  An operand that overlaps a declared
                  one BY THE BYTE RANGE its elements span counts as written (``frozen_bn_act_forward(x, ..., out=x)``).
  outside a view  the whole storage of every declared operand is copied before the call; afterwards every byte of it that the
                  operand's elements do not address is unchanged: the other columns of ``tokens_from_levels(out=buffer[..., :d])``,
                  the rows around ``assign_match(out=match_dev[at:...])``.  Whole storages are copied, which is why this is opt-in
                  and stays with the small shapes of tests/test_gpu_write_sets.py.
  bands           with ``guard`` (the installed tests/guard.py), after each entry the bands of the buffers allocated inside it and of
                  the storages of its tensor operands; ``finish_bands()`` (``assert_ok`` calls it) checks every band once more
                  when the case ends, and damage in a buffer that was clean when its own entry returned is an error against
                  "a later launch", with the entry the buffer was allocated in.  The guard steps aside for the harness's own
                  allocations (copies, masks, the float64 references).
The ``WRITES`` rule: the table names, for EVERY checked entry, the parameters the call may write -- ``out``, ``scores`` of
``bias_softmax_``, ``x`` of ``zero_masked_rows_``, a dict key by its dotted name (``class_head.out``) -- and most entries get ``()``;
no wildcards; an entry without a rule is an error.  The two FusedAdamW methods, whose operands are not arguments, have a callable
that returns the allowed tensors from the snapshot.  The ``out`` that the two attention backwards REQUIRE is the saved forward
output, an operand: it is not in their write sets.  tests/test_shadow_complete.py holds the table complete.
What this cannot see: a write farther from an allocation than one band (2 MiB, the largest row tile of csrc/ times its widest row:
tests/guard.py has the derivation); a write into the payload of a tensor that is neither an operand of the call nor guarded (the
weights of a network built before the guard, torch's own results); a write that stores the value that was there; and memory that
does not come from a covered allocator.  profiles/r29/ has the tables of the composed cases: no entry wrote outside its set.
"""
from __future__ import annotations

import collections
import contextlib
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
    kind: str = "values"                     # "writes": the record Shadow(writes=True) adds per call (failing / checked in elements of
                                             # operands, bytes outside an out= view and bytes of guard bands)


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
        # an excluded element (a kink point) may be inaccurate, it may not be unwritten: a NaN or inf where the reference is finite
        # fails there too
        unwritten = ~torch.isfinite(got) & torch.isfinite(ref)
        ratio = torch.where(unwritten, torch.full_like(ratio, math.inf), ratio)
    checked = int(ratio.numel() if c.keep is None else c.keep.expand_as(ratio).sum().item())
    if ratio.numel() == 0:
        return 0.0, 0, 0, c.label
    flat = int(torch.argmax(ratio).item())
    worst = float(ratio.reshape(-1)[flat].item())              # reshape: a channels-last result is not viewable flat
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


def relation_bias_bound(src_boxes, tgt_boxes, proj_weight, num_pos_feats=16, temperature=10000.0, scale=100.0, eps=1e-5):
    """1e-4 + 4 2^-24 sum_(coord, k) sqrt(W_sin^2 + W_cos^2) |a|  per (image, head, pair), a the sine argument of (coord, k).

    The kernel follows the reference's fp32 operations: an argument a = RN(RN(e scale) / dim_t) of an fp32 logarithm e carries at
    most 4 2^-24 |a| of rounding (logf to one ulp, i.e. two half-ulps, and one half-ulp for each of the two operations).  A
    perturbation da moves W_sin sin a + W_cos cos a by da (W_sin cos a - W_cos sin a), at most |da| sqrt(W_sin^2 + W_cos^2).  A
    constant cannot hold that: the arguments reach 100 |log(1e-5)| = 1.2e3 for a box of no width, which the noised denoising
    queries of a real step do produce and the random boxes of the unit test (0.01 .. 0.5) do not, and the sum grows with the
    weights.  For the two size-ratio coordinates the kernel forms the angle per box (tables of log(w_i + eps) scale / dim_t,
    combined by the angle-difference identities), so their |a| is the sum of the two boxes'."""
    src = _d(src_boxes)
    tgt = src if tgt_boxes is None else _d(tgt_boxes)
    c1, s1, c2, s2 = src[..., :2], src[..., 2:], tgt[..., :2], tgt[..., 2:]
    dist = torch.log((c1[:, :, None, :] - c2[:, None, :, :]).abs() / (s1[:, :, None, :] + eps) + 1.0).abs()
    ratio = (torch.log(s1 + eps).abs()[:, :, None, :] + torch.log(s2 + eps).abs()[:, None, :, :])
    k = torch.arange(num_pos_feats // 2, dtype=torch.float64, device=src.device)
    per_coord = torch.cat([dist, ratio], -1) * scale                                                  # [B, N1, N2, 4]
    w = _d(proj_weight).reshape(proj_weight.shape[0], 4, num_pos_feats // 2, 2).pow(2).sum(-1).sqrt()  # per (head, coord, k)
    w = (w / temperature ** (k * 2 / num_pos_feats)).sum(-1)                                          # [H, 4]
    return 1e-4 + 4 * 2.0 ** -24 * torch.einsum("bnmc,hc->bhnm", per_coord, w)


def chk_relation_bias(a, res):
    ref = torch_ref.relation_bias(_d(a["src_boxes"]), _d(a["tgt_boxes"]), _d(a["proj_weight"]), _d(a["proj_bias"]),
                                  a["num_pos_feats"], a["temperature"], a["scale"])
    return [Cmp("out", res, ref, relation_bias_bound(a["src_boxes"], a["tgt_boxes"], a["proj_weight"], a["num_pos_feats"],
                                                     a["temperature"], a["scale"]))]


def bias_softmax_bound(logits, probs):
    """2e-6 + 2^-22 max_row |logit| p  per element, from the float64 logits (scores + bias, -inf where masked) and probabilities.

    The kernel rounds the sum scores + bias to fp32 and scales it to base 2 for the exponential: a logit l reaches the exponential
    with two roundings, |dl| <= 2 2^-24 |l|.  p_i = exp(l_i) / sum_j exp(l_j) moves by p_i (dl_i - sum_j p_j dl_j), at most
    2 p_i max |dl| = 2^-22 max |l| p_i.  The constant alone holds only while the logits stay small (the unit test's are below 20);
    the fp32 decoder of a synthetic-weight network hands over logits in the hundreds, where one fp32 ulp of a logit is already
    several 1e-6 of p.  The 2e-6 stays for the exponential's own error and the normalisation."""
    size = torch.where(torch.isfinite(logits), logits.abs(), torch.zeros_like(logits)).amax(-1, keepdim=True)
    return 2e-6 + 2.0 ** -22 * size * probs


def chk_bias_softmax_(a, res):
    s = _d(a["scores"])
    if a["bias"] is not None:
        s = s + _d(a["bias"])
    if a["mask"] is not None:
        s = s.masked_fill(a["mask"].bool(), float("-inf"))
    ref = s.softmax(-1)
    return [Cmp("probs", res, ref, bias_softmax_bound(s, torch.nan_to_num(ref, nan=0.0)))]


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
            "dv": (p.transpose(-1, -2) @ heads(dout, N)).transpose(1, 2).reshape(B, M, C),
            "rounding": attention_grad_rounding(p, ds, q, dout, H, scale)}
    return refs, ds


def _attn_grad_bound(ref):
    return 2.0 ** -7 * ref.abs() + 2e-2 * ref.abs().max() + 1e-30


def attention_grad_rounding(p, ds, q, dout, num_heads, scale):
    """The scale the dk and dv bounds lacked.  dV = P^T dO and dK = scale dS^T Q run on the matrix pipe with P and dS rounded to
    bf16, a relative error of up to 2^-9 per element, so whatever else the kernel does exactly
        |dv_kernel - dv| <= 2^-9 (P^T |dO|),    |dk_kernel - dk| <= 2^-9 scale (|dS|^T |Q|).
    Where the sums cancel -- a nearly flat softmax over 1,500 keys, as the hybrid pass of the ragged training step of
    tests/test_gpu_dirty_shapes.py has it, where max |dv| is 6e-5 and max |dk| 3e-6 -- max |ref| falls orders below these sums
    and 2e-2 max |ref| below that rounding.  (dq = scale dS K has the same term; no composition has needed it, so it keeps the
    narrower form.)  p, ds [B,H,N,M] float64, q [B,N,C], dout [B,N,C] -> {"dk", "dv"} [B,M,C]."""
    B, H, N, M = p.shape
    heads = lambda t: t.double().abs().view(B, N, num_heads, -1).transpose(1, 2)                      # noqa: E731
    back = lambda t: t.transpose(1, 2).reshape(B, M, -1)                                             # noqa: E731
    return {"dv": 2.0 ** -9 * back(p.transpose(-1, -2) @ heads(dout)),
            "dk": 2.0 ** -9 * scale * back(ds.abs().transpose(-1, -2) @ heads(q))}


def chk__relation_attention_backward(a, res):
    refs, ds = _attention_backward64(a, a["bias"])
    refs["dbias"] = ds.reshape(-1, *ds.shape[2:]) if a["bias"] is not None and a["need_dbias"] else None
    cmps = []
    for name, got in zip(("dq", "dk", "dv", "dbias"), res[:4]):
        ref = refs[name]
        if ref is not None:
            extra = refs["rounding"][name].reshape(got.shape) if name in refs["rounding"] else 0.0
            cmps.append(Cmp(name, got, ref.reshape(got.shape), _attn_grad_bound(ref.reshape(got.shape)) + extra))
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
# modules of the package, dotted below it ("backbones.epilogue" is relation_detr_amd/backbones/epilogue.py)
TRAIN_MODULES = ("ffn_train", "ln_train", "attn_rel_train", "msda_train_hm", "amp_train", "neck", "denoising", "criterion", "optim",
                 "backbones.epilogue", "frontend.images")
# classes whose methods (static ones too) are classified like module-level functions ("module.Class.method")
TRAIN_CLASSES = {"optim": ("FusedAdamW",), "backbones.epilogue": ("FrozenBNActFunction",), "frontend.images": ("ImagePreprocessor",)}
PACKAGE = "relation_detr_amd"
LN_EPS = 1e-5                    # add_layer_norm_backward takes no eps: every norm of the network keeps nn.LayerNorm's default
TAU = 8e-3                       # |pre-activation relation bias| below which the bf16 sine features may switch the ReLU branch


def train_functions(module) -> List[str]:
    """Every module-level function defined in one of the training modules, as "module.function"."""
    short = module_key(module)
    names = [f"{short}.{n}" for n, f in vars(module).items() if inspect.isfunction(f) and f.__module__ == module.__name__]
    for cls in TRAIN_CLASSES.get(short, ()):                   # and the methods of the classes named there, "module.Class.method"
        for n, f in vars(getattr(module, cls)).items():
            f = f.__func__ if isinstance(f, (staticmethod, classmethod)) else f
            if inspect.isfunction(f) and f.__module__ == module.__name__:
                names.append(f"{short}.{cls}.{n}")
    return sorted(names)


def module_key(module) -> str:
    """relation_detr_amd.backbones.epilogue -> "backbones.epilogue": the module's name below the package."""
    assert module.__name__.startswith(PACKAGE + "."), module.__name__
    return module.__name__[len(PACKAGE) + 1:]


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


def boxes_lse_bound(proj_weight, num_heads, rows):
    """1e-3 (the bound of the materialised-bias forward) + 2^-9 sum_ch |W[h, ch]| for a row of head h: the kernel rounds the 64
    sine features, each within [-1, 1], to bf16, so the bias it generates for a pair is off by up to that sum, and the row's
    log-sum-exp moves by at most the largest bias error of its pairs.  With Conv2d's default initialisation (|W| <= 1/8) the sum
    is at most 7.8e-3, the TAU of tests/test_gpu_attn_rel_train.py; weights of another scale move it with them, which the
    constant alone did not.  -> [B * H, N] for `rows` = B * H rows."""
    per_head = 1e-3 + 2.0 ** -9 * _d(proj_weight).reshape(num_heads, -1).abs().sum(1)
    return per_head.repeat(rows // num_heads)[:, None]


def chk__relation_attention_boxes_train(a, res):
    ref, s = _attention(a["q"], a["k"], a["v"], a["num_heads"], _boxes_bias64(a), a["mask"], a["scale"])
    lse = torch.logsumexp(s, -1).reshape(-1, s.shape[2])
    bound = boxes_lse_bound(a["proj_weight"], a["num_heads"], lse.shape[0]).expand_as(lse)
    return [_attn_cmp("out", res[0], ref), Cmp("lse", res[1].double() * math.log(2.0), lse, bound)]


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
    cmps = [Cmp(n, got, refs[n].reshape(got.shape), _attn_grad_bound(refs[n].reshape(got.shape)) + (refs["rounding"][n].reshape(got.shape) if n in refs["rounding"] else 0.0))
            for n, got in zip(("dq", "dk", "dv"), res[:3])]
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


# ------------------------------------------------------------------- the detector step: amp_train, neck, denoising, criterion, optim
FLOOR = 2.0 ** -20               # 8 fp32 ulps of the scale: tests/test_gpu_criterion.py, test_gpu_denoising.py, test_gpu_optim.py
GN_EPS = 1e-5                    # group_norm_levels_backward takes no eps: every GroupNorm of the neck keeps nn.GroupNorm's default
F32, F64 = torch.float32, torch.float64


def _floor_cmp(label, got, ref64, ref32, scale, rel=0.0, keep=None):
    """|got - ref64| <= max(4 e32, 2^-20 scale) + rel |ref64|, e32 = |ref32 - ref64| the fp32 torch route's own error."""
    ref64 = ref64.detach().double()
    e32 = (ref32.detach().double().to(ref64.device) - ref64).abs()
    scale = scale if torch.is_tensor(scale) else torch.full_like(ref64, float(scale))
    return Cmp(label, got, ref64, torch.maximum(4 * e32, FLOOR * scale.double().to(ref64.device)) + rel * ref64.abs(), keep)


def _within(label, got, ref64, ref32, floor_scale="element", rel=0.0, keep=None):
    """tests/test_gpu_criterion.py::within: the floor's scale is max(1, |checker|), per element or of the whole tensor."""
    r = ref64.detach().double().abs()
    scale = r if floor_scale == "element" or not r.numel() else r.max().expand_as(r)
    return _floor_cmp(label, got, ref64, ref32, scale.clamp(min=1.0), rel, keep)


def _rb(t):
    return None if t is None else t.detach().to(BF16)


def chk_add_layer_norm_mixed_train(a, res):
    """out (fp32) as add_layer_norm's fp32 bound, mean / rstd as ln_train.add_layer_norm_train, on the float64 sum of the stored operands."""
    out, stats = res
    s, mean, rstd = _ln_stats64(a["x"], a["residual"], a["eps"])
    ref = _layer_norm(s, a["weight"], a["bias"], a["eps"])
    mean, rstd = mean.reshape(-1), rstd.reshape(-1)
    return [Cmp("out", out, ref, 2e-5), Cmp("mean", stats[:, 0], mean, 1e-5 * mean.abs().clamp_min(1.0)),
            Cmp("rstd", stats[:, 1], rstd, 1e-5 * rstd.abs().clamp_min(1.0))]


def chk_add_layer_norm_mixed_backward(a, res):
    """The fp32 bounds of ln_train.add_layer_norm_backward on the fp32 dx; the bf16 dx is the rounding of the fp32 one (exact where
    both are returned, else the fp32 bound + 2^-8 |ref|)."""
    dx, dxb, dgamma, dbeta = res
    x = a["x"]
    s, mean, rstd = _ln_stats64(x, a["residual"], LN_EPS)
    dy = a["dy"].float().double()
    xhat = (s - mean) * rstd
    g = dy * _d(a["weight"]).reshape(-1)
    ref_dx = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    ref_dg, ref_db = (dy * xhat).reshape(-1, 256).sum(0), dy.reshape(-1, 256).sum(0)
    top = lambda r: max(1.0, float(r.abs().max()) if r.numel() else 1.0)                               # noqa: E731
    par = 1e-6 + 4 * 2.0 ** -24 * math.sqrt(x.numel() // 256)
    cmps = []
    if dx is not None:
        cmps.append(Cmp("dx", dx, ref_dx, 1e-5 * top(ref_dx)))
    if dxb is not None:
        cmps.append(Cmp("dx_bf16", dxb, dx.to(BF16)) if dx is not None else
                    Cmp("dx_bf16", dxb, ref_dx, 1e-5 * top(ref_dx) + 2.0 ** -8 * ref_dx.abs()))
    assert cmps, "add_layer_norm_mixed_backward returned no dx"
    if a["need_params"]:
        cmps += [Cmp("dgamma", dgamma.reshape(-1), ref_dg, par * top(ref_dg)), Cmp("dbeta", dbeta.reshape(-1), ref_db, par * top(ref_db))]
    else:
        assert dgamma is None and dbeta is None
    return cmps


def chk_ffn_mixed_train(a, res):
    """ffn_train.ffn_k256_train's checker on the operands rounded to bf16 (the kernel rounds them as it loads); the third result is
    x's rounding itself, exact."""
    out, hid, xlp = res
    b = dict(x=_rb(a["x"]), w1=_rb(a["w1"]), b1=_rb(a["b1"]), w2=_rb(a["w2"]), b2=_rb(a["b2"]))
    return chk_ffn_k256_train(b, (out, hid)) + [Cmp("x_bf16", xlp, b["x"])]


def chk_ffn_mixed_backward(a, res):
    """ffn_train.ffn_k256_backward's checker on the weights rounded to bf16.  The unrounded fp32 dx: (1e-6 + 4 2^-24 sqrt(F))
    max(1, max |ref|) against float64 dH_returned @ bf16(w1), the running-sum form of tests/test_gpu_amp_train.py."""
    cmps = chk_ffn_k256_backward(dict(dy=a["dy"], hid=a["hid"], w1=_rb(a["w1"]), w2=_rb(a["w2"])), res)
    if a["fp32_dx"]:
        ref = cmps[1].ref
        cmps[1].bound = (1e-6 + 4 * 2.0 ** -24 * math.sqrt(a["w1"].shape[0])) * max(1.0, float(ref.abs().max()) if ref.numel() else 1.0)
    return cmps


# -- neck: torch's own GroupNorm on the CPU, float64 and fp32, as tests/test_gpu_neck.py::cpu_group_norm
def _cpu_group_norm(xs, ws, bs, gos, G, eps, dtype):
    out = []
    for i, (x, w, b) in enumerate(zip(xs, ws, bs)):
        with torch.enable_grad():
            x, w, b = (t.detach().cpu().to(dtype).requires_grad_() for t in (x, w, b))
            y = F.group_norm(x, G, w, b, eps)
            if gos is not None:
                y.backward(gos[i].detach().cpu().to(dtype))
        out.append((y.detach(), x.grad, w.grad, b.grad))
    return out


def _yardstick(ref64, cpu32):
    """tests/test_gpu_neck.py::yardstick_bound: 4 max(torch's fp32 CPU kernel's own error, 2^-23 max |ref|), per tensor."""
    own = float((cpu32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    return 4.0 * max(own, 2.0 ** -23 * (float(ref64.abs().max()) if ref64.numel() else 0.0))


def _group_stats(xs, G, eps, dtype):
    """mean, rstd [L, B, G] of the levels as ``dtype`` arithmetic of torch on the CPU gives them."""
    B = xs[0].shape[0]
    flat = [x.detach().cpu().to(dtype).reshape(B, G, -1) for x in xs]
    return torch.stack([f.mean(-1) for f in flat]), torch.stack([(f.var(-1, unbiased=False) + eps).rsqrt() for f in flat])


def chk_group_norm_levels_forward(a, res):
    ys, mean, rstd = res
    G, eps, xs = a["num_groups"], a["eps"], a["xs"]
    ref64 = _cpu_group_norm(xs, a["weights"], a["biases"], None, G, eps, F64)
    cpu32 = _cpu_group_norm(xs, a["weights"], a["biases"], None, G, eps, F32)
    cmps = []
    for l, y in enumerate(ys):
        r = ref64[l][0]
        cmps.append(Cmp(f"y{l}", y, r, _yardstick(r, cpu32[l][0]) + (2.0 ** -8 * r.abs() if y.dtype == BF16 else 0.0)))
    m64, r64 = _group_stats(xs, G, eps, F64)
    _, r32 = _group_stats(xs, G, eps, F32)
    cmps.append(Cmp("mean", mean, m64, 4 * 2.0 ** -23 * max(1.0, float(m64.abs().max()))))
    cmps.append(Cmp("rstd", rstd, r64, _yardstick(r64, r32)))
    return cmps


def chk_group_norm_levels_backward(a, res):
    """The statistics are recomputed in float64 from the levels (not the handed fp32 ones): what the forward launch handed over is
    part of what is checked."""
    dxs, dgamma, dbeta = res
    G, xs = a["num_groups"], a["xs"]
    zeros = [torch.zeros_like(w) for w in a["weights"]]
    ref64 = _cpu_group_norm(xs, a["weights"], zeros, a["grads"], G, GN_EPS, F64)
    cpu32 = _cpu_group_norm(xs, a["weights"], zeros, a["grads"], G, GN_EPS, F32)
    cmps = []
    for l, dx in enumerate(dxs):
        r = ref64[l][1]
        cmps.append(Cmp(f"dx{l}", dx, r, _yardstick(r, cpu32[l][1]) + (2.0 ** -8 * r.abs() if dx.dtype == BF16 else 0.0)))
        cmps.append(Cmp(f"dgamma{l}", dgamma[l], ref64[l][2], _yardstick(ref64[l][2], cpu32[l][2])))
        cmps.append(Cmp(f"dbeta{l}", dbeta[l], ref64[l][3], _yardstick(ref64[l][3], cpu32[l][3])))
    return cmps


def _cpu_masks(mask, level_hw):
    fm = mask.detach().cpu().float()
    masks = [F.interpolate(fm[None], size=tuple(hw))[0].to(torch.bool) for hw in level_hw]
    return masks, [(~m).int().cumsum(1, dtype=torch.int32) for m in masks], [(~m).int().cumsum(2, dtype=torch.int32) for m in masks]


def chk__masks_and_counts(a, res):
    masks, cum = res
    want, ys, xs = _cpu_masks(a["mask"], a["level_hw"])
    packed = torch.cat([t.reshape(-1) for t in (*ys, *xs)])
    return [Cmp(f"mask{l}", m, want[l]) for l, m in enumerate(masks)] + [Cmp("counts", cum, packed)]


def chk__sine_pos_packed(a, res):
    """float64 sin / cos of the fp32 argument, rebuilt on the CPU with the reference's single fp32 operations
    (tests/test_gpu_neck.py::pos_reference): 5e-6, + 2^-8 |ref| in bf16."""
    B, level_hw = a["B"], [tuple(int(v) for v in hw) for hw in a["level_hw"]]
    cum = a["cum"].detach().cpu()
    total, off, cmps = cum.numel() // 2, 0, []
    dim_t = a["dim_t"].detach().cpu()
    for l, (h, w) in enumerate(level_hw):
        n = B * h * w
        y, x = cum[off:off + n].view(B, h, w), cum[total + off:total + off + n].view(B, h, w)
        off += n
        if a["normalize"]:
            ye = (y + a["offset"]) / (y[:, -1:, :] + a["eps"]) * a["scale"]
            xe = (x + a["offset"]) / (x[:, :, -1:] + a["eps"]) * a["scale"]
        else:
            ye, xe = y + a["offset"], x + a["offset"]
        assert ye.dtype == F32
        ax, ay = (xe.unsqueeze(-1) / dim_t).double(), (ye.unsqueeze(-1) / dim_t).double()
        px = torch.stack((ax.sin(), ax.cos()), -1).flatten(-2)
        py = torch.stack((ay.sin(), ay.cos()), -1).flatten(-2)
        ref = torch.cat((py, px), 3).permute(0, 3, 1, 2)
        cmps.append(Cmp(f"pos{l}", res[l], ref, 5e-6 + (2.0 ** -8 * ref.abs() if res[l].dtype == BF16 else 0.0)))
    return cmps


# -- denoising
def _denoising():
    from relation_detr_amd import denoising
    return denoising


def chk_cdn_noise(a, res):
    want = _denoising()._noise_numpy(int(a["key"]), int(a["Q"]), int(a["num_classes"]))
    return [Cmp(n, got, torch.from_numpy(w)) for n, got, w in zip(("label_u", "label_r", "box_sign", "box_u"), res, want)]


chk_cdn_noise.applies = lambda a: torch.device(a["device"]).type == "cuda"


def chk_denoising_mask(a, res):
    return [Cmp("mask", res, _denoising().denoising_mask(a["groups"], a["group_size"], a["num_queries"], "cpu", fused=False))]


chk_denoising_mask.applies = lambda a: bool(a["fused"]) and torch.device(a["device"]).type == "cuda"


def chk_cdn_queries_forward(a, res):
    """Noised labels and label queries (copies of embedding rows) exact; the box queries against the module's torch route in
    float64, max(4 e32, 2^-20 max(1, |ref|)) (tests/test_gpu_denoising.py)."""
    dn = _denoising()
    label_query, box_query, noised = res
    counts, groups = [int(c) for c in a["counts"]], int(a["groups"])
    noise, dev = a["noise"], a["embed"].device
    if noise is None:
        noise = tuple(torch.from_numpy(x).to(dev) for x in dn._noise_numpy(int(a["key"]), 2 * groups * sum(counts), a["embed"].shape[0]))
    run = lambda boxes: dn._cdn_queries_torch(a["embed"].detach(), a["gt_labels"], boxes, counts, groups,       # noqa: E731
                                              float(a["label_noise_prob"]), float(a["box_noise_scale"]), noise)
    lq64, bq64, lab64 = run(a["gt_boxes"].double())
    _, bq32, _ = run(a["gt_boxes"].float())
    return [Cmp("noised_label", noised, lab64), Cmp("label_query", label_query, lq64), _within("box_query", box_query, bq64, bq32)]


def chk_cdn_embed_backward(a, res):
    grad, labels = a["grad_label_query"], a["noised_label"]
    used = labels >= 0
    index = labels[used].long()
    d = grad.shape[-1]
    ref64 = torch.zeros(a["num_classes"], d, dtype=F64, device=grad.device).index_add_(0, index, grad[used].double())
    ref32 = torch.zeros(a["num_classes"], d, dtype=F32, device=grad.device).index_add_(0, index, grad[used].float())
    return [_within("grad_embed", res, ref64, ref32, rel=0.0 if grad.dtype == F32 else 2.0 ** -8)]


# -- criterion
def _criterion():
    from relation_detr_amd import criterion
    return criterion


def _match_cost_route(a, dtype):
    crit = _criterion()
    logits, boxes = a["logits"].detach().to(dtype), a["boxes"].detach().to(dtype)
    R, N, _ = logits.shape
    B, Gmax = a["gt_labels"].shape
    counts = a["gt_count"].tolist()
    cost = torch.zeros(R, N, Gmax, dtype=dtype, device=logits.device)
    terms = torch.zeros_like(cost)
    live = torch.zeros(R, 1, Gmax, dtype=torch.bool, device=logits.device)
    for r in range(R):
        g = min(max(int(counts[r % B]), 0), Gmax)
        live[r, :, :g] = True
        if g:
            gt_b, gt_l = a["gt_boxes"][r % B, :g].to(dtype), a["gt_labels"][r % B, :g]
            cost[r, :, :g] = crit._image_cost(logits[r], boxes[r], gt_b, gt_l, a["cost_class"], a["cost_bbox"], a["cost_giou"], a["alpha"],
                                              a["gamma"])
            # the magnitudes of what _image_cost adds up: both focal terms of the class cost, the L1 distance, the GIoU
            prob = logits[r].sigmoid()
            neg = (1 - a["alpha"]) * prob ** a["gamma"] * (1 - prob + 1e-6).log().abs()
            pos = a["alpha"] * (1 - prob) ** a["gamma"] * (prob + 1e-6).log().abs()
            valid = ((gt_l >= 0) & (gt_l < logits.shape[-1])).to(dtype)
            lab = gt_l.clamp(0, logits.shape[-1] - 1).long()
            giou = crit.generalized_box_iou(crit.box_cxcywh_to_xyxy(boxes[r]), crit.box_cxcywh_to_xyxy(gt_b)).abs()
            terms[r, :, :g] = (a["cost_class"] * (pos[:, lab] + neg[:, lab]) * valid + a["cost_bbox"] * torch.cdist(boxes[r], gt_b, p=1)
                               + a["cost_giou"] * giou)
    return cost, live, terms


def match_cost_scale(a):
    """The floor's scale of a match cost: cost_class (|pos| + |neg|) + cost_bbox L1 + cost_giou |GIoU| per element, in float64.
    The cost is the SIGNED sum of those terms and each carries the fp32 rounding of its own magnitude (the class cost alone is
    the difference of two focal terms that reach 0.75 * 13.8 at a saturated logit), so an element where they cancel keeps the
    rounding of the large ones: 8 fp32 ulps of the result itself, the floor's first form, held on the unit test's random stacks
    and not on the proposals of a real step -- the reason tests/test_gpu_criterion.py already gives for the box gradients."""
    return _match_cost_route(a, F64)[2]


def chk_match_cost(a, res):
    """The module's torch route in float64 (tests/test_gpu_criterion.py::test_match_cost); columns at or beyond an image's count are
    exactly 0."""
    ref64, live, terms = _match_cost_route(a, F64)
    ref32 = _match_cost_route(a, F32)[0]
    live = live.expand_as(ref64)
    return [_floor_cmp("cost", res, ref64, ref32, terms.clamp(min=1.0), keep=live), Cmp("padded_columns", res, torch.zeros_like(ref64), keep=~live)]


chk_match_cost.applies = lambda a: bool(a["fused"]) and a["logits"].is_cuda


def _set_loss_route(a, dtype):
    crit = _criterion()
    with torch.enable_grad():
        x = a["logits"].detach().to(dtype).requires_grad_(True)
        b = a["boxes"].detach().to(dtype).requires_grad_(True)
        sums = crit._set_loss_torch(x, b, a["match"], a["gt_boxes"].to(dtype), a["gt_labels"], int(a["n_split"]), a["inv_norm_a"],
                                    a["inv_norm_b"], a["alpha"], a["gamma"])
        dlogits, = torch.autograd.grad(sums[..., 0].sum(), x, retain_graph=True)
        dl1, = torch.autograd.grad(sums[..., 1].sum(), b, retain_graph=True)
        dgiou, = torch.autograd.grad(sums[..., 2].sum(), b)
    return sums.detach(), dlogits, dl1, dgiou


def chk_set_loss_forward(a, res):
    """tests/test_gpu_criterion.py::test_set_loss: sums and dlogits per element (bf16 dlogits + 2^-8 |ref|), the box gradients with
    the tensor's max |ref| in the floor."""
    c64, c32 = _set_loss_route(a, F64), _set_loss_route(a, F32)
    sums, dlogits, dl1, dgiou = res
    return [_within("sums", sums, c64[0], c32[0]), _within("dlogits", dlogits, c64[1], c32[1], rel=0.0 if dlogits.dtype == F32 else 2.0 ** -8),
            _within("dbox_l1", dl1, c64[2], c32[2], floor_scale="tensor"), _within("dbox_giou", dgiou, c64[3], c32[3], floor_scale="tensor")]


def chk_assign_match(a, res):
    """The device matcher as tests/test_gpu_assign.py checks it, without asking for scipy's table (ties): per row, the table is a valid
    assignment over the image's count, its total cost on the copied costs is scipy's optimum to 1e-9 of the sum of magnitudes, the
    denoising prefix is the fixed pattern and status is 0.  One compared element per row and property."""
    import numpy as np
    crit = _criterion()
    match, status = res
    cost = a["cost"].detach().cpu()
    R, N, Gmax = cost.shape
    counts, repeat, skip = [int(c) for c in a["gt_count"].tolist()], int(a["repeat"]), int(a["skip"])
    B = len(counts)
    used = cost.clone()
    for r in range(R):
        used[r, :, counts[r % B]:] = 0                                                      # scipy never sees the padding either
    pairs = crit.hungarian_match(used, counts, repeat)
    host, got = cost.double().numpy(), match.detach().cpu().numpy()
    valid, total, want_total, tol = np.zeros(R), np.zeros(R), np.zeros(R), np.zeros(R)
    for r in range(R):
        g, m = counts[r % B], got[r, skip:]
        ok = m.shape == (N,) and bool(((m >= -1) & (m < max(g, 1))).all()) and (g > 0 or bool((m == -1).all()))
        if ok:
            per_target = np.bincount(m[m >= 0], minlength=max(g, 1))[:max(g, 1)]
            ok = bool((per_target == (repeat if g else 0)).all()) if g * repeat <= N else bool((m >= 0).all() and (per_target <= repeat).all())
            q = np.nonzero(m >= 0)[0]
            total[r] = host[r, q, m[q]].sum()
        valid[r] = float(ok)
        src, tgt = pairs[r]
        chosen = host[r, src.numpy(), tgt.numpy()]
        want_total[r], tol[r] = chosen.sum(), 1e-9 * np.abs(chosen).sum()
    cmps = [Cmp("valid_assignment", torch.from_numpy(valid), torch.ones(R, dtype=F64)),
            Cmp("total_cost", torch.from_numpy(total), torch.from_numpy(want_total), torch.from_numpy(tol)),
            Cmp("status", status, torch.zeros(R, dtype=torch.int32))]
    if skip:
        groups, max_gt = int(a["dn_meta"][0]), int(a["dn_meta"][1])
        slot = torch.arange(max_gt, dtype=torch.int32)
        fixed = torch.stack([torch.where(slot < counts[r % B], slot, slot.new_tensor(-1)).repeat(groups) for r in range(R)])
        same = (torch.from_numpy(got[:, :skip]) == fixed).all(1)
        cmps.append(Cmp("denoising_prefix", same.double(), torch.ones(R, dtype=F64)))
    return cmps


chk_assign_match.applies = lambda a: bool(a["fused"]) and a["cost"].is_cuda          # the host matcher is scipy itself: no launch


# -- optimizer: the torch route's single step in float64 from the kernel's own state before the step (tests/test_gpu_optim.py)
def _optim_snapshot(a):
    from helpers import snapshot
    opt = a["self"]
    return dict(a, rows=snapshot(opt), coef=None if opt._armed is None else opt._armed[-1].detach().clone())


def chk_clip_fused(a, res):
    """total norm and the armed coefficient: max(4 e32, 2^-20 |checker|)."""
    from helpers import torch_route_step
    opt, rows, max_norm = a["self"], a["rows"], float(a["max_norm"])
    n64, _ = torch_route_step(opt, rows, max_norm, F64)
    n32, _ = torch_route_step(opt, rows, max_norm, F32)
    c64, c32 = (max_norm / (n64 + 1e-6)).clamp(max=1.0), (max_norm / (n32 + 1e-6)).clamp(max=1.0)
    coef = opt.clip_coef
    assert coef is not None, "_clip_fused armed no coefficient"
    return [_floor_cmp("total_norm", res.reshape(1), n64.reshape(1), n32.reshape(1), n64.abs().reshape(1)),
            _floor_cmp("coef", coef.reshape(1), c64.reshape(1), c32.reshape(1), c64.abs().reshape(1))]


chk_clip_fused.snapshot = _optim_snapshot


def chk_step_fused(a, res):
    """Everything the step wrote, against the torch route stepped from the snapshot with the gradients scaled by the coefficient
    that was armed (the value the kernel read).  Elementwise, gc = |g coef|: exp_avg max(4 e32, 2^-20 max(|m_old|, gc)); exp_avg_sq
    max(4 e32, 2^-20 max(v_old, gc^2)); param max(4 e32, 2^-20 (|p_old| + step_size (|m_old| + gc) / denom64)); a tensor without
    a gradient keeps its bits; every live state's step advances by one."""
    from helpers import torch_route_step
    from relation_detr_amd.optim import step_scalars
    opt, rows, coef = a["self"], a["rows"], a["coef"]
    scaled = lambda dtype: [dict(r, g=None if r["g"] is None else (r["g"].to(dtype) if coef is None else r["g"].to(dtype) * coef.to(dtype)))  # noqa: E731
                            for r in rows]
    _, want = torch_route_step(opt, scaled(F64), None, F64)
    _, fp32 = torch_route_step(opt, scaled(F32), None, F32)
    parts = {k: ([], [], [], []) for k in ("param", "exp_avg", "exp_avg_sq")}
    steps_got, steps_want = [], []

    def add(key, got, ref64, ref32, scale):
        for lst, t in zip(parts[key], (got, ref64, ref32, scale)):
            lst.append(t.detach().double().reshape(-1))
    i = 0
    for group in opt.param_groups:
        beta1, beta2 = group["betas"]
        for p in group["params"]:
            row, (p64, m64, v64, g64), (p32, m32, v32, _) = rows[i], want[i], fp32[i]
            state = opt.state.get(p) or {}
            steps_got.append(float(state["step"]) if state else 0.0)
            steps_want.append(row["step"] + (0.0 if row["g"] is None else 1.0))
            if row["g"] is None:
                add("param", p, row["p"], row["p"], torch.zeros_like(row["p"]))
                if row["m"] is not None:
                    add("exp_avg", state["exp_avg"], row["m"], row["m"], torch.zeros_like(row["m"]))
                    add("exp_avg_sq", state["exp_avg_sq"], row["v"], row["v"], torch.zeros_like(row["v"]))
            else:
                step_size, bias2_sqrt = step_scalars(group["lr"], beta1, beta2, group["eps"], group["weight_decay"], row["step"] + 1)[4:6]
                m_old = torch.zeros_like(p64) if row["m"] is None else row["m"].double().abs()
                v_old = torch.zeros_like(p64) if row["v"] is None else row["v"].double()
                gc = g64.abs()
                denom = v64.sqrt() / bias2_sqrt + group["eps"]
                add("exp_avg", state["exp_avg"], m64, m32, torch.maximum(m_old, gc))
                add("exp_avg_sq", state["exp_avg_sq"], v64, v32, torch.maximum(v_old, gc * gc))
                add("param", p, p64, p32, row["p"].double().abs() + step_size * (m_old + gc) / denom)
            i += 1
    cmps = [_floor_cmp(k, *(torch.cat(lst) for lst in v)) for k, v in parts.items() if v[0]]
    return cmps + [Cmp("step", torch.tensor(steps_got, dtype=F64), torch.tensor(steps_want, dtype=F64))]


chk_step_fused.snapshot = _optim_snapshot


# -- the backbone's epilogues (tests/test_gpu_backbone.py): the operands are the COPIES, so an in-place call (out is x) is checked
#    against what x held before the launch
def _present(label, got, wanted):
    """One exact element: a result that is there (1) or None (0), against whether the call asked for it."""
    return Cmp(label, torch.tensor([0.0 if got is None else 1.0], dtype=F64), torch.tensor([1.0 if wanted else 0.0], dtype=F64))


def _epilogue_operands(a):
    x, r = a["x"], a["residual"]
    return x, a["scale"], a["shift"], (None if r is None else r.to(x.dtype))      # the entry converts the residual to x's dtype


def chk_frozen_bn_act_forward(a, res):
    """fp32: x * s, + shift, + residual, relu as separate fp32 torch operators, exact.  bf16: float64 of the same, within
    2^-8 |ref| + 2^-20 (|x s| + |shift| + |res|) (test_gpu_backbone.check_forward)."""
    from helpers import bf16_slack, torch_bn_act
    x, s, h, r = _epilogue_operands(a)
    relu = bool(a["relu"])
    if x.dtype == F32:
        return [Cmp("out", res, torch_bn_act(x, s, h, r, relu))]
    ref = torch_bn_act(x.double(), s.double(), h.double(), None if r is None else r.double(), relu)
    return [Cmp("out", res, ref, 2.0 ** -8 * ref.abs() + bf16_slack(x, s, h, r))]


def chk_frozen_bn_act_backward(a, res):
    """What autograd makes of the operator sequence, from the y the call was handed: relu's backward passes dy where not (y <= 0)
    and writes 0 elsewhere, the residual's gradient is that masked dy, x's is the masked dy times s.  fp32: both as fp32 torch
    operators, exact.  bf16: dx within 2^-8 |ref| of the float64 product, dres the masked dy exactly
    (test_gpu_backbone.test_frozen_bn_act_backward).  dres is None exactly when it was not asked for."""
    dy, y, s, relu = a["dy"], a["y"], a["scale"], bool(a["relu"])
    dx, dres = res
    masked = torch.where(y <= 0, torch.zeros_like(dy), dy) if relu else dy
    cmps = [_present("dres_returned", dres, a["want_dres"])]
    if dy.dtype == F32:
        cmps.append(Cmp("dx", dx, masked * s.reshape(1, -1, 1, 1)))
    else:
        ref = masked.double() * s.double().reshape(1, -1, 1, 1)
        cmps.append(Cmp("dx", dx, ref, 2.0 ** -8 * ref.abs()))
    if dres is not None:
        cmps.append(Cmp("dres", dres, masked))
    return cmps


def chk_stem_bn_relu_maxpool(a, res):
    """fp32: max_pool2d(relu(x * s + h), 3, 2, 1) in fp32 torch operators, exact.  bf16: float64 of the same, within 2^-8 |ref| + the
    forward's slack max-pooled (test_gpu_backbone.test_stem_pool)."""
    from helpers import bf16_slack, torch_stem
    x, s, h = a["x"], a["scale"], a["shift"]
    if x.dtype == F32:
        return [Cmp("out", res, torch_stem(x, s, h))]
    ref = torch_stem(x.double(), s.double(), h.double())
    return [Cmp("out", res, ref, 2.0 ** -8 * ref.abs() + F.max_pool2d(bf16_slack(x, s, h, None), 3, 2, 1))]


# -- the image front end (tests/test_gpu_images.check_batch, with the float64 filter and the near-tie rule of tests/test_images_host.py)
def _frontend():
    from relation_detr_amd.frontend import images
    return images


def _batch_images_operands(a):
    """(images, sizes) as batch_images forms them, or None where it raises before it looks at the kernel's conditions."""
    images = a["images"]
    images = list(images.unbind(0)) if torch.is_tensor(images) else list(images)
    if not all(torch.is_tensor(im) and im.dim() >= 2 for im in images):
        return images, None
    sizes = [(int(im.shape[-2]), int(im.shape[-1])) for im in images] if a["sizes"] is None else [(int(s[0]), int(s[1])) for s in a["sizes"]]
    return images, (sizes if len(sizes) == len(images) and a["dtype"] in (F32, BF16) else None)


def _batch_images_applies(a):
    images, sizes = _batch_images_operands(a)
    return sizes is not None and _frontend()._kernel_takes(images, sizes, a["size_divisible"], a["normalize"]) is None


def _normalised(values, mean, std):
    """(values - mean) / std per channel with torch's two in-place fp32 operations (ImagePreprocessor.batch_torch); values [3, ...] fp32."""
    shape = (3,) + (1,) * (values.dim() - 1)
    return values.clone().sub_(torch.tensor(mean, dtype=F32).view(shape)).div_(torch.tensor(std, dtype=F32).view(shape))


def _resize64(image, oh, ow):
    """test_images_host.resize64, the exact antialias filter in float64, as two matrix products (its three-operand einsum takes
    seconds at 300 x 400 pixels)."""
    from test_images_host import filter_matrix
    x = image.astype("float64")
    return filter_matrix(x.shape[1], oh) @ x @ filter_matrix(x.shape[2], ow).T


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def chk_batch_images(a, res):
    """Every element of the batch, the mask and the two size tables.  The mask, the sizes and the padding (+0 to the bit) exact.  The
    valid region per image, ``got`` against the float64 filter v64 = resize64(source):
      uint8 source   off the near ties the table value (float(rint(v64)) / 255 - mean) / std, exact; on them one of the three
                     neighbouring table values; near ties above NEAR_TIE_SHARE of the batch's valid values fail the call as ill-posed
      float source   resized: within max(4 e32, 2^-20 max(1, |ref|)) of ref = (v64 - mean) / std (v64 itself without normalisation);
                     not resized: the torch route's fp32 value, exact (a copy without normalisation)
    A bf16 batch is the rounding of the fp32 value (tests/test_gpu_images.py): exact wherever the fp32 value is; for a resized float
    source, whose fp32 value f is only known to lie in [ref - b, ref + b], rounding is monotonic, so got lies in
    [bf16(ref - b), bf16(ref + b)]."""
    import numpy as np
    from test_images_host import NEAR_TIE_SHARE, interpolate_error, near_tie
    resize64 = _resize64
    images, sizes = _batch_images_operands(a)
    mean, std, normalize, dtype = tuple(a["mean"]), tuple(a["std"]), bool(a["normalize"]), a["dtype"]
    Hp, Wp = _frontend().batched_size(sizes, a["size_divisible"])
    B = len(images)
    tensors = res.tensors.detach().cpu()
    want_mask = torch.ones(B, Hp, Wp, dtype=torch.bool)
    for i, (oh, ow) in enumerate(sizes):
        want_mask[i, :oh, :ow] = False
    original = [[int(im.shape[-2]), int(im.shape[-1])] for im in images]
    cmps = [Cmp("mask", res.mask.detach().cpu().to(torch.uint8), want_mask.to(torch.uint8)),
            Cmp("image_sizes", res.image_sizes, torch.tensor(sizes, dtype=torch.int64).reshape(B, 2)),
            Cmp("original_sizes", res.original_sizes, torch.tensor(original, dtype=torch.int64).reshape(B, 2))]
    cmps.append(Cmp("batch_dtype", torch.tensor([float(tensors.dtype == dtype)], dtype=F64), torch.ones(1, dtype=F64)))
    if tuple(tensors.shape) != (B, 3, Hp, Wp) or tensors.dtype != dtype:
        return cmps + [Cmp("batch", tensors, torch.zeros(B, 3, Hp, Wp, dtype=F64))]
    pad = want_mask[:, None].expand(B, 3, Hp, Wp)
    cmps.append(Cmp("padding_bits", torch.where(pad, _bits(tensors), torch.zeros((), dtype=_bits(tensors).dtype)), torch.zeros(B, 3, Hp, Wp, dtype=F64)))
    n_near = n_all = 0
    for i, (im, (oh, ow)) in enumerate(zip(images, sizes)):
        got = tensors[i, :, :oh, :ow]
        src = im.detach().cpu()
        copied = (oh, ow) == tuple(src.shape[-2:])
        if src.dtype == torch.uint8:
            v64 = resize64(src.numpy(), oh, ow)
            q64, near = near_tie(v64, interpolate_error(src.numpy(), v64))
            table = _normalised(torch.arange(256, dtype=F32).view(1, 256).repeat(3, 1) / 255, mean, std).to(dtype)
            q, near, rows = torch.from_numpy(q64).long(), torch.from_numpy(near), torch.arange(3).view(3, 1, 1)
            cmps.append(Cmp(f"image{i}", got, table[rows, q], keep=~near))
            if bool(near.any()):
                ok = (got == table[rows, q]) | (got == table[rows, (q - 1).clamp(0, 255)]) | (got == table[rows, (q + 1).clamp(0, 255)])
                cmps.append(Cmp(f"image{i}_near_ties", ok[near].double(), torch.ones(int(near.sum()), dtype=F64)))
            n_near, n_all = n_near + int(near.sum()), n_all + near.numel()
        elif copied:
            cmps.append(Cmp(f"image{i}", got, (_normalised(src, mean, std) if normalize else src).to(dtype)))
        else:
            v64 = resize64(src.numpy(), oh, ow)
            e32 = interpolate_error(src.numpy(), v64)
            ref = (v64 - np.array(mean).reshape(3, 1, 1)) / np.array(std).reshape(3, 1, 1) if normalize else v64
            ref = torch.from_numpy(ref)
            bound = torch.clamp(2.0 ** -20 * ref.abs().clamp(min=1.0), min=4.0 * e32)
            if dtype == BF16:
                lo, hi = (ref - bound).float().to(BF16).double(), (ref + bound).float().to(BF16).double()
                ref, bound = (lo + hi) / 2, (hi - lo) / 2
            cmps.append(Cmp(f"image{i}", got, ref, bound))
    if n_all:
        cmps.append(Cmp("near_tie_share", torch.tensor([float(n_near)], dtype=F64), torch.zeros(1, dtype=F64), NEAR_TIE_SHARE * n_all, gate=True))
    return cmps


chk_batch_images.applies = _batch_images_applies

# ------------------------------------------------------------------------------------------ every entry outside ops.py, one table
TRAIN_ENTRIES: Dict[str, Callable] = {
    "ffn_train.ffn_k256_train": chk_ffn_k256_train,
    "ffn_train.ffn_k256_backward": chk_ffn_k256_backward,
    "ln_train.add_layer_norm_train": chk_add_layer_norm_train,
    "ln_train.add_layer_norm_backward": chk_add_layer_norm_backward,
    "attn_rel_train._relation_attention_boxes_train": chk__relation_attention_boxes_train,
    "attn_rel_train._relation_attention_boxes_backward": chk__relation_attention_boxes_backward,
    "msda_train_hm.ms_deform_attn_backward_fused_hm": chk_ms_deform_attn_backward_fused_hm,
    "msda_train_hm.grad_value_from_head_major": chk_grad_value_from_head_major,
    "amp_train.add_layer_norm_mixed_train": chk_add_layer_norm_mixed_train,
    "amp_train.add_layer_norm_mixed_backward": chk_add_layer_norm_mixed_backward,
    "amp_train.ffn_mixed_train": chk_ffn_mixed_train,
    "amp_train.ffn_mixed_backward": chk_ffn_mixed_backward,
    "neck.group_norm_levels_forward": chk_group_norm_levels_forward,
    "neck.group_norm_levels_backward": chk_group_norm_levels_backward,
    "neck._masks_and_counts": chk__masks_and_counts,
    "neck._sine_pos_packed": chk__sine_pos_packed,
    "denoising.cdn_noise": chk_cdn_noise,
    "denoising.denoising_mask": chk_denoising_mask,
    "denoising.cdn_queries_forward": chk_cdn_queries_forward,
    "denoising.cdn_embed_backward": chk_cdn_embed_backward,
    "criterion.match_cost": chk_match_cost,
    "criterion.assign_match": chk_assign_match,
    "criterion.set_loss_forward": chk_set_loss_forward,
    "optim.FusedAdamW._clip_fused": chk_clip_fused,
    "optim.FusedAdamW._step_fused": chk_step_fused,
    "backbones.epilogue.frozen_bn_act_forward": chk_frozen_bn_act_forward,
    "backbones.epilogue.frozen_bn_act_backward": chk_frozen_bn_act_backward,
    "backbones.epilogue.stem_bn_relu_maxpool": chk_stem_bn_relu_maxpool,
    "frontend.images.batch_images": chk_batch_images,
}

# the rest of the four training modules: routing predicates and argument helpers that launch nothing; ffn_train._pack, which launches a
# re-layout only from inside a checked entry (as the ops packers); and the two public natural-log wrappers of attn_rel_train,
# whose one launch is the checked private entry
# and of the five modules of the detector step: routing predicates, argument checks, the torch routes (which serve as references above), the
# differentiable wrappers whose launches are the checked entries, amp_train.ffn_pack_f32 and neck._gn_workspace (LAUNCH_INSIDE_ENTRY),
# and every method of FusedAdamW but the two that launch
TRAIN_HOST_ONLY = frozenset({
    "ffn_train.ffn_train_supported", "ffn_train._pack", "ffn_train._aligned_rows",
    "ln_train._aligned", "ln_train._rows", "ln_train.add_layer_norm_train_supported", "ln_train._param", "ln_train._entry",
    "attn_rel_train._f32", "attn_rel_train.relation_attention_boxes_train", "attn_rel_train.relation_attention_boxes_backward",
    "msda_train_hm._merged_slices", "msda_train_hm.split_merged_projection",
    "amp_train.autocast_bf16_active", "amp_train.mixed_norm_operands_ok", "amp_train.add_layer_norm_mixed_supported",
    "amp_train._ffn_dims_ok", "amp_train.ffn_mixed_supported", "amp_train.ffn_pack_f32",
    "neck._stream", "neck._require_device", "neck._pointers", "neck._level_hw", "neck._gn_check", "neck._gn_workspace",
    "neck.group_norm_levels", "neck._split_counts", "neck.pyramid_masks", "neck.sine_dim_t", "neck.pyramid_sine_pos", "neck._conv_norm",
    "neck.build_pyramid",
    "denoising.denoising_groups", "denoising.philox4x32_10", "denoising._noise_numpy", "denoising._layout", "denoising._suffix",
    "denoising._cdn_queries_torch", "denoising._check_noise", "denoising.cdn_queries",
    "criterion.box_cxcywh_to_xyxy", "criterion._inter_union", "criterion.box_iou", "criterion.generalized_box_iou", "criterion._image_cost",
    "criterion._varifocal", "criterion._set_losses", "criterion._set_loss_torch", "criterion._rows", "criterion._suffix",
    "criterion._check_stack", "criterion.hungarian_match", "criterion._dn_groups", "criterion.set_loss", "criterion._layer_keys",
    "optim.build_chunk_map", "optim.step_scalars", "optim.fused_refusal", "optim.relation_param_groups", "optim.train_step",
    "optim.FusedAdamW.__init__", "optim.FusedAdamW.add_param_group", "optim.FusedAdamW._params", "optim.FusedAdamW._on_fused_route",
    "optim.FusedAdamW._first_param", "optim.FusedAdamW._grad_of", "optim.FusedAdamW._check_flags", "optim.FusedAdamW._check_groups", "optim.FusedAdamW._init_state",
    "optim.FusedAdamW._clip_torch", "optim.FusedAdamW._step_torch", "optim.FusedAdamW._gather", "optim.FusedAdamW._group_keys",
    "optim.FusedAdamW._build_tables", "optim.FusedAdamW._prepare", "optim.FusedAdamW._prepared_still_holds",
    "optim.FusedAdamW.clip_grad_norm_", "optim.FusedAdamW.step", "optim.FusedAdamW.load_state_dict",
    # the backbone's epilogues: layout and argument helpers, and the differentiable wrapper with its autograd Function, which reach the
    # two checked entries through the module's own globals
    "backbones.epilogue._need_device", "backbones.epilogue._channels_last", "backbones.epilogue._dense", "backbones.epilogue._constants",
    "backbones.epilogue._shape", "backbones.epilogue._stream", "backbones.epilogue.frozen_bn_act",
    "backbones.epilogue.FrozenBNActFunction.forward", "backbones.epilogue.FrozenBNActFunction.backward",
    # the image front end: the size rules, the kernel's conditions, the torch route (the reference of the host test), the targets, and
    # every method of the module, whose one launching call is the checked batch_images
    "frontend.images.resized_size", "frontend.images._resize_bounds", "frontend.images.batched_size", "frontend.images._kernel_takes",
    "frontend.images.resize_image", "frontend.images.check_boxes", "frontend.images.prepare_targets",
    "frontend.images.ImagePreprocessor.__init__", "frontend.images.ImagePreprocessor.target_sizes",
    "frontend.images.ImagePreprocessor.takes_fused_route", "frontend.images.ImagePreprocessor.batch_torch",
    "frontend.images.ImagePreprocessor.batch_fused", "frontend.images.ImagePreprocessor._targets",
    "frontend.images.ImagePreprocessor.forward_torch", "frontend.images.ImagePreprocessor.forward_fused",
    "frontend.images.ImagePreprocessor.forward",
})


# functions ("module.function") that name a launching rdetr_* symbol, or a *_workspace_bytes size, without being a checked entry:
# each launches only from inside one.  tests/test_shadow_complete.py holds this from the source: every function of the package that
# names such a symbol is an entry or listed here, and every caller of a listed function is an entry or listed.
LAUNCH_INSIDE_ENTRY = frozenset({
    "ops._packed_k256", "ops._packed_k_halves", "ops._packed_query_proj", "ops.ffn_k256_packed_weights", "ffn_train._pack",
    "rowtail.linear_ln_rows", "amp_train.ffn_pack_f32",
    "ln_train._entry",                                        # picks the symbol its two callers, both entries, launch
    "ops._msda_backward_buffers", "neck._gn_workspace",      # callers of a *_workspace_bytes size
})


# ------------------------------------------------------------------------------------------------------------ write sets
# For every checked entry, the parameters the call is ALLOWED to write (``Shadow(writes=True)``); every other tensor operand must
# come back bit-identical.  A dotted name is a key of a dict parameter ("class_head.out": ``class_head["out"]``, where the caller may
# hand in the destination).  No wildcards; tests/test_shadow_complete.py holds that the keys are exactly the checked entries, that
# every name is a parameter and that every parameter called ``out`` is declared.  The two FusedAdamW methods take their operands
# from the optimizer: a callable (the snapshot dictionary, which holds ``self`` as before the call) -> the tensors it may write.
def _adamw_clip_writes(a):
    """The clip reads the gradients and arms a coefficient in a workspace of its own: it may write no parameter, gradient or state."""
    return []


def _adamw_step_writes(a):
    """Parameter, exp_avg, exp_avg_sq and step of every parameter that has a gradient."""
    opt, out = a["self"], []
    for group in opt.param_groups:
        for p in group["params"]:
            if p.grad is not None:
                out.append(p)
                out += [v for v in (opt.state.get(p) or {}).values() if torch.is_tensor(v)]
    return out


WRITES: Dict[str, object] = {
    "ms_deform_attn_forward": (), "ms_deform_attn_forward_fused": (), "value_to_head_major": (), "value_proj_head_major": (),
    "encoder_proj": (),
    "linear_k256": ("out",), "ffn_k256": ("out",), "ffn_ln_k256": ("out",),
    "linear_ln_k256": ("out", "extra.out_plus_pos"),
    "add_layer_norm": ("out",),
    "relation_bias": (),
    "bias_softmax_": ("scores",),
    "relation_attention": (), "relation_attention_boxes": (), "_relation_attention_train": (), "_relation_attention_backward": (),
    "relation_bias_backward": (), "ms_deform_attn_backward": (), "ms_deform_attn_backward_fused": (),
    "box_refine": (), "sine_pos_embed": (),
    "zero_masked_rows_": ("x",),
    "row_max": (),
    "box_head_k256": ("class_head.out",),
    "query_pos_k256": ("in_proj.qk", "in_proj.v"),
    "topk": (), "detections_from_topk": (), "scaled_pos": (), "decoder_reference": (), "pyramid_points": (),
    "tokens_from_levels": ("out",),
    "ffn_train.ffn_k256_train": (), "ffn_train.ffn_k256_backward": (),
    "ln_train.add_layer_norm_train": (), "ln_train.add_layer_norm_backward": (),
    "attn_rel_train._relation_attention_boxes_train": (), "attn_rel_train._relation_attention_boxes_backward": (),
    "msda_train_hm.ms_deform_attn_backward_fused_hm": ("grad_producer_out",),
    "msda_train_hm.grad_value_from_head_major": ("out",),
    "amp_train.add_layer_norm_mixed_train": (), "amp_train.add_layer_norm_mixed_backward": (),
    "amp_train.ffn_mixed_train": (), "amp_train.ffn_mixed_backward": (),
    "neck.group_norm_levels_forward": (), "neck.group_norm_levels_backward": (), "neck._masks_and_counts": (), "neck._sine_pos_packed": (),
    "denoising.cdn_noise": (), "denoising.denoising_mask": (), "denoising.cdn_queries_forward": (), "denoising.cdn_embed_backward": (),
    "criterion.match_cost": ("out",),
    "criterion.assign_match": ("out",),
    "criterion.set_loss_forward": (),
    "optim.FusedAdamW._clip_fused": _adamw_clip_writes,
    "optim.FusedAdamW._step_fused": _adamw_step_writes,
    "backbones.epilogue.frozen_bn_act_forward": ("out",),
    "backbones.epilogue.frozen_bn_act_backward": (), "backbones.epilogue.stem_bn_relu_maxpool": (),
    "frontend.images.batch_images": (),
}


def operand_tensors(x, path=""):
    """-> [(path, tensor)] of every tensor reachable from an argument: tensors, and those inside lists, tuples (a Noise too) and
    dicts; the parameters and buffers of a module (``layers`` of box_head_k256 are nn.Linear); the parameters, their gradients and
    the state of an optimizer (``self`` of the FusedAdamW methods)."""
    if torch.is_tensor(x):
        return [(path, x)] if x.layout == torch.strided else []
    found = []
    if isinstance(x, dict):
        for k, v in x.items():
            found += operand_tensors(v, f"{path}.{k}" if path else str(k))
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            found += operand_tensors(v, f"{path}[{i}]")
    elif isinstance(x, torch.nn.Module):
        for k, v in list(x.named_parameters()) + list(x.named_buffers()):
            found.append((f"{path}.{k}", v))
    elif isinstance(x, torch.optim.Optimizer):
        i = 0
        for group in x.param_groups:
            for p in group["params"]:
                found.append((f"{path}.param[{i}]", p))
                if p.grad is not None:
                    found += operand_tensors(p.grad, f"{path}.param[{i}].grad")
                found += operand_tensors({k: v for k, v in (x.state.get(p) or {}).items()}, f"{path}.state[{i}]")
                i += 1
    return found


def _declared(paths, operands):
    """The operands a tuple of WRITES names: "out" names the argument and whatever it holds, "extra.out_plus_pos" one key."""
    names = tuple(paths)
    return [(p, t) for p, t in operands if any(p == n or p.startswith(n + ".") or p.startswith(n + "[") for n in names)]


def byte_range(t):
    """[lo, hi): the addresses the elements of ``t`` span (non-negative strides, as torch's are)."""
    lo = t.data_ptr()
    n = 0 if t.numel() == 0 else 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
    return lo, lo + n * t.element_size()


def _overlaps(a, b):
    (alo, ahi), (blo, bhi) = byte_range(a), byte_range(b)
    return a.device == b.device and alo < bhi and blo < ahi


_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def int_bits(t):
    """The elements of ``t`` as integers of the same size, so that a NaN equals itself and -0.0 differs from +0.0."""
    t = t.detach()
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    if t.is_complex():
        t = torch.view_as_real(t)
    return t if not t.is_floating_point() else t.view(_INT_OF_SIZE[t.element_size()])


def storage_bytes(t):
    """The whole storage ``t`` lives in, as a uint8 tensor (no copy)."""
    return torch.Tensor.set_(torch.tensor([], dtype=torch.uint8, device=t.device), t.untyped_storage())


def addressed_bytes(t, n):
    """uint8 [n]: 1 at every byte of ``t``'s storage (of n bytes) that an element of ``t`` occupies."""
    mask = torch.zeros(n, dtype=torch.uint8, device=t.device)
    item = t.element_size()
    if t.numel() and all(st > 0 or s == 1 for s, st in zip(t.shape, t.stride())):
        mask.as_strided(tuple(t.shape) + (item,), tuple(s * item for s in t.stride()) + (1,), t.storage_offset() * item).fill_(1)
    elif t.numel():                                            # an expanded view: the range its elements span
        lo = t.storage_offset() * item
        mask[lo:lo + byte_range(t)[1] - byte_range(t)[0]].fill_(1)
    return mask


@dataclasses.dataclass
class _WriteWatch:
    """What ``Shadow(writes=True)`` holds between the copies before a call and the comparison after it."""
    kept: list                    # (path, tensor, copy): operands that must come back bit-identical
    views: list                   # (storage bytes, copy of them, [(path, tensor)]): the storages of the declared operands
    operands: list                # (path, tensor), all of them
    mark: int                     # guard allocations before the call


# ----------------------------------------------------------------------------------------------------------------- harness
def patch_targets():
    """(owner, attribute, key, entries, host-only set) of every function the harness classifies: the functions of ops, and of every
    module of TRAIN_MODULES with the methods of its TRAIN_CLASSES (owner: the class)."""
    import importlib
    ops = importlib.import_module(PACKAGE + ".ops")
    targets = [(ops, name, name, KERNEL_ENTRIES, HOST_ONLY) for name in ops_functions(ops)]
    for short in TRAIN_MODULES:
        module = importlib.import_module(f"{PACKAGE}.{short}")
        for key in train_functions(module):
            *owners, attr = key[len(short) + 1:].split(".")
            owner = module
            for name in owners:                                    # "module.Class.method": patched on the class
                owner = getattr(owner, name)
            targets.append((owner, attr, key, TRAIN_ENTRIES, TRAIN_HOST_ONLY))
    return targets


def aliases(fn, owner, attr):
    """Every (module, name) of the package, other than (owner, attr), whose global ``name`` is the function object ``fn``."""
    import sys
    found = []
    for mod_name, module in sorted(sys.modules.items()):
        if module is None or not (mod_name == PACKAGE or mod_name.startswith(PACKAGE + ".")):
            continue
        for name, value in list(vars(module).items()):
            if value is fn and (module is not owner or name != attr):
                found.append((module, name))
    return found


def _copy(x):
    if torch.is_tensor(x):
        return x.detach().clone()
    if isinstance(x, (list, tuple)) and any(torch.is_tensor(t) for t in x):
        return type(x)(_copy(t) for t in x)
    return x


class Shadow:
    """``Shadow(monkeypatch, fault=None, check=True, writes=False, guard=None)``; ``fault(name, call, bound_args, result, rerun) ->
    result`` may replace a kernel's result before the check (the harness's own fault-injection test), or write where the call
    should not have.  ``check=False`` installs only the counting tripwires at the C boundary (``launches``): no wrapper, no
    reference, no error for a launch outside an entry.  ``writes=True`` adds the write-set record of the module docstring to every
    call; ``guard``: the installed tests/guard.py ``Guard`` whose bands it checks (needs ``writes=True``)."""

    def __init__(self, monkeypatch, fault: Optional[Callable] = None, check: bool = True, writes: bool = False, guard=None):
        from relation_detr_amd import _lib
        if guard is not None and not writes:
            raise ValueError("Shadow(guard=...) needs writes=True: the bands are checked by the write-set record")
        self.writes, self.guard = bool(writes), guard
        # comparisons made: "operand_bits" (elements), "outside_view" and "bands" (bytes); "declared": the destinations handed in
        self.write_checks: collections.Counter = collections.Counter()
        self._bands_reported: set = set()
        self._bands_done = False
        self.records: List[Record] = []
        self.calls: collections.Counter = collections.Counter()
        self.checked: collections.Counter = collections.Counter()
        self.errors: List[str] = []
        self.launches: collections.Counter = collections.Counter()
        self.depth = 0
        self.fault = fault
        self.check = check
        for owner, attr, key, entries, host_only in patch_targets() if check else ():
            if key in host_only:
                continue
            fn = getattr(owner, attr)
            wrapper = self._checked(key, fn, entries[key]) if key in entries else self._unclassified(key, fn)
            wrapper.shadow_key = key
            monkeypatch.setattr(owner, attr, wrapper)
            # ... and wherever another module of the package holds the same function object as a global (``from .epilogue import
            # stem_bn_relu_maxpool`` in backbones/resnet.py, the re-exports of an __init__): a call through that name is the same launch
            for other, name in aliases(fn, owner, attr) if inspect.ismodule(owner) else ():
                monkeypatch.setattr(other, name, wrapper)
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
        # a checker may carry `applies(arguments) -> bool` (False: this call takes the function's host route, which launches
        # nothing and is not recorded; the tripwire still stands behind it) and `snapshot(arguments) -> copies` (its own
        # pre-call copy, for operands that are not tensor arguments: an optimizer's parameters, state and armed coefficient)
        applies, snapshot = getattr(checker, "applies", None), getattr(checker, "snapshot", None)

        def wrapper(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            if applies is not None and not applies(bound.arguments):
                return fn(*args, **kwargs)
            call = self.calls[name]
            self.calls[name] += 1
            copies = snapshot(bound.arguments) if snapshot is not None else {k: _copy(v) for k, v in bound.arguments.items()}
            watch = self._watch(name, bound.arguments, copies if snapshot is not None else bound.arguments) if self.writes else None
            self.depth += 1
            if self.guard is not None:
                self.guard.active.append(name)
            try:
                result = fn(*args, **kwargs)
                if self.fault is not None:
                    result = self.fault(name, call, bound.arguments, result, fn)
            finally:
                self.depth -= 1
                if self.guard is not None:
                    self.guard.active.pop()
            if watch is not None:
                with torch.no_grad(), self._paused():
                    self._record_writes(name, call, watch)
            # the references are torch's own float64 operators, some of which have no deterministic variant (grid_sample's
            # backward): a step run under torch.use_deterministic_algorithms(True) is for the kernels, not for them
            strict, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
            torch.use_deterministic_algorithms(False)
            try:
                # autocast off: the fp32 torch routes that give e32 must run in fp32 (float64 is never autocast)
                with torch.no_grad(), torch.autocast("cuda", enabled=False), self._paused():
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

    # ------------------------------------------------------------------------------------------------------- write sets
    def _paused(self):
        """The guard steps aside for the harness's own allocations (copies, masks, float64 references): no kernel writes them."""
        return self.guard.pause() if self.guard is not None else contextlib.nullcontext()

    def _watch(self, name, arguments, snapshot_arguments) -> _WriteWatch:
        """Before the call: a copy of every operand that must come back unchanged, and of the whole storage of every declared one."""
        with torch.no_grad(), self._paused():
            operands = [(p, t) for k, v in arguments.items() for p, t in operand_tensors(v, k)]
            rule = WRITES.get(name)
            if rule is None:
                self.errors.append(f"`{name}` has no WRITES entry")
                rule = ()
            declared = [("allowed", t) for t in rule(snapshot_arguments)] if callable(rule) else _declared(rule, operands)
            written = {id(t) for _, t in declared}
            self.write_checks["declared"] += len(declared)      # destinations handed in: without one there is no view to look outside of
            kept, seen = [], set()
            for p, t in operands:
                if id(t) in written or id(t) in seen or t.numel() == 0 or any(_overlaps(t, d) for _, d in declared):
                    continue                                   # frozen_bn_act_forward(x, ..., out=x): x is written
                seen.add(id(t))
                kept.append((p, t, t.detach().clone()))
            views = {}
            for p, t in declared:
                if t.numel():
                    key = (t.device, t.untyped_storage().data_ptr())
                    if key not in views:
                        raw = storage_bytes(t)
                        views[key] = (raw, raw.clone(), [])
                    views[key][2].append((p, t))
            return _WriteWatch(kept, list(views.values()), operands, len(self.guard.allocations) if self.guard is not None else 0)

    def _record_writes(self, name, call, w: _WriteWatch):
        """After the call: one more record under the same op.  failing = changed elements of operands that are not in the write set
        + changed bytes of a declared operand's storage that its elements do not address + changed bytes of guard bands."""
        counts, labels = [], []
        checked = 0
        for p, t, before in w.kept:
            counts.append((int_bits(t) != int_bits(before)).sum())
            labels.append(("operand_bits", p, t, before))
            checked += t.numel()
            self.write_checks["operand_bits"] += t.numel()
        for raw, before, members in w.views:
            inside = torch.zeros(raw.numel(), dtype=torch.uint8, device=raw.device)
            for _, t in members:
                inside |= addressed_bytes(t, raw.numel())
            outside = int(raw.numel()) - int(inside.sum())
            counts.append(((raw != before) & (inside == 0)).sum())
            labels.append(("outside_view", "/".join(p for p, _ in members), raw, torch.where(inside == 0, before, raw)))
            checked += outside
            self.write_checks["outside_view"] += outside
        bad, failing, where = [], 0, ""
        by_device: Dict[torch.device, List[int]] = {}
        for i, c in enumerate(counts):
            by_device.setdefault(c.device, []).append(i)
        for idx in by_device.values():                                           # one read back per device
            for i, v in zip(idx, torch.stack([counts[i] for i in idx]).tolist()):
                if v:
                    bad.append((i, int(v)))
        for i, v in sorted(bad):
            kind, p, now, before = labels[i]
            failing += v
            if kind == "operand_bits":
                flat = int(torch.nonzero((int_bits(now) != int_bits(before)).reshape(-1))[0])
                where = where or f"operand `{p}` is not in the write set and changed in {v} elements, the first at flat index {flat}"
            else:
                first = int(torch.nonzero(now != before)[0])
                where = where or f"{v} bytes of the storage of `{p}` changed outside the view, the first at storage byte {first}"
        if self.guard is not None:
            mine = self.guard.allocations[w.mark:]
            seen = {a.index for a in mine}
            for _, t in w.operands:
                a = self.guard.of(t)
                if a is not None and a.index not in seen:
                    seen.add(a.index)
                    mine.append(a)
            n = self.guard.band_bytes(mine)
            checked += n
            self.write_checks["bands"] += n
            for d in self.guard.check(mine):
                if (d.index, d.side) in self._bands_reported:
                    continue
                self._bands_reported.add((d.index, d.side))
                failing += d.changed
                where = where or str(d)
        self.records.append(Record(name, call, math.inf if failing else 0.0, failing, checked, "writes: " + (where or "clean"), "writes"))

    def finish_bands(self) -> List[str]:
        """Once, when the case ends: every band of the guard again.  Damage in a buffer that was clean when its own entry returned
        is an error against "a later launch", with the allocation's entry named."""
        if self.guard is None or self._bands_done:
            return []
        self._bands_done = True
        found = []
        n = self.guard.band_bytes()
        self.write_checks["bands"] += n
        for d in self.guard.check():
            if (d.index, d.side) not in self._bands_reported:
                self._bands_reported.add((d.index, d.side))
                found.append(f"a later launch wrote into the {d}")
        self.errors += found
        return found

    # ---------------------------------------------------------------------------------------------------------- results
    def called(self) -> set:
        return {r.op for r in self.records}

    def failures(self) -> List[Record]:
        return [r for r in self.records if r.failing or not math.isfinite(r.ratio)]

    def report(self, title: str = "") -> str:
        by = collections.OrderedDict()
        for r in sorted(self.records, key=lambda r: r.op):
            by.setdefault(r.op, []).append(r)
        writes = f" {'writes: checked / bad':>24s}" if self.writes else ""
        lines = [f"shadow checks: {title}", f"{'op':34s} {'calls':>6s} {'elements checked':>17s} {'max err/bound':>14s}{writes}  worst at"]
        for op, both in by.items():
            rs, ws = [r for r in both if r.kind == "values"], [r for r in both if r.kind == "writes"]
            w = max(rs, key=lambda r: r.ratio)
            column = f" {sum(r.checked for r in ws):15d} / {sum(r.failing for r in ws):<6d}" if self.writes else ""
            lines.append(f"{op:34s} {len(rs):6d} {sum(r.checked for r in rs):17d} {w.ratio:14.4f}{column}  call {w.call}: {w.where}")
            for r in ws:
                if r.failing:
                    lines.append(f"{'':34s} call {r.call}: {r.where}")
        if self.writes:
            lines.append("write checks: " + ", ".join(f"{k} {v}" for k, v in sorted(self.write_checks.items())))
        for e in sorted(set(self.errors)):
            lines.append("ERROR " + e)
        text = "\n".join(lines)
        print(text)
        return text

    def assert_ok(self, expected_ops=None):
        self.finish_bands()
        bad = self.failures()
        msgs = [f"{r.op} call {r.call}: {r.failing} elements over bound, worst ratio {r.ratio:.3g} at {r.where}" for r in bad[:20]]
        assert not self.errors, sorted(set(self.errors))
        assert not bad, "\n".join(msgs)
        assert all(self.checked[op] > 0 for op in self.called()), [op for op in self.called() if not self.checked[op]]
        if expected_ops is not None:
            assert self.called() == set(expected_ops), (sorted(self.called() - set(expected_ops)),
                                                        sorted(set(expected_ops) - self.called()))
