"""Training route of the encoder's deformable attention on the head-major value ``[B, 8, S, 32]`` (bf16; csrc/msda_bwd.hip,
csrc/glue.hip).

Inference of an encoder layer already gathers from the head-major value (``ops.value_to_head_major`` with the padding zero-fill
folded in, ``ops.ms_deform_attn_forward_fused(..., value_layout="bhsd")``, the resident-levels kernel where it pays).  This module
is the training counterpart, so that both modes share one data path:

* ``ms_deform_attn_backward_fused_hm`` -- the fused-producer backward reading the head-major value and accumulating ``grad_value``
  head-major (``rdetr_msda_backward_fused_hm_bf16``: the kernel body of ``ops.ms_deform_attn_backward_fused`` with another
  addressing, the same bits for the offset / logit / reference-point gradients).  Offsets and logits may be the two column slices
  of one merged projection output; their gradients are then written into the matching slices of one buffer;
* ``grad_value_from_head_major`` -- the adjoint of ``ops.value_to_head_major``: fp32 ``[B, 8, S, 32]`` -> bf16 ``[B, S, 256]`` with
  the padded rows zero, one pass (``rdetr_grad_value_from_head_major_bf16``) instead of a cast pass plus the masked-fill backward;
* ``MultiScaleDeformableAttnHeadMajorFunction`` -- the three as one autograd node whose forward makes the very calls of the eval path;
* ``split_merged_projection`` -- the two column slices of the merged query projection, with a backward that hands the merged
  gradient buffer on as it is instead of re-assembling it from the slices.

No CPU path: a tensor that is not on a ROCm device raises.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops
from .ops import (_check_fused_operands, _mask_u8, _msda_backward_buffers, _producer_operand, _require_contiguous, _require_device,
                  _stream_ptr, _value_dims)


def grad_value_from_head_major(grad_hm: torch.Tensor, key_padding_mask: Optional[torch.Tensor] = None,
                               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """grad_hm [B,8,S,32] fp32 (the head-major ``grad_value``) -> [B,S,256] bf16, channel = head * 32 + c, rounded once; the rows of
    padded positions (``key_padding_mask`` [B,S]) are zeros.  Same bits as
    ``grad_hm.permute(0, 2, 1, 3).reshape(B, S, 256).to(bfloat16).masked_fill(mask[..., None], 0)``.  ``out``: a bf16 [B,S,256]
    tensor to write into, which may be a column slice of a wider buffer (rows evenly strided, 16-byte aligned)."""
    _require_device(grad_hm, key_padding_mask, out)
    if grad_hm.dim() != 4 or tuple(grad_hm.shape[1::2]) != (8, 32) or grad_hm.dtype != torch.float32:
        raise _lib.RdetrError("grad_value_from_head_major: expected a float32 [B, 8, S, 32] tensor")
    grad_hm = grad_hm.contiguous()
    B, _, S, _ = grad_hm.shape
    mask = _mask_u8(key_padding_mask, B, S)
    if out is None:
        out = torch.empty(B, S, 256, dtype=torch.bfloat16, device=grad_hm.device)
    elif (out.dtype != torch.bfloat16 or tuple(out.shape) != (B, S, 256) or out.stride(2) != 1 or out.stride(1) < 256 or out.stride(1) % 8
          or (B > 1 and out.stride(0) != S * out.stride(1)) or out.data_ptr() % 16):
        raise _lib.RdetrError("grad_value_from_head_major: out must be bf16 [B, S, 256] with evenly strided 16-byte aligned rows")
    st = _lib.load().rdetr_grad_value_from_head_major_bf16(grad_hm.data_ptr(), None if mask is None else mask.data_ptr(), B, S, 8, 32,
                                                           out.data_ptr(), out.stride(1), _stream_ptr(grad_hm))
    _lib.check(st, "rdetr_grad_value_from_head_major_bf16")
    return out


def _merged_slices(sampling_offsets: torch.Tensor, attn_logits: torch.Tensor, ld_off, ld_lg, n_lg: int) -> bool:
    """True if the two tensors are the column slices [0, 2n) and [2n, 3n) of the rows of one buffer."""
    return bool(ld_off and ld_off == ld_lg and ld_off >= 3 * n_lg
                and attn_logits.data_ptr() == sampling_offsets.data_ptr() + 2 * n_lg * sampling_offsets.element_size())


def ms_deform_attn_backward_fused_hm(value_hm: torch.Tensor, spatial_shapes: torch.Tensor, level_start_index: torch.Tensor,
                                     sampling_offsets: torch.Tensor, attn_logits: torch.Tensor, reference_points: torch.Tensor,
                                     grad_output: torch.Tensor, deterministic: Optional[bool] = None, need_ref_grad: bool = False,
                                     grad_producer_out: Optional[torch.Tensor] = None):
    """Gradients of ``ops.ms_deform_attn_forward_fused(value_hm, ..., value_layout="bhsd")`` with respect to its own inputs
    -> [grad_value_hm [B,8,S,32] fp32, grad_offsets, grad_logits (bf16), grad_reference_points (fp32, summed over heads) or None].
    value_hm [B,8,S,32] bf16; sampling_offsets [B,Nq,8,L,4,2] and attn_logits [B,Nq,8,L*4] bf16, contiguous or column slices of a
    wider row-major buffer; reference_points [B,Nq,L,2|4] fp32; grad_output [B,Nq,256].
    When the two are the slices [0, 2n) and [2n, 3n) (n = 8*L*4) of ONE buffer, their gradients are views of the matching slices of
    one new [B,Nq,3n] tensor -- or of ``grad_producer_out`` (bf16 [B,Nq,W], W >= 3n, contiguous) if given, whose other columns are
    left untouched.  ``deterministic`` (default ``torch.are_deterministic_algorithms_enabled()``): grad_value through sorted per-row
    sums instead of float atomics; the other gradients are the same bits either way, and the bits of
    ``ops.ms_deform_attn_backward_fused`` on the [B,S,8,32] copy of the value."""
    _require_device(value_hm, spatial_shapes, level_start_index, sampling_offsets, attn_logits, reference_points, grad_output,
                    grad_producer_out)
    if value_hm.dtype != torch.bfloat16:
        raise _lib.RdetrError("ms_deform_attn_backward_fused_hm: expected a bfloat16 value [B,H,S,D]")
    B, S, H, D = dims = _value_dims(value_hm, "bhsd")
    Nq, L, P, ref_dim = _check_fused_operands(dims, value_hm.dtype, spatial_shapes, level_start_index, sampling_offsets, attn_logits,
                                              reference_points)
    if tuple(grad_output.shape) != (B, Nq, H * D) or grad_output.dtype != value_hm.dtype:
        raise _lib.RdetrError("grad_output must be [B, Nq, H*D] in value's dtype")
    if not ops.msda_fast_path(H, D, L, P):
        raise _lib.RdetrError("ms_deform_attn_backward_fused_hm: H = 8, D = 32, P = 4, L <= 8 only")
    sampling_offsets, ld_off = _producer_operand(sampling_offsets)
    attn_logits, ld_lg = _producer_operand(attn_logits)
    grad_output = grad_output.contiguous()
    _require_contiguous(value=value_hm, spatial_shapes=spatial_shapes, level_start_index=level_start_index,
                        reference_points=reference_points)
    n_lg = H * L * P
    dev = value_hm.device
    if grad_producer_out is not None or _merged_slices(sampling_offsets, attn_logits, ld_off, ld_lg, n_lg):
        buf = grad_producer_out
        if buf is None:
            buf = torch.empty(B, Nq, 3 * n_lg, dtype=torch.bfloat16, device=dev)
        elif (buf.dtype != torch.bfloat16 or buf.dim() != 3 or tuple(buf.shape[:2]) != (B, Nq) or buf.shape[2] < 3 * n_lg
              or not buf.is_contiguous() or buf.shape[2] % 2 or buf.data_ptr() % 4):
            raise _lib.RdetrError("grad_producer_out must be a contiguous bfloat16 [B, Nq, W] tensor with W >= 3*H*L*P, W even")
        grad_off = buf[..., :2 * n_lg].view(B, Nq, H, L, P, 2)
        grad_lg = buf[..., 2 * n_lg:3 * n_lg].view(B, Nq, H, L * P)
        ld_goff = ld_glg = buf.shape[2]
    else:
        grad_off = torch.empty(B, Nq, H, L, P, 2, dtype=torch.bfloat16, device=dev)
        grad_lg = torch.empty(B, Nq, H, L * P, dtype=torch.bfloat16, device=dev)
        ld_goff = ld_glg = 0
    ws, nbytes, grad_value, grad_ref = _msda_backward_buffers("ms_deform_attn_backward_fused_hm", value_hm, dims, L, Nq, P,
                                                              deterministic, ref_dim if need_ref_grad else None)
    st = _lib.load().rdetr_msda_backward_fused_hm_bf16(
        value_hm.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), sampling_offsets.data_ptr(), ld_off,
        attn_logits.data_ptr(), ld_lg, reference_points.data_ptr(), ref_dim, grad_output.data_ptr(), B, S, H, D, L, Nq, P,
        None if ws is None else ws.data_ptr(), nbytes, grad_value.data_ptr(), grad_off.data_ptr(), ld_goff, grad_lg.data_ptr(), ld_glg,
        None if grad_ref is None else grad_ref.data_ptr(), _stream_ptr(value_hm))
    _lib.check(st, "rdetr_msda_backward_fused_hm_bf16")
    return [grad_value, grad_off, grad_lg, None if grad_ref is None else grad_ref.sum(2)]


class MultiScaleDeformableAttnHeadMajorFunction(torch.autograd.Function):
    """Differentiable MSDA core of an encoder layer on the head-major value:
    ``apply(projected_value [B,S,256] bf16, key_padding_mask [B,S] | None, spatial_shapes, level_start_index, sampling_offsets,
    attn_logits, reference_points)`` -> [B,S,256] bf16.  ``projected_value`` is ``value_proj(value)`` WITHOUT the padding fill.
    Forward = the eval path's two calls (``ops.value_to_head_major`` with the mask, ``ops.ms_deform_attn_forward_fused`` on the
    head-major value, ``algo="auto"``: its kernels, its bits); the head-major value is what is saved.  Backward =
    ``ms_deform_attn_backward_fused_hm`` + ``grad_value_from_head_major`` with the same mask; gradients for value, offsets, logits
    and reference points, those autograd asks for."""

    @staticmethod
    def forward(ctx, projected_value, key_padding_mask, value_spatial_shapes, value_level_start_index, sampling_offsets, attn_logits,
                reference_points):
        vh = ops.value_to_head_major(projected_value, key_padding_mask)
        out = ops.ms_deform_attn_forward_fused(vh, value_spatial_shapes, value_level_start_index, sampling_offsets, attn_logits,
                                               reference_points, None, value_layout="bhsd")
        ctx.save_for_backward(vh, key_padding_mask, value_spatial_shapes, value_level_start_index, sampling_offsets, attn_logits,
                              reference_points)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        vh, mask, shapes, starts, offsets, logits, ref = ctx.saved_tensors
        need = ctx.needs_input_grad
        gv, go, gl, gr = ms_deform_attn_backward_fused_hm(vh, shapes, starts, offsets, logits, ref, grad_output.to(vh.dtype),
                                                          need_ref_grad=need[6])
        return (grad_value_from_head_major(gv, mask) if need[0] else None, None, None, None, go if need[4] else None,
                gl if need[5] else None, gr)


class _SplitMergedProjection(torch.autograd.Function):
    @staticmethod
    def forward(ctx, both, n_off):
        ctx.n_off, ctx.shape = n_off, tuple(both.shape)
        return both[..., :n_off], both[..., n_off:]

    @staticmethod
    def backward(ctx, g_off, g_lg):
        n_off, shape = ctx.n_off, ctx.shape
        W = shape[-1]
        if g_off is None or g_lg is None:
            zeros = lambda n, like: torch.zeros(*shape[:-1], n, dtype=like.dtype, device=like.device)
            other = g_lg if g_off is None else g_off
            if other is None:
                return None, None
            g_off = zeros(n_off, other) if g_off is None else g_off
            g_lg = zeros(W - n_off, other) if g_lg is None else g_lg
        base = g_off._base
        rows = (shape[-2] * W, W, 1) if len(shape) == 3 else None
        if (base is not None and base is g_lg._base and tuple(base.shape) == shape and base.is_contiguous() and rows is not None
                and g_off.dim() == 3 and g_lg.dim() == 3 and g_off.stride() == rows and g_lg.stride() == rows
                and g_off.storage_offset() == base.storage_offset() and g_lg.storage_offset() == base.storage_offset() + n_off):
            return base, None                    # the two gradients ARE the slices of one buffer: hand it on as it is
        return torch.cat([g_off, g_lg], -1), None


def split_merged_projection(both: torch.Tensor, n_off: int):
    """``both`` [B,Nq,W] -> (both[..., :n_off], both[..., n_off:]) as views.  Differentiable; where the two incoming gradients are
    the matching column slices of one contiguous [B,Nq,W] buffer (what ``ms_deform_attn_backward_fused_hm`` writes for slices of
    one merged projection output) that buffer is the gradient of ``both`` -- no zero-fill, no copy; otherwise they are
    concatenated."""
    return _SplitMergedProjection.apply(both, n_off)
