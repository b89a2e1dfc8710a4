"""Training route of ``LayerNorm(x + residual)`` (fp32 / bf16, embed_dim 256, csrc/layernorm.hip).

``ops.add_layer_norm`` is the inference operator; this module is its training counterpart:

* ``add_layer_norm_train``    -- the same kernel body and output bits, plus the fp32 row statistics ``stats[rows, 2] = {mean, rstd}``
  (``rdetr_add_layernorm_train_*``);
* ``add_layer_norm_backward`` -- one pass over ``dy``, ``x`` and ``residual`` that writes ONE ``dx`` (the gradient of both operands:
  ``d(x + r)/dx = d(x + r)/dr = 1``) and, unless the parameters are frozen, ``dgamma`` / ``dbeta`` through per-workgroup partial sums
  added in a fixed order (``rdetr_add_layernorm_backward_*``; no atomics, the same bits on every run);
* ``AddLayerNormFunction``    -- the two as one autograd node.

Replaces, per call of a training step, the add pass (which rounds the sum to the storage type), the normalisation, the library
LayerNorm backward and its parameter-gradient pass: the sum ``x + residual`` is formed in fp32 in both kernels and never stored.
Saved for backward: x, residual, the statistics and gamma -- autograd on the unfused route keeps the rounded sum instead of the two
operands, which the surrounding graph keeps alive anyway (the block's input and the sublayer's output).  No CPU path: a tensor that
is not on a ROCm device raises.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .ops import _require_device, _row_matrix, _stream_ptr

MAX_PARTIALS = 1024              # grid cap of the backward kernel = most [2, 256] partials (kLnBwdMaxBlocks: 4 workgroups per CU x 256 CUs)
_DTYPES = (torch.float32, torch.bfloat16)


# _rows and _param are also used by amp_train.py (the mixed-precision form of this route): rename them there too


def _aligned(t: torch.Tensor, ld: int) -> bool:
    return t.data_ptr() % 16 == 0 and (ld * t.element_size()) % 16 == 0


def _rows(t: torch.Tensor):
    """``t`` [..., 256] as evenly strided, 16-byte aligned rows (`ops._row_matrix`; copied where that view is off the 16-byte grid)
    -> (tensor, leading dimension)."""
    if t.is_contiguous():                      # the common case, without the stride walk: this path is launch-bound at decoder height
        ld = t.shape[-1]
    else:
        t, ld = _row_matrix(t)
    if not _aligned(t, ld):
        t, ld = t.clone(memory_format=torch.contiguous_format), t.shape[-1]
    return t, ld


def add_layer_norm_train_supported(x: torch.Tensor, residual: Optional[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor) -> bool:
    """True where the training route applies: ROCm tensors, fp32 or bf16, 256 channels, parameters of x's dtype with 256 elements,
    residual None or of x's shape and dtype.  (Rows that are not evenly strided or 16-byte aligned are copied, never refused.)"""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype in _DTYPES and x.dim() >= 1 and x.shape[-1] == 256):
        return False
    if weight is None or bias is None:
        return False
    for p in (weight, bias):
        if not p.is_cuda or p.dtype != x.dtype or p.numel() != 256:
            return False
    if residual is not None and not (residual.is_cuda and residual.shape == x.shape and residual.dtype == x.dtype):
        return False
    return True


def _param(p: torch.Tensor) -> torch.Tensor:
    if p.dim() != 1 or not p.is_contiguous() or p.data_ptr() % 16:
        p = p.detach().reshape(-1).clone(memory_format=torch.contiguous_format)
    return p


def _entry(kind: str, dtype: torch.dtype):
    return getattr(_lib.load(), f"rdetr_add_layernorm_{kind}_{'f32' if dtype == torch.float32 else 'bf16'}")


def add_layer_norm_train(x: torch.Tensor, residual: Optional[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5):
    """Training forward of ``ops.add_layer_norm`` -> (out of x's shape and dtype, stats [rows, 2] fp32 = {mean, rstd}); out has the
    bits of ``ops.add_layer_norm``."""
    _require_device(x, residual, weight, bias)
    if not add_layer_norm_train_supported(x, residual, weight, bias):
        raise _lib.RdetrError("add_layer_norm_train: needs fp32 or bf16 x [..., 256], weight / bias [256] of x's dtype and residual None "
                              "or of x's shape and dtype")
    x, ldx = _rows(x)
    ldr = 256
    if residual is not None:
        residual, ldr = _rows(residual)
    rows = x.numel() // 256
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
    w, b = _param(weight), _param(bias)
    st = _entry("train", x.dtype)(x.data_ptr(), None if residual is None else residual.data_ptr(), w.data_ptr(), b.data_ptr(), rows, 256,
                                  ldx, ldr, 256, float(eps), out.data_ptr(), stats.data_ptr(), _stream_ptr(x))
    _lib.check(st, "rdetr_add_layernorm_train")
    return out, stats


def add_layer_norm_backward(dy: torch.Tensor, x: torch.Tensor, residual: Optional[torch.Tensor], stats: torch.Tensor,
                            weight: torch.Tensor, need_params: bool = True):
    """Gradients of ``add_layer_norm_train`` from the upstream ``dy`` (x's shape) and its ``stats`` -> (dx, dgamma, dbeta): dx of
    x's shape and dtype, contiguous, the gradient of x AND of residual; dgamma / dbeta [256] in the parameter dtype, or None with
    ``need_params=False`` (one launch, no workspace).  Deterministic."""
    _require_device(dy, x, residual, stats, weight)
    if x.dtype not in _DTYPES or x.shape[-1] != 256 or weight.dtype != x.dtype or weight.numel() != 256:
        raise _lib.RdetrError("add_layer_norm_backward: needs fp32 or bf16 x [..., 256] and weight [256] of x's dtype")
    if residual is not None and (residual.shape != x.shape or residual.dtype != x.dtype):
        raise _lib.RdetrError("add_layer_norm_backward: residual must have x's shape and dtype")
    rows = x.numel() // 256
    if dy.shape != x.shape:
        raise _lib.RdetrError("add_layer_norm_backward: dy must have x's shape")
    if stats.dtype != torch.float32 or tuple(stats.shape) != (rows, 2) or not stats.is_contiguous():
        raise _lib.RdetrError("add_layer_norm_backward: stats must be the contiguous fp32 [rows, 2] of add_layer_norm_train")
    if dy.dtype != x.dtype:
        dy = dy.to(x.dtype)
    dy, lddy = _rows(dy)                       # an expanded (out.sum().backward()) or oddly strided gradient: copied
    x, ldx = _rows(x)
    ldr = 256
    if residual is not None:
        residual, ldr = _rows(residual)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    w = _param(weight)
    dgamma = dbeta = ws = None
    nbytes = 0
    if need_params:
        dgamma, dbeta = torch.empty(2, 256, dtype=x.dtype, device=x.device).unbind(0)
        nbytes = int(_lib.load().rdetr_add_layernorm_backward_workspace_bytes(rows))
        ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=x.device)
    st = _entry("backward", x.dtype)(dy.data_ptr(), lddy, x.data_ptr(), ldx, None if residual is None else residual.data_ptr(), ldr,
                                     w.data_ptr(), stats.data_ptr(), rows, 256, None if ws is None else ws.data_ptr(), nbytes,
                                     dx.data_ptr(), None if dgamma is None else dgamma.data_ptr(),
                                     None if dbeta is None else dbeta.data_ptr(), _stream_ptr(x))
    _lib.check(st, "rdetr_add_layernorm_backward")
    return dx, dgamma, dbeta


class AddLayerNormFunction(torch.autograd.Function):
    """Differentiable ``layer_norm(x + residual, (256,), weight, bias, eps)``: ``apply(x, residual, weight, bias, eps)``; residual
    may be None.  Saves x, residual, the row statistics and weight.  The backward returns the SAME dx tensor as the gradient of x
    and of residual (each only where autograd asks) and computes the parameter gradients only when one of them is asked for."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps):
        out, stats = add_layer_norm_train(x, residual, weight, bias, eps)
        ctx.has_residual = residual is not None
        if ctx.has_residual:
            ctx.save_for_backward(x, residual, stats, weight)
        else:
            ctx.save_for_backward(x, stats, weight)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if ctx.has_residual:
            x, residual, stats, weight = ctx.saved_tensors
        else:
            (x, stats, weight), residual = ctx.saved_tensors, None
        need_x, need_r, need_w, need_b = ctx.needs_input_grad[:4]
        dx, dgamma, dbeta = add_layer_norm_backward(grad_out, x, residual, stats, weight, need_params=need_w or need_b)
        return (dx if need_x else None, dx if need_r and residual is not None else None,
                dgamma.view(weight.shape) if need_w else None, dbeta.view(weight.shape) if need_b else None, None)
