"""Mixed-precision forms of the fused LayerNorm and feed-forward training routes: ``torch.autocast(bfloat16)`` over fp32 parameters.

``ln_train`` and ``ffn_train`` want every operand in one dtype -- a network converted with ``.to(bfloat16)``.  Under bf16 autocast
with fp32 master parameters the operands differ instead: the residual stream is fp32, every linear output bf16, the LayerNorm
parameters fp32 and its result fp32; the feed-forward block reads the fp32 stream and returns bf16.  This module runs those calls
through the same kernel bodies (csrc/layernorm.hip, csrc/ffn.hip) instantiated for the mixed operand types:

* ``add_layer_norm_mixed_train`` / ``add_layer_norm_mixed_backward`` / ``AddLayerNormMixedFunction`` -- x and the residual each
  fp32 or bf16, parameters and result fp32.  The sum is formed in fp32 and never stored; the backward writes the fp32 ``dx`` and, in
  the same pass, its bf16 rounding for a bf16 operand (autograd wants each gradient in its operand's dtype; no cast pass).
* ``ffn_pack_f32`` -- the fragment-order weights straight from the fp32 parameters, read through strides (the backward's transposed
  operands in place) and rounded on the way; the biases rounded by the same launch.
* ``ffn_mixed_train`` / ``ffn_mixed_backward`` / ``FeedForwardMixedFunction`` -- fp32 x is rounded as the kernel loads it, the rounded
  copy stored for ``dW1``; ``dx`` leaves the data-gradient kernel as the unrounded fp32 sum.  bf16 x takes ``ffn_train``'s kernels.

``transformer.add_norm`` / ``feed_forward`` and the MSDA module's output stage come here under ``ln_train_fused`` /
``ffn_train_fused`` while ``autocast_bf16_active()`` and the same-dtype route does not apply.  No CPU path: a tensor that is not on a
ROCm device raises.
"""
from __future__ import annotations

import functools
from typing import Optional

import torch

from . import _lib
from .ffn_train import _GRAD_BLOCK, _OFFSET_LIMIT, _aligned_rows
from .ln_train import _param, _rows
from .ops import _require_device, _rows_view, _stream_ptr

_DTYPES = (torch.float32, torch.bfloat16)
F32, BF16 = torch.float32, torch.bfloat16

try:                                             # the forward's autocast state restored around the backward's library calls
    _custom_fwd = functools.partial(torch.amp.custom_fwd, device_type="cuda")
    _custom_bwd = functools.partial(torch.amp.custom_bwd, device_type="cuda")
except AttributeError:                           # the older spelling
    from torch.cuda.amp import custom_bwd as _custom_bwd, custom_fwd as _custom_fwd


def autocast_bf16_active() -> bool:
    """True inside ``torch.autocast("cuda", dtype=torch.bfloat16)``."""
    try:
        return bool(torch.is_autocast_enabled("cuda")) and torch.get_autocast_dtype("cuda") == BF16
    except (TypeError, AttributeError):          # the older spelling: no device argument
        return bool(torch.is_autocast_enabled()) and torch.get_autocast_gpu_dtype() == BF16


# ------------------------------------------------------------------------------------------------------ add + LayerNorm
def mixed_norm_operands_ok(x, residual, weight, bias, autocast: bool) -> bool:
    """The dtype / shape rule of the mixed add + LayerNorm route, on tensors of any device: 256 channels, x and the residual (None
    or of x's shape) each fp32 or bf16, fp32 parameters of 256 elements -- and not "everything fp32 outside autocast", which is
    ``ln_train``'s case."""
    if not (torch.is_tensor(x) and x.dtype in _DTYPES and x.dim() >= 1 and x.shape[-1] == 256):
        return False
    if weight is None or bias is None:
        return False
    for p in (weight, bias):
        if p.dtype != F32 or p.numel() != 256:
            return False
    if residual is not None and not (residual.dtype in _DTYPES and residual.shape == x.shape):
        return False
    all_fp32 = x.dtype == F32 and (residual is None or residual.dtype == F32)
    return autocast or not all_fp32


def add_layer_norm_mixed_supported(x: torch.Tensor, residual: Optional[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor) -> bool:
    """True where the mixed route applies: ROCm tensors that satisfy `mixed_norm_operands_ok` under the current autocast state."""
    if not (torch.is_tensor(x) and x.is_cuda and weight is not None and bias is not None and weight.is_cuda and bias.is_cuda
            and (residual is None or residual.is_cuda)):
        return False
    return mixed_norm_operands_ok(x, residual, weight, bias, autocast_bf16_active())


def add_layer_norm_mixed_train(x: torch.Tensor, residual: Optional[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor,
                               eps: float = 1e-5):
    """``layer_norm(x.float() + residual.float(), (256,), weight, bias, eps)`` for x / residual each fp32 or bf16 and fp32 parameters
    -> (out fp32 of x's shape, stats [rows, 2] fp32 = {mean, rstd})."""
    _require_device(x, residual, weight, bias)
    if not mixed_norm_operands_ok(x, residual, weight, bias, True):
        raise _lib.RdetrError("add_layer_norm_mixed_train: needs x [..., 256] and residual (None or of x's shape) each fp32 or bf16, "
                              "and fp32 weight / bias [256]")
    x, ldx = _rows(x)
    ldr = 256
    if residual is not None:
        residual, ldr = _rows(residual)
    rows = x.numel() // 256
    out = torch.empty(x.shape, dtype=F32, device=x.device)
    stats = torch.empty(rows, 2, dtype=F32, device=x.device)
    w, b = _param(weight), _param(bias)
    st = _lib.load().rdetr_add_layernorm_train_mixed(
        x.data_ptr(), int(x.dtype == BF16), ldx, None if residual is None else residual.data_ptr(),
        int(residual is not None and residual.dtype == BF16), ldr, w.data_ptr(), b.data_ptr(), rows, 256, float(eps), out.data_ptr(), 256,
        stats.data_ptr(), _stream_ptr(x))
    _lib.check(st, "rdetr_add_layernorm_train_mixed")
    return out, stats


def add_layer_norm_mixed_backward(dy: torch.Tensor, x: torch.Tensor, residual: Optional[torch.Tensor], stats: torch.Tensor,
                                  weight: torch.Tensor, need_params: bool = True):
    """Gradients of `add_layer_norm_mixed_train` from the upstream ``dy`` (x's shape; fp32) and its ``stats`` -> (dx_f32, dx_bf16,
    dgamma, dbeta).  dx_f32 is the gradient of every fp32 operand, dx_bf16 -- the same values rounded to bf16 by the same pass -- of
    every bf16 one; the one no operand needs is None.  dgamma / dbeta are fp32 [256], or None with ``need_params=False`` (one
    launch, no workspace).  Deterministic."""
    _require_device(dy, x, residual, stats, weight)
    if not mixed_norm_operands_ok(x, residual, weight, weight, True):
        raise _lib.RdetrError("add_layer_norm_mixed_backward: needs x [..., 256] and residual (None or of x's shape) each fp32 or bf16, "
                              "and fp32 weight [256]")
    rows = x.numel() // 256
    if dy.shape != x.shape:
        raise _lib.RdetrError("add_layer_norm_mixed_backward: dy must have x's shape")
    if stats.dtype != F32 or tuple(stats.shape) != (rows, 2) or not stats.is_contiguous():
        raise _lib.RdetrError("add_layer_norm_mixed_backward: stats must be the contiguous fp32 [rows, 2] of add_layer_norm_mixed_train")
    if dy.dtype != F32:
        dy = dy.to(F32)
    dy, lddy = _rows(dy)                       # an expanded (out.sum().backward()) or oddly strided gradient: copied
    x, ldx = _rows(x)
    ldr = 256
    if residual is not None:
        residual, ldr = _rows(residual)
    dtypes = {x.dtype} | (set() if residual is None else {residual.dtype})
    dx = torch.empty(x.shape, dtype=F32, device=x.device) if F32 in dtypes else None
    dxb = torch.empty(x.shape, dtype=BF16, device=x.device) if BF16 in dtypes else None
    w = _param(weight)
    dgamma = dbeta = ws = None
    nbytes = 0
    lib = _lib.load()
    if need_params:
        dgamma, dbeta = torch.empty(2, 256, dtype=F32, device=x.device).unbind(0)
        nbytes = int(lib.rdetr_add_layernorm_backward_workspace_bytes(rows))
        ws = torch.empty(max(nbytes // 4, 4), dtype=F32, device=x.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    st = lib.rdetr_add_layernorm_backward_mixed(
        dy.data_ptr(), lddy, x.data_ptr(), int(x.dtype == BF16), ldx, ptr(residual), int(residual is not None and residual.dtype == BF16),
        ldr, w.data_ptr(), stats.data_ptr(), rows, 256, ptr(ws), nbytes, ptr(dx), ptr(dxb), ptr(dgamma), ptr(dbeta), _stream_ptr(x))
    _lib.check(st, "rdetr_add_layernorm_backward_mixed")
    return dx, dxb, dgamma, dbeta


class AddLayerNormMixedFunction(torch.autograd.Function):
    """Differentiable ``layer_norm(x + residual, (256,), weight, bias, eps)`` as bf16 autocast computes it (the sum and the result
    fp32) for x / residual each fp32 or bf16 and fp32 parameters: ``apply(x, residual, weight, bias, eps)``; residual may be None.
    Saves x, residual, the row statistics and weight.  The backward hands each operand its gradient in its own dtype -- the SAME
    tensor to both where they share one -- and computes the parameter gradients only when one of them is asked for."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps):
        out, stats = add_layer_norm_mixed_train(x, residual, weight, bias, eps)
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
        dx, dxb, dgamma, dbeta = add_layer_norm_mixed_backward(grad_out, x, residual, stats, weight, need_params=need_w or need_b)
        pick = lambda t: dxb if t.dtype == BF16 else dx
        return (pick(x) if need_x else None, pick(residual) if need_r and residual is not None else None,
                dgamma.view(weight.shape) if need_w else None, dbeta.view(weight.shape) if need_b else None, None)


# ---------------------------------------------------------------------------------------------------------- feed-forward
def _ffn_dims_ok(w1, b1, w2, b2) -> int:
    """d_ffn if (w1 [F, 256], b1 [F], w2 [256, F], b2 [256]) are fp32 of the kernel's shapes, else 0."""
    if w1 is None or w2 is None or w1.dim() != 2 or w2.dim() != 2:
        return 0
    F = w1.shape[0]
    if tuple(w1.shape) != (F, 256) or tuple(w2.shape) != (256, F) or F % 64 or not 0 < F <= 4096:
        return 0
    if w1.dtype != F32 or w2.dtype != F32:
        return 0
    if b1 is None or b2 is None or b1.dtype != F32 or b2.dtype != F32 or b1.numel() != F or b2.numel() != 256:
        return 0
    return F


def ffn_mixed_supported(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor) -> bool:
    """True where the mixed feed-forward route applies: ROCm tensors, x fp32 or bf16 [..., 256] in evenly strided 16-byte aligned
    rows, fp32 parameters of the kernel's shapes (d_ffn % 64 == 0, <= 4096) and [rows, d_ffn] within 32-bit byte offsets."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype in _DTYPES and x.dim() >= 2 and x.shape[-1] == 256):
        return False
    F = _ffn_dims_ok(w1, b1, w2, b2)
    if not F or not all(p.is_cuda for p in (w1, b1, w2, b2)):
        return False
    try:
        rows, _, ld = _rows_view(x, "ffn_mixed")
    except _lib.RdetrError:
        return False
    if ld < 256 or (ld * x.element_size()) % 16 or x.data_ptr() % 16:
        return False
    return rows * F * 2 < _OFFSET_LIMIT


def ffn_pack_f32(w1: torch.Tensor, w2: torch.Tensor, b1: Optional[torch.Tensor] = None, b2: Optional[torch.Tensor] = None):
    """fp32 (w1 [F, 256], w2 [256, F]) of ANY strides -> the bf16 fragment order of ``rdetr_ffn_k256_pack_bf16`` on their rounded
    values, in one launch on the current stream; ``ffn_pack_f32(w2.t(), w1.t())`` reads the backward's operands in place.  With
    b1 [F] / b2 [256] also their bf16 roundings -> (packed, b1_bf16, b2_bf16), else (packed, None, None)."""
    _require_device(w1, w2, b1, b2)
    F = w1.shape[0] if w1.dim() == 2 else 0
    if (w1.dtype != F32 or w2.dtype != F32 or tuple(w1.shape) != (F, 256) or w2.dim() != 2 or tuple(w2.shape) != (256, F)
            or (b1 is None) != (b2 is None)):
        raise _lib.RdetrError("ffn_pack_f32: needs fp32 w1 [F, 256] and w2 [256, F], and b1 / b2 both or neither")
    if min(w1.stride() + w2.stride()) < 1:
        w1, w2 = w1.contiguous(), w2.contiguous()
    nb = 0
    if b1 is not None:
        if b1.dtype != F32 or b2.dtype != F32 or b1.numel() != F or b2.numel() != 256:
            raise _lib.RdetrError("ffn_pack_f32: needs fp32 b1 [F] and b2 [256]")
        b1, b2, nb = b1.reshape(-1).contiguous(), b2.reshape(-1).contiguous(), F + 256
    buf = torch.empty(2 * 256 * F + nb, dtype=BF16, device=w1.device)         # one allocation: the fragments, then (b1, b2)
    packed, biases = buf[:2 * 256 * F], buf[2 * 256 * F:]
    st = _lib.load().rdetr_ffn_k256_pack_f32(w1.data_ptr(), w1.stride(0), w1.stride(1), w2.data_ptr(), w2.stride(0), w2.stride(1),
                                             None if b1 is None else b1.data_ptr(), None if b2 is None else b2.data_ptr(), F,
                                             packed.data_ptr(), biases.data_ptr() if nb else None, _stream_ptr(w1))
    _lib.check(st, "rdetr_ffn_k256_pack_f32")
    return (packed, biases[:F], biases[F:]) if nb else (packed, None, None)


def ffn_mixed_train(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor):
    """Training forward of the block for fp32 parameters -> (out [..., 256] bf16, H [..., F] bf16, x as bf16).  fp32 x is rounded
    by the kernel as it loads the rows and the rounded copy comes back as the third result (``rdetr_ffn_k256_train_xf32_bf16``); bf16 x
    goes through ``rdetr_ffn_k256_train_bf16`` and is returned as it is.  out and H have the bits of `ffn_train.ffn_k256_train` on the
    operands rounded to bf16."""
    _require_device(x, w1, b1, w2, b2)
    if not ffn_mixed_supported(x, w1, b1, w2, b2):
        raise _lib.RdetrError("ffn_mixed_train: needs fp32 or bf16 x [..., 256] (evenly strided 16-byte aligned rows), fp32 w1 [F, 256], "
                              "w2 [256, F], b1 [F], b2 [256], d_ffn % 64 == 0 (<= 4096) and rows * d_ffn * 2 < 2^31")
    F = w1.shape[0]
    rows, _, ldx = _rows_view(x, "ffn_mixed_train")
    packed, b1b, b2b = ffn_pack_f32(w1, w2, b1, b2)
    out = torch.empty(*x.shape[:-1], 256, dtype=BF16, device=x.device)
    hid = torch.empty(*x.shape[:-1], F, dtype=BF16, device=x.device)
    lib = _lib.load()
    if x.dtype == F32:
        xlp = torch.empty(x.shape, dtype=BF16, device=x.device)
        st = lib.rdetr_ffn_k256_train_xf32_bf16(x.data_ptr(), ldx, packed.data_ptr(), b1b.data_ptr(), b2b.data_ptr(), rows, F,
                                                out.data_ptr(), 256, hid.data_ptr(), F, xlp.data_ptr(), 256, _stream_ptr(x))
        _lib.check(st, "rdetr_ffn_k256_train_xf32_bf16")
    else:
        xlp = x
        st = lib.rdetr_ffn_k256_train_bf16(x.data_ptr(), ldx, packed.data_ptr(), b1b.data_ptr(), b2b.data_ptr(), rows, F, out.data_ptr(),
                                           256, hid.data_ptr(), F, _stream_ptr(x))
        _lib.check(st, "rdetr_ffn_k256_train_bf16")
    return out, hid, xlp


def ffn_mixed_backward(dy: torch.Tensor, hid: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, fp32_dx: bool = True):
    """Data gradient of the block from the upstream ``dy`` [..., 256], the ``hid`` of `ffn_mixed_train` and the fp32 weights ->
    (dx [..., 256], dH [..., F] bf16): ``dH = bf16(dy bf16(w2)) * (hid > 0)``, ``dx = dH bf16(w1)`` summed in fp32 over all of F and
    returned unrounded (``fp32_dx``, ``rdetr_ffn_k256_backward_dxf32_bf16``) or rounded once to bf16.  The weights are packed from
    the parameters in place, transposed through their strides.  Deterministic."""
    _require_device(dy, hid, w1, w2)
    F = w1.shape[0] if w1.dim() == 2 else 0
    if (w1.dtype != F32 or w2.dtype != F32 or tuple(w1.shape) != (F, 256) or tuple(w2.shape) != (256, F) or F % 64 or not 0 < F <= 4096):
        raise _lib.RdetrError("ffn_mixed_backward: needs fp32 w1 [F, 256] and w2 [256, F], d_ffn % 64 == 0 (<= 4096)")
    if hid.dtype != BF16 or hid.shape[-1] != F or dy.shape[-1] != 256 or tuple(hid.shape[:-1]) != tuple(dy.shape[:-1]):
        raise _lib.RdetrError("ffn_mixed_backward: dy must be [..., 256] and hid bf16 [..., F] over the same rows")
    dy, rows, lddy = _aligned_rows(dy, "ffn_mixed_backward")
    hid, _, ldh = _aligned_rows(hid, "ffn_mixed_backward")
    if rows * max(ldh, F) * 2 >= _OFFSET_LIMIT:
        raise _lib.RdetrError("ffn_mixed_backward: rows * d_ffn * 2 must stay below 2^31")
    dx = torch.empty(*dy.shape[:-1], 256, dtype=F32 if fp32_dx else BF16, device=dy.device)
    dh = torch.empty(*dy.shape[:-1], F, dtype=BF16, device=dy.device)
    packed_t, _, _ = ffn_pack_f32(w2.t(), w1.t())            # the same kernel with the roles exchanged: w2^T for w1, w1^T for w2
    lib = _lib.load()
    entry, name = ((lib.rdetr_ffn_k256_backward_dxf32_bf16, "rdetr_ffn_k256_backward_dxf32_bf16") if fp32_dx
                   else (lib.rdetr_ffn_k256_backward_bf16, "rdetr_ffn_k256_backward_bf16"))
    st = entry(dy.data_ptr(), lddy, packed_t.data_ptr(), hid.data_ptr(), ldh, rows, F, dh.data_ptr(), F, dx.data_ptr(), 256,
               _stream_ptr(dy))
    _lib.check(st, name)
    return dx, dh


class FeedForwardMixedFunction(torch.autograd.Function):
    """Differentiable ``linear2(relu(linear1(x)))`` as bf16 autocast computes it, for fp32 parameters and fp32 or bf16 x [..., 256]:
    ``apply(x, w1, b1, w2, b2)`` -> bf16.  Saves x's bf16 copy (written by the forward kernel), the hidden activations and the fp32
    weights themselves -- no bf16 weight copies.  Gradients: x's in x's dtype (fp32: the unrounded sum), the parameters' fp32; the
    weight and bias gradients are library calls on the bf16 tensors the kernels wrote, in `ffn_train`'s column blocks.  The backward
    kernel runs only when x, w1 or b1 needs a gradient."""

    @staticmethod
    @_custom_fwd
    def forward(ctx, x, w1, b1, w2, b2):
        out, hid, xlp = ffn_mixed_train(x, w1, b1, w2, b2)
        ctx.save_for_backward(xlp, hid, w1, w2)
        ctx.x_fp32 = x.dtype == F32
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @_custom_bwd
    def backward(ctx, grad_out):
        xlp, hid, w1, w2 = ctx.saved_tensors
        need_x, need_w1, need_b1, need_w2, need_b2 = ctx.needs_input_grad
        F = w1.shape[0]
        dy, rows, lddy = _aligned_rows(grad_out, "FeedForwardMixedFunction")  # expanded (out.sum()) or oddly strided: copied
        dy2 = dy.as_strided((rows, 256), (lddy, 1))
        dx = dw1 = db1 = dw2 = db2 = None
        if need_w2:
            dw2 = dy2.t().mm(hid.view(rows, F)).to(F32)
        if need_b2:
            db2 = dy2.sum(0).to(F32)
        if need_x or need_w1 or need_b1:
            dx, dh = ffn_mixed_backward(dy, hid, w1, w2, fp32_dx=ctx.x_fp32)
            dh = dh.view(rows, F)
            blocks = [slice(j, min(j + _GRAD_BLOCK, F)) for j in range(0, F, _GRAD_BLOCK)]   # see ffn_train.FeedForwardFunction
            if need_w1:
                _, _, ldx = _rows_view(xlp, "FeedForwardMixedFunction")
                xt = xlp.as_strided((rows, 256), (ldx, 1)).t()
                dw1 = torch.cat([xt.mm(dh[:, b]) for b in blocks], 1).t().to(F32)
            if need_b1:
                db1 = torch.cat([dh[:, b].sum(0) for b in blocks]).to(F32)
            dx = dx.view(xlp.shape) if need_x else None
        return dx, dw1, db1, dw2, db2
