"""What follows each convolution of the ResNet backbone, as one kernel call each (csrc/backbone.hip).

``frozen_bn_act(x, scale, shift, residual=None, relu=True, out=None)`` is ``act(x * scale[c] + shift[c] (+ residual))`` with its
gradient; ``stem_bn_relu_maxpool(x, scale, shift)`` is ``max_pool2d(relu(x * scale[c] + shift[c]), 3, 2, 1)``, forward only.  Tensors
are fp32 or bf16, dense NCHW or dense channels-last (anything else is copied into the layout it is nearest to); ``scale`` and
``shift`` are fp32 ``[C]`` and take no gradient (they come from frozen buffers).  In fp32 the results are torch's for the reference's
operator sequence, bit for bit, forward and backward.

The backward needs the OUTPUT and ``scale`` only, so ``out=x`` (in place on the convolution's result) is always possible; the
modules use it everywhere.  CPU tensors raise ``RdetrError``: the modules' ``forward_torch`` is the CPU path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _lib

_DTYPES = {torch.float32: "f32", torch.bfloat16: "bf16"}


def _need_device(*tensors: Optional[Tensor]) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.RdetrError("relation_detr_amd.backbones kernels need tensors on a ROCm device (got a CPU tensor); "
                                  "the modules' torch route is the CPU path")


def _channels_last(x: Tensor) -> Optional[bool]:
    """False for dense NCHW, True for dense channels-last, None for neither.  A tensor that is both (C = 1 or H * W = 1) is NCHW."""
    if x.is_contiguous():
        return False
    if x.is_contiguous(memory_format=torch.channels_last):
        return True
    return None


def _dense(x: Tensor, channels_last: Optional[bool] = None) -> Tuple[Tensor, bool]:
    """``x`` dense in the asked layout (None: its own, or NCHW when it has none) and on the 16-byte grid; copied only when needed."""
    own = _channels_last(x)
    want = (own if own is not None else False) if channels_last is None else channels_last
    if own is None or (own != want and not (x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last))):
        x = x.contiguous(memory_format=torch.channels_last if want else torch.contiguous_format)
    if x.data_ptr() % 16:
        x = x.clone(memory_format=torch.preserve_format)
    return x, want


def _constants(scale: Tensor, shift: Optional[Tensor], C: int) -> Tuple[Tensor, Optional[Tensor]]:
    done = []
    for name, t in (("scale", scale), ("shift", shift)):
        if t is None:
            done.append(None)
            continue
        if t.dtype != torch.float32 or t.numel() != C:
            raise ValueError(f"frozen_bn_act: {name} is fp32 [C = {C}], got {t.dtype} {tuple(t.shape)}")
        if t.requires_grad:
            raise ValueError(f"frozen_bn_act: {name} takes no gradient (the norm is frozen)")
        t = t.reshape(C).contiguous()
        done.append(t.clone() if t.data_ptr() % 16 else t)
    return done[0], done[1]


def _shape(x: Tensor) -> Tuple[int, int, int, int]:
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"expected a non-empty [B, C, H, W] tensor, got {tuple(x.shape)}")
    if x.dtype not in _DTYPES:
        raise ValueError(f"expected float32 or bfloat16, got {x.dtype}")
    return tuple(int(s) for s in x.shape)


def _stream(x: Tensor) -> int:
    return torch.cuda.current_stream(x.device).cuda_stream


def frozen_bn_act_forward(x: Tensor, scale: Tensor, shift: Tensor, residual: Optional[Tensor] = None, relu: bool = True,
                          out: Optional[Tensor] = None) -> Tensor:
    """The forward kernel alone, no autograd.  ``out``: None for a fresh tensor in ``x``'s layout, ``x`` itself for in place, or a
    dense tensor of ``x``'s shape, dtype and layout."""
    _need_device(x, scale, shift, residual, out)
    B, C, H, W = _shape(x)
    in_place = out is x
    dense, channels_last = _dense(x)
    if in_place and dense is not x:
        raise ValueError("frozen_bn_act: in place needs a dense NCHW or channels-last tensor on the 16-byte grid")
    scale, shift = _constants(scale, shift, C)
    if residual is not None:
        if residual.shape != x.shape:
            raise ValueError(f"frozen_bn_act: residual {tuple(residual.shape)} against x {tuple(x.shape)}")
        residual, _ = _dense(residual.to(x.dtype), channels_last)
    if in_place:
        out = dense
    elif out is None:
        out = torch.empty_like(dense)
    elif out.shape != x.shape or out.dtype != x.dtype or _dense(out, channels_last)[0] is not out:
        raise ValueError("frozen_bn_act: out has x's shape and dtype and is dense in x's layout")
    fn = getattr(_lib.load(), "rdetr_frozen_bn_act_" + _DTYPES[x.dtype])
    _lib.check(fn(dense.data_ptr(), scale.data_ptr(), shift.data_ptr(), None if residual is None else residual.data_ptr(), B, C, H, W,
                  int(channels_last), int(bool(relu)), out.data_ptr(), _stream(x)), "rdetr_frozen_bn_act")
    return out


def frozen_bn_act_backward(dy: Tensor, y: Optional[Tensor], scale: Tensor, relu: bool = True,
                           want_dres: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """``(dx, dres)`` from the output gradient, the saved output and ``scale``; ``dres`` is None unless asked for.  With ``relu`` off
    ``y`` is not read and may be None."""
    _need_device(dy, y, scale)
    B, C, H, W = _shape(dy)
    if relu:
        if y is None or y.shape != dy.shape or y.dtype != dy.dtype:
            raise ValueError("frozen_bn_act_backward: y has dy's shape and dtype")
        y, channels_last = _dense(y)
        dy, _ = _dense(dy, channels_last)
    else:
        y = None
        dy, channels_last = _dense(dy)
    scale, _ = _constants(scale, None, C)
    dx = torch.empty_like(dy)
    dres = torch.empty_like(dy) if want_dres else None
    fn = getattr(_lib.load(), "rdetr_frozen_bn_act_backward_" + _DTYPES[dy.dtype])
    _lib.check(fn(dy.data_ptr(), None if y is None else y.data_ptr(), scale.data_ptr(), B, C, H, W, int(channels_last), int(bool(relu)),
                  dx.data_ptr(), None if dres is None else dres.data_ptr(), _stream(dy)), "rdetr_frozen_bn_act_backward")
    return dx, dres


class FrozenBNActFunction(torch.autograd.Function):
    """``apply(x, scale, shift, residual, relu, in_place)``.  Saves the output (and ``scale``) only."""

    @staticmethod
    def forward(ctx, x, scale, shift, residual, relu, in_place):
        y = frozen_bn_act_forward(x, scale, shift, residual, relu, x if in_place else None)
        if in_place:
            ctx.mark_dirty(x)
        ctx.relu = bool(relu)
        ctx.save_for_backward(y if relu else None, scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, scale = ctx.saved_tensors
        dx, dres = frozen_bn_act_backward(dy, y, scale, ctx.relu, want_dres=ctx.needs_input_grad[3])
        return dx if ctx.needs_input_grad[0] else None, None, None, dres, None, None


def frozen_bn_act(x: Tensor, scale: Tensor, shift: Tensor, residual: Optional[Tensor] = None, relu: bool = True,
                  out: Optional[Tensor] = None) -> Tensor:
    """``act(x * scale[c] + shift[c] (+ residual))`` with its gradient for ``x`` and ``residual``.  ``out=x`` runs in place (``x`` must
    then be dense; a convolution's result is).  An ``out`` other than ``x`` is for calls that need no gradient."""
    if out is not None and out is not x and torch.is_grad_enabled() and (x.requires_grad or (residual is not None and residual.requires_grad)):
        raise ValueError("frozen_bn_act: with a gradient, out is None or x itself")
    if out is not None and out is not x:
        return frozen_bn_act_forward(x, scale, shift, residual, relu, out)
    return FrozenBNActFunction.apply(x, scale, shift, residual, relu, out is x)


def stem_bn_relu_maxpool(x: Tensor, scale: Tensor, shift: Tensor) -> Tensor:
    """``max_pool2d(relu(x * scale[c] + shift[c]), 3, 2, 1)`` in one launch: ``[B, C, H, W] -> [B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1]``
    in ``x``'s layout.  Forward only: an ``x`` that needs a gradient is refused (the module then runs the stem with torch's
    operators)."""
    _need_device(x, scale, shift)
    if torch.is_grad_enabled() and x.requires_grad:
        raise _lib.RdetrError("stem_bn_relu_maxpool is forward only; the input needs a gradient")
    B, C, H, W = _shape(x)
    dense, channels_last = _dense(x)
    scale, shift = _constants(scale, shift, C)
    out = torch.empty((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=x.dtype, device=x.device,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    fn = getattr(_lib.load(), "rdetr_stem_pool_" + _DTYPES[x.dtype])
    _lib.check(fn(dense.data_ptr(), scale.data_ptr(), shift.data_ptr(), B, C, H, W, int(channels_last), out.data_ptr(), _stream(x)),
               "rdetr_stem_pool")
    return out
