"""Training route of the fused feed-forward block ``linear2(relu(linear1(x)))`` (bf16, embed_dim 256, csrc/ffn.hip).

``ops.ffn_k256`` is the inference operator; this module is its training counterpart:

* ``ffn_k256_train``    -- the same kernel body and output bits, plus the hidden activations ``H = relu(bf16(x W1^T + b1))``
  stored as bf16 ``[rows, F]`` (``rdetr_ffn_k256_train_bf16``);
* ``ffn_k256_backward`` -- the data gradient: ``dH = bf16(dY W2)`` zeroed where ``H <= 0``, stored, and ``dx = dH W1`` accumulated in
  fp32 over all of F, from the same kernel with the operands' roles exchanged (``rdetr_ffn_k256_backward_bf16``; no atomics);
* ``FeedForwardFunction`` -- the two as one autograd node.  The weight and bias gradients are library GEMMs / column sums over
  the tensors the two kernels wrote (``dW2 = dY^T H``, ``dW1 = dH^T x``).

Replaces, per block of a training step, two library GEMMs and the ReLU pass of the forward, and the ``dY W2`` GEMM, the ReLU
backward pass over ``[rows, F]`` and the ``dx`` GEMM of the backward.  Saved for backward: x, H and the weights -- what autograd
keeps on the unfused route (the ReLU output).  No CPU path: a tensor that is not on a ROCm device raises.
"""
from __future__ import annotations

import torch

from . import _lib
from .ops import _cptr, _require_device, _rows_view, _stream_ptr, ffn_k256_supported

# _GRAD_BLOCK, _OFFSET_LIMIT and _aligned_rows are also used by amp_train.py (the mixed-precision form of this route): rename them there too
_GRAD_BLOCK = 512                # hidden units per library call of the weight / bias gradient of linear1
_OFFSET_LIMIT = 1 << 31          # H / dH are addressed with 32-bit byte offsets whose top bit marks a row beyond the last


def ffn_train_supported(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor) -> bool:
    """True where the training route applies: what `ops.ffn_k256` needs, bf16 biases, and [rows, F] within 32-bit byte offsets."""
    if not ffn_k256_supported(x, w1, w2):
        return False
    F = w1.shape[0]
    if b1 is None or b2 is None or b1.dtype != torch.bfloat16 or b2.dtype != torch.bfloat16 or b1.numel() != F or b2.numel() != 256:
        return False
    return (x.numel() // 256) * F * 2 < _OFFSET_LIMIT


def _pack(w1: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """(w1 [F, 256], w2 [256, F]) in the kernel's fragment order, on the launch stream and WITHOUT the host synchronisation and the
    cache of `ops.ffn_k256_packed_weights`: an optimizer step changes the weights every iteration, and the only consumer is the
    launch that follows on the same stream."""
    F = w1.shape[0]
    packed = torch.empty(2 * 256 * F, dtype=torch.bfloat16, device=w1.device)
    st = _lib.load().rdetr_ffn_k256_pack_bf16(w1.data_ptr(), w2.data_ptr(), F, packed.data_ptr(), _stream_ptr(w1))
    _lib.check(st, "rdetr_ffn_k256_pack_bf16")
    return packed


def _aligned_rows(t: torch.Tensor, name: str):
    """``t`` [..., C] as evenly strided, 16-byte aligned bf16 rows (copied if it is not: an expanded or oddly strided gradient)
    -> (tensor, rows, leading dimension)."""
    if t.dtype != torch.bfloat16:
        t = t.to(torch.bfloat16)
    try:
        rows, _, ld = _rows_view(t, name)
        ok = ld >= t.shape[-1] and ld % 8 == 0 and t.data_ptr() % 16 == 0
    except _lib.RdetrError:
        ok = False
    if not ok:
        t = t.contiguous()
        rows, _, ld = _rows_view(t, name)
    return t, rows, ld


def ffn_k256_train(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor):
    """Training forward of ``ops.ffn_k256`` -> (out [..., 256], H [..., F]), both bf16; out has the bits of ``ops.ffn_k256``."""
    _require_device(x, w1, b1, w2, b2)
    if not ffn_train_supported(x, w1, b1, w2, b2):
        raise _lib.RdetrError("ffn_k256_train: needs bf16 x [..., 256] (evenly strided 16-byte aligned rows), w1 [F, 256], w2 [256, F], "
                              "b1 [F], b2 [256], d_ffn % 64 == 0 (<= 4096) and rows * d_ffn * 2 < 2^31")
    F = w1.shape[0]
    rows, _, ldx = _rows_view(x, "ffn_k256_train")
    out = torch.empty(*x.shape[:-1], 256, dtype=x.dtype, device=x.device)
    hid = torch.empty(*x.shape[:-1], F, dtype=x.dtype, device=x.device)
    packed = _pack(w1, w2)
    st = _lib.load().rdetr_ffn_k256_train_bf16(x.data_ptr(), ldx, packed.data_ptr(), _cptr(b1), _cptr(b2), rows, F, out.data_ptr(), 256,
                                               hid.data_ptr(), F, _stream_ptr(x))
    _lib.check(st, "rdetr_ffn_k256_train_bf16")
    return out, hid


def ffn_k256_backward(dy: torch.Tensor, hid: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor):
    """Data gradient of the block from the upstream ``dy`` [..., 256] and the ``hid`` of `ffn_k256_train` -> (dx [..., 256],
    dH [..., F]) bf16: ``dH = bf16(dy w2) * (hid > 0)``, ``dx = dH w1`` (fp32 accumulation over all of F).  Deterministic."""
    _require_device(dy, hid, w1, w2)
    F = w1.shape[0] if w1.dim() == 2 else 0
    if (w1.dtype != torch.bfloat16 or w2.dtype != torch.bfloat16 or tuple(w1.shape) != (F, 256) or tuple(w2.shape) != (256, F)
            or F % 64 or not 0 < F <= 4096):
        raise _lib.RdetrError("ffn_k256_backward: needs bf16 w1 [F, 256] and w2 [256, F], d_ffn % 64 == 0 (<= 4096)")
    if hid.dtype != torch.bfloat16 or hid.shape[-1] != F or dy.shape[-1] != 256 or tuple(hid.shape[:-1]) != tuple(dy.shape[:-1]):
        raise _lib.RdetrError("ffn_k256_backward: dy must be [..., 256] and hid bf16 [..., F] over the same rows")
    dy, rows, lddy = _aligned_rows(dy, "ffn_k256_backward")
    hid, hrows, ldh = _aligned_rows(hid, "ffn_k256_backward")
    if rows * max(ldh, F) * 2 >= _OFFSET_LIMIT:
        raise _lib.RdetrError("ffn_k256_backward: rows * d_ffn * 2 must stay below 2^31")
    dx = torch.empty(*dy.shape[:-1], 256, dtype=torch.bfloat16, device=dy.device)
    dh = torch.empty(*dy.shape[:-1], F, dtype=torch.bfloat16, device=dy.device)
    # the same kernel with the roles exchanged: dy for x, w2^T [F, 256] for w1, w1^T [256, F] for w2
    packed_t = _pack(w2.t().contiguous(), w1.t().contiguous())
    st = _lib.load().rdetr_ffn_k256_backward_bf16(dy.data_ptr(), lddy, packed_t.data_ptr(), hid.data_ptr(), ldh, rows, F, dh.data_ptr(), F,
                                                  dx.data_ptr(), 256, _stream_ptr(dy))
    _lib.check(st, "rdetr_ffn_k256_backward_bf16")
    return dx, dh


class FeedForwardFunction(torch.autograd.Function):
    """Differentiable ``linear2(relu(linear1(x)))`` for bf16 x [..., 256]: ``apply(x, w1, b1, w2, b2)``.  Saves x, the hidden
    activations and the two weights; returns gradients for all five inputs (those autograd asks for).  The backward kernel runs
    only when x, w1 or b1 needs a gradient."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        out, hid = ffn_k256_train(x, w1, b1, w2, b2)
        ctx.save_for_backward(x, hid, w1, w2)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, hid, w1, w2 = ctx.saved_tensors
        need_x, need_w1, need_b1, need_w2, need_b2 = ctx.needs_input_grad
        F = w1.shape[0]
        dy, rows, lddy = _aligned_rows(grad_out, "FeedForwardFunction")     # expanded (out.sum()) or oddly strided: copied
        dy2 = dy.as_strided((rows, 256), (lddy, 1))
        dx = dw1 = db1 = dw2 = db2 = None
        if need_w2:
            dw2 = dy2.t().mm(hid.view(rows, F))
        if need_b2:
            db2 = dy2.sum(0)
        if need_x or need_w1 or need_b1:
            dx, dh = ffn_k256_backward(dy, hid, w1, w2)
            dh = dh.view(rows, F)
            # dW1 and db1 are taken from dH in column blocks.  This is the point where the most is alive (x, H, dH, dx), and the
            # library calls may hold a temporary of the size of their [rows, .] operand: a block keeps that to a fraction of
            # [rows, F].  Blocks of hidden units are independent outputs, so nothing is summed or rounded twice.
            blocks = [slice(j, min(j + _GRAD_BLOCK, F)) for j in range(0, F, _GRAD_BLOCK)]
            if need_w1:
                _, _, ldx = _rows_view(x, "FeedForwardFunction")
                xt = x.as_strided((rows, 256), (ldx, 1)).t()
                dw1 = torch.cat([xt.mm(dh[:, b]) for b in blocks], 1).t()      # x^T dH, transposed: the form autograd uses
            if need_b1:
                db1 = torch.cat([dh[:, b].sum(0) for b in blocks])
            dx = dx.view(x.shape) if need_x else None
        return dx, dw1, db1, dw2, db2
