"""Host side of the short-row projection + residual + LayerNorm kernel (csrc/rowtail.hip), the half of ``ops.linear_ln_k256`` that
serves the decoder: a few hundred to a few thousand rows of an attention output projection (K = 256), optionally with ``out + pos``
from the same launch.

``ops.linear_ln_k256`` is the checked entry; everything here runs inside it (the packing launches included)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib

# Row count up to which the 32-row-per-workgroup kernel serves ``linear_ln_k256``; above it the 256-row-tile kernel of
# csrc/linear.hip does (no extras).  The measured crossover of the two (tools/time_rowtail.py, profiles/r19/time_rowtail.txt;
# DESIGN.md 4.7): the short-row kernel wins every run up to 28,800 rows (15.3 against 16.9 us) and loses at 44,646 (21.0 against 18.4).
MAX_ROWS = 28800


def takes(rows: int) -> bool:
    """True where ``ops.linear_ln_k256`` runs the short-row kernel."""
    return rows <= MAX_ROWS


def _vector(t: Optional[torch.Tensor], name: str, keep) -> Optional[int]:
    """Device pointer of a bf16 [256] parameter vector, contiguous and 16-byte aligned (a copy, kept alive, where it is not)."""
    if t is None:
        return None
    if t.dtype != torch.bfloat16 or t.numel() != 256:
        raise _lib.RdetrError(f"linear_ln_k256: {name} must be bf16 [256]")
    t = t.detach()
    if not t.is_contiguous() or t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
        keep.append(t)
    return t.data_ptr()


def _rows(t: torch.Tensor, rows: int, what: str, rows_view):
    r, C, ld = rows_view(t, "linear_ln_k256")
    if r != rows or C != 256 or ld % 8 or t.data_ptr() % 16 or t.dtype != torch.bfloat16:
        raise _lib.RdetrError(f"linear_ln_k256: {what} must be bf16 [..., 256] with one row per input row, 16-byte aligned rows")
    return ld


def linear_ln_rows(x, weight, bias, residual, gamma, beta, eps, out, extra, *, rows_view, packed, keep):
    """The launch behind ``ops.linear_ln_k256`` for short inputs; ``packed``: the weight in fragment order.  ``extra``: None or a dict --
    ``"pos"`` (bf16, x's shape) asks for ``extra["out_plus_pos"] = out + pos`` (a tensor already under that key is the destination).
    A dict also gets ``extra["out"]``, the returned tensor: how a caller further up tells that the launch happened."""
    rows, _, ldx = rows_view(x, "linear_ln_k256")
    ldr = _rows(residual, rows, "residual", rows_view)
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != tuple(x.shape):
        raise _lib.RdetrError("linear_ln_k256: out must have x's shape and dtype")
    ldo = _rows(out, rows, "out", rows_view)
    pos = out_pos = None
    ldp = ldop = 0
    if extra:
        unknown = set(extra) - {"pos", "out_plus_pos", "out"}
        if unknown:
            raise _lib.RdetrError(f"linear_ln_k256: unknown extra keys {sorted(unknown)}")
        pos = extra.get("pos")
        if pos is not None:
            if not pos.is_cuda or tuple(pos.shape) != tuple(x.shape):
                raise _lib.RdetrError("linear_ln_k256: extra['pos'] must be a device tensor of x's shape")
            ldp = _rows(pos, rows, "extra['pos']", rows_view)
            out_pos = extra.get("out_plus_pos")
            if out_pos is None:
                out_pos = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            ldop = _rows(out_pos, rows, "extra['out_plus_pos']", rows_view)
    st = _lib.load().rdetr_linear_ln_rows_bf16(
        x.data_ptr(), ldx, packed.data_ptr(), _vector(bias, "bias", keep), residual.data_ptr(), ldr, _vector(gamma, "gamma", keep),
        _vector(beta, "beta", keep), float(eps), None if pos is None else pos.data_ptr(), ldp, rows, out.data_ptr(), ldo,
        None if out_pos is None else out_pos.data_ptr(), ldop, torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(st, "rdetr_linear_ln_rows_bf16")
    if extra is not None:
        extra["out"] = out
        if pos is not None:
            extra["out_plus_pos"] = out_pos
    return out
