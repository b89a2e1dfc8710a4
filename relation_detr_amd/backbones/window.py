"""The geometry of Swin's shifted-window attention (``models/backbones/swin.py:133-221`` of the reference) as plain arithmetic: what
csrc/attn_win.hip computes per lane, written once on the host for the modules and the tests.  Names no kernel; launches nothing.

A map of ``H x W`` tokens is padded to ``pH x pW`` (multiples of the window), rolled by ``(-sh, -sw)`` and cut into windows of
``wh x ww``.  Rolled-frame position ``(y, x)`` lies in window ``(y // wh, x // ww)`` at ``(y % wh, x % ww)`` and holds the token of
source position ``((y + sh) % pH, (x + sw) % pW)``; a source position outside ``H x W`` is a padding token.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

MASK_VALUE = -100.0
MAX_WINDOW_TOKENS = 144           # what the kernel holds of one window: three chunks of 64 keys, the last with 16
HEAD_DIM = 32


def padded_size(H: int, W: int, wh: int, ww: int) -> Tuple[int, int]:
    return -(-H // wh) * wh, -(-W // ww) * ww


def effective_shift(H: int, W: int, wh: int, ww: int, sh: int, sw: int) -> Tuple[int, int]:
    """The reference's rule: no shift in a dimension whose window is at least the padded size."""
    pH, pW = padded_size(H, W, wh, ww)
    return (0 if wh >= pH else sh), (0 if ww >= pW else sw)


def region_ids(pH: int, pW: int, wh: int, ww: int, sh: int, sw: int) -> Tensor:
    """``[pH, pW]`` int64 region id ``3 * hr + wr`` of every rolled-frame position: ``hr`` is 0 below ``pH - wh``, 1 below
    ``pH - sh``, else 2.  A dimension with shift 0 is split at the last window's boundary only, which no window straddles, so the
    pairs of different regions INSIDE a window are those of the reference's slice construction."""
    y, x = torch.arange(pH), torch.arange(pW)
    hr = (y >= pH - wh).long() + (y >= pH - sh).long()
    wr = (x >= pW - ww).long() + (x >= pW - sw).long()
    return 3 * hr[:, None] + wr[None, :]


def window_partition(t: Tensor, wh: int, ww: int) -> Tensor:
    """``[..., pH, pW] -> [..., windows, wh * ww]`` in the reference's window and token order."""
    *lead, pH, pW = t.shape
    t = t.reshape(*lead, pH // wh, wh, pW // ww, ww)
    n = len(lead)
    return t.permute(*range(n), n, n + 2, n + 1, n + 3).reshape(*lead, (pH // wh) * (pW // ww), wh * ww)


def shift_mask(H: int, W: int, wh: int, ww: int, sh: int, sw: int) -> Optional[Tensor]:
    """The reference's ``attn_mask`` ``[windows, N, N]`` (0 / -100) for an EFFECTIVE shift, or None without one."""
    if sh + sw == 0:
        return None
    pH, pW = padded_size(H, W, wh, ww)
    region = window_partition(region_ids(pH, pW, wh, ww, sh, sw), wh, ww)
    differ = region[:, None, :] != region[:, :, None]
    return torch.where(differ, torch.tensor(MASK_VALUE), torch.tensor(0.0))


def bias_index(wh: int, ww: int) -> Tensor:
    """``[N, N]`` int64: row of the relative-position-bias table for query ``i = ri * ww + ci`` and key ``j``,
    ``(ri - rj + wh - 1) * (2 * ww - 1) + (ci - cj + ww - 1)`` -- the reference's ``relative_position_index`` buffer, unflattened."""
    r = torch.arange(wh * ww)
    ri, ci = r // ww, r % ww
    return (ri[:, None] - ri[None, :] + wh - 1) * (2 * ww - 1) + (ci[:, None] - ci[None, :] + ww - 1)


def source_index(H: int, W: int, wh: int, ww: int, sh: int, sw: int) -> Tensor:
    """``[windows, N]`` int64: the source row ``sy * W + sx`` of every window token, -1 for a padding token."""
    pH, pW = padded_size(H, W, wh, ww)
    sy, sx = (torch.arange(pH) + sh) % pH, (torch.arange(pW) + sw) % pW
    src = torch.where((sy[:, None] < H) & (sx[None, :] < W), sy[:, None] * W + sx[None, :], torch.tensor(-1))
    return window_partition(src, wh, ww)


def window_attention_reference(q: Tensor, k: Tensor, v: Tensor, num_heads: int, table: Tensor, window: Sequence[int],
                               pad: Optional[Tuple[Optional[Tensor], Optional[Tensor]]] = None, scale: Optional[float] = None,
                               round_p: bool = False) -> Tensor:
    """The windowed operator restated in float64 from the geometry above: ``q, k, v [B, H*W, C]`` of the unpadded map, ``table
    [(2wh-1)(2ww-1), heads]``, ``window = (H, W, wh, ww, sh, sw)`` with the effective shift, ``pad = (k_pad, v_pad)`` rows ``[C]`` of a
    padding token (zeros when None) -> ``[B, H*W, C]`` float64 at the tokens' source rows.  ``round_p`` rounds the soft-max
    numerators to bf16 before the P V product, as the kernel does."""
    H, W, wh, ww, sh, sw = (int(x) for x in window)
    B, L, C = q.shape
    D, N = C // num_heads, wh * ww
    assert L == H * W and C % num_heads == 0
    scale = D ** -0.5 if scale is None else float(scale)
    f64 = lambda t: t.detach().to("cpu", torch.float64)                                                    # noqa: E731
    q, k, v, table = f64(q), f64(k), f64(v), f64(table)
    k_pad, v_pad = (None, None) if pad is None else pad
    zero = torch.zeros(C, dtype=torch.float64)
    k_pad = zero if k_pad is None else f64(k_pad).reshape(C)
    v_pad = zero if v_pad is None else f64(v_pad).reshape(C)
    src = source_index(H, W, wh, ww, sh, sw)                               # [nW, N]
    nW = src.shape[0]
    inside = src >= 0
    take = src.clamp(min=0).reshape(-1)

    def windows(t, pad_row):                                               # [B, L, C] -> [B, nW, heads, N, D], padding tokens filled in
        w = t[:, take].reshape(B, nW, N, C)
        w = torch.where(inside[None, :, :, None], w, pad_row.expand(B, nW, N, C))
        return w.reshape(B, nW, N, num_heads, D).permute(0, 1, 3, 2, 4)
    qw, kw, vw = windows(q, zero), windows(k, k_pad), windows(v, v_pad)
    logits = (qw @ kw.transpose(-1, -2)) * scale + table[bias_index(wh, ww)].permute(2, 0, 1)
    mask = shift_mask(H, W, wh, ww, sh, sw)
    if mask is not None:
        logits = logits + mask.to(torch.float64)[None, :, None]
    logits = logits - logits.amax(-1, keepdim=True)
    p = logits.exp()
    denom = p.sum(-1, keepdim=True)
    if round_p:
        p = p.to(torch.bfloat16).to(torch.float64)
    o = ((p @ vw) / denom).permute(0, 1, 3, 2, 4).reshape(B, nW * N, C)
    out = torch.zeros(B, L, C, dtype=torch.float64)
    out[:, take[inside.reshape(-1)]] = o[:, inside.reshape(-1)]
    return out


def fused_window_supported(dim: int, num_heads: int, wh: int, ww: int) -> bool:
    """What the kernel is built for: head dim 32 and at most 144 tokens per window."""
    return num_heads > 0 and dim == num_heads * HEAD_DIM and 0 < wh * ww <= MAX_WINDOW_TOKENS
