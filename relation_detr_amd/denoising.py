"""Contrastive denoising query generator of Relation-DETR (csrc/denoising.hip): ``GenerateCDNQueries``.

``GenerateCDNQueries`` has the reference's constructor, parameter (``label_encoder``) and results (``models/bricks/denoising.py:
180-331``): from the per-image ground truth it makes the noised label queries ``[B, Ndn, d]``, the noised logit-space box queries
``[B, Ndn, 4]`` and the visibility mask ``[Ndn + num_queries] ** 2`` that ``RelationTransformer.forward`` takes, and the
``(denoising_groups, 2 * max_gt)`` that ``RelationCriterion`` takes as ``dn_meta``.

The reference consumes four random draws in a fixed order -- ``label_u [Q]`` (``rand_like``), ``label_r [Q]`` int64
(``randint_like(0, C)``), ``box_sign [Q, 4]`` fp32 in {0, 1} (``randint_like(0, 2)``), ``box_u [Q, 4]`` (``rand_like``), Q =
2 * groups * G flat rows -- and everything else is a function of them and of the targets.  ``forward(..., noise=...)`` takes those
four, so both routes can be pinned to the reference exactly.  Two routes, chosen by the constructor's ``fused`` (CPU tensors
always take the second):

* fused -- two ``torch.cat``, one small pinned non-blocking copy of the offsets, one launch for the queries of every slot (padding
  included, so no memset and no scatter) and one for the mask; no wait for the device.  With ``noise=None`` one 63-bit key is drawn
  on the host from ``generator`` (a CPU ``torch.Generator``, default torch's global one, so ``torch.manual_seed`` reproduces a
  step) and the draws are made in registers with Philox4x32-10 (``cdn_noise`` writes the same draws out).  The backward is the
  gradient of ``label_encoder.weight``: a deterministic reduction without atomics.
* torch -- a vectorised restatement of the reference's operation sequence (repeat, noise, embedding, host-built index tensors, two
  scatter assignments, the mask) consuming the same ``noise``; with ``noise=None`` it draws the four tensors with torch in the
  reference's order.  It is what the fused route is timed against and, in float64, what it is checked against.

Measured on an MI355X (tools/time_denoising.py, profiles/r17/denoising_ab.txt: C = 91, d = 256, 900 queries, B = 2 / 4 with 7 / 20
boxes per image, forward + backward from an idle device, median of 20): fused 0.23-0.40 ms, torch 0.63-0.84 ms (2.1-2.7x); 8-9
launches against 68 (the cats, the offsets copy, the two forward kernels, the backward kernel and autograd's bookkeeping), no wait
for the device against two blocking host-to-device copies of the index tensors, 0.05-0.09 ms of device time against 0.20-0.23.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor, nn
from torch.nn import functional as F

from . import _lib
from .ops import _require_device, _stream_ptr
from .transformer import inverse_sigmoid

_DTYPES = (torch.float32, torch.bfloat16)
Noise = Tuple[Optional[Tensor], Optional[Tensor], Optional[Tensor], Optional[Tensor]]


def denoising_groups(denoising_nums: int, max_gt: int) -> int:
    """``denoising.py:253-254``: the number of (positive, negative) group pairs; 1 when no image has a box."""
    return max(denoising_nums * max_gt // max(max_gt ** 2, 1), 1)


# ---------------------------------------------------------------------------------------------------------------- the keyed draws
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32 with 10 rounds in numpy: ``counter [..., 4]`` and ``key [..., 2]`` of 32-bit words -> ``[..., 4]`` uint32.  The
    restatement of csrc/cdn_noise.h that the tests hold the kernels to."""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] & _MASK32 for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & _MASK32 for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c[0], np.uint64(_PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK32]
        k = [(k[0] + np.uint64(_PHILOX_W0)) & _MASK32, (k[1] + np.uint64(_PHILOX_W1)) & _MASK32]
    return np.stack(c, axis=-1).astype(np.uint32)


def _noise_numpy(key: int, Q: int, num_classes: int):
    r = np.arange(Q, dtype=np.uint64)
    zero = np.zeros_like(r)
    words = np.array([key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    a = philox4x32_10(np.stack([r, zero, zero, zero], -1), words).astype(np.uint64)
    b = philox4x32_10(np.stack([r, zero + np.uint64(1), zero, zero], -1), words)
    scale = np.float32(2.0 ** -24)
    label_u = (a[:, 0] >> np.uint64(8)).astype(np.float32) * scale
    label_r = ((a[:, 1] * np.uint64(num_classes)) >> np.uint64(32)).astype(np.int64)
    box_sign = ((a[:, 2:3] >> np.arange(4, dtype=np.uint64)[None]) & np.uint64(1)).astype(np.float32)
    box_u = (b >> np.uint32(8)).astype(np.float32) * scale
    return label_u, label_r, box_sign, box_u


def cdn_noise(key: int, Q: int, num_classes: int, device) -> Noise:
    """The four draws of ``key`` for Q flat rows, in the reference's layout and dtypes: ``(label_u [Q] fp32, label_r [Q] int64,
    box_sign [Q, 4] fp32, box_u [Q, 4] fp32)``.  One launch on a ROCm device, the numpy restatement on the CPU."""
    key, Q, device = int(key), int(Q), torch.device(device)
    if not 0 <= key < 2 ** 64 or Q < 0 or num_classes <= 0:
        raise _lib.RdetrError("cdn_noise: needs a key in [0, 2^64), Q >= 0 and num_classes > 0")
    if device.type != "cuda":
        return tuple(torch.from_numpy(x) for x in _noise_numpy(key, Q, int(num_classes)))
    label_u = torch.empty(Q, dtype=torch.float32, device=device)
    label_r = torch.empty(Q, dtype=torch.int64, device=device)
    box = torch.empty(2, Q, 4, dtype=torch.float32, device=device)
    st = _lib.load().rdetr_cdn_noise(key, Q, int(num_classes), label_u.data_ptr(), label_r.data_ptr(), box[0].data_ptr(), box[1].data_ptr(),
                                     _stream_ptr(label_u))
    _lib.check(st, "rdetr_cdn_noise")
    return label_u, label_r, box[0], box[1]


# ------------------------------------------------------------------------------------------------------------------------ mask
def denoising_mask(groups: int, group_size: int, num_queries: int, device, fused: bool = True) -> Tensor:
    """The bool visibility mask ``[T, T]``, T = groups * group_size + num_queries (``denoising.py:66-78``): True where query r may
    NOT see query c -- the matching queries see no denoising query, a denoising group sees only itself and the matching queries."""
    groups, group_size, num_queries, device = int(groups), int(group_size), int(num_queries), torch.device(device)
    n_dn = groups * group_size
    T = n_dn + num_queries
    if not (fused and device.type == "cuda"):
        index = torch.arange(T, device=device)
        block = index // max(group_size, 1)
        return (index[None, :] < n_dn) & ((index[:, None] >= n_dn) | (block[:, None] != block[None, :]))
    mask = torch.empty(T, T, dtype=torch.bool, device=device)
    st = _lib.load().rdetr_cdn_mask(groups, group_size, num_queries, mask.data_ptr(), _stream_ptr(mask))
    _lib.check(st, "rdetr_cdn_mask")
    return mask


# --------------------------------------------------------------------------------------------------------------------- queries
def _layout(counts: Sequence[int], groups: int):
    counts = [int(c) for c in counts]
    if not counts or min(counts) < 0 or groups < 1:
        raise _lib.RdetrError("cdn_queries: needs one non-negative count per image and groups >= 1")
    return counts, sum(counts), max(counts)


def _suffix(dtype: torch.dtype) -> str:
    return "f32" if dtype == torch.float32 else "bf16"


def _cdn_queries_torch(embed: Tensor, gt_labels: Tensor, gt_boxes: Tensor, counts: List[int], groups: int, label_noise_prob: float,
                       box_noise_scale: float, noise: Noise) -> Tuple[Tensor, Tensor, Tensor]:
    """The reference's sequence on the flat rows, in the dtype of ``gt_boxes``; differentiable with respect to ``embed``."""
    B, G, max_gt = len(counts), sum(counts), max(counts)
    n_dn, copies, dev, dt = 2 * groups * max_gt, 2 * groups, gt_boxes.device, gt_boxes.dtype
    label_u, label_r, box_sign, box_u = noise
    labels = gt_labels.repeat(copies, 1).flatten()
    boxes = gt_boxes.repeat(copies, 1)
    if label_noise_prob > 0:
        labels = torch.where(label_u < label_noise_prob * 0.5, label_r.to(labels.dtype), labels)
    if box_noise_scale > 0:
        negative = (torch.arange(copies * G, device=dev) // max(G, 1)) % 2 == 1
        diff = torch.cat((boxes[:, 2:] / 2, boxes[:, 2:] / 2), dim=-1)
        sign = box_sign.to(dt) * 2.0 - 1.0
        part = (box_u.to(dt) + negative.to(dt)[:, None]) * sign
        cx, cy, w, h = boxes.unbind(-1)
        xyxy = torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)
        xyxy = (xyxy + torch.mul(part, diff) * box_noise_scale).clamp(min=0.0, max=1.0)
        x1, y1, x2, y2 = xyxy.unbind(-1)
        boxes = torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), dim=-1)
    boxes = inverse_sigmoid(boxes)
    embedding = F.embedding(labels, embed)

    label_query = torch.zeros(B, n_dn, embed.shape[1], dtype=embed.dtype, device=dev)
    box_query = torch.zeros(B, n_dn, 4, dtype=dt, device=dev)
    noised_label = torch.full((B, n_dn), -1, dtype=torch.int32, device=dev)
    if G:                                                                       # the reference builds these two on the host as well
        image = torch.repeat_interleave(torch.arange(B), torch.tensor(counts, dtype=torch.long)).repeat(copies)
        slot = torch.cat([torch.arange(c) for c in counts])
        slot = torch.cat([slot + max_gt * i for i in range(copies)]).long()
        image, slot = image.to(dev), slot.to(dev)
        label_query[(image, slot)] = embedding
        box_query[(image, slot)] = boxes
        noised_label[(image, slot)] = labels.to(torch.int32)
    return label_query, box_query, noised_label


def _check_noise(noise: Noise, Q: int, need_label: bool, need_box: bool) -> List[Optional[Tensor]]:
    if len(noise) != 4:
        raise _lib.RdetrError("cdn_queries: noise has to be (label_u, label_r, box_sign, box_u)")
    label_u, label_r, box_sign, box_u = noise
    out: List[Optional[Tensor]] = [None] * 4
    if need_label:
        if label_u is None or label_r is None or label_u.dtype != torch.float32 or label_r.dtype != torch.int64 \
                or label_u.numel() != Q or label_r.numel() != Q:
            raise _lib.RdetrError(f"cdn_queries: needs label_u fp32 [{Q}] and label_r int64 [{Q}]")
        out[0], out[1] = label_u.contiguous(), label_r.contiguous()
    if need_box:
        if box_sign is None or box_u is None or box_sign.dtype != torch.float32 or box_u.dtype != torch.float32 \
                or tuple(box_sign.shape) != (Q, 4) or tuple(box_u.shape) != (Q, 4):
            raise _lib.RdetrError(f"cdn_queries: needs box_sign and box_u fp32 [{Q}, 4]")
        out[2], out[3] = box_sign.contiguous(), box_u.contiguous()
    return out


def cdn_queries_forward(embed: Tensor, gt_labels: Tensor, gt_boxes: Tensor, counts: Sequence[int], groups: int, label_noise_prob: float,
                        box_noise_scale: float, noise: Optional[Noise] = None, key: Optional[int] = None):
    """One launch of ``rdetr_cdn_queries_*`` -> (label_query [B, Ndn, d] in the dtype of ``embed``, box_query [B, Ndn, 4] fp32,
    noised_label [B, Ndn] int32 with -1 for padding).  Exactly one of ``noise`` and ``key`` is given."""
    _require_device(embed, gt_labels, gt_boxes)
    counts, G, max_gt = _layout(counts, groups)
    if (noise is None) == (key is None):
        raise _lib.RdetrError("cdn_queries: give either the four draws or a key")
    if embed.dim() != 2 or embed.dtype not in _DTYPES:
        raise _lib.RdetrError("cdn_queries: needs an fp32 or bf16 embedding [C, d]")
    if gt_labels.dtype != torch.int64 or gt_boxes.dtype != torch.float32 or tuple(gt_labels.shape) != (G,) or tuple(gt_boxes.shape) != (G, 4):
        raise _lib.RdetrError(f"cdn_queries: needs gt_labels int64 [{G}] and gt_boxes fp32 [{G}, 4]")
    C, d = embed.shape
    B, n_dn, dev = len(counts), 2 * groups * max_gt, embed.device
    embed, gt_labels, gt_boxes = embed.detach().contiguous(), gt_labels.contiguous(), gt_boxes.contiguous()
    draws: List[Optional[Tensor]] = [None] * 4
    if noise is not None:
        _require_device(*noise)
        draws = _check_noise(noise, 2 * groups * G, label_noise_prob > 0, box_noise_scale > 0)
    elif not 0 <= int(key) < 2 ** 64:
        raise _lib.RdetrError("cdn_queries: the key has to be in [0, 2^64)")
    offsets = torch.tensor(np.concatenate(([0], np.cumsum(counts))), dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    label_query = torch.empty(B, n_dn, d, dtype=embed.dtype, device=dev)
    box_query = torch.empty(B, n_dn, 4, dtype=torch.float32, device=dev)
    noised_label = torch.empty(B, n_dn, dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    fn = getattr(_lib.load(), "rdetr_cdn_queries_" + _suffix(embed.dtype))
    st = fn(gt_labels.data_ptr(), gt_boxes.data_ptr(), offsets.data_ptr(), B, G, max_gt, int(groups), C, d, float(label_noise_prob),
            float(box_noise_scale), embed.data_ptr(), ptr(draws[0]), ptr(draws[1]), ptr(draws[2]), ptr(draws[3]), int(noise is None),
            int(key or 0), label_query.data_ptr(), box_query.data_ptr(), noised_label.data_ptr(), _stream_ptr(embed))
    _lib.check(st, "rdetr_cdn_queries")
    return label_query, box_query, noised_label


def cdn_embed_backward(grad_label_query: Tensor, noised_label: Tensor, num_classes: int) -> Tensor:
    """``rdetr_cdn_embed_backward_*``: grad_embed [C, d] from grad_label_query [..., d] and noised_label [...] int32."""
    _require_device(grad_label_query, noised_label)
    if grad_label_query.dtype not in _DTYPES or noised_label.dtype != torch.int32 or grad_label_query.shape[:-1] != noised_label.shape:
        raise _lib.RdetrError("cdn_embed_backward: needs an fp32 or bf16 gradient [..., d] and int32 labels [...]")
    d = grad_label_query.shape[-1]
    grad = grad_label_query.contiguous()
    labels = noised_label.contiguous()
    grad_embed = torch.empty(int(num_classes), d, dtype=grad.dtype, device=grad.device)
    fn = getattr(_lib.load(), "rdetr_cdn_embed_backward_" + _suffix(grad.dtype))
    st = fn(grad.data_ptr() if grad.numel() else None, labels.data_ptr() if labels.numel() else None, labels.numel(), int(num_classes), d,
            grad_embed.data_ptr(), _stream_ptr(grad))
    _lib.check(st, "rdetr_cdn_embed_backward")
    return grad_embed


class CdnQueryFunction(torch.autograd.Function):
    """``apply(embed, gt_labels, gt_boxes, counts, groups, label_noise_prob, box_noise_scale, noise, key) -> (label_query, box_query,
    noised_label)``, differentiable with respect to ``embed`` only (the boxes carry no gradient in the reference either: the
    ground truth does not require one)."""

    @staticmethod
    def forward(ctx, embed, gt_labels, gt_boxes, counts, groups, label_noise_prob, box_noise_scale, noise, key):
        label_query, box_query, noised_label = cdn_queries_forward(embed, gt_labels, gt_boxes, counts, groups, label_noise_prob,
                                                                   box_noise_scale, noise, key)
        ctx.save_for_backward(noised_label)
        ctx.num_classes = embed.shape[0]
        ctx.mark_non_differentiable(box_query, noised_label)
        return label_query, box_query, noised_label

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_label_query, _grad_box, _grad_label):
        noised_label, = ctx.saved_tensors
        grad_embed = cdn_embed_backward(grad_label_query, noised_label, ctx.num_classes) if ctx.needs_input_grad[0] else None
        return grad_embed, None, None, None, None, None, None, None, None


def cdn_queries(embed: Tensor, gt_labels: Tensor, gt_boxes: Tensor, counts: Sequence[int], groups: int, label_noise_prob: float = 0.5,
                box_noise_scale: float = 1.0, noise: Optional[Noise] = None, key: Optional[int] = None,
                fused: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
    """The denoising queries of every slot: ``(label_query [B, Ndn, d], box_query [B, Ndn, 4] in logit space, noised_label [B, Ndn]
    int32, -1 for padding)``, Ndn = 2 * groups * max(counts).

    ``embed [C, d]`` is the label embedding (fp32 or bf16), ``gt_labels [G]`` int64 and ``gt_boxes [G, 4]`` cxcywh the ground
    truth of the images back to back, ``counts`` the boxes per image (host integers).  ``noise`` is the reference's four draws
    (module docstring; an entry may be None where its noise is switched off); on the fused route ``key`` may stand for them: the
    draws of ``cdn_noise(key, ...)``.  The torch route (``fused=False`` or CPU tensors) computes in the dtype of ``gt_boxes`` and
    needs ``noise``.  Differentiable with respect to ``embed`` on both routes."""
    if fused and embed.is_cuda:
        return CdnQueryFunction.apply(embed, gt_labels, gt_boxes, counts, int(groups), float(label_noise_prob), float(box_noise_scale),
                                      noise, key)
    counts, G, _ = _layout(counts, groups)
    if noise is None:
        if key is None:
            raise _lib.RdetrError("cdn_queries: the torch route needs the four draws or a key")
        noise = cdn_noise(key, 2 * int(groups) * G, embed.shape[0], embed.device)
    return _cdn_queries_torch(embed, gt_labels, gt_boxes, counts, int(groups), float(label_noise_prob), float(box_noise_scale), noise)


# ---------------------------------------------------------------------------------------------------------------------- module
class GenerateCDNQueries(nn.Module):
    """``models/bricks/denoising.py:180-331`` with the same constructor arguments and the same parameter, ``label_encoder.weight``
    (a ``RelationDETR`` checkpoint's ``denoising_generator.label_encoder.weight`` loads), plus ``fused``.

    ``forward(gt_labels_list, gt_boxes_list, noise=None, generator=None)`` -> ``(noised_label_query [B, Ndn, d], noised_box_query
    [B, Ndn, 4], attn_mask [Ndn + num_queries] ** 2 bool, denoising_groups, 2 * max_gt)`` and sets ``self.denoising_groups``.
    ``noise``: the four draws (module docstring); None draws them -- on the fused route as one host key from ``generator``, on
    the torch route as four tensors in the reference's order (from ``generator`` where given, which then has to live on the
    targets' device)."""

    def __init__(self, num_queries: int = 300, num_classes: int = 80, label_embed_dim: int = 256, denoising_nums: int = 100,
                 label_noise_prob: float = 0.5, box_noise_scale: float = 1.0, fused: bool = True):
        super().__init__()
        self.num_queries = int(num_queries)
        self.num_classes = int(num_classes)
        self.label_embed_dim = int(label_embed_dim)
        self.denoising_nums = int(denoising_nums)
        self.label_noise_prob = float(label_noise_prob)
        self.box_noise_scale = float(box_noise_scale)
        self.denoising_groups = 1
        self.fused = bool(fused)
        self.label_encoder = nn.Embedding(num_classes, label_embed_dim)

    def draw_noise(self, Q: int, device, generator: Optional[torch.Generator] = None) -> Noise:
        """The four draws with torch, in the reference's order; a switched-off noise consumes none (``denoising.py:47-54,218-224``)."""
        label_u = label_r = box_sign = box_u = None
        kw = {"device": device, "generator": generator}
        if self.label_noise_prob > 0:
            label_u = torch.rand(Q, dtype=torch.float32, **kw)
            label_r = torch.randint(0, self.num_classes, (Q,), dtype=torch.int64, **kw)
        if self.box_noise_scale > 0:
            box_sign = torch.randint(0, 2, (Q, 4), dtype=torch.float32, **kw)
            box_u = torch.rand(Q, 4, dtype=torch.float32, **kw)
        return label_u, label_r, box_sign, box_u

    def forward(self, gt_labels_list: Sequence[Tensor], gt_boxes_list: Sequence[Tensor], noise: Optional[Noise] = None,
                generator: Optional[torch.Generator] = None):
        if len(gt_labels_list) != len(gt_boxes_list) or not len(gt_labels_list):
            raise ValueError("GenerateCDNQueries: one label tensor and one box tensor per image")
        counts = [int(x.numel()) for x in gt_labels_list]
        max_gt = max(counts)
        self.denoising_groups = groups = denoising_groups(self.denoising_nums, max_gt)
        gt_labels = torch.cat(list(gt_labels_list))
        gt_boxes = torch.cat(list(gt_boxes_list)).reshape(-1, 4)
        weight = self.label_encoder.weight
        fused = self.fused and weight.is_cuda
        key = None
        if noise is None:
            if fused:                                                           # one host draw: no launch, reproducible by manual_seed
                key = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, generator=generator).item())
            else:
                noise = self.draw_noise(2 * groups * sum(counts), gt_labels.device, generator)
        if fused:
            gt_labels, gt_boxes = gt_labels.to(torch.int64), gt_boxes.to(torch.float32)
        label_query, box_query, _ = cdn_queries(weight, gt_labels, gt_boxes, counts, groups, self.label_noise_prob,
                                                self.box_noise_scale, noise=noise, key=key, fused=fused)
        attn_mask = denoising_mask(groups, 2 * max_gt, self.num_queries, gt_labels.device, fused=fused)
        return label_query, box_query, attn_mask, groups, 2 * max_gt
