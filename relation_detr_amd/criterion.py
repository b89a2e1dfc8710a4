"""Training criterion of Relation-DETR: Hungarian match costs and the hybrid set losses (csrc/criterion.hip).

``RelationCriterion`` turns the eight tensors of ``RelationTransformer.forward`` in training mode into the weighted loss dict the
reference trains on (``models/detectors/relation_detr.py:124-141``): ``HybridSetCriterion`` on the one-to-one sets, the same on the
hybrid branch with the targets repeated ``hybrid_assign`` times, and ``compute_dn_loss`` on the denoising queries.

Two routes, chosen by the constructor's ``fused`` (CPU tensors always take the second):

* fused -- every decoder layer's set is one row of a stack.  ``match_cost`` fills the cost matrices of a whole stack in one launch
  (up to four per step: decoder, encoder proposals, hybrid decoder, hybrid proposals) into one buffer; ``assign_match`` turns it
  into the match tables, the fixed denoising matches among them; ``set_loss`` computes every loss and gradient of a stack in one
  pass.  The constructor's ``matcher`` says where the assignments are solved: ``"scipy"`` (the default) copies the buffer to the
  host, the step's only synchronisation, solves there and copies the tables back; ``"device"`` solves every stack with one launch
  of ``rdetr_assign_match`` (csrc/assign.hip) straight into the device table: no copy, and nothing waits for the device.
* torch -- a restatement of the reference, set by set and image by image: ``HungarianMatcher.calculate_cost``
  (``models/matcher/hungarian_matcher.py:41-70``), ``HybridSetCriterion.loss_labels``, ``SetCriterion.loss_boxes``
  (``models/bricks/set_criterion.py:84-106,178-216``) and ``vari_sigmoid_focal_loss`` (``models/bricks/losses.py:15-21``), with
  the box IoU / GIoU written from their formulas.  It is what the fused route is timed against and, in float64, what it is checked
  against.

``match_cost``, ``hungarian_match`` / ``assign_match`` and ``set_loss`` are the pieces, usable alone.  Not built: the plain focal
``SetCriterion``, ``ia_bce_loss``, ``two_stage_binary_cls`` and ``mixed_match``.  The denoising
query generator whose ``dn_meta`` this takes is ``denoising.GenerateCDNQueries``; ``detector.RelationDETRHead`` chains the two
around the transformer.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed
from torch import Tensor, nn
from torch.nn import functional as F

from . import _lib
from .ops import _require_device, _stream_ptr

_DTYPES = (torch.float32, torch.bfloat16)
MAX_GT = 2048                    # kCostMaxGt: one image's gt table has to fit the cost kernel's LDS
MAX_ASSIGN = 2048                # kAssignMaxSide: queries, and Gmax * repeat target copies, of one problem of the device matcher


# ------------------------------------------------------------------------------------------------------------------ torch route
def box_cxcywh_to_xyxy(boxes: Tensor) -> Tensor:
    cx, cy, w, h = boxes.unbind(-1)
    return torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)


def _inter_union(boxes1: Tensor, boxes2: Tensor) -> Tuple[Tensor, Tensor]:
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    lt = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    rb = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter, area1[:, None] + area2 - inter


def box_iou(boxes1: Tensor, boxes2: Tensor) -> Tensor:
    """Pairwise IoU [N, M] of xyxy boxes."""
    inter, union = _inter_union(boxes1, boxes2)
    return inter / union


def generalized_box_iou(boxes1: Tensor, boxes2: Tensor) -> Tensor:
    """Pairwise GIoU [N, M] of xyxy boxes: IoU - (hull - union) / hull."""
    inter, union = _inter_union(boxes1, boxes2)
    iou = inter / union
    lti = torch.min(boxes1[:, None, :2], boxes2[:, :2])
    rbi = torch.max(boxes1[:, None, 2:], boxes2[:, 2:])
    whi = (rbi - lti).clamp(min=0)
    areai = whi[:, :, 0] * whi[:, :, 1]
    return iou - (areai - union) / areai


def _image_cost(logits: Tensor, boxes: Tensor, gt_boxes: Tensor, gt_labels: Tensor, w_class: float, w_bbox: float, w_giou: float,
                alpha: float, gamma: float) -> Tensor:
    """``HungarianMatcher.calculate_cost`` of one image -> [N, G]; a label outside [0, C) has class term 0."""
    C = logits.shape[-1]
    prob = logits.sigmoid()
    neg = -(1 - alpha) * prob ** gamma * (1 - prob + 1e-6).log()
    pos = -alpha * (1 - prob) ** gamma * (prob + 1e-6).log()
    valid = (gt_labels >= 0) & (gt_labels < C)
    labels = gt_labels.clamp(0, C - 1).long()
    cost_class = (pos[:, labels] - neg[:, labels]) * valid.to(prob.dtype)
    cost_bbox = torch.cdist(boxes, gt_boxes, p=1)
    cost_giou = -generalized_box_iou(box_cxcywh_to_xyxy(boxes), box_cxcywh_to_xyxy(gt_boxes))
    return w_bbox * cost_bbox + w_class * cost_class + w_giou * cost_giou


def _varifocal(logits: Tensor, hot: Tensor, score: Tensor, num_boxes: float, alpha: float, gamma: float) -> Tensor:
    """The varifocal class loss of one set [B, N, C]: BCE against the IoU-valued one-hot target, weighted by that target on the matched
    class and by (1 - alpha) p^gamma elsewhere, p detached.  Summed per image, divided by N, then over images and by num_boxes -- the
    reference's order of operations, which the fp32 fixture pins."""
    p = logits.sigmoid().detach()
    soft = hot * score.unsqueeze(-1)
    w = (1 - alpha) * p.pow(gamma) * (1 - hot) + soft
    per_element = F.binary_cross_entropy_with_logits(logits, soft, weight=w, reduction="none")
    return (per_element.sum(1) / max(logits.shape[1], 1)).sum() / num_boxes


def _set_losses(logits: Tensor, boxes: Tensor, indices, gt_boxes: Sequence[Tensor], gt_labels: Sequence[Tensor], num_boxes: float,
                alpha: float, gamma: float) -> Tuple[Tensor, Tensor, Tensor]:
    """The three losses of ONE prediction set [B, N, *] under per-image (query, gt) index pairs, as the reference forms them."""
    B, N, C = logits.shape
    dev = logits.device
    image = torch.cat([torch.full_like(q, i) for i, (q, _) in enumerate(indices)]).to(dev)
    query = torch.cat([q for q, _ in indices]).to(dev)
    pred = boxes[image, query]
    gt = torch.cat([g[j.to(dev)] for g, (_, j) in zip(gt_boxes, indices)], dim=0).to(pred.dtype)
    pred_xyxy, gt_xyxy = box_cxcywh_to_xyxy(pred), box_cxcywh_to_xyxy(gt)
    iou = torch.diag(box_iou(pred_xyxy, gt_xyxy)).detach()

    classes = torch.full((B, N), C, dtype=torch.int64, device=dev)            # C = "no object": the column dropped below
    classes[image, query] = torch.cat([lab[j.to(dev)] for lab, (_, j) in zip(gt_labels, indices)]).long()
    hot = F.one_hot(classes, C + 1)[..., :-1]
    score = torch.zeros((B, N), dtype=iou.dtype, device=dev)
    score[image, query] = iou
    loss_class = _varifocal(logits, hot, score, num_boxes, alpha, gamma) * N

    loss_bbox = F.l1_loss(pred, gt, reduction="none").sum() / num_boxes
    loss_giou = (1 - torch.diag(generalized_box_iou(pred_xyxy, gt_xyxy))).sum() / num_boxes
    return loss_class, loss_bbox, loss_giou


def _set_loss_torch(logits: Tensor, boxes: Tensor, match: Tensor, gt_boxes: Tensor, gt_labels: Tensor, n_split: int, inv_norm_a: float,
                    inv_norm_b: float, alpha: float, gamma: float) -> Tensor:
    """``set_loss`` in torch ops over the whole stack (differentiable through autograd), in the dtype of ``boxes``."""
    R, N, C = logits.shape
    B, Gmax = gt_labels.shape
    dt = boxes.dtype
    logits = logits.to(dt)
    matched = (match >= 0) & (match < Gmax)
    m = match.clamp(0, Gmax - 1).long()
    image = torch.arange(R, device=logits.device) % B
    tgt = gt_boxes.to(dt)[image[:, None], m]                                  # [R, N, 4]
    lab = gt_labels[image[:, None], m].long()
    a, b = box_cxcywh_to_xyxy(boxes), box_cxcywh_to_xyxy(tgt)
    area_a, area_b = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]), (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    wh = (torch.min(a[..., 2:], b[..., 2:]) - torch.max(a[..., :2], b[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a + area_b - inter
    iou = inter / union
    whi = (torch.max(a[..., 2:], b[..., 2:]) - torch.min(a[..., :2], b[..., :2])).clamp(min=0)
    areai = whi[..., 0] * whi[..., 1]
    giou = iou - (areai - union) / areai
    zero = torch.zeros((), dtype=dt, device=logits.device)
    l1 = torch.where(matched, (boxes - tgt).abs().sum(-1), zero)
    lg = torch.where(matched, 1 - giou, zero)

    score = torch.where(matched, iou.detach(), zero)
    hot = (torch.arange(C, device=logits.device) == lab[..., None]) & matched[..., None] & ((lab >= 0) & (lab < C))[..., None]
    onehot = hot.to(dt)
    target = onehot * score[..., None]
    prob = logits.sigmoid().detach()
    weight = (1 - alpha) * prob.pow(gamma) * (1 - onehot) + target
    cls = F.binary_cross_entropy_with_logits(logits, target, weight=weight, reduction="none").sum(-1)
    per_query = torch.stack((cls, l1, lg), dim=-1)                            # [R, N, 3]
    return torch.stack((per_query[:, :n_split].sum(1) * inv_norm_a, per_query[:, n_split:].sum(1) * inv_norm_b), dim=1)


# ------------------------------------------------------------------------------------------------------------------ fused route
def _rows(t: Tensor) -> Tuple[Tensor, int]:
    """``t`` [R, N, K] as rows that are contiguous inside and evenly spaced -> (tensor, row stride in elements); copied otherwise."""
    R, N, K = t.shape
    if N * K and not (t.stride(2) == 1 and t.stride(1) == K and (R <= 1 or t.stride(0) >= N * K)):
        t = t.contiguous()
    return t, (t.stride(0) if R > 1 else N * K)


def _suffix(dtype: torch.dtype) -> str:
    return "f32" if dtype == torch.float32 else "bf16"


def _check_stack(name: str, logits: Tensor, boxes: Tensor, gt_boxes: Tensor, gt_labels: Tensor) -> Tuple[int, int, int, int, int]:
    if logits.dim() != 3 or boxes.dim() != 3 or boxes.shape[-1] != 4 or boxes.shape[:2] != logits.shape[:2]:
        raise _lib.RdetrError(f"{name}: needs logits [R, N, C] and boxes [R, N, 4]")
    if logits.dtype not in _DTYPES or boxes.dtype != torch.float32:
        raise _lib.RdetrError(f"{name}: needs fp32 or bf16 logits and fp32 boxes")
    if gt_boxes.dim() != 3 or gt_boxes.shape[-1] != 4 or gt_labels.shape != gt_boxes.shape[:2] or gt_boxes.shape[1] < 1:
        raise _lib.RdetrError(f"{name}: needs gt_boxes [B, Gmax, 4] and gt_labels [B, Gmax] with Gmax >= 1")
    if gt_boxes.dtype != torch.float32 or gt_labels.dtype != torch.int32 or not gt_boxes.is_contiguous() or not gt_labels.is_contiguous():
        raise _lib.RdetrError(f"{name}: needs contiguous fp32 gt_boxes and int32 gt_labels")
    R, N, C = logits.shape
    B, Gmax = gt_labels.shape
    if R % B:
        raise _lib.RdetrError(f"{name}: the {R} rows are not a multiple of the {B} images")
    return R, N, C, B, Gmax


def match_cost(logits: Tensor, boxes: Tensor, gt_boxes: Tensor, gt_labels: Tensor, gt_count: Tensor, cost_class: float = 2.0,
               cost_bbox: float = 5.0, cost_giou: float = 2.0, alpha: float = 0.25, gamma: float = 2.0, fused: bool = True,
               out: Optional[Tensor] = None) -> Tensor:
    """The matcher's cost ``[R, N, Gmax]`` of a stack of prediction sets: row ``r`` against the ground truth of image ``r % B``.

    logits [R, N, C] (fp32 or bf16) and boxes [R, N, 4] (cxcywh) may be query slices of taller tensors; gt_boxes [B, Gmax, 4],
    gt_labels [B, Gmax] int32 and gt_count [B] int32 are the padded tables.  Columns at or beyond an image's count are 0.  fp32 on
    the fused route (``out``, when given, receives it); the dtype of ``boxes`` on the torch route (``fused=False`` or CPU tensors),
    which takes logits of any float type upcast to it."""
    if not (fused and logits.is_cuda):
        R, N, C = logits.shape
        B, Gmax = gt_labels.shape
        counts = gt_count.tolist()
        cost = torch.zeros(R, N, Gmax, dtype=boxes.dtype, device=boxes.device)
        for r in range(R):
            g = min(max(int(counts[r % B]), 0), Gmax)
            if g:
                cost[r, :, :g] = _image_cost(logits[r].to(boxes.dtype), boxes[r], gt_boxes[r % B, :g].to(boxes.dtype), gt_labels[r % B, :g],
                                             cost_class, cost_bbox, cost_giou, alpha, gamma)
        return cost
    _require_device(logits, boxes, gt_boxes, gt_labels, gt_count)
    R, N, C, B, Gmax = _check_stack("match_cost", logits, boxes, gt_boxes, gt_labels)
    if gt_count.dtype != torch.int32 or gt_count.numel() != B or not gt_count.is_contiguous():
        raise _lib.RdetrError("match_cost: gt_count has to be contiguous int32 [B]")
    if out is None:
        out = torch.empty(R, N, Gmax, dtype=torch.float32, device=logits.device)
    elif out.dtype != torch.float32 or out.numel() != R * N * Gmax or not out.is_contiguous() or not out.is_cuda:
        raise _lib.RdetrError("match_cost: out has to be a contiguous fp32 device tensor of R * N * Gmax elements")
    logits, ldl = _rows(logits.detach())
    boxes, ldb = _rows(boxes.detach())
    fn = getattr(_lib.load(), "rdetr_match_cost_" + _suffix(logits.dtype))
    st = fn(logits.data_ptr(), ldl, boxes.data_ptr(), ldb, gt_boxes.data_ptr(), gt_labels.data_ptr(), gt_count.data_ptr(), R, B, N, C,
            Gmax, float(alpha), float(gamma), float(cost_class), float(cost_bbox), float(cost_giou), out.data_ptr(), _stream_ptr(logits))
    _lib.check(st, "rdetr_match_cost")
    return out.view(R, N, Gmax)


def hungarian_match(cost, gt_count: Sequence[int], repeat: int = 1) -> List[Tuple[Tensor, Tensor]]:
    """Optimal assignment of every row of a host cost stack ``[R, N, Gmax]`` -> R pairs (src, tgt) of int64 CPU tensors.

    Row ``r`` uses the first ``gt_count[r % B]`` columns, tiled ``repeat`` times (the hybrid branch's repeated targets: the copies
    cost the same, so they are never computed twice); ``tgt`` is returned modulo the image's count."""
    from scipy.optimize import linear_sum_assignment

    cost = cost.detach().cpu().numpy() if torch.is_tensor(cost) else np.asarray(cost)
    counts = [int(c) for c in (gt_count.tolist() if torch.is_tensor(gt_count) else gt_count)]
    empty = torch.zeros(0, dtype=torch.int64)
    pairs = []
    for r in range(cost.shape[0]):
        g = counts[r % len(counts)]
        if g == 0:
            pairs.append((empty, empty))
            continue
        c = cost[r, :, :g]
        src, tgt = linear_sum_assignment(np.tile(c, (1, repeat)) if repeat > 1 else c)
        pairs.append((torch.as_tensor(src, dtype=torch.int64), torch.as_tensor(tgt % g, dtype=torch.int64)))
    return pairs


def _dn_groups(skip: int, dn_meta) -> Tuple[int, int]:
    if not skip:
        return 0, 0
    if dn_meta is None or int(dn_meta[0]) * int(dn_meta[1]) != skip or skip < 0:
        raise ValueError("assign_match: skip has to be dn_meta's groups * max_gt")
    return int(dn_meta[0]), int(dn_meta[1])


def assign_match(cost: Tensor, gt_count, repeat: int = 1, skip: int = 0, dn_meta=None, out: Optional[Tensor] = None,
                 fused: bool = True) -> Tuple[Tensor, Tensor]:
    """The match table ``set_loss`` reads, from a cost stack ``[R, N, Gmax]`` -> (match int32 [R, skip + N], status int32 [R]).

    Row ``r`` is solved over the first ``gt_count[r % B]`` columns tiled ``repeat`` times, as ``hungarian_match`` solves it: entry
    ``skip + q`` holds query q's gt index or -1.  The first ``skip = groups * max_gt`` entries (``dn_meta``) are the denoising
    queries' fixed matches: entry ``grp * max_gt + t`` is ``t`` where ``t`` is below the image's count, else -1.  ``out``, when
    given, is an int32 table of R rows and at least ``skip + N`` columns (a column slice of a wider one will do); only those
    columns are written.  ``status[r]`` is 1 where the row's costs are not all finite (its matcher entries are then -1), else 0.

    fp32 device tensors (cost contiguous, gt_count int32 [B]) go to ``rdetr_assign_match``, which enqueues one launch and never
    waits for the device; CPU tensors, or ``fused=False``, go through scipy on the host (``gt_count`` may then be a sequence)."""
    R, N, Gmax = cost.shape
    groups, max_gt = _dn_groups(int(skip), dn_meta)
    if repeat < 1:
        raise ValueError("assign_match: repeat has to be at least 1")
    if out is not None and (out.dtype != torch.int32 or out.dim() != 2 or out.shape[0] != R or out.shape[1] < skip + N
                            or (out.shape[1] > 1 and out.stride(1) != 1)):
        raise _lib.RdetrError("assign_match: out has to be int32 [R, >= skip + N] with unit column stride")
    if not (fused and cost.is_cuda):
        counts = [int(c) for c in (gt_count.tolist() if torch.is_tensor(gt_count) else gt_count)]
        B = len(counts)
        if B < 1 or R % B:
            raise ValueError(f"assign_match: the {R} rows are not a multiple of the {B} images")
        host = cost.detach().cpu()
        table = torch.empty(R, skip + N, dtype=torch.int32) if out is None or out.is_cuda else out
        table[:, :skip + N] = -1
        status = torch.zeros(R, dtype=torch.int32)
        try:
            pairs = hungarian_match(host, counts, repeat)
        except ValueError:                                                    # scipy refuses a matrix with NaN or -inf: row by row
            pairs = []
            for r in range(R):
                try:
                    pairs += hungarian_match(host[r:r + 1], counts[r % B:r % B + 1], repeat)
                except ValueError:
                    pairs.append((torch.zeros(0, dtype=torch.int64),) * 2)
                    status[r] = 1
        for r, (src, tgt) in enumerate(pairs):
            table[r, src + skip] = tgt.to(torch.int32)
        if skip:                                                              # the denoising queries: group g, target t -> gt t
            slot = torch.arange(max_gt, dtype=torch.int32)
            for b in range(B):
                fixed = torch.where(slot < counts[b], slot, slot.new_tensor(-1)).repeat(groups)
                table[b::B, :skip] = fixed
        if table is not out and out is not None:
            out[:, :skip + N] = table.to(out.device)
            table = out
        return table[:, :skip + N], status.to(cost.device)
    if not torch.is_tensor(gt_count):
        raise _lib.RdetrError("assign_match: gt_count has to be a device tensor on the device route")
    _require_device(cost, gt_count)
    if cost.dtype != torch.float32 or not cost.is_contiguous():
        raise _lib.RdetrError("assign_match: cost has to be a contiguous fp32 device tensor [R, N, Gmax]")
    B = gt_count.numel()
    if gt_count.dtype != torch.int32 or not gt_count.is_contiguous() or B < 1 or R % B:
        raise _lib.RdetrError("assign_match: gt_count has to be contiguous int32 [B] with R a multiple of B")
    if out is None:
        out = torch.empty(R, skip + N, dtype=torch.int32, device=cost.device)
    elif not out.is_cuda:
        raise _lib.RdetrError("assign_match: out has to be a device tensor on the device route")
    status = torch.empty(R, dtype=torch.int32, device=cost.device)
    ld = out.stride(0) if R > 1 else max(out.shape[1], 1)
    st = _lib.load().rdetr_assign_match(cost.data_ptr(), gt_count.data_ptr(), R, B, N, Gmax, int(repeat), int(skip), groups, max_gt,
                                        out.data_ptr(), ld, status.data_ptr(), _stream_ptr(cost))
    _lib.check(st, "rdetr_assign_match")
    return out[:, :skip + N], status


def set_loss_forward(logits: Tensor, boxes: Tensor, match: Tensor, gt_boxes: Tensor, gt_labels: Tensor, n_split: int, inv_norm_a: float,
                     inv_norm_b: float, alpha: float = 0.25, gamma: float = 2.0):
    """One pass of ``rdetr_set_loss_*`` -> (sums [R, 2, 3] fp32, dlogits [R, N, C] in the logits' dtype, dbox_l1, dbox_giou [R, N, 4]
    fp32); the three gradients already carry the segment's ``inv_norm``."""
    _require_device(logits, boxes, match, gt_boxes, gt_labels)
    R, N, C, B, Gmax = _check_stack("set_loss", logits, boxes, gt_boxes, gt_labels)
    if match.dtype != torch.int32 or tuple(match.shape) != (R, N) or not match.is_contiguous():
        raise _lib.RdetrError("set_loss: match has to be contiguous int32 [R, N]")
    if not 0 <= n_split <= N:
        raise _lib.RdetrError("set_loss: n_split outside [0, N]")
    lib = _lib.load()
    dev = logits.device
    logits, ldl = _rows(logits.detach())
    boxes, ldb = _rows(boxes.detach())
    sums = torch.empty(R, 2, 3, dtype=torch.float32, device=dev)
    dlogits = torch.empty(R, N, C, dtype=logits.dtype, device=dev)
    dbox = torch.empty(2, R, N, 4, dtype=torch.float32, device=dev)
    nbytes = int(lib.rdetr_set_loss_workspace_bytes(R, N))
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
    fn = getattr(lib, "rdetr_set_loss_" + _suffix(logits.dtype))
    st = fn(logits.data_ptr(), ldl, boxes.data_ptr(), ldb, match.data_ptr(), gt_boxes.data_ptr(), gt_labels.data_ptr(), R, B, N, C, Gmax,
            int(n_split), float(inv_norm_a), float(inv_norm_b), float(alpha), float(gamma), ws.data_ptr(), nbytes, sums.data_ptr(),
            dlogits.data_ptr(), dbox[0].data_ptr(), dbox[1].data_ptr(), _stream_ptr(logits))
    _lib.check(st, "rdetr_set_loss")
    return sums, dlogits, dbox[0], dbox[1]


class SetLossFunction(torch.autograd.Function):
    """``apply(logits, boxes, match, gt_boxes, gt_labels, n_split, inv_norm_a, inv_norm_b, alpha, gamma) -> sums [R, 2, 3]``,
    differentiable with respect to logits and boxes.  The forward launch already wrote the gradients; the backward scales them by
    the upstream gradient of their row and segment."""

    @staticmethod
    def forward(ctx, logits, boxes, match, gt_boxes, gt_labels, n_split, inv_norm_a, inv_norm_b, alpha, gamma):
        sums, dlogits, dbox_l1, dbox_giou = set_loss_forward(logits, boxes, match, gt_boxes, gt_labels, n_split, inv_norm_a, inv_norm_b,
                                                             alpha, gamma)
        ctx.save_for_backward(dlogits, dbox_l1, dbox_giou)
        ctx.n_split = int(n_split)
        return sums

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_sums):
        dlogits, dbox_l1, dbox_giou = ctx.saved_tensors
        R, N, _ = dlogits.shape
        g = grad_sums.to(torch.float32)
        per_query = torch.cat((g[:, :1].expand(R, ctx.n_split, 3), g[:, 1:].expand(R, N - ctx.n_split, 3)), dim=1)     # [R, N, 3]
        grad_logits = grad_boxes = None
        if ctx.needs_input_grad[0]:
            grad_logits = (dlogits * per_query[..., 0:1]).to(dlogits.dtype)
        if ctx.needs_input_grad[1]:
            grad_boxes = dbox_l1 * per_query[..., 1:2] + dbox_giou * per_query[..., 2:3]
        return grad_logits, grad_boxes, None, None, None, None, None, None, None, None


def set_loss(logits: Tensor, boxes: Tensor, match: Tensor, gt_boxes: Tensor, gt_labels: Tensor, n_split: int, inv_norm_a: float,
             inv_norm_b: float, alpha: float = 0.25, gamma: float = 2.0, fused: bool = True) -> Tensor:
    """Loss sums ``[R, 2, 3]`` of a stack of matched sets: per row and segment {varifocal class loss, L1, GIoU loss}, unweighted.

    ``match`` [R, N] int32 holds each query's gt index in the tables of image ``r % B``, or -1.  Queries below ``n_split`` are
    segment 0 (the denoising queries), scaled by ``inv_norm_a``; the rest segment 1, scaled by ``inv_norm_b``.  Differentiable with
    respect to logits and boxes on both routes."""
    if fused and logits.is_cuda:
        return SetLossFunction.apply(logits, boxes, match, gt_boxes, gt_labels, n_split, inv_norm_a, inv_norm_b, alpha, gamma)
    return _set_loss_torch(logits, boxes, match, gt_boxes, gt_labels, n_split, inv_norm_a, inv_norm_b, alpha, gamma)


# -------------------------------------------------------------------------------------------------------------------- criterion
_NAMES = ("loss_class", "loss_bbox", "loss_giou")


def _layer_keys(L: int) -> List[str]:
    """Key suffixes of the L decoder layers in stack order: ``_{i}`` for the earlier layers, none for the last."""
    return [f"_{i}" for i in range(L - 1)] + [""]


class RelationCriterion(nn.Module):
    """The loss of Relation-DETR from the transformer's eight training outputs.

    ``forward(outputs, targets, dn_meta=None)``: ``outputs`` is what ``RelationTransformer.forward`` returns in training mode,
    ``targets`` the list of ``{"labels": int64 [G_b], "boxes": [G_b, 4] cxcywh in (0, 1)}`` (``G_b = 0`` allowed) and ``dn_meta =
    (denoising_groups, max_gt_num_per_image)`` of the denoising generator (``models/bricks/denoising.py:325-331``): the first
    ``groups * max_gt`` queries of ``outputs[0]`` / ``outputs[1]`` are the denoising queries, query ``g * max_gt + t`` matched to
    gt ``t``.  Returns the weighted dict of ``relation_detr.py:124-141``: ``loss_{class,bbox,giou}`` of the last decoder layer, the
    same with ``_{i}`` per earlier layer and ``_enc`` for the encoder proposals; ``_dn`` / ``_dn_{i}`` with ``dn_meta``; all of the
    first group again with ``_hybrid`` where the hybrid outputs are present.

    ``matcher`` ("scipy" or "device") chooses the fused route's assignment solver; a step whose shapes exceed ``MAX_ASSIGN``
    takes the scipy path.  The device matcher's ``status`` is not read inside the step (that would be a wait for the device): a
    cost that is not finite comes from predictions that are not finite, and those already give losses that are not finite."""

    def __init__(self, num_classes: int, cost_class: float = 2.0, cost_bbox: float = 5.0, cost_giou: float = 2.0, loss_class: float = 1.0,
                 loss_bbox: float = 5.0, loss_giou: float = 2.0, alpha: float = 0.25, gamma: float = 2.0, hybrid_assign: int = 6,
                 fused: bool = True, two_stage_binary_cls: bool = False, mixed_match: bool = False, matcher: str = "scipy"):
        super().__init__()
        if matcher not in ("scipy", "device"):
            raise ValueError(f"RelationCriterion: matcher has to be 'scipy' or 'device', got {matcher!r}")
        if two_stage_binary_cls or mixed_match:
            raise NotImplementedError("RelationCriterion: two_stage_binary_cls and mixed_match are not built")
        if cost_class == 0 and cost_bbox == 0 and cost_giou == 0:
            raise ValueError("all costs cant be 0")
        self.num_classes = int(num_classes)
        self.costs = (float(cost_class), float(cost_bbox), float(cost_giou))
        self.weights = (float(loss_class), float(loss_bbox), float(loss_giou))
        self.alpha, self.gamma = float(alpha), float(gamma)
        self.hybrid_assign = int(hybrid_assign)
        self.fused = bool(fused)
        self.matcher = matcher

    # -- shared
    @staticmethod
    def _num_boxes(total: int, device) -> float:
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            n = torch.as_tensor([total], dtype=torch.float, device=device)
            torch.distributed.all_reduce(n)
            return torch.clamp(n / torch.distributed.get_world_size(), min=1).item()
        return float(max(total, 1))

    def _unpack(self, outputs, dn_meta):
        if len(outputs) != 8:
            raise ValueError("RelationCriterion: outputs has to be the 8-tuple RelationTransformer.forward returns in training mode")
        cls, box, enc_cls, enc_box, hyb_cls, hyb_box, hyb_enc_cls, hyb_enc_box = outputs
        if cls.dim() != 4 or cls.shape[-1] != self.num_classes:
            raise ValueError(f"RelationCriterion: decoder classes have to be [L, B, N, {self.num_classes}]")
        n_dn = 0
        if dn_meta is not None:
            groups, max_gt = int(dn_meta[0]), int(dn_meta[1])
            n_dn = groups * max_gt
            if groups < 1 or n_dn > cls.shape[2]:
                raise ValueError("RelationCriterion: dn_meta does not fit the decoder outputs")
        return (cls, box), (enc_cls, enc_box), (hyb_cls, hyb_box), (hyb_enc_cls, hyb_enc_box), n_dn

    def forward(self, outputs, targets, dn_meta=None) -> Dict[str, Tensor]:
        dec, enc, hyb, hyb_enc, n_dn = self._unpack(outputs, dn_meta)
        if len(targets) != dec[0].shape[1]:
            raise ValueError("RelationCriterion: one target dict per image")
        counts = [int(t["labels"].shape[0]) for t in targets]
        if dn_meta is not None and max(counts) > int(dn_meta[1]):
            raise ValueError("RelationCriterion: an image has more boxes than dn_meta's max_gt_num_per_image")
        dev = dec[0].device
        num_boxes = self._num_boxes(sum(counts), dev)
        num_boxes_hybrid = num_boxes if hyb[0] is None else self._num_boxes(sum(counts) * self.hybrid_assign, dev)
        if self.fused and dec[0].is_cuda:
            return self._forward_fused(dec, enc, hyb, hyb_enc, n_dn, dn_meta, targets, counts, num_boxes, num_boxes_hybrid)
        return self._forward_torch(dec, enc, hyb, hyb_enc, n_dn, dn_meta, targets, counts, num_boxes, num_boxes_hybrid)

    # -- torch route: the reference's loops
    def _match_set(self, logits, boxes, gt_boxes, gt_labels, repeat):
        """``HungarianMatcher.forward`` per image of one set [B, N, *], the targets repeated ``repeat`` times."""
        from scipy.optimize import linear_sum_assignment

        indices = []
        with torch.no_grad():
            for b in range(logits.shape[0]):
                c = _image_cost(logits[b], boxes[b], gt_boxes[b].repeat(repeat, 1), gt_labels[b].repeat(repeat), *self.costs, self.alpha,
                                self.gamma)
                src, tgt = linear_sum_assignment(c.cpu())
                indices.append((torch.as_tensor(src), torch.as_tensor(tgt)))
        return indices

    def _forward_torch(self, dec, enc, hyb, hyb_enc, n_dn, dn_meta, targets, counts, num_boxes, num_boxes_hybrid):
        dt = dec[1].dtype
        gt_boxes = [t["boxes"].to(dt) for t in targets]
        gt_labels = [t["labels"] for t in targets]
        losses: Dict[str, Tensor] = {}

        def add(suffix, logits, boxes, indices, boxes_t, labels_t, norm):
            values = _set_losses(logits.to(dt), boxes, indices, boxes_t, labels_t, norm, self.alpha, self.gamma)
            for name, value, weight in zip(_NAMES, values, self.weights):
                losses[name + suffix] = value * weight

        def branch(tail, stack, proposals, skip, repeat, norm):
            boxes_t = [g.repeat(repeat, 1) for g in gt_boxes]
            labels_t = [lab.repeat(repeat) for lab in gt_labels]
            L = stack[0].shape[0]
            for suffix, l in zip([""] + [f"_{i}" for i in range(L - 1)], [L - 1] + list(range(L - 1))):
                logits, boxes = stack[0][l, :, skip:], stack[1][l, :, skip:]
                add(suffix + tail, logits, boxes, self._match_set(logits, boxes, gt_boxes, gt_labels, repeat), boxes_t, labels_t, norm)
            if proposals[0] is not None:
                add("_enc" + tail, proposals[0], proposals[1], self._match_set(*proposals, gt_boxes, gt_labels, repeat), boxes_t,
                    labels_t, norm)

        branch("", dec, enc, n_dn, 1, num_boxes)
        if dn_meta is not None:
            groups, max_gt = int(dn_meta[0]), int(dn_meta[1])
            dn_idx = []
            for g in counts:
                t = torch.arange(g).repeat(groups)
                dn_idx.append((torch.arange(groups).repeat_interleave(g) * max_gt + t, t))
            L = dec[0].shape[0]
            for suffix, l in zip(["_dn"] + [f"_dn_{i}" for i in range(L - 1)], [L - 1] + list(range(L - 1))):
                add(suffix, dec[0][l, :, :n_dn], dec[1][l, :, :n_dn], dn_idx, gt_boxes, gt_labels, num_boxes * groups)
        if hyb[0] is not None:
            branch("_hybrid", hyb, hyb_enc, 0, self.hybrid_assign, num_boxes_hybrid)
        return losses

    # -- fused route
    def _forward_fused(self, dec, enc, hyb, hyb_enc, n_dn, dn_meta, targets, counts, num_boxes, num_boxes_hybrid):
        dev = dec[0].device
        B = len(counts)
        Gmax = max(1, max(counts))
        if Gmax > MAX_GT:
            raise _lib.RdetrError(f"RelationCriterion: {Gmax} boxes in one image, the kernels take {MAX_GT}")
        gt_boxes = torch.zeros(B, Gmax, 4, dtype=torch.float32, device=dev)
        gt_labels = torch.zeros(B, Gmax, dtype=torch.int32, device=dev)
        for b, t in enumerate(targets):
            if counts[b]:
                gt_boxes[b, :counts[b]] = t["boxes"].to(device=dev, dtype=torch.float32)
                gt_labels[b, :counts[b]] = t["labels"].to(device=dev, dtype=torch.int32)
        gt_count = torch.tensor(counts, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)

        # the stacks: (key tail, logits [R, N, C], boxes [R, N, 4], queries skipped by the matcher, targets repeated, normaliser)
        stacks = [("", dec[0].flatten(0, 1), dec[1].flatten(0, 1), n_dn, 1, num_boxes)]
        if enc[0] is not None:
            stacks.append(("_enc", enc[0], enc[1], 0, 1, num_boxes))
        if hyb[0] is not None:
            stacks.append(("_hybrid", hyb[0].flatten(0, 1), hyb[1].flatten(0, 1), 0, self.hybrid_assign, num_boxes_hybrid))
            if hyb_enc[0] is not None:
                stacks.append(("_enc_hybrid", hyb_enc[0], hyb_enc[1], 0, self.hybrid_assign, num_boxes_hybrid))
        stacks = [(tail, lg, bx.float(), skip, rep, norm) for tail, lg, bx, skip, rep, norm in stacks]

        sizes = [lg.shape[0] * (lg.shape[1] - skip) * Gmax for _, lg, _, skip, _, _ in stacks]
        cost_dev = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        start = 0
        with torch.no_grad():
            for (_, lg, bx, skip, _, _), size in zip(stacks, sizes):
                match_cost(lg[:, skip:], bx[:, skip:], gt_boxes, gt_labels, gt_count, *self.costs, self.alpha, self.gamma,
                           out=cost_dev[start:start + size])
                start += size
        shapes = [(lg.shape[0], lg.shape[1]) for _, lg, *_ in stacks]
        ats = [sum(R * N for R, N in shapes[:k]) for k in range(len(shapes))]
        tables = [(at, R, N) for at, (R, N) in zip(ats, shapes)]
        device = self.matcher == "device" and all(N - skip <= MAX_ASSIGN and Gmax * rep <= MAX_ASSIGN
                                                  for (_, N), (_, _, _, skip, rep, _) in zip(shapes, stacks))
        if device:                                                            # no copy, no wait: the tables are solved where they are
            match_dev = torch.empty(sum(R * N for R, N in shapes), dtype=torch.int32, device=dev)
            start = at = k = 0
            while k < len(stacks):
                (R, N), (_, _, _, skip, rep, _) = shapes[k], stacks[k]
                # neighbours of one shape (a branch's layers and its proposals) are one taller stack, in both buffers: one launch,
                # and twice the workgroups of a kernel that is latency-bound
                while k + 1 < len(stacks) and (shapes[k + 1][1], *stacks[k + 1][3:5]) == (N, skip, rep):
                    k += 1
                    R += shapes[k][0]
                assign_match(cost_dev[start:start + R * (N - skip) * Gmax].view(R, N - skip, Gmax), gt_count, rep, skip,
                             dn_meta if skip else None, out=match_dev[at:at + R * N].view(R, N))
                start, at, k = start + R * (N - skip) * Gmax, at + R * N, k + 1
        else:
            cost_host = torch.empty(cost_dev.shape, dtype=torch.float32, pin_memory=True)
            cost_host.copy_(cost_dev, non_blocking=True)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(dev))
            done.synchronize()                                                # the step's only wait for the device
            match_host = torch.empty(sum(R * N for R, N in shapes), dtype=torch.int32).pin_memory()
            start = 0
            for (_, _, _, skip, rep, _), size, (at, R, N) in zip(stacks, sizes, tables):
                assign_match(cost_host[start:start + size].view(R, N - skip, Gmax), counts, rep, skip, dn_meta if skip else None,
                             out=match_host[at:at + R * N].view(R, N))
                start += size
            match_dev = match_host.to(dev, non_blocking=True)

        losses: Dict[str, Tensor] = {}
        weights = torch.tensor(self.weights, dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
        for (tail, lg, bx, skip, _, norm), (at, R, N) in zip(stacks, tables):
            groups = int(dn_meta[0]) if skip else 1
            sums = SetLossFunction.apply(lg, bx, match_dev[at:at + R * N].view(R, N), gt_boxes, gt_labels, skip, 1.0 / (norm * groups),
                                         1.0 / norm, self.alpha, self.gamma)
            values = (sums.view(R // B, B, 2, 3).sum(1) * weights).reshape(-1).unbind(0)      # L x {dn, matched} x 3 scalars, one node
            keys = [tail] if "_enc" in tail else [k + tail for k in _layer_keys(R // B)]      # proposals: one set per image
            for l, key in enumerate(keys):
                for i, name in enumerate(_NAMES):
                    losses[name + key] = values[(2 * l + 1) * 3 + i]
                    if skip:
                        losses[name + "_dn" + key] = values[2 * l * 3 + i]
        return losses
