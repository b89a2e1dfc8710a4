"""From (feature pyramid, targets) to the loss dict: the part of ``RelationDETR.forward`` behind backbone and neck
(``models/detectors/relation_detr.py:52-141``).

``RelationDETRHead(transformer, criterion, denoising_generator)`` keeps the reference detector's attribute names, so its
state-dict keys are the reference's minus ``backbone.*`` and ``neck.*``.  One deviation: when no image of the batch has a box the
reference still builds (empty) denoising queries and reports ``_dn`` losses of zero; here the transformer then runs without
denoising queries and the criterion with ``dn_meta=None``, so the dict has no ``_dn`` keys.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

from torch import Tensor, nn

from .criterion import RelationCriterion
from .denoising import GenerateCDNQueries, Noise
from .transformer import RelationTransformer


class RelationDETRHead(nn.Module):
    """``forward(multi_level_feats, multi_level_masks, multi_level_pos_embeds, targets=None, noise=None)``.

    Training mode: ``targets`` is the list of ``{"labels": int64 [G_b], "boxes": [G_b, 4] cxcywh in (0, 1)}``; the generator makes
    the denoising queries (``noise``: its four draws, None to draw them), the transformer runs with them and the criterion turns
    its eight outputs into the weighted loss dict.  Eval mode: the last decoder layer's ``(logits [B, N, C], boxes [B, N, 4])``."""

    def __init__(self, transformer: RelationTransformer, criterion: RelationCriterion, denoising_generator: GenerateCDNQueries):
        super().__init__()
        self.transformer = transformer
        self.criterion = criterion
        self.denoising_generator = denoising_generator

    def forward(self, multi_level_feats: Sequence[Tensor], multi_level_masks: Sequence[Tensor], multi_level_pos_embeds: Sequence[Tensor],
                targets: Optional[Sequence[Dict[str, Tensor]]] = None, noise: Optional[Noise] = None):
        if not self.training:
            classes, coords, *_ = self.transformer(multi_level_feats, multi_level_masks, multi_level_pos_embeds)
            return classes[-1], coords[-1]
        if targets is None:
            raise ValueError("RelationDETRHead: training mode needs targets")
        if not any(int(t["labels"].numel()) for t in targets):                   # no box in the batch: no denoising part at all
            outputs = self.transformer(multi_level_feats, multi_level_masks, multi_level_pos_embeds)
            return self.criterion(outputs, targets, dn_meta=None)
        label_query, box_query, attn_mask, groups, group_size = self.denoising_generator(
            [t["labels"] for t in targets], [t["boxes"] for t in targets], noise=noise)
        outputs = self.transformer(multi_level_feats, multi_level_masks, multi_level_pos_embeds, label_query, box_query, attn_mask)
        return self.criterion(outputs, targets, dn_meta=(groups, group_size))
