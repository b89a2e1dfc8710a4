"""From (feature pyramid, targets) to the loss dict: the part of ``RelationDETR.forward`` behind backbone and neck
(``models/detectors/relation_detr.py:52-141``).

``RelationDETRHead(transformer, criterion, denoising_generator)`` keeps the reference detector's attribute names, so its
state-dict keys are the reference's minus ``backbone.*`` and ``neck.*``; ``RelationDETR(neck, position_embedding, transformer, criterion,
denoising_generator)`` puts the neck and the position encoding in front, so its keys are the reference's minus ``backbone.*`` and its
``forward`` starts at the backbone's feature maps and the padding mask; ``RelationDETRWithBackbone(backbone, ..., preprocessor)`` starts at
the list of images, as the reference's detector does, and in eval mode ends at the detections.  One deviation: when no image of the batch has a box the
reference still builds (empty) denoising queries and reports ``_dn`` losses of zero; here the transformer then runs without
denoising queries and the criterion with ``dn_meta=None``, so the dict has no ``_dn`` keys.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
from torch import Tensor, nn

from .criterion import RelationCriterion
from .denoising import GenerateCDNQueries, Noise
from .neck import build_pyramid
from .transformer import RelationTransformer, select_detections


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


class RelationDETR(RelationDETRHead):
    """``forward(features, mask, targets=None, noise=None)``: ``features`` the backbone's maps (dict or sequence, contiguous NCHW),
    ``mask`` the image-level padding mask ``[B, H, W]`` (non-zero = padded).  The pyramid is built as ``PyramidBuilder`` does
    (``DETRDetector.get_multi_levels`` behind the backbone), the rest is ``RelationDETRHead.forward``.

    The attributes are the reference detector's (``neck``, ``position_embedding``, ``transformer``, ``criterion``,
    ``denoising_generator``), so ``state_dict()`` holds ``neck.convs.{i}.0.weight``, ``neck.convs.{i}.1.{weight,bias}`` and the head's
    keys; ``position_embedding`` contributes none.  ``relation_param_groups`` sorts the neck by name like every other parameter,
    as the reference does: ``neck.convs.{i}.0.weight`` and ``neck.convs.{i}.1.weight`` (no "norm" in the name) fall in the default
    group, ``neck.convs.{i}.1.bias`` in the no-decay group of the other biases.  ``train_step(model, optimizer, features, mask, None,
    targets)`` steps them with the rest."""

    def __init__(self, neck: nn.Module, position_embedding: nn.Module, transformer: RelationTransformer, criterion: RelationCriterion,
                 denoising_generator: GenerateCDNQueries):
        nn.Module.__init__(self)
        self.neck = neck
        self.position_embedding = position_embedding
        self.transformer = transformer
        self.criterion = criterion
        self.denoising_generator = denoising_generator

    def get_multi_levels(self, features, mask: Tensor, dtype=None):
        return build_pyramid(self.neck, self.position_embedding, features, mask, dtype)

    def forward(self, features, mask: Tensor, targets: Optional[Sequence[Dict[str, Tensor]]] = None, noise: Optional[Noise] = None):
        feats, masks, pos = self.get_multi_levels(features, mask)
        return RelationDETRHead.forward(self, feats, masks, pos, targets, noise)


class RelationDETRWithBackbone(RelationDETR):
    """``forward(images, targets=None, noise=None)``, the reference's ``RelationDETR.forward(images, targets)``: ``images`` a list of
    ``[3, h, w]`` tensors (eval: uint8 or float in [0, 1], any sizes; training: augmented, float, normalised), ``targets`` with
    ``boxes`` in xyxy pixels.  ``preprocessor`` (``frontend.ImagePreprocessor``) makes the batch, the mask and the prepared targets,
    ``backbone`` -- ``backbones.ResNetBackbone`` or the caller's module -- maps ``batch.tensors`` to the feature maps
    ``RelationDETR.forward`` takes.  ``relation_detr_r50`` assembles the reference's R50 configuration.

    Training mode returns the loss dict.  Eval mode returns ``(detections, tensor)``: ``tensor`` is ``select_detections``' ``[B, k, 6]``
    = (x1, y1, x2, y2, score, label) in pixels of the ORIGINAL images, ``detections`` the reference's list of
    ``{"scores", "labels", "boxes"}`` as views of it.

    The attributes are the reference detector's, so ``state_dict()`` holds ``backbone.*`` and what ``RelationDETR`` holds; the
    preprocessor has neither parameters nor buffers."""

    def __init__(self, backbone: nn.Module, neck: nn.Module, position_embedding: nn.Module, transformer: RelationTransformer,
                 criterion: RelationCriterion, denoising_generator: GenerateCDNQueries, preprocessor: nn.Module, num_select: int = 300):
        RelationDETR.__init__(self, neck, position_embedding, transformer, criterion, denoising_generator)
        self.backbone = backbone
        self.preprocessor = preprocessor
        self.num_select = num_select

    def forward(self, images, targets: Optional[Sequence[Dict[str, Tensor]]] = None, noise: Optional[Noise] = None):
        batch, targets = self.preprocessor(images, targets)
        features = self.backbone(batch.tensors)
        outputs = RelationDETR.forward(self, features, batch.mask, targets, noise)
        if self.training:
            return outputs
        logits, boxes = outputs
        return self.detections(logits, boxes, batch.original_sizes)

    def detections(self, logits: Tensor, boxes: Tensor, original_sizes: Tensor):
        sizes = original_sizes.to(device=logits.device, dtype=torch.int64)
        dets = select_detections(logits.float(), boxes.float(), sizes, self.num_select)
        return [{"scores": d[:, 4], "labels": d[:, 5].to(torch.int64), "boxes": d[:, :4]} for d in dets], dets


def relation_detr_r50(num_classes: int = 91, weights=None, num_queries: int = 900, hybrid_num_proposals: int = 1500, hybrid_assign: int = 6,
                      enc_layers: int = 6, dec_layers: int = 6, d_ffn: int = 2048, denoising_nums: int = 100, min_size: int = 800,
                      max_size: int = 1333, num_select: int = 300, fused: bool = True, **transformer_kwargs) -> RelationDETRWithBackbone:
    """``configs/relation_detr/relation_detr_resnet50_800_1333.py`` from this package's parts: ``ResNetBackbone("resnet50",
    return_indices=(1, 2, 3), freeze_indices=(0,))`` with ``FrozenBatchNorm2d``, a four-level ``ChannelMapper`` to 256 channels, the
    normalised sine position encoding with offset -0.5, the 6 + 6 layer transformer, the hybrid criterion, 100 denoising pairs and
    the 800 / 1333 front end.  ``weights``: the backbone's state dict or a local path (``ResNetBackbone``'s argument).  The size
    arguments are there for reduced models; ``transformer_kwargs`` go to ``build_relation_transformer``."""
    from .backbones import ResNetBackbone
    from .frontend import ImagePreprocessor
    from .neck import ChannelMapper, PositionEmbeddingSine
    from .transformer import build_relation_transformer
    embed_dim, levels = 256, 4
    backbone = ResNetBackbone("resnet50", weights=weights, return_indices=(1, 2, 3), freeze_indices=(0,), fused=fused)
    transformer = build_relation_transformer(num_classes=num_classes, embed_dim=embed_dim, d_ffn=d_ffn, num_levels=levels,
                                             enc_layers=enc_layers, dec_layers=dec_layers, num_queries=num_queries,
                                             hybrid_num_proposals=hybrid_num_proposals, **transformer_kwargs)
    return RelationDETRWithBackbone(
        backbone, ChannelMapper(backbone.num_channels, embed_dim, levels, fused=fused),
        PositionEmbeddingSine(embed_dim // 2, 10000, True, offset=-0.5, fused=fused), transformer,
        RelationCriterion(num_classes, hybrid_assign=hybrid_assign, fused=fused),
        GenerateCDNQueries(num_queries=num_queries, num_classes=num_classes, label_embed_dim=embed_dim, denoising_nums=denoising_nums,
                           fused=fused),
        ImagePreprocessor(min_size, max_size, fused=fused), num_select)


def relation_detr_swin_l(num_classes: int = 91, weights=None, num_queries: int = 900, hybrid_num_proposals: int = 1500, hybrid_assign: int = 6,
                         enc_layers: int = 6, dec_layers: int = 6, d_ffn: int = 2048, denoising_nums: int = 100, min_size: int = 800,
                         max_size: int = 1333, num_select: int = 300, fused: bool = True, arch: str = "swin_l", backbone_kwargs=None,
                         **transformer_kwargs) -> RelationDETRWithBackbone:
    """``configs/relation_detr/relation_detr_swin_l_800_1333.py`` from this package's parts: ``SwinTransformerBackbone("swin_l",
    return_indices=(1, 2, 3), freeze_indices=(0,))``, and behind it what ``relation_detr_r50`` assembles: the four-level
    ``ChannelMapper`` to 256 channels, the sine position encoding, the 6 + 6 layer transformer, the hybrid criterion, 100 denoising
    pairs and the 800 / 1333 front end.  ``weights``: the backbone's state dict or a local path (``SwinTransformerBackbone``'s
    argument).  ``arch`` and ``backbone_kwargs`` (entries of the architecture: ``embed_dim``, ``depths``, ``num_heads``, ...) and the
    size arguments are there for reduced models; ``transformer_kwargs`` go to ``build_relation_transformer``."""
    from .backbones import SwinTransformerBackbone
    from .frontend import ImagePreprocessor
    from .neck import ChannelMapper, PositionEmbeddingSine
    from .transformer import build_relation_transformer
    embed_dim, levels = 256, 4
    backbone = SwinTransformerBackbone(arch, weights=weights, return_indices=(1, 2, 3), freeze_indices=(0,), fused=fused,
                                       **(backbone_kwargs or {}))
    transformer = build_relation_transformer(num_classes=num_classes, embed_dim=embed_dim, d_ffn=d_ffn, num_levels=levels,
                                             enc_layers=enc_layers, dec_layers=dec_layers, num_queries=num_queries,
                                             hybrid_num_proposals=hybrid_num_proposals, **transformer_kwargs)
    return RelationDETRWithBackbone(
        backbone, ChannelMapper(backbone.num_channels, embed_dim, levels, fused=fused),
        PositionEmbeddingSine(embed_dim // 2, 10000, True, offset=-0.5, fused=fused), transformer,
        RelationCriterion(num_classes, hybrid_assign=hybrid_assign, fused=fused),
        GenerateCDNQueries(num_queries=num_queries, num_classes=num_classes, label_embed_dim=embed_dim, denoising_nums=denoising_nums,
                           fused=fused),
        ImagePreprocessor(min_size, max_size, fused=fused), num_select)
