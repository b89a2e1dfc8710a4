"""relation_detr_amd -- MI355X-native hot path of Relation-DETR.

Multi-scale deformable attention + position-relation attention bias as hand-written gfx950 HIP
kernels behind a C ABI (include/relation_detr_amd.h), with the reference's nn.Module API on top.
"""
from .ms_deform_attn import MultiScaleDeformableAttention
from .relation import PositionRelationEmbedding, PositionRelationEncoder, box_rel_encoding
from .self_attn import RelationSelfAttention
from .transformer import RelationTransformer, build_relation_transformer, select_detections
from .ops import (MultiScaleDeformableAttnFunction, MultiScaleDeformableAttnFusedFunction, RelationAttentionFunction, bias_softmax_,
                  ms_deform_attn_backward, ms_deform_attn_backward_fused, ms_deform_attn_forward, ms_deform_attn_forward_fused,
                  relation_attention_backward, relation_attention_train, relation_bias)
from .attn_rel_train import RelationAttentionBoxesFunction, relation_attention_boxes_backward, relation_attention_boxes_train
from .ffn_train import FeedForwardFunction, ffn_k256_backward, ffn_k256_train
from .ln_train import AddLayerNormFunction
from .amp_train import AddLayerNormMixedFunction, FeedForwardMixedFunction
from .msda_train_hm import MultiScaleDeformableAttnHeadMajorFunction, grad_value_from_head_major, ms_deform_attn_backward_fused_hm
from .criterion import RelationCriterion, SetLossFunction, assign_match, hungarian_match, match_cost, set_loss
from .denoising import CdnQueryFunction, GenerateCDNQueries, cdn_noise, cdn_queries, denoising_mask
from .detector import RelationDETR, RelationDETRHead, RelationDETRWithBackbone, relation_detr_r50, relation_detr_swin_l
from .neck import (ChannelMapper, GroupNormLevelsFunction, PositionEmbeddingSine, PyramidBuilder, group_norm_levels, pyramid_masks,
                   pyramid_sine_pos)
from .optim import FusedAdamW, relation_param_groups, train_step
from .frontend import (DetrAugment, DetrChoice, ImageBatch, ImagePreprocessor, batch_images, detr_plan, resized_size, sample_detr_choices,
                       shortest_size, transform_targets)
from .backbones import (FrozenBatchNorm2d, PatchMerging, ResNet, ResNetBackbone, ShiftedWindowAttention, SwinTransformer,
                        SwinTransformerBackbone, SwinTransformerBlock)

__all__ = [
    "MultiScaleDeformableAttention", "PositionRelationEmbedding", "PositionRelationEncoder", "box_rel_encoding",
    "RelationSelfAttention", "RelationTransformer", "build_relation_transformer", "select_detections",
    "MultiScaleDeformableAttnFunction", "MultiScaleDeformableAttnFusedFunction", "ms_deform_attn_forward",
    "ms_deform_attn_forward_fused", "ms_deform_attn_backward", "ms_deform_attn_backward_fused", "relation_bias", "bias_softmax_",
    "RelationAttentionFunction", "relation_attention_train", "relation_attention_backward",
    "RelationAttentionBoxesFunction", "relation_attention_boxes_train", "relation_attention_boxes_backward",
    "FeedForwardFunction", "ffn_k256_train", "ffn_k256_backward", "AddLayerNormFunction",
    "MultiScaleDeformableAttnHeadMajorFunction", "ms_deform_attn_backward_fused_hm", "grad_value_from_head_major",
    "AddLayerNormMixedFunction", "FeedForwardMixedFunction",
    "RelationCriterion", "SetLossFunction", "match_cost", "hungarian_match", "assign_match", "set_loss",
    "GenerateCDNQueries", "CdnQueryFunction", "cdn_queries", "cdn_noise", "denoising_mask", "RelationDETRHead",
    "FusedAdamW", "relation_param_groups", "train_step",
    "ChannelMapper", "PositionEmbeddingSine", "PyramidBuilder", "RelationDETR", "GroupNormLevelsFunction", "group_norm_levels",
    "pyramid_masks", "pyramid_sine_pos",
    "ImageBatch", "ImagePreprocessor", "batch_images", "resized_size", "RelationDETRWithBackbone",
    "DetrAugment", "DetrChoice", "detr_plan", "sample_detr_choices", "shortest_size", "transform_targets",
    "FrozenBatchNorm2d", "ResNet", "ResNetBackbone", "relation_detr_r50",
    "PatchMerging", "ShiftedWindowAttention", "SwinTransformerBlock", "SwinTransformer", "SwinTransformerBackbone", "relation_detr_swin_l",
]
