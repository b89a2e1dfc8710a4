"""Backbones: image batch -> feature maps.  ``resnet`` holds the modules, ``epilogue`` the kernel calls between their convolutions."""
from .epilogue import (FrozenBNActFunction, frozen_bn_act, frozen_bn_act_backward, frozen_bn_act_forward, stem_bn_relu_maxpool)
from .resnet import ARCHITECTURES, BasicBlock, Bottleneck, FrozenBatchNorm2d, ResNet, ResNetBackbone
from .swin import PatchMerging, ShiftedWindowAttention, SwinTransformer, SwinTransformerBackbone, SwinTransformerBlock

__all__ = ["ARCHITECTURES", "BasicBlock", "Bottleneck", "FrozenBatchNorm2d", "ResNet", "ResNetBackbone", "FrozenBNActFunction",
           "frozen_bn_act", "frozen_bn_act_forward", "frozen_bn_act_backward", "stem_bn_relu_maxpool",
           "PatchMerging", "ShiftedWindowAttention", "SwinTransformerBlock", "SwinTransformer", "SwinTransformerBackbone"]
