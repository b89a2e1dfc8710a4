"""The ResNet family as the reference's detector uses it (``models/backbones/resnet.py``, ``models/bricks/misc.py``): torchvision's
ResNet v1.5 with ``FrozenBatchNorm2d``, cut behind the last returned stage.

Two routes, as in ``neck.py``.  ``forward_torch`` is the reference's operator sequence: after every convolution ``x * scale``,
``+ bias`` and the in-place ReLU as separate passes, ``out += identity`` at a block's tail, ``MaxPool2d`` behind the stem.
``forward_fused`` keeps the library convolutions and runs everything between them through ``epilogue.frozen_bn_act`` (in place on
the convolution's result, the residual added in the same pass) and ``epilogue.stem_bn_relu_maxpool``.  In fp32 the two routes
differ only by what the convolution library does with its own operands: the epilogues are the reference's arithmetic bit for bit,
forward and backward.

Deviations, both on the fused route only: under ``torch.autocast(bfloat16)`` the epilogues keep the convolutions' bf16 where the
reference's ``bf16 * fp32`` promotion returns fp32 maps (the neck's documented deviation); and a ``.to(bfloat16)`` model keeps
``scale`` and ``shift`` in fp32, computed from the buffers, where the reference rounds both to bf16 and every intermediate with them.
"""
from __future__ import annotations

import functools
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Type, Union

import torch
from torch import Tensor, nn
from torch.nn.modules.batchnorm import _BatchNorm

from .. import derived
from .epilogue import frozen_bn_act, stem_bn_relu_maxpool

_FUSED_DTYPES = (torch.float32, torch.bfloat16)

# FrozenBatchNorm2d's folded (scale, shift) pair: sources are the module's four buffers
_SCALE_SHIFT = derived.DerivedCache(kind="frozen_bn_scale_shift")


def _scale_shift(eps, weight, bias, running_mean, running_var):
    w, b, rm, rv = (t.detach().float() for t in (weight, bias, running_mean, running_var))
    scale = w * (rv + eps).rsqrt()
    return scale, b - rm * scale


def _fill_scale_shift(eps, pair, *buffers):
    for dst, src in zip(pair, _scale_shift(eps, *buffers)):
        dst.copy_(src)


class FrozenBatchNorm2d(nn.Module):
    """BatchNorm2d with fixed statistics and affine parameters: four buffers (``weight``, ``bias``, ``running_mean``,
    ``running_var``), no parameter; ``num_batches_tracked`` of a checkpoint is dropped on load."""

    def __init__(self, num_features: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        state_dict.pop(prefix + "num_batches_tracked", None)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, x: Tensor) -> Tensor:
        w, b = self.weight.reshape(1, -1, 1, 1), self.bias.reshape(1, -1, 1, 1)
        rv, rm = self.running_var.reshape(1, -1, 1, 1), self.running_mean.reshape(1, -1, 1, 1)
        scale = w * (rv + self.eps).rsqrt()
        bias = b - rm * scale
        return x * scale + bias

    def scale_shift(self) -> Tuple[Tensor, Tensor]:
        """The fp32 ``[C]`` pair ``forward`` multiplies and adds: ``w * (rv + eps).rsqrt()`` and ``b - rm * scale``, the same
        operations on the same device.  Computed once per state of the buffers (their ``_version``, storage and device)."""
        buffers = (self.weight, self.bias, self.running_mean, self.running_var)
        eps = self.eps

        def build():
            with torch.no_grad():
                return _scale_shift(eps, *buffers)
        fill = functools.partial(_fill_scale_shift, eps) if derived.active() is not None else None      # only a ledger keeps it
        return _SCALE_SHIFT.get(buffers, build, fill, extra=eps)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.weight.shape[0]}, eps={self.eps})"


def conv3x3(cin: int, cout: int, stride: int = 1, groups: int = 1, dilation: int = 1) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, 3, stride=stride, padding=dilation, groups=groups, bias=False, dilation=dilation)


def conv1x1(cin: int, cout: int, stride: int = 1) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, 1, stride=stride, bias=False)


def _no_dcn(with_dcn: bool) -> None:
    if with_dcn:
        raise NotImplementedError("deformable convolution (stage_with_dcn / with_dcn) is not part of this package")


def _fused_norm(conv: nn.Module, norm: FrozenBatchNorm2d, x: Tensor, residual: Optional[Tensor] = None, relu: bool = True) -> Tensor:
    y = conv(x)
    return frozen_bn_act(y, *norm.scale_shift(), residual=residual, relu=relu, out=y)


class _Block(nn.Module):
    def _identity_torch(self, x: Tensor) -> Tensor:
        return x if self.downsample is None else self.downsample(x)

    def _identity_fused(self, x: Tensor) -> Tensor:
        return x if self.downsample is None else _fused_norm(self.downsample[0], self.downsample[1], x, relu=False)

    def forward(self, x: Tensor) -> Tensor:
        return self.forward_torch(x)


class BasicBlock(_Block):
    expansion: int = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None, groups: int = 1,
                 base_width: int = 64, dilation: int = 1, norm_layer: Optional[Callable[..., nn.Module]] = None, with_dcn: bool = False):
        super().__init__()
        _no_dcn(with_dcn)
        norm_layer = nn.BatchNorm2d if norm_layer is None else norm_layer
        if groups != 1 or base_width != 64:
            raise ValueError("BasicBlock only supports groups=1 and base_width=64")
        if dilation > 1:
            raise NotImplementedError("Dilation > 1 not supported in BasicBlock")
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = norm_layer(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = norm_layer(planes)
        self.downsample = downsample
        self.stride = stride

    def forward_torch(self, x: Tensor) -> Tensor:
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        out += self._identity_torch(x)
        return self.relu(out)

    def forward_fused(self, x: Tensor) -> Tensor:
        out = _fused_norm(self.conv1, self.bn1, x)
        return _fused_norm(self.conv2, self.bn2, out, residual=self._identity_fused(x))


class Bottleneck(_Block):
    """The v1.5 bottleneck: the stride sits on the 3x3 convolution."""
    expansion: int = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None, groups: int = 1,
                 base_width: int = 64, dilation: int = 1, norm_layer: Optional[Callable[..., nn.Module]] = None, with_dcn: bool = False):
        super().__init__()
        _no_dcn(with_dcn)
        norm_layer = nn.BatchNorm2d if norm_layer is None else norm_layer
        width = int(planes * (base_width / 64.0)) * groups
        self.conv1 = conv1x1(inplanes, width)
        self.bn1 = norm_layer(width)
        self.conv2 = conv3x3(width, width, stride, groups, dilation)
        self.bn2 = norm_layer(width)
        self.conv3 = conv1x1(width, planes * self.expansion)
        self.bn3 = norm_layer(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward_torch(self, x: Tensor) -> Tensor:
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        out += self._identity_torch(x)
        return self.relu(out)

    def forward_fused(self, x: Tensor) -> Tensor:
        out = _fused_norm(self.conv1, self.bn1, x)
        out = _fused_norm(self.conv2, self.bn2, out)
        return _fused_norm(self.conv3, self.bn3, out, residual=self._identity_fused(x))


class ResNet(nn.Module):
    """The reference's constructor arguments and attribute names (``conv1``, ``bn1``, ``layer1..4``, ``downsample.0/.1``), plus two
    keyword-only ones of this package: ``stages`` (how many of ``layer1..4`` are built) and ``head`` (``avgpool`` and ``fc``).
    ``forward`` is the classifier's when there is a head, else the list of stage outputs."""

    def __init__(self, block: Type[Union[BasicBlock, Bottleneck]], layers: Sequence[int], num_classes: int = 1000,
                 zero_init_residual: bool = False, groups: int = 1, width_per_group: int = 64,
                 replace_stride_with_dilation: Optional[Sequence[bool]] = None, stage_with_dcn: Optional[Sequence[bool]] = None,
                 norm_layer: Optional[Callable[..., nn.Module]] = None, *, stages: int = 4, head: bool = True, fused: bool = True):
        super().__init__()
        if stage_with_dcn is not None and any(stage_with_dcn):
            _no_dcn(True)
        norm_layer = nn.BatchNorm2d if norm_layer is None else norm_layer
        if replace_stride_with_dilation is None:
            replace_stride_with_dilation = [False, False, False]
        if len(replace_stride_with_dilation) != 3:
            raise ValueError(f"replace_stride_with_dilation should be None or a 3-element tuple, got {replace_stride_with_dilation}")
        if not 1 <= stages <= 4 or (head and stages != 4):
            raise ValueError("ResNet: 1 <= stages <= 4, and a head needs all four")
        self._norm_layer = norm_layer
        self.inplanes, self.dilation = 64, 1
        self.groups, self.base_width = groups, width_per_group
        self.num_stages, self.fused = stages, bool(fused)
        self.conv1 = nn.Conv2d(3, self.inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        dilate = [False] + list(replace_stride_with_dilation)
        for i in range(stages):
            setattr(self, f"layer{i + 1}", self._make_layer(block, 64 << i, layers[i], stride=1 if i == 0 else 2, dilate=dilate[i]))
        if head:
            self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
            self.fc = nn.Linear(512 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if zero_init_residual:
            for m in self.modules():
                last = m.bn3 if isinstance(m, Bottleneck) else (m.bn2 if isinstance(m, BasicBlock) else None)
                if last is not None and isinstance(getattr(last, "weight", None), Tensor):
                    nn.init.constant_(last.weight, 0)
        self._frozen_norms = all(type(m) is FrozenBatchNorm2d for m in self.modules() if _is_norm(m))

    def _make_layer(self, block, planes: int, blocks: int, stride: int = 1, dilate: bool = False) -> nn.Sequential:
        norm_layer, downsample, previous_dilation = self._norm_layer, None, self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * block.expansion, stride), norm_layer(planes * block.expansion))
        made = [block(self.inplanes, planes, stride, downsample, self.groups, self.base_width, previous_dilation, norm_layer)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            made.append(block(self.inplanes, planes, groups=self.groups, base_width=self.base_width, dilation=self.dilation,
                              norm_layer=norm_layer))
        return nn.Sequential(*made)

    # ---- routes -------------------------------------------------------------------------------------------------------------
    def takes_fused_route(self, x: Tensor) -> bool:
        """The kernels take the input: ``fused`` is on, every norm is this package's ``FrozenBatchNorm2d``, the input is on a ROCm
        device, and it and the weights are fp32 or bf16 (an autocast to anything but bf16 takes the torch route)."""
        if not (self.fused and self._frozen_norms and isinstance(x, Tensor) and x.is_cuda):
            return False
        if x.dtype not in _FUSED_DTYPES or self.conv1.weight.dtype not in _FUSED_DTYPES:
            return False
        if torch.is_autocast_enabled():
            return torch.get_autocast_dtype("cuda") == torch.bfloat16
        return x.dtype == self.conv1.weight.dtype

    def stages_torch(self, x: Tensor) -> List[Tensor]:
        """The reference's operator sequence, on any device."""
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        outs = []
        for i in range(self.num_stages):
            for block in getattr(self, f"layer{i + 1}"):
                x = block.forward_torch(x)
            outs.append(x)
        return outs

    def stages_fused(self, x: Tensor) -> List[Tensor]:
        """The same network with csrc/backbone.hip between the convolutions.  The stem's fused tail is forward only, so it runs
        where the stem's output needs no gradient (a frozen stem: every configuration of the reference freezes ``conv1`` / ``bn1``);
        otherwise the stem takes torch's operators and the stages the kernels."""
        y = self.conv1(x)
        if torch.is_grad_enabled() and y.requires_grad:
            x = self.maxpool(self.relu(self.bn1(y)))
        else:
            x = stem_bn_relu_maxpool(y, *self.bn1.scale_shift())
        outs = []
        for i in range(self.num_stages):
            for block in getattr(self, f"layer{i + 1}"):
                x = block.forward_fused(x)
            outs.append(x)
        return outs

    def stages(self, x: Tensor) -> List[Tensor]:
        return self.stages_fused(x) if self.takes_fused_route(x) else self.stages_torch(x)

    def forward(self, x: Tensor):
        outs = self.stages(x)
        if not hasattr(self, "fc"):
            return outs
        return self.fc(torch.flatten(self.avgpool(outs[-1]), 1))

    def train(self, mode: bool = True):
        """Training mode for everything but the norms, which stay in eval mode."""
        super().train(mode)
        for m in self.modules():
            if _is_norm(m):
                m.eval()
        return self


def _is_norm(m: nn.Module) -> bool:
    return isinstance(m, (_BatchNorm, FrozenBatchNorm2d))


# name -> (block, blocks per stage, groups, width per group): the reference's table without the checkpoint URLs
ARCHITECTURES: Dict[str, Tuple[type, Tuple[int, int, int, int], int, int]] = {
    "resnet18": (BasicBlock, (2, 2, 2, 2), 1, 64),
    "resnet34": (BasicBlock, (3, 4, 6, 3), 1, 64),
    "resnet50": (Bottleneck, (3, 4, 6, 3), 1, 64),
    "resnet101": (Bottleneck, (3, 4, 23, 3), 1, 64),
    "resnet152": (Bottleneck, (3, 8, 36, 3), 1, 64),
    "resnext50_32x4d": (Bottleneck, (3, 4, 6, 3), 32, 4),
    "resnext101_32x4d": (Bottleneck, (3, 4, 23, 3), 32, 4),
    "resnext101_32x8d": (Bottleneck, (3, 4, 23, 3), 32, 8),
    "resnext101_64x4d": (Bottleneck, (3, 4, 23, 3), 64, 4),
    "wide_resnet50_2": (Bottleneck, (3, 4, 6, 3), 1, 128),
    "wide_resnet101_2": (Bottleneck, (3, 4, 23, 3), 1, 128),
}


class ResNetBackbone(ResNet):
    """``ResNetBackbone(arch, weights=None, return_indices=(0, 1, 2, 3), freeze_indices=(), norm_layer=FrozenBatchNorm2d,
    fused=True, **kwargs)``: ``forward(x) -> {"layer{i+1}": map for i in return_indices}``, contiguous NCHW maps, in order.

    An ordinary module, built up to the last returned stage and without ``avgpool`` / ``fc``, so its ``state_dict()`` has the keys
    of the reference's feature extractor.  ``weights``: a state dict (or ``{"model": state dict}``) or a LOCAL path, read with
    ``torch.load(..., weights_only=True)``; nothing here reaches a network, and without weights the initialisation stays.  ``fc.*``,
    ``num_batches_tracked`` and the stages behind the last returned one are dropped on every load, so a full torchvision or
    reference state dict loads strictly.  ``freeze_indices`` follows the reference's ``_freeze_stages``: any index freezes the stem,
    index ``i`` freezes ``layer{i+1}``.  ``kwargs`` go to ``ResNet`` (``replace_stride_with_dilation``, ``zero_init_residual``, ...).

    ``fused=True`` takes the kernels where ``takes_fused_route(x)`` holds; CPU tensors, another norm layer, fp16 or float64 take
    ``forward_torch``.  A channels-last input stays channels-last through the network."""

    def __init__(self, arch: str, weights=None, return_indices: Sequence[int] = (0, 1, 2, 3), freeze_indices: Sequence[int] = (),
                 norm_layer: Optional[Callable[..., nn.Module]] = FrozenBatchNorm2d, fused: bool = True, **kwargs):
        if arch not in ARCHITECTURES:
            raise ValueError(f"Expected architecture in {sorted(ARCHITECTURES)} but got {arch}")
        return_indices = tuple(int(i) for i in return_indices)
        if not return_indices or min(return_indices) < 0 or max(return_indices) > 3:
            raise ValueError(f"return_indices within 0..3, got {return_indices}")
        block, layers, groups, width = ARCHITECTURES[arch]
        kwargs.setdefault("groups", groups)
        kwargs.setdefault("width_per_group", width)
        stages = max(return_indices) + 1
        if any(i >= stages or i < 0 for i in freeze_indices):
            raise ValueError(f"freeze_indices {tuple(freeze_indices)} name a stage that is not built (stages: {stages})")
        super().__init__(block, layers, norm_layer=norm_layer, stages=stages, head=False, fused=fused, **kwargs)
        self.arch = arch
        self.return_indices = return_indices
        self.return_layers = [f"layer{i + 1}" for i in return_indices]
        self.num_channels = [64 * block.expansion * 2 ** i for i in return_indices]
        if weights is not None:
            if not isinstance(weights, dict):
                weights = torch.load(weights, map_location="cpu", weights_only=True)
            self.load_state_dict(weights["model"] if "model" in weights else weights)
        self.freeze_indices = tuple(int(i) for i in freeze_indices)
        if self.freeze_indices:
            _freeze(self.conv1)
            _freeze(self.bn1)
        for i in self.freeze_indices:
            _freeze(getattr(self, f"layer{i + 1}"))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        behind = tuple(f"{prefix}layer{i + 1}." for i in range(self.num_stages, 4)) + (prefix + "fc.",)
        for key in [k for k in state_dict if k.startswith(behind)]:
            del state_dict[key]
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def _named(self, outs: List[Tensor]) -> Dict[str, Tensor]:
        return {f"layer{i + 1}": outs[i].contiguous() for i in self.return_indices}

    def forward_torch(self, x: Tensor) -> Dict[str, Tensor]:
        return self._named(self.stages_torch(x))

    def forward_fused(self, x: Tensor) -> Dict[str, Tensor]:
        return self._named(self.stages_fused(x))

    def forward(self, x: Tensor) -> Dict[str, Tensor]:
        return self.forward_fused(x) if self.takes_fused_route(x) else self.forward_torch(x)


def _freeze(module: nn.Module) -> None:
    module.eval()
    for p in module.parameters():
        p.requires_grad = False
