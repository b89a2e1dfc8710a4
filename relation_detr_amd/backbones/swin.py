"""The Swin Transformer (v1) family as the reference's detector uses it (``models/backbones/swin.py``): its constructor arguments,
attribute names and state-dict keys, cut behind the last returned stage.  ``MLP`` and ``Permute`` restate ``models/bricks/misc.py``,
``StochasticDepth`` torchvision's definition (mode ``"row"``); torchvision itself is not needed.

Two routes, as in ``resnet.py``.  ``forward_torch`` is the reference's operator sequence on any device and dtype.  ``forward_fused``
keeps the library's qkv / proj / MLP GEMMs and LayerNorms and replaces everything between the qkv and the proj GEMM of an attention
-- pad, roll, window partition, the head permute, the ``[B*nW, heads, N, N]`` scores, bias, shift mask, softmax, ``P V``, window
reverse, roll back, unpad -- by ONE call of ``ops.relation_attention(..., window=..., pad=...)`` (csrc/attn_win.hip) on the qkv
GEMM's output of the UNPADDED map.  The route is chosen per attention (``ShiftedWindowAttention.takes_fused_route``); an attention
that does not qualify runs the torch route.

Deviation on the fused route: the reference pads the map before the qkv linear, so a padding token's q, k, v are the linear's bias
row exactly; here that row is passed to the kernel (``qkv.bias`` rounded to bf16, which is what the bf16 linear returns for a zero
input).  The kernel is forward only: an attention whose operands need a gradient takes the torch route.
"""
from __future__ import annotations

from functools import partial
from typing import Callable, Dict, List, Optional, Sequence

import torch
from torch import Tensor, nn
from torch.nn import functional as F

from .. import ops
from . import window as wgeo


# ---- restated bricks ------------------------------------------------------------------------------------------------------------
class Permute(nn.Module):
    def __init__(self, dims: List[int]):
        super().__init__()
        self.dims = dims

    def forward(self, x: Tensor) -> Tensor:
        return torch.permute(x, self.dims)


class MLP(nn.Sequential):
    """Linear (-> norm) -> activation -> Dropout per hidden width, then Linear -> Dropout."""

    def __init__(self, in_channels: int, hidden_channels: List[int], norm_layer: Optional[Callable[..., nn.Module]] = None,
                 activation_layer: Optional[Callable[..., nn.Module]] = nn.ReLU, inplace: Optional[bool] = True, bias: bool = True,
                 dropout: float = 0.0):
        params = {} if inplace is None else {"inplace": inplace}
        layers, in_dim = [], in_channels
        for hidden_dim in hidden_channels[:-1]:
            layers.append(nn.Linear(in_dim, hidden_dim, bias=bias))
            if norm_layer is not None:
                layers.append(norm_layer(hidden_dim))
            layers.append(activation_layer(**params))
            layers.append(nn.Dropout(dropout, **params))
            in_dim = hidden_dim
        layers.append(nn.Linear(in_dim, hidden_channels[-1], bias=bias))
        layers.append(nn.Dropout(dropout, **params))
        super().__init__(*layers)


class StochasticDepth(nn.Module):
    """Drops the residual branch of whole samples (``"row"``) or of the batch with probability ``p`` while training, and divides the
    survivors by ``1 - p``; the identity in eval mode or with ``p == 0``."""

    def __init__(self, p: float, mode: str):
        super().__init__()
        if p < 0.0 or p > 1.0:
            raise ValueError(f"drop probability has to be between 0 and 1, but got {p}")
        if mode not in ("batch", "row"):
            raise ValueError(f"mode has to be either 'batch' or 'row', but got {mode}")
        self.p, self.mode = p, mode

    def forward(self, x: Tensor) -> Tensor:
        if not self.training or self.p == 0.0:
            return x
        survival = 1.0 - self.p
        size = [x.shape[0]] + [1] * (x.ndim - 1) if self.mode == "row" else [1] * x.ndim
        noise = torch.empty(size, dtype=x.dtype, device=x.device).bernoulli_(survival)
        if survival > 0.0:
            noise.div_(survival)
        return x * noise

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(p={self.p}, mode={self.mode})"


def _patch_merging_pad(x: Tensor) -> Tensor:
    H, W, _ = x.shape[-3:]
    x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    return torch.cat([x[..., 0::2, 0::2, :], x[..., 1::2, 0::2, :], x[..., 0::2, 1::2, :], x[..., 1::2, 1::2, :]], -1)


class PatchMerging(nn.Module):
    """``[..., H, W, C] -> [..., ceil(H/2), ceil(W/2), 2C]``: the four phases of a 2 x 2 cell side by side, LayerNorm, Linear."""

    def __init__(self, dim: int, norm_layer: Callable[..., nn.Module] = nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x: Tensor) -> Tensor:
        return self.reduction(self.norm(_patch_merging_pad(x)))


# ---- attention ------------------------------------------------------------------------------------------------------------------
class ShiftedWindowAttention(nn.Module):
    """Window attention with relative position bias, shifted or not: the reference's module (``qkv``, ``proj``,
    ``relative_position_bias_table``, the persistent ``relative_position_index`` buffer) plus ``fused``."""

    def __init__(self, dim: int, window_size: List[int], shift_size: List[int], num_heads: int, qkv_bias: bool = True,
                 proj_bias: bool = True, attention_dropout: float = 0.0, dropout: float = 0.0, fused: bool = True):
        super().__init__()
        if len(window_size) != 2 or len(shift_size) != 2:
            raise ValueError("window_size and shift_size must be of length 2")
        self.window_size = list(window_size)
        self.shift_size = list(shift_size)
        self.num_heads = num_heads
        self.attention_dropout = attention_dropout
        self.dropout = dropout
        self.fused = bool(fused)
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim, bias=proj_bias)
        wh, ww = self.window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * wh - 1) * (2 * ww - 1), num_heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        self.register_buffer("relative_position_index", wgeo.bias_index(wh, ww).flatten())

    def get_relative_position_bias(self) -> Tensor:
        N = self.window_size[0] * self.window_size[1]
        bias = self.relative_position_bias_table[self.relative_position_index].view(N, N, -1)
        return bias.permute(2, 0, 1).contiguous().unsqueeze(0)

    # ---- routes -------------------------------------------------------------------------------------------------------------
    def fused_route_refusal(self, x: Tensor) -> Optional[str]:
        """Why the kernel does not take this attention, or None when it does.  It takes it when ``fused`` is on; head dim is 32 and a
        window has at most 144 tokens; dropout is inactive; the tensors are bf16 (a ``.to(bfloat16)`` model, or
        ``torch.autocast(bfloat16)`` on the device); no operand needs a gradient (the kernel is forward only); and the input is
        on a ROCm device."""
        if not self.fused:
            return "switched off"
        if self.qkv.in_features != self.num_heads * wgeo.HEAD_DIM:
            return "head dim"
        if not wgeo.fused_window_supported(self.qkv.in_features, self.num_heads, *self.window_size):
            return "window"
        if not isinstance(x, Tensor) or x.dim() != 4:
            return "input"
        if self.training and (self.attention_dropout > 0.0 or self.dropout > 0.0):
            return "dropout"
        if x.is_cuda and torch.is_autocast_enabled("cuda"):
            if torch.get_autocast_dtype("cuda") != torch.bfloat16 or x.dtype not in (torch.float32, torch.bfloat16):
                return "dtype"
        elif x.dtype != torch.bfloat16 or self.qkv.weight.dtype != torch.bfloat16:
            return "dtype"
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return "gradient"
        return None if x.is_cuda else "device"

    def takes_fused_route(self, x: Tensor) -> bool:
        return self.fused_route_refusal(x) is None

    def forward_torch(self, x: Tensor) -> Tensor:
        """The reference's ``shifted_window_attention`` (swin.py:133-221), operator by operator."""
        B, H, W, C = x.shape
        wh, ww = self.window_size
        num_heads = self.num_heads
        x = F.pad(x, (0, 0, 0, (ww - W % ww) % ww, 0, (wh - H % wh) % wh))
        _, pH, pW, _ = x.shape
        sh, sw = wgeo.effective_shift(H, W, wh, ww, *self.shift_size)
        if sh + sw > 0:
            x = torch.roll(x, shifts=(-sh, -sw), dims=(1, 2))
        num_windows = (pH // wh) * (pW // ww)
        x = x.view(B, pH // wh, wh, pW // ww, ww, C).permute(0, 1, 3, 2, 4, 5).reshape(B * num_windows, wh * ww, C)
        qkv = self.qkv(x)
        qkv = qkv.reshape(x.size(0), x.size(1), 3, num_heads, C // num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        q = q * (C // num_heads) ** -0.5
        attn = q.matmul(k.transpose(-2, -1))
        attn = attn + self.get_relative_position_bias()
        if sh + sw > 0:
            attn_mask = x.new_zeros((pH, pW))
            count = 0
            for hs in ((0, -wh), (-wh, -sh), (-sh, None)):
                for ws in ((0, -ww), (-ww, -sw), (-sw, None)):
                    attn_mask[hs[0]:hs[1], ws[0]:ws[1]] = count
                    count += 1
            attn_mask = attn_mask.view(pH // wh, wh, pW // ww, ww).permute(0, 2, 1, 3).reshape(num_windows, wh * ww)
            attn_mask = attn_mask.unsqueeze(1) - attn_mask.unsqueeze(2)
            attn_mask = attn_mask.masked_fill(attn_mask != 0, float(-100.0)).masked_fill(attn_mask == 0, float(0.0))
            attn = attn.view(x.size(0) // num_windows, num_windows, num_heads, x.size(1), x.size(1))
            attn = attn + attn_mask.unsqueeze(1).unsqueeze(0)
            attn = attn.view(-1, num_heads, x.size(1), x.size(1))
        attn = F.softmax(attn, dim=-1)
        attn = F.dropout(attn, p=self.attention_dropout, training=self.training)
        x = attn.matmul(v).transpose(1, 2).reshape(x.size(0), x.size(1), C)
        x = self.proj(x)
        x = F.dropout(x, p=self.dropout, training=self.training)
        x = x.view(B, pH // wh, pW // ww, wh, ww, C).permute(0, 1, 3, 2, 4, 5).reshape(B, pH, pW, C)
        if sh + sw > 0:
            x = torch.roll(x, shifts=(sh, sw), dims=(1, 2))
        return x[:, :H, :W, :].contiguous()

    def forward_fused(self, x: Tensor) -> Tensor:
        """qkv GEMM on the unpadded map -> one kernel -> proj GEMM.  The caller has asked ``takes_fused_route``."""
        B, H, W, C = x.shape
        wh, ww = self.window_size
        sh, sw = wgeo.effective_shift(H, W, wh, ww, *self.shift_size)
        qkv = self.qkv(x.reshape(B, H * W, C))
        if qkv.dtype != torch.bfloat16:
            raise RuntimeError("ShiftedWindowAttention.forward_fused needs bfloat16 (a bf16 model or bf16 autocast)")
        pad = None
        if self.qkv.bias is not None and wgeo.padded_size(H, W, wh, ww) != (H, W):
            row = self.qkv.bias.detach().to(torch.bfloat16)
            pad = (row[C:2 * C], row[2 * C:])
        y = ops.relation_attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], self.num_heads,
                                   bias=self.relative_position_bias_table.detach(), window=(H, W, wh, ww, sh, sw), pad=pad)
        y = F.dropout(self.proj(y), p=self.dropout, training=self.training)
        return y.reshape(B, H, W, C)

    def forward(self, x: Tensor) -> Tensor:
        return self.forward_fused(x) if self.takes_fused_route(x) else self.forward_torch(x)


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim: int, num_heads: int, window_size: List[int], shift_size: List[int], mlp_ratio: float = 4.0,
                 dropout: float = 0.0, attention_dropout: float = 0.0, stochastic_depth_prob: float = 0.0,
                 norm_layer: Callable[..., nn.Module] = nn.LayerNorm, attn_layer: Callable[..., nn.Module] = ShiftedWindowAttention,
                 fused: bool = True):
        super().__init__()
        self.norm1 = norm_layer(dim)
        extra = {"fused": fused} if attn_layer is ShiftedWindowAttention else {}
        self.attn = attn_layer(dim, window_size, shift_size, num_heads, attention_dropout=attention_dropout, dropout=dropout, **extra)
        self.stochastic_depth = StochasticDepth(stochastic_depth_prob, "row")
        self.norm2 = norm_layer(dim)
        self.mlp = MLP(dim, [int(dim * mlp_ratio), dim], activation_layer=nn.GELU, inplace=None, dropout=dropout)
        for m in self.mlp.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.normal_(m.bias, std=1e-6)

    def _tail(self, x: Tensor, a: Tensor) -> Tensor:
        x = x + self.stochastic_depth(a)
        return x + self.stochastic_depth(self.mlp(self.norm2(x)))

    def forward_torch(self, x: Tensor) -> Tensor:
        attn = self.attn.forward_torch if hasattr(self.attn, "forward_torch") else self.attn
        return self._tail(x, attn(self.norm1(x)))

    def forward_fused(self, x: Tensor) -> Tensor:
        """The attention decides for itself (``takes_fused_route``)."""
        return self._tail(x, self.attn(self.norm1(x)))

    def forward(self, x: Tensor) -> Tensor:
        return self.forward_fused(x)


class SwinTransformer(nn.Module):
    """The reference's constructor arguments and attribute names (``features.0`` = patch embedding, ``features.{2i+1}`` = stage
    ``i``, ``features.{2i+2}`` = the patch merging behind it), plus three keyword-only ones of this package: ``stages`` (how many
    stages are built; the patch merging behind the last built one is not), ``head`` (``norm``, ``avgpool``, ``head``) and ``fused``.
    ``forward`` is the classifier's when there is a head, else the list of stage outputs ``[B, H, W, C]``."""

    def __init__(self, patch_size: List[int], embed_dim: int, depths: List[int], num_heads: List[int], window_size: List[int],
                 mlp_ratio: float = 4.0, dropout: float = 0.0, attention_dropout: float = 0.0, stochastic_depth_prob: float = 0.1,
                 num_classes: int = 1000, norm_layer: Optional[Callable[..., nn.Module]] = None,
                 block: Optional[Callable[..., nn.Module]] = None, downsample_layer: Callable[..., nn.Module] = PatchMerging, *,
                 stages: Optional[int] = None, head: bool = True, fused: bool = True):
        super().__init__()
        self.num_classes = num_classes
        stages = len(depths) if stages is None else int(stages)
        if not 1 <= stages <= len(depths) or (head and stages != len(depths)):
            raise ValueError(f"SwinTransformer: 1 <= stages <= {len(depths)}, and a head needs all of them")
        self.num_stages, self.fused = stages, bool(fused)
        extra = {"fused": fused} if block is None else {}
        if block is None:
            block = SwinTransformerBlock
        if norm_layer is None:
            norm_layer = partial(nn.LayerNorm, eps=1e-5)
        layers: List[nn.Module] = [nn.Sequential(
            nn.Conv2d(3, embed_dim, kernel_size=(patch_size[0], patch_size[1]), stride=(patch_size[0], patch_size[1])),
            Permute([0, 2, 3, 1]), norm_layer(embed_dim))]
        total_stage_blocks = sum(depths)
        stage_block_id = 0
        for i_stage in range(stages):
            stage: List[nn.Module] = []
            dim = embed_dim * 2 ** i_stage
            for i_layer in range(depths[i_stage]):
                # the stochastic depth rate grows with the block's index over ALL stages of the architecture, built or not
                sd_prob = stochastic_depth_prob * float(stage_block_id) / max(total_stage_blocks - 1, 1)
                stage.append(block(dim, num_heads[i_stage], window_size=list(window_size),
                                   shift_size=[0 if i_layer % 2 == 0 else w // 2 for w in window_size], mlp_ratio=mlp_ratio,
                                   dropout=dropout, attention_dropout=attention_dropout, stochastic_depth_prob=sd_prob,
                                   norm_layer=norm_layer, **extra))
                stage_block_id += 1
            layers.append(nn.Sequential(*stage))
            if i_stage < stages - 1:
                layers.append(downsample_layer(dim, norm_layer))
        self.features = nn.Sequential(*layers)
        if head:
            num_features = embed_dim * 2 ** (len(depths) - 1)
            self.norm = norm_layer(num_features)
            self.permute = Permute([0, 3, 1, 2])
            self.avgpool = nn.AdaptiveAvgPool2d(1)
            self.flatten = nn.Flatten(1)
            self.head = nn.Linear(num_features, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def _stages(self, x: Tensor, fused: bool) -> List[Tensor]:
        outs = []
        for i, layer in enumerate(self.features):
            if i % 2 == 1:
                for blk in layer:
                    x = blk.forward_fused(x) if fused else blk.forward_torch(x)
                outs.append(x)
            else:
                x = layer(x)
        return outs

    def stages_torch(self, x: Tensor) -> List[Tensor]:
        """The reference's operator sequence, on any device."""
        return self._stages(x, False)

    def stages_fused(self, x: Tensor) -> List[Tensor]:
        """The same network with csrc/attn_win.hip inside every attention that qualifies."""
        return self._stages(x, True)

    def stages(self, x: Tensor) -> List[Tensor]:
        return self.stages_fused(x) if self.fused else self.stages_torch(x)

    def forward(self, x: Tensor):
        outs = self.stages(x)
        if not hasattr(self, "head"):
            return outs
        return self.head(self.flatten(self.avgpool(self.permute(self.norm(outs[-1])))))


# name -> the reference's table without the checkpoint URLs
ARCHITECTURES: Dict[str, dict] = {
    "swin_t": dict(patch_size=(4, 4), embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), window_size=(7, 7), stochastic_depth_prob=0.2),
    "swin_s": dict(patch_size=(4, 4), embed_dim=96, depths=(2, 2, 18, 2), num_heads=(3, 6, 12, 24), window_size=(7, 7), stochastic_depth_prob=0.3),
    "swin_b": dict(patch_size=(4, 4), embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=(7, 7), stochastic_depth_prob=0.5),
    "swin_l": dict(patch_size=(4, 4), embed_dim=192, depths=(2, 2, 18, 2), num_heads=(6, 12, 24, 48), window_size=(7, 7), stochastic_depth_prob=0.2),
    "swin_b_384": dict(patch_size=(4, 4), embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=(12, 12),
                       stochastic_depth_prob=0.2),
    "swin_l_384": dict(patch_size=(4, 4), embed_dim=192, depths=(2, 2, 18, 2), num_heads=(6, 12, 24, 48), window_size=(12, 12),
                       stochastic_depth_prob=0.2),
}
V2_ARCHITECTURES = ("swin_v2_t", "swin_v2_b")        # cosine attention and a continuous bias MLP: another operator


class SwinTransformerBackbone(SwinTransformer):
    """``SwinTransformerBackbone(arch, weights=None, return_indices=(0, 1, 2, 3), freeze_indices=(), fused=True, **kwargs)``:
    ``forward(x) -> {"features.{2i+1}": map for i in return_indices}``, contiguous NCHW maps, in order.

    An ordinary module, built up to the last returned stage and without ``norm`` / ``head``, so its ``state_dict()`` has the keys of
    the reference's feature extractor.  ``weights``: a state dict (or ``{"model": state dict}``) or a LOCAL path, read with
    ``torch.load(..., weights_only=True)``; nothing here reaches a network, and without weights the reference constructors'
    initialisation stays.  ``norm.*``, ``head.*`` and what lies behind the last returned stage are dropped on every load, so a full
    checkpoint loads strictly; the ``0.`` in front of a reference detector checkpoint's backbone keys is stripped.  ``freeze_indices`` follows the reference's ``_freeze_stages``: any index freezes the patch
    embedding, index ``i`` freezes stage ``i`` and the patch merging behind it.  ``kwargs`` replace entries of the architecture
    (``stochastic_depth_prob``, ``window_size``, ...).  The v2 architectures are not part of this package."""

    def __init__(self, arch: str, weights=None, return_indices: Sequence[int] = (0, 1, 2, 3), freeze_indices: Sequence[int] = (),
                 fused: bool = True, **kwargs):
        if arch in V2_ARCHITECTURES:
            raise NotImplementedError(f"{arch}: Swin Transformer V2 (cosine attention, continuous position bias) is not part of this package")
        if arch not in ARCHITECTURES:
            raise ValueError(f"Expected architecture in {sorted(ARCHITECTURES)} but got {arch}")
        config = dict(ARCHITECTURES[arch])
        config.update({k: v for k, v in kwargs.items() if v is not None})
        return_indices = tuple(int(i) for i in return_indices)
        if not return_indices or min(return_indices) < 0 or max(return_indices) >= len(config["depths"]):
            raise ValueError(f"return_indices within 0..{len(config['depths']) - 1}, got {return_indices}")
        stages = max(return_indices) + 1
        if any(i >= stages or i < 0 for i in freeze_indices):
            raise ValueError(f"freeze_indices {tuple(freeze_indices)} name a stage that is not built (stages: {stages})")
        super().__init__(**config, stages=stages, head=False, fused=fused)
        self.arch = arch
        self.return_indices = return_indices
        self.return_layers = [f"features.{2 * i + 1}" for i in return_indices]
        self.num_channels = [config["embed_dim"] * 2 ** i for i in return_indices]
        if weights is not None:
            if not isinstance(weights, dict):
                weights = torch.load(weights, map_location="cpu", weights_only=True)
            self.load_state_dict(weights["model"] if "model" in weights else weights)
        self.freeze_indices = tuple(int(i) for i in freeze_indices)
        self._freeze_stages(self.freeze_indices)

    def _freeze_stages(self, freeze_indices: Sequence[int]) -> None:
        if len(freeze_indices) > 0:
            _freeze(self.features[0])
        for idx in freeze_indices:
            _freeze(self.features[2 * idx + 1])
            if 2 * idx + 2 < len(self.features):
                _freeze(self.features[2 * idx + 2])

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        # the reference's backbone is nn.Sequential(extractor, PostProcess()): a detector checkpoint holds these keys under "0."
        for key in [k for k in state_dict if k.startswith(prefix + "0.")]:
            state_dict[prefix + key[len(prefix) + 2:]] = state_dict.pop(key)
        built = tuple(f"{prefix}features.{i}." for i in range(len(self.features)))
        for key in [k for k in state_dict if k.startswith(prefix)]:
            rest = key[len(prefix):]
            if rest.startswith(("norm.", "head.")) or (rest.startswith("features.") and not key.startswith(built)):
                del state_dict[key]
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def _named(self, outs: List[Tensor]) -> Dict[str, Tensor]:
        return {f"features.{2 * i + 1}": outs[i].permute(0, 3, 1, 2).contiguous() for i in self.return_indices}

    def forward_torch(self, x: Tensor) -> Dict[str, Tensor]:
        return self._named(self.stages_torch(x))

    def forward_fused(self, x: Tensor) -> Dict[str, Tensor]:
        return self._named(self.stages_fused(x))

    def forward(self, x: Tensor) -> Dict[str, Tensor]:
        return self.forward_fused(x) if self.fused else self.forward_torch(x)


def _freeze(module: nn.Module) -> None:
    module.eval()
    for p in module.parameters():
        p.requires_grad = False
