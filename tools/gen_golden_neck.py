"""Generate tests/golden/g12_neck.npz by running the REFERENCE's own ChannelMapper and PositionEmbeddingSine (build machine only; no
test runs this).

Run:  RELATION_DETR_REFERENCE=<checkout of the reference> python tools/gen_golden_neck.py

Imported unmodified from the reference: ``models/necks/channel_mapper.py`` and ``models/bricks/position_encoding.py`` (with
``models/bricks/misc.py`` behind the first); all three need only torch.  The fixture holds data only.  Everything runs on the CPU in
float32.

Contents (B = 2, in_channels (16, 24, 40) -> 32 channels, GroupNorm(8), feature maps (12, 20), (6, 10), (3, 5)):
  sd.<key>        the randomised state dict of ChannelMapper(num_outs=4): conv weights, GroupNorm weights and biases
  x{i}            the three inputs;  y{i} the four outputs (the extra level is (2, 3));  go{i} the seeded output gradients
  gx{i}, gsd.<key>   autograd's gradients of sum_i <y_i, go_i> for every input and parameter
  sd5.<key>, y5_{i}  a 5-level mapper on the same inputs (an extra level behind the extra level -> (1, 2)), forward only
  img_mask        [2, 96, 160] float, valid regions (96, 160) and (70, 121);  img_mask_rand: random, not rectangular
  m{i}, mr{i}     F.interpolate(mask[None], size)[0].to(bool) at the four level sizes
  pos{i}, posr{i} PositionEmbeddingSine(16, 10000, True, offset=-0.5) of m{i} / mr{i};  posu{i}: normalize=False, offset=0 of m{i}
"""
import os
import sys
from functools import partial

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g12_neck.npz")
IN_CHANNELS, OUT_CHANNELS, GROUPS, B = (16, 24, 40), 32, 8, 2
SIZES = ((12, 20), (6, 10), (3, 5))
IMAGE = (96, 160)
VALID = ((96, 160), (70, 121))


def import_reference():
    ref = os.environ.get("RELATION_DETR_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "models")):
        sys.exit("set RELATION_DETR_REFERENCE to a checkout of the reference")
    sys.path.insert(0, ref)
    from models.bricks.position_encoding import PositionEmbeddingSine
    from models.necks.channel_mapper import ChannelMapper
    return ChannelMapper, PositionEmbeddingSine


def randomise(module: nn.Module, g: torch.Generator) -> None:
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / (p.shape[1] * p.shape[2] * p.shape[3]) ** 0.5))
            elif name.endswith("weight"):
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))


def main():
    ChannelMapper, PositionEmbeddingSine = import_reference()
    g = torch.Generator().manual_seed(12)
    out = {}
    xs = [torch.randn(B, c, h, w, generator=g).requires_grad_() for c, (h, w) in zip(IN_CHANNELS, SIZES)]
    feats = {str(i): x for i, x in enumerate(xs)}

    neck = ChannelMapper(list(IN_CHANNELS), OUT_CHANNELS, 4, norm_layer=partial(nn.GroupNorm, GROUPS))
    randomise(neck, g)
    ys = neck(feats)
    gos = [torch.randn(y.shape, generator=g) for y in ys]
    sum((y * go).sum() for y, go in zip(ys, gos)).backward()
    for k, v in neck.state_dict().items():
        out[f"sd.{k}"] = v.numpy()
    for k, p in neck.named_parameters():
        out[f"gsd.{k}"] = p.grad.numpy()
    for i, x in enumerate(xs):
        out[f"x{i}"], out[f"gx{i}"] = x.detach().numpy(), x.grad.numpy()
    for i, (y, go) in enumerate(zip(ys, gos)):
        out[f"y{i}"], out[f"go{i}"] = y.detach().numpy(), go.numpy()

    neck5 = ChannelMapper(list(IN_CHANNELS), OUT_CHANNELS, 5, norm_layer=partial(nn.GroupNorm, GROUPS))
    randomise(neck5, g)
    with torch.no_grad():
        for i, y in enumerate(neck5(feats)):
            out[f"y5_{i}"] = y.numpy()
    for k, v in neck5.state_dict().items():
        out[f"sd5.{k}"] = v.numpy()

    mask = torch.ones(B, *IMAGE)
    for b, (h, w) in enumerate(VALID):
        mask[b, :h, :w] = 0
    mask_rand = (torch.rand(B, *IMAGE, generator=g) < 0.35).float()
    mask_rand[1, :, 100:] = 1                                                   # whole columns without a valid pixel
    mask_rand[0, 40:56] = 1                                                     # whole rows without a valid pixel
    out["img_mask"], out["img_mask_rand"] = mask.numpy(), mask_rand.numpy()
    pe = PositionEmbeddingSine(16, 10000, True, offset=-0.5)
    pe_u = PositionEmbeddingSine(16, 10000, False, offset=0.0)
    for i, y in enumerate(ys):
        size = tuple(y.shape[-2:])
        m = F.interpolate(mask[None], size=size)[0].to(torch.bool)
        mr = F.interpolate(mask_rand[None], size=size)[0].to(torch.bool)
        out[f"m{i}"], out[f"mr{i}"] = m.numpy(), mr.numpy()
        out[f"pos{i}"], out[f"posr{i}"], out[f"posu{i}"] = pe(m).contiguous().numpy(), pe(mr).contiguous().numpy(), pe_u(m).contiguous().numpy()

    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
