"""The DETR training augmentation on device images (``transforms/presets.py``: ``detr`` and ``multiscale``):
``RandomHorizontalFlip`` -> either ``RandomShortestSize(scales, max_size)`` or ``RandomShortestSize(crop_resize)`` -> ``RandomSizeCrop`` ->
``RandomShortestSize(scales, max_size)`` -> ``ConvertImageDtype`` -> ``Normalize`` -> ``SanitizeBoundingBox``, then the detector's own
batching, mask and ``prepare_targets``: decoded uint8 images and xyxy boxes in, ``ImageBatch`` and prepared targets out.

What is random is drawn on the host into ``DetrChoice`` records (``sample_detr_choices``); ``detr_plan`` turns a record into the sizes
and the window, ``transform_targets`` moves the boxes as the reference's box kernels do, in fp32 torch, and the pixels go through
``images.batch_images(..., plans=...)`` (two launches per ``MAX_IMAGES`` images at most) or, on the torch route, through the
reference's operator sequence.  This module launches nothing itself.

Two things that are easy to restate wrongly:
  * ``RandomShortestSize`` computes its size in Python doubles with ``int()`` truncation (``shortest_size``), not in the float32 of
    ``EvalResize`` (``images.resized_size``);
  * the boxes are multiplied by a float32 tensor of ratios that were divided in doubles, and a crop subtracts first and clamps after.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import images

DETR_SCALES = (480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800)
Plan = Tuple[bool, Optional[Tuple[int, int]], Optional[Tuple[int, int, int, int]]]


def shortest_size(h: int, w: int, min_size: int, max_size: Optional[int] = None) -> Tuple[int, int]:
    """``RandomShortestSize._get_params`` once ``min_size`` is chosen: doubles, truncated."""
    r = min_size / min(h, w)
    if max_size is not None:
        r = min(r, max_size / max(h, w))
    return int(h * r), int(w * r)


class DetrChoice(NamedTuple):
    """What the reference draws for one image.  ``crop`` is the branch; the last three fields belong to it."""
    flip: bool
    crop: bool
    min_size: int                                        # the scale of the (last) RandomShortestSize
    first_min_size: Optional[int] = None                 # the scale of the resize in front of the crop
    crop_size: Optional[Tuple[int, int]] = None          # (h, w)
    crop_corner: Optional[Tuple[int, int]] = None        # (top, left)


def detr_plan(h: int, w: int, choice: DetrChoice, max_size: Optional[int] = 1333,
              crop_range: Tuple[int, int] = (384, 600)) -> Tuple[Plan, Tuple[int, int]]:
    """-> ``((flip, first, crop), (oh, ow))``: the plan ``images.batch_images`` takes and the final size.  The crop must lie in the
    ranges ``RandomSizeCrop._get_params`` draws from: its height in ``[min, min(rh1, max)]``, its top in ``[0, rh1 - ch]``, likewise
    across."""
    if not choice.crop:
        return (bool(choice.flip), None, None), shortest_size(h, w, choice.min_size, max_size)
    rh1, rw1 = shortest_size(h, w, choice.first_min_size)
    (ch, cw), (top, left) = choice.crop_size, choice.crop_corner
    lo, hi = crop_range
    if not (lo <= ch <= min(rh1, hi) and lo <= cw <= min(rw1, hi)):
        raise ValueError(f"detr_plan: a crop of {(ch, cw)} from {(rh1, rw1)} is outside [{lo}, min(size, {hi})]")
    if not (0 <= top <= rh1 - ch and 0 <= left <= rw1 - cw):
        raise ValueError(f"detr_plan: a crop of {(ch, cw)} at {(top, left)} leaves {(rh1, rw1)}")
    return (bool(choice.flip), (rh1, rw1), (int(top), int(left), int(ch), int(cw))), shortest_size(ch, cw, choice.min_size, max_size)


def sample_detr_choices(sizes: Sequence[Tuple[int, int]], generator: Optional[torch.Generator] = None,
                        scales: Sequence[int] = DETR_SCALES, crop_resize: Optional[Sequence[int]] = (400, 500, 600),
                        crop_range: Tuple[int, int] = (384, 600), p_flip: float = 0.5) -> List[DetrChoice]:
    """One ``DetrChoice`` per ``(h, w)`` with the reference's distributions, all from one host generator: flip iff ``u < p``, a uniform
    branch, uniform indices into the scale lists, inclusive integer ranges for the crop.  (The reference mixes ``random`` and
    ``torch``; its stream is not reproduced.)"""
    def integer(low, high):                              # inclusive
        return int(torch.randint(low, high + 1, (), generator=generator))

    out = []
    for h, w in sizes:
        flip = bool(torch.rand((), generator=generator) < p_flip)
        crop = crop_resize is not None and integer(0, 1) == 1
        if not crop:
            out.append(DetrChoice(flip, False, scales[integer(0, len(scales) - 1)]))
            continue
        first = crop_resize[integer(0, len(crop_resize) - 1)]
        rh1, rw1 = shortest_size(h, w, first)
        ch, cw = integer(crop_range[0], min(rh1, crop_range[1])), integer(crop_range[0], min(rw1, crop_range[1]))
        top, left = integer(0, rh1 - ch), integer(0, rw1 - cw)
        out.append(DetrChoice(flip, True, scales[integer(0, len(scales) - 1)], first, (ch, cw), (top, left)))
    return out


def transform_targets(targets: Sequence[Dict[str, Tensor]], sizes: Sequence[Tuple[int, int]], plans: Sequence[Optional[Plan]],
                      final_sizes: Sequence[Tuple[int, int]]) -> List[Dict[str, Tensor]]:
    """The boxes (xyxy pixels) through a plan as the reference's box kernels move them, then ``SanitizeBoundingBox(min_size=1)`` on boxes
    and labels alike.  ``sizes``: the images' (h, w) as they came in.  New dicts; the inputs are not written.  An image may end with
    no box."""
    def resize(boxes, old, new):
        w_ratio, h_ratio = new[1] / old[1], new[0] / old[0]                      # doubles; the tensor is float32
        return boxes.mul(torch.tensor([w_ratio, h_ratio, w_ratio, h_ratio], device=boxes.device))

    out = []
    for target, (h, w), plan, final in zip(targets, sizes, plans, final_sizes):
        boxes = target["boxes"].clone().reshape(-1, 4)
        flip, first, crop = (False, None, None) if plan is None else plan
        size = (int(h), int(w))
        if flip:
            boxes[:, [2, 0]] = boxes[:, [0, 2]].sub_(size[1]).neg_()
        if first is not None:
            boxes, size = resize(boxes, size, first), (int(first[0]), int(first[1]))
        if crop is not None:
            top, left, ch, cw = crop
            boxes = boxes - torch.tensor([left, top, left, top], dtype=boxes.dtype, device=boxes.device)
            boxes[..., 0::2].clamp_(min=0, max=cw)
            boxes[..., 1::2].clamp_(min=0, max=ch)
            size = (int(ch), int(cw))
        boxes, size = resize(boxes, size, final), (int(final[0]), int(final[1]))
        ws, hs = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
        valid = (ws >= 1) & (hs >= 1) & (boxes >= 0).all(dim=-1)
        valid &= (boxes[:, 0] <= size[1]) & (boxes[:, 2] <= size[1])
        valid &= (boxes[:, 1] <= size[0]) & (boxes[:, 3] <= size[0])
        moved = dict(target)
        moved["boxes"], moved["labels"] = boxes[valid], target["labels"][valid]
        out.append(moved)
    return out


class DetrAugment(nn.Module):
    """``forward(images, targets=None, choices=None) -> (ImageBatch, targets)``: ``ImagePreprocessor.forward``'s contract, so an instance
    is a ``preprocessor=`` of ``RelationDETRWithBackbone``.

    Training mode: ``images`` are [3, h, w] uint8 (or float32 in [0, 1]) as decoded, ``targets`` hold xyxy pixel boxes and labels;
    every image is augmented by its ``DetrChoice`` (``choices``, or drawn from ``generator``), normalised and batched, and the targets
    are moved, sanitised, checked and prepared.  Eval mode: an inner ``ImagePreprocessor(eval_min_size, eval_max_size)``.

    ``crop_resize=None`` is the ``multiscale`` preset (one resize, no crop branch); the 1.5 x lists of ``strong_album_1200_2000`` are
    ``scales``, ``max_size=2000``, ``crop_resize=(600, 750, 900)``, ``crop_range=(576, 900)``.  ``fused=True`` runs csrc/images.hip where
    ``takes_fused_route`` holds and the torch route elsewhere.  No parameters, no buffers, nothing kept between calls."""

    def __init__(self, scales: Sequence[int] = DETR_SCALES, max_size: Optional[int] = 1333,
                 crop_resize: Optional[Sequence[int]] = (400, 500, 600), crop_range: Tuple[int, int] = (384, 600), p_flip: float = 0.5,
                 eval_min_size: Optional[int] = 800, eval_max_size: Optional[int] = 1333, size_divisible: int = 32,
                 mean: Sequence[float] = images.IMAGENET_MEAN, std: Sequence[float] = images.IMAGENET_STD,
                 dtype: torch.dtype = torch.float32, channels_last: bool = False, fused: bool = True,
                 generator: Optional[torch.Generator] = None):
        super().__init__()
        self.scales, self.max_size = tuple(int(s) for s in scales), max_size
        self.crop_resize = None if crop_resize is None else tuple(int(s) for s in crop_resize)
        self.crop_range, self.p_flip = (int(crop_range[0]), int(crop_range[1])), float(p_flip)
        self.size_divisible = int(size_divisible)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.dtype, self.channels_last, self.fused, self.generator = dtype, bool(channels_last), bool(fused), generator
        # eval mode as a whole, and the torch route's tail (/ 255, normalise, pad, mask): both stay in eval mode
        self.eval_preprocessor = images.ImagePreprocessor(eval_min_size, eval_max_size, size_divisible, mean, std, dtype, channels_last, fused)
        self.batcher = images.ImagePreprocessor(None, None, size_divisible, mean, std, dtype, channels_last, fused=False)
        self.eval_preprocessor.eval()
        self.batcher.eval()

    def train(self, mode: bool = True):
        super().train(mode)
        self.eval_preprocessor.eval()
        self.batcher.eval()
        return self

    def sample(self, image_list: Sequence[Tensor]) -> List[DetrChoice]:
        return sample_detr_choices([(int(im.shape[-2]), int(im.shape[-1])) for im in image_list], self.generator, self.scales,
                                   self.crop_resize, self.crop_range, self.p_flip)

    def plans(self, image_list: Sequence[Tensor], choices: Sequence[DetrChoice]):
        """-> (plans, final sizes), one each per image."""
        if len(choices) != len(image_list):
            raise ValueError("DetrAugment: one choice per image")
        both = [detr_plan(int(im.shape[-2]), int(im.shape[-1]), c, self.max_size, self.crop_range) for im, c in zip(image_list, choices)]
        return [p for p, _ in both], [s for _, s in both]

    def takes_fused_route(self, image_list, choices: Sequence[DetrChoice]) -> bool:
        image_list = list(image_list.unbind(0)) if isinstance(image_list, Tensor) else list(image_list)
        plans, finals = self.plans(image_list, choices)
        return self.fused and images._kernel_takes(image_list, finals, self.size_divisible, True, plans) is None

    def _targets(self, batch, targets, plans, finals):
        if targets:
            targets = transform_targets(targets, batch.original_sizes.tolist(), plans, finals)
            images.check_boxes(targets)
            targets = images.prepare_targets(batch.image_sizes, targets)
        return targets

    @torch.no_grad()
    def forward_torch(self, image_list, targets=None, choices: Optional[Sequence[DetrChoice]] = None):
        """The reference's operator sequence, on any device."""
        if not self.training:
            return self.eval_preprocessor.forward_torch(image_list, targets)
        image_list = list(image_list.unbind(0)) if isinstance(image_list, Tensor) else list(image_list)
        plans, finals = self.plans(image_list, self.sample(image_list) if choices is None else choices)
        done = []
        for im, (flip, first, crop), final in zip(image_list, plans, finals):
            if flip:
                im = im.flip(-1)
            if first is not None:
                im = images.resize_image(im, first)
            if crop is not None:
                im = im[..., crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]]
            done.append(images.resize_image(im, final))
        batch = self.batcher.batch_torch(done)
        batch = batch._replace(original_sizes=torch.tensor([tuple(im.shape[-2:]) for im in image_list], dtype=torch.int64).reshape(-1, 2))
        return batch, self._targets(batch, targets, plans, finals)

    @torch.no_grad()
    def forward_fused(self, image_list, targets=None, choices: Optional[Sequence[DetrChoice]] = None):
        """The kernel route; raises where the kernel does not take the batch."""
        if not self.training:
            return self.eval_preprocessor.forward_fused(image_list, targets)
        image_list = list(image_list.unbind(0)) if isinstance(image_list, Tensor) else list(image_list)
        plans, finals = self.plans(image_list, self.sample(image_list) if choices is None else choices)
        batch = images.batch_images(image_list, finals, self.size_divisible, self.mean, self.std, normalize=True, dtype=self.dtype,
                                    channels_last=self.channels_last, plans=plans)
        return batch, self._targets(batch, targets, plans, finals)

    def forward(self, image_list, targets=None, choices: Optional[Sequence[DetrChoice]] = None):
        if not self.training:
            return self.eval_preprocessor(image_list, targets)
        image_list = list(image_list.unbind(0)) if isinstance(image_list, Tensor) else list(image_list)
        choices = self.sample(image_list) if choices is None else choices
        route = self.forward_fused if self.takes_fused_route(image_list, choices) else self.forward_torch
        return route(image_list, targets, choices)
