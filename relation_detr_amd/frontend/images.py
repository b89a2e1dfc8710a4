"""The image front end: a list of images -> the padded, normalised batch, its padding mask and the prepared targets
(``models/detectors/base_detector.py``: ``EvalResize`` -> ``ConvertImageDtype`` -> ``Normalize`` -> ``image_list_from_tensors`` ->
``construct_mask`` -> ``prepare_targets``).

``batch_images`` is the fused call: csrc/images.hip resizes, rounds, normalises, pads and writes the mask in one launch per
``MAX_IMAGES`` images; with ``plans`` it also flips, crops and resizes twice, the training augmentation's geometry (frontend/augment.py).  ``ImagePreprocessor`` is the module with the two routes the neck's modules have: ``forward_torch`` restates the
reference's operator sequence on any device, ``forward_fused`` is the kernel.

Two things that are easy to restate wrongly:
  * the size rule is float32 arithmetic on 0-dim tensors (``resized_size``); Python floats give another size for about one size in
    seven, and a size one pixel off changes every tap weight;
  * a uint8 image is resized as ``round(interpolate(float32 copy))`` and only then divided by 255, so values on x.5 round either way
    depending on the last bit of the fp32 filter sum (tests/test_images_host.py states the near-tie rule the parity tests use).

One deviation on both routes: the mask is bool where the reference's is a float tensor of ones and zeros; ``RelationDETR.forward``
takes either.
"""
from __future__ import annotations

import copy
import ctypes
import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor, nn
from torch.nn import functional as F

from .. import _lib

MAX_IMAGES = 16                  # RDETR_IMAGE_MAX_IMAGES: descriptors of one launch
MAX_DOWNSCALE = 8                # RDETR_IMAGE_MAX_DOWNSCALE: n_in <= 8 * n_out per axis
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
_OUT_DTYPES = (torch.float32, torch.bfloat16)


class ImageBatch(NamedTuple):
    tensors: Tensor              # [B, 3, Hp, Wp]
    mask: Tensor                 # [B, Hp, Wp] bool, True = padded
    image_sizes: Tensor          # [B, 2] int64 on the host: the resized (h, w), the reference's ImageList.image_sizes
    original_sizes: Tensor       # [B, 2] int64 on the host: (h, w) as the images came in


class _ImageDesc(ctypes.Structure):                    # rdetr_image_desc
    _fields_ = [("src", ctypes.c_void_p), ("row_stride", ctypes.c_longlong), ("channel_stride", ctypes.c_longlong),
                ("h", ctypes.c_int), ("w", ctypes.c_int), ("oh", ctypes.c_int), ("ow", ctypes.c_int)]


class _WindowDesc(ctypes.Structure):                   # rdetr_image_window_desc
    _fields_ = [("src", ctypes.c_void_p), ("row_stride", ctypes.c_longlong), ("channel_stride", ctypes.c_longlong),
                ("h", ctypes.c_int), ("w", ctypes.c_int), ("flip", ctypes.c_int), ("rh", ctypes.c_int), ("rw", ctypes.c_int),
                ("top", ctypes.c_int), ("left", ctypes.c_int), ("oh", ctypes.c_int), ("ow", ctypes.c_int),
                ("dst", ctypes.c_void_p), ("dst_row_stride", ctypes.c_longlong), ("dst_channel_stride", ctypes.c_longlong)]

    @staticmethod
    def stages(h: int, w: int, size: Tuple[int, int], plan):
        """One image's plan ``(flip, first, crop)`` -> ``(scratch, batch)``, the launches that run it.  Each is a tuple ``(vt, vl, sh, sw,
        flip, rh, rw, top, left, oh, ow)``: the launch reads the ``sh x sw`` view at ``(vt, vl)`` of its source (in the flipped image's
        coordinates), flips it, resizes it to ``(rh, rw)`` and produces the ``oh x ow`` window at ``(top, left)``.  ``scratch`` is None,
        or the U8 launch whose window becomes the source of ``batch``.  A crop with no first resize is a view of the source; a crop
        whose second resize is the identity is a window of one launch."""
        oh, ow = int(size[0]), int(size[1])
        if plan is None:
            return None, (0, 0, h, w, 0, oh, ow, 0, 0, oh, ow)
        flip, first, crop = plan
        flip = int(bool(flip))
        if first is None:
            top, left, ch, cw = (0, 0, h, w) if crop is None else (int(v) for v in crop)
            return None, (top, left, ch, cw, flip, oh, ow, 0, 0, oh, ow)
        rh1, rw1 = int(first[0]), int(first[1])
        top, left, ch, cw = (0, 0, rh1, rw1) if crop is None else (int(v) for v in crop)
        if (ch, cw) == (oh, ow):
            return None, (0, 0, h, w, flip, rh1, rw1, top, left, oh, ow)
        return (0, 0, h, w, flip, rh1, rw1, top, left, ch, cw), (0, 0, ch, cw, 0, oh, ow, 0, 0, oh, ow)


def resized_size(h: int, w: int, min_size: int, max_size: Optional[int] = None) -> Tuple[int, int]:
    """``EvalResize.forward``'s output size.  The reference computes it on 0-dim tensors, so in float32, and ``number / tensor`` is
    torch's ``tensor.reciprocal() * number``: ``r = (1 / min(h, w)) * min_size``, each step rounded to float32, likewise
    ``(1 / max(h, w)) * max_size``; ``(orig * r).to(int64)`` multiplies in float32 and truncates."""
    h32, w32, one = np.float32(h), np.float32(w), np.float32(1)
    r = one / min(h32, w32) * np.float32(min_size)
    if max_size is not None:
        r = min(r, one / max(h32, w32) * np.float32(max_size))
    return int(h32 * r), int(w32 * r)


def _resize_bounds(min_size, max_size) -> Optional[Tuple[int, int]]:
    """``BaseDetector.__init__``: whichever of the two is a number; one number alone is both bounds."""
    size = [s for s in (min_size, max_size) if isinstance(s, (int, float))]
    return (min(size), max(size)) if size else None


def batched_size(sizes: Sequence[Tuple[int, int]], size_divisible: int) -> Tuple[int, int]:
    hp, wp = max(s[0] for s in sizes), max(s[1] for s in sizes)
    return (int(math.ceil(float(hp) / size_divisible) * size_divisible), int(math.ceil(float(wp) / size_divisible) * size_divisible))


def _kernel_takes(images: Sequence[Tensor], sizes: Sequence[Tuple[int, int]], size_divisible: int, normalize: bool,
                  plans: Optional[Sequence] = None) -> Optional[str]:
    """None when csrc/images.hip takes the batch, else the reason it does not.  With ``plans`` both launches' downscales and the
    windows are checked."""
    if len(images) == 0:
        return "an empty list"
    first = images[0]
    for im in images:
        if not isinstance(im, Tensor) or not im.is_cuda:
            return "a tensor that is not on a ROCm device"
        if im.device != first.device or im.dtype != first.dtype:
            return "images of several devices or dtypes"
        if im.dim() != 3 or im.shape[0] != 3 or im.shape[1] == 0 or im.shape[2] == 0:
            return "an image that is not [3, h, w]"
        if im.stride(2) != 1 and im.shape[2] > 1:
            return "rows that are not contiguous"
        if im.stride(0) < 0 or im.stride(1) < 0:
            return "a negative stride"
    if first.dtype not in (torch.uint8, torch.float32):
        return f"dtype {first.dtype}"
    if first.dtype == torch.uint8 and not normalize:
        return "uint8 images without normalisation"
    if plans is not None and len(plans) != len(images):
        return "a list of plans that is not one per image"
    for k, (im, (oh, ow)) in enumerate(zip(images, sizes)):
        if oh <= 0 or ow <= 0:
            return "an empty resized image"
        H, W = int(im.shape[1]), int(im.shape[2])
        scratch, batch = _WindowDesc.stages(H, W, (oh, ow), None if plans is None else plans[k])
        if scratch is not None and first.dtype != torch.uint8:
            return "a resize, crop, resize plan on float images"
        for stage in (scratch, batch):
            if stage is None:
                continue
            vt, vl, sh, sw, _, rh, rw, top, left, wh, ww = stage
            if sh <= 0 or sw <= 0 or vt < 0 or vl < 0 or vt + sh > H or vl + sw > W:
                return "a crop outside the image"
            if rh <= 0 or rw <= 0 or wh <= 0 or ww <= 0 or top < 0 or left < 0 or top + wh > rh or left + ww > rw:
                return "a crop outside the resized image"
            if sh > MAX_DOWNSCALE * rh or sw > MAX_DOWNSCALE * rw:
                return f"a downscale beyond {MAX_DOWNSCALE}"
            H, W = wh, ww                                       # the scratch is the next launch's source
    if batched_size(sizes, size_divisible)[1] % 8:
        return "a batch width that is no multiple of 8"
    return None


def batch_images(images: Sequence[Tensor], sizes: Optional[Sequence[Tuple[int, int]]] = None, size_divisible: int = 32,
                 mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD, normalize: bool = True,
                 dtype: torch.dtype = torch.float32, channels_last: bool = False, *, plans: Optional[Sequence] = None) -> ImageBatch:
    """The fused front end on device tensors.  ``images``: [3, h_i, w_i] uint8 or float32 (values in [0, 1]), rows contiguous (a
    crop of a larger tensor is fine).  ``sizes``: the (oh_i, ow_i) to resize to, None for no resize.  uint8 images are resized,
    rounded, divided by 255 and normalised; float32 images are resized and normalised, or with ``normalize=False`` only copied.
    The batch is ``dtype`` (float32 or bfloat16), NCHW-contiguous or channels-last.  Raises where the kernel does not take the batch;
    ``ImagePreprocessor`` is what falls back to the torch route.

    ``plans``: per image None or ``(flip, first, crop)``, the geometry of the training augmentation: flip horizontally, resize to
    ``first = (rh1, rw1)`` (uint8 images: rounded to uint8), crop ``(top, left, ch, cw)``, resize to ``sizes[i]``; ``first`` and ``crop``
    may each be None.  Images that resize twice go through one launch per ``MAX_IMAGES`` of them that writes the crop of the first
    resize as uint8 into scratch memory allocated here; then one launch per ``MAX_IMAGES`` images writes the batch.  ``plans=None``
    is the call as it always was."""
    images = list(images.unbind(0)) if isinstance(images, Tensor) else list(images)
    original = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
    sizes = original if sizes is None else [(int(s[0]), int(s[1])) for s in sizes]
    if len(sizes) != len(images):
        raise ValueError("batch_images: one size per image")
    if dtype not in _OUT_DTYPES:
        raise ValueError(f"batch_images: dtype {dtype}; the batch is float32 or bfloat16")
    reason = _kernel_takes(images, sizes, size_divisible, normalize, plans)
    if reason is not None:
        raise _lib.RdetrError(f"batch_images: the kernel does not take {reason}; ImagePreprocessor(fused=False) is the torch route")
    lib = _lib.load()
    B, device = len(images), images[0].device
    Hp, Wp = batched_size(sizes, size_divisible)
    out = torch.empty((B, 3, Hp, Wp), dtype=dtype, device=device,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    mask = torch.empty((B, Hp, Wp), dtype=torch.bool, device=device)
    c_mean, c_std = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    stream = torch.cuda.current_stream(device).cuda_stream
    if plans is not None:
        u8 = int(images[0].dtype == torch.uint8)
        descs, twice, scratch_bytes = [], [], 0
        for im, size, plan in zip(images, sizes, plans):
            scratch, batch = _WindowDesc.stages(int(im.shape[1]), int(im.shape[2]), size, plan)
            vt, vl, _, sw, flip = (scratch or batch)[:5]
            col = int(im.shape[2]) - vl - sw if flip else vl                  # the view's first column in the source as it lies
            src = im.data_ptr() + (vt * im.stride(1) + col) * im.element_size()
            if scratch is None:
                descs.append(_WindowDesc(src, im.stride(1), im.stride(0), *batch[2:], None, 0, 0))
                continue
            ch, cw = scratch[9:]
            ld = (cw + 15) // 16 * 16                                          # rows of whole 16-byte pieces
            twice.append((_WindowDesc(src, im.stride(1), im.stride(0), *scratch[2:], None, ld, ch * ld), len(descs), scratch_bytes))
            descs.append(_WindowDesc(None, ld, ch * ld, *batch[2:], None, 0, 0))
            scratch_bytes += 3 * ch * ld
        if twice:
            memory = torch.empty(scratch_bytes, dtype=torch.uint8, device=device)
            for d, k, at in twice:
                d.dst = descs[k].src = memory.data_ptr() + at
            for first in range(0, len(twice), MAX_IMAGES):
                n = min(MAX_IMAGES, len(twice) - first)
                table = (_WindowDesc * n)(*[d for d, _, _ in twice[first:first + n]])
                _lib.check(lib.rdetr_augment_image_batch(table, n, 1, 1, 0, 0, None, None, 0, 0, 0, None, None, stream),
                           "rdetr_augment_image_batch")
        for first in range(0, B, MAX_IMAGES):
            n = min(MAX_IMAGES, B - first)
            table = (_WindowDesc * n)(*descs[first:first + n])
            _lib.check(lib.rdetr_augment_image_batch(table, n, u8, 0, Hp, Wp, c_mean, c_std, int(normalize), int(dtype == torch.bfloat16),
                                                     int(channels_last), out[first:first + n].data_ptr(), mask[first:first + n].data_ptr(),
                                                     stream), "rdetr_augment_image_batch")
        return ImageBatch(out, mask, torch.tensor(sizes, dtype=torch.int64).reshape(B, 2),
                          torch.tensor(original, dtype=torch.int64).reshape(B, 2))
    for first in range(0, B, MAX_IMAGES):
        n = min(MAX_IMAGES, B - first)
        table = (_ImageDesc * n)()
        for k in range(n):
            im, (oh, ow) = images[first + k], sizes[first + k]
            table[k] = _ImageDesc(im.data_ptr(), im.stride(1), im.stride(0), im.shape[1], im.shape[2], oh, ow)
        _lib.check(lib.rdetr_image_batch(table, n, int(images[0].dtype == torch.uint8), Hp, Wp, c_mean, c_std, int(normalize),
                                         int(dtype == torch.bfloat16), int(channels_last), out[first:first + n].data_ptr(),
                                         mask[first:first + n].data_ptr(), stream), "rdetr_image_batch")
    return ImageBatch(out, mask, torch.tensor(sizes, dtype=torch.int64).reshape(B, 2), torch.tensor(original, dtype=torch.int64).reshape(B, 2))


def resize_image(image: Tensor, size: Tuple[int, int]) -> Tensor:
    """``transforms/_functional_tensor.py::resize`` with bilinear + antialias: ``interpolate`` on a float32 copy, and for an integer
    image ``round`` and the cast back."""
    x = image if image.dtype in (torch.float32, torch.float64) else image.to(torch.float32)
    x = F.interpolate(x[None], size=[int(size[0]), int(size[1])], mode="bilinear", align_corners=False, antialias=True)[0]
    return x if x.dtype == image.dtype else torch.round(x).to(image.dtype)


def check_boxes(targets: Sequence[Dict[str, Tensor]]) -> None:
    for index, target in enumerate(targets):
        boxes = target["boxes"]
        degenerate = boxes[:, 2:] <= boxes[:, :2]
        if degenerate.any():
            bad = boxes[torch.where(degenerate.any(dim=1))[0][0]].tolist()
            raise ValueError(f"All bounding boxes should have positive height and width. Found invalid box {bad} for target at index {index}.")


def prepare_targets(image_sizes: Tensor, targets: Sequence[Dict[str, Tensor]]) -> List[Dict[str, Tensor]]:
    """``DETRDetector.prepare_targets``: a deep copy with the boxes from xyxy pixels to cxcywh divided by the image's (w, h, w, h)."""
    targets = copy.deepcopy(list(targets))
    for (h, w), target in zip(image_sizes.tolist(), targets):
        x1, y1, x2, y2 = target["boxes"].unbind(-1)
        boxes = torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), dim=-1)
        target["boxes"] = boxes / boxes.new_tensor([w, h, w, h])
    return targets


class ImagePreprocessor(nn.Module):
    """``forward(images, targets=None) -> (ImageBatch, targets)``, ``DETRDetector.preprocess``.

    Eval mode: every image is resized to ``resized_size(h, w, min, max)`` when ``min_size`` / ``max_size`` are given, converted to
    float (uint8: / 255) and normalised.  Training mode: the images arrive augmented, float and normalised and are only batched
    (``augment.DetrAugment`` is the preprocessor that takes decoded images and augments them itself).
    Both modes pad to the batch's largest size rounded up to ``size_divisible`` and build the mask.  Targets, when given, are
    checked and their boxes go from xyxy pixels to cxcywh normalised by ``image_sizes``; they stay torch (a few boxes).

    ``fused=True`` runs csrc/images.hip where ``takes_fused_route`` holds and the torch route elsewhere; ``dtype`` and
    ``channels_last`` describe the batch on both routes.  No parameters, no buffers: the state dict is empty."""

    def __init__(self, min_size: Optional[int] = None, max_size: Optional[int] = None, size_divisible: int = 32,
                 mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD, dtype: torch.dtype = torch.float32,
                 channels_last: bool = False, fused: bool = True):
        super().__init__()
        if dtype not in _OUT_DTYPES:
            raise ValueError(f"ImagePreprocessor: dtype {dtype}; the batch is float32 or bfloat16")
        self.resize = _resize_bounds(min_size, max_size)
        self.size_divisible = int(size_divisible)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.dtype, self.channels_last, self.fused = dtype, bool(channels_last), bool(fused)

    def target_sizes(self, images: Sequence[Tensor]) -> List[Tuple[int, int]]:
        original = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
        if self.training or self.resize is None:
            return original
        return [resized_size(h, w, *self.resize) for h, w in original]

    def takes_fused_route(self, images) -> bool:
        images = list(images.unbind(0)) if isinstance(images, Tensor) else list(images)
        return self.fused and _kernel_takes(images, self.target_sizes(images), self.size_divisible, not self.training) is None

    def batch_torch(self, images: Sequence[Tensor]) -> ImageBatch:
        """The reference's operator sequence: resize -> / 255 -> sub mean, div std -> zero batch, copy -> mask."""
        images = list(images.unbind(0)) if isinstance(images, Tensor) else list(images)
        original = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
        if not self.training:
            done = []
            for im, size in zip(images, self.target_sizes(images)):
                if self.resize is not None:
                    im = resize_image(im, size)
                # a tensor divisor: torch's device kernels turn ``x / 255`` into ``x * (1 / 255)``, which is not the CPU's division
                im = im.to(torch.float32) / im.new_full((1, 1, 1), 255, dtype=torch.float32) if im.dtype == torch.uint8 else im.to(torch.float32)
                mean, std = im.new_tensor(self.mean).view(-1, 1, 1), im.new_tensor(self.std).view(-1, 1, 1)
                done.append(im.clone().sub_(mean).div_(std))
            images = done
        sizes = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
        Hp, Wp = batched_size(sizes, self.size_divisible)
        batch = images[0].new_full((len(images), images[0].shape[0], Hp, Wp), 0)
        mask = torch.ones((len(images), Hp, Wp), dtype=torch.bool, device=batch.device)
        for k, im in enumerate(images):
            batch[k, :, :im.shape[1], :im.shape[2]].copy_(im)
            mask[k, :im.shape[1], :im.shape[2]] = False
        batch = batch.to(self.dtype)
        if self.channels_last:
            batch = batch.contiguous(memory_format=torch.channels_last)
        return ImageBatch(batch, mask, torch.tensor(sizes, dtype=torch.int64).reshape(-1, 2),
                          torch.tensor(original, dtype=torch.int64).reshape(-1, 2))

    def batch_fused(self, images: Sequence[Tensor]) -> ImageBatch:
        images = list(images.unbind(0)) if isinstance(images, Tensor) else list(images)
        return batch_images(images, self.target_sizes(images), self.size_divisible, self.mean, self.std, normalize=not self.training,
                            dtype=self.dtype, channels_last=self.channels_last)

    def _targets(self, batch: ImageBatch, targets):
        if targets:
            check_boxes(targets)
            targets = prepare_targets(batch.image_sizes, targets)
        return targets

    @torch.no_grad()
    def forward_torch(self, images, targets=None):
        batch = self.batch_torch(images)
        return batch, self._targets(batch, targets)

    @torch.no_grad()
    def forward_fused(self, images, targets=None):
        batch = self.batch_fused(images)
        return batch, self._targets(batch, targets)

    def forward(self, images, targets=None):
        return self.forward_fused(images, targets) if self.takes_fused_route(images) else self.forward_torch(images, targets)
