"""GPU checks of the image front end (csrc/images.hip, relation_detr_amd/frontend, RelationDETRWithBackbone).

Every comparison is element by element against the float64 restatement of torch's antialias filter (test_images_host.resize64):
  uint8 sources   the near-tie rule of tests/test_images_host.py: off the ties the value is (float(rint(v64)) / 255 - mean) / std to
                  the bit; on them one of the three neighbouring values; a batch with more than 2 % near ties fails as ill-posed
  float sources   within max(4 * e32, 2^-20 * max(1, |ref64|)) of ref64 = (v64 - mean) / std, e32 the error of torch's own fp32 CPU
                  interpolate on that image
  copies          (no resize) bit-equal to the source, or to the table value of the source byte
  always          the mask exact, the padding +0 to the bit, bf16 = the rounding of the fp32 result to the bit, channels-last equal to
                  NCHW to the bit
The shapes are the smallest that reach each path of the kernel: ragged uint8 rows, one lane, one tile, several tiles per axis, tiles
of pure padding, a batch split over two launches, the downscale limit and one step beyond it."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from relation_detr_amd import _lib, frontend
from relation_detr_amd.frontend import ImagePreprocessor, batch_images, images as fimages
from test_images_host import (MEAN, NEAR_TIE_SHARE, STD, check_float, check_normalised, interpolate_error, near_tie, normalised_table,
                              resize64, tiny_detector, training_inputs)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def g13():
    return load_golden("g13_preprocess.npz")


def random_images(sizes, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return [torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g) for h, w in sizes]
    return [torch.rand(3, h, w, generator=g) for h, w in sizes]


def check_layout(batch, sizes, originals, Hp, Wp):
    B = len(sizes)
    assert tuple(batch.tensors.shape) == (B, 3, Hp, Wp) and tuple(batch.mask.shape) == (B, Hp, Wp) and batch.mask.dtype == torch.bool
    assert batch.image_sizes.tolist() == [list(s) for s in sizes] and batch.original_sizes.tolist() == [list(s) for s in originals]
    assert batch.image_sizes.device.type == "cpu" and batch.image_sizes.dtype == torch.int64
    mask = batch.mask.cpu().numpy()
    got = batch.tensors.float().cpu().numpy()
    for i, (oh, ow) in enumerate(sizes):
        want = np.ones((Hp, Wp), dtype=bool)
        want[:oh, :ow] = False
        assert np.array_equal(mask[i], want), (i, "mask")
        pad = got[i].copy()
        pad[:, :oh, :ow] = 0
        assert not pad.view(np.uint32).any(), (i, "padding is not +0")
    return got


def check_batch(batch, sources, sizes, what=""):
    """An fp32 batch against float64, every element.  ``sources``: the CPU images the device images were copied from."""
    originals = [tuple(s.shape[1:]) for s in sources]
    Hp, Wp = frontend.batched_size(sizes, 32)
    got = check_layout(batch, sizes, originals, Hp, Wp)
    assert batch.tensors.dtype == F32
    n_near = n_all = 0
    for i, (src, (oh, ow)) in enumerate(zip(sources, sizes)):
        src = src.numpy()
        if src.dtype == np.uint8:
            v64 = resize64(src, oh, ow)
            q64, near = near_tie(v64, interpolate_error(src, v64))
            if (oh, ow) == src.shape[1:]:
                assert not near.any()                                               # a copy has no ties
            check_normalised(got[i, :, :oh, :ow], q64, near, (what, i))
            n_near, n_all = n_near + int(near.sum()), n_all + near.size
        else:
            check_float(got[i, :, :oh, :ow], src, oh, ow, (what, i))
    assert n_near <= NEAR_TIE_SHARE * max(n_all, 1), f"{what}: {n_near} of {n_all} values are near ties; the comparison is ill-posed"
    return got


def run(sources, sizes, **kw):
    return batch_images([s.to(DEV) for s in sources], sizes, **kw)


# ------------------------------------------------------------------------------------------------------------- the golden batches
@pytest.mark.parametrize("name", ("u8a", "u8b"))
def test_golden_uint8_batches_every_dtype_and_layout(g13, name):
    lo, hi, div = g13[f"{name}.config"].tolist()
    n = len(g13[f"{name}.image_sizes"])
    sources = [T(g13[f"{name}.src{i}"]) for i in range(n)]
    sizes = [tuple(s) for s in g13[f"{name}.image_sizes"].tolist()]
    pre = ImagePreprocessor(lo, hi, div).eval()
    device_images = [s.to(DEV) for s in sources]
    assert pre.takes_fused_route(device_images) and pre.target_sizes(device_images) == sizes
    batch, _ = pre(device_images)
    got = check_batch(batch, sources, sizes, name)
    assert batch.tensors.is_contiguous()
    fixture = g13[f"{name}.tensors"]
    assert np.array_equal(batch.mask.cpu().numpy(), g13[f"{name}.mask"] != 0)
    for i, (oh, ow) in enumerate(sizes):                                            # and against what the reference recorded
        v64 = resize64(g13[f"{name}.src{i}"], oh, ow)
        _, near = near_tie(v64, interpolate_error(g13[f"{name}.src{i}"], v64))
        a, b = got[i, :, :oh, :ow], fixture[i, :, :oh, :ow]
        print(f"{name}[{i}]: {int((a != b).sum())} of {a.size} values differ from the fixture, {int(near.sum())} near ties")
        assert np.array_equal(a[~near], b[~near])
    for dtype in (F32, BF16):
        for cl in (False, True):
            other = ImagePreprocessor(lo, hi, div, dtype=dtype, channels_last=cl).eval()(device_images)[0]
            assert other.tensors.dtype == dtype
            assert other.tensors.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
            assert torch.equal(other.tensors, batch.tensors.to(dtype)), (dtype, cl)      # bf16: the rounding of the fp32 value
            assert torch.equal(other.mask, batch.mask)
            padded = np.broadcast_to((g13[f"{name}.mask"] != 0)[:, None], other.tensors.shape)
            assert not other.tensors.float().cpu().numpy()[padded].view(np.uint32).any()             # +0, not -0


def test_float_batch_is_not_rounded(g13):
    n = len(g13["f32.image_sizes"])
    sources = [T(g13[f"f32.src{i}"]) for i in range(n)]
    sizes = [tuple(s) for s in g13["f32.image_sizes"].tolist()]
    pre = ImagePreprocessor(*g13["f32.config"].tolist()).eval()
    batch, _ = pre([s.to(DEV) for s in sources])
    check_batch(batch, sources, sizes, "f32")
    for cl in (False, True):
        other = ImagePreprocessor(*g13["f32.config"].tolist(), dtype=BF16, channels_last=cl).eval()([s.to(DEV) for s in sources])[0]
        assert torch.equal(other.tensors, batch.tensors.to(BF16)) and torch.equal(other.mask, batch.mask)


def test_training_mode_and_no_resize_copy_bits(g13):
    images, targets = training_inputs(g13, DEV)
    pre = ImagePreprocessor(800, 1333).train()
    assert pre.takes_fused_route(images)
    batch, prepared = pre(images, targets)
    assert np.array_equal(batch.tensors.cpu().numpy().view(np.uint32), g13["train.tensors"].view(np.uint32))
    assert np.array_equal(batch.mask.cpu().numpy(), g13["train.mask"] != 0)
    assert torch.equal(batch.image_sizes, batch.original_sizes) and np.array_equal(batch.image_sizes.numpy(), g13["train.image_sizes"])
    for i, p in enumerate(prepared):
        np.testing.assert_array_equal(p["boxes"].cpu().numpy(), g13[f"train.boxes_out{i}"])
    for dtype, cl in ((BF16, False), (F32, True), (BF16, True)):
        other = ImagePreprocessor(dtype=dtype, channels_last=cl).train()(images)[0]
        assert torch.equal(other.tensors, batch.tensors.to(dtype)) and torch.equal(other.mask, batch.mask)
    # eval mode without sizes: uint8 bytes through the table, float images through (v - mean) / std, no filter
    sources = random_images([(37, 67), (64, 33), (5, 1)], torch.uint8, 5)
    batch, _ = ImagePreprocessor().eval()([s.to(DEV) for s in sources])
    got = check_layout(batch, [tuple(s.shape[1:]) for s in sources], [tuple(s.shape[1:]) for s in sources], 64, 96)
    table = normalised_table()
    for i, s in enumerate(sources):
        assert np.array_equal(got[i, :, :s.shape[1], :s.shape[2]], table[np.arange(3).reshape(3, 1, 1), s.numpy().astype(np.int64)])
    sources = random_images([(37, 67), (64, 36)], F32, 6)
    batch, _ = ImagePreprocessor().eval()([s.to(DEV) for s in sources])
    for i, s in enumerate(sources):
        want = s.clone().sub_(torch.tensor(MEAN).view(3, 1, 1)).div_(torch.tensor(STD).view(3, 1, 1))
        assert torch.equal(batch.tensors[i, :, :s.shape[1], :s.shape[2]].cpu(), want)


# -------------------------------------------------------------------------------------------------- shapes that can break a kernel
# name -> (source sizes, resized sizes or None, source dtype)
SHAPES = {
    "widths 1, 3, 5, 67 copied": ([(9, 1), (7, 3), (11, 5), (13, 67)], None, torch.uint8),
    "widths 1, 3, 5, 67 resized": ([(9, 1), (7, 3), (11, 5), (13, 67)], [(13, 2), (10, 4), (8, 7), (17, 83)], torch.uint8),
    "smaller than one tile": ([(5, 7)], [(9, 11)], torch.uint8),
    "one image sets Hp, another Wp": ([(100, 30), (20, 140)], [(90, 27), (17, 131)], torch.uint8),
    "already divisible by 32: no padding tile": ([(50, 91)], [(64, 96)], torch.uint8),
    "upscale, downscale and copy in one batch": ([(40, 60), (120, 90), (64, 64)], [(57, 85), (53, 41), (64, 64)], torch.uint8),
    "downscale 4.1 x 4.7, uint8: taps beyond the registers": ([(131, 155)], [(32, 33)], torch.uint8),
    "downscale 7.9 x 7.7, uint8": ([(127, 131)], [(16, 17)], torch.uint8),
    "the largest downscale, 8 x 8, float, two tiles down": ([(136, 128)], [(17, 16)], F32),
    "float, several tiles per axis": ([(45, 150), (70, 61)], [(37, 131), (90, 77)], F32),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(name):
    originals, sizes, dtype = SHAPES[name]
    sources = random_images(originals, dtype, len(name))
    sizes = sizes or originals
    batch = run(sources, sizes)
    check_batch(batch, sources, sizes, name)
    again = run(sources, sizes)
    assert torch.equal(batch.tensors, again.tensors) and torch.equal(batch.mask, again.mask)           # the same bits
    other = run(sources, sizes, dtype=BF16, channels_last=True)
    assert torch.equal(other.tensors, batch.tensors.to(BF16)) and torch.equal(other.mask, batch.mask)


def test_crop_of_a_larger_tensor():
    for dtype in (torch.uint8, F32):
        big = random_images([(90, 150)], dtype, 9)[0]
        crop = big[:, 7:80, 13:118]                                                 # rows 150 apart, the first byte at offset 13
        assert not crop.is_contiguous()
        device_crop = big.to(DEV)[:, 7:80, 13:118]
        for sizes in ([(57, 83)], [(73, 105)]):
            batch = batch_images([device_crop], sizes)
            check_batch(batch, [crop], sizes, ("crop", dtype, sizes))


def test_batch_split_over_two_launches():
    B = frontend.MAX_IMAGES + 1
    originals = [(20 + i, 30 + 2 * i) for i in range(B)]
    sizes = [(23 + i, 37 + i) for i in range(B)]
    sources = random_images(originals, torch.uint8, 17)
    batch = run(sources, sizes)
    check_batch(batch, sources, sizes, "B = MAX_IMAGES + 1")
    one = run(sources[-1:], sizes[-1:])                                             # B = 1, and the slice of the second launch
    assert torch.equal(one.tensors[0, :, :sizes[-1][0], :sizes[-1][1]], batch.tensors[-1, :, :sizes[-1][0], :sizes[-1][1]])


def test_beyond_the_downscale_limit_takes_the_torch_route():
    source = random_images([(400, 90)], torch.uint8, 3)[0].to(DEV)
    pre = ImagePreprocessor(20, 50).eval()
    assert pre.target_sizes([source]) == [(50, 11)] and not pre.takes_fused_route([source])         # 8.2 x down in width
    batch, _ = pre([source])
    plain, _ = ImagePreprocessor(20, 50, fused=False).eval()([source])
    assert torch.equal(batch.tensors, plain.tensors) and torch.equal(batch.mask, plain.mask)
    with pytest.raises(_lib.RdetrError, match="downscale"):
        batch_images([source], [(50, 11)])
    out, mask = torch.empty(1, 3, 64, 32, device=DEV), torch.empty(1, 64, 32, dtype=torch.bool, device=DEV)
    mean, std = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    table = (fimages._ImageDesc * 1)(fimages._ImageDesc(source.data_ptr(), 90, 36000, 400, 90, 50, 11))
    assert _lib.load().rdetr_image_batch(table, 1, 1, 64, 32, mean, std, 1, 0, 0, out.data_ptr(), mask.data_ptr(), None) == -2


def test_orders_after_work_on_its_stream():
    old, new = random_images([(70, 90), (70, 90)], torch.uint8, 21)
    want = run([new], [(57, 73)])
    source = old.to(DEV)
    fresh = new.to(DEV)
    a = torch.randn(1024, 1024, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(8):                                                           # work in front of the copy on the side stream
            a = a @ a * 1e-3
        source.copy_(fresh, non_blocking=True)
        got = batch_images([source], [(57, 73)])
    side.synchronize()
    assert torch.equal(got.tensors, want.tensors) and torch.equal(got.mask, want.mask)


# ------------------------------------------------------------------------------------------------------------------ the detector
def test_detector_from_images_end_to_end(g13):
    images = [T(g13[f"u8b.src{i}"]).to(DEV) for i in range(4)]
    sizes = [tuple(s) for s in g13["u8b.image_sizes"].tolist()]
    model = tiny_detector(DEV, True).eval()
    assert isinstance(model.preprocessor, ImagePreprocessor) and model.preprocessor.takes_fused_route(images)
    plain_pre = ImagePreprocessor(64, 100, fused=False).eval()
    with torch.no_grad():
        fused_batch, _ = model.preprocessor(images)
        plain_batch, _ = plain_pre(images)
    check_batch(fused_batch, [im.cpu() for im in images], sizes, "detector")
    check_batch(plain_batch, [im.cpu() for im in images], sizes, "detector, torch route")
    assert torch.equal(fused_batch.mask, plain_batch.mask) and torch.equal(fused_batch.original_sizes, plain_batch.original_sizes)

    class Fixed(torch.nn.Module):                                                     # the fused batch handed to both detectors
        def forward(self, images, targets=None):
            return fused_batch, targets

    from relation_detr_amd import RelationDETRWithBackbone
    parts = (model.backbone, model.neck, model.position_embedding, model.transformer, model.criterion, model.denoising_generator)
    other = RelationDETRWithBackbone(*parts, plain_pre, 10).eval()                   # the same network behind the torch front end
    # the library's 3 x 3 stride-2 convolution of the neck's extra level adds with atomics unless told otherwise (2.4e-7 from run to
    # run on its [4, 256, 2, 2] input, measured); equal detections need it deterministic
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            dets, tensor = model(images)
            dets_plain, tensor_plain = other(images)                                 # runs; differs where a near tie rounded the other way
            model.preprocessor = other.preprocessor = Fixed()
            dets_a, tensor_a = model(images)
            dets_b, tensor_b = other(images)
    finally:
        torch.backends.cudnn.deterministic = was
    assert tuple(tensor.shape) == (4, 10, 6) == tuple(tensor_plain.shape) and len(dets_plain) == 4
    assert torch.equal(tensor_a, tensor_b) and torch.equal(tensor, tensor_a)
    for a, b in zip(dets_a, dets_b):
        assert all(torch.equal(a[k], b[k]) for k in ("scores", "labels", "boxes"))
    assert torch.isfinite(tensor).all() and torch.isfinite(tensor_plain).all()
    wh = fused_batch.original_sizes.to(DEV).flip(1).repeat(1, 2).to(tensor.dtype)          # boxes in pixels of the original images
    assert (tensor[:, :, :4].abs() <= 2.0 * wh[:, None, :]).all()
