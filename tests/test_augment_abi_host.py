"""The C entry of the training augmentation (``rdetr_augment_image_batch``, csrc/images.hip) on the host: what it refuses, before any HIP
call, in both output modes, and the descriptor's mirror.  Needs the built library and no GPU; the calls that would launch are in
tests/test_gpu_augment.py."""
import ctypes
import os
import re

from relation_detr_amd import _lib
from relation_detr_amd.frontend import images as fimages
from test_images_host import C_MEAN, C_STD, C_STD_ZERO, ONE, P8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = "images B src_is_u8 out_mode Hp Wp mean std normalize out_bf16 channels_last out mask stream".split()


def descs(n=1, **change):
    fields = dict(src=16, row_stride=64, channel_stride=4096, h=48, w=40, flip=0, rh=32, rw=27, top=0, left=0, oh=32, ow=27, dst=None,
                  dst_row_stride=0, dst_channel_stride=0)
    fields.update(change)
    table = (fimages._WindowDesc * n)()
    for k in range(n):
        table[k] = fimages._WindowDesc(**fields)
    return table


def to_u8(n=1, **change):
    return descs(n, **dict(dict(dst=16, dst_row_stride=32, dst_channel_stride=1024), **change))


BATCH = dict(images=descs(), B=1, src_is_u8=1, out_mode=0, Hp=64, Wp=64, mean=C_MEAN, std=C_STD, normalize=1, out_bf16=0, channels_last=0,
             out=ONE, mask=ONE, stream=None)
U8 = dict(BATCH, images=to_u8(), out_mode=1, Hp=0, Wp=0, mean=None, std=None, normalize=0, out=None, mask=None)
CASES = [
    (BATCH, {"B": 0}, 0), (BATCH, {"B": 0, "images": None}, 0), (BATCH, {"B": -1}, -1), (BATCH, {"images": None}, -1),
    (BATCH, {"out_mode": 2}, -1), (BATCH, {"out_mode": -1}, -1), (BATCH, {"out": None}, -1), (BATCH, {"mask": None}, -1),
    (BATCH, {"Hp": 0}, -1), (BATCH, {"mean": None}, -1), (BATCH, {"std": C_STD_ZERO}, -1), (BATCH, {"normalize": 2}, -1),
    (BATCH, {"images": descs(src=None)}, -1), (BATCH, {"images": descs(h=0)}, -1), (BATCH, {"images": descs(rw=0)}, -1),
    (BATCH, {"images": descs(ow=-1)}, -1), (BATCH, {"images": descs(row_stride=-64)}, -1), (BATCH, {"images": descs(flip=2)}, -1),
    (BATCH, {"images": descs(top=-1)}, -1), (BATCH, {"images": descs(top=1)}, -1), (BATCH, {"images": descs(left=1)}, -1),
    (BATCH, {"images": descs(left=-1, ow=20)}, -1), (BATCH, {"images": descs(rh=100, oh=65)}, -1), (BATCH, {"images": descs(rw=100, ow=65)}, -1),
    (BATCH, {"images": descs(17), "B": 17}, -2), (BATCH, {"images": descs(h=257)}, -2), (BATCH, {"images": descs(w=217)}, -2),
    (BATCH, {"Wp": 68}, -2),
    (BATCH, {"out": P8}, -2), (BATCH, {"mask": ctypes.c_void_p(4)}, -2), (BATCH, {"normalize": 0}, -2),
    (BATCH, {"images": descs(src=18), "src_is_u8": 0}, -2), (BATCH, {"B": 0, "Wp": 68}, -2),
    (U8, {"B": 0}, 0), (U8, {"images": to_u8(dst=None)}, -1), (U8, {"images": to_u8(dst_row_stride=-16)}, -1), (U8, {"images": to_u8(top=1)}, -1),
    (U8, {"src_is_u8": 0}, -2), (U8, {"images": to_u8(dst=8)}, -2), (U8, {"images": to_u8(dst_row_stride=24)}, -2),
    (U8, {"images": to_u8(dst_row_stride=16)}, -2), (U8, {"images": to_u8(dst_channel_stride=1000)}, -2), (U8, {"images": to_u8(h=257)}, -2),
    (U8, {"images": to_u8(17), "B": 17}, -2),
]


def test_refusal_before_any_hip_call():
    fn = _lib.load().rdetr_augment_image_batch
    wrong = []
    for base, change, status in CASES:
        assert set(change) <= set(NAMES) and sorted(base) == sorted(NAMES)
        args = dict(base, **change)
        got = fn(*(args[n] for n in NAMES))
        if got != status:
            wrong.append((base["out_mode"], {k: v for k, v in change.items() if k != "images"} or "images", got, status))
    assert not wrong, wrong


def test_descriptor_and_header():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert len(re.findall(r"^int rdetr_augment_image_batch\s*\(", header, re.M)) == 1
    declared = re.search(r"^int rdetr_augment_image_batch\s*\(([^;]*)\);", header, re.M | re.S).group(1)
    assert len(declared.split(",")) == len(_lib.SIGNATURES["rdetr_augment_image_batch"]) == len(NAMES)
    assert "#define RDETR_IMAGE_OUT_BATCH 0\n" in header and "#define RDETR_IMAGE_OUT_U8 1\n" in header
    struct = re.search(r"typedef struct rdetr_image_window_desc \{(.*?)\} rdetr_image_window_desc;", header, re.S).group(1)
    names = re.findall(r"[\s\*,](\w+)(?=[,;])", struct)
    assert names == [n for n, _ in fimages._WindowDesc._fields_], names
    assert ctypes.sizeof(fimages._WindowDesc) == 88 and fimages._WindowDesc.dst.offset == 64
    assert "#define RDETR_ABI_VERSION 3" in header                                # an added symbol, no changed one
