"""Host side of the image front end (relation_detr_amd/frontend, RelationDETRWithBackbone): the float32 size rule and the torch route
against what the reference's own code recorded (tests/golden/g13_preprocess.npz), the ABI's refusals, the exports, and the detector
from a list of images on the CPU.  Needs no GPU.  tests/test_gpu_images.py imports the float64 filter and the near-tie rule from here.

The near-tie rule.  A uint8 image is resized as round(filter(float32 copy)); where the exact filter value v64 lies on x.5 the
rounding is decided by the last bits of an fp32 sum, and torch's own CPU result flips there from build to build.  So, with
q64 = rint(v64), d = |v64 - floor(v64) - 0.5| and delta = max(4 * e32, 255 * 2^-20) (e32: the largest error of torch's fp32 CPU
interpolate against v64 on that image):  d >= delta -> the result is the value for q64, exactly;  d < delta -> q64 - 1, q64 or
q64 + 1;  and near-tie values are at most 2 % of a batch's valid values, else the test is ill-posed and fails.
"""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import relation_detr_amd
from conftest import load_golden
from helpers import synthetic_state_dict
from relation_detr_amd import _lib, detector, frontend, options
from relation_detr_amd.frontend import ImagePreprocessor, images as fimages, resized_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NEAR_TIE_SHARE = 0.02
UINT8_BATCHES = ("u8a", "u8b")


@pytest.fixture(scope="module")
def g13():
    return load_golden("g13_preprocess.npz")


# ------------------------------------------------------------------------------------------------- float64 filter, near-tie rule
def filter_matrix(n_in: int, n_out: int) -> np.ndarray:
    """[n_out, n_in] float64: torch's antialiased bilinear taps for n_in -> n_out."""
    W = np.zeros((n_out, n_in))
    scale = n_in / n_out
    support = max(scale, 1.0)
    inv = 1.0 / support
    for o in range(n_out):
        center = scale * (o + 0.5)
        lo, hi = max(int(center - support + 0.5), 0), min(int(center + support + 0.5), n_in)
        w = np.maximum(0.0, 1.0 - np.abs((np.arange(lo, hi) - center + 0.5) * inv))
        W[o, lo:hi] = w / w.sum()
    return W


def resize64(image: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """[3, h, w] -> [3, oh, ow] float64, the exact filter."""
    x = image.astype(np.float64)
    return np.einsum("yj,cji,xi->cyx", filter_matrix(x.shape[1], oh), x, filter_matrix(x.shape[2], ow))


def interpolate_error(image: np.ndarray, v64: np.ndarray) -> float:
    """e32: torch's fp32 CPU interpolate against the exact filter, in the image's own units."""
    x = torch.from_numpy(np.ascontiguousarray(image)).to(torch.float32)[None]
    y = torch.nn.functional.interpolate(x, size=list(v64.shape[1:]), mode="bilinear", align_corners=False, antialias=True)[0]
    return float(np.abs(y.numpy().astype(np.float64) - v64).max())


def near_tie(v64: np.ndarray, e32: float):
    """(q64, the mask of near-tie values) for a uint8 image's exact filter values."""
    delta = max(4.0 * e32, 255.0 * 2.0 ** -20)
    return np.rint(v64), np.abs(v64 - np.floor(v64) - 0.5) < delta


def check_quantised(got_q: np.ndarray, q64: np.ndarray, near: np.ndarray, what=""):
    """The rule on integer values: exact off the ties, within one step on them.  Returns the mismatch count on the ties."""
    off = ~near
    assert np.array_equal(got_q[off], q64[off]), (what, int((got_q[off] != q64[off]).sum()), "values differ off the ties")
    assert (np.abs(got_q[near].astype(np.float64) - q64[near]) <= 1).all(), (what, "a near-tie value is more than one step off")
    return int((got_q[near] != q64[near]).sum())


def normalised_table() -> np.ndarray:
    """[3, 256] float32: (float(q) / 255 - mean) / std with torch's three fp32 operations."""
    q = torch.arange(256, dtype=torch.float32).view(1, 256).repeat(3, 1) / 255
    return q.sub_(torch.tensor(MEAN).view(3, 1)).div_(torch.tensor(STD).view(3, 1)).numpy()


def check_normalised(got: np.ndarray, q64: np.ndarray, near: np.ndarray, what=""):
    """The rule on a normalised [3, oh, ow] float32 result: bit-equal to the table's value for q64 off the ties, one of the three
    neighbouring table values on them."""
    table = normalised_table()
    rows = np.arange(3).reshape(3, 1, 1)
    q = q64.astype(np.int64)
    want = table[rows, q]
    off = ~near
    assert np.array_equal(got[off], want[off]), (what, int((got[off] != want[off]).sum()), "values differ off the ties")
    ok = (got == want) | (got == table[rows, np.clip(q - 1, 0, 255)]) | (got == table[rows, np.clip(q + 1, 0, 255)])
    assert ok[near].all(), (what, "a near-tie value is none of the three neighbours")


def check_float(got: np.ndarray, src: np.ndarray, oh: int, ow: int, what=""):
    """A float32 image, no rounding: within max(4 * e32, 2^-20 * max(1, |ref64|)) of ref64 = (v64 - mean) / std."""
    v64 = resize64(src, oh, ow)
    e32 = interpolate_error(src, v64)
    ref = (v64 - np.array(MEAN).reshape(3, 1, 1)) / np.array(STD).reshape(3, 1, 1)
    err = np.abs(got.astype(np.float64) - ref)
    bound = np.maximum(4.0 * e32, 2.0 ** -20 * np.maximum(1.0, np.abs(ref)))
    print(f"{what}: float error {err.max():.3e}, e32 {e32:.3e}, smallest bound {bound.min():.3e}")
    assert (err <= bound).all(), (what, float(err.max()), float(bound.min()))


def uint8_batch_reference(g13, name):
    """Per image of a golden uint8 batch: (source, v64, q64, near), and the check that the batch is well-posed."""
    sizes = g13[f"{name}.image_sizes"]
    out, n_near, n_all = [], 0, 0
    for i, (oh, ow) in enumerate(sizes.tolist()):
        src = g13[f"{name}.src{i}"]
        v64 = resize64(src, oh, ow)
        q64, near = near_tie(v64, interpolate_error(src, v64))
        out.append((src, v64, q64, near))
        n_near, n_all = n_near + int(near.sum()), n_all + near.size
    assert n_near <= NEAR_TIE_SHARE * n_all, f"{name}: {n_near} of {n_all} values are near ties; the comparison is ill-posed"
    return out


# ----------------------------------------------------------------------------------------------------------------- the size rule
def test_resized_size_is_the_reference_rule(g13):
    table = g13["sizes"]
    assert len(table) >= 300
    wrong = [tuple(r) for r in table.tolist() if resized_size(r[0], r[1], r[2], r[3]) != (r[4], r[5])]
    assert not wrong, wrong[:5]
    assert {(800, 1333), (1200, 2000), (64, 100), (31, 50)} <= {(r[2], r[3]) for r in table.tolist()}


def test_resized_size_is_not_the_python_float_rule(g13):
    def python_rule(h, w, lo, hi):
        r = min(lo / min(h, w), hi / max(h, w))
        return int(h * r), int(w * r)
    differ = [tuple(r) for r in g13["sizes"].tolist() if python_rule(*r[:4]) != (r[4], r[5])]
    assert differ, "every row agrees with double arithmetic: the table no longer pins the float32 rule"
    assert all(isinstance(v, int) for v in resized_size(480, 640, 800, 1333))


# ------------------------------------------------------------------------------------------------------------- the torch route
@pytest.mark.parametrize("name", UINT8_BATCHES)
def test_torch_route_resizes_uint8_as_the_reference(g13, name):
    lo, hi, _ = g13[f"{name}.config"].tolist()
    mismatches = 0
    for i, (src, v64, q64, near) in enumerate(uint8_batch_reference(g13, name)):
        oh, ow = g13[f"{name}.image_sizes"][i].tolist()
        assert resized_size(src.shape[1], src.shape[2], lo, hi) == (oh, ow)
        got = frontend.resize_image(T(src), (oh, ow))
        assert got.dtype == torch.uint8
        check_quantised(got.numpy(), q64, near, (name, i))
        check_quantised(g13[f"{name}.resized{i}"], q64, near, (name, i, "fixture"))
        mismatches += int((got.numpy() != g13[f"{name}.resized{i}"]).sum())
    print(f"{name}: {mismatches} resized values differ from the fixture")       # 0 where it was recorded; the rule is what must hold


@pytest.mark.parametrize("name", UINT8_BATCHES + ("f32",))
def test_torch_route_batches_as_the_reference(g13, name):
    lo, hi, div = g13[f"{name}.config"].tolist()
    n = len(g13[f"{name}.image_sizes"])
    pre = ImagePreprocessor(lo, hi, div, fused=False).eval()
    batch, targets = pre([T(g13[f"{name}.src{i}"]) for i in range(n)])
    assert targets is None and pre.state_dict() == {} and not pre.takes_fused_route([T(g13[f"{name}.src0"])])
    want = g13[f"{name}.tensors"]
    assert batch.tensors.dtype == torch.float32 and tuple(batch.tensors.shape) == want.shape
    assert batch.mask.dtype == torch.bool and np.array_equal(batch.mask.numpy(), g13[f"{name}.mask"] != 0)
    assert batch.image_sizes.dtype == torch.int64 and np.array_equal(batch.image_sizes.numpy(), g13[f"{name}.image_sizes"])
    assert np.array_equal(batch.original_sizes.numpy(), [g13[f"{name}.src{i}"].shape[1:] for i in range(n)])
    got = batch.tensors.numpy()
    for i, (oh, ow) in enumerate(g13[f"{name}.image_sizes"].tolist()):
        pad = got[i].copy()
        pad[:, :oh, :ow] = 0
        assert not pad.view(np.uint32).any(), (name, i, "padding is not +0")
        src = g13[f"{name}.src{i}"]
        if name == "f32":
            # two fp32 evaluations of one filter, each within e32 of v64 before the division by std, and one fp32 rounding each after
            e32 = interpolate_error(src, resize64(src, oh, ow))
            a, b = got[i, :, :oh, :ow].astype(np.float64), want[i, :, :oh, :ow].astype(np.float64)
            assert (np.abs(a - b) <= 2.0 * e32 / min(STD) + 2.0 ** -22 * np.maximum(1.0, np.abs(b))).all(), (name, i, np.abs(a - b).max())
        else:
            v64 = resize64(src, oh, ow)
            q64, near = near_tie(v64, interpolate_error(src, v64))
            check_normalised(got[i, :, :oh, :ow], q64, near, (name, i))
            check_normalised(want[i, :, :oh, :ow], q64, near, (name, i, "fixture"))


def test_torch_route_other_layouts(g13):
    images = [T(g13[f"u8a.src{i}"]) for i in range(3)]
    base = ImagePreprocessor(31, 50, fused=False).eval()(images)[0].tensors
    for dtype in (torch.float32, torch.bfloat16):
        for cl in (False, True):
            t = ImagePreprocessor(31, 50, dtype=dtype, channels_last=cl, fused=False).eval()(images)[0].tensors
            assert t.dtype == dtype and t.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
            assert torch.equal(t, base.to(dtype))


def training_inputs(g13, device="cpu"):
    n = len(g13["train.image_sizes"])
    images = [T(g13[f"train.src{i}"]).to(device) for i in range(n)]
    targets = [{"labels": T(g13[f"train.labels{i}"]).to(device), "boxes": T(g13[f"train.boxes_in{i}"]).to(device)} for i in range(n)]
    return images, targets


def test_training_mode_batches_and_prepares_targets(g13):
    images, targets = training_inputs(g13)
    kept = [t["boxes"].clone() for t in targets]
    pre = ImagePreprocessor(800, 1333, fused=False).train()
    batch, prepared = pre(images, targets)
    assert np.array_equal(batch.tensors.numpy().view(np.uint32), g13["train.tensors"].view(np.uint32))         # copies: every bit
    assert np.array_equal(batch.mask.numpy(), g13["train.mask"] != 0)
    assert np.array_equal(batch.image_sizes.numpy(), g13["train.image_sizes"]) and torch.equal(batch.image_sizes, batch.original_sizes)
    for i, (t, p) in enumerate(zip(targets, prepared)):
        assert torch.equal(t["boxes"], kept[i]) and p["boxes"] is not t["boxes"]            # the input is not overwritten
        assert torch.equal(p["labels"], t["labels"])
        np.testing.assert_array_equal(p["boxes"].numpy(), g13[f"train.boxes_out{i}"])
    bad = [{"labels": torch.zeros(1, dtype=torch.int64), "boxes": torch.tensor([[4.0, 4.0, 4.0, 9.0]])}]
    with pytest.raises(ValueError, match="positive height and width"):
        pre(images[:1], bad)


# -------------------------------------------------------------------------------------------------------------------------- ABI
ONE, P8 = ctypes.c_void_p(16), ctypes.c_void_p(8)
C_MEAN, C_STD, C_STD_ZERO = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD), (ctypes.c_float * 3)(0.229, 0.0, 0.225)


def descs(n=1, **change):
    fields = dict(src=16, row_stride=64, channel_stride=4096, h=48, w=40, oh=32, ow=27)
    fields.update(change)
    table = (fimages._ImageDesc * n)()
    for k in range(n):
        table[k] = fimages._ImageDesc(**fields)
    return table


IMAGE_BATCH = ("images B src_is_u8 Hp Wp mean std normalize out_bf16 channels_last out mask stream",
               dict(images=descs(), B=1, src_is_u8=1, Hp=64, Wp=64, mean=C_MEAN, std=C_STD, normalize=1, out_bf16=0, channels_last=0, out=ONE,
                    mask=ONE, stream=None),
               [({"B": 0}, 0), ({"B": 0, "images": None}, 0), ({"B": -1}, -1), ({"images": None}, -1), ({"out": None}, -1), ({"mask": None}, -1),
                ({"Hp": 0}, -1), ({"Wp": -8}, -1), ({"mean": None}, -1), ({"std": None}, -1), ({"std": C_STD_ZERO}, -1), ({"normalize": 2}, -1),
                ({"images": descs(src=None)}, -1), ({"images": descs(h=0)}, -1), ({"images": descs(ow=-1)}, -1),
                ({"images": descs(row_stride=-64)}, -1), ({"images": descs(oh=65)}, -1), ({"images": descs(ow=65)}, -1),
                ({"images": descs(17), "B": 17}, -2), ({"images": descs(h=257)}, -2), ({"images": descs(w=217)}, -2), ({"Wp": 68}, -2),
                ({"out": P8}, -2), ({"mask": ctypes.c_void_p(4)}, -2), ({"normalize": 0}, -2),
                ({"images": descs(src=18), "src_is_u8": 0}, -2), ({"B": 0, "Wp": 68}, -2)])
TABLE = {"rdetr_image_batch": IMAGE_BATCH}


@pytest.mark.parametrize("entry", sorted(TABLE))
def test_refusal_before_any_hip_call(entry):
    names, base, cases = TABLE[entry]
    names = names.split()
    assert sorted(names) == sorted(base), entry
    fn = getattr(_lib.load(), entry)
    wrong = []
    for change, status in cases:
        assert set(change) <= set(names), (entry, change)
        args = dict(base, **change)
        got = fn(*(args[n] for n in names))
        if got != status:
            wrong.append((change, got, status))
    assert not wrong, [(f"{c}: answered {g}, expected {s}") for c, g, s in wrong]


def test_abi_and_exports():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    new = [n for n in _lib.SIGNATURES if n.startswith("rdetr_image_")]
    assert new == ["rdetr_image_batch"]
    for name in new:
        assert len(re.findall(rf"^int {name}\s*\(", header, re.M)) == 1, name
    assert "#define RDETR_ABI_VERSION 3" in header and _lib.load().rdetr_abi_version() == 3
    assert f"#define RDETR_IMAGE_MAX_IMAGES {frontend.MAX_IMAGES}\n" in header
    assert f"#define RDETR_IMAGE_MAX_DOWNSCALE {frontend.MAX_DOWNSCALE}\n" in header
    assert ctypes.sizeof(fimages._ImageDesc) == 40
    assert "images.hip" in open(os.path.join(ROOT, "relation_detr_amd", "csrc", "Makefile")).read()
    assert len(dataclasses.fields(options.Options)) == 25                        # `fused` is a constructor argument
    for name in ("ImageBatch", "ImagePreprocessor", "batch_images", "resized_size"):
        assert name in relation_detr_amd.__all__ and getattr(relation_detr_amd, name) is getattr(frontend, name)
    assert "RelationDETRWithBackbone" in relation_detr_amd.__all__
    assert relation_detr_amd.RelationDETRWithBackbone is detector.RelationDETRWithBackbone
    assert relation_detr_amd.ImageBatch._fields == ("tensors", "mask", "image_sizes", "original_sizes")


def test_fused_call_has_no_cpu_path(g13):
    images = [T(g13["u8a.src0"])]
    with pytest.raises(_lib.RdetrError, match="not on a ROCm device"):
        frontend.batch_images(images, [(42, 31)])
    pre = ImagePreprocessor(31, 50).eval()                                       # fused=True: CPU tensors take the torch route
    assert not pre.takes_fused_route(images)
    assert torch.equal(pre(images)[0].tensors, ImagePreprocessor(31, 50, fused=False).eval()(images)[0].tensors)


# ------------------------------------------------------------------------------------------------------------------ the detector
class StandInBackbone(nn.Module):
    """Two convolutions: strides 8 and 16, 16 and 24 channels."""

    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(3, 16, 8, 8)
        self.b = nn.Conv2d(16, 24, 2, 2)

    def forward(self, x):
        a = self.a(x.float())
        return [a, self.b(a)]


def tiny_detector(device, fused, num_select=10, pre=None, **kw):
    from relation_detr_amd.neck import ChannelMapper, PositionEmbeddingSine
    from test_denoising_host import tiny_head
    head = tiny_head(device, fused, **kw)
    backbone, mapper = StandInBackbone(), ChannelMapper([16, 24], 256, 4, fused=fused)
    backbone.load_state_dict(synthetic_state_dict(backbone.state_dict()))
    mapper.load_state_dict(synthetic_state_dict(mapper.state_dict()))
    pre = pre if pre is not None else ImagePreprocessor(64, 100, fused=fused)
    return detector.RelationDETRWithBackbone(backbone, mapper, PositionEmbeddingSine(128, 10000, True, offset=-0.5, fused=fused),
                                             head.transformer, head.criterion, head.denoising_generator, pre, num_select).to(device)


def test_detector_from_images_on_cpu(g13):
    from oracle.cpu_modules import OracleMSDA, OracleRelation, OracleSelfAttention
    from relation_detr_amd import denoising as dn, select_detections
    from test_denoising_host import EXPECTED_KEYS, C
    model = tiny_detector("cpu", False, msda_cls=OracleMSDA, self_attn_cls=OracleSelfAttention, relation_cls=OracleRelation)
    plain = detector.RelationDETR(model.neck, model.position_embedding, model.transformer, model.criterion, model.denoising_generator)
    assert list(model.state_dict()) == list(plain.state_dict()) + [f"backbone.{k}" for k in model.backbone.state_dict()]
    assert sorted(model.state_dict()) == sorted(list(plain.state_dict()) + ["backbone.a.weight", "backbone.a.bias", "backbone.b.weight",
                                                                            "backbone.b.bias"])

    model.eval()
    images = [T(g13[f"u8b.src{i}"]) for i in range(2)]
    with torch.no_grad():
        dets, tensor = model(images)
        batch, _ = model.preprocessor(images)
        logits, boxes = plain.eval()(model.backbone(batch.tensors), batch.mask)
    assert tuple(tensor.shape) == (2, 10, 6) and len(dets) == 2
    assert torch.equal(tensor, select_detections(logits, boxes, batch.original_sizes, 10))
    assert not torch.equal(tensor, select_detections(logits, boxes, batch.image_sizes, 10))        # not the resized sizes
    for b, d in enumerate(dets):
        assert set(d) == {"scores", "labels", "boxes"} and d["labels"].dtype == torch.int64
        assert tuple(d["boxes"].shape) == (10, 4) and tuple(d["scores"].shape) == (10,) and tuple(d["labels"].shape) == (10,)
        assert torch.equal(d["boxes"], tensor[b, :, :4]) and torch.equal(d["scores"], tensor[b, :, 4])
        h, w = batch.original_sizes[b].tolist()
        assert float(d["boxes"][:, 0::2].abs().max()) <= 2.0 * w and float(d["boxes"][:, 1::2].abs().max()) <= 2.0 * h

    model.train()
    images, targets = training_inputs(g13)
    noise = dn.cdn_noise(11, 2 * dn.denoising_groups(6, 3) * 5, C, "cpu")
    losses = model(images, targets, noise)
    batch, prepared = model.preprocessor(images, targets)
    want = plain.train()(model.backbone(batch.tensors), batch.mask, prepared, noise)
    assert set(losses) == EXPECTED_KEYS == set(want)
    for k in want:
        assert torch.equal(losses[k], want[k]), k
