"""Generate tests/golden/g13_preprocess.npz by running the REFERENCE's own image front end (build machine only; no test runs this).

Run:  RELATION_DETR_REFERENCE=<checkout of the reference> python tools/gen_golden_preprocess.py

Run unmodified from the reference:
  transforms/_functional_tensor.py            loaded by file path (it imports only torch); ``resize`` is what resizes every image here
  models/detectors/base_detector.py           loaded by file path: ``EvalResize.forward``, ``BaseDetector.__init__`` /
                                              ``preprocess_image``, ``DETRDetector.construct_mask`` / ``prepare_targets`` / ``preprocess``
  util/misc.py::image_list_from_tensors       the function's source, taken from its file as oracle/gen_golden.py takes ``inverse_sigmoid``
                                              (the module itself imports fvcore, accelerate, terminaltables and the logger)
Stubs and restated pieces (tests/golden/g13_preprocess.md names them too):
  torchvision                                 ``_is_tracing() -> False``; ``models.detection.image_list.ImageList`` (tensors, image_sizes);
                                              ``ops.boxes._box_xyxy_to_cxcywh`` from its formula
  transforms.functional                       ``resize`` forwards to the real ``_functional_tensor.resize`` with the enum turned into its
                                              string and the two 0-dim size tensors into ints, as torchvision's does; it also records
                                              the size it was handed, which is the size table; ``InterpolationMode`` with BILINEAR
  transforms.v2                               ``ConvertImageDtype`` (``x.to(float32) / 255`` for uint8, float32 unchanged) and ``Normalize``
                                              (``x.sub_(mean).div_(std)`` on a clone), from their formulas
  util.misc, util.utils                       hold only the names base_detector.py imports; ``image_list_from_tensors`` is the reference's

The fixture holds data only.  Keys:
  sizes                       [N, 6] int64: h, w, min_size, max_size, oh, ow as EvalResize handed them to resize
  <batch>.src<i>              the source images; <batch>.resized<i> what resize returned; <batch>.tensors, .mask, .image_sizes
  <batch>.config              min_size, max_size, size_divisible
  u8a, u8b                    uint8 batches; f32 a float32 batch with values in [0, 1]
  train.*                     training mode: float images, no resize, targets before (boxes_in<i>, labels<i>) and after (boxes_out<i>)
"""
import ast
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g13_preprocess.npz")
BATCHES = {
    "u8a": dict(sizes=[(96, 70), (120, 131), (77, 203)], min_size=31, max_size=50, dtype=torch.uint8, seed=1),
    "u8b": dict(sizes=[(50, 91), (131, 80), (64, 64), (203, 77)], min_size=64, max_size=100, dtype=torch.uint8, seed=2),
    "f32": dict(sizes=[(45, 83), (110, 57)], min_size=37, max_size=61, dtype=torch.float32, seed=3),
}
TRAIN = dict(sizes=[(40, 57), (64, 33), (21, 64)], boxes=(3, 0, 2), seed=4)
HANDED = []                      # every size EvalResize handed to resize
SIZES_ONLY = [False]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return module


def _box_xyxy_to_cxcywh(boxes):
    x1, y1, x2, y2 = boxes.unbind(-1)
    return torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), dim=-1)


class ImageList:
    def __init__(self, tensors, image_sizes):
        self.tensors, self.image_sizes = tensors, image_sizes


class ConvertImageDtype(nn.Module):
    def __init__(self, dtype):
        super().__init__()
        assert dtype == torch.float32

    def forward(self, x):
        return x.to(torch.float32) / 255 if x.dtype == torch.uint8 else x


class Normalize(nn.Module):
    def __init__(self, mean, std, inplace=False):
        super().__init__()
        self.mean, self.std = mean, std

    def forward(self, x):
        mean, std = x.new_tensor(self.mean).view(-1, 1, 1), x.new_tensor(self.std).view(-1, 1, 1)
        return x.clone().sub_(mean).div_(std)


def import_reference():
    ref = os.environ.get("RELATION_DETR_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "models")):
        sys.exit("set RELATION_DETR_REFERENCE to a checkout of the reference")
    real = _load("_reference_functional_tensor", os.path.join(ref, "transforms", "_functional_tensor.py"))

    tv = types.ModuleType("torchvision")
    tv._is_tracing = lambda: False
    names = ["torchvision.models", "torchvision.models.detection", "torchvision.models.detection.image_list", "torchvision.ops",
             "torchvision.ops.boxes"]
    mods = {n: types.ModuleType(n) for n in names}
    mods["torchvision.models.detection.image_list"].ImageList = ImageList
    mods["torchvision.ops.boxes"]._box_xyxy_to_cxcywh = _box_xyxy_to_cxcywh
    tv.models, tv.ops = mods["torchvision.models"], mods["torchvision.ops"]
    mods["torchvision.models"].detection = mods["torchvision.models.detection"]
    mods["torchvision.models.detection"].image_list = mods["torchvision.models.detection.image_list"]
    mods["torchvision.ops"].boxes = mods["torchvision.ops.boxes"]
    sys.modules["torchvision"] = tv
    sys.modules.update(mods)

    class InterpolationMode:
        BILINEAR = "bilinear"

    def resize(image, size, interpolation=InterpolationMode.BILINEAR, antialias=None):
        size = [int(s) for s in size]
        HANDED.append(tuple(size))
        if SIZES_ONLY[0]:
            return image
        return real.resize(image, size=size, interpolation=str(interpolation), antialias=antialias)

    functional = types.ModuleType("transforms.functional")
    functional.resize, functional.InterpolationMode = resize, InterpolationMode
    v2 = types.ModuleType("transforms.v2")
    v2.ConvertImageDtype, v2.Normalize = ConvertImageDtype, Normalize
    transforms = types.ModuleType("transforms")
    transforms.__path__ = []
    transforms.functional, transforms.v2 = functional, v2
    sys.modules.update({"transforms": transforms, "transforms.functional": functional, "transforms.v2": v2})

    tree = ast.parse(open(os.path.join(ref, "util", "misc.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "image_list_from_tensors"][0]
    misc = types.ModuleType("util.misc")
    misc.__dict__.update(torch=torch, torchvision=tv, math=math, ImageList=ImageList, List=list, Tensor=torch.Tensor,
                         decode_labels=None, encode_labels=None)
    exec(compile(ast.Module([fn], []), "util/misc.py", "exec"), misc.__dict__)
    utils = types.ModuleType("util.utils")
    utils.get_world_size, utils.is_dist_avail_and_initialized = (lambda: 1), (lambda: False)
    util = types.ModuleType("util")
    util.__path__ = []
    util.misc, util.utils = misc, utils
    sys.modules.update({"util": util, "util.misc": misc, "util.utils": utils})
    return _load("_reference_base_detector", os.path.join(ref, "models", "detectors", "base_detector.py"))


def size_table(base):
    rows = []
    coco = [(480, 640), (427, 640), (640, 480), (375, 500), (500, 375), (333, 500), (640, 427), (612, 612), (428, 640), (640, 640),
            (360, 640), (480, 360), (1080, 1920), (2160, 3840), (600, 1000), (1200, 800), (51, 640), (640, 59), (1, 1), (3, 1000)]
    cases = [(h, w, 800, 1333) for h, w in coco] + [(h, w, 1200, 2000) for h, w in coco[:8]]
    cases += [(h, w, 800, 1333) for h in range(200, 700, 37) for w in range(200, 700, 29)]
    cases += [(h, w, 64, 100) for h in range(37, 140, 17) for w in range(41, 210, 23)]
    cases += [(h, w, 31, 50) for h in (70, 77, 96, 120) for w in (70, 131, 203)] + [(h, w, 37, 61) for h, w in BATCHES["f32"]["sizes"]]
    SIZES_ONLY[0] = True
    for h, w, lo, hi in cases:
        del HANDED[:]
        base.EvalResize(lo, hi, antialias=True)(torch.empty(1, h, w, dtype=torch.uint8))
        rows.append((h, w, lo, hi) + HANDED[0])
    SIZES_ONLY[0] = False
    return np.array(rows, dtype=np.int64)


def eval_batch(base, cfg):
    g = torch.Generator().manual_seed(cfg["seed"])
    if cfg["dtype"] == torch.uint8:
        images = [torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g) for h, w in cfg["sizes"]]
    else:
        images = [torch.rand(3, h, w, generator=g) for h, w in cfg["sizes"]]
    detector = base.DETRDetector(min_size=cfg["min_size"], max_size=cfg["max_size"], size_divisible=32).eval()
    resized = [detector.eval_transform[0](im) for im in images]
    batch, targets, mask = detector.preprocess([im.clone() for im in images], None)
    data = {"config": np.array([cfg["min_size"], cfg["max_size"], 32], dtype=np.int64), "tensors": batch.tensors.numpy(),
            "mask": mask.numpy(), "image_sizes": np.array([tuple(s) for s in batch.image_sizes], dtype=np.int64)}
    for i, (im, rs) in enumerate(zip(images, resized)):
        data[f"src{i}"], data[f"resized{i}"] = im.numpy(), rs.numpy()
    return data


def train_batch(base):
    g = torch.Generator().manual_seed(TRAIN["seed"])
    images = [torch.randn(3, h, w, generator=g) for h, w in TRAIN["sizes"]]
    targets = []
    for (h, w), k in zip(TRAIN["sizes"], TRAIN["boxes"]):
        xy = torch.rand(k, 2, generator=g) * torch.tensor([w * 0.5, h * 0.5])
        wh = 1.0 + torch.rand(k, 2, generator=g) * torch.tensor([w * 0.5 - 1.0, h * 0.5 - 1.0])
        targets.append({"labels": torch.randint(0, 11, (k,), generator=g), "boxes": torch.cat((xy, xy + wh), dim=-1)})
    detector = base.DETRDetector(min_size=800, max_size=1333, size_divisible=32).train()
    batch, prepared, mask = detector.preprocess([im.clone() for im in images], targets)
    data = {"tensors": batch.tensors.numpy(), "mask": mask.numpy(),
            "image_sizes": np.array([tuple(s) for s in batch.image_sizes], dtype=np.int64)}
    for i, (im, t, p) in enumerate(zip(images, targets, prepared)):
        data[f"src{i}"], data[f"labels{i}"] = im.numpy(), t["labels"].numpy()
        data[f"boxes_in{i}"], data[f"boxes_out{i}"] = t["boxes"].numpy().reshape(-1, 4), p["boxes"].numpy().reshape(-1, 4)
    return data


def main():
    base = import_reference()
    out = {"sizes": size_table(base)}
    print("size table", out["sizes"].shape)
    for name, cfg in BATCHES.items():
        data = eval_batch(base, cfg)
        out.update({f"{name}.{k}": v for k, v in data.items()})
        print(name, "image_sizes", data["image_sizes"].tolist(), "batch", data["tensors"].shape, "padded", int(data["mask"].sum()))
    data = train_batch(base)
    out.update({f"train.{k}": v for k, v in data.items()})
    print("train image_sizes", data["image_sizes"].tolist(), "batch", data["tensors"].shape)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
