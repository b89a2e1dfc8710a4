"""Generate tests/golden/g15_augment.npz by running the REFERENCE's own transform code (build machine only; no test runs this).

Run:  RELATION_DETR_REFERENCE=<checkout of the reference> python tools/gen_golden_augment.py

torchvision and PIL are not needed: the reference's ``transforms/v2`` package imports both at every level, so its modules are not
imported.  Instead the SOURCE of the functions and methods that do the work is taken from the reference's files (as
tools/gen_golden_preprocess.py takes ``image_list_from_tensors``) and executed unmodified in a namespace of stand-ins.

Run unmodified from the reference (the transform CLASSES did not run, only these pieces of them):
  transforms/v2/_geometry.py              ``RandomShortestSize.__init__`` and ``._get_params``: every size of this fixture
  transforms/crop.py                      ``RandomSizeCrop.__init__`` and ``._get_params``: every crop (``random`` and ``torch`` seeded here)
  transforms/v2/functional/_geometry.py   ``horizontal_flip_image_tensor``, ``horizontal_flip_bounding_box``, ``_compute_resized_output_size``,
                                          ``resize_image_tensor``, ``resize_bounding_box``, ``crop_image_tensor``, ``crop_bounding_box``
  transforms/v2/functional/_meta.py       ``_clamp_bounding_box``
  transforms/v2/_misc.py                  ``SanitizeBoundingBox.forward``: its statements from ``ws, hs = ...`` to the last ``valid &= ...``
Stand-ins (tests/golden/g15_augment.md names them too):
  datapoints.BoundingBoxFormat            an enum with XYXY, XYWH, CXCYWH; every box here is XYXY
  InterpolationMode                       an enum with BILINEAR = "bilinear", BICUBIC, NEAREST; ``_check_interpolation`` returns its argument,
                                          ``_check_antialias`` returns ``antialias``
  __compute_resized_output_size           torchvision's rule for a size of two numbers: the size itself
  convert_format_bounding_box             XYXY -> XYXY: the tensor itself;  clamp_bounding_box -> the reference's ``_clamp_bounding_box``
  query_spatial_size                      the (h, w) of the one image in the flat inputs
  the flip and the branch                 set per case, not drawn (``RandomHorizontalFlip`` / ``RandomChoice`` did not run); the scales are
                                          drawn here and handed to ``RandomShortestSize`` as one-element lists
  the boxes handed to ``SanitizeBoundingBox``'s statements are a tensor subclass that carries ``spatial_size``

The preset is ``presets.detr`` scaled down: scales 48 .. 80 step 8, max_size 133, crop resize (40, 50, 60), crop range (38, 60).

For every crop case the source is redrawn until the float64 filter of tests/test_images_host.py finds no near tie in the crop of the
first resize (a redraw keeps the image and moves, per near tie, the source pixel under the tap centre by 1 to 3: exact x.5 sums are
too common for fresh noise to avoid); the second stage may have near ties within that file's 2 % cap.  Both are asserted here and the counts printed.

Keys (data only):
  sizes                 [N, 6] int64: h, w, min_size, max_size (-1: none), oh, ow from ``RandomShortestSize._get_params``
  preset                scales..., and preset.max_size, preset.crop_resize, preset.crop_range
  c<i>.choice           [8] int64: flip, crop branch, min_size, first min_size, crop h, crop w, top, left (-1 where unused)
  c<i>.src, .boxes, .labels            the uint8 image [3, h, w], xyxy fp32 boxes, int64 labels
  c<i>.first, .final    the sizes ``_get_params`` returned (first: crop cases)
  c<i>.mid              crop cases: the uint8 crop of the first resize
  c<i>.out              the uint8 image in front of ``ConvertImageDtype``
  c<i>.boxes_out, .labels_out, .valid  after the sanitising statements, and their mask
  c<i>.near             [2] int64: near ties in the crop of the first resize (0) and in the last resize
  batch.cases           the cases that form the mixed batch
"""
import ast
import enum
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "g15_augment.npz")
SCALES, MAX_SIZE, CROP_RESIZE, CROP_RANGE = (48, 56, 64, 72, 80), 133, (40, 50, 60), (38, 60)
# (flip, crop branch, (h, w), boxes)
CASES = [(0, 0, (70, 100), 4), (1, 0, (83, 111), 5), (0, 1, (77, 104), 6), (1, 1, (95, 130), 6),
         (0, 0, (90, 71), 3), (1, 0, (72, 127), 0), (0, 1, (101, 74), 7), (1, 1, (74, 99), 5)]
BATCH = [1, 2, 4, 7]


class BoundingBoxFormat(enum.Enum):
    XYXY, XYWH, CXCYWH = "XYXY", "XYWH", "CXCYWH"


class InterpolationMode(enum.Enum):
    NEAREST, BILINEAR, BICUBIC = "nearest", "bilinear", "bicubic"


class Boxes(torch.Tensor):
    """What ``SanitizeBoundingBox.forward`` reads of a ``datapoints.BoundingBox``: the values and ``spatial_size``."""


def _definitions(path, wanted):
    """{name: ast node} of the module-level functions, and "Class.method" of the methods, that ``wanted`` names."""
    with open(path) as f:
        tree = ast.parse(f.read())
    found = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in wanted:
            found[node.name] = node
        elif isinstance(node, ast.ClassDef):
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and f"{node.name}.{sub.name}" in wanted:
                    found[f"{node.name}.{sub.name}"] = sub
    missing = set(wanted) - set(found)
    assert not missing, (path, missing)
    return found


def _run(nodes, namespace, filename):
    exec(compile(ast.fix_missing_locations(ast.Module(list(nodes), [])), filename, "exec"), namespace)


def import_reference():
    ref = os.environ.get("RELATION_DETR_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "transforms", "v2")):
        sys.exit("set RELATION_DETR_REFERENCE to a checkout of the reference")
    import typing
    from torch.nn.functional import interpolate
    datapoints = types.SimpleNamespace(BoundingBoxFormat=BoundingBoxFormat)
    ns = dict(vars(typing))
    ns.update(torch=torch, random=random, datapoints=datapoints, BoundingBoxFormat=BoundingBoxFormat, InterpolationMode=InterpolationMode,
              interpolate=interpolate, _check_interpolation=lambda interpolation: interpolation,
              _check_antialias=lambda img, antialias, interpolation: antialias,
              __compute_resized_output_size=lambda spatial_size, size, max_size=None: [int(size[0]), int(size[1])],
              convert_format_bounding_box=_same_format, query_spatial_size=lambda flat_inputs: tuple(flat_inputs[0].shape[-2:]))
    ns["__builtins__"] = __builtins__
    functional = os.path.join(ref, "transforms", "v2", "functional", "_geometry.py")
    names = ["horizontal_flip_image_tensor", "horizontal_flip_bounding_box", "_compute_resized_output_size", "resize_image_tensor",
             "resize_bounding_box", "crop_image_tensor", "crop_bounding_box"]
    _run(_definitions(functional, names).values(), ns, functional)
    meta = os.path.join(ref, "transforms", "v2", "functional", "_meta.py")
    _run(_definitions(meta, ["_clamp_bounding_box"]).values(), ns, meta)
    ns["clamp_bounding_box"] = lambda inpt, format=None, spatial_size=None: ns["_clamp_bounding_box"](inpt, format, spatial_size)

    class Transform:                                     # what the two __init__ call through super()
        def __init__(self):
            pass
    for path, cls in ((os.path.join(ref, "transforms", "v2", "_geometry.py"), "RandomShortestSize"),
                      (os.path.join(ref, "transforms", "crop.py"), "RandomSizeCrop")):
        methods = _definitions(path, [f"{cls}.__init__", f"{cls}._get_params"])
        body = ast.ClassDef(name=cls, bases=[ast.Name("Transform", ast.Load())], keywords=[], body=list(methods.values()), decorator_list=[])
        ns["Transform"] = Transform
        _run([body], ns, path)
    misc = os.path.join(ref, "transforms", "v2", "_misc.py")
    forward = _definitions(misc, ["SanitizeBoundingBox.forward"])["SanitizeBoundingBox.forward"]
    text = [ast.unparse(s).lstrip("(") for s in forward.body]
    first = [i for i, t in enumerate(text) if t.startswith("ws, hs")][0]
    last = [i for i, t in enumerate(text) if t.startswith("valid &=")][-1]
    assert last - first == 4, text[first:last + 1]
    statements = forward.body[first:last + 1]

    def sanitize(boxes, spatial_size, min_size=1):
        b = boxes.as_subclass(Boxes)
        b.spatial_size = spatial_size
        scope = dict(ns, boxes=b, self=types.SimpleNamespace(min_size=min_size))
        _run(statements, scope, misc)
        return scope["valid"].as_subclass(torch.Tensor)
    ns["sanitize"] = sanitize
    return types.SimpleNamespace(**{k: v for k, v in ns.items() if not k.startswith("__")})


def _same_format(inpt, old_format=None, new_format=None, inplace=False):
    assert old_format == new_format == BoundingBoxFormat.XYXY
    return inpt


def size_table(ref):
    rows = []
    coco = [(480, 640), (427, 640), (640, 480), (375, 500), (500, 375), (333, 500), (640, 427), (612, 612), (428, 640), (640, 640),
            (360, 640), (480, 360), (1080, 1920), (600, 1000), (1200, 800), (51, 640), (640, 59), (3, 1000)]
    cases = [(h, w, s, 1333) for h, w in coco for s in (480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800)]
    cases += [(h, w, s, None) for h, w in coco[:10] for s in (400, 500, 600)]
    cases += [(h, w, s, 2000) for h, w in coco[:6] for s in (720, 960, 1200)]
    cases += [(h, w, s, MAX_SIZE) for h in range(61, 110, 7) for w in range(67, 140, 9) for s in SCALES[::2]]
    cases += [(h, w, s, None) for h in range(61, 110, 11) for w in range(67, 140, 13) for s in CROP_RESIZE]
    for h, w, s, m in cases:
        size = ref.RandomShortestSize(min_size=[s], max_size=m, antialias=True)._get_params([torch.empty(3, h, w, dtype=torch.uint8)])["size"]
        rows.append((h, w, s, -1 if m is None else m, size[0], size[1]))
    return np.array(rows, dtype=np.int64)


def near_ties(src, size):
    """(count, share) of near-tie values of the uint8 resize ``src -> size`` by the rule of tests/test_images_host.py, and the mask."""
    from test_images_host import interpolate_error, near_tie, resize64
    v64 = resize64(src, *size)
    _, near = near_tie(v64, interpolate_error(src, v64))
    return near


def one_case(ref, g, flip, crop, hw, n_boxes):
    from test_images_host import NEAR_TIE_SHARE
    h, w = hw
    xy = torch.rand(n_boxes, 2, generator=g) * torch.tensor([w * 0.8, h * 0.8])
    wh = torch.rand(n_boxes, 2, generator=g) * torch.tensor([w * 0.5, h * 0.5])
    if n_boxes:
        wh[0] = torch.tensor([0.9, 0.7])                # a box the last resize leaves below one pixel in height or width
    boxes = torch.cat((xy, torch.minimum(xy + wh + 0.4, torch.tensor([float(w), float(h)]))), dim=-1)
    labels = torch.randint(0, 11, (n_boxes,), generator=g)
    min_size = SCALES[int(torch.randint(len(SCALES), (), generator=g))]
    first_min = CROP_RESIZE[int(torch.randint(len(CROP_RESIZE), (), generator=g))] if crop else -1
    fmt = BoundingBoxFormat.XYXY
    pending = None
    for attempt in range(400):
        src = torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g) if pending is None else pending.contiguous()
        state = (random.getstate(), torch.get_rng_state())
        data = {"src": src.numpy(), "boxes": boxes.numpy().reshape(-1, 4), "labels": labels.numpy()}
        image, bxs, size = src, boxes.clone(), (h, w)
        choice = [flip, crop, min_size, first_min, -1, -1, -1, -1]
        near = [0, 0]
        if flip:
            image, bxs = ref.horizontal_flip_image_tensor(image), ref.horizontal_flip_bounding_box(bxs, fmt, size)
        if crop:
            first = ref.RandomShortestSize([first_min], antialias=True)._get_params([image])["size"]
            resized = ref.resize_image_tensor(image, list(first), InterpolationMode.BILINEAR, antialias=True)
            bxs, size = ref.resize_bounding_box(bxs, size, list(first))
            params = ref.RandomSizeCrop(*CROP_RANGE)._get_params([resized])
            window = (slice(None), slice(params["top"], params["top"] + params["height"]), slice(params["left"], params["left"] + params["width"]))
            ties = near_ties(image.numpy(), first)[window]
            near[0] = int(ties.sum())
            if near[0]:
                # Random sources do not get there: exact x.5 sums are common (the weights are small rationals), about 0.6 % of the
                # values.  So the next source is this one with, per near tie, the source pixel under the tap centre moved a little.
                from test_images_host import filter_matrix
                rows = filter_matrix(image.shape[1], first[0]).argmax(1)[params["top"]:params["top"] + params["height"]]
                cols = filter_matrix(image.shape[2], first[1]).argmax(1)[params["left"]:params["left"] + params["width"]]
                moved = image.clone()
                for c, y, x in zip(*np.nonzero(ties)):
                    step = int(torch.randint(1, 4, (), generator=g)) * (1 if int(moved[c, rows[y], cols[x]]) < 128 else -1)
                    moved[c, rows[y], cols[x]] += step
                pending = moved.flip(-1) if flip else moved
                random.setstate(state[0])               # the same crop for the next source
                torch.set_rng_state(state[1])
                continue
            image = ref.crop_image_tensor(resized, **params)
            bxs, size = ref.crop_bounding_box(bxs, fmt, **params)
            choice[4:] = [params["height"], params["width"], params["top"], params["left"]]
            data["first"], data["mid"] = np.array(first, dtype=np.int64), image.numpy().copy()
        final = ref.RandomShortestSize([min_size], max_size=MAX_SIZE, antialias=True)._get_params([image])["size"]
        last_near = near_ties(np.ascontiguousarray(image.numpy()), final)
        near[1] = int(last_near.sum())
        assert near[1] <= NEAR_TIE_SHARE * last_near.size, (near, last_near.size)
        out = ref.resize_image_tensor(image.contiguous(), list(final), InterpolationMode.BILINEAR, antialias=True)
        bxs, size = ref.resize_bounding_box(bxs, size, list(final))
        valid = ref.sanitize(bxs, size)
        assert out.dtype == torch.uint8 and tuple(out.shape[-2:]) == tuple(final) == tuple(size)
        data.update(choice=np.array(choice, dtype=np.int64), final=np.array(final, dtype=np.int64), out=out.numpy(),
                    valid=valid.numpy(), boxes_out=bxs[valid].numpy().reshape(-1, 4), labels_out=labels[valid].numpy(),
                    near=np.array(near, dtype=np.int64), boxes_moved=bxs.numpy().reshape(-1, 4))
        return data, attempt + 1, last_near.size
    raise AssertionError("no source without a near tie in the first resize")


def main():
    ref = import_reference()
    random.seed(15)
    torch.manual_seed(15)
    g = torch.Generator().manual_seed(15)
    out = {"sizes": size_table(ref), "preset.scales": np.array(SCALES), "preset.max_size": np.array(MAX_SIZE),
           "preset.crop_resize": np.array(CROP_RESIZE), "preset.crop_range": np.array(CROP_RANGE), "batch.cases": np.array(BATCH)}
    print("size table", out["sizes"].shape)
    for i, (flip, crop, hw, n_boxes) in enumerate(CASES):
        data, draws, n_last = one_case(ref, g, flip, crop, hw, n_boxes)
        out.update({f"c{i}.{k}": v for k, v in data.items()})
        print(f"c{i}: flip {flip} crop {crop} source {hw} choice {data['choice'].tolist()} final {data['final'].tolist()} "
              f"boxes {n_boxes} -> {len(data['boxes_out'])}; sources drawn {draws}; near ties: first resize {int(data['near'][0])}, "
              f"last resize {int(data['near'][1])} of {n_last}")
    assert any(len(out[f"c{i}.boxes_out"]) < len(out[f"c{i}.boxes"]) for i in range(len(CASES))), "no case drops a box"
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
