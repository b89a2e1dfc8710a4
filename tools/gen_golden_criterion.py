"""Generate tests/golden/g10_criterion.npz by running the REFERENCE's own criterion (build machine only; no test runs this).

Run:  RELATION_DETR_REFERENCE=<checkout of the reference> python tools/gen_golden_criterion.py

Imported unmodified from the reference: ``models/bricks/set_criterion.py`` (HybridSetCriterion), ``models/bricks/losses.py``,
``models/matcher/hungarian_matcher.py`` and ``DNDETRDetector.compute_dn_loss`` / ``dn_post_process``
(``models/detectors/base_detector.py``).  Two stubs stand in for what is not installed: a ``torchvision.ops.boxes`` with
``box_iou``, ``generalized_box_iou`` and ``_box_cxcywh_to_xyxy`` written from their formulas, and a ``util.utils`` with
``get_world_size -> 1`` and ``is_dist_avail_and_initialized -> False``; every other name base_detector.py imports (image
transforms, ImageList) is an inert placeholder that the two methods never touch.  The flow around them is
``RelationDETR.forward`` (``models/detectors/relation_detr.py:100-141``).

The fixture holds data only: seeded predictions (L = 3, B = 2, C = 11, 24 matching + 6 denoising queries, 30 hybrid queries),
targets with 3 and 2 boxes, the reference's loss dict and the gradients of its sum with respect to the eight tensors, in fp32 and
fp64, every set's cost matrices, the assignments as query -> gt maps, and per (set, image) the MARGIN: how much the optimal
assignment cost rises once any one matched (query, gt) pair is forbidden in all of its column copies, on the fp64 matrix.  A
seed is accepted only if every margin is >= 1e-3: the match is then unique far beyond any fp32 cost error, and tests may compare
the maps exactly.
"""
import copy
import os
import sys
import types

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g10_criterion.npz")
L, B, C, NQ, GROUPS, MAX_GT, NH, ASSIGN = 3, 2, 11, 24, 1, 6, 30, 6
COUNTS = (3, 2)
MIN_MARGIN = 1e-3


# ------------------------------------------------------------------------------------------------------------------------ stubs
def _box_cxcywh_to_xyxy(boxes):
    cx, cy, w, h = boxes.unbind(-1)
    return torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)


def _inter_union(a, b):
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2])).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter, area_a[:, None] + area_b - inter


def box_iou(a, b):
    inter, union = _inter_union(a, b)
    return inter / union


def generalized_box_iou(a, b):
    inter, union = _inter_union(a, b)
    whi = (torch.max(a[:, None, 2:], b[:, 2:]) - torch.min(a[:, None, :2], b[:, :2])).clamp(min=0)
    areai = whi[:, :, 0] * whi[:, :, 1]
    return inter / union - (areai - union) / areai


class _PlaceholderMeta(type):
    def __getattr__(cls, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return cls


class _Placeholder(metaclass=_PlaceholderMeta):
    """Stands for any name the two imported methods never use."""

    def __init__(self, *args, **kwargs):
        pass


class _PlaceholderModule(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Placeholder


def import_reference():
    ref = os.environ.get("RELATION_DETR_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "models")):
        sys.exit("set RELATION_DETR_REFERENCE to a checkout of the reference")
    boxes = types.ModuleType("torchvision.ops.boxes")
    boxes.box_iou, boxes.generalized_box_iou, boxes._box_cxcywh_to_xyxy = box_iou, generalized_box_iou, _box_cxcywh_to_xyxy
    utils = types.ModuleType("util.utils")
    utils.get_world_size = lambda: 1
    utils.is_dist_avail_and_initialized = lambda: False
    for name in ("torchvision", "torchvision.ops", "torchvision.models", "torchvision.models.detection",
                 "torchvision.models.detection.image_list", "transforms", "transforms.functional", "transforms.v2", "util", "util.misc"):
        sys.modules[name] = _PlaceholderModule(name)
    sys.modules["torchvision.ops.boxes"] = sys.modules["torchvision.ops"].boxes = boxes
    sys.modules["util.utils"] = sys.modules["util"].utils = utils
    sys.path.insert(0, ref)
    from models.bricks.set_criterion import HybridSetCriterion
    from models.detectors.base_detector import DNDETRDetector
    from models.matcher.hungarian_matcher import HungarianMatcher
    return HybridSetCriterion, HungarianMatcher, DNDETRDetector


# ----------------------------------------------------------------------------------------------------------------------- inputs
def make_inputs(seed):
    g = torch.Generator().manual_seed(seed)

    def logits(*shape):
        return (2 * torch.randn(*shape, C, generator=g)).clamp(-6, 6)

    def boxes(*shape):
        return torch.cat((torch.rand(*shape, 2, generator=g), 0.02 + 0.4 * torch.rand(*shape, 2, generator=g)), dim=-1)

    n = GROUPS * MAX_GT + NQ
    outputs = [logits(L, B, n), boxes(L, B, n), logits(B, NQ), boxes(B, NQ), logits(L, B, NH), boxes(L, B, NH), logits(B, NH),
               boxes(B, NH)]
    targets = [{"labels": torch.randint(0, C, (k,), generator=g), "boxes": boxes(k)} for k in COUNTS]
    return outputs, targets


def weight_dict():
    w = {"loss_class": 1, "loss_bbox": 5, "loss_giou": 2}
    w.update({"loss_class_dn": 1, "loss_bbox_dn": 5, "loss_giou_dn": 2})
    w.update({k + f"_{i}": v for i in range(L - 1) for k, v in list(w.items())})
    w.update({"loss_class_enc": 1, "loss_bbox_enc": 5, "loss_giou_enc": 2})
    w.update({k + "_hybrid": v for k, v in list(w.items())})
    return w


def aux(classes, coords):
    return [{"pred_logits": a, "pred_boxes": b} for a, b in zip(classes[:-1], coords[:-1])]


def reference_losses(ref, outputs, targets, dtype):
    """relation_detr.py:100-141 on the given outputs -> (loss dict, gradients of the dict's sum with respect to the eight)."""
    HybridSetCriterion, HungarianMatcher, DNDETRDetector = ref
    matcher = HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2, focal_alpha=0.25, focal_gamma=2.0)
    criterion = HybridSetCriterion(num_classes=C, matcher=matcher, weight_dict=weight_dict(), alpha=0.25, gamma=2.0)
    detector = types.SimpleNamespace(criterion=criterion, device=torch.device("cpu"))
    detector._set_aux_loss = aux
    outs = [t.detach().to(dtype).clone().requires_grad_(True) for t in outputs]
    targets = [{"labels": t["labels"], "boxes": t["boxes"].to(dtype)} for t in targets]
    cls, box, enc_cls, enc_box, hyb_cls, hyb_box, hyb_enc_cls, hyb_enc_box = outs
    dn_metas = {"denoising_groups": GROUPS, "max_gt_num_per_image": MAX_GT}
    cls, box = DNDETRDetector.dn_post_process(detector, cls, box, dn_metas)
    output = {"pred_logits": cls[-1], "pred_boxes": box[-1], "aux_outputs": aux(cls, box),
              "enc_outputs": {"pred_logits": enc_cls, "pred_boxes": enc_box}}
    hybrid = {"pred_logits": hyb_cls[-1], "pred_boxes": hyb_box[-1], "aux_outputs": aux(hyb_cls, hyb_box),
              "enc_outputs": {"pred_logits": hyb_enc_cls, "pred_boxes": hyb_enc_box}}
    loss_dict = criterion(output, targets)
    loss_dict.update(DNDETRDetector.compute_dn_loss(detector, dn_metas, targets))
    multi = copy.deepcopy(targets)
    for t in multi:
        t["boxes"] = t["boxes"].repeat(ASSIGN, 1)
        t["labels"] = t["labels"].repeat(ASSIGN)
    loss_dict.update({k + "_hybrid": v for k, v in criterion(hybrid, multi).items()})
    w = criterion.weight_dict
    loss_dict = {k: loss_dict[k] * w[k] for k in loss_dict if k in w}
    torch.stack(list(loss_dict.values())).sum().backward()
    return loss_dict, [t.grad for t in outs], matcher


def matched_sets(outputs):
    """(name, logits [B, N, C], boxes [B, N, 4], target copies) of the 14 matched sets."""
    n_dn = GROUPS * MAX_GT
    sets = [(f"dec{l}", outputs[0][l, :, n_dn:], outputs[1][l, :, n_dn:], 1) for l in range(L)]
    sets.append(("enc", outputs[2], outputs[3], 1))
    sets += [(f"hyb{l}", outputs[4][l], outputs[5][l], ASSIGN) for l in range(L)]
    sets.append(("hyb_enc", outputs[6], outputs[7], ASSIGN))
    return sets


def query_map(n, src, tgt, g):
    m = np.full(n, -1, dtype=np.int32)
    m[np.asarray(src)] = np.asarray(tgt) % g
    return m


def margin(cost, copies):
    """Optimal cost of the tiled matrix, and by how much it rises at least when one matched pair is forbidden in all its copies."""
    g = cost.shape[1]
    tiled = np.tile(cost, (1, copies))
    src, tgt = linear_sum_assignment(tiled)
    best = tiled[src, tgt].sum()
    rise = np.inf
    for q, t in zip(src, tgt):
        blocked = tiled.copy()
        blocked[q, (t % g)::g] = 1e6
        s2, t2 = linear_sum_assignment(blocked)
        rise = min(rise, blocked[s2, t2].sum() - best)
    return rise


def generate(ref, seed):
    outputs, targets = make_inputs(seed)
    data = {f"out.{i}": t.numpy() for i, t in enumerate(outputs)}
    for b, t in enumerate(targets):
        data[f"tgt.labels.{b}"] = t["labels"].numpy()
        data[f"tgt.boxes.{b}"] = t["boxes"].numpy()
    data["dn_meta"] = np.array([GROUPS, MAX_GT], dtype=np.int64)
    data["hybrid_assign"] = np.array(ASSIGN, dtype=np.int64)
    data["seed"] = np.array(seed, dtype=np.int64)
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        losses, grads, matcher = reference_losses(ref, outputs, targets, dtype)
        for k, v in losses.items():
            data[f"loss{tag}.{k}"] = v.detach().numpy()
        for i, gr in enumerate(grads):
            data[f"grad{tag}.{i}"] = gr.numpy()
        for name, logits, boxes, copies in matched_sets([t.to(dtype) for t in outputs]):
            for b, t in enumerate(targets):
                cost = matcher.calculate_cost(boxes[b], logits[b], t["boxes"].to(dtype), t["labels"])
                data[f"cost{tag}.{name}.{b}"] = cost.numpy()
                src, tgt = matcher(boxes[b], logits[b], t["boxes"].to(dtype).repeat(copies, 1), t["labels"].repeat(copies))
                qmap = query_map(logits.shape[1], src, tgt, COUNTS[b])
                if tag == "32":
                    data[f"match.{name}.{b}"] = qmap
                else:
                    if not np.array_equal(qmap, data[f"match.{name}.{b}"]):
                        return None
                    data[f"margin.{name}.{b}"] = np.array(margin(cost.numpy(), copies))
                    if data[f"margin.{name}.{b}"] < MIN_MARGIN:
                        return None
    return data


def main():
    ref = import_reference()
    for seed in range(100):
        data = generate(ref, seed)
        if data is not None:
            break
        print("seed", seed, "rejected: a margin below", MIN_MARGIN)
    else:
        sys.exit("no seed gave unique matches")
    np.savez_compressed(OUT, **data)
    margins = [float(v) for k, v in data.items() if k.startswith("margin.")]
    print(f"wrote {OUT}: seed {seed}, {sum(k.startswith('loss32.') for k in data)} losses, smallest margin {min(margins):.3e}, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
