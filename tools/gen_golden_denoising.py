"""Generate tests/golden/g11_denoising.npz by running the REFERENCE's own GenerateCDNQueries (build machine only; no test runs this).

Run:  RELATION_DETR_REFERENCE=<checkout of the reference> python tools/gen_golden_denoising.py

Imported unmodified from the reference: ``models/bricks/denoising.py``.  Two stubs stand in for what is not installed: a
``torchvision.ops.boxes`` with ``_box_cxcywh_to_xyxy`` and ``_box_xyxy_to_cxcywh`` written from their formulas, and a ``util.misc``
holding only the reference's ``inverse_sigmoid``, taken from its file as oracle/gen_golden.py does.

What is recorded besides the results: the four random draws, by wrapping ``torch.rand_like`` and ``torch.randint_like`` for the
duration of the call (the generator consumes exactly label_u, label_r, box_sign, box_u, in this order; a switched-off noise
consumes none), and the noised labels, by a forward pre-hook on ``label_encoder``.  The fixture holds data only.

Cases (C = 11, d = 256, 24 matching queries), keys ``<case>.<name>``:
  a  counts [3, 0, 5], denoising_nums 12 (groups 2, Ndn 20); also the label queries and the embedding weight
  b  counts [1], denoising_nums 10
  c  counts [130, 7], denoising_nums 100, label_noise_prob 0.6
  d  the targets of a, both noises off
  e  counts [0, 0]
"""
import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g11_denoising.npz")
C, D, NQ = 11, 256, 24
CASES = {
    "a": dict(counts=(3, 0, 5), denoising_nums=12, label_noise_prob=0.5, box_noise_scale=1.0, seed=1),
    "b": dict(counts=(1,), denoising_nums=10, label_noise_prob=0.5, box_noise_scale=1.0, seed=2),
    "c": dict(counts=(130, 7), denoising_nums=100, label_noise_prob=0.6, box_noise_scale=1.0, seed=3),
    "d": dict(counts=(3, 0, 5), denoising_nums=12, label_noise_prob=0.0, box_noise_scale=0.0, seed=1),
    "e": dict(counts=(0, 0), denoising_nums=100, label_noise_prob=0.5, box_noise_scale=1.0, seed=5),
}


def _box_cxcywh_to_xyxy(boxes):
    cx, cy, w, h = boxes.unbind(-1)
    return torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)


def _box_xyxy_to_cxcywh(boxes):
    x1, y1, x2, y2 = boxes.unbind(-1)
    return torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), dim=-1)


def import_reference():
    ref = os.environ.get("RELATION_DETR_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "models")):
        sys.exit("set RELATION_DETR_REFERENCE to a checkout of the reference")
    boxes = types.ModuleType("torchvision.ops.boxes")
    boxes._box_cxcywh_to_xyxy, boxes._box_xyxy_to_cxcywh = _box_cxcywh_to_xyxy, _box_xyxy_to_cxcywh
    tv, ops = types.ModuleType("torchvision"), types.ModuleType("torchvision.ops")
    tv.ops, ops.boxes = ops, boxes
    sys.modules["torchvision"], sys.modules["torchvision.ops"], sys.modules["torchvision.ops.boxes"] = tv, ops, boxes
    tree = ast.parse(open(os.path.join(ref, "util/misc.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "inverse_sigmoid"][0]
    misc = types.ModuleType("util.misc")
    misc.torch = torch
    exec(compile(ast.Module([fn], []), "util/misc.py", "exec"), misc.__dict__)
    util = types.ModuleType("util")
    util.__path__ = []
    util.misc = misc
    sys.modules["util"], sys.modules["util.misc"] = util, misc
    for name in ("models", "models.bricks"):                                    # the packages' own __init__ import far more
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(ref, *name.split("."))]
        sys.modules[name] = pkg
    from models.bricks.denoising import GenerateCDNQueries
    return GenerateCDNQueries


def make_targets(counts, seed):
    g = torch.Generator().manual_seed(seed)
    labels = [torch.randint(0, C, (k,), generator=g) for k in counts]
    boxes = [torch.cat((0.05 + 0.9 * torch.rand(k, 2, generator=g), 0.02 + 0.5 * torch.rand(k, 2, generator=g)), dim=-1) for k in counts]
    return labels, boxes


class RecordDraws:
    """Wraps torch.rand_like / torch.randint_like while active and keeps what they returned, in call order."""

    def __enter__(self):
        self.draws, self._rand, self._randint = [], torch.rand_like, torch.randint_like

        def rand_like(*a, **kw):
            self.draws.append(("rand", self._rand(*a, **kw)))
            return self.draws[-1][1].clone()

        def randint_like(*a, **kw):
            self.draws.append(("randint", self._randint(*a, **kw)))
            return self.draws[-1][1].clone()

        torch.rand_like, torch.randint_like = rand_like, randint_like
        return self

    def __exit__(self, *exc):
        torch.rand_like, torch.randint_like = self._rand, self._randint


def run_case(cls, weight, cfg):
    labels, boxes = make_targets(cfg["counts"], cfg["seed"])
    module = cls(num_queries=NQ, num_classes=C, label_embed_dim=D, denoising_nums=cfg["denoising_nums"],
                 label_noise_prob=cfg["label_noise_prob"], box_noise_scale=cfg["box_noise_scale"])
    with torch.no_grad():
        module.label_encoder.weight.copy_(weight)
    seen = []
    module.label_encoder.register_forward_pre_hook(lambda _, args: seen.append(args[0].detach().clone()))
    torch.manual_seed(100 + cfg["seed"])
    with RecordDraws() as rec, torch.no_grad():
        label_query, box_query, mask, groups, group_size = module(labels, [b.clone() for b in boxes])
    kinds = [k for k, _ in rec.draws]
    want = (["rand", "randint"] if cfg["label_noise_prob"] > 0 else []) + (["randint", "rand"] if cfg["box_noise_scale"] > 0 else [])
    assert kinds == want, (kinds, want)
    assert len(seen) == 1
    G = sum(cfg["counts"])
    Q = 2 * groups * G
    draws = [t for _, t in rec.draws]
    data = {"counts": np.array(cfg["counts"], dtype=np.int64),
            "settings": np.array([cfg["denoising_nums"], cfg["label_noise_prob"], cfg["box_noise_scale"]], dtype=np.float64),
            "meta": np.array([groups, group_size], dtype=np.int64),
            "gt_labels": torch.cat(labels).numpy(), "gt_boxes": torch.cat(boxes).numpy().reshape(G, 4),
            "noised_labels": seen[0].numpy(), "box_query": box_query.numpy(), "mask": mask.numpy()}
    if cfg["label_noise_prob"] > 0:
        data["label_u"], data["label_r"] = draws[0].numpy(), draws[1].numpy()
        assert data["label_u"].shape == (Q,) and data["label_r"].dtype == np.int64
        draws = draws[2:]
    if cfg["box_noise_scale"] > 0:
        data["box_sign"], data["box_u"] = draws[0].numpy(), draws[1].numpy()
        assert data["box_sign"].shape == (Q, 4) and data["box_sign"].dtype == np.float32
    return data, label_query.numpy()


def main():
    cls = import_reference()
    weight = torch.randn(C, D, generator=torch.Generator().manual_seed(0))
    out = {"embed": weight.numpy()}
    for name, cfg in CASES.items():
        data, label_query = run_case(cls, weight, cfg)
        if name == "a":
            data["label_query"] = label_query
        out.update({f"{name}.{k}": v for k, v in data.items()})
        print(name, "counts", cfg["counts"], "groups", int(data["meta"][0]), "Ndn", data["box_query"].shape[1], "mask True",
              int(data["mask"].sum()))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
