"""CPU checks of the training criterion (relation_detr_amd/criterion.py): its torch route against the reference's recorded loss
dict, gradients, cost matrices and assignments (tests/golden/g10_criterion.npz, tools/gen_golden_criterion.py), the structural
cases (empty images, more target copies than queries, no denoising queries, no hybrid branch, one decoder layer), and the new C
entries declared once, bound and exported with the ABI version and the Options fields unchanged."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import relation_detr_amd
from conftest import load_golden
from relation_detr_amd import _lib, criterion as crit, options
from relation_detr_amd.criterion import RelationCriterion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
SYMBOLS = ("rdetr_match_cost_f32", "rdetr_match_cost_bf16", "rdetr_set_loss_f32", "rdetr_set_loss_bf16", "rdetr_set_loss_workspace_bytes")
SETS = [f"dec{l}" for l in range(3)] + ["enc"] + [f"hyb{l}" for l in range(3)] + ["hyb_enc"]


@pytest.fixture(scope="module")
def g10():
    return load_golden("g10_criterion.npz")


def fixture_inputs(z, dtype):
    outputs = [torch.from_numpy(z[f"out.{i}"]).to(dtype).requires_grad_(True) for i in range(8)]
    targets = [{"labels": torch.from_numpy(z[f"tgt.labels.{b}"]), "boxes": torch.from_numpy(z[f"tgt.boxes.{b}"]).to(dtype)} for b in range(2)]
    return outputs, targets, tuple(int(v) for v in z["dn_meta"])


def run(outputs, targets, dn_meta, **kw):
    losses = RelationCriterion(outputs[0].shape[-1], fused=False, **kw)(tuple(outputs), targets, dn_meta)
    torch.stack(list(losses.values())).sum().backward()
    return losses, [t.grad for t in outputs if t is not None]


def set_tensors(outputs, name, n_dn=6):
    l = int(name[3]) if name[3:].isdigit() else None
    if name.startswith("dec"):
        return outputs[0][l, :, n_dn:], outputs[1][l, :, n_dn:]
    if name == "enc":
        return outputs[2], outputs[3]
    if name == "hyb_enc":
        return outputs[6], outputs[7]
    return outputs[4][l], outputs[5][l]


def test_fp64_route_matches_the_reference(g10):
    outputs, targets, dn_meta = fixture_inputs(g10, torch.float64)
    losses, grads = run(outputs, targets, dn_meta)
    want = {k[len("loss64."):]: v for k, v in g10.items() if k.startswith("loss64.")}
    assert set(losses) == set(want) and len(want) == 33
    for k, v in want.items():
        assert abs(losses[k].item() - float(v)) <= 1e-9 * abs(float(v)), k
    for i, g in enumerate(grads):
        ref = torch.from_numpy(g10[f"grad64.{i}"])
        assert (g - ref).abs().max() <= 1e-9 * ref.abs().max(), i


def test_fp32_route_matches_the_reference(g10):
    outputs, targets, dn_meta = fixture_inputs(g10, torch.float32)
    losses, grads = run(outputs, targets, dn_meta)
    want = {k[len("loss32."):]: v for k, v in g10.items() if k.startswith("loss32.")}
    assert set(losses) == set(want)
    for k, v in want.items():
        assert losses[k].dtype == torch.float32
        assert abs(losses[k].item() - float(v)) <= 16 * ULP32 * max(1.0, abs(float(v))), k
    for i, g in enumerate(grads):
        ref = torch.from_numpy(g10[f"grad32.{i}"])
        assert ((g - ref).abs() <= 16 * ULP32 * ref.abs().clamp(min=1.0)).all(), i


@pytest.mark.parametrize("tag,dtype,rel", [("64", torch.float64, 1e-9), ("32", torch.float32, 16 * ULP32)])
def test_costs_and_maps_match_the_reference(g10, tag, dtype, rel):
    outputs, targets, _ = fixture_inputs(g10, dtype)
    counts = [3, 2]
    gt_boxes = torch.zeros(2, 3, 4, dtype=dtype)
    gt_labels = torch.zeros(2, 3, dtype=torch.int32)
    for b, t in enumerate(targets):
        gt_boxes[b, :counts[b]], gt_labels[b, :counts[b]] = t["boxes"], t["labels"].int()
    with torch.no_grad():
        for name in SETS:
            logits, boxes = set_tensors(outputs, name)
            cost = crit.match_cost(logits, boxes, gt_boxes, gt_labels, torch.tensor(counts, dtype=torch.int32), fused=False)
            assert cost.dtype == dtype and tuple(cost.shape) == (2, logits.shape[1], 3)
            pairs = crit.hungarian_match(cost, counts, repeat=6 if name.startswith("hyb") else 1)
            for b in range(2):
                ref = torch.from_numpy(g10[f"cost{tag}.{name}.{b}"])
                assert ((cost[b, :, :counts[b]] - ref).abs() <= rel * ref.abs().clamp(min=1.0)).all(), (name, b)
                assert (cost[b, :, counts[b]:] == 0).all()
                src, tgt = pairs[b]
                assert src.dtype == tgt.dtype == torch.int64 and (tgt < counts[b]).all()
                qmap = np.full(logits.shape[1], -1, dtype=np.int32)
                qmap[src.numpy()] = tgt.numpy()
                assert np.array_equal(qmap, g10[f"match.{name}.{b}"]), (name, b)
                assert float(g10[f"margin.{name}.{b}"]) >= 1e-3


def test_set_loss_on_the_match_table_agrees_with_the_per_set_route(g10):
    """`set_loss` (the whole stack at once, the checker of the kernel) against the loss dict of the reference-shaped loops."""
    outputs, targets, dn_meta = fixture_inputs(g10, torch.float64)
    losses, _ = run(outputs, targets, dn_meta)
    gt_boxes = torch.zeros(2, 3, 4, dtype=torch.float64)
    gt_labels = torch.zeros(2, 3, dtype=torch.int32)
    for b, t in enumerate(targets):
        gt_boxes[b, :len(t["labels"])], gt_labels[b, :len(t["labels"])] = t["boxes"], t["labels"].int()
    match = torch.full((3, 2, 30), -1, dtype=torch.int32)
    for l in range(3):
        for b, g in enumerate((3, 2)):
            match[l, b, :g] = torch.arange(g, dtype=torch.int32)
            match[l, b, 6:] = torch.from_numpy(g10[f"match.dec{l}.{b}"])
    sums = crit.set_loss(outputs[0].flatten(0, 1), outputs[1].flatten(0, 1), match.flatten(0, 1), gt_boxes, gt_labels, 6, 1 / 5.0, 1 / 5.0,
                         fused=False).view(3, 2, 2, 3).sum(1)
    for l, suffix in enumerate(("_0", "_1", "")):
        for i, (name, w) in enumerate((("loss_class", 1.0), ("loss_bbox", 5.0), ("loss_giou", 2.0))):
            assert abs(sums[l, 1, i].item() * w - losses[name + suffix].item()) <= 1e-12 * max(1.0, losses[name + suffix].item())
            assert abs(sums[l, 0, i].item() * w - losses[name + "_dn" + suffix].item()) <= 1e-12 * max(1.0, losses[name + "_dn" + suffix].item())


def random_outputs(L=2, B=2, C=5, nq=8, n_dn=0, nh=10, seed=1, dtype=torch.float64, hybrid=True):
    g = torch.Generator().manual_seed(seed)
    logits = lambda *s: (2 * torch.randn(*s, C, generator=g, dtype=dtype)).requires_grad_(True)
    boxes = lambda *s: torch.cat((torch.rand(*s, 2, generator=g, dtype=dtype), 0.02 + 0.4 * torch.rand(*s, 2, generator=g, dtype=dtype)),
                                 -1).requires_grad_(True)
    outs = [logits(L, B, n_dn + nq), boxes(L, B, n_dn + nq), logits(B, nq), boxes(B, nq)]
    outs += [logits(L, B, nh), boxes(L, B, nh), logits(B, nh), boxes(B, nh)] if hybrid else [None] * 4
    return outs, g


def random_targets(counts, C, g, dtype=torch.float64):
    return [{"labels": torch.randint(0, C, (k,), generator=g),
             "boxes": torch.cat((torch.rand(k, 2, generator=g, dtype=dtype), 0.02 + 0.4 * torch.rand(k, 2, generator=g, dtype=dtype)), -1)}
            for k in counts]


def test_an_image_without_boxes():
    outs, g = random_outputs(n_dn=6)
    targets = random_targets((3, 0), 5, g)
    losses, grads = run(outs, targets, (2, 3))
    assert len(losses) == 3 * (2 * (2 + 1) + 2) and all(torch.isfinite(v) for v in losses.values())
    assert all(torch.isfinite(gr).all() for gr in grads)
    assert (grads[1][:, 1] == 0).all() and (grads[1][:, 0] != 0).any()       # the empty image's boxes get no gradient


def test_all_images_empty_clamps_num_boxes_to_one():
    outs, g = random_outputs(n_dn=2)
    targets = random_targets((0, 0), 5, g)
    losses, grads = run(outs, targets, (1, 2))
    assert all(torch.isfinite(v) for v in losses.values()) and all(torch.isfinite(gr).all() for gr in grads)
    assert all(losses[k].item() == 0 for k in losses if "bbox" in k or "giou" in k)
    # only the negative focal term is left, over num_boxes = 1
    x = outs[2].detach()
    want = (0.75 * x.sigmoid() ** 2 * torch.nn.functional.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")).sum()
    assert abs(losses["loss_class_enc"].item() - want.item()) <= 1e-12 * want.item()


def test_more_target_copies_than_queries():
    """N = 8, G = 3, six copies: 18 columns for 8 queries, and the reference matches all 8."""
    outs, g = random_outputs(B=1, nq=8, nh=8)
    targets = random_targets((3,), 5, g)
    cost = crit.match_cost(outs[4][0].detach(), outs[5][0].detach(), targets[0]["boxes"][None], targets[0]["labels"][None].int(),
                           torch.tensor([3], dtype=torch.int32), fused=False)
    (src, tgt), = crit.hungarian_match(cost, [3], repeat=6)
    assert sorted(src.tolist()) == list(range(8)) and (tgt < 3).all() and (tgt >= 0).all()
    losses, grads = run(outs, targets, None)
    assert all(torch.isfinite(v) for v in losses.values())
    assert (grads[5].abs().sum(-1) != 0).all()                                # every hybrid query is matched


def test_without_denoising_queries_and_without_the_hybrid_branch():
    outs, g = random_outputs(hybrid=False)
    targets = random_targets((2, 1), 5, g)
    losses, _ = run(outs, targets, None)
    assert set(losses) == {f"loss_{n}{s}" for n in ("class", "bbox", "giou") for s in ("", "_0", "_enc")}


def test_key_names_for_one_decoder_layer():
    outs, g = random_outputs(L=1, n_dn=4)
    targets = random_targets((2, 1), 5, g)
    losses, _ = run(outs, targets, (2, 2))
    assert set(losses) == {f"loss_{n}{s}" for n in ("class", "bbox", "giou") for s in ("", "_enc", "_dn", "_hybrid", "_enc_hybrid")}


def test_denoising_groups_index_the_reference_way():
    """Query g * max_gt + t is matched to gt t; slots t >= G_b are unmatched."""
    outs, g = random_outputs(L=1, n_dn=6, hybrid=False)
    targets = random_targets((2, 1), 5, g)
    _, grads = run(outs, targets, (2, 3))
    touched = grads[1][0, :, :6].abs().sum(-1) != 0
    assert touched.tolist() == [[True, True, False, True, True, False], [True, False, False, True, False, False]]


def test_what_is_not_built_raises():
    with pytest.raises(NotImplementedError):
        RelationCriterion(5, two_stage_binary_cls=True)
    with pytest.raises(NotImplementedError):
        RelationCriterion(5, mixed_match=True)


def test_fused_pieces_have_no_cpu_kernel_path():
    x, b = torch.zeros(1, 4, 3), torch.zeros(1, 4, 4)
    gb, gl = torch.zeros(1, 1, 4), torch.zeros(1, 1, dtype=torch.int32)
    with pytest.raises(_lib.RdetrError):
        crit.set_loss_forward(x, b, torch.zeros(1, 4, dtype=torch.int32), gb, gl, 0, 1.0, 1.0)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_once_bound_and_exported(name):
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    ret = "long long" if name.endswith("_workspace_bytes") else "int"
    assert len(re.findall(r"^" + ret + " " + name + r"\s*\(", header, re.M)) == 1
    assert name in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert callable(getattr(_lib.load(), name))


def test_abi_version_and_options_are_unchanged():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert "#define RDETR_ABI_VERSION 3" in header and _lib.load().rdetr_abi_version() == 3
    assert len(dataclasses.fields(options.Options)) == 25                   # the criterion is a class, not a routing switch


def test_workspace_bytes_and_argument_refusals():
    lib = _lib.load()
    ws = lib.rdetr_set_loss_workspace_bytes
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(1, 1) == 24 and ws(3, 32) == 72 and ws(3, 33) == 144
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(8)

    def cost(fn=lib.rdetr_match_cost_f32, logits=one, boxes=one, R=2, B=2, N=4, C=3, G=2, ld=(12, 16), out=one):
        return fn(logits, ld[0], boxes, ld[1], one, one, one, R, B, N, C, G, 0.25, 2.0, 2.0, 5.0, 2.0, out, None)
    assert cost(R=0, logits=None, boxes=None, out=None) == 0
    assert cost(logits=None) == -1 and cost(out=None) == -1 and cost(B=0) == -1 and cost(G=0) == -1
    assert cost(ld=(11, 16)) == -1 and cost(ld=(12, 15)) == -1
    assert cost(G=2049) == -2 and cost(boxes=odd) == -2 and cost(ld=(12, 18)) == -2
    assert cost(fn=lib.rdetr_match_cost_bf16, logits=ctypes.c_void_p(3)) == -2

    def loss(fn=lib.rdetr_set_loss_f32, logits=one, R=2, N=4, C=3, split=0, ws=(one, 48), ld=(12, 16), dlogits=one, dbox=one):
        return fn(logits, ld[0], one, ld[1], one, one, one, R, 2, N, C, 2, split, 1.0, 1.0, 0.25, 2.0, ws[0], ws[1], one, dlogits, dbox, dbox, None)
    assert loss(R=0) == 0
    assert loss(logits=None) == -1 and loss(dlogits=None) == -1 and loss(ws=(None, 48)) == -1 and loss(ws=(one, 47)) == -1
    assert loss(split=-1) == -1 and loss(ld=(11, 16)) == -1
    assert loss(dbox=odd) == -2 and loss(fn=lib.rdetr_set_loss_bf16, dlogits=ctypes.c_void_p(3)) == -2


def test_package_exports_and_shadow_tables_still_complete():
    for name in ("RelationCriterion", "SetLossFunction", "match_cost", "hungarian_match", "set_loss"):
        assert name in relation_detr_amd.__all__ and getattr(relation_detr_amd, name) is getattr(crit, name)
    import test_shadow_complete as t
    t.test_every_ops_function_is_classified()
    t.test_every_rdetr_symbol_is_under_the_tripwire_or_excluded()
    t.test_every_training_module_function_is_classified()
