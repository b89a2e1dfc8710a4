"""GPU checks of the training criterion's kernels (csrc/criterion.hip) and of ``RelationCriterion`` on its fused route.

The checker is the module's torch route in float64 on the same device values (bf16 logits upcast).  ``e32`` is the error of that
route run in fp32 on the same values against the checker, computed here, elementwise.  The bound of a quantity q is
    |kernel - checker| <= max(4 * e32, 2^-20 * max(1, |checker|))
elementwise: the kernels compute in fp32 like the fp32 route, in another operation order (the factor 4), and 2^-20 = 8 fp32 ulps
covers the elements where the fp32 route happens to round to the checker.  Box gradients use max |checker| of the tensor in the
floor (their terms cancel, so a small element carries the rounding of the large ones), the match cost for the same reason the
summed magnitude of its own terms (tests/shadow.py, match_cost_scale); bf16 ``dlogits`` are rounded once to bf16:
2^-8 |checker| + 4 * e32, and the bf16 gradient that autograd returns twice (the saved ``dlogits``, then its product with the
upstream gradient): ((1 + 2^-8)^2 - 1) |checker| + 4 * e32.  With ``RDETR_CRITERION_ERRORS=<file>`` the worst error of each
quantity, as a fraction of its bound, is written there (profiles/r16/criterion_errors.txt)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import synthetic_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
FLOOR = 2.0 ** -20
CASES = [(6, 37, 11, [3, 0]), (2, 130, 91, [1, 17]), (1, 8, 3, [5])]           # (R, N, C, gt counts of the B images)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def error_report():
    yield
    path = os.environ.get("RDETR_CRITERION_ERRORS")
    if path and WORST:
        with open(path, "w") as f:
            f.write("worst |kernel - fp64 checker| of each quantity: as a fraction of its bound, absolute, and the fp32 torch route's own\n")
            for k in sorted(WORST):
                f.write(f"{k:58s} {WORST[k][0]:8.3f} of bound   abs {WORST[k][1]:.3e}   fp32 torch route abs {WORST[k][2]:.3e}\n")


def within(what, got, checker, fp32, floor_scale="element", rel=0.0):
    """Record and assert |got - checker| <= max(4 e32, 2^-20 max(1, scale)) + rel |checker|."""
    got, checker, fp32 = got.detach().to(F64), checker.detach().to(F64), fp32.detach().to(F64)
    assert got.shape == checker.shape, (what, got.shape, checker.shape)
    if not got.numel():
        return
    assert torch.isfinite(got).all(), what
    e32 = (fp32 - checker).abs()
    scale = floor_scale.to(F64) if torch.is_tensor(floor_scale) else checker.abs() if floor_scale == "element" else checker.abs().max()
    bound = torch.maximum(4 * e32, FLOOR * scale.clamp(min=1.0)) + rel * checker.abs()
    err = (got - checker).abs()
    frac = (err / bound).max().item()
    print(f"{what}: worst {frac:.3f} of the bound, abs {err.max().item():.3e}, fp32 route abs {e32.max().item():.3e}")
    if frac >= WORST.get(what, (0.0,))[0]:
        WORST[what] = (frac, err.max().item(), e32.max().item())
    assert frac <= 1.0, (what, frac)


def make_case(R, N, C, counts, dtype, seed=0, label_c=False):
    """A stack that is a query slice of a taller tensor, padded gt tables, and a match table with -1, repeated gts and, in row 0, a
    pair of disjoint boxes."""
    from relation_detr_amd import criterion as crit
    g = torch.Generator().manual_seed(seed + 97 * N)
    B, Gmax = len(counts), max(1, max(counts))
    tall_l = (2 * torch.randn(R, N + 5, C, generator=g)).clamp(-6, 6).to(dtype).to(DEV)
    tall_b = torch.cat((torch.rand(R, N + 5, 2, generator=g), 0.02 + 0.4 * torch.rand(R, N + 5, 2, generator=g)), -1).to(DEV)
    gt_boxes = torch.cat((torch.rand(B, Gmax, 2, generator=g), 0.02 + 0.4 * torch.rand(B, Gmax, 2, generator=g)), -1)
    gt_labels = torch.randint(0, C, (B, Gmax), generator=g, dtype=torch.int32)
    match = torch.full((R, N), -1, dtype=torch.int32)
    for r in range(R):
        k = counts[r % B]
        if k:
            match[r] = torch.randint(-1, k, (N,), generator=g, dtype=torch.int32)       # -1 and repeated gts
    if counts[0]:
        gt_boxes[0, 0] = torch.tensor([0.2, 0.2, 0.1, 0.1])
        tall_b[0, 3] = torch.tensor([0.8, 0.7, 0.1, 0.2], device=DEV)                       # query 0 of the slice: IoU 0 with gt 0
        match[0, 0] = 0
    if label_c:
        gt_labels[0, 0] = C
    logits, boxes = tall_l[:, 3:3 + N], tall_b[:, 3:3 + N]
    assert not logits.is_contiguous() or R == 1
    return crit, logits, boxes, gt_boxes.to(DEV), gt_labels.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV), match.to(DEV)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R,N,C,counts", CASES)
def test_match_cost(R, N, C, counts, dtype):
    crit, logits, boxes, gt_boxes, gt_labels, gt_count, _ = make_case(R, N, C, counts, dtype)
    got = crit.match_cost(logits, boxes, gt_boxes, gt_labels, gt_count)
    assert got.dtype == F32 and tuple(got.shape) == (R, N, gt_boxes.shape[1])
    checker = crit.match_cost(logits.to(F64), boxes.to(F64), gt_boxes.to(F64), gt_labels, gt_count, fused=False)
    fp32 = crit.match_cost(logits.to(F32), boxes, gt_boxes, gt_labels, gt_count, fused=False)
    # the floor's scale is the magnitude of the terms the cost adds up, not of their signed sum (tests/shadow.py, match_cost_scale)
    import shadow
    scale = shadow.match_cost_scale(dict(logits=logits, boxes=boxes, gt_boxes=gt_boxes, gt_labels=gt_labels, gt_count=gt_count, cost_class=2.0,
                                         cost_bbox=5.0, cost_giou=2.0, alpha=0.25, gamma=2.0))
    within(f"match_cost {'f32' if dtype == F32 else 'bf16'}", got, checker, fp32, floor_scale=scale)
    for r in range(R):
        assert (got[r, :, counts[r % len(counts)]:] == 0).all()                             # padded columns: exactly 0
    assert counts[0] == 0 or (got[0, :, :counts[0]] != 0).all()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_match_cost_label_equal_to_c_has_no_class_term(dtype):
    R, N, C, counts = CASES[0]
    crit, logits, boxes, gt_boxes, gt_labels, gt_count, _ = make_case(R, N, C, counts, dtype)
    base = crit.match_cost(logits, boxes, gt_boxes, gt_labels, gt_count)
    boxes_only = crit.match_cost(logits, boxes, gt_boxes, gt_labels, gt_count, cost_class=0.0)
    bad = gt_labels.clone()
    bad[0, 0] = C
    got = crit.match_cost(logits, boxes, gt_boxes, bad, gt_count)
    rows = torch.arange(0, R, 2, device=DEV)                                               # the rows of image 0
    assert torch.equal(got[rows, :, 0], boxes_only[rows, :, 0])                            # the class term is 0 ...
    keep = torch.ones_like(got, dtype=torch.bool)
    keep[rows, :, 0] = False
    assert torch.equal(got[keep], base[keep])                                               # ... and nothing else changes
    checker = crit.match_cost(logits.to(F64), boxes.to(F64), gt_boxes.to(F64), bad, gt_count, fused=False)
    within("match_cost label = C", got, checker, crit.match_cost(logits.to(F32), boxes, gt_boxes, bad, gt_count, fused=False))


def checker_grads(crit, logits, boxes, match, gt_boxes, gt_labels, n_split, inv_a, inv_b, dtype):
    x = logits.detach().to(dtype).requires_grad_(True)
    b = boxes.detach().to(dtype).requires_grad_(True)
    sums = crit.set_loss(x, b, match, gt_boxes.to(dtype), gt_labels, n_split, inv_a, inv_b, fused=False)
    dlogits, = torch.autograd.grad(sums[..., 0].sum(), x, retain_graph=True)
    dl1, = torch.autograd.grad(sums[..., 1].sum(), b, retain_graph=True)
    dgiou, = torch.autograd.grad(sums[..., 2].sum(), b, retain_graph=True)
    return sums, dlogits, dl1, dgiou, x, b


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n_split", [0, 6])
@pytest.mark.parametrize("R,N,C,counts", CASES)
def test_set_loss(R, N, C, counts, n_split, dtype):
    crit, logits, boxes, gt_boxes, gt_labels, _, match = make_case(R, N, C, counts, dtype, seed=1, label_c=(N == 37))
    inv_a, inv_b = 1.0 / 12.0, 1.0 / 5.0
    tag = f"{'f32' if dtype == F32 else 'bf16'}"
    got = crit.set_loss_forward(logits, boxes, match, gt_boxes, gt_labels, n_split, inv_a, inv_b)
    again = crit.set_loss_forward(logits, boxes, match, gt_boxes, gt_labels, n_split, inv_a, inv_b)
    for a, b in zip(got, again):
        assert torch.equal(a, b)                                                            # fixed-order sums: the same bits
    sums, dlogits, dl1, dgiou = got
    assert dlogits.dtype == dtype and sums.dtype == dl1.dtype == dgiou.dtype == F32
    c64 = checker_grads(crit, logits, boxes, match, gt_boxes, gt_labels, n_split, inv_a, inv_b, F64)
    c32 = checker_grads(crit, logits, boxes, match, gt_boxes, gt_labels, n_split, inv_a, inv_b, F32)
    within(f"set_loss sums {tag}", sums, c64[0], c32[0])
    within(f"set_loss dbox_l1 {tag}", dl1, c64[2], c32[2], floor_scale="tensor")
    within(f"set_loss dbox_giou {tag}", dgiou, c64[3], c32[3], floor_scale="tensor")
    within(f"set_loss dlogits {tag}", dlogits, c64[1], c32[1], rel=0.0 if dtype == F32 else 2.0 ** -8)
    # the same stack as a tensor of its own: the logits and their gradient share one alignment, so the vectors are stored whole
    fresh = lambda t: t.clone(memory_format=torch.contiguous_format)
    packed = crit.set_loss_forward(fresh(logits), fresh(boxes), match, gt_boxes, gt_labels, n_split, inv_a, inv_b)
    assert torch.equal(packed[1], dlogits) and torch.equal(packed[2], dl1) and torch.equal(packed[3], dgiou)
    within(f"set_loss sums {tag}", packed[0], c64[0], c32[0])
    unmatched = (match < 0)[..., None].expand_as(dl1)
    assert (dl1[unmatched] == 0).all() and (dgiou[unmatched] == 0).all()
    if n_split == 0:
        assert (sums[:, 0] == 0).all()
    if counts[0]:                                                                           # the disjoint pair: IoU 0, a GIoU loss above 1
        assert dlogits[0, 0].float().abs().max() > 0 and (dgiou[0, 0] != 0).any()

    # autograd through the Function under a random upstream gradient
    up = torch.randn(R, 2, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    x = logits.detach().requires_grad_(True)                                               # the same memory: the same summation order
    b = boxes.detach().requires_grad_(True)
    out = crit.set_loss(x, b, match, gt_boxes, gt_labels, n_split, inv_a, inv_b)
    assert torch.equal(out, sums)
    out.backward(up)
    want = []
    for c, dt in ((c64, F64), (c32, F32)):
        want.append(torch.autograd.grad(c[0], (c[4], c[5]), up.to(dt)))
    # bf16: the saved gradient is rounded to bf16 once and its product with the upstream gradient once more
    within(f"set_loss autograd logits {tag}", x.grad, want[0][0], want[1][0], rel=0.0 if dtype == F32 else (1 + 2.0 ** -8) ** 2 - 1)
    within(f"set_loss autograd boxes {tag}", b.grad, want[0][1], want[1][1], floor_scale="tensor")


def fixture_on_device(z, dtype):
    outputs = [torch.from_numpy(z[f"out.{i}"]).to(DEV).to(dtype).requires_grad_(True) for i in range(8)]
    targets = [{"labels": torch.from_numpy(z[f"tgt.labels.{b}"]).to(DEV), "boxes": torch.from_numpy(z[f"tgt.boxes.{b}"]).to(DEV).to(dtype)}
               for b in range(2)]
    return outputs, targets, tuple(int(v) for v in z["dn_meta"])


def losses_and_grads(outputs, targets, dn_meta, fused, num_classes=11):
    from relation_detr_amd import RelationCriterion
    losses = RelationCriterion(num_classes, fused=fused)(tuple(outputs), targets, dn_meta)
    grads = torch.autograd.grad(torch.stack([v.to(outputs[1].dtype) for v in losses.values()]).sum(), outputs)
    return losses, grads


def test_fixture_end_to_end_on_the_device():
    from relation_detr_amd import criterion as crit
    z = load_golden("g10_criterion.npz")
    outputs, targets, dn_meta = fixture_on_device(z, F32)
    got, got_grads = losses_and_grads(outputs, targets, dn_meta, fused=True)
    fp32, fp32_grads = losses_and_grads(outputs, targets, dn_meta, fused=False)
    out64, tgt64, _ = fixture_on_device(z, F64)
    checker, checker_g = losses_and_grads(out64, tgt64, dn_meta, fused=False)
    want = {k[len("loss64."):]: float(v) for k, v in z.items() if k.startswith("loss64.")}
    assert set(got) == set(checker) == set(want) and len(got) == 33
    for k in want:
        assert abs(checker[k].item() - want[k]) <= 1e-9 * abs(want[k]), k                  # the checker is the reference's fp64
        within("criterion loss values (fixture)", got[k], checker[k], fp32[k])
    for i in range(8):
        within(f"criterion gradient of output {i} (fixture)", got_grads[i], checker_g[i], fp32_grads[i],
               floor_scale="element" if i % 2 == 0 else "tensor")
    # the assignments, from the device costs
    gt_boxes = torch.zeros(2, 3, 4, device=DEV)
    gt_labels = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    for b, t in enumerate(targets):
        n = len(t["labels"])
        gt_boxes[b, :n], gt_labels[b, :n] = t["boxes"], t["labels"].int()
    gt_count = torch.tensor([3, 2], dtype=torch.int32, device=DEV)
    o = [t.detach() for t in outputs]
    stacks = {"dec": (o[0].flatten(0, 1)[:, 6:], o[1].flatten(0, 1)[:, 6:], 1), "enc": (o[2], o[3], 1),
              "hyb": (o[4].flatten(0, 1), o[5].flatten(0, 1), 6), "hyb_enc": (o[6], o[7], 6)}
    for name, (logits, boxes, copies) in stacks.items():
        cost = crit.match_cost(logits, boxes, gt_boxes, gt_labels, gt_count)
        for r, (src, tgt) in enumerate(crit.hungarian_match(cost.cpu(), [3, 2], repeat=copies)):
            qmap = np.full(logits.shape[1], -1, dtype=np.int32)
            qmap[src.numpy()] = tgt.numpy()
            key = f"match.{name}{r // 2}.{r % 2}" if name in ("dec", "hyb") else f"match.{name}.{r}"
            assert np.array_equal(qmap, z[key]), key


def test_one_training_step_through_the_transformer():
    """The g8-sized network, default options, fp32: forward -> RelationCriterion -> backward.  Values against the torch route on the
    same outputs; gradients only finite (tied proposals may legitimately be matched to different duplicates)."""
    from relation_detr_amd import RelationCriterion
    from relation_detr_amd.transformer import build_relation_transformer
    g = load_golden("g8_transformer_train.npz")
    z = load_golden("g10_criterion.npz")
    T = torch.from_numpy
    net = build_relation_transformer(num_classes=11, d_ffn=64, enc_layers=2, dec_layers=3, num_queries=24, hybrid_num_proposals=30)
    net.load_state_dict(synthetic_state_dict(net.state_dict()))
    net = net.to(DEV).train()
    feats = [T(g[f"feat{i}"]).to(DEV) for i in range(4)]
    masks = [T(g[f"mask{i}"]).to(DEV) for i in range(4)]
    pos = [T(g[f"pos{i}"]).to(DEV) for i in range(4)]
    outs = net(feats, masks, pos, T(g["dn_label"]).to(DEV), T(g["dn_box"]).to(DEV), T(g["attn_mask"]).to(DEV))
    targets = [{"labels": T(z[f"tgt.labels.{b}"]).to(DEV), "boxes": T(z[f"tgt.boxes.{b}"]).to(DEV)} for b in range(2)]
    dn_meta = (2, 3)
    losses = RelationCriterion(11)(outs, targets, dn_meta)
    assert len(losses) == 33
    detached = tuple(o.detach() for o in outs)
    fp32 = RelationCriterion(11, fused=False)(detached, targets, dn_meta)
    checker = RelationCriterion(11, fused=False)(tuple(o.to(F64) for o in detached),
                                                 [{"labels": t["labels"], "boxes": t["boxes"].to(F64)} for t in targets], dn_meta)
    assert set(losses) == set(checker)
    for k in checker:
        within("criterion loss values (transformer step)", losses[k], checker[k], fp32[k])
    torch.stack(list(losses.values())).sum().backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert len(grads) > 100 and all(torch.isfinite(gr).all() for gr in grads)
    assert any(gr.abs().max() > 0 for gr in grads)
