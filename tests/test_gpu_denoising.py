"""GPU checks of the denoising generator's kernels (csrc/denoising.hip), of ``GenerateCDNQueries`` on its fused route and of
``RelationDETRHead``.

Noised labels, masks and label queries (copies of embedding rows, bf16 included) are compared exactly.  For the box queries and
the embedding gradient the checker is the module's torch route in float64 on the same device values, ``e32`` the error of that
route in fp32 against it, and the bound, elementwise,
    |kernel - checker| <= max(4 * e32, 2^-20 * max(1, |checker|))
the criterion tests' convention: the kernel computes in fp32 like the fp32 route (the box arithmetic in the same order, so only
``logf`` differs; the gradient's rows in ascending instead of atomic order, the factor 4), and 2^-20 = 8 fp32 ulps covers the
elements where the fp32 route happens to round to the checker.  A bf16 gradient is rounded once more: + 2^-8 |checker|."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_denoising_host import C, D, EXPECTED_KEYS, NQ, fixture_case, head_inputs, slot_labels, tiny_head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
FLOOR = 2.0 ** -20
T = torch.from_numpy
# (counts, denoising_nums): padding and an empty image; one gt in 100 groups; two blocks' worth of slots with a long padded tail;
# one group of more boxes than denoising_nums; no box at all
RANDOM_CASES = [([3, 0, 5], 12), ([1], 100), ([130, 7], 100), ([101], 100), ([0, 0], 100)]


@pytest.fixture(scope="module")
def g11():
    return load_golden("g11_denoising.npz")


def within(what, got, checker, fp32, rel=0.0):
    got, checker, fp32 = got.detach().to(F64), checker.detach().to(F64), fp32.detach().to(F64)
    assert got.shape == checker.shape, (what, got.shape, checker.shape)
    if not got.numel():
        return
    assert torch.isfinite(got).all(), what
    e32 = (fp32 - checker).abs()
    bound = torch.maximum(4 * e32, FLOOR * checker.abs().clamp(min=1.0)) + rel * checker.abs()
    err = (got - checker).abs()
    print(f"{what}: worst {(err / bound).max().item():.3f} of the bound, abs {err.max().item():.3e}, fp32 route abs {e32.max().item():.3e}")
    assert (err <= bound).all(), (what, (err / bound).max().item())


def targets_for(counts, seed=0):
    g = torch.Generator().manual_seed(seed + 31 * sum(counts))
    labels = torch.randint(0, C, (sum(counts),), generator=g)
    boxes = torch.cat((0.05 + 0.9 * torch.rand(sum(counts), 2, generator=g), 0.02 + 0.5 * torch.rand(sum(counts), 2, generator=g)), -1)
    return labels.to(DEV), boxes.to(DEV)


def embedding(d, dtype, seed=0):
    return torch.randn(C, d, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


def check_against_torch_route(what, embed, labels, boxes, counts, groups, prob, scale, noise, got):
    from relation_detr_amd import denoising as dn
    label_query, box_query, noised = got
    B, n_dn = len(counts), 2 * groups * max(counts)
    assert label_query.dtype == embed.dtype and tuple(label_query.shape) == (B, n_dn, embed.shape[1])
    assert box_query.dtype == F32 and tuple(box_query.shape) == (B, n_dn, 4) and noised.dtype == torch.int32
    lq64, bq64, lab64 = dn.cdn_queries(embed, labels, boxes.to(F64), counts, groups, prob, scale, noise=noise, fused=False)
    _, bq32, _ = dn.cdn_queries(embed, labels, boxes, counts, groups, prob, scale, noise=noise, fused=False)
    assert torch.equal(noised, lab64)
    assert torch.equal(label_query, lq64)                                       # copies of rows; zeros for padding
    within(what, box_query, bq64, bq32)
    pad = noised < 0
    assert (box_query[pad] == 0).all() and (label_query[pad] == 0).all()


@pytest.mark.parametrize("name", list("abcde"))
def test_fused_forward_on_the_recorded_draws(g11, name):
    from relation_detr_amd import GenerateCDNQueries, denoising as dn
    settings, labels, boxes, noise, counts = fixture_case(g11, name, device=DEV)
    module = GenerateCDNQueries(num_queries=NQ, num_classes=C, label_embed_dim=D, **settings)
    module.load_state_dict({"label_encoder.weight": T(g11["embed"])})
    module = module.to(DEV)
    label_query, box_query, mask, groups, group_size = module(labels, boxes, noise=noise)
    assert (groups, group_size) == tuple(int(v) for v in g11[f"{name}.meta"])
    assert mask.dtype == torch.bool and torch.equal(mask.cpu(), T(g11[f"{name}.mask"]))
    want_labels = slot_labels(counts, groups, g11[f"{name}.noised_labels"])
    got = dn.cdn_queries(module.label_encoder.weight, torch.cat(labels), torch.cat(boxes).reshape(-1, 4), counts, groups,
                         settings["label_noise_prob"], settings["box_noise_scale"], noise=noise)
    assert np.array_equal(got[2].cpu().numpy(), want_labels)
    assert torch.equal(got[0], label_query) and torch.equal(got[1], box_query)
    embed = g11["embed"]
    assert np.array_equal(label_query.detach().cpu().numpy(), np.where(want_labels[..., None] >= 0, embed[np.maximum(want_labels, 0)], 0.0))
    if name == "a":
        assert np.array_equal(label_query.detach().cpu().numpy(), g11["a.label_query"])
    check_against_torch_route(f"box queries, fixture {name}", module.label_encoder.weight.detach(), torch.cat(labels),
                              torch.cat(boxes).reshape(-1, 4), counts, groups, settings["label_noise_prob"], settings["box_noise_scale"],
                              noise, got)
    # and against the reference's own fp32 numbers: the same operations in the same order up to the quotient, then logf
    want = T(g11[f"{name}.box_query"]).to(DEV)
    assert ((box_query - want).abs() <= FLOOR * want.abs().clamp(min=1.0)).all()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [256, 64])
@pytest.mark.parametrize("counts,nums", RANDOM_CASES)
def test_fused_forward_random(counts, nums, d, dtype):
    from relation_detr_amd import denoising as dn
    groups = dn.denoising_groups(nums, max(counts))
    labels, boxes = targets_for(counts)
    embed = embedding(d, dtype)
    noise = dn.cdn_noise(1234 + d, 2 * groups * sum(counts), C, DEV)
    got = dn.cdn_queries(embed, labels, boxes, counts, groups, 0.6, 1.0, noise=noise)
    check_against_torch_route(f"box queries {counts} d={d}", embed, labels, boxes, counts, groups, 0.6, 1.0, noise, got)
    off = dn.cdn_queries(embed, labels, boxes, counts, groups, 0.0, 0.0, noise=(None,) * 4)
    check_against_torch_route(f"box queries {counts} d={d}, noise off", embed, labels, boxes, counts, groups, 0.0, 0.0, (None,) * 4, off)
    mask = dn.denoising_mask(groups, 2 * max(counts), NQ, DEV)
    assert mask.dtype == torch.bool and torch.equal(mask, dn.denoising_mask(groups, 2 * max(counts), NQ, DEV, fused=False))


def test_mask_counts_and_odd_sizes():
    from relation_detr_amd import denoising as dn
    assert int(dn.denoising_mask(100, 2, 24, DEV).sum()) == 44400 and int(dn.denoising_mask(1, 260, 24, DEV).sum()) == 6240
    for groups, gs, nq in ((1, 0, 24), (3, 2, 1), (2, 6, 5), (1, 2, 0), (5, 14, 33)):       # T * T not a multiple of 4 among them
        got = dn.denoising_mask(groups, gs, nq, DEV)
        assert tuple(got.shape) == (groups * gs + nq,) * 2 and torch.equal(got, dn.denoising_mask(groups, gs, nq, DEV, fused=False))


def test_label_outside_the_classes_is_never_an_index():
    from relation_detr_amd import denoising as dn
    counts = [3, 2]
    labels, boxes = targets_for(counts)
    labels = labels.clone()
    labels[1], labels[4] = C, -3
    embed = embedding(64, F32)
    label_query, box_query, noised = dn.cdn_queries(embed, labels, boxes, counts, 2, 0.0, 1.0, key=5)
    want = T(slot_labels(counts, 2, np.tile(labels.cpu().numpy(), 4))).to(DEV)
    want = torch.where((want >= 0) & (want < C), want, torch.full_like(want, -1))
    assert torch.equal(noised, want)
    assert torch.equal(label_query, torch.where((want >= 0)[..., None], embed[want.clamp(min=0).long()], torch.zeros((), device=DEV)))
    assert torch.isfinite(box_query).all()


# --------------------------------------------------------------------------------------------------------------------- key path
def test_keyed_noise_is_the_numpy_restatement():
    from relation_detr_amd import denoising as dn
    for key, Q in ((0, 5), (0x5EED0123456789AB, 8192), (2 ** 64 - 1, 300)):
        got = dn.cdn_noise(key, Q, 91, DEV)
        want = dn.cdn_noise(key, Q, 91, "cpu")
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and torch.equal(a.cpu(), b)
    assert all(x.numel() == 0 for x in dn.cdn_noise(1, 0, 91, DEV))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("counts,nums", RANDOM_CASES[:3])
def test_keyed_queries_equal_the_queries_of_the_written_draws(counts, nums, dtype):
    from relation_detr_amd import denoising as dn
    groups = dn.denoising_groups(nums, max(counts))
    labels, boxes = targets_for(counts, seed=2)
    embed = embedding(64, dtype)
    key = 0xC0FFEE12345
    keyed = dn.cdn_queries(embed, labels, boxes, counts, groups, 0.6, 1.0, key=key)
    noise = dn.cdn_noise(key, 2 * groups * sum(counts), C, DEV)
    written = dn.cdn_queries(embed, labels, boxes, counts, groups, 0.6, 1.0, noise=noise)
    again = dn.cdn_queries(embed, labels, boxes, counts, groups, 0.6, 1.0, key=key)
    other = dn.cdn_queries(embed, labels, boxes, counts, groups, 0.6, 1.0, key=key + 1)
    for a, b, c in zip(keyed, written, again):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(keyed[1], other[1])


def test_module_key_comes_from_the_host_generator():
    from relation_detr_amd import GenerateCDNQueries
    module = GenerateCDNQueries(num_queries=NQ, num_classes=C, label_embed_dim=64, denoising_nums=12).to(DEV)
    labels, boxes = targets_for([3, 0, 5])
    labels, boxes = list(labels.split([3, 0, 5])), list(boxes.split([3, 0, 5]))
    torch.manual_seed(3)
    first = module(labels, boxes)
    second = module(labels, boxes)
    torch.manual_seed(3)
    repeat = module(labels, boxes)
    by_generator = module(labels, boxes, generator=torch.Generator().manual_seed(3))
    assert torch.equal(first[1], repeat[1]) and torch.equal(first[0], repeat[0]) and not torch.equal(first[1], second[1])
    assert torch.equal(by_generator[1], module(labels, boxes, generator=torch.Generator().manual_seed(3))[1])
    assert first[3:] == (2, 10) and module.denoising_groups == 2 and tuple(first[2].shape) == (20 + NQ, 20 + NQ)


# --------------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [256, 64])
@pytest.mark.parametrize("counts,nums,prob", [([3, 0, 5], 12, 0.0), ([1], 100, 0.5), ([130, 7], 100, 0.6)])
def test_embedding_gradient(counts, nums, prob, d, dtype):
    from relation_detr_amd import denoising as dn
    groups = dn.denoising_groups(nums, max(counts))
    labels, boxes = targets_for(counts, seed=4)
    embed = embedding(d, dtype).requires_grad_(True)
    label_query, _, noised = dn.cdn_queries(embed, labels, boxes, counts, groups, prob, 1.0, key=77)
    B, n_dn = noised.shape
    up = torch.randn(n_dn, B, d, generator=torch.Generator().manual_seed(9)).to(dtype).to(DEV).transpose(0, 1)
    assert not up.is_contiguous() or B == 1
    label_query.backward(up)                                                    # through CdnQueryFunction, the gradient not contiguous
    got = embed.grad
    assert got.dtype == dtype and tuple(got.shape) == (C, d)
    assert torch.equal(got, dn.cdn_embed_backward(up, noised, C)) and torch.equal(got, dn.cdn_embed_backward(up.contiguous(), noised, C))
    used = noised >= 0
    index = noised[used].long()
    checker = torch.zeros(C, d, dtype=F64, device=DEV).index_add_(0, index, up[used].to(F64))
    fp32 = torch.zeros(C, d, dtype=F32, device=DEV).index_add_(0, index, up[used].to(F32))
    within(f"grad_embed {counts} d={d}", got, checker, fp32, rel=0.0 if dtype == F32 else 2.0 ** -8)
    unused = sorted(set(range(C)) - set(index.tolist()))
    assert prob > 0 or len(unused) >= 3
    assert (got[unused] == 0).all() and (got[sorted(set(index.tolist()))] != 0).any()


def test_embedding_gradient_without_any_slot():
    from relation_detr_amd import denoising as dn
    got = dn.cdn_embed_backward(torch.zeros(2, 0, 64, device=DEV), torch.zeros(2, 0, dtype=torch.int32, device=DEV), C)
    assert tuple(got.shape) == (C, 64) and (got == 0).all()


# ------------------------------------------------------------------------------------------------------------------------- head
def test_head_training_step():
    from relation_detr_amd import denoising as dn
    head = tiny_head(DEV, True).train()
    (feats, masks, pos), targets = head_inputs(DEV)
    noise = dn.cdn_noise(11, 2 * 2 * 5, C, DEV)

    def by_hand():
        label_query, box_query, mask, groups, group_size = head.denoising_generator([t["labels"] for t in targets],
                                                                                   [t["boxes"] for t in targets], noise=noise)
        assert (groups, group_size) == (2, 6)
        return head.criterion(head.transformer(feats, masks, pos, label_query, box_query, mask), targets, dn_meta=(groups, group_size))

    losses = head(feats, masks, pos, targets, noise=noise)
    assert set(losses) == EXPECTED_KEYS and all(torch.isfinite(v) for v in losses.values())
    torch.stack(list(losses.values())).sum().backward()
    grad = head.denoising_generator.label_encoder.weight.grad
    assert grad is not None and torch.isfinite(grad).all() and grad.abs().max() > 0
    first, second = by_hand(), by_hand()                                        # with autograd on: the routes the head took
    for k in losses:
        spread = (first[k] - second[k]).abs().item()
        print(f"{k}: head {losses[k].item():.9g} by hand {first[k].item():.9g} spread {spread:.3e}")
        assert (losses[k].detach() - first[k]).abs().item() <= spread, k

    keyed = head(feats, masks, pos, targets)                                     # the draws from a host key
    assert set(keyed) == EXPECTED_KEYS and all(torch.isfinite(v) for v in keyed.values())
    head.eval()
    with torch.no_grad():
        logits, boxes = head(feats, masks, pos)
    assert tuple(logits.shape) == (2, NQ, C) and tuple(boxes.shape) == (2, NQ, 4)
