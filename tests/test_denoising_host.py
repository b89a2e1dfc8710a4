"""CPU checks of the denoising query generator (relation_detr_amd/denoising.py) and of ``RelationDETRHead``: the torch route fed
the reference's recorded draws against the reference's recorded results (tests/golden/g11_denoising.npz, made by
tools/gen_golden_denoising.py), the shapes the reference runs at its edges, the numpy Philox restatement against the published
known answers, and the new C entries declared once, bound and exported with the ABI version and the Options fields unchanged.

Box queries are compared within 2^-20 * max(1, |want|) = 8 fp32 ulps: every operation in front of the logarithm is a single
IEEE operation in the reference's order, so only the host's ``log`` rounding may differ between machines
(tests/golden/README.md).  Labels, masks, metas and the label queries (copies of embedding rows) are exact."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import relation_detr_amd
from conftest import load_golden
from helpers import synthetic_state_dict
from relation_detr_amd import _lib, denoising as dn, options
from relation_detr_amd.denoising import GenerateCDNQueries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
C, D, NQ = 11, 256, 24
SEEDS = {"a": 1, "b": 2, "c": 3, "d": 1, "e": 5}                              # tools/gen_golden_denoising.py: torch.manual_seed(100 + seed)
SYMBOLS = ("rdetr_cdn_queries_f32", "rdetr_cdn_queries_bf16", "rdetr_cdn_mask", "rdetr_cdn_embed_backward_f32",
           "rdetr_cdn_embed_backward_bf16", "rdetr_cdn_noise")
STAT_KEY = 0x5EED0123456789AB                                                  # the fixed key of the statistics test: it passes, see there


@pytest.fixture(scope="module")
def g11():
    return load_golden("g11_denoising.npz")


def fixture_case(z, name, device="cpu", dtype=torch.float32):
    """-> (module settings, labels list, boxes list, noise 4-tuple, counts) of one recorded case."""
    counts = [int(c) for c in z[f"{name}.counts"]]
    nums, prob, scale = z[f"{name}.settings"]
    labels = list(T(z[f"{name}.gt_labels"]).to(device).split(counts))
    boxes = list(T(z[f"{name}.gt_boxes"]).to(device).to(dtype).split(counts))
    noise = tuple(T(z[f"{name}.{k}"]).to(device) if f"{name}.{k}" in z else None for k in ("label_u", "label_r", "box_sign", "box_u"))
    return dict(denoising_nums=int(nums), label_noise_prob=float(prob), box_noise_scale=float(scale)), labels, boxes, noise, counts


def slot_labels(counts, groups, flat_labels):
    """The noised labels per slot [B, Ndn] from the reference's flat rows, -1 for padding: slot (b, j), i, t = divmod(j, max_gt),
    is flat row i * G + off[b] + t when t < G_b."""
    B, G, max_gt = len(counts), sum(counts), max(counts)
    off = np.concatenate(([0], np.cumsum(counts)))
    out = np.full((B, 2 * groups * max_gt), -1, dtype=np.int32)
    for b in range(B):
        for j in range(out.shape[1]):
            i, t = divmod(j, max_gt)
            if t < counts[b]:
                out[b, j] = flat_labels[i * G + off[b] + t]
    return out


def module_for(z, settings, fused=False):
    m = GenerateCDNQueries(num_queries=NQ, num_classes=C, label_embed_dim=D, fused=fused, **settings)
    m.load_state_dict({"label_encoder.weight": T(z["embed"])})
    return m


def box_bound(want):
    return 2.0 ** -20 * want.abs().clamp(min=1.0)


@pytest.mark.parametrize("name", list("abcde"))
def test_torch_route_matches_the_reference(g11, name):
    settings, labels, boxes, noise, counts = fixture_case(g11, name)
    module = module_for(g11, settings)
    label_query, box_query, mask, groups, group_size = module(labels, boxes, noise=noise)
    assert (groups, group_size) == tuple(int(v) for v in g11[f"{name}.meta"]) and module.denoising_groups == groups
    assert mask.dtype == torch.bool and torch.equal(mask, T(g11[f"{name}.mask"]))
    want = T(g11[f"{name}.box_query"])
    assert box_query.dtype == torch.float32 and box_query.shape == want.shape
    assert ((box_query - want).abs() <= box_bound(want)).all(), (box_query - want).abs().max()
    _, _, noised = dn.cdn_queries(module.label_encoder.weight, torch.cat(labels), torch.cat(boxes), counts, groups, settings["label_noise_prob"],
                                  settings["box_noise_scale"], noise=noise, fused=False)
    want_labels = slot_labels(counts, groups, g11[f"{name}.noised_labels"])
    assert noised.dtype == torch.int32 and np.array_equal(noised.numpy(), want_labels)
    assert tuple(label_query.shape) == (len(counts), group_size * groups, D)
    embed = g11["embed"]
    assert np.array_equal(label_query.detach().numpy(), np.where(want_labels[..., None] >= 0, embed[np.maximum(want_labels, 0)], 0.0))
    if name == "a":
        assert groups == 2 and label_query.shape[1] == 20
        assert np.array_equal(label_query.detach().numpy(), g11["a.label_query"])
    if name == "d":                                                            # both noises off: the gt itself, no draw consumed
        assert noise == (None, None, None, None)
        assert np.array_equal(noised.numpy(), slot_labels(counts, groups, np.tile(g11["d.gt_labels"], 2 * groups)))


@pytest.mark.parametrize("name", list("abcde"))
def test_torch_route_draws_in_the_reference_order(g11, name):
    """With ``noise=None`` the torch route consumes torch's generator as the reference does: under the fixture's seed it lands on
    the recorded results."""
    settings, labels, boxes, _, _ = fixture_case(g11, name)
    module = module_for(g11, settings)
    torch.manual_seed(100 + SEEDS[name])
    _, box_query, _, _, _ = module(labels, boxes)
    want = T(g11[f"{name}.box_query"])
    assert ((box_query - want).abs() <= box_bound(want)).all()
    Q = 2 * module.denoising_groups * sum(int(x.numel()) for x in labels)
    drawn = module.draw_noise(Q, "cpu", torch.Generator().manual_seed(100 + SEEDS[name]))
    for got, key in zip(drawn, ("label_u", "label_r", "box_sign", "box_u")):
        if f"{name}.{key}" in g11:
            assert got.dtype == T(g11[f"{name}.{key}"]).dtype and torch.equal(got, T(g11[f"{name}.{key}"])), key
        else:
            assert got is None


def test_float64_route_agrees_with_the_fixture(g11):
    """The checker of the GPU tests: the same route in float64 stays within the fp32 reference's own rounding of it.  A clamped box
    coordinate x in fp32 is at most 8 roundings of numbers below 2 away from the exact one (corner, noise product, scale, sum,
    centre): delta = 8 * 2^-24.  log(x / (1 - x)) then moves by at most delta / max(x, eps) + delta / max(1 - x, eps), plus the 8
    ulps of the logarithm and the quotient."""
    settings, labels, boxes, noise, _ = fixture_case(g11, "c", dtype=torch.float64)
    _, box_query, _, _, _ = module_for(g11, settings)(labels, boxes, noise=noise)
    want = T(g11["c.box_query"]).double()
    assert box_query.dtype == torch.float64
    x, delta = box_query.sigmoid(), 8 * 2.0 ** -24
    bound = delta / x.clamp(min=1e-3) + delta / (1 - x).clamp(min=1e-3) + 2.0 ** -20 * want.abs().clamp(min=1.0)
    assert ((box_query - want).abs() <= bound).all()


@pytest.mark.parametrize("counts,nums,n_dn,groups,mask_true", [
    ([0, 0], 100, 0, 1, 0), ([1], 100, 200, 100, 44400), ([101], 100, 202, 1, None), ([130, 7], 100, 260, 1, 6240)])
def test_edge_shapes_the_reference_runs(counts, nums, n_dn, groups, mask_true):
    g = torch.Generator().manual_seed(7)
    labels = [torch.randint(0, C, (k,), generator=g) for k in counts]
    boxes = [torch.cat((torch.rand(k, 2, generator=g), 0.02 + 0.4 * torch.rand(k, 2, generator=g)), -1) for k in counts]
    module = GenerateCDNQueries(num_queries=NQ, num_classes=C, label_embed_dim=64, denoising_nums=nums, fused=False)
    label_query, box_query, mask, got_groups, group_size = module(labels, boxes, generator=g)
    B = len(counts)
    assert tuple(label_query.shape) == (B, n_dn, 64) and tuple(box_query.shape) == (B, n_dn, 4)
    assert tuple(mask.shape) == (n_dn + NQ, n_dn + NQ) and mask.dtype == torch.bool
    assert (got_groups, group_size) == (groups, 2 * max(counts)) and got_groups * group_size == n_dn
    if mask_true is not None:
        assert int(mask.sum()) == mask_true
    assert torch.isfinite(box_query).all() and (box_query.abs() <= 6.9078).all()      # |log(1e-3 / 1)| = 6.90776
    for b, k in enumerate(counts):                                                  # padding rows: zeros in both
        pad = torch.arange(n_dn) % max(max(counts), 1) >= k
        assert (label_query[b, pad] == 0).all() and (box_query[b, pad] == 0).all()


def test_mask_is_the_reference_loop():
    for groups, gs, nq in ((2, 6, 5), (1, 0, 4), (3, 2, 0)):
        n = groups * gs
        want = torch.zeros(n + nq, n + nq, dtype=torch.bool)
        want[n:, :n] = True
        for i in range(groups):
            want[gs * i:gs * (i + 1), :gs * i] = True
            want[gs * i:gs * (i + 1), gs * (i + 1):n] = True
        assert torch.equal(dn.denoising_mask(groups, gs, nq, "cpu"), want)


def test_philox_known_answers():
    zero = dn.philox4x32_10([0, 0, 0, 0], [0, 0])
    assert [f"{v:08x}" for v in zero] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = dn.philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)
    assert [f"{v:08x}" for v in ones] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    pi = dn.philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])     # Random123's third vector
    assert [f"{v:08x}" for v in pi] == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_keyed_draws_layout_and_statistics():
    """Q = 8192 rows of STAT_KEY.  A share p estimated from n draws has standard error sqrt(p (1 - p) / n); 5 of them is a
    1-in-1.7-million event per statistic for a sound generator, and the key is fixed, so the test cannot flake."""
    Q = 8192
    label_u, label_r, box_sign, box_u = dn.cdn_noise(STAT_KEY, Q, C, "cpu")
    assert (label_u.dtype, label_r.dtype, box_sign.dtype, box_u.dtype) == (torch.float32, torch.int64, torch.float32, torch.float32)
    assert tuple(label_u.shape) == (Q,) and tuple(label_r.shape) == (Q,) and tuple(box_sign.shape) == tuple(box_u.shape) == (Q, 4)
    # the layout, row 5, from the two counter blocks
    words = [STAT_KEY & 0xFFFFFFFF, STAT_KEY >> 32]
    a, b = dn.philox4x32_10([5, 0, 0, 0], words), dn.philox4x32_10([5, 1, 0, 0], words)
    assert label_u[5].item() == (int(a[0]) >> 8) * 2.0 ** -24 and label_r[5].item() == (int(a[1]) * C) >> 32
    assert box_sign[5].tolist() == [float((int(a[2]) >> k) & 1) for k in range(4)]
    assert box_u[5].tolist() == [(int(v) >> 8) * 2.0 ** -24 for v in b]
    assert (label_u >= 0).all() and (label_u < 1).all() and (box_u >= 0).all() and (box_u < 1).all()
    assert (label_r >= 0).all() and (label_r < C).all() and set(label_r.tolist()) == set(range(C))
    share = (label_u < 0.25).double().mean().item()
    assert abs(share - 0.25) <= 5 * (0.25 * 0.75 / Q) ** 0.5, share
    for k in range(4):
        mean = box_sign[:, k].double().mean().item()
        assert abs(mean - 0.5) <= 5 * (0.25 / Q) ** 0.5, (k, mean)
    again = dn.cdn_noise(STAT_KEY, Q, C, "cpu")
    other = dn.cdn_noise(STAT_KEY + 1, Q, C, "cpu")
    assert all(torch.equal(x, y) for x, y in zip(again, (label_u, label_r, box_sign, box_u)))
    assert not torch.equal(other[0], label_u) and not torch.equal(other[3], box_u)


def test_gradient_reaches_the_embedding_only_through_its_rows(g11):
    settings, labels, boxes, noise, counts = fixture_case(g11, "a")
    module = module_for(g11, settings)
    label_query, box_query, _, groups, _ = module(labels, boxes, noise=noise)
    assert label_query.requires_grad and not box_query.requires_grad
    up = torch.randn(label_query.shape, generator=torch.Generator().manual_seed(3))
    (label_query * up).sum().backward()
    lab = T(slot_labels(counts, groups, g11["a.noised_labels"])).long()
    want = torch.zeros(C, D).index_add_(0, lab[lab >= 0], up[lab >= 0])
    assert torch.allclose(module.label_encoder.weight.grad, want, rtol=0, atol=1e-5)
    unused = sorted(set(range(C)) - set(lab[lab >= 0].tolist()))
    assert (module.label_encoder.weight.grad[unused] == 0).all()


def test_fused_pieces_have_no_cpu_kernel_path():
    embed, labels, boxes = torch.zeros(3, 8), torch.zeros(2, dtype=torch.int64), torch.rand(2, 4)
    with pytest.raises(_lib.RdetrError):
        dn.cdn_queries_forward(embed, labels, boxes, [2], 1, 0.5, 1.0, key=1)
    with pytest.raises(_lib.RdetrError):
        dn.cdn_embed_backward(torch.zeros(2, 8), torch.zeros(2, dtype=torch.int32), 3)
    with pytest.raises(_lib.RdetrError):
        dn.cdn_queries(embed, labels, boxes, [2], 1, fused=False)                # the torch route needs draws or a key
    with pytest.raises(_lib.RdetrError):
        dn.cdn_noise(-1, 4, 3, "cpu")


def test_checkpoint_key_is_the_reference_detectors():
    from relation_detr_amd import RelationCriterion, RelationDETRHead
    from relation_detr_amd.transformer import build_relation_transformer
    net = build_relation_transformer(num_classes=C, d_ffn=64, enc_layers=1, dec_layers=1, num_queries=NQ, hybrid_num_proposals=30)
    head = RelationDETRHead(net, RelationCriterion(C, fused=False), GenerateCDNQueries(NQ, C, 256, fused=False))
    keys = set(head.state_dict())
    assert "denoising_generator.label_encoder.weight" in keys and "transformer.tgt_embed.weight" in keys
    assert {k.split(".")[0] for k in keys} == {"transformer", "denoising_generator"}
    assert [n for n, _ in GenerateCDNQueries(NQ, C, 256).named_parameters()] == ["label_encoder.weight"]


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_once_bound_and_exported(name):
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert len(re.findall(r"^int " + name + r"\s*\(", header, re.M)) == 1
    assert name in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert callable(getattr(_lib.load(), name))


def test_abi_version_and_options_are_unchanged():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert "#define RDETR_ABI_VERSION 3" in header and _lib.load().rdetr_abi_version() == 3
    assert len(dataclasses.fields(options.Options)) == 25                   # `fused` is a constructor argument, not a routing switch


def test_argument_refusals():
    lib = _lib.load()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(8)

    def queries(fn=lib.rdetr_cdn_queries_f32, labels=one, boxes=one, B=2, G=3, max_gt=2, groups=1, C=5, d=8, prob=0.5, scale=1.0, embed=one,
                label=(one, one), box=(one, one), keyed=0, out=one, lab_out=one):
        return fn(labels, boxes, one, B, G, max_gt, groups, C, d, prob, scale, embed, label[0], label[1], box[0], box[1], keyed, 7, out, one,
                  lab_out, None)
    assert queries(G=0, max_gt=0, labels=None, boxes=None, embed=None, out=None) == 0         # zero work: no launch
    assert queries(labels=None) == -1 and queries(embed=None) == -1 and queries(out=None) == -1 and queries(lab_out=None) == -1
    assert queries(B=0) == -1 and queries(groups=0) == -1 and queries(C=0) == -1 and queries(max_gt=4) == -1
    assert queries(label=(None, one)) == -1 and queries(box=(one, None)) == -1              # draws missing while their noise is on
    assert queries(d=6) == -2 and queries(fn=lib.rdetr_cdn_queries_bf16, d=12) == -2
    assert queries(embed=odd) == -2 and queries(boxes=odd) == -2 and queries(out=odd) == -2 and queries(box=(odd, one)) == -2
    assert queries(labels=ctypes.c_void_p(4)) == -2 and queries(label=(one, ctypes.c_void_p(4))) == -2

    mask = lib.rdetr_cdn_mask
    assert mask(1, 0, 0, None, None) == 0
    assert mask(0, 2, 4, one, None) == -1 and mask(1, -1, 4, one, None) == -1 and mask(1, 2, 4, None, None) == -1
    assert mask(1, 2, 4, ctypes.c_void_p(6), None) == -2 and mask(1, 2, 50000, one, None) == -2

    def backward(fn=lib.rdetr_cdn_embed_backward_f32, grad=one, labels=one, rows=4, C=5, d=8, out=one):
        return fn(grad, labels, rows, C, d, out, None)
    assert backward(grad=None) == -1 and backward(labels=None) == -1 and backward(out=None) == -1 and backward(rows=-1) == -1
    assert backward(C=0) == -1
    assert backward(d=6) == -2 and backward(fn=lib.rdetr_cdn_embed_backward_bf16, d=12) == -2 and backward(out=odd) == -2

    noise = lib.rdetr_cdn_noise
    assert noise(7, 0, 5, None, None, None, None, None) == 0
    assert noise(7, 4, 5, None, one, one, one, None) == -1 and noise(7, 4, 0, one, one, one, one, None) == -1 and noise(7, -1, 5, one, one, one, one, None) == -1
    assert noise(7, 4, 5, one, ctypes.c_void_p(4), one, one, None) == -2 and noise(7, 4, 5, one, one, odd, one, None) == -2


def test_package_exports_and_shadow_tables_still_complete():
    for name in ("GenerateCDNQueries", "CdnQueryFunction", "cdn_queries", "cdn_noise", "denoising_mask"):
        assert name in relation_detr_amd.__all__ and getattr(relation_detr_amd, name) is getattr(dn, name)
    from relation_detr_amd import detector
    assert "RelationDETRHead" in relation_detr_amd.__all__ and relation_detr_amd.RelationDETRHead is detector.RelationDETRHead
    import test_shadow_complete as t
    t.test_every_ops_function_is_classified()
    t.test_every_rdetr_symbol_is_under_the_tripwire_or_excluded()
    t.test_every_training_module_function_is_classified()


# ------------------------------------------------------------------------------------------------------------------------ head
def tiny_head(device, fused, **kw):
    from relation_detr_amd import RelationCriterion, RelationDETRHead
    from relation_detr_amd.transformer import build_relation_transformer
    net = build_relation_transformer(num_classes=C, d_ffn=64, enc_layers=2, dec_layers=3, num_queries=NQ, hybrid_num_proposals=30, **kw)
    net.load_state_dict(synthetic_state_dict(net.state_dict()))
    generator = GenerateCDNQueries(num_queries=NQ, num_classes=C, label_embed_dim=256, denoising_nums=6, fused=fused)
    generator.load_state_dict(synthetic_state_dict(generator.state_dict()))
    return RelationDETRHead(net, RelationCriterion(C, fused=fused), generator).to(device)


def head_inputs(device):
    g, z = load_golden("g8_transformer_train.npz"), load_golden("g10_criterion.npz")
    pyramid = tuple([T(g[f"{k}{i}"]).to(device) for i in range(4)] for k in ("feat", "mask", "pos"))
    targets = [{"labels": T(z[f"tgt.labels.{b}"]).to(device), "boxes": T(z[f"tgt.boxes.{b}"]).to(device)} for b in range(2)]
    return pyramid, targets


EXPECTED_KEYS = {f"loss_{n}{s}" for n in ("class", "bbox", "giou")
                 for s in ("", "_0", "_1", "_enc", "_dn", "_dn_0", "_dn_1", "_hybrid", "_0_hybrid", "_1_hybrid", "_enc_hybrid")}


def test_head_equals_the_hand_composition_on_cpu():
    from oracle.cpu_modules import OracleMSDA, OracleRelation, OracleSelfAttention
    head = tiny_head("cpu", False, msda_cls=OracleMSDA, self_attn_cls=OracleSelfAttention, relation_cls=OracleRelation).train()
    (feats, masks, pos), targets = head_inputs("cpu")
    counts = [3, 2]
    groups = dn.denoising_groups(6, 3)
    assert groups == 2
    noise = dn.cdn_noise(11, 2 * groups * sum(counts), C, "cpu")
    losses = head(feats, masks, pos, targets, noise=noise)
    assert set(losses) == EXPECTED_KEYS and all(torch.isfinite(v) for v in losses.values())
    torch.stack(list(losses.values())).sum().backward()
    grad = head.denoising_generator.label_encoder.weight.grad
    assert grad is not None and torch.isfinite(grad).all() and grad.abs().max() > 0

    label_query, box_query, mask, got_groups, group_size = head.denoising_generator([t["labels"] for t in targets],
                                                                                   [t["boxes"] for t in targets], noise=noise)
    assert (got_groups, group_size) == (2, 6) and tuple(label_query.shape) == (2, 12, 256)
    outputs = head.transformer(feats, masks, pos, label_query, box_query, mask)
    by_hand = head.criterion(outputs, targets, dn_meta=(got_groups, group_size))
    assert set(by_hand) == set(losses)
    for k in losses:
        assert torch.equal(losses[k], by_hand[k]), k

    head.eval()
    with torch.no_grad():
        logits, boxes = head(feats, masks, pos)
        want = head.transformer(feats, masks, pos)
    assert tuple(logits.shape) == (2, NQ, C) and torch.equal(logits, want[0][-1]) and torch.equal(boxes, want[1][-1])


def test_head_without_any_box_has_no_denoising_part():
    from oracle.cpu_modules import OracleMSDA, OracleRelation, OracleSelfAttention
    head = tiny_head("cpu", False, msda_cls=OracleMSDA, self_attn_cls=OracleSelfAttention, relation_cls=OracleRelation).train()
    (feats, masks, pos), _ = head_inputs("cpu")
    targets = [{"labels": torch.zeros(0, dtype=torch.int64), "boxes": torch.zeros(0, 4)} for _ in range(2)]
    losses = head(feats, masks, pos, targets)
    assert set(losses) == {k for k in EXPECTED_KEYS if "_dn" not in k} and all(torch.isfinite(v) for v in losses.values())
    with pytest.raises(ValueError):
        head(feats, masks, pos)
